"""CPU: the action-repeat entry of the C ABI — declared in include/mcr.h, exported by the built library, bound by _lib with its argument types."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    src = open(os.path.join(ROOT, "include", "mcr.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_the_entry_and_its_bound():
    src = _header()
    m = re.search(r"\bint\s+mcr_step_repeat\s*\(([^)]*)\)\s*;", src)
    assert m, "include/mcr.h does not declare mcr_step_repeat"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["mcr_env* h", "const float* d_actions", "int repeat", "uint8_t* d_obs", "double* d_reward", "uint8_t* d_done",
                      "uint8_t* d_trunc", "void* stream"], params
    d = re.search(r"^#define\s+MCR_REPEAT_MAX\s+(\d+)\s*$", src, flags=re.M)
    assert d and int(d.group(1)) == 16
    assert re.search(r"\bint\s+mcr_step\s*\(", src), "mcr_step stays declared"


def test_library_exports_and_lib_binds_it(lib):
    L = lib.load()
    assert hasattr(L, "mcr_step_repeat"), "libmcr_hip.so does not export mcr_step_repeat"
    res, args = lib.SYMBOLS["mcr_step_repeat"]
    vp = ctypes.c_void_p
    assert res is ctypes.c_int and args == [vp, vp, ctypes.c_int, vp, vp, vp, vp, vp]
    assert L.mcr_step_repeat.restype is ctypes.c_int and list(L.mcr_step_repeat.argtypes) == args
    assert lib.REPEAT_MAX == 16
    # the same arguments as mcr_step with `repeat` in third place
    assert args[:2] + args[3:] == lib.SYMBOLS["mcr_step"][1]


def test_bad_arguments_come_back_as_codes_without_a_gpu(lib):
    L = lib.load()
    assert L.mcr_step_repeat(None, None, 4, None, None, None, None, None) == -1          # MCR_ERR_ARG: no handle
    assert b"null" in L.mcr_last_error()


def test_kernel_parameter_table_names_the_two_fields():
    src = open(os.path.join(ROOT, "multi_car_racing_amd", "csrc", "mcr_kernels.h")).read()
    assert re.search(r"int32_t\s+defer_respawn\s*;", src) and re.search(r"int32_t\s+accumulate\s*;", src)
    common = open(os.path.join(ROOT, "multi_car_racing_amd", "csrc", "mcr_common.h")).read()
    assert re.search(r"#define\s+MCR_PARKED\s+2\b", common)
    # McrEnvState keeps its 48 bytes: parked is a VALUE of `frozen`, not a member
    body = re.search(r"struct McrEnvState \{(.*?)\};", common, flags=re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    members = re.findall(r"\b(double|int32_t|uint32_t)\s+(\w+)\s*;", body)
    assert sum(8 if t == "double" else 4 for t, _ in members) == 48 and [n for _, n in members][-3:] == ["frozen", "touch_blocks", "bp_step"]
