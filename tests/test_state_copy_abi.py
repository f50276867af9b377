"""CPU: the C ABI of the batched device-side snapshots (include/mcr.h: mcr_state_blob_pitch, mcr_save_states, mcr_load_states,
mcr_copy_states) — exported, declared, bound, and refusing a NULL handle before any HIP call.  tests/test_abi.py checks that the header
and _lib.SYMBOLS agree on the whole symbol set."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MCR_ERR_ARG = -1
NAMES = ("mcr_state_blob_pitch", "mcr_state_blob_header", "mcr_save_states", "mcr_load_states", "mcr_copy_states")


def test_state_copy_symbols_exported_and_declared(lib):
    L = lib.load()
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcr.h")).read(), flags=re.S)
    for n in NAMES:
        assert hasattr(L, n), f"{n} is not exported by libmcr_hip.so"
        assert re.search(r"\b%s\s*\(" % n, code), f"{n} is not declared in include/mcr.h"
        assert n in lib.SYMBOLS


def test_null_handle_is_an_argument_error(lib):
    L = lib.load()
    assert L.mcr_state_blob_pitch(None) == 0
    assert L.mcr_state_blob_header(None, None) == MCR_ERR_ARG
    assert L.mcr_save_states(None, None, 1, None, None) == MCR_ERR_ARG
    assert L.mcr_load_states(None, None, 1, None, None, None) == MCR_ERR_ARG
    assert L.mcr_copy_states(None, None, None, 1, None) == MCR_ERR_ARG
    assert L.mcr_last_error()


def test_the_kernel_is_in_the_gfx950_code_object():
    so = os.path.join(ROOT, "multi_car_racing_amd", "_lib", "libmcr_hip.so")
    assert b"k_envcopy" in open(so, "rb").read()
