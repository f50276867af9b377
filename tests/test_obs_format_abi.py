"""CPU: the observation-format entry points (include/mcr.h: mcr_set_obs_format, mcr_obs_bytes_per_view, mcr_obs_window) are declared,
exported, bound, and refuse a NULL handle without a GPU."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mcr_set_obs_format", "mcr_obs_bytes_per_view", "mcr_obs_window")


def test_header_declares_obs_format_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcr.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(r"\b" + n + r"\s*\(", src), f"include/mcr.h does not declare {n}"
    for m in ("MCR_OBS_RGB 0", "MCR_OBS_GRAY 1", "MCR_OBS_STACK_MAX 8"):
        assert "#define " + m in src


def test_library_exports_and_binds_them(lib):
    L = lib.load()
    for n in NEW:
        assert hasattr(L, n) and n in lib.SYMBOLS
    assert (lib.OBS_RGB, lib.OBS_GRAY, lib.OBS_STACK_MAX) == (0, 1, 8)


def test_null_handle(lib):
    L = lib.load()
    MCR_ERR_ARG = -1
    assert L.mcr_set_obs_format(None, lib.OBS_GRAY, 4) == MCR_ERR_ARG
    assert L.mcr_set_obs_format(None, lib.OBS_RGB, 1) == MCR_ERR_ARG
    assert L.mcr_obs_bytes_per_view(None) == 0
    assert L.mcr_obs_window(None) == MCR_ERR_ARG
    assert L.mcr_obs_bytes_per_view.restype is ctypes.c_size_t
