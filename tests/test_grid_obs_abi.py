"""CPU: the grid observation's C ABI (include/mcr.h: mcr_set_grid_obs / mcr_grid_obs_now / mcr_check_grid_obs) and the keyword validation of
VecMultiCarRacing(grid_obs=True) — which raises before any device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mcr_set_grid_obs", "mcr_grid_obs_now", "mcr_check_grid_obs")
cf = ctypes.c_float


def test_grid_obs_symbols_exported_declared_and_bound(lib):
    L = lib.load()
    src = open(os.path.join(ROOT, "include", "mcr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for n in NAMES:
        assert hasattr(L, n), f"{n} is not exported by libmcr_hip.so"
        assert re.search(r"\bint\s+%s\s*\(" % n, code), f"{n} is not declared in include/mcr.h"
        assert n in lib.SYMBOLS
    m = re.search(r"#define\s+MCR_GRID_MAX\s+(\d+)", code)
    assert m and int(m.group(1)) == lib.GRID_MAX == 64
    for name, bit in (("ROAD", 1), ("FRESH", 2), ("TAKEN", 4), ("CAR", 8)):
        m = re.search(r"#define\s+MCR_GRID_%s\s+(\d+)" % name, code)
        assert m and int(m.group(1)) == getattr(lib, "GRID_" + name) == bit
    import multi_car_racing_amd as pkg
    assert (pkg.GRID_ROAD, pkg.GRID_FRESH, pkg.GRID_TAKEN, pkg.GRID_CAR) == (1, 2, 4, 8)
    # argument checks that need no device: a NULL handle comes first
    assert L.mcr_set_grid_obs(None, None, 32, 32, cf(1.5), cf(24.0), cf(16.0)) == -1
    assert L.mcr_set_grid_obs(None, None, 0, 0, cf(0.0), cf(0.0), cf(0.0)) == -1
    assert L.mcr_grid_obs_now(None, None) == -1


def test_check_grid_obs_accepts_and_refuses_exactly_the_documented_ranges(lib):
    L = lib.load()
    ok = lambda r, c, cell=1.5, orow=24.0, ocol=16.0: L.mcr_check_grid_obs(r, c, cf(cell), cf(orow), cf(ocol))
    for r, c in ((1, 1), (64, 64), (1, 64), (64, 1), (32, 32), (7, 64), (33, 17)):
        assert ok(r, c) == 0
    for r, c in ((0, 32), (32, 0), (65, 32), (32, 65), (-1, 32), (32, -1), (0, 0), (1 << 20, 1)):
        assert ok(r, c) == -1
    tiny = float(np.nextafter(np.float32(0), np.float32(1)))
    big = float(np.finfo(np.float32).max)
    for cell in (tiny, 1e-20, 0.25, 6.0, big):
        assert ok(32, 32, cell) == 0
    for cell in (0.0, -0.0, -1.5, float("nan"), float("inf"), -float("inf")):
        assert ok(32, 32, cell) == -1
    for o in (0.0, -100.0, 1e6, 0.3, big, -big):
        assert ok(32, 32, 1.5, o, 16.0) == 0 and ok(32, 32, 1.5, 24.0, o) == 0      # fractional, outside the grid: fine
    for o in (float("nan"), float("inf"), -float("inf")):
        assert ok(32, 32, 1.5, o, 16.0) == -1 and ok(32, 32, 1.5, 24.0, o) == -1


def test_keyword_validation_raises_before_any_device(lib, monkeypatch):
    """bad grid_* keywords are ValueErrors on a box with no GPU: nothing may be created first (a missing device is an McrError)"""
    import torch
    from multi_car_racing_amd import vec_env
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    bad = (dict(grid_shape=(0, 32)), dict(grid_shape=(32, 65)), dict(grid_shape=(32,)), dict(grid_shape=32), dict(grid_shape=(32.0, 32)),
           dict(grid_shape=(True, 32)), dict(grid_shape=(32, 32, 2)),
           dict(grid_cell=0.0), dict(grid_cell=-1.0), dict(grid_cell=float("nan")), dict(grid_cell=float("inf")), dict(grid_cell=1e39),
           dict(grid_cell=1e-50), dict(grid_cell="wide"),
           dict(grid_origin=(float("nan"), 0.0)), dict(grid_origin=(0.0, float("inf"))), dict(grid_origin=(1e39, 0.0)), dict(grid_origin=5.0),
           dict(grid_origin=(1.0, 2.0, 3.0)))
    for kw in bad:
        with pytest.raises(ValueError):
            vec_env.VecMultiCarRacing(2, 2, grid_obs=True, **kw)
    # a good set gets as far as the device check; without grid_obs=True the other keywords are not looked at
    for kw in (dict(grid_obs=True), dict(grid_obs=True, grid_shape=(7, 64), grid_cell=0.25, grid_origin=(-3.5, 100.0)), dict(grid_obs=False, grid_shape=(0, 0))):
        with pytest.raises(lib.McrError):
            vec_env.VecMultiCarRacing(2, 2, **kw)


def test_grid_geometry_defaults(lib):
    from multi_car_racing_amd.vec_env import grid_obs_geometry
    assert grid_obs_geometry() == (32, 32, 1.5, 24.0, 16.0)                      # the car a quarter from the bottom, in the middle
    assert grid_obs_geometry((7, 64), 0.25) == (7, 64, 0.25, 5.25, 32.0)
    H, W, cell, orow, ocol = grid_obs_geometry((33, 17), 0.1, (20.3, -8.7))
    assert (H, W) == (33, 17) and cell == float(np.float32(0.1)) and (orow, ocol) == (float(np.float32(20.3)), float(np.float32(-8.7)))
    assert L_check(lib, H, W, cell, orow, ocol) == 0


def L_check(lib, H, W, cell, orow, ocol):
    return lib.load().mcr_check_grid_obs(H, W, cf(cell), cf(orow), cf(ocol))
