"""CPU: the range-finder observation's C ABI (include/mcr.h: mcr_set_range_obs / mcr_range_obs_now / mcr_check_range_obs), the keyword
validation of VecMultiCarRacing(range_obs=True) — which raises before any device is touched — and the hull polygons of the numpy
restatement (tests/range_obs_ref.py) against the ones the kernels hold."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests import range_obs_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mcr_set_range_obs", "mcr_range_obs_now", "mcr_check_range_obs", "mcr_hull_polygons")


def test_range_obs_symbols_exported_and_declared(lib):
    L = lib.load()
    src = open(os.path.join(ROOT, "include", "mcr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for n in NAMES:
        assert hasattr(L, n), f"{n} is not exported by libmcr_hip.so"
        assert re.search(r"\bint\s+%s\s*\(" % n, code), f"{n} is not declared in include/mcr.h"
        assert n in lib.SYMBOLS
    m = re.search(r"#define\s+MCR_RANGE_RAYS_MAX\s+(\d+)", code)
    assert m and int(m.group(1)) == lib.RANGE_RAYS_MAX == 32
    # argument checks that need no device: a NULL handle
    dirs = np.array([[1.0, 0.0]], np.float32)
    assert L.mcr_set_range_obs(None, None, lib.ptr(dirs), 1, ctypes.c_float(100.0)) == -1
    assert L.mcr_set_range_obs(None, None, None, 0, ctypes.c_float(0.0)) == -1
    assert L.mcr_range_obs_now(None, None) == -1


def test_check_range_obs_validates_table_count_and_range(lib):
    """mcr_set_range_obs' validation, reached without a handle through mcr_check_range_obs"""
    L = lib.load()
    _, d19 = R.default_dirs(19)
    d19 = np.ascontiguousarray(d19)
    ok = lambda d, n, r: L.mcr_check_range_obs(None if d is None else lib.ptr(d), n, ctypes.c_float(r))
    assert ok(d19, 19, 100.0) == 0 and ok(d19, 1, 1e-3) == 0
    d32 = np.ascontiguousarray(R.default_dirs(32, 2 * math.pi)[1])
    assert ok(d32, 32, 400.0) == 0
    assert ok(d32, 0, 100.0) == -1 and ok(d32, 33, 100.0) == -1 and ok(d32, -1, 100.0) == -1      # rays outside 1..32
    assert ok(None, 19, 100.0) == -1                                                             # NULL dirs
    for bad in (float("nan"), float("inf"), -float("inf")):
        for pos in ((0, 0), (18, 1)):
            d = d19.copy(); d[pos] = bad
            assert ok(d, 19, 100.0) == -1
        assert ok(d19, 19, bad) == -1                                                            # max_range not finite
    d = d19.copy(); d[18, 1] = float("nan")
    assert ok(d, 18, 100.0) == 0                                                                 # (only the first `rays` rows are read)
    assert ok(d19, 19, 0.0) == -1 and ok(d19, 19, -1.0) == -1                                    # max_range <= 0


def test_keyword_validation_raises_before_any_device(lib, monkeypatch):
    """bad range_* keywords are ValueErrors on a box with no GPU: nothing may be created first (a missing device is an McrError)"""
    import torch
    from multi_car_racing_amd import vec_env
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    bad = (dict(range_rays=0), dict(range_rays=33), dict(range_rays=2.5), dict(range_rays=True),
           dict(range_fov=float("nan")), dict(range_fov=float("inf")),
           dict(range_angles=[]), dict(range_angles=[0.0] * 33), dict(range_angles=[0.0, float("nan")]), dict(range_angles=[0.0, float("inf")]),
           dict(range_angles=[[0.0, 1.0]]),
           dict(range_max=0.0), dict(range_max=-5.0), dict(range_max=float("nan")), dict(range_max=float("inf")), dict(range_max=1e39))
    for kw in bad:
        with pytest.raises(ValueError):
            vec_env.VecMultiCarRacing(2, 2, range_obs=True, **kw)
    # a good set gets as far as the device check; without range_obs=True the other keywords are not looked at
    for kw in (dict(range_obs=True), dict(range_obs=True, range_angles=[-0.5, 0.0, 0.5], range_max=30.0), dict(range_obs=False, range_rays=0)):
        with pytest.raises(lib.McrError):
            vec_env.VecMultiCarRacing(2, 2, **kw)


def test_ray_table(lib):
    from multi_car_racing_amd.vec_env import range_obs_table
    ang, dirs, rmax = range_obs_table()
    assert ang.dtype == np.float64 and dirs.dtype == np.float32 and dirs.shape == (19, 2) and rmax == 100.0
    assert np.array_equal(ang, np.linspace(-math.pi / 2, math.pi / 2, 19)) and ang[9] == 0.0
    assert np.array_equal(dirs, np.stack([np.cos(ang), np.sin(ang)], 1).astype(np.float32))
    assert np.array_equal(dirs, R.default_dirs()[1])
    assert dirs[9].tolist() == [1.0, 0.0] and dirs[18, 1] == 1.0 and dirs[0, 1] == -1.0      # centre ray ahead, last ray to the right
    ang1, dirs1, _ = range_obs_table(range_rays=1, range_fov=2.0)
    assert ang1.tolist() == [0.0] and dirs1.tolist() == [[1.0, 0.0]]                         # a single ray points straight ahead
    ang3, dirs3, _ = range_obs_table(range_rays=7, range_angles=(0.0, 1.0, 3.0))             # explicit angles override rays / fov
    assert ang3.tolist() == [0.0, 1.0, 3.0] and dirs3.shape == (3, 2)


def test_restated_hull_polygons_are_the_kernels(lib):
    """channel 1 is defined on McrShapes::hull in its stored vertex order; the restatement builds the polygons from gym's HULL_POLY1..4 x SIZE"""
    L = lib.load()
    out = np.zeros((4, 8, 2), np.float32); counts = np.zeros(4, np.int32)
    assert L.mcr_hull_polygons(lib.ptr(out), lib.ptr(counts)) == 0
    assert L.mcr_hull_polygons(None, lib.ptr(counts)) == -1
    polys = R.hull_polygons()
    assert counts.tolist() == [len(p) for p in polys] == [4, 4, 8, 4]
    for k, p in enumerate(polys):
        assert np.array_equal(out[k, :len(p)], p), f"hull polygon {k}: {out[k, :len(p)].tolist()} vs the restatement's {p.tolist()}"
