"""CPU: the scripted driver's C ABI (include/mcr.h: mcr_set_drivers / mcr_driver_actions and the handle-free mcr_check_drivers /
mcr_driver_defaults), the package's defaults against the header's, the keyword validation of VecMultiCarRacing — all without a device —
and the restatement's (tests/driver_ref.py) own edge cases."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import driver_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mcr_driver_defaults", "mcr_check_drivers", "mcr_set_drivers", "mcr_driver_actions")
ERR_ARG = -1


def _header():
    return open(os.path.join(ROOT, "include", "mcr.h")).read()


def test_driver_symbols_exported_and_declared(lib):
    L = lib.load()
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for n in NAMES:
        assert hasattr(L, n), f"{n} is not exported by libmcr_hip.so"
        assert re.search(r"\bint\s+%s\s*\(" % n, code), f"{n} is not declared in include/mcr.h"
        assert n in lib.SYMBOLS
    assert re.search(r"#define\s+MCR_DRV_PARAMS\s+10\b", code) and lib.DRV_PARAMS == 10 and D.PARAMS == 10
    # argument checks that need no device: a NULL handle
    rows = D.default_params(2)
    assert L.mcr_set_drivers(None, lib.ptr(rows), 0, None) == ERR_ARG
    assert L.mcr_driver_actions(None, None, 0, None, None) == ERR_ARG
    assert L.mcr_driver_defaults(None) == ERR_ARG


def test_defaults_equal_the_headers(lib):
    import multi_car_racing_amd as pkg
    from multi_car_racing_amd import drivers
    m = re.search(r"#define\s+MCR_DRV_DEFAULTS\s+\{([^}]*)\}", _header())
    header = [float(v.strip().rstrip("f")) for v in m.group(1).split(",")]
    assert len(header) == 10
    assert pkg.DRIVER_PARAM_NAMES == ("L1", "L2", "v_max", "K_s", "K_c", "K_g", "K_b", "offset", "gas_max", "brake_max")
    assert [pkg.DRIVER_DEFAULTS[k] for k in pkg.DRIVER_PARAM_NAMES] == header == [4, 12, 70, 8, 20, 0.2, 0.1, 0, 1, 0.8]
    out = np.zeros(10, np.float32)
    assert lib.load().mcr_driver_defaults(lib.ptr(out)) == 0
    assert np.array_equal(out, np.asarray(header, np.float32)) and np.array_equal(out, np.asarray(D.DEFAULTS, np.float32))
    assert np.array_equal(drivers.default_params(3), np.tile(out, (3, 1))) and np.array_equal(D.default_params(3), np.tile(out, (3, 1)))


BAD_FIELDS = [("L1", 0), ("L1", 65), ("L1", 2.5), ("L2", 0), ("L2", 65), ("L2", 7.25), ("v_max", 0), ("v_max", -1), ("K_s", -0.5), ("K_c", -1),
              ("K_g", -0.1), ("K_b", -0.1), ("gas_max", -0.1), ("gas_max", 1.5), ("brake_max", -0.1), ("brake_max", 1.01)]


def test_check_drivers_refuses_each_invalid_field(lib):
    """mcr_set_drivers' validation through its handle-free twin: every field out of range, every field non-finite, mask bits >= N, NULL rows"""
    L = lib.load()
    names = lib.DRIVER_PARAM_NAMES
    N = 3
    good = D.default_params(N)
    assert L.mcr_check_drivers(N, lib.ptr(good), 0b111) == 0 and L.mcr_check_drivers(N, lib.ptr(good), 0) == 0
    edge = good.copy(); edge[:, names.index("L1")] = [1, 64, 4]; edge[:, names.index("gas_max")] = [0, 1, 0.5]; edge[:, names.index("K_c")] = 0
    edge[:, names.index("offset")] = [-3, 3, 0]
    assert L.mcr_check_drivers(N, lib.ptr(edge), 0b101) == 0
    for name, v in BAD_FIELDS:
        for car in (0, N - 1):
            rows = good.copy(); rows[car, names.index(name)] = v
            assert L.mcr_check_drivers(N, lib.ptr(rows), 0) == ERR_ARG, f"{name} = {v} of car {car} was accepted"
            assert f"car {car}".encode() in L.mcr_last_error()
    for j, name in enumerate(names):
        for v in (np.nan, np.inf, -np.inf):
            rows = good.copy(); rows[1, j] = v
            assert L.mcr_check_drivers(N, lib.ptr(rows), 0) == ERR_ARG, f"{name} = {v} was accepted"
    assert L.mcr_check_drivers(N, lib.ptr(good), 0b1000) == ERR_ARG and L.mcr_check_drivers(N, lib.ptr(good), 0x80000000) == ERR_ARG
    assert L.mcr_check_drivers(N, None, 0) == ERR_ARG
    assert L.mcr_check_drivers(0, lib.ptr(good), 0) == ERR_ARG and L.mcr_check_drivers(9, lib.ptr(good), 0) == ERR_ARG
    bad = good.copy(); bad[N - 1, 0] = 0                     # only the first num_agents rows are looked at
    assert L.mcr_check_drivers(N - 1, lib.ptr(bad), 0) == 0


def test_set_drivers_with_a_handle(lib):
    """the same refusals through mcr_set_drivers itself, plus the NULL buffer and MCR_ERR_STATE of mcr_driver_actions — needs a device for the handle"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device: mcr_create needs one (the handle-free twin covers the validation)")
    L = lib.load()
    N = 2
    cfg = lib.Config(4, N, 0, 0, 0, 1, 0, 1, 0, 1, 0.25)
    h = ctypes.c_void_p()
    lib.check(L.mcr_create(ctypes.byref(cfg), ctypes.byref(h)), "mcr_create")
    buf = torch.zeros((4, N, 3), dtype=torch.float32, device="cuda")
    good = D.default_params(N)
    assert L.mcr_driver_actions(h, None, 0, None, None) == -3            # MCR_ERR_STATE: nothing set
    assert L.mcr_set_drivers(h, lib.ptr(good), 0b11, None) == ERR_ARG
    assert L.mcr_set_drivers(h, None, 0b11, ctypes.c_void_p(buf.data_ptr())) == ERR_ARG
    assert L.mcr_set_drivers(h, lib.ptr(good), 0b100, ctypes.c_void_p(buf.data_ptr())) == ERR_ARG
    for name, v in BAD_FIELDS:
        rows = good.copy(); rows[1, lib.DRIVER_PARAM_NAMES.index(name)] = v
        assert L.mcr_set_drivers(h, lib.ptr(rows), 0b11, ctypes.c_void_p(buf.data_ptr())) == ERR_ARG
    assert L.mcr_driver_actions(h, None, 0, None, None) == -3            # a refused call registers nothing
    assert L.mcr_set_drivers(h, lib.ptr(good), 0, ctypes.c_void_p(buf.data_ptr())) == 0        # mask 0 with a buffer: expert labels only
    assert L.mcr_set_drivers(h, lib.ptr(good), 0b10, ctypes.c_void_p(buf.data_ptr())) == 0     # ... and again, to change it
    L.mcr_destroy(h)


def test_keyword_validation_needs_no_device(lib):
    """ValueError before anything is created: on a box without a device the constructor would otherwise end in McrError"""
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    bad = [dict(scripted_agents=(2,)), dict(scripted_agents=(-1,)), dict(scripted_agents=(0, 0)), dict(scripted_agents=(0.5,)), dict(scripted_agents=1),
           dict(scripted_agents="01"), dict(driver_params={"speed": 1.0}), dict(driver_params={"L1": 0}), dict(driver_params={"L1": [4, 4, 4]}),
           dict(driver_params={"v_max": [70.0, 0.0]}), dict(driver_params={"K_c": float("nan")}), dict(driver_params=np.zeros((2, 9), np.float32)),
           dict(driver_params=np.zeros((3, 10), np.float32)), dict(driver_params=np.zeros((2, 10), np.float32)), dict(driver_params="fast"),
           dict(scripted_agents=(1,), driver_params={"brake_max": 2.0})]
    for kw in bad:
        with pytest.raises(ValueError):
            VecMultiCarRacing(4, 2, **kw)


def test_driver_params_forms(lib):
    from multi_car_racing_amd import drivers
    d = drivers.default_params(2)
    assert np.array_equal(drivers.driver_params_array(2, None), d) and np.array_equal(drivers.driver_params_array(2, {}), d)
    got = drivers.driver_params_array(2, {"v_max": 55, "offset": (-1.5, 1.5)})
    want = d.copy(); want[:, 2] = 55; want[:, 7] = (-1.5, 1.5)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert np.array_equal(drivers.driver_params_array(2, want.astype(np.float64).tolist()), want)
    assert drivers.driver_mask(3, None) == 0 and drivers.driver_mask(3, ()) == 0 and drivers.driver_mask(3, [2, 0]) == 0b101
    assert drivers.driver_mask(3, np.array([1])) == 0b010


def _car(prm, px=0.0, py=0.0, s=0.0, c=1.0, vx=0.0, vy=0.0, i=0, cw=False, track=None):
    """one car on a small closed track (default: 8 points on a circle of radius 10 around the origin would put p off the line; a straight line
    of points along +y, heading +y, is the simplest: f = (0, 1), r = (1, 0))"""
    if track is None:
        tx = np.zeros(100); ty = np.arange(100, dtype=np.float64); tc = np.ones(100); ts = np.zeros(100)      # beta = 0: C = 1, S = 0: "right" is +x
    else:
        tx, ty, tc, ts = track
    return D.car_action(px, py, s, c, vx, vy, i, tx, ty, tc, ts, cw, np.asarray(prm, np.float32))


def test_restatement_edge_cases():
    q = np.asarray(D.DEFAULTS, np.float32)
    # on the line, at rest, heading along it: no steering, full gas, no brake
    a = _car(q)
    assert a.dtype == np.float32 and a.tolist() == [0.0, 1.0, 0.0]
    # at v_f = v_max on a straight: e = 0 — neither gas nor brake
    assert _car(q, vy=70.0).tolist() == [0.0, 0.0, 0.0]
    # faster than v*: brake K_b e, clamped to brake_max
    assert _car(q, vy=72.0).tolist() == [0.0, 0.0, np.float32(0.1 * 2.0)]
    assert _car(q, vy=100.0).tolist() == [0.0, 0.0, np.float32(0.8)]
    # the target to the right (the car sits left of the line): positive steer; a positive offset moves the line to the right for CCW, to the left for CW
    assert _car(q, px=-1.0)[0] > 0 and _car(q, px=1.0)[0] < 0
    off = q.copy(); off[D.OFFSET] = 2.0
    assert _car(off)[0] > 0 and _car(off, cw=True, i=50, s=0.0, c=-1.0, py=50.0)[0] > 0     # CW: the car heads -y, its right is -x, the line moves to -x
    # the curvature: target (x, y) = (4, 3) in the car's frame -> kappa = 2 * 3 / 25, steer = clamp(8 * 0.24) = 1
    assert _car(q, px=-3.0)[0] == 1.0
    k = q.copy(); k[D.K_S] = 1.0
    assert _car(k, px=-3.0)[0] == np.float32(2.0 * 3.0 / (4.0 * 4.0 + 3.0 * 3.0))
    # the car ON its target: denominator 0 -> kappa = 0, not a division by zero
    one = q.copy(); one[D.L1] = 1; one[D.L2] = 1
    assert _car(one, py=1.0).tolist() == [0.0, 1.0, 0.0]
    # K_c = 0: the target speed ignores the curvature
    kc0 = q.copy(); kc0[D.K_C] = 0.0
    assert _car(kc0, px=-3.0, vy=69.0)[1] == np.float32(0.2 * 1.0)
    # a non-finite state yields zeros, component by component
    assert _car(q, px=float("nan")).tolist() == [0.0, 0.0, 0.0]
    assert _car(q, vy=float("inf")).tolist() == [0.0, 0.0, 0.0]
    assert _car(q, vy=float("nan"), px=-3.0).tolist() == [1.0, 0.0, 0.0]
    # the index wraps in both directions
    assert _car(q, i=98, py=98.0)[1] == 1.0 and _car(q, i=1, py=1.0, cw=True, c=-1.0)[1] == 1.0
