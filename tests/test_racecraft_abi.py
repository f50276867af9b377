"""CPU: racecraft's C ABI (include/mcr.h: mcr_set_racecraft and the handle-free mcr_check_racecraft / mcr_racecraft_defaults), the package's
defaults against the header's and the restatement's (tests/racecraft_ref.py), and the validation of VecMultiCarRacing(racecraft=...) —
all without a device."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import driver_ref as D
from tests import racecraft_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mcr_racecraft_defaults", "mcr_check_racecraft", "mcr_set_racecraft")
ERR_ARG, ERR_STATE = -1, -3


def _header():
    return open(os.path.join(ROOT, "include", "mcr.h")).read()


def test_racecraft_symbols_exported_and_declared(lib):
    L = lib.load()
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for n in NAMES:
        assert hasattr(L, n), f"{n} is not exported by libmcr_hip.so"
        assert re.search(r"\bint\s+%s\s*\(" % n, code), f"{n} is not declared in include/mcr.h"
        assert n in lib.SYMBOLS
    assert re.search(r"#define\s+MCR_RC_PARAMS\s+8\b", code) and lib.RC_PARAMS == 8 and R.PARAMS == 8
    assert re.search(r"#define\s+MCR_DRV_PARAMS\s+10\b", code), "the driver's row must stay what it was"
    assert L.mcr_set_racecraft(None, lib.ptr(R.default_params(2)), 0b11) == ERR_ARG
    assert L.mcr_racecraft_defaults(None) == ERR_ARG


def test_defaults_agree(lib):
    import multi_car_racing_amd as pkg
    from multi_car_racing_amd import drivers
    m = re.search(r"#define\s+MCR_RC_DEFAULTS\s+\{([^}]*)\}", _header())
    header = [float(v.strip().rstrip("f")) for v in m.group(1).split(",")]
    assert len(header) == 8
    assert pkg.RACECRAFT_PARAM_NAMES == R.NAMES == ("look", "w_block", "w_pass", "off_max", "d_safe", "K_f", "w_off", "v_off")
    assert [pkg.RACECRAFT_DEFAULTS[k] for k in pkg.RACECRAFT_PARAM_NAMES] == header == list(R.DEFAULTS)
    out = np.zeros(8, np.float32)
    assert lib.load().mcr_racecraft_defaults(lib.ptr(out)) == 0
    assert np.array_equal(out, np.asarray(header, np.float32))
    assert np.array_equal(drivers.default_racecraft_params(3), np.tile(out, (3, 1))) and np.array_equal(R.default_params(3), np.tile(out, (3, 1)))
    # the follow rule must release once the car is beside its leader: the side-step goes further than the blocking width
    assert R.DEFAULTS[R.W_PASS] > R.DEFAULTS[R.W_BLOCK] and R.DEFAULTS[R.OFF_MAX] >= R.DEFAULTS[R.W_PASS]


BAD_FIELDS = [("look", 0), ("look", 65), ("look", 2.5), ("look", -1), ("w_block", -0.5), ("w_pass", -1), ("off_max", -0.1), ("d_safe", -3),
              ("K_f", -0.1), ("w_off", -1), ("v_off", -0.5)]


def test_check_racecraft_refuses_each_invalid_field(lib):
    L = lib.load()
    names = lib.RACECRAFT_PARAM_NAMES
    N = 3
    good = R.default_params(N)
    assert L.mcr_check_racecraft(N, lib.ptr(good), 0b111) == 0 and L.mcr_check_racecraft(N, lib.ptr(good), 0) == 0
    edge = good.copy(); edge[:, 0] = [1, 64, 24]; edge[:, 1:] = 0
    assert L.mcr_check_racecraft(N, lib.ptr(edge), 0b101) == 0
    for name, v in BAD_FIELDS:
        for car in (0, N - 1):
            rows = good.copy(); rows[car, names.index(name)] = v
            assert L.mcr_check_racecraft(N, lib.ptr(rows), 0) == ERR_ARG, f"{name} = {v} of car {car} was accepted"
            assert f"car {car}".encode() in L.mcr_last_error()
    for j, name in enumerate(names):
        for v in (np.nan, np.inf, -np.inf):
            rows = good.copy(); rows[1, j] = v
            assert L.mcr_check_racecraft(N, lib.ptr(rows), 0) == ERR_ARG, f"{name} = {v} was accepted"
    assert L.mcr_check_racecraft(N, lib.ptr(good), 0b1000) == ERR_ARG and L.mcr_check_racecraft(N, lib.ptr(good), 0x80000000) == ERR_ARG
    assert L.mcr_check_racecraft(N, None, 0) == ERR_ARG
    assert L.mcr_check_racecraft(0, lib.ptr(good), 0) == ERR_ARG and L.mcr_check_racecraft(9, lib.ptr(good), 0) == ERR_ARG
    bad = good.copy(); bad[N - 1, 0] = 0                     # only the first num_agents rows are looked at
    assert L.mcr_check_racecraft(N - 1, lib.ptr(bad), 0) == 0


def test_set_racecraft_with_a_handle(lib):
    """MCR_ERR_STATE before mcr_set_drivers, the refusals through the handle, on / off / on again — needs a device for the handle"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device: mcr_create needs one (the handle-free twin covers the validation)")
    L = lib.load()
    N = 2
    cfg = lib.Config(4, N, 0, 0, 0, 1, 0, 1, 0, 1, 0.25)
    h = ctypes.c_void_p()
    lib.check(L.mcr_create(ctypes.byref(cfg), ctypes.byref(h)), "mcr_create")
    buf = torch.zeros((4, N, 3), dtype=torch.float32, device="cuda")
    good = R.default_params(N)
    assert L.mcr_set_racecraft(h, lib.ptr(good), 0b11) == ERR_STATE
    assert L.mcr_set_racecraft(h, None, 0) == ERR_STATE
    assert L.mcr_set_drivers(h, lib.ptr(D.default_params(N)), 0b11, ctypes.c_void_p(buf.data_ptr())) == 0
    assert L.mcr_set_racecraft(h, lib.ptr(good), 0b100) == ERR_ARG
    for name, v in BAD_FIELDS:
        rows = good.copy(); rows[1, lib.RACECRAFT_PARAM_NAMES.index(name)] = v
        assert L.mcr_set_racecraft(h, lib.ptr(rows), 0b11) == ERR_ARG
    assert L.mcr_set_racecraft(h, lib.ptr(good), 0b10) == 0
    assert L.mcr_set_racecraft(h, None, 0b10) == 0 and L.mcr_set_racecraft(h, lib.ptr(good), 0) == 0      # off, both ways
    assert L.mcr_set_racecraft(h, lib.ptr(good), 0b11) == 0
    L.mcr_destroy(h)


def test_keyword_validation_needs_no_device(lib):
    """ValueError before anything is created"""
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    s = dict(scripted_agents=(0, 1))
    bad = [dict(racecraft=True), dict(racecraft={}), dict(racecraft=R.default_params(2)),                       # nothing to apply it to
           dict(s, racecraft={"speed": 1.0}), dict(s, racecraft={"look": 0}), dict(s, racecraft={"look": 2.5}), dict(s, racecraft={"look": [8, 8, 8]}),
           dict(s, racecraft={"w_block": -1.0}), dict(s, racecraft={"K_f": float("nan")}), dict(s, racecraft={"v_off": [15.0, -1.0]}),
           dict(s, racecraft={"agents": (2,)}), dict(s, racecraft={"agents": (0, 0)}), dict(s, racecraft={"agents": 1}), dict(s, racecraft={"agents": (0.5,)}),
           dict(s, racecraft=np.zeros((2, 7), np.float32)), dict(s, racecraft=np.zeros((3, 8), np.float32)), dict(s, racecraft=np.zeros((2, 8), np.float32)),
           dict(s, racecraft="fast"), dict(s, racecraft=1.5)]
    for kw in bad:
        with pytest.raises(ValueError):
            VecMultiCarRacing(4, 2, **kw)


def test_racecraft_params_forms(lib):
    from multi_car_racing_amd import drivers
    d = drivers.default_racecraft_params(2)
    assert drivers.racecraft_params_array(2, None) == (None, 0) and drivers.racecraft_params_array(2, False, 0b11) == (None, 0)
    rows, mask = drivers.racecraft_params_array(2, True, 0b10)
    assert np.array_equal(rows, d) and mask == 0b10
    rows, mask = drivers.racecraft_params_array(2, True, 0)           # labels only: every car
    assert np.array_equal(rows, d) and mask == 0b11
    rows, mask = drivers.racecraft_params_array(2, {}, 0b01)
    assert np.array_equal(rows, d) and mask == 0b01
    rows, mask = drivers.racecraft_params_array(2, {"look": 32, "d_safe": (10.0, 20.0), "agents": [1]}, 0b11)
    want = d.copy(); want[:, 0] = 32; want[:, 4] = (10.0, 20.0)
    assert rows.dtype == np.float32 and np.array_equal(rows, want) and mask == 0b10
    rows, mask = drivers.racecraft_params_array(2, want.astype(np.float64).tolist(), 0b11)
    assert np.array_equal(rows, want) and mask == 0b11
    assert drivers.racecraft_params_array(3, {"agents": ()}, 0b111)[1] == 0


def _flat(N=100):
    """a straight line of points along +y (beta = 0: "right" is +x), as tests/test_driver_abi.py's"""
    return np.zeros(N), np.arange(N, dtype=np.float64), np.ones(N), np.zeros(N)


def _cars(*cars):
    """(px, py, vy) per car, heading +y"""
    return [dict(px=float(px), py=float(py), s=0.0, c=1.0, vx=0.0, vy=float(vy), i=int(round(py)), lat=float(px), counts=bool(np.isfinite([px, py, vy]).all()))
            for px, py, vy in cars]


def test_restatement_edge_cases():
    q = np.asarray(D.DEFAULTS, np.float32); w = np.asarray(R.DEFAULTS, np.float32)
    tr = _flat()

    def act(cars, a=0, cw=False, rc=w):
        rep = {}
        return R.car_action(cars, a, tr, cw, q, rc, rep), rep
    plain = D.car_action(0.0, 10.0, 0.0, 1.0, 0.0, 30.0, 10, *tr, False, q)
    # alone, or with the other car behind: the plain controller's action
    a, rep = act(_cars((0, 10, 30)))
    assert np.array_equal(a, plain) and rep["leader"] is None
    a, rep = act(_cars((0, 10, 30), (0, 5, 10)))
    assert np.array_equal(a, plain) and rep["leader"] is None
    # a slow car 8 ahead on the line: the car on the line itself goes right (lat_a < lat_l is false), the cap is max(0, 10 + 2 (8 - 16)) = 0
    a, rep = act(_cars((0, 10, 30), (0, 18, 10)))
    assert rep["leader"] == 1 and rep["step_right"] and rep["follow"] and rep["follow_zero"] and a[0] > 0 and a[1] == 0 and a[2] == np.float32(0.8)
    # from the left it goes left
    a, rep = act(_cars((-0.5, 10, 30), (0, 18, 10)))
    assert rep["step_left"] and not rep["step_flipped"] and a[0] < 0
    # a leader beside the line (|lat_l - o| >= w_block): no side-step, and |y| >= w_block: no cap
    a, rep = act(_cars((0, 10, 30), (3.5, 18, 10)))
    assert rep["leader"] == 1 and not (rep["step_left"] or rep["step_right"] or rep["follow"]) and np.array_equal(a, plain)
    # the nearer of two is the leader; equal x: the lowest index
    assert act(_cars((0, 10, 30), (0, 25, 10), (1, 18, 10)))[1]["leader"] == 2
    assert act(_cars((0, 10, 30), (1, 18, 10), (-1, 18, 10)))[1]["leader"] == 1
    # beyond `look` tiles: not a candidate
    assert act(_cars((0, 10, 30), (0, 35, 10)))[1]["leader"] is None and act(_cars((0, 10, 30), (0, 34, 10)))[1]["leader"] == 1
    # off the road: the cap v_off
    a, rep = act(_cars((8.0, 10, 30)))
    assert rep["off_road"] and a[1] == 0 and a[2] > 0
    assert not act(_cars((7.5, 10, 30)))[1]["off_road"]
    # a car that does not count is nobody's leader; a car that does not count itself gets the plain controller's zeros
    a, rep = act(_cars((0, 10, 30), (float("nan"), 18, 10)))
    assert rep["leader"] is None and rep["ignored"] == 1 and np.array_equal(a, plain)
    a, rep = act(_cars((float("nan"), 10, 30), (0, 18, 10)))
    assert rep["self_nonfinite"] and a.tolist() == [0.0, 0.0, 0.0]
