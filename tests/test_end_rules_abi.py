"""CPU: the C ABI of early episode ending (include/mcr.h: mcr_set_end_rules, mcr_check_end_rules, mcr_end_rules_now) and VecMultiCarRacing's
keyword checks.  Every check here comes before the handle is touched or before anything is created: no device is needed."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mcr_set_end_rules", "mcr_check_end_rules", "mcr_end_rules_now")
MCR_OK, MCR_ERR_ARG = 0, -1


def test_symbols_declared_exported_and_bound(lib):
    L = lib.load()
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcr.h")).read(), flags=re.S)
    for n in NAMES:
        assert hasattr(L, n), f"{n} is not exported by libmcr_hip.so"
        assert re.search(r"\bint\s+%s\s*\(" % n, code), f"{n} is not declared in include/mcr.h"
        assert n in lib.SYMBOLS and getattr(L, n).argtypes == lib.SYMBOLS[n][1]
    assert len(lib.SYMBOLS["mcr_set_end_rules"][1]) == 9 and lib.SYMBOLS["mcr_set_end_rules"][1][5] is ctypes.c_double
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "mcr_set_end_rules" in integration and "mcr_end_rules_now" in integration


def test_argument_checks_without_a_device(lib):
    L = lib.load()
    buf = np.zeros(64, np.int32)
    p = ctypes.c_void_p(buf.ctypes.data - buf.ctypes.data % 16 + 16)      # 16-byte aligned, inside the array
    bufs = (p, p, p)

    def refused(*args, what):
        assert L.mcr_set_end_rules(*args) == MCR_ERR_ARG, what
        assert what.encode() in L.mcr_last_error(), (what, L.mcr_last_error())

    # some but not all buffers: refused whatever the handle
    for some in ((p, None, None), (None, p, None), (None, None, p), (p, p, None), (p, None, p), (None, p, p)):
        refused(None, 5, 0, 0, 1, 0.0, *some, what="together or not at all")
    refused(None, -1, 0, 0, 1, 0.0, *bufs, what="must be >= 0")
    refused(None, 3, -2, 0, 1, 0.0, *bufs, what="must be >= 0")
    refused(None, 0, 0, 0, 1, 0.0, *bufs, what="both patiences are 0")
    refused(None, 5, 0, 2, 1, 0.0, *bufs, what="offroad_mode")
    refused(None, 5, 0, -1, 1, 0.0, *bufs, what="offroad_mode")
    for bad in (math.nan, math.inf, -math.inf):
        refused(None, 5, 0, 0, 1, bad, *bufs, what="not finite")
    refused(None, 5, 0, 0, 1, 0.0, ctypes.c_void_p(p.value + 4), p, p, what="16-byte aligned")
    # everything in order but the handle — and the off call, which has nothing else to check
    refused(None, 5, 4, 1, 1, -1.5, *bufs, what="null handle")
    refused(None, 0, 0, 0, 0, 0.0, None, None, None, what="null handle")
    assert L.mcr_end_rules_now(None, None) == MCR_ERR_ARG
    # the value checks for a given num_agents, the agent mask among them
    assert L.mcr_check_end_rules(2, 5, 0, 0, 0b01, 0.0) == MCR_OK and L.mcr_check_end_rules(8, 0, 7, 1, 0x80, -3.0) == MCR_OK
    assert L.mcr_check_end_rules(2, 5, 0, 0, 0b111, 0.0) == MCR_OK          # (bits of cars >= num_agents are ignored)
    for args, what in (((2, 5, 0, 0, 0, 0.0), "names no car"), ((2, 5, 0, 0, 0b100, 0.0), "names no car"), ((1, 5, 0, 0, 0b10, 0.0), "names no car"),
                       ((0, 5, 0, 0, 1, 0.0), "num_agents"), ((9, 5, 0, 0, 1, 0.0), "num_agents"), ((2, -1, 0, 0, 1, 0.0), "must be >= 0"),
                       ((2, 0, 0, 0, 1, 0.0), "both patiences"), ((2, 1, 1, 3, 1, 0.0), "offroad_mode"), ((2, 1, 1, 0, 1, math.nan), "not finite")):
        assert L.mcr_check_end_rules(*args) == MCR_ERR_ARG and what.encode() in L.mcr_last_error(), (args, L.mcr_last_error())


@pytest.mark.parametrize("kw", [dict(end_patience=-1), dict(end_patience=2 ** 31), dict(end_patience=2.5), dict(end_patience=True), dict(end_offroad=-3),
                                dict(end_offroad="4"), dict(end_patience=5, end_offroad_mode="some"), dict(end_offroad_mode=None),
                                dict(end_patience=5, end_agents=()), dict(end_patience=5, end_agents=(2,)), dict(end_patience=5, end_agents=(-1,)),
                                dict(end_patience=5, end_agents=(0.5,)), dict(end_patience=5, end_agents=3), dict(end_patience=5, end_reward=float("nan")),
                                dict(end_patience=5, end_reward=float("inf")), dict(end_reward="much"), dict(end_agents=(7,))])
def test_keyword_validation_comes_before_anything_is_created(lib, kw):
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    with pytest.raises(ValueError, match="end_"):
        VecMultiCarRacing(4, 2, **kw)


def test_keyword_defaults_are_off():
    from multi_car_racing_amd.vec_env import end_rules_config
    assert end_rules_config(2, 0, 0, "all", None, 0.0) is None and end_rules_config(2, 0, 0, "any", (1,), -5.0) is None
    assert end_rules_config(3, 100, 0, "all", None, 0.0) == (100, 0, "all", (0, 1, 2), 0.0)
    assert end_rules_config(3, np.int64(0), 50, "any", [2, 0, 2], -1) == (0, 50, "any", (0, 2), -1.0)
