"""CPU: the state-vector observation's C ABI (include/mcr.h: mcr_state_obs_dim / mcr_set_state_obs / mcr_state_obs_now) and the sanity of
its numpy restatement (tests/state_obs_ref.py) on oracle episodes — which pins d, the index direction the cars are spawned facing."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests import state_obs_ref as R
from tests.util import oracle_episode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mcr_state_obs_dim", "mcr_set_state_obs", "mcr_state_obs_now")


def test_state_obs_dim_values(lib):
    L = lib.load()
    for N in (1, 2, 8):
        for K in (0, 6):
            want = 18 + 2 * K + 4 * (N - 1)
            assert L.mcr_state_obs_dim(N, K) == want and lib.state_obs_dim(N, K) == want and R.dim(N, K) == want
    assert lib.state_obs_dim(2) == 18 + 12 + 4                 # the default: 6 waypoints
    for N, K in ((0, 6), (9, 6), (2, -1), (2, 17)):
        assert L.mcr_state_obs_dim(N, K) == -1                 # MCR_ERR_ARG


def test_state_obs_symbols_exported_and_declared(lib):
    L = lib.load()
    src = open(os.path.join(ROOT, "include", "mcr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for n in NAMES:
        assert hasattr(L, n), f"{n} is not exported by libmcr_hip.so"
        assert re.search(r"\bint\s+%s\s*\(" % n, code), f"{n} is not declared in include/mcr.h"
        assert n in lib.SYMBOLS
    # argument checks that need no device
    assert L.mcr_set_state_obs(None, None, 6, 5) == -1 and L.mcr_state_obs_now(None, None) == -1


def test_slot_holds_libm_cos_sin_of_beta(lib):
    """the restatement takes (C, S) from math.cos / math.sin of the oracle's beta: the episode slot must hold the same doubles"""
    L = lib.load()
    N, seed = 2, 31
    mt_t = np.zeros(lib.MT_WORDS, np.uint32); L.mcr_mt_seed(lib.ptr(mt_t), ctypes.c_uint32(seed))
    blob = np.zeros(lib.episode_bytes(), np.uint8); info = np.zeros(12, np.int32)
    order = np.arange(N, dtype=np.int32)
    assert L.mcr_episode_generate(lib.ptr(mt_t), N, 0, lib.ptr(order), lib.ptr(blob), lib.ptr(info)) == 0
    ep = lib.unpack_episode(blob)
    T = ep["T"]
    off_c = 256 + 8 * lib.TILE_CAP * 4                          # mcr_common.h: MCR_OFF_TRACK_C, then MCR_OFF_TRACK_S
    C = blob[off_c:off_c + 8 * T].view(np.float64); S = blob[off_c + 8 * lib.TILE_CAP:off_c + 8 * lib.TILE_CAP + 8 * T].view(np.float64)
    beta = ep["track"][:, 2]
    assert np.array_equal(C, np.array([math.cos(b) for b in beta])) and np.array_equal(S, np.array([math.sin(b) for b in beta]))


@pytest.mark.parametrize("direction", ["CW", "CCW"])
@pytest.mark.parametrize("N", [1, 2, 3, 4])
def test_restatement_sanity_after_reset(lib, oracle, N, direction):
    """After reset() every car looks down the track: its first waypoint lies AHEAD (positive .f component — this pins d = +1 for CCW, -1 for
    CW), the nearest track point is within a tile's size (features 13, 14), and the heading agrees with the track's (feature 15 > 0)."""
    L = lib.load()
    tile = 2 * 40 / 6.0            # a tile's width across the road, 2 * TRACK_WIDTH = 13.3 (its length, TRACK_DETAIL_STEP = 3.5, is smaller)
    for seed in (3, 4, 5):
        ep = oracle_episode(oracle, N, seed, 0, direction=direction)
        assert ep["direction"] == direction
        o = oracle.OracleEnv(N)
        o.reset(ep, render=False)
        f = R.of_oracle(L, o, ep)
        assert f.shape == (N, R.dim(N)) and f.dtype == np.float32 and np.isfinite(f).all()
        for a in range(N):
            assert f[a, 18] > 0, f"seed {seed} car {a}: the first waypoint is behind the car ({f[a, 18]})"
            assert abs(f[a, 13]) < tile and abs(f[a, 14]) < tile, f"seed {seed} car {a}: offset from the nearest track point {f[a, 13:15]}"
            assert f[a, 15] > 0, f"seed {seed} car {a}: heading against the track's: cos {f[a, 15]}"
            assert f[a, 17] == (-1.0 if direction == "CW" else 1.0)
            assert f[a, 12] >= 0 and set(f[a, 8:12].tolist()) <= {0.0, 1.0}
        if N > 1:                   # the other-car block is antisymmetric in position up to the two frames: distances agree
            d01 = math.hypot(f[0, 30], f[0, 31]); d10 = math.hypot(f[1, 30], f[1, 31])
            assert abs(d01 - d10) < 1e-3 and d01 > 1.0
        o.close()
