"""MI355X: k_stateobs (csrc/k_stateobs.h) and the search it shares with k_driver (csrc/k_nearest.h) on the synthetic tracks and poses of
tests/obs_cases.py, through the kernel's own launch (mcr_set_state_obs / mcr_state_obs_now) — bit for bit against tests/state_obs_ref.py
on get_state() arrays, tests/util.py's hull_positions and the track rows.  No rollouts, no oracle.

What the oracle rollouts of tests/test_gpu_state_obs.py (N <= 3, T ~ 300) cannot reach and this file does: F > 64 (the feature loop's
second trip: F = 66 and 78) and F = 64 exactly; other-car indices up to 7; strides up to 64 with 16 waypoints (a CW wrap of many laps on a
20-tile track); tracks of 20 .. 512 tiles on either side of every multiple of 64 (tile registers 6 and 7; none at all in most lanes); exact
f64 ties between lanes and inside one; poses from which every tile lies inside the search's f32 band; poses 1e5 away; NaN and inf cars."""
import ctypes
import math

import numpy as np
import pytest

from tests import obs_cases as C
from tests import state_obs_ref
from tests.util import assert_f32_bits, hull_positions, make_env

pytestmark = pytest.mark.gpu

CONFIGS = [(0, 1), (6, 5), (9, 7), (10, 64), (16, 64)]          # (waypoints, stride)


@pytest.fixture(scope="module", params=[1, 2, 4, 5, 8], ids=lambda n: f"N{n}")
def rig(request, lib):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    r = C.Rig(lib, C.all_tracks(lib), request.param, "state", steps=C.WARMUP_STEPS, spread=True)
    r.sets = C.pose_sets(r.L, r.tracks, r.N, r.base["bodies"])
    yield r
    r.close()


def _launch(rig, K, stride):
    """the kernel's rows [B, N, F] for the handle's current state, written into a guarded buffer"""
    F = state_obs_ref.dim(rig.N, K)
    assert rig.lib.state_obs_dim(rig.N, K) == F
    whole, view = rig.guarded(rig.B * rig.N * F)
    st = rig.torch.cuda.current_stream(rig.env.device)
    assert rig.L.mcr_set_state_obs(rig.env.h, ctypes.c_void_p(view.data_ptr()), K, stride) == 0
    assert rig.L.mcr_state_obs_now(rig.env.h, ctypes.c_void_p(st.cuda_stream)) == 0
    st.synchronize()
    assert rig.guards_intact(whole), "the words around the tensor were written"
    return view.cpu().numpy().reshape(rig.B, rig.N, F)


def test_feature_counts():
    assert state_obs_ref.dim(8, 9) == 64 and state_obs_ref.dim(5, 16) == 66 and state_obs_ref.dim(8, 10) == 66 and state_obs_ref.dim(8, 16) == 78


def test_the_cars_of_an_env_differ(rig):
    """host assertions on get_state(): the steps behind the rig's reset left every car of an env with wheel speeds and a steering angle of
    its own, and in EVERY env the cars' on-road bits are not all the same (obs_cases.spread_bodies puts the even cars on the road and the odd
    ones beside it; tests/test_obs_cases.py shows the same on the oracle).  A kernel that read another car's words would show.  With N = 1
    there is no other car: nothing to differ from."""
    st = rig.base
    assert np.isfinite(st["bodies"]).all() and np.isfinite(st["wheels"]).all()
    assert (np.abs(st["wheels"][:, :, :, 4]).max(axis=2) > 0).all(), "a car whose wheels never turned"
    if rig.N == 1:
        return
    steer = st["bodies"][:, :, 1, 2].astype(np.float64) - st["bodies"][:, :, 0, 2].astype(np.float64)
    for e in range(rig.B):
        assert len(set(steer[e].tolist())) == rig.N, f"env {e}: steering angles {steer[e].tolist()}"
        assert len(set(map(tuple, st["wheels"][e, :, :, 4].tolist()))) == rig.N, f"env {e}: wheel speeds"
        nibbles = set(map(tuple, (st["on_road"][e] != 0).tolist()))
        assert len(nibbles) >= 2, f"env {e} ({rig.tracks[e][0]}): every car's on-road bits are {nibbles}"


def test_hull_positions_is_what_the_device_hands_out(rig):
    for name, bodies in rig.sets.items():
        rig.set_bodies(bodies)
        assert_f32_bits(rig.env.positions(), hull_positions(rig.L, bodies), f"positions, poses {name}")


@pytest.mark.parametrize("K,stride", CONFIGS, ids=[f"K{k}s{s}" for k, s in CONFIGS])
def test_rows_equal_the_restatement(rig, K, stride):
    for name, bodies in rig.sets.items():
        st = rig.set_bodies(bodies)
        got = _launch(rig, K, stride)
        want = C.state_ref(rig.L, rig.tracks, st, rig.tvc, K, stride)
        assert_f32_bits(got, want, f"N {rig.N} K {K} stride {stride}, poses {name}")
        if name == "nonfinite":
            pos = hull_positions(rig.L, bodies)
            for e in range(rig.B):
                a = int(np.nonzero(np.isnan(pos[e]).any(axis=1))[0][0])
                assert np.isnan(got[e, a, 13]) and got[e, a, 17] == (-1.0 if rig.tracks[e][2] else 1.0), "the NaN car's row: defined, nearest tile 0"


def test_lattice_ties_pick_the_lowest_index(rig):
    """features 13, 14 of a car on a tie name the tile the search chose: the offset from the LOWEST tied tile (host: tests/test_obs_cases.py)"""
    bodies = rig.sets["ties"]
    rig.set_bodies(bodies)
    got = _launch(rig, 0, 1)
    pos = hull_positions(rig.L, bodies)
    for e, (name, rows, cw) in enumerate(rig.tracks):
        if name != "lattice":
            continue
        for a in range(rig.N):
            x, y, tied = C.LATTICE_TIES[(a + e) % len(C.LATTICE_TIES)]
            assert pos[e, a].tolist() == [x, y]
            i = min(tied)
            dx, dy = x - rows[i, 2], y - rows[i, 3]
            c, s = math.cos(rows[i, 1]), math.sin(rows[i, 1])           # (the slot holds libm's)
            assert got[e, a, 13] == np.float32(dx * c + dy * s) and got[e, a, 14] == np.float32(-dx * s + dy * c), f"env {e} car {a}: tiles {tied}"


def test_a_never_reset_env_is_a_zero_row_also_alone(lib):
    import torch
    for N, K in ((1, 6), (8, 16)):
        env = make_env(1, N, 3, obs=False, streams=1, state_obs=True, state_waypoints=K)
        try:
            env.state.fill_(7.0)
            got = env.refresh_state()
            torch.cuda.synchronize()
            assert got.shape == (1, N, state_obs_ref.dim(N, K)) and (got == 0).all().item()
        finally:
            env.close()


def test_rows_do_not_depend_on_the_batch(lib):
    """env e's rows inside B = 10 and alone (B = 1, env_offset = e: the same level of the cycle)"""
    N, K, stride = 4, 16, 7
    tracks = C.all_tracks(lib)[8:18]
    big = C.Rig(lib, tracks, N, "state")
    try:
        sets = C.pose_sets(big.L, tracks, N, big.base["bodies"])
        rows = {}
        for name in ("scatter", "centre", "close"):
            big.set_bodies(sets[name])
            rows[name] = _launch(big, K, stride)
        for e in (0, 3, 9):
            one = C.Rig(lib, tracks[e:e + 1], N, "state", env_offset=e, every=tracks)
            try:
                for name in rows:
                    one.set_bodies(sets[name][e:e + 1])
                    assert_f32_bits(_launch(one, K, stride), rows[name][e:e + 1], f"env {e} alone, poses {name}")
            finally:
                one.close()
    finally:
        big.close()
