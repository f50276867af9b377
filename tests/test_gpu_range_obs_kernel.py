"""MI355X: k_rangeobs (csrc/k_rangeobs.h) on the synthetic tracks and poses of tests/obs_cases.py, through the kernel's own launch
(mcr_set_range_obs / mcr_range_obs_now) — bit for bit against tests/range_obs_ref.py on get_state() arrays, tests/util.py's hull_positions
and the track rows.  No rollouts, no oracle.

What the oracle rollouts of tests/test_gpu_range_obs.py (N <= 3, T ~ 300) cannot reach and this file does: hull-edge slots 2 and 3 (cars
4-7), the slot skip with N > 3 and the self-skip for cars >= 3; a lane that holds two passing segments in one ray (tiles i and i + 64 k, a
tile's left and right segment), the nearest of them parked first; q exactly 0 and 1 on a border vertex and on a hull corner, den == 0, t = 0,
directions that are no unit vectors (0.5, 3, 1e-20, zero); culling with every tile far and with a short range beside the 200-unit wrap
segment of a truncated track; tile runs beyond 384; NaN and inf cars beside finite ones.  tests/test_obs_cases.py asserts on the host, from
the restatement alone, that these situations occur in the poses."""
import ctypes

import numpy as np
import pytest

from tests import obs_cases as C
from tests import range_obs_ref
from tests.util import assert_f32_bits

pytestmark = pytest.mark.gpu


def _fan(rays):
    return range_obs_ref.default_dirs(rays)[1]


def _full(rays):
    ang = np.linspace(-np.pi, np.pi, rays, endpoint=False)
    return np.ascontiguousarray(np.stack([np.cos(ang), np.sin(ang)], axis=1).astype(np.float32))


# direction tables set through mcr_set_range_obs directly: the axes (at hull angle 0 the rays (0, 1), (1, 0), (-1, 0)), lengths 0.5 and 3, an
# all-zero direction and one of length 1e-20; SHORT holds nothing longer than 0.5 (max_range * max|dir| is the cull radius)
AXES = np.array([(1, 0), (0, 1), (0, -1), (0.5, 0), (0, 3), (0, 0), (1e-20, 0), (-1.5, 2.598076)], np.float32)
SHORT = np.array([(0.5, 0), (0, 0.5), (1e-20, 0), (0, -0.5), (-0.3, 0.4)], np.float32)
CONFIGS = {
    "fan19_25": (_fan(19), 25.0), "fan19_400": (_fan(19), 400.0), "full32_400": (_full(32), 400.0), "fan1_2000": (_fan(1), 2000.0),
    "full19_0.5": (_full(19), 0.5), "fan32_25": (_fan(32), 25.0), "full32_2000": (_full(32), 2000.0),
    "axes_25": (AXES, 25.0), "axes_400": (AXES, 400.0), "short_25": (SHORT, 25.0), "short_2000": (SHORT, 2000.0), "axes_0.5": (AXES, 0.5),
}
# the pose sets a configuration runs on (every set under the default fan, a full circle and the axes)
EVERY = ("scatter", "scatter2", "centre", "ties", "border", "far", "nonfinite", "close", "graze", "start")
SETS = {"fan19_25": EVERY, "fan19_400": EVERY, "full32_400": EVERY, "axes_25": EVERY, "axes_400": ("scatter", "border", "graze", "close", "nonfinite"),
        "fan1_2000": ("scatter", "far", "centre"), "full19_0.5": ("scatter", "border", "close", "graze"), "fan32_25": ("scatter2", "close", "start"),
        "full32_2000": ("scatter2", "far", "nonfinite"), "short_25": ("scatter", "close", "border"), "short_2000": ("scatter2", "far", "centre"),
        "axes_0.5": ("scatter", "border", "graze", "close")}


@pytest.fixture(scope="module", params=[1, 2, 4, 5, 7, 8], ids=lambda n: f"N{n}")
def rig(request, lib):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    r = C.Rig(lib, C.all_tracks(lib), request.param, "range")
    r.sets = C.pose_sets(r.L, r.tracks, r.N, r.base["bodies"])
    yield r
    r.close()


def _launch(rig, dirs, max_range):
    """the kernel's tensor [B, N, 2, R] for the handle's current state, written into a guarded buffer"""
    dirs = np.ascontiguousarray(dirs, np.float32); R = len(dirs)
    whole, view = rig.guarded(rig.B * rig.N * 2 * R)
    st = rig.torch.cuda.current_stream(rig.env.device)
    assert rig.L.mcr_set_range_obs(rig.env.h, ctypes.c_void_p(view.data_ptr()), rig.lib.ptr(dirs), R, ctypes.c_float(max_range)) == 0
    assert rig.L.mcr_range_obs_now(rig.env.h, ctypes.c_void_p(st.cuda_stream)) == 0
    st.synchronize()
    assert rig.guards_intact(whole), "the words around the tensor were written"
    return view.cpu().numpy().reshape(rig.B, rig.N, 2, R)


@pytest.mark.parametrize("config", list(CONFIGS))
def test_ranges_equal_the_restatement(rig, config):
    dirs, max_range = CONFIGS[config]
    for name in SETS[config]:
        bodies = rig.sets[name]
        st = rig.set_bodies(bodies)
        got = _launch(rig, dirs, max_range)
        want = C.range_ref(rig.L, rig.tracks, st["bodies"], dirs, max_range)
        assert_f32_bits(got, want, f"N {rig.N} {config}, poses {name}")
        if rig.N == 1:
            assert (got[:, :, 1] == np.float32(max_range)).all(), "one car: channel 1 is max_range"
        if name == "far":
            assert (got == np.float32(max_range)).all(), "5e3 and more away: nothing within range"


def test_ranges_do_not_depend_on_the_batch(lib):
    """env e's rows inside B = 10 and alone (B = 1, env_offset = e: the same level of the cycle)"""
    N = 5
    dirs, max_range = _full(32), 400.0
    tracks = C.all_tracks(lib)[14:24]
    big = C.Rig(lib, tracks, N, "range")
    try:
        sets = C.pose_sets(big.L, tracks, N, big.base["bodies"])
        rows = {}
        for name in ("scatter", "close", "border"):
            big.set_bodies(sets[name])
            rows[name] = _launch(big, dirs, max_range)
        for e in (0, 6, 9):
            one = C.Rig(lib, tracks[e:e + 1], N, "range", env_offset=e, every=tracks)
            try:
                for name in rows:
                    one.set_bodies(sets[name][e:e + 1])
                    assert_f32_bits(_launch(one, dirs, max_range), rows[name][e:e + 1], f"env {e} alone, poses {name}")
            finally:
                one.close()
    finally:
        big.close()
