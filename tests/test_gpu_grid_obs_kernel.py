"""MI355X: k_gridobs (csrc/k_gridobs.h) on the synthetic tracks, poses and visit bits of tests/grid_cases.py, through the kernel's own
launch (mcr_set_grid_obs / mcr_grid_obs_now) — byte for byte against tests/grid_obs_ref.py on get_state() arrays, tests/util.py's
hull_positions and the track rows.  No rollouts, no oracle.

What the oracle rollouts of tests/test_gpu_grid_obs.py (N <= 3, T ~ 300, 32 x 32) cannot reach and this file does: cars 4-7; grids of one
cell, of 64 x 64, of odd H * W at every byte misalignment of the buffer; cell centres exactly on a polygon's edge and one float32 beside it
(the float32 prefilter's band); a view under 300 polygons and one whose box meets all 768 entries; views that meet nothing; NaN and inf
cars beside finite ones; visit bits of cars that do not exist and the recolour bit.  tests/test_grid_cases.py asserts on the host, from
the restatement alone, that these situations occur in the inputs."""
import ctypes

import numpy as np
import pytest

from tests import grid_cases as GC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[1, 2, 5, 8], ids=lambda n: f"N{n}")
def rig(request, lib):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    N = request.param
    r = GC.GridRig(lib, GC.tracks_for(lib, N), N)
    r.sets = GC.pose_sets(r.L, r.tracks, N, r.base["bodies"])
    r.flags = GC.flag_sets(r.tracks, N)
    yield r
    r.close()


def _assert_grids(got, want, tracks, what):
    for e, w in want.items():
        if not np.array_equal(got[e], w):
            bad = np.argwhere(got[e] != w)
            a, i, j = (int(v) for v in bad[0])
            raise AssertionError(f"{what}: env {e} ({tracks[e][0]}): {len(bad)} of {w.size} cells differ, first at car {a} cell ({i}, {j}): got {got[e][a, i, j]} want {w[a, i, j]}")


@pytest.fixture(scope="module", params=[1, 2], ids=lambda n: f"N{n}")
def big_rig(request, lib):
    """64 x 64 grids: on the tracks that need them and N <= 2 (the restatement is the slow side)"""
    N = request.param
    r = GC.GridRig(lib, [t for t in GC.tracks_for(lib, N) if t[0] in GC.BIG_TRACKS], N)
    r.sets = GC.pose_sets(r.L, r.tracks, N, r.base["bodies"])
    r.flags = GC.flag_sets(r.tracks, N)
    yield r
    r.close()


_ids = lambda c: "-".join(str(v) for v in c)


@pytest.mark.parametrize("case", [c for c in GC.CASES if c[0] != "big"], ids=_ids)
def test_grid_equals_the_restatement(rig, case):
    _compare_case(rig, case)


@pytest.mark.parametrize("case", [c for c in GC.CASES if c[0] == "big"], ids=_ids)
def test_big_grid_equals_the_restatement(big_rig, case):
    _compare_case(big_rig, case)


def _compare_case(rig, case):
    config, poses, bits, offset = case
    st = rig.set_bodies(rig.sets[poses])
    rig.env.set_env_state(tile_flags=rig.flags[bits])
    got = rig.launch(config, offset)
    want = GC.reference(rig.L, rig.tracks, st["bodies"], rig.flags[bits], config)
    _assert_grids(got, want, rig.tracks, f"N {rig.N} {config}, poses {poses}, bits {bits}, offset {offset}")
    assert not (got & 0xf0).any(), "bits 4..7 are 0"
    if rig.N == 1:
        assert not (got & (GC.G.GRID_TAKEN | GC.G.GRID_CAR)).any(), "one car: bits 2 and 3 are never set"
    if poses == "far":
        assert not got.any(), "5e3 and more away: nothing under the grid"
    if bits == "high":                                          # bits of cars that do not exist and the recolour bit change nothing
        rig.env.set_env_state(tile_flags=rig.flags["clear"])
        assert np.array_equal(rig.launch(config, offset), got), "visit bits >= N or bit 8 changed the grid"


def test_grid_does_not_depend_on_the_batch(lib):
    """env e's views inside the batch and alone (B = 1, env_offset = e: the same level of the cycle), at another misalignment"""
    N = 5
    tracks = GC.tracks_for(lib, N)
    big = GC.GridRig(lib, tracks, N)
    try:
        sets = GC.pose_sets(big.L, tracks, N, big.base["bodies"])
        flags = GC.flag_sets(tracks, N)["random"]
        big.env.set_env_state(tile_flags=flags)
        rows = {}
        for name in ("scatter", "close", "overlap"):
            big.set_bodies(sets[name])
            rows[name] = big.launch("odd", 1)
        for e in (0, 5, len(tracks) - 1):
            one = GC.GridRig(lib, tracks[e:e + 1], N, env_offset=e, every=tracks)
            try:
                one.env.set_env_state(tile_flags=flags[e:e + 1])
                for name in rows:
                    one.set_bodies(sets[name][e:e + 1])
                    assert np.array_equal(one.launch("odd", 2), rows[name][e:e + 1]), f"env {e} alone, poses {name}"
            finally:
                one.close()
    finally:
        big.close()


def test_never_reset_handle_gives_zeros_and_null_turns_it_off(lib):
    import torch
    from tests.util import make_env
    L = lib.load()
    env = make_env(3, 2, 0, obs=False, streams=1)
    try:
        assert L.mcr_grid_obs_now(env.h, None) == -3             # MCR_ERR_STATE: no buffer set
        buf = torch.full((3 * 2 * 33 * 17 + 64,), 0x5A, dtype=torch.uint8, device=env.device)
        view = buf[31:31 + 3 * 2 * 33 * 17]
        st = torch.cuda.current_stream(env.device)
        assert L.mcr_set_grid_obs(env.h, ctypes.c_void_p(view.data_ptr()), 33, 17, ctypes.c_float(1.5), ctypes.c_float(20.3), ctypes.c_float(8.7)) == 0
        assert L.mcr_grid_obs_now(env.h, ctypes.c_void_p(st.cuda_stream)) == 0
        st.synchronize()
        h = buf.cpu().numpy()
        assert not h[31:31 + view.numel()].any(), "rows of envs that were never reset must be zeros"
        assert (h[:31] == 0x5A).all() and (h[31 + view.numel():] == 0x5A).all()
        assert L.mcr_set_grid_obs(env.h, ctypes.c_void_p(view.data_ptr()), 65, 17, ctypes.c_float(1.5), ctypes.c_float(0.0), ctypes.c_float(0.0)) == -1
        assert L.mcr_set_grid_obs(env.h, None, 0, 0, ctypes.c_float(0.0), ctypes.c_float(0.0), ctypes.c_float(0.0)) == 0      # NULL: off, the rest is ignored
        assert L.mcr_grid_obs_now(env.h, None) == -3
        buf.fill_(0x5A)
        env.reset(); torch.cuda.synchronize()
        assert bool((buf == 0x5A).all()), "off: a reset writes nothing"
    finally:
        env.close()
