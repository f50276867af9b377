"""MI355X: k_driver (csrc/k_driver.h) on the synthetic tracks and poses of tests/obs_cases.py, through the kernel's own launch
(mcr_set_drivers / mcr_driver_actions) — bit for bit against tests/driver_ref.py on get_state() arrays, tests/util.py's hull_positions and
the track rows.  No rollouts, no oracle.

What the oracle rollouts of tests/test_gpu_driver.py (N <= 3, T ~ 300) cannot reach and this file does: N = 4 and 8; look-aheads of 64
across the wrap in both directions on tracks of 20, 64, 65 and 512 tiles (several laps on the smallest); masks with high bits; `in` null,
given and equal to `out`; a NaN car."""
import ctypes

import numpy as np
import pytest

from tests import driver_ref
from tests import obs_cases as C
from tests.util import assert_f32_bits, hull_positions

pytestmark = pytest.mark.gpu

MASKS = {1: (0x01, 0x00), 4: (0x01, 0x08, 0x05, 0x0f), 8: (0x01, 0x80, 0xa5, 0xff)}
SETS = ("start", "scatter", "centre", "far", "nonfinite", "close")


def params(N):
    """a row of its own per car: car 0 the defaults, then L1 and L2 from {1, 4, 64} and offsets +-3"""
    p = driver_ref.default_params(N)
    for a in range(1, N):
        p[a, driver_ref.L1] = (1, 4, 64)[a % 3]; p[a, driver_ref.L2] = (64, 1, 4)[(a // 2) % 3]
        p[a, driver_ref.OFFSET] = (3.0, -3.0, 0.0)[a % 3]
        p[a, driver_ref.V_MAX] = 20.0 + 9.0 * a; p[a, driver_ref.K_S] = 0.5 * a; p[a, driver_ref.GAS_MAX] = 1.0 - 0.1 * a
    return np.ascontiguousarray(p, np.float32)


@pytest.fixture(scope="module", params=[1, 4, 8], ids=lambda n: f"N{n}")
def rig(request, lib):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    r = C.Rig(lib, C.driver_tracks(lib), request.param, "driver")
    r.sets = C.pose_sets(r.L, r.tracks, r.N, r.base["bodies"])
    r.params = params(r.N)
    r.want = {}                      # pose set -> the restatement's actions for every car (computed once)
    yield r
    r.close()


def _want(rig, name):
    if name not in rig.want:
        rig.want[name] = C.driver_ref_actions(rig.L, rig.tracks, rig.sets[name], rig.params)
    return rig.want[name]


def _launch(rig, mask, mode, rng):
    """(out [B, N, 3], `in` as the kernel saw it or None) — mode: "null", "given" or "inplace" """
    n = rig.B * rig.N * 3
    whole, view = rig.guarded(n)
    fill = rng.uniform(-1, 1, n).astype(np.float32); fill[::7] = -0.0
    src = None
    if mode == "given":
        src = rig.torch.from_numpy(fill).to(rig.env.device)
    elif mode == "inplace":
        view.copy_(rig.torch.from_numpy(fill).to(rig.env.device)); src = view
    if rig.scratch is None:          # the buffer mcr_set_drivers registers with the handle: it lives as long as the rig
        rig.scratch = rig.torch.zeros(n, dtype=rig.torch.float32, device=rig.env.device)
    scratch = rig.scratch
    assert rig.L.mcr_set_drivers(rig.env.h, rig.lib.ptr(rig.params), ctypes.c_uint32(mask), ctypes.c_void_p(scratch.data_ptr())) == 0
    st = rig.torch.cuda.current_stream(rig.env.device)
    assert rig.L.mcr_driver_actions(rig.env.h, None if src is None else ctypes.c_void_p(src.data_ptr()), ctypes.c_uint32(0),
                                    ctypes.c_void_p(view.data_ptr()), ctypes.c_void_p(st.cuda_stream)) == 0
    st.synchronize()
    assert rig.guards_intact(whole), "the words around the tensor were written"
    assert (scratch == 0).all().item(), "the handle's own action buffer was written though `out` was given"
    return view.cpu().numpy().reshape(rig.B, rig.N, 3), (None if mode == "null" else fill.reshape(rig.B, rig.N, 3))


def test_parameter_rows_are_valid_and_distinct(rig):
    assert rig.L.mcr_check_drivers(rig.N, rig.lib.ptr(rig.params), ctypes.c_uint32((1 << rig.N) - 1)) == 0
    assert len(set(map(tuple, rig.params.tolist()))) == rig.N
    if rig.N == 8:
        assert {1.0, 4.0, 64.0} <= set(rig.params[:, driver_ref.L1].tolist()) and {1.0, 4.0, 64.0} <= set(rig.params[:, driver_ref.L2].tolist())
        assert {3.0, -3.0, 0.0} <= set(rig.params[:, driver_ref.OFFSET].tolist())


@pytest.mark.parametrize("mode", ["null", "given", "inplace"])
def test_actions_equal_the_restatement(rig, mode):
    rng = np.random.RandomState(17)
    for name in SETS:
        rig.set_bodies(rig.sets[name])
        ref = _want(rig, name)
        for mask in MASKS[rig.N]:
            got, src = _launch(rig, mask, mode, rng)
            scripted = np.array([(mask >> a) & 1 for a in range(rig.N)], bool)
            want = np.where(scripted[None, :, None], ref, np.zeros_like(ref) if src is None else src)
            assert_f32_bits(got, want, f"N {rig.N} mask {mask:#04x} in {mode}, poses {name}")
        if name == "nonfinite":
            got, _ = _launch(rig, (1 << rig.N) - 1, "null", rng)
            pos = hull_positions(rig.L, rig.sets[name])
            for e in range(rig.B):
                a = int(np.nonzero(np.isnan(pos[e]).any(axis=1))[0][0])
                assert (got[e, a].view(np.uint32) == 0).all(), f"env {e}: the NaN car's action {got[e, a].tolist()}"


def test_look_ahead_64_wraps_both_ways(rig):
    """host: from the poses near tile 0 a look-ahead of exactly 64 crosses the end of the track in CCW episodes and its start in CW ones (on
    20 tiles it laps the track three times).  With N = 1 the one car has the default row (4, 12): no 64 is involved, and the condition is
    only that the defaults cross the seam both ways."""
    pos = hull_positions(rig.L, rig.sets["start"])
    up = down = 0
    for e, (name, rows, cw) in enumerate(rig.tracks):
        T = len(rows)
        for a in range(rig.N):
            i = C.tied_tiles(rows, pos[e, a, 0], pos[e, a, 1])[1]
            assert min(i, T - i) <= 4
            for m in (rig.params[a, driver_ref.L1], rig.params[a, driver_ref.L2]):
                if rig.N > 1 and m != 64:
                    continue
                t = i + (-1 if cw else 1) * int(m)
                up += t >= T; down += t < 0
    assert up >= 2 and down >= 2, (up, down)


def test_actions_do_not_depend_on_the_batch(lib):
    """env e's rows inside B = 10 and alone (B = 1, env_offset = e: the same level of the cycle)"""
    N = 8
    tracks = C.all_tracks(lib)[0:10]
    prm = params(N)
    rng = np.random.RandomState(5)

    def run(r, bodies):
        r.params = prm
        r.set_bodies(bodies)
        return _launch(r, 0xff, "null", rng)[0]
    big = C.Rig(lib, tracks, N, "driver")
    try:
        sets = C.pose_sets(big.L, tracks, N, big.base["bodies"])
        rows = {name: run(big, sets[name]) for name in ("start", "scatter", "close")}
        for e in (0, 5, 9):
            one = C.Rig(lib, tracks[e:e + 1], N, "driver", env_offset=e, every=tracks)
            try:
                for name in rows:
                    assert_f32_bits(run(one, sets[name][e:e + 1]), rows[name][e:e + 1], f"env {e} alone, poses {name}")
            finally:
                one.close()
    finally:
        big.close()
