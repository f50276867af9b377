"""MI355X: k_driver<true> (csrc/k_driver.h) on the pose sets of tests/racecraft_cases.py, through the kernel's own launch (mcr_set_drivers +
mcr_set_racecraft + mcr_driver_actions) — bit for bit against tests/racecraft_ref.py on get_state() arrays.  No rollouts, no oracle.
tests/test_racecraft_cases.py holds every set to the branch it is named for."""
import ctypes

import numpy as np
import pytest

from tests import obs_cases as C
from tests import racecraft_cases as K
from tests import racecraft_ref as R
from tests.util import assert_f32_bits

pytestmark = pytest.mark.gpu

# (driver mask, racecraft mask): every car both; one scripted car among unscripted ones (which it still sees); racecraft for a strict subset
# of the scripted cars; masks that overlap in part
MASKS = {1: ((0x1, 0x1),), 2: ((0x3, 0x3), (0x1, 0x3), (0x3, 0x1), (0x2, 0x2)), 4: ((0xf, 0xf), (0x1, 0xf), (0xf, 0x5), (0x9, 0x3)),
         8: ((0xff, 0xff), (0x01, 0xff), (0xff, 0xa5), (0xa5, 0x0f))}
MODES = ("null", "given", "inplace")


@pytest.fixture(scope="module", params=[1, 2, 4, 8], ids=lambda n: f"N{n}")
def rig(request, lib):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    r = C.Rig(lib, K.tracks(lib), request.param, "driver")
    r.sets = K.pose_sets(r.L, r.tracks, r.N, r.base["bodies"])
    r.drv = K.drv_rows(r.N)
    r.want = {}
    yield r
    r.close()


def _want(rig, name, rc_mask):
    if (name, rc_mask) not in rig.want:
        rig.want[name, rc_mask] = K.ref_actions(rig.L, rig.tracks, rig.sets[name], rig.drv, K.rc_rows(rig.N, name), rc_mask)
    return rig.want[name, rc_mask]


def _launch(rig, name, drv_mask, rc_mask, mode, rng):
    """(out [B, N, 3], `in` as the kernel saw it or None); rc_mask None: racecraft turned off (a null row pointer)"""
    n = rig.B * rig.N * 3
    whole, view = rig.guarded(n)
    fill = rng.uniform(-1, 1, n).astype(np.float32); fill[::7] = -0.0
    src = None
    if mode == "given":
        src = rig.torch.from_numpy(fill).to(rig.env.device)
    elif mode == "inplace":
        view.copy_(rig.torch.from_numpy(fill).to(rig.env.device)); src = view
    if rig.scratch is None:
        rig.scratch = rig.torch.zeros(n, dtype=rig.torch.float32, device=rig.env.device)
    assert rig.L.mcr_set_drivers(rig.env.h, rig.lib.ptr(rig.drv), ctypes.c_uint32(drv_mask), ctypes.c_void_p(rig.scratch.data_ptr())) == 0
    if rc_mask is None:
        assert rig.L.mcr_set_racecraft(rig.env.h, None, ctypes.c_uint32(0)) == 0
    else:
        rows = K.rc_rows(rig.N, name)
        assert rig.L.mcr_set_racecraft(rig.env.h, rig.lib.ptr(rows), ctypes.c_uint32(rc_mask)) == 0
    st = rig.torch.cuda.current_stream(rig.env.device)
    assert rig.L.mcr_driver_actions(rig.env.h, None if src is None else ctypes.c_void_p(src.data_ptr()), ctypes.c_uint32(0),
                                    ctypes.c_void_p(view.data_ptr()), ctypes.c_void_p(st.cuda_stream)) == 0
    st.synchronize()
    assert rig.guards_intact(whole), "the words around the tensor were written"
    assert (rig.scratch == 0).all().item(), "the handle's own action buffer was written though `out` was given"
    return view.cpu().numpy().reshape(rig.B, rig.N, 3), (None if mode == "null" else fill.reshape(rig.B, rig.N, 3))


def _merge(ref, drv_mask, src, N):
    scripted = np.array([(drv_mask >> a) & 1 for a in range(N)], bool)
    return np.where(scripted[None, :, None], ref, np.zeros_like(ref) if src is None else src)


def test_actions_equal_the_restatement(rig):
    rng = np.random.RandomState(23)
    seen = set()
    for si, name in enumerate(rig.sets):
        rig.set_bodies(rig.sets[name])
        for ci, (drv_mask, rc_mask) in enumerate(MASKS[rig.N]):
            mode = MODES[(si + ci) % 3]
            seen.add((ci, mode))
            got, src = _launch(rig, name, drv_mask, rc_mask, mode, rng)
            assert_f32_bits(got, _merge(_want(rig, name, rc_mask), drv_mask, src, rig.N), f"N {rig.N} set {name} masks {drv_mask:#04x} / {rc_mask:#04x} in {mode}")
    assert len(seen) == 3 * len(MASKS[rig.N]), "every mask pair with `in` null, given and equal to `out`"


def test_cars_outside_the_racecraft_mask_drive_plainly(rig):
    """racecraft for a strict subset: the rest bit-equal to driver_ref, the subset different from it somewhere"""
    if rig.N == 1:
        pytest.skip("one car has no strict non-empty subset")
    rng = np.random.RandomState(29)
    drv_mask, rc_mask = MASKS[rig.N][2]
    differs = False
    for name in ("queue", "follow_zero", "step_left"):
        rig.set_bodies(rig.sets[name])
        plain = C.driver_ref_actions(rig.L, rig.tracks, rig.sets[name], rig.drv)
        got, _ = _launch(rig, name, drv_mask, rc_mask, "null", rng)
        rest = [a for a in range(rig.N) if not (rc_mask >> a) & 1]
        assert_f32_bits(got[:, rest], plain[:, rest], f"N {rig.N} set {name}: the cars outside the racecraft mask")
        differs |= bool((got[:, 0] != plain[:, 0]).any())
    assert differs, "car 0 races: its actions must differ from the plain controller's where it has a leader"


def test_racecraft_off_again_is_the_plain_driver(rig):
    """the same rig and inputs after mcr_set_racecraft(NULL): driver_ref, bit for bit — also for N = 1, where racecraft ON equals the plain
    driver except where the off-road cap holds"""
    rng = np.random.RandomState(31)
    full = (1 << rig.N) - 1
    for name in ("queue", "step_flipped", "w_off_above", "self_nonfinite"):
        rig.set_bodies(rig.sets[name])
        plain = C.driver_ref_actions(rig.L, rig.tracks, rig.sets[name], rig.drv)
        on, _ = _launch(rig, name, full, full, "null", rng)
        off, _ = _launch(rig, name, full, None, "null", rng)
        assert_f32_bits(off, plain, f"N {rig.N} set {name}: racecraft off again")
        if rig.N == 1 and name != "w_off_above":
            assert_f32_bits(on, plain, f"N 1 set {name}: alone on the road racecraft changes nothing")
        if name == "w_off_above":
            # (not in every env: on the 20-tile circle the plain controller's own target speed already asks for the full brake)
            assert (on[:, 0] != plain[:, 0]).any(axis=1).sum() >= rig.B // 2, "the off-road cap changes car 0's action"


def test_expert_override_uses_the_racecraft_mask(rig):
    """mcr_driver_actions(NULL, 0xffffffff, buf): every car, racecraft for the cars of the racecraft mask, whatever the driver mask is"""
    n = rig.B * rig.N * 3
    drv_mask, rc_mask = MASKS[rig.N][-1]
    name = "queue"
    rig.set_bodies(rig.sets[name])
    whole, view = rig.guarded(n)
    if rig.scratch is None:
        rig.scratch = rig.torch.zeros(n, dtype=rig.torch.float32, device=rig.env.device)
    assert rig.L.mcr_set_drivers(rig.env.h, rig.lib.ptr(rig.drv), ctypes.c_uint32(drv_mask), ctypes.c_void_p(rig.scratch.data_ptr())) == 0
    assert rig.L.mcr_set_racecraft(rig.env.h, rig.lib.ptr(K.rc_rows(rig.N, name)), ctypes.c_uint32(rc_mask)) == 0
    st = rig.torch.cuda.current_stream(rig.env.device)
    assert rig.L.mcr_driver_actions(rig.env.h, None, ctypes.c_uint32(0xffffffff), ctypes.c_void_p(view.data_ptr()), ctypes.c_void_p(st.cuda_stream)) == 0
    st.synchronize()
    assert rig.guards_intact(whole)
    assert_f32_bits(view.cpu().numpy().reshape(rig.B, rig.N, 3), _want(rig, name, rc_mask), f"N {rig.N}: expert override")
