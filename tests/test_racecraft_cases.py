"""CPU: the pose sets of tests/racecraft_cases.py take the branches of racecraft's definition (csrc/k_driver.h) they are named for — from
the restatement alone (tests/racecraft_ref.py: branches), no device.  tests/test_gpu_racecraft_kernel.py runs the kernel on the same sets."""
import collections

import numpy as np
import pytest

from tests import driver_ref as D
from tests import racecraft_cases as K
from tests import racecraft_ref as R
from tests.util import hull_positions


@pytest.fixture(scope="module")
def trks(lib):
    return K.tracks(lib)


@pytest.fixture(scope="module", params=K.NS, ids=lambda n: f"N{n}")
def cases(request, lib, trks):
    N = request.param
    L = lib.load()
    sets = K.pose_sets(L, trks, N, np.zeros((len(trks), N, 5, 6), np.float32))
    reports = {}
    for name, bodies in sets.items():
        reps = []
        K.ref_actions(L, trks, bodies, K.drv_rows(N), K.rc_rows(N, name), (1 << N) - 1, reps)
        reports[name] = reps
    return N, L, sets, reports


def test_every_set_takes_its_branch(cases, trks):
    N, L, sets, reports = cases
    assert set(sets) == set(K.SETS) - ({"twins"} if N < 3 else set())
    table = collections.OrderedDict()
    for name, reps in reports.items():
        fired = collections.Counter()
        for e, env in enumerate(reps):
            assert K.expect(name, env[0], N), f"N {N} set {name} env {e} ({trks[e][0]}, cw {trks[e][2]}): car 0's branches {env[0]}"
            for rep in env:
                fired.update(k for k, v in rep.items() if v not in (False, None, 0) or (k == "leader" and v is not None))
        table[name] = fired
    print(f"\nN = {N}: branches fired, summed over the {len(trks)} envs and all cars")
    for name, fired in table.items():
        print(f"  {name:16}" + "  ".join(f"{k} {fired[k]}" for k in R.BRANCHES if fired[k]))
    allf = sum(table.values(), collections.Counter())
    assert all(allf[k] for k in R.BRANCHES), f"a branch no set reaches: {[k for k in R.BRANCHES if not allf[k]]}"


def test_seam_is_crossed_both_ways(cases, trks):
    N, L, sets, _ = cases
    pos = hull_positions(L, sets["seam"])
    up = down = 0
    for e, (_, rows, cw) in enumerate(trks):
        tx, ty = D.track_arrays(rows)[:2]
        i0, i1 = (R.nearest_tile(tx, ty, np.float64(pos[e, a, 0]), np.float64(pos[e, a, 1])) for a in (0, 1))
        up += (not cw) and i1 < i0; down += cw and i1 > i0
    assert up == len(trks) // 2 and down == len(trks) // 2


def test_the_clamp_decides_on_the_small_track(cases, trks):
    """on 20 tiles with look = 64 the leader 9 tiles on is seen and the one 10 tiles on is not: (T - 1) / 2 = 9; on 512 tiles look itself decides"""
    N, L, sets, reports = cases
    for e, (name, rows, cw) in enumerate(trks):
        T = len(rows)
        G = min(64, (T - 1) // 2)
        assert (G < 64) == (T < 129)
        for which, want in (("clamp_in", G), ("clamp_out", G + 1)):
            pos = hull_positions(L, sets[which])
            tx, ty = D.track_arrays(rows)[:2]
            i0, i1 = (R.nearest_tile(tx, ty, np.float64(pos[e, a, 0]), np.float64(pos[e, a, 1])) for a in (0, 1))
            assert ((i1 - i0) * (-1 if cw else 1)) % T == want, (name, which)
    assert {len(t[1]) for t in trks} >= {20, 512}


def test_twins_have_bit_equal_x_and_differ_in_speed(cases, trks):
    N, L, sets, reports = cases
    if N < 3:
        pytest.skip("twins needs three cars")
    b = sets["twins"]
    assert np.array_equal(b[:, 1, 0, :3].view(np.uint32), b[:, 2, 0, :3].view(np.uint32)) and not np.array_equal(b[:, 1, 0, 3:5], b[:, 2, 0, 3:5])
    # the lowest index wins: with cars 1 and 2 exchanged car 0's follow cap — and its action — changes where the cap is active
    swapped = b.copy(); swapped[:, 1], swapped[:, 2] = b[:, 2], b[:, 1]
    drv, rc = K.drv_rows(N), K.rc_rows(N, "twins")
    one = K.ref_actions(L, trks, b, drv, rc, (1 << N) - 1); two = K.ref_actions(L, trks, swapped, drv, rc, (1 << N) - 1)
    assert (one[:, 0] != two[:, 0]).any()


def test_w_off_poses_are_one_float32_apart(cases, trks):
    N, L, sets, reports = cases
    up, dn = sets["w_off_above"][:, 0, 0], sets["w_off_below"][:, 0, 0]
    w = float(np.float32(R.DEFAULTS[R.W_OFF]))
    for e, (_, rows, cw) in enumerate(trks):
        diff = np.nonzero(up[e, :2] != dn[e, :2])[0]
        assert len(diff) == 1 and np.nextafter(dn[e, diff[0]], up[e, diff[0]]) == up[e, diff[0]], f"env {e}: {up[e, :2]} / {dn[e, :2]}"
        assert K._lat0(L, sets["w_off_above"][e, :1][0][None][0], rows, cw) > w >= K._lat0(L, sets["w_off_below"][e, 0], rows, cw)


def test_racecraft_off_mask_is_the_plain_driver(cases, trks):
    """a car outside the racecraft mask gets driver_ref's action whatever stands in front of it"""
    N, L, sets, _ = cases
    from tests import obs_cases as C
    for name in ("queue", "follow_zero"):
        got = K.ref_actions(L, trks, sets[name], K.drv_rows(N), K.rc_rows(N, name), 0)
        want = C.driver_ref_actions(L, trks, sets[name], K.drv_rows(N))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        on = K.ref_actions(L, trks, sets[name], K.drv_rows(N), K.rc_rows(N, name), (1 << N) - 1)
        assert (on[:, 0] != want[:, 0]).any(), name
