"""MI355X: k_endrules alone (csrc/k_endrules.h).  The caller owns the counters, so the tests write rows directly, then run the settle pass
(refresh_end_rules) or take one step (the advance pass), and hold every row to tests/end_rules_ref.py applied to the state the device
reports (tile_visited_count, the wheels' on_road bits).  Batch sizes round the 64-lane wavefront, N = 1, 2, 8."""
import warnings

import numpy as np
import pytest

from tests import end_rules_ref as R
from tests.util import rigid_teleport

pytestmark = pytest.mark.gpu

P, G = 6, 4
IMAX = R.INT32_MAX
SENTINEL = -77


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _make(B, N, **kw):
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    kw.setdefault("end_patience", P); kw.setdefault("end_offroad", G)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return VecMultiCarRacing(B, N, seed=5, car_contacts=True, obs=False, async_refill=False, auto_reset=False, max_episode_steps=0,
                                 use_random_direction=False, streams=1, **kw)


def _rules(env):
    return [R.EndRules(env.N, patience=env.end_patience, offroad=env.end_offroad, mode=env.end_offroad_mode, agents=env.end_agents,
                       end_reward=env.end_reward) for _ in range(env.B)]


def _read(env):
    """per env (s, cond) from the device's own state, through the reference's reader"""
    tvc = env.get_env_state()["tile_visited_count"]; on = env.get_state()["on_road"]
    return [r.read_arrays(tvc[e], on[e]) for e, r in enumerate(_rules(env))], tvc, on


def _rows(B, s):
    """counter rows that meet every branch: idle at P - 2, P - 1, P and INT32_MAX, the sum unchanged or changed, offroad at 0, G - 1, G, INT32_MAX"""
    idle = [P - 2, P - 1, P, IMAX, 0]; off = [0, G - 1, G, IMAX]
    rows = np.zeros((B, 4), np.int32)
    for e in range(B):
        rows[e] = (idle[e % 5], off[(e // 5) % 4], s[e] + (1 if e % 7 == 3 else 0), 0)
    return rows


def _off_road(env, envs):
    st = env.get_state()["bodies"].copy()
    for e in envs:
        for c in range(env.N):
            st[e, c] = rigid_teleport(st[e, c], 300.0 - 14.0 * (c % 4), 300.0 - 14.0 * (c // 4), float(st[e, c, 0, 2]))
    env.set_bodies(st)


@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("N,agents", [(1, None), (2, None), (8, None), (8, (7,))], ids=["N1", "N2", "N8", "N8_last_car"])
def test_settle_and_advance_match_the_reference_row_by_row(torch_cuda, B, N, agents):
    torch = torch_cuda
    env = _make(B, N, end_agents=agents, end_reward=-2.0)
    assert env.end_agents == (tuple(range(N)) if agents is None else agents)
    a = torch.zeros((B, N, 3), dtype=torch.float32, device="cuda")
    # ---- before reset(): inactive rows keep their counters, are disarmed, and the reason is left alone by the settle pass
    env.end_counters.fill_(SENTINEL); env.end_armed.fill_(3); env.end_reason.fill_(2)
    cnt, why = env.refresh_end_rules()
    assert cnt is env.end_counters and why is env.end_reason
    assert (env.end_counters == SENTINEL).all().item() and not env.end_armed.any().item() and (env.end_reason == 2).all().item()
    # ---- reset(): the first state of an episode starts over
    env.reset()
    reads, tvc, _ = _read(env)
    assert (tvc.sum(1) > 0).all(), "reset() visits the tiles under the cars"
    assert env.end_counters.cpu().numpy().tolist() == [[0, 0, s, 0] for s, _ in reads] and not env.end_armed.any().item() and not env.end_reason.any().item()
    first = _rules(env)
    for e, r in enumerate(first):
        r.first_state(reads[e][0])
    env.step(a)                                              # steps = 1: from here on the rows are a running episode's
    reads, _, _ = _read(env)
    for e, r in enumerate(first):                            # (a standing car may still settle onto one more tile in its first step: idle 0 there, 1 elsewhere)
        r.advance(*reads[e])
    assert env.end_counters.cpu().numpy().tolist() == [r.counters.tolist() for r in first]
    assert {int(r.counters[0]) for r in first} <= {0, 1} and (B < 63 or any(int(r.counters[0]) == 1 for r in first))
    # ---- settle on rows written by the caller: counters untouched, armed recomputed from them
    rows = _rows(B, [s for s, _ in reads])
    env.end_counters.copy_(torch.from_numpy(rows)); env.end_armed.fill_(3); env.end_reason.fill_(1)
    env.refresh_end_rules()
    rules = _rules(env)
    for e, r in enumerate(rules):
        r.counters[:] = rows[e]; r.settle(1, reads[e][0])
    assert np.array_equal(env.end_counters.cpu().numpy(), rows)
    armed0 = np.array([r.armed for r in rules], np.uint8)
    assert np.array_equal(env.end_armed.cpu().numpy(), armed0) and (env.end_reason == 1).all().item()
    if B >= 63:
        assert set(armed0.tolist()) == {0, 1, 2, 3}
    # ---- one step: the armed rows end (reason = the word they entered with), every row advances; half of the envs are on the grass
    _off_road(env, range(0, B, 2))
    _, rew, done, info = env.step(a)
    assert np.array_equal(info["end_reason"].cpu().numpy(), armed0) and np.array_equal(done.cpu().numpy() != 0, armed0 != 0)
    assert np.array_equal(env.truncated.cpu().numpy() != 0, armed0 != 0)
    reads, _, on = _read(env)
    for e, r in enumerate(rules):
        r.advance(*reads[e])
        assert reads[e][1] == (e % 2 == 0), f"env {e}: on_road {on[e].tolist()}"
    want = np.array([r.counters for r in rules], np.int32)
    got = env.end_counters.cpu().numpy()
    assert np.array_equal(got, want), f"rows {np.nonzero((got != want).any(1))[0][:8].tolist()}: {got[(got != want).any(1)][:4].tolist()} vs {want[(got != want).any(1)][:4].tolist()}"
    armed1 = np.array([r.armed for r in rules], np.uint8)
    assert np.array_equal(env.end_armed.cpu().numpy(), armed1)
    for e in range(B):                                       # the saturated rows stay where they are
        if rows[e, 0] == IMAX and rows[e, 2] == reads[e][0]:
            assert got[e, 0] == IMAX
        if rows[e, 1] == IMAX and e % 2 == 0:
            assert got[e, 1] == IMAX
    if B >= 63:
        assert 3 in armed1.tolist(), "no row armed by both rules together"
    # ---- and the step after it ends those: reason 3 where both rules armed
    _, _, done, info = env.step(a)
    assert np.array_equal(info["end_reason"].cpu().numpy(), armed1) and np.array_equal(done.cpu().numpy() != 0, armed1 != 0)
    assert env.status_words()[:5].tolist() == [0] * 5
    env.close()


@pytest.mark.parametrize("B,N", [(65, 2), (3, 8)])
def test_views_one_row_off_their_allocation(torch_cuda, B, N):
    """the three tensors as views that start one row into a larger allocation (16 bytes for the counters, ONE byte for armed and reason): the
    rows in front of and behind the views keep their sentinels through a settle pass and two steps"""
    torch = torch_cuda
    env = _make(B, N)
    big_c = torch.full((B + 2, 4), SENTINEL, dtype=torch.int32, device="cuda")
    big_a = torch.full((B + 2,), 9, dtype=torch.uint8, device="cuda"); big_r = torch.full((B + 2,), 9, dtype=torch.uint8, device="cuda")
    env.end_counters, env.end_armed, env.end_reason = big_c[1:B + 1], big_a[1:B + 1], big_r[1:B + 1]
    env._set_end_rules()
    env.reset()
    a = torch.zeros((B, N, 3), dtype=torch.float32, device="cuda")
    env.step(a)
    reads, _, _ = _read(env)
    rows = _rows(B, [s for s, _ in reads])
    env.end_counters.copy_(torch.from_numpy(rows))
    env.refresh_end_rules()
    rules = _rules(env)
    for e, r in enumerate(rules):
        r.counters[:] = rows[e]; r.settle(1, reads[e][0])
    armed0 = np.array([r.armed for r in rules], np.uint8)
    _, _, done, info = env.step(a)
    reads, _, _ = _read(env)
    for e, r in enumerate(rules):
        r.advance(*reads[e])
    assert np.array_equal(env.end_counters.cpu().numpy(), np.array([r.counters for r in rules], np.int32))
    assert np.array_equal(env.end_reason.cpu().numpy(), armed0) and np.array_equal(done.cpu().numpy() != 0, armed0 != 0)
    assert np.array_equal(env.end_armed.cpu().numpy(), np.array([r.armed for r in rules], np.uint8))
    for t, v in ((big_c, SENTINEL), (big_a, 9), (big_r, 9)):
        assert (t[0] == v).all().item() and (t[B + 1] == v).all().item(), "a guard row was written"
    env.close()
