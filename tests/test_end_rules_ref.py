"""CPU: known answers of the end-rule wrapper (tests/end_rules_ref.py) on the oracle — the definition the device is held to in
tests/test_gpu_end_rules.py: counters, the one env step of lag, both off-road modes, the counted cars, and what a natural ending or the
TimeLimit in the armed step leaves of `truncated`."""
import numpy as np
import pytest

from tests import end_rules_ref as R
from tests.util import lap_run, oracle_episode, rigid_teleport

FAR = 300.0          # a hull centre at (FAR, FAR): inside the playfield (|x|, |y| <= 2000 / 6), clear of every tile (asserted per episode)


def _env(O, N, seed, max_steps=0, **rules):
    ep = oracle_episode(O, N, seed, 0)
    w = R.EndRulesEnv(O.OracleEnv(N, car_contacts=True), max_steps=max_steps, **rules)
    w.reset(ep)
    return w, ep


def _teleport(w, car, x, y):
    b = w.o.state()["bodies"]
    moved = rigid_teleport(b[car], x, y, float(b[car, 0, 2]))
    for k in range(5):
        w.o.set_body(car, k, moved[k])


def _clear_of_tiles(ep, x, y):
    tr = ep["track"]
    return float(np.min(np.hypot(tr[:, 2] - x, tr[:, 3] - y))) > 40.0      # (a tile is ~7 wide and ~4 long, a car under 5 from hull centre to any corner)


@pytest.mark.parametrize("end_reward", [0.0, -25.5])
def test_idle_rule_counts_arms_and_ends_one_step_later(oracle, end_reward):
    w, ep = _env(oracle, 1, 11, patience=5, end_reward=end_reward)
    bare = oracle.OracleEnv(1, car_contacts=True); bare.reset(ep, render=False)
    s0 = int(w.o.env_state()["tile_visited_count"].sum())
    assert s0 > 0, "reset() visits the tiles the car stands on"
    # (the reference hands out what reset() earned with the first step: reset() zeroes prev_reward behind its own action-less step, so the
    # return of six idle steps is that credit - 0.6, not - 0.6)
    r0 = float(w.o.env_state()["reward"][0])
    assert abs(r0 - s0 * 1000.0 / len(ep["track"])) < 1e-9
    assert w.rules.counters.tolist() == [0, 0, s0, 0] and w.rules.armed == 0
    a = np.zeros((1, 3), np.float32)
    ret = np.zeros(1)
    for k in range(1, 7):
        _, rew, done, info = w.step(a)
        _, brew, bdone, _ = bare.step(a, render=False)
        assert not bdone
        if k < 6:
            assert np.array_equal(rew, brew) and not done and not info["truncated"] and info["end_reason"] == 0, k
            assert w.rules.counters.tolist() == [k, 0, s0, 0], (k, w.rules.counters)
            assert w.rules.armed == (R.END_IDLE if k == 5 else 0), k
            ret = ret + brew
        else:
            ret = ret + (brew + np.float64(end_reward))
            assert np.array_equal(rew, brew + np.float64(end_reward)), "one f64 add behind the reference's reward"
            assert done and info["truncated"] and info["end_reason"] == R.END_IDLE
            assert info["episode_length"] == 6 and np.array_equal(info["episode_return"], ret)
            assert abs(float(info["episode_return"][0]) - (r0 - 0.6 + end_reward)) < 1e-9
    # stepped past the ending without a reset (auto_reset=False): still idle, still armed, done again
    _, rew, done, info = w.step(a)
    assert done and info["truncated"] and info["end_reason"] == R.END_IDLE and w.rules.counters[0] == 7


def test_only_the_counted_cars_count(oracle):
    """N = 2, car 1 drives along the track, car 0 stays on the grid: counting the parked car ends the episode at step P + 1, counting the
    driving car alone does not end it within the run (its longest wait for a new tile is asserted to be shorter than P)"""
    P, steps = 60, 150
    for agents, ends in (((0,), True), ((1,), False), (None, False)):
        run = lap_run(oracle, "n2", envs=[0])
        assert run.lap_car == 1
        w = R.EndRulesEnv(run.orcs[0], patience=P, agents=agents)
        w.rules.first_state(w.rules.read(w.o)[0])
        ended_at, longest = None, 0
        for k in range(1, steps + 1):
            _, _, done, info = w.step(run.drive_actions()[0])
            longest = max(longest, int(w.rules.counters[0]))
            if done:
                ended_at = k
                assert info["truncated"] and info["end_reason"] == R.END_IDLE
                break
        if ends:
            assert ended_at == P + 1
        else:
            assert ended_at is None and longest < P - 10, f"end_agents={agents}: ended at {ended_at}, longest wait {longest}"
            assert int(w.o.env_state()["tile_visited_count"][1]) > 20, "the driving car did not get anywhere"


@pytest.mark.parametrize("mode, moved, ends", [("all", (0, 1), True), ("all", (1,), False), ("any", (1,), True), ("any", (), False)])
def test_offroad_rule_in_both_modes(oracle, mode, moved, ends):
    """N = 2, G = 4, the cars of `moved` put on the grass far from every tile before the first step: the count runs 1..4, the env is armed
    behind step 4 and ends in step 5 — in "all" mode only when no counted car is left on the road, in "any" mode as soon as one has left it"""
    w, ep = _env(oracle, 2, 23, offroad=4, mode=mode)
    assert _clear_of_tiles(ep, FAR, FAR) and _clear_of_tiles(ep, FAR, FAR - 30.0)
    for c in moved:
        _teleport(w, c, FAR, FAR - 30.0 * c)
    a = np.zeros((2, 3), np.float32)
    for k in range(1, 9):
        _, rew, done, info = w.step(a)
        on = w.o.state()["on_road"]
        for c in range(2):
            assert bool(on[c].any()) == (c not in moved), f"step {k}: car {c} on_road {on[c]}"
        if ends:
            assert int(w.rules.counters[1]) == k, (k, w.rules.counters)
            assert w.rules.armed == (R.END_OFFROAD if k >= 4 else 0)
            assert done == (k >= 5) and info["end_reason"] == (R.END_OFFROAD if k >= 5 else 0) and info["truncated"] == (k >= 5)
        else:
            assert int(w.rules.counters[1]) == 0 and w.rules.armed == 0 and not done and info["end_reason"] == 0
    # back on the road (the spawn pose is on tiles): the count starts over
    if ends and mode == "all":
        w2, _ = _env(oracle, 2, 23, offroad=4, mode=mode)
        spawn = w2.o.state()["bodies"]
        for c in moved:
            for kb in range(5):
                w.o.set_body(c, kb, spawn[c, kb])
        w.step(a)
        assert int(w.rules.counters[1]) == 0 and w.rules.armed == 0


def test_both_rules_arm_together(oracle):
    w, ep = _env(oracle, 1, 5, patience=3, offroad=3)
    _teleport(w, 0, FAR, FAR)
    assert _clear_of_tiles(ep, FAR, FAR)
    a = np.zeros((1, 3), np.float32)
    for k in range(1, 4):
        _, _, done, _ = w.step(a)
        assert not done
    assert w.rules.counters[:2].tolist() == [3, 3] and w.rules.armed == (R.END_IDLE | R.END_OFFROAD)
    _, _, done, info = w.step(a)
    assert done and info["truncated"] and info["end_reason"] == 3


@pytest.mark.parametrize("natural", ["playfield", "timelimit", "none"])
def test_truncated_is_0_when_the_armed_step_ends_by_itself(oracle, natural):
    """P = 5: step 6 is the armed step.  The car leaves the playfield in it (the reference's own ending: reward -100), or the TimeLimit falls
    on it (max_episode_steps = 6): truncated = 0, end_reason still says that the rule was met.  Neither: truncated = 1."""
    w, ep = _env(oracle, 1, 11, max_steps=6 if natural == "timelimit" else 0, patience=5, end_reward=-2.0)
    a = np.zeros((1, 3), np.float32)
    for k in range(1, 6):
        _, _, done, _ = w.step(a)
        assert not done
    assert w.rules.armed == R.END_IDLE
    if natural == "playfield":
        _teleport(w, 0, 2000 / 6.0 + 20.0, 0.0)
    _, rew, done, info = w.step(a)
    assert done and info["end_reason"] == R.END_IDLE and info["episode_length"] == 6
    assert info["truncated"] == (natural == "none")
    if natural == "playfield":
        assert rew[0] == -100.0 + -2.0


def test_counters_saturate():
    r = R.EndRules(1, patience=3, offroad=2)
    r.counters[:] = (R.INT32_MAX - 1, R.INT32_MAX, 7, 0)
    r.advance(7, True)
    assert r.counters.tolist() == [R.INT32_MAX, R.INT32_MAX, 7, 0] and r.armed == 3
    r.advance(7, True)
    assert r.counters.tolist() == [R.INT32_MAX, R.INT32_MAX, 7, 0]
    r.advance(8, False)
    assert r.counters.tolist() == [0, 0, 8, 0] and r.armed == 0


def test_settle_keeps_the_counters_of_a_running_episode():
    r = R.EndRules(2, patience=4, agents=(1,))
    r.counters[:] = (4, 9, 3, 0)
    r.settle(17, 99)
    assert r.counters.tolist() == [4, 9, 3, 0] and r.armed == R.END_IDLE
    r.settle(0, 5)
    assert r.counters.tolist() == [0, 0, 5, 0] and r.armed == 0
    # the sum wraps as u32 and reads as int32
    assert r.read_arrays(np.array([1, 2 ** 31 - 1], np.int32), np.ones((2, 4), np.uint8)) == (2 ** 31 - 1, False)
    assert R.EndRules(2, offroad=1).read_arrays(np.array([2 ** 31 - 1, 1], np.int32), np.zeros((2, 4), np.uint8)) == (-2 ** 31, True)
