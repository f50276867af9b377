"""The lap scenario of tests/util.py on the CPU oracle alone: the conditions tests/test_gpu_lap_completion.py rests on.  A scenario that
stops reaching them — a track on which the controller stalls, a teleport that raises `done` — fails HERE instead of silently testing nothing
on the GPU.  Every (N, lapping car, direction, seed, env) of LAP_CASES, the trailing-car, touching-cars, teleport-onto-the-last-tile and
held-action (frame skip) variants."""
import numpy as np
import pytest

from tests.util import (LAP_CASES, LAP_DRIVE_MAX, LAP_TELEPORT_CONTACTS, lap_run, lap_teleport_phase, lap_drive_phase, lap_touching_pair,
                        playfield_ok)


def _teleport(run, trail=False):
    """teleport phase + its conditions; returns the car<->car contacts seen (summed over steps) per env"""
    B = len(run.orcs)
    cc = np.zeros(B, int)

    def chk(i, rew, done, got):
        assert not done.any(), f"teleport {i}: done raised"
        cc[:] += [o.num_car_contacts() for o in run.orcs]
    lap_teleport_phase(run, chk)
    for e, o in enumerate(run.orcs):
        left = o.T - int(run.tvc()[e, run.lap_car])
        assert 1 <= left <= 8, f"env {e}: {left} tiles left after the teleport phase (T = {o.T})"
    return cc


def _assert_lap_is_the_cause(run, e):
    o = run.orcs[e]
    assert int(o.env_state()["tile_visited_count"][run.lap_car]) == o.T
    assert playfield_ok(o), f"env {e}: a hull is outside the playfield"


@pytest.mark.parametrize("case", sorted(LAP_CASES))
def test_scenario_completes_a_lap_on_the_normal_path(oracle, case):
    N, lap_car, direction, seed, B = LAP_CASES[case]
    run = lap_run(oracle, case)
    cc_teleport = _teleport(run)
    assert cc_teleport.tolist() == list(LAP_TELEPORT_CONTACTS.get(case, (0,) * B)), f"manifold-steps of the teleport phase: {cc_teleport}"
    cc = np.zeros(B, int)
    first = [None] * B

    def chk(k, rew, done, got):
        cc[:] += [o.num_car_contacts() for o in run.orcs]
        for e in range(B):
            assert bool(done[e]) == bool(run.lapped()[e]), f"drive step {k} env {e}: done {done[e]} without / with a lap"
            if done[e] and first[e] is None:
                first[e] = k
                _assert_lap_is_the_cause(run, e)
                assert rew[e, lap_car] > 1000.0 / run.orcs[e].T - 0.2, f"env {e}: the completing step's reward {rew[e, lap_car]} lacks the tile's share"
    lap_drive_phase(run, chk)
    assert all(f is not None for f in first), f"lap not completed within {LAP_DRIVE_MAX} drive steps: {first}, tvc {run.tvc()[:, lap_car]}"
    assert min(first) >= 20, f"only {min(first)} ordinary steps between the last teleport and the completing step: too close to the re-created proxies"
    assert not cc.any(), f"car<->car contacts in the drive phase: {cc}"
    # three digits on the score label in the completing frame
    for o in run.orcs:
        assert o.env_state()["reward"][lap_car] >= 900.0


@pytest.mark.parametrize("case", ["n2", "n2cw"])
def test_scenario_with_a_trailing_car(oracle, case):
    N, lap_car, direction, seed, B = LAP_CASES[case]
    run = lap_run(oracle, case, trail_car=1 - lap_car)
    cc = _teleport(run)
    first = [None] * B

    def chk(k, rew, done, got):
        cc[:] += [o.num_car_contacts() for o in run.orcs]
        for e in range(B):
            if done[e] and first[e] is None:
                first[e] = k; _assert_lap_is_the_cause(run, e)
    lap_drive_phase(run, chk)
    assert all(f is not None and f >= 20 for f in first), first
    assert not cc.any(), f"the two cars touched: {cc}"
    for e, o in enumerate(run.orcs):
        r = o.env_state()["reward"]; tv = o.env_state()["tile_visited_count"]
        assert r[1 - lap_car] < r[lap_car], r
        assert tv[1 - lap_car] >= o.T - 12 and r[1 - lap_car] > 0.4 * r[lap_car], f"env {e}: the trailer did not follow the lap ({tv}, {r})"


def test_scenario_with_the_last_tile_reached_by_teleport(oracle):
    """the script simply goes on below LAP_K: `done` comes up in a step that directly follows a teleport"""
    run = lap_run(oracle, "n2")
    _teleport(run)
    first = [None] * len(run.orcs)
    for i in range(run.script_len(), run.script_len() + 16):
        run.teleport_to_point(i)
        rew, done, _ = run.step(run.idle())
        assert run.last_teleport == run.steps - 1
        for e in range(len(run.orcs)):
            assert bool(done[e]) == bool(run.lapped()[e])
            if done[e] and first[e] is None:
                first[e] = i; _assert_lap_is_the_cause(run, e)
        if all(f is not None for f in first):
            break
    assert all(f is not None for f in first), (first, run.tvc())


def test_scenario_with_touching_idle_cars(oracle):
    """N = 3: cars 1 and 2 stand overlapping a little while car 0 laps — the env holds manifolds in the completing step"""
    run = lap_run(oracle, "n3")
    _teleport(run)
    first = [None] * len(run.orcs)

    def chk(k, rew, done, got):
        for e in range(len(run.orcs)):
            if done[e] and first[e] is None:
                first[e] = k; _assert_lap_is_the_cause(run, e)
                assert run.orcs[e].num_car_contacts() > 0, f"env {e}: no car<->car contact in the completing step"
    lap_drive_phase(run, chk, before=lambda: lap_touching_pair(run, 1, 2))
    assert all(f is not None and f >= 20 for f in first), first


def test_scenario_under_held_actions(oracle):
    """frame_skip = 4: n single drive steps, then macro-steps of four env steps under one action — the lap completes, and over n = 0..3 in
    each of the four sub-steps"""
    subs = set()
    for n in range(4):
        run = lap_run(oracle, "n2", envs=[0])
        _teleport(run)
        run.to_spawn()
        for _ in range(n):
            _, done, _ = run.step(run.drive_actions()); assert not done.any()
        end = None
        for m in range(LAP_DRIVE_MAX // 4):
            a = run.drive_actions()
            for s in range(4):
                _, done, _ = run.step(a)
                if done[0]:
                    end = s; break
            if end is not None:
                break
        assert end is not None, f"n = {n}: no lap under held actions"
        _assert_lap_is_the_cause(run, 0)
        assert run.steps - 1 - run.last_teleport >= 20
        subs.add(end)
    assert subs == {0, 1, 2, 3}, subs
