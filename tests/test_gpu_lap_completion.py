"""MI355X: lap completion — the episode ending of `len(self.track) in self.tile_visited_count` (multi_car_racing.py:498), which a trained policy
produces and no random rollout of a few hundred steps reaches.  The lap scenario of tests/util.py (a teleport phase that visits all but a
handful of tiles, then an ordinary finishing stretch; tests/test_lap_scenario.py holds it to its conditions on the CPU) brings a car to
`tile_visited_count == T` in ~350 steps.  The reference is the oracle throughout: rewards, done, truncated, the rigid-body and env state are
compared BIT-EXACT, frames exactly outside the oracle's ambiguity mask (budget 40 per view, as tests/test_gpu_parity.py compares such frames).

(a) the step the lap ends in, on the normal contact-pass path; (b) with the contact pass in front (right after a set_bodies); (c) from the
contact chain; (d) a trailing car taking the damped share of every tile; (e) a lap on the TimeLimit step; (f) the auto-reset behind a lap;
(g) its terminal frame; (h) inside a macro-step of frame_skip = 4; (i) the state vector; (j) 256 envs finishing in one step."""
import os

import numpy as np
import pytest

from tests import state_obs_ref as R
from tests.util import (LAP_CASES, LAP_DRIVE_MAX, assert_frame, assert_state, env_streams, lap_drive_phase, lap_run, lap_teleport_phase,
                        lap_touching_pair, make_env)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _make(case, B=None, **kw):
    N, _, direction, seed, nB = LAP_CASES[case]
    return make_env(nB if B is None else B, N, seed, direction=direction, **kw)


def _np(got):
    obs, rew, done, info = got
    return (None if obs is None else obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy().astype(bool),
            info["TimeLimit.truncated"].cpu().numpy().astype(bool))


def _same_step(what, rew, done, got, truncated=None):
    """one step's outputs against the oracles': rewards bit for bit, done, truncated (default: never); returns (obs, rewards, done, truncated)"""
    obs, rw, dn, tr = _np(got)
    n = len(rew)
    assert np.array_equal(rw[:n], rew), f"{what}: rewards {rw[:n].tolist()} vs the oracle's {rew.tolist()}"
    assert np.array_equal(dn[:n], done), f"{what}: done {dn[:n].tolist()} vs the oracle's {done.tolist()}"
    assert np.array_equal(tr[:n], np.zeros(n, bool) if truncated is None else truncated), f"{what}: truncated {tr[:n].tolist()}"
    return obs, rw, dn, tr


def _contact_counts(env):
    from multi_car_racing_amd import _lib
    cnt = np.zeros(env.B, np.int32)
    _lib.check(env.L.mcr_debug_read_contact_counts(env.h, _lib.ptr(cnt)))
    return cnt


def _teleport_in_lockstep(run):
    def chk(i, rew, done, got):
        _same_step(f"teleport {i}", rew, done, got)
    lap_teleport_phase(run, chk)
    assert not run.lapped().any()


def _assert_lap_end(env, run, e, obs, what):
    """the completing step of env e: the lapping car's count is T on both sides, the whole state is the oracle's, the frame is the oracle's —
    with a score of 900 and more on the label and every tile touched"""
    o = run.orcs[e]; es = env.get_env_state(); eo = o.env_state()
    assert int(es["tile_visited_count"][e, run.lap_car]) == int(es["num_tiles"][e]) == o.T == int(eo["tile_visited_count"][run.lap_car]), what
    assert_state(env, enumerate(run.orcs), what)
    if run.N == 8:      # the eighth "visited" bit of tile_flags
        assert np.array_equal(es["tile_flags"][e, :o.T] & 0xff, eo["visited"]) and ((es["tile_flags"][e, :o.T] >> 7) & 1).all(), what
    if obs is not None:
        assert eo["reward"][run.lap_car] >= 900.0 and eo["touched"].all(), "the frame is meant to show a three-digit score and a fully touched track"
        assert_frame(obs[e], o.last_obs, o.last_amb, what, 40)


def _drive_to_the_lap(env, run, before=None, on_end=None):
    """drive phase in lockstep: every step's outputs, the state every 10 steps, _assert_lap_end in each env's completing step"""
    ended = [None] * len(run.orcs)

    def chk(k, rew, done, got):
        obs, _, _, _ = _same_step(f"drive step {k}", rew, done, got)
        if k % 10 == 9:
            assert_state(env, enumerate(run.orcs), f"drive step {k}")
        for e in range(len(run.orcs)):
            if done[e] and ended[e] is None:
                ended[e] = k
                _assert_lap_end(env, run, e, obs, f"completing step (drive step {k}) env {e}")
                if on_end is not None:
                    on_end(e, k)
    lap_drive_phase(run, chk, before=before, render=env.obs_enabled)
    assert all(k is not None for k in ended), f"no lap within {LAP_DRIVE_MAX} drive steps: {ended}"
    return ended


# ------------------------------------------------------------------------------------------------------------ (a) the step the lap ends in
@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("case", ["n1", "n2", "n2cw", "n3", "n8"])
def test_lap_ends_in_the_oracles_step(torch_cuda, oracle, case, streams):
    """(N, lapping car) = (1, 0), (2, 1) CCW and CW, (3, 0), (8, 7), the other cars idle on the grid; auto_reset off.  `done` comes up in the step
    whose contact pass touches the last tile — not a step later — with the 1000/T share in that step's reward, in whichever lane the car sits."""
    env = _make(case, streams=streams); env.reset()
    run = lap_run(oracle, case, env=env)
    assert_state(env, enumerate(run.orcs), "after reset")
    _teleport_in_lockstep(run)
    assert_state(env, enumerate(run.orcs), "end of the teleport phase")
    ended = _drive_to_the_lap(env, run)
    assert min(ended) >= 20, ended
    assert not env.status_words()[:5].any() and env.verdict_mismatches() == 0
    env.close()


# ------------------------------------------------------------------------------------------------------------ (b) contact pass in front
def test_lap_ends_in_the_step_after_a_teleport(torch_cuda, oracle):
    """the last tile is reached by a teleport: the completing step is the one right behind a set_bodies, which runs the contact pass in
    front of the dynamics with every car proxy re-created"""
    env = _make("n2"); env.reset()
    run = lap_run(oracle, "n2", env=env)
    _teleport_in_lockstep(run)
    ended = [None] * env.B
    for i in range(run.script_len(), run.script_len() + 16):
        run.teleport_to_point(i)
        rew, done, got = run.step(run.idle(), render=True)
        obs, _, _, _ = _same_step(f"teleport {i}", rew, done, got)
        assert run.last_teleport == run.steps - 1
        for e in range(env.B):
            if done[e] and ended[e] is None:
                ended[e] = i; _assert_lap_end(env, run, e, obs, f"completing teleport {i} env {e}")
        if run.lapped().all():
            break
    assert all(k is not None for k in ended), ended
    env.close()


# ------------------------------------------------------------------------------------------------------------ (c) from the contact chain
def test_lap_ends_in_an_env_of_the_contact_chain(torch_cuda, oracle):
    """N = 3, streams = 2: car 0 laps while cars 1 and 2 stand touching — the env is stepped by the contact chain, which reads the lapping
    car's count on its own branch"""
    env = _make("n3", streams=2); env.reset()
    run = lap_run(oracle, "n3", env=env)
    _teleport_in_lockstep(run)

    def on_end(e, k):
        assert _contact_counts(env)[e] > 0 and run.orcs[e].num_car_contacts() > 0, f"env {e}: no manifold in the completing step"
    _drive_to_the_lap(env, run, before=lambda: lap_touching_pair(run, 1, 2), on_end=on_end)
    assert not env.status_words()[:5].any() and env.verdict_mismatches() == 0
    env.close()


# ------------------------------------------------------------------------------------------------------------ (d) both cars lap
@pytest.mark.parametrize("case", ["n2", "n2cw"])
def test_trailing_car_takes_the_damped_share_of_a_whole_lap(torch_cuda, oracle, case):
    """N = 2, the other car teleported 4 track points behind the lapping one: second visitor of ~250 tiles, `1 - past_visitors / N` of 1000/T
    each (multi_car_racing.py:113-120), summed in f64 in Box2D's event order"""
    N, lap_car, _, _, _ = LAP_CASES[case]
    env = _make(case); env.reset()
    run = lap_run(oracle, case, trail_car=1 - lap_car, env=env)
    _teleport_in_lockstep(run)
    _drive_to_the_lap(env, run)
    es = env.get_env_state()
    for e, o in enumerate(run.orcs):
        eo = o.env_state()
        assert np.array_equal(es["reward"][e], eo["reward"]) and np.array_equal(es["tile_visited_count"][e], eo["tile_visited_count"])
        assert eo["tile_visited_count"][1 - lap_car] >= o.T - 12 and 0.4 * eo["reward"][lap_car] < eo["reward"][1 - lap_car] < eo["reward"][lap_car]
    env.close()


# ------------------------------------------------------------------------------------------------------------ handles restored from a builder
_BLOBS = {}


def _near_complete(oracle, case):
    """state blobs of the case's envs at the end of the teleport phase, built once on a small handle (every step checked against the oracle)"""
    if case not in _BLOBS:
        env = _make(case, streams=1); env.reset()
        run = lap_run(oracle, case, env=env)
        _teleport_in_lockstep(run)
        _BLOBS[case] = [env.get_state_blob(e) for e in range(env.B)]
        env.close()
    return _BLOBS[case]


def _restored(oracle, case, B=None, **kw):
    """(handle of configuration kw whose envs continue from the builder's blobs, LapRun of fresh oracles that replayed the teleport script on
    the CPU, the f64 return of every car so far)"""
    blobs = _near_complete(oracle, case)
    env = _make(case, B=B, **kw); env.reset()
    n = min(env.B, len(blobs))
    for e in range(n):
        env.set_state_blob(e, blobs[e])
    run = lap_run(oracle, case, envs=range(n))
    ret = np.zeros((n, run.N))

    def add(i, rew, done, got):
        ret[:] = ret + rew
    lap_teleport_phase(run, add)
    run.env = env
    return env, run, ret


def _second_episode(oracle, run, e, render=True):
    """env e's oracle installs its second episode on its one world; returns the first observation"""
    ep = oracle.new_episode(run.N, *run.streams[e], direction=run.direction, use_random_direction=False)
    run.eps[e] = ep
    obs = run.orcs[e].reset(ep, render=render)
    run.spawn[e] = run.orcs[e].state()["bodies"].copy()
    return obs


# ------------------------------------------------------------------------------------------------------------ (e) lap on the TimeLimit step
def test_lap_on_the_time_limit_step_is_not_truncated(torch_cuda, oracle):
    """`trunc = !done`: a lap that completes exactly on the TimeLimit step reports TimeLimit.truncated == False; a limit one step shorter
    truncates a step early; one step longer changes nothing"""
    def play(limit):
        env, run, _ = _restored(oracle, "n2", B=1, auto_reset=True, max_episode_steps=limit)
        run.to_spawn()
        for k in range(LAP_DRIVE_MAX):
            rew, done, got = run.step(run.drive_actions())
            over = limit > 0 and run.steps >= limit
            _, _, dn, tr = _same_step(f"limit {limit} step {run.steps}", rew, done | over, got, truncated=np.array([over and not done[0]]))
            if dn[0]:
                length = int(got[3]["episode_length"][0].item())
                env.close()
                return run.steps, bool(done[0]), bool(tr[0]), length
        raise AssertionError(f"limit {limit}: the episode did not end")
    s, lapped, trunc, length = play(0)
    assert lapped and not trunc and length == s, (s, lapped, trunc, length)      # (s: the env's own step counter at the completing step)
    assert play(s - 1) == (s - 1, False, True, s - 1)
    assert play(s) == (s, True, False, s)
    assert play(s + 1) == (s, True, False, s)


# ------------------------------------------------------------------------------------------------------------ (f), (g) auto-reset, terminal frame
def _lap_then_auto_reset(torch, oracle, streams, terminal):
    env, run, ret = _restored(oracle, "n2", auto_reset=True, streams=streams, terminal_obs=terminal)
    B = env.B
    run.to_spawn()
    ended = [None] * B
    n_before, _ = env.rollout_stats()
    assert n_before == 0
    for k in range(LAP_DRIVE_MAX + 30):
        rew, done, got = run.step(run.drive_actions(), render=True)
        obs, _, dn, _ = _same_step(f"drive step {k}", rew, done, got)
        ret[:] = ret + rew * np.array([x is None for x in ended])[:, None]
        if terminal:
            ids, frames = env.terminal_observations()
            assert sorted(ids.cpu().numpy().tolist()) == np.nonzero(dn)[0].tolist(), f"drive step {k}: terminal entries"
        for e in np.nonzero(done)[0]:
            assert ended[e] is None, f"env {e}: a second ending"
            ended[e] = k
            o = run.orcs[e]
            assert int(o.env_state()["tile_visited_count"][run.lap_car]) == o.T, "the lap is meant to be the cause"
            if terminal:       # the LAST frame of the finished episode: the oracle's frame of the completing step
                i = ids.cpu().numpy().tolist().index(e)
                assert_frame(frames[i].cpu().numpy(), o.last_obs, o.last_amb, f"terminal frame env {e}", 40)
            assert np.array_equal(got[3]["episode_return"][e].cpu().numpy(), ret[e]), f"env {e}: episode_return vs the ordered f64 sum"
            assert int(got[3]["episode_length"][e].item()) == run.steps
            first = _second_episode(oracle, run, e)
            assert_frame(obs[e], first, o.last_amb, f"env {e}: first frame after the lap", 40)
        if len(np.nonzero(done)[0]) or k % 10 == 9:
            assert_state(env, enumerate(run.orcs), f"drive step {k}")             # (a re-spawned env: its new episode's reset state, counts cleared)
        if all(x is not None for x in ended) and k >= max(ended) + 30:
            break
    assert all(x is not None for x in ended), ended
    n_ep, ret_sum = env.rollout_stats()
    # (the one comparison here that is not bit-exact: the B * N returns, ~1e3 each, reach the sum through f64 atomicAdds in no fixed order,
    #  so it is any of their orderings' sums — a few ulp of 1e3-1e4, ~1e-12, apart; 1e-9 is far above that and far below any one reward)
    assert n_ep == B and abs(ret_sum - ret.sum()) < 1e-9
    assert not env.status_words()[:5].any() and int(env.debug_counters()[3]) == 0
    env.close()


@pytest.mark.parametrize("streams", [1, 2])
def test_auto_reset_behind_a_lap(torch_cuda, oracle, streams):
    """the completing step returns the next episode's first observation and state (the oracle's second episode on its one world), the
    episode statistics of the lap, and 30 further steps stay bit-exact without another `done`"""
    _lap_then_auto_reset(torch_cuda, oracle, streams, terminal=False)


def test_terminal_frame_of_a_lap(torch_cuda, oracle):
    _lap_then_auto_reset(torch_cuda, oracle, int(os.environ.get("MCR_TEST_STREAMS", "1")), terminal=True)


# ------------------------------------------------------------------------------------------------------------ (h) frame skip
def test_lap_inside_a_macro_step(torch_cuda, oracle):
    """frame_skip = 4 (tests/test_gpu_frame_skip.py states the contract): after n = 0..3 single drive steps the macro-steps begin, so the lap
    completes in each of the four sub-steps.  The macro-step's reward is the f64 sum up to and including the completing sub-step, `done` is
    set, and no sub-step of the new episode is taken: observation and state are the untouched first ones of the next episode."""
    K = 4
    subs = set()
    for n in range(4):
        env, run, _ = _restored(oracle, "n2", B=1, auto_reset=True, frame_skip=K)
        if n:               # single steps need a frame_skip = 1 handle: it takes the first n drive steps and hands its state on
            one, _, _ = _restored(oracle, "n2", B=1)
            run.env = one
            run.to_spawn()
            for k in range(n):
                rew, done, got = run.step(run.drive_actions()); _same_step(f"n {n} single step {k}", rew, done, got)
            env.set_state_blob(0, one.get_state_blob(0)); one.close()
            run.env = env
        else:
            run.to_spawn()
        o = run.orcs[0]
        end = None
        for m in range(LAP_DRIVE_MAX // K):
            a = run.drive_actions()
            obs, rew, done, info = env.step(torch_cuda.from_numpy(a).cuda())
            total = np.zeros(run.N)
            for s in range(K):
                _, r, d, _ = o.step(a[0], render=False); run.steps += 1
                total = total + r
                if d:
                    end = s; break
            assert np.array_equal(rew[0].cpu().numpy(), total), f"n {n} macro-step {m}: reward vs the ordered sum (ending in sub-step {end})"
            assert bool(done[0].item()) == (end is not None) and not bool(info["TimeLimit.truncated"][0].item())
            if end is not None:
                break
        assert end is not None and int(o.env_state()["tile_visited_count"][run.lap_car]) == o.T, f"n {n}: no lap"
        assert int(info["episode_length"][0].item()) == run.steps
        first = _second_episode(oracle, run, 0)
        assert_frame(obs[0].cpu().numpy(), first, o.last_amb, f"n {n}: first frame of the next episode", 40)
        assert_state(env, enumerate(run.orcs), f"n {n}: the next episode, not advanced")
        subs.add(end)
        env.close()
    assert subs == {0, 1, 2, 3}, f"completing sub-steps seen: {subs}"


# ------------------------------------------------------------------------------------------------------------ (i) state vector
def test_state_vector_reports_a_complete_lap(torch_cuda, oracle, lib):
    """state_obs: feature 12 (tile_visited_count / T) of the lapping car is exactly 1.0 after the completing step, and the whole vector is the
    restatement's"""
    L = lib.load()
    env, run, _ = _restored(oracle, "n2", obs=False, state_obs=True)
    ended = [None] * env.B

    def chk(k, rew, done, got):
        _same_step(f"drive step {k}", rew, done, got)
        for e in np.nonzero(done)[0]:
            if ended[e] is None:
                ended[e] = k
                row = env.state[e].cpu().numpy()
                assert row[run.lap_car, 12] == np.float32(1.0)
                assert np.array_equal(row, R.of_oracle(L, run.orcs[e], run.eps[e])), f"env {e}: state vector in the completing step"
    lap_drive_phase(run, chk)
    assert all(k is not None for k in ended), ended
    env.close()


# ------------------------------------------------------------------------------------------------------------ (j) many envs at once
def test_256_envs_complete_their_lap_in_one_step(torch_cuda, oracle):
    """B = 256, N = 2, auto_reset, streams = 2: one near-complete env cloned into every slot and driven alike — 256 endings in one step (the
    re-spawn list appends, the statistics atomics), then 256 different new episodes"""
    torch = torch_cuda
    B, nS = 256, 4
    blobs = _near_complete(oracle, "n2")

    def build(b):
        env = _make("n2", B=b, auto_reset=True, streams=2); env.reset()
        env.set_state_blob(0, blobs[0])
        env.clone_envs([0] * (b - 1), list(range(1, b)))
        return env
    big, small = build(B), build(nS)
    # env g's oracle: env 0's history on its world, then g's own second episode
    runs = []
    for g in range(nS):
        run = lap_run(oracle, "n2", envs=[0]); lap_teleport_phase(run); run.to_spawn(); runs.append(run)
    st = runs[0].bodies()
    big.set_bodies(np.repeat(st, B, 0)); small.set_bodies(np.repeat(st, nS, 0))
    limit = _make("n2", B=B, auto_reset=True, streams=2, max_episode_steps=3); limit.reset()      # a TimeLimit ending of the same size
    for _ in range(3):
        _, _, d, _ = limit.step(torch.zeros((B, 2, 3), device="cuda"))
    assert bool(d.all())
    baseline = limit.status_words().copy(); limit.close()
    end = None
    for k in range(LAP_DRIVE_MAX):
        a = runs[0].drive_actions()
        at = torch.from_numpy(np.repeat(a, B, 0)).cuda()
        obs, rew, done, info = big.step(at); small.step(at[:nS].contiguous())
        rw, dn = rew.cpu().numpy(), done.cpu().numpy().astype(bool)
        stepped = [run.step(a) for run in runs]
        r, d, _ = stepped[0]
        assert all(np.array_equal(x[0], r) and np.array_equal(x[1], d) for x in stepped[1:]), f"drive step {k}: the oracle replicas disagree"
        assert (rw == rw[0]).all() and (dn == dn[0]).all(), f"drive step {k}: the clones disagree"
        assert np.array_equal(rw[0], r[0]) and dn[0] == d[0], f"drive step {k}"
        if d[0]:
            end = k; break
    assert end is not None and dn.all()
    n_ep, _ = big.rollout_stats()
    assert n_ep == B
    assert (info["episode_length"].cpu().numpy() == runs[0].steps).all()
    assert np.array_equal(big.status_words(), baseline), f"status {big.status_words().tolist()} vs a TimeLimit ending of {B} envs {baseline.tolist()}"
    # the sampled envs against their oracles: env g's second episode on env 0's world
    first = []
    for g, run in enumerate(runs):
        tr, gr = env_streams(LAP_CASES["n2"][3], g)
        oracle.new_episode(2, tr, gr, direction=run.direction, use_random_direction=False)      # g's first draw: consumed by its reset()
        run.streams[0] = (tr, gr)
        first.append(_second_episode(oracle, run, 0))
    orcs = [run.orcs[0] for run in runs]
    ob = obs[:nS].cpu().numpy()
    for g in range(nS):
        assert_frame(ob[g], first[g], orcs[g].last_amb, f"env {g}: first frame after the lap", 40)
    assert_state(big, enumerate(orcs), "the re-spawned envs")
    gen = torch.Generator(device="cuda"); gen.manual_seed(3)
    for k in range(20):
        at = torch.rand((B, 2, 3), device="cuda", generator=gen); at[..., 0] = at[..., 0] * 2 - 1; at[..., 2] *= 0.2
        o1, r1, d1, _ = big.step(at); o2, r2, d2, _ = small.step(at[:nS].contiguous())
        assert torch.equal(r1[:nS], r2) and torch.equal(d1[:nS], d2) and torch.equal(o1[:nS], o2), f"step {k} after the lap: B = {B} vs B = {nS}"
        assert not bool(d1.any())
        a = at[:nS].cpu().numpy()
        for g, o in enumerate(orcs):
            _, r, d, _ = o.step(a[g], render=False)
            assert np.array_equal(r, r1[g].cpu().numpy()), f"step {k} after the lap env {g}"
    assert_state(big, enumerate(orcs), "20 steps after the lap")
    assert np.array_equal(big.status_words(), baseline) and int(big.debug_counters()[3]) == 0
    big.close(); small.close()
