"""MI355X: early episode ending (VecMultiCarRacing(end_patience=..., end_offroad=...) -> include/mcr.h: mcr_set_end_rules) in lockstep with
the wrapper of tests/end_rules_ref.py round the oracle: reward, done, truncated, episode_return, episode_length, end_reason and end_counters
after every step() call, the whole state at the end.  The wrapper has the same one env step of lag by definition."""
import os
import warnings

import numpy as np
import pytest

from tests import end_rules_ref as R
from tests import level_stats_ref
from tests.util import Follower, assert_state, make_env, oracles, random_actions, rear_end_setup, rigid_teleport

pytestmark = pytest.mark.gpu

FAR = 300.0


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _make(B, N, seed, **kw):
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    kw.setdefault("obs", False); kw.setdefault("async_refill", False); kw.setdefault("use_random_direction", True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                      # (a second handle of a process orders its streams with events: the same results)
        return VecMultiCarRacing(B, N, seed=seed, car_contacts=True, **kw)


class _Fol(Follower):
    """Follower with the end rules on top and the episode's return"""

    def __init__(self, O, N, seed, g, max_steps, **rules):
        self.rules = R.EndRules(N, **rules)
        super().__init__(O, N, seed, g, max_steps, render=False)

    def new_episode(self):
        super().new_episode()
        self.ret = np.zeros(self.N)
        self.rules.first_state(self.rules.read(self.o)[0])


def _rules_kw(env):
    return dict(patience=env.end_patience, offroad=env.end_offroad, mode=env.end_offroad_mode, agents=env.end_agents, end_reward=env.end_reward)


def _followers(O, env, seed, max_steps):
    return [_Fol(O, env.N, seed, g, max_steps, **_rules_kw(env)) for g in range(env.B)]


def _macro(O, fols, a, k, auto_reset):
    """one step() call of the wrapper on every follower: up to k env steps with the same actions; an auto-reset env stops at the step that ends
    its episode (parked: not live, nothing counted) and starts its next episode behind the call"""
    n = len(fols)
    reward = [None] * n; ep_return = [None] * n
    done = np.zeros(n, bool); trunc = np.zeros(n, bool); reason = np.zeros(n, np.uint8); ep_len = np.zeros(n, int); end_sub = -np.ones(n, int)
    live = list(range(n))
    for s in range(k):
        if not live:
            break
        _, _, o_rew, o_done = O.step_batch([fols[j].o for j in live], np.ascontiguousarray(a[live]), np.zeros(len(live), np.uint8), threads=min(16, os.cpu_count() or 1))
        nxt = []
        for i, j in enumerate(live):
            f = fols[j]
            d, t = f.after_step(bool(o_done[i]))
            rew, d, t, why = f.rules.end(o_rew[i].copy(), d, t)
            f.ret = f.ret + rew
            reward[j] = rew if reward[j] is None else reward[j] + rew
            reason[j] |= why
            if d:
                done[j] = True; trunc[j] |= t; ep_return[j] = f.ret.copy(); ep_len[j] = f.steps
                if end_sub[j] < 0:
                    end_sub[j] = s
            if d and auto_reset:
                f.rules.not_live()
            else:
                f.rules.advance(*f.rules.read(f.o))
                nxt.append(j)
        live = nxt
    if auto_reset:
        for j in np.nonzero(done)[0]:
            fols[j].new_episode()
    return dict(reward=reward, done=done, trunc=trunc, reason=reason, ep_return=ep_return, ep_len=ep_len, end_sub=end_sub)


def _compare(env, fols, got, want, what):
    _, rew, done, info = got
    assert info["end_reason"] is env.end_reason and env.end_reason.dtype.itemsize == 1 and tuple(env.end_counters.shape) == (env.B, 4)
    rw = rew.cpu().numpy(); dn = done.cpu().numpy().astype(bool); tr = info["TimeLimit.truncated"].cpu().numpy().astype(bool)
    why = env.end_reason.cpu().numpy(); cnt = env.end_counters.cpu().numpy(); armed = env.end_armed.cpu().numpy()
    er = info["episode_return"].cpu().numpy(); el = info["episode_length"].cpu().numpy()
    for j, f in enumerate(fols):
        w = f"{what} env {j}"
        assert np.array_equal(rw[j], want["reward"][j]), f"{w}: reward {rw[j]} vs {want['reward'][j]}"
        assert dn[j] == want["done"][j] and tr[j] == want["trunc"][j], f"{w}: done/truncated {dn[j]}/{tr[j]} vs {want['done'][j]}/{want['trunc'][j]}"
        assert why[j] == want["reason"][j], f"{w}: end_reason {why[j]} vs {want['reason'][j]}"
        assert cnt[j].tolist() == f.rules.counters.tolist(), f"{w}: end_counters {cnt[j].tolist()} vs {f.rules.counters.tolist()}"
        assert armed[j] == f.rules.armed, f"{w}: armed {armed[j]} vs {f.rules.armed}"
        if want["done"][j]:
            assert np.array_equal(er[j], want["ep_return"][j]) and el[j] == want["ep_len"][j], f"{w}: episode statistics {er[j]}, {el[j]} vs {want['ep_return'][j]}, {want['ep_len'][j]}"


def _off_road(env, fols, envs):
    """every car of the listed envs onto the grass far from every tile, on both sides"""
    st = env.get_state()["bodies"].copy()
    for e in envs:
        for c in range(env.N):
            st[e, c] = rigid_teleport(st[e, c], FAR - 14.0 * c, FAR, float(st[e, c, 0, 2]))
    env.set_bodies(st)
    for e, f in enumerate(fols):
        for c in range(env.N):
            for k in range(5):
                f.o.set_body(c, k, st[e, c, k])


# ---------------------------------------------------------------------------------------------------------------- 1. auto-reset rollouts
@pytest.mark.parametrize("N,streams,B,P,G,end_reward", [(1, 1, 5, 3, 4, 0.0), (1, 2, 66, 7, 4, -25.5), (2, 1, 5, 7, 4, -25.5), (2, 2, 67, 3, 4, 0.0),
                                                        (3, 1, 4, 3, 0, -25.5), (3, 2, 65, 7, 4, 0.0)])
def test_auto_reset_rollout_follows_the_wrapper(torch_cuda, oracle, N, streams, B, P, G, end_reward):
    """random actions, TimeLimit 23, auto_reset: at least three episodes per env.  Every third env starts its first episode on the grass (the
    off-road rule, reason 2, ahead of the idle rule where P = 7); the others end by the idle rule or the TimeLimit."""
    torch = torch_cuda
    seed, limit = 900 + 10 * N + streams, 23
    env = _make(B, N, seed, streams=streams, auto_reset=True, max_episode_steps=limit, end_patience=P, end_offroad=G, end_reward=end_reward)
    env.reset()
    fols = _followers(oracle, env, seed, limit)
    assert env.end_counters.cpu().numpy().tolist() == [f.rules.counters.tolist() for f in fols] and not env.end_armed.any() and not env.end_reason.any()
    _off_road(env, fols, range(0, B, 3))
    rng = np.random.RandomState(seed)
    episodes = np.zeros(B, int); reasons = np.zeros(4, int); forced_trunc = 0
    for k in range(3 * limit + 1):
        a = random_actions(rng, B, N, 0.3)
        got = env.step(torch.from_numpy(a).cuda())
        want = _macro(oracle, fols, a, 1, True)
        _compare(env, fols, got, want, f"step {k}")
        episodes += want["done"]
        for j in np.nonzero(want["done"])[0]:
            reasons[want["reason"][j]] += 1
            forced_trunc += int(want["reason"][j] != 0 and want["trunc"][j])
    assert_state(env, [(j, f.o) for j, f in enumerate(fols)], "end of the rollout")
    print(f"N {N} streams {streams}: endings by reason {reasons.tolist()}, forced and truncated {forced_trunc}")
    assert episodes.min() >= 3, episodes
    assert reasons[R.END_IDLE] > 0 and forced_trunc > 0
    if G and P > G:                                          # (P = 3: the idle rule ends the grass envs' first episode a step earlier)
        assert reasons[R.END_OFFROAD] + reasons[3] > 0, "the off-road rule never ended an episode"
    assert env.status_words()[:5].tolist() == [0] * 5 and env.verdict_mismatches() == 0
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 2. auto_reset off
def test_without_auto_reset_an_ended_env_stays_armed(torch_cuda, oracle):
    """zero actions, P = 3: done in step 4 (step 5 where a standing car settles onto one more tile in its first step) and in every step
    past it — until reset_envs()"""
    torch = torch_cuda
    B, N, seed = 4, 2, 41
    env = _make(B, N, seed, streams=1, auto_reset=False, max_episode_steps=0, end_patience=3, end_reward=-25.5)
    env.reset()
    fols = _followers(oracle, env, seed, 0)
    a = np.zeros((B, N, 3), np.float32)
    first_done = np.full(B, -1)
    for k in range(16):                                      # (a standing car may settle onto one more tile in its first steps: the count starts over there)
        got = env.step(torch.from_numpy(a).cuda())
        want = _macro(oracle, fols, a, 1, False)
        _compare(env, fols, got, want, f"step {k}")
        assert np.array_equal(want["reason"] != 0, want["done"]) and (want["trunc"] == want["done"]).all()
        assert not (k < 3 and want["done"].any()), f"step {k}: {want['done']}"
        assert want["done"][first_done >= 0].all(), f"step {k}: an env that ended is no longer done: {want['done']}, first endings {first_done}"
        first_done[(first_done < 0) & want["done"]] = k
        if first_done.min() >= 0 and k >= first_done.max() + 2:
            break
    assert first_done.min() >= 3 and k == first_done.max() + 2, f"every env ended and was stepped twice past its ending: {first_done}"
    # an action-less step counts nothing and ends nothing
    before = env.end_counters.clone()
    _, _, done, info_none = env.step(None)
    for f in fols:
        f.o.step(None, render=False)                         # (the followers take the action-less step too: no TimeLimit count, no rule)
    assert not done.any().item() and torch.equal(env.end_counters, before) and env.end_armed.all().item()
    assert not info_none["end_reason"].any().item() and info_none["end_reason"] is env.end_reason, "step(None) ended nothing: end_reason 0"
    got = env.step(torch.from_numpy(a).cuda())               # ... and the next step with actions ends the armed envs again, reason and all
    _compare(env, fols, got, _macro(oracle, fols, a, 1, False), "the step behind step(None)")
    assert got[2].all().item() and (env.end_reason == R.END_IDLE).all().item()
    mask = torch.zeros(B, dtype=torch.uint8, device="cuda"); mask[1] = 1
    env.reset_envs(mask)
    cnt = env.end_counters.cpu().numpy(); armed = env.end_armed.cpu().numpy()
    assert cnt[1, :2].tolist() == [0, 0] and armed.tolist() == [1, 0, 1, 1] and cnt[0].tolist() == fols[0].rules.counters.tolist() and cnt[0, 0] >= 3
    env.close()


def test_time_limit_in_the_armed_step_leaves_truncated_0(torch_cuda, oracle):
    """zero actions, P = 5, max_episode_steps = 6: the TimeLimit falls on the armed step of every env whose count ran from the first step —
    truncated = 0 with end_reason = 1 — and ends the others alone (truncated = 1, end_reason = 0)"""
    torch = torch_cuda
    B, N, seed, P = 12, 1, 47, 5
    env = _make(B, N, seed, streams=1, auto_reset=True, max_episode_steps=P + 1, end_patience=P, end_reward=-25.5)
    env.reset()
    fols = _followers(oracle, env, seed, P + 1)
    a = np.zeros((B, N, 3), np.float32)
    both = alone = 0
    for k in range(2 * (P + 1)):
        got = env.step(torch.from_numpy(a).cuda())
        want = _macro(oracle, fols, a, 1, True)
        _compare(env, fols, got, want, f"step {k}")
        assert want["done"].all() == (k % (P + 1) == P) and (want["trunc"] == (want["done"] & (want["reason"] == 0))).all()
        both += int((want["done"] & (want["reason"] != 0)).sum()); alone += int((want["done"] & (want["reason"] == 0)).sum())
    assert both > 0 and both + alone == 2 * B, (both, alone)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 3. frame_skip
@pytest.mark.parametrize("P", [4, 5, 7])
def test_frame_skip_ends_in_the_right_sub_step(torch_cuda, oracle, P):
    """frame_skip = 4, zero actions: the forced end is env step P + 1 of an episode, sub-step P % 4 of its macro-step — 0, 1 and 3 — or one
    env step later where a standing car settles onto one more tile in its first step"""
    torch = torch_cuda
    B, N, seed, K = 5, 2, 57, 4
    env = _make(B, N, seed, streams=2, auto_reset=True, max_episode_steps=0, end_patience=P, frame_skip=K, end_reward=-25.5)
    env.reset()
    fols = _followers(oracle, env, seed, 0)
    a = np.zeros((B, N, 3), np.float32)
    subs = []; episodes = np.zeros(B, int)
    for m in range(3 * ((P + 2 + K) // K) + 1):
        got = env.step(torch.from_numpy(a).cuda())
        want = _macro(oracle, fols, a, K, True)
        _compare(env, fols, got, want, f"macro-step {m}")
        subs += want["end_sub"][want["done"]].tolist(); episodes += want["done"]
        assert np.isin(want["ep_len"][want["done"]], (P + 1, P + 2)).all() and (want["reason"][want["done"]] == R.END_IDLE).all()
    assert_state(env, [(j, f.o) for j, f in enumerate(fols)], "end")
    print(f"P {P}: forced ends per sub-step {np.bincount(subs, minlength=K).tolist()}")
    assert episodes.min() >= 3 and P % K in subs and set(subs) <= {P % K, (P + 1) % K}, (episodes, subs)
    assert int(env.debug_counters()[3]) == 0 and env.status_words()[:5].tolist() == [0] * 5
    env.close()


def test_frame_skip_without_auto_reset_goes_on_past_the_ending(torch_cuda, oracle):
    """frame_skip = 4, auto_reset = False, zero actions, P = 5: nobody is parked — an env that ends in a sub-step is stepped through the
    rest of the macro-step and through the next ones, armed while its rule holds: rewards summed over all four sub-steps, done in every call"""
    torch = torch_cuda
    B, N, seed, K, P = 4, 2, 59, 4, 5
    env = _make(B, N, seed, streams=1, auto_reset=False, max_episode_steps=0, end_patience=P, frame_skip=K, end_reward=-25.5)
    env.reset()
    fols = _followers(oracle, env, seed, 0)
    a = np.zeros((B, N, 3), np.float32)
    first_done = np.full(B, -1)
    for m in range(6):
        got = env.step(torch.from_numpy(a).cuda())
        want = _macro(oracle, fols, a, K, False)
        _compare(env, fols, got, want, f"macro-step {m}")
        assert want["done"][first_done >= 0].all() and np.array_equal(want["reason"] != 0, want["done"])
        first_done[(first_done < 0) & want["done"]] = m
    assert_state(env, [(j, f.o) for j, f in enumerate(fols)], "end")
    assert first_done.min() >= 1 and first_done.max() <= 3, first_done
    assert all(int(f.steps) == 6 * K for f in fols) and (env.episode_length.cpu().numpy() == 6 * K).all(), "every env took every env step"
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 4. terminal observations
def test_every_forced_end_leaves_a_terminal_entry(torch_cuda, oracle):
    torch = torch_cuda
    B, N, seed, P = 4, 1, 63, 3
    env = _make(B, N, seed, streams=1, obs=True, auto_reset=True, max_episode_steps=0, end_patience=P, terminal_obs=True)
    env.reset()
    fols = _followers(oracle, env, seed, 0)
    a = np.zeros((B, N, 3), np.float32)
    entries = 0; ends = np.zeros(B, int)
    for k in range(2 * (P + 2) + 1):
        got = env.step(torch.from_numpy(a).cuda())
        want = _macro(oracle, fols, a, 1, True)
        _compare(env, fols, got, want, f"step {k}")
        ids, frames = env.terminal_observations()
        assert sorted(ids.cpu().numpy().tolist()) == np.nonzero(want["done"])[0].tolist(), f"step {k}"
        assert frames.shape[0] == int(want["done"].sum())
        entries += frames.shape[0]; ends += want["done"]
        assert (want["reason"][want["done"]] == R.END_IDLE).all()
    assert entries == ends.sum() and ends.min() >= 2, ends
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 5. level statistics
def test_level_stats_count_forced_ends_as_truncated(torch_cuda):
    torch = torch_cuda
    B, N, K, P = 6, 2, 4, 3
    env = _make(B, N, 77, streams=1, auto_reset=True, max_episode_steps=0, end_patience=P, levels=K, level_stats=True, end_reward=-1.0)
    env.reset()
    acc = level_stats_ref.LevelStats(K, N)
    a = torch.zeros((B, N, 3), dtype=torch.float32, device="cuda")
    forced = 0
    for k in range(3 * (P + 2)):
        before = env.level.cpu().numpy().copy()
        _, _, done, info = env.step(a)
        d = done.cpu().numpy()
        acc.step(before, d, env.truncated.cpu().numpy(), env.episode_return.cpu().numpy(), env.episode_length.cpu().numpy())
        assert np.array_equal(env.level_stats.cpu().numpy().view(np.uint64), acc.array().view(np.uint64)), f"step {k}"
        assert np.array_equal(d != 0, info["end_reason"].cpu().numpy() != 0) and np.array_equal(d, env.truncated.cpu().numpy())
        forced += int((d != 0).sum())
    s = env.level_stats.cpu().numpy()
    assert forced >= 3 * B and s[:, 0].sum() == forced and s[:, 1].sum() == forced, "every ending was a forced one and counts as truncated"
    assert (s[:, 2] >= (P + 1) * s[:, 0]).all() and (s[:, 2] <= (P + 2) * s[:, 0]).all()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 6. the contact chain
def test_forced_end_of_a_touching_pair(torch_cuda, oracle):
    """the rear-end run (car 1 floors it into the braking car 0; touching from step 3 on) with the braking car counted alone: P = 7 ends the
    episode in step 8, while the env holds a touching pair and — B = 67, two streams — runs in the contact chain"""
    torch = torch_cuda
    B, N, seed, P = 67, 2, 62, 7
    env = _make(B, N, seed, streams=2, auto_reset=True, max_episode_steps=0, use_random_direction=False, end_patience=P, end_agents=(0,), end_reward=-25.5)
    env.reset()
    fols = [_fol_fixed(oracle, N, seed, g, env) for g in range(B)]
    rear_end_setup(env, [f.o for f in fols])
    rng = np.random.RandomState(4)
    touching_ends = 0
    for k in range(2 * P + 4):
        a = random_actions(rng, B, 2, 0.0)
        a[:, 0, 1] = 0.0; a[:, 0, 2] = 0.8; a[:, 1, 0] *= 0.2; a[:, 1, 1] = 1.0
        got = env.step(torch.from_numpy(a).cuda())
        touching = np.array([f.o.num_car_contacts() > 0 for f in fols])          # (as of the step before: who is in the contact chain now)
        want = _macro(oracle, fols, a, 1, True)
        _compare(env, fols, got, want, f"step {k}")
        touching_ends += int((want["done"] & (want["reason"] != 0) & touching).sum())
    assert_state(env, [(j, f.o) for j, f in enumerate(fols)], "end")
    assert touching_ends >= B // 2, f"only {touching_ends} forced ends fell on an env with a touching pair"
    assert env.status_words()[:5].tolist() == [0] * 5 and env.verdict_mismatches() == 0
    env.close()


def _fol_fixed(O, N, seed, g, env):
    """a follower of an env created with use_random_direction=False"""
    f = _Fol.__new__(_Fol)
    f.rules = R.EndRules(N, **_rules_kw(env))
    Follower.__init__(f, O, N, seed, g, 0, use_random_direction=False, render=False)
    return f


# ---------------------------------------------------------------------------------------------------------------- 7. a scripted opponent
def test_learner_counted_scripted_car_not(torch_cuda, oracle):
    """scripted_agents = (1,), end_agents = (0,): the learner idles and ends the episode at step P + 1 although the scripted car keeps visiting
    tiles (P + 2 where the standing learner settles onto one more tile in its first step); the oracle is driven by the actions the step applied (info["actions"])"""
    torch = torch_cuda
    B, N, seed, P = 4, 2, 83, 7
    env = _make(B, N, seed, streams=1, auto_reset=True, max_episode_steps=0, end_patience=P, end_agents=(0,), scripted_agents=(1,))
    env.reset()
    fols = _followers(oracle, env, seed, 0)
    mine = torch.zeros((B, N, 3), dtype=torch.float32, device="cuda")
    ends = 0; moved = False
    for k in range(2 * (P + 2)):
        got = env.step(mine)
        a = got[3]["actions"].cpu().numpy()
        assert (a[:, 0] == 0).all()
        moved = moved or bool((a[:, 1, 1] > 0).any())
        want = _macro(oracle, fols, a, 1, True)
        _compare(env, fols, got, want, f"step {k}")
        ends += int(want["done"].sum())
        assert np.isin(want["ep_len"][want["done"]], (P + 1, P + 2)).all() and (want["reason"][want["done"]] == R.END_IDLE).all()
    assert ends >= 2 * B and moved
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 8. clones and snapshots
def test_clone_of_an_env_one_step_short_of_arming(torch_cuda):
    torch = torch_cuda
    B, N, P = 4, 1, 5
    env = _make(B, N, 29, streams=1, auto_reset=False, max_episode_steps=0, end_patience=P)
    env.reset()
    a = torch.zeros((B, N, 3), dtype=torch.float32, device="cuda")
    for _ in range(P + 1):                                    # until env 0 is one step short of arming
        env.step(a)
        if int(env.end_counters[0, 0].item()) == P - 1:
            break
    assert int(env.end_counters[0, 0].item()) == P - 1 and int(env.end_armed[0].item()) == 0
    env.end_counters[2:] = 0                                   # the destinations' own history: gone with the clone
    env.end_counters[2:, 2] = -5
    env.clone_envs([0, 0], [2, 3])
    assert torch.equal(env.end_counters[2], env.end_counters[0]) and torch.equal(env.end_counters[3], env.end_counters[0])
    assert env.end_armed.cpu().numpy()[[0, 2, 3]].tolist() == [0, 0, 0]
    _, _, done, _ = env.step(a)
    assert not done.cpu().numpy()[[0, 2, 3]].any() and env.end_armed.cpu().numpy()[[0, 2, 3]].tolist() == [1, 1, 1]
    _, rew, done, info = env.step(a)
    assert done.cpu().numpy()[[0, 2, 3]].all() and info["end_reason"].cpu().numpy()[[0, 2, 3]].tolist() == [1, 1, 1]
    assert torch.equal(rew[2], rew[0]) and torch.equal(rew[3], rew[0])
    env.close()


def test_restore_with_saved_counters_continues_bit_identically(torch_cuda):
    torch = torch_cuda
    B, N, P = 5, 2, 7
    env = _make(B, N, 35, streams=1, auto_reset=False, max_episode_steps=0, end_patience=P, end_offroad=9, end_offroad_mode="any", end_reward=-3.25)
    env.reset()
    rng = np.random.RandomState(8)
    acts = [torch.from_numpy(random_actions(rng, B, N, 0.3)).cuda() * (0.0 if k % 12 < 9 else 1.0) for k in range(5 + 14)]

    def run(ks):
        rec = []
        for k in ks:
            _, rew, done, info = env.step(acts[k])
            rec.append([t.clone() for t in (rew, done, info["TimeLimit.truncated"], info["end_reason"], env.end_counters, env.end_armed,
                                              info["episode_return"] * done[:, None], info["episode_length"] * done)])      # (the statistics rows are valid where done is set)
        return rec
    run(range(5))
    blobs, counters = env.save_states(), env.end_counters.clone()
    assert (counters[:, 0] > 0).any().item()
    first = run(range(5, 19))
    assert any(r[1].any().item() for r in first), "nothing ended in the recorded stretch"
    s0 = env.get_state()
    env.end_counters.copy_(counters)                           # the caller's rows, in front of the restore whose settle pass reads them
    env.load_states(blobs)
    second = run(range(5, 19))
    for k, (x, y) in enumerate(zip(first, second)):
        for i, (p, q) in enumerate(zip(x, y)):
            assert torch.equal(p, q), f"step {5 + k}: output {i} differs after the restore"
    s1 = env.get_state()
    for key in s0:
        assert np.array_equal(s0[key], s1[key]), key
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 9. off changes nothing
def test_defaults_leave_the_plain_step_alone(torch_cuda, oracle):
    """every end_* keyword at its default: no tensors, no info entry, and the rollout is the oracle's, as before the feature"""
    torch = torch_cuda
    B, N, seed = 6, 2, 19
    env = make_env(B, N, seed, streams=2)
    assert env.end_counters is None and env.end_reason is None and env.end_patience == 0 and env.end_offroad == 0
    with pytest.raises(Exception, match="end_patience"):
        env.refresh_end_rules()
    env.reset()
    orcs = oracles(oracle, B, N, seed)
    rng = np.random.RandomState(3)
    for k in range(30):
        a = random_actions(rng, B, N, 0.3)
        _, rew, done, info = env.step(torch.from_numpy(a).cuda())
        assert "end_reason" not in info
        rw = rew.cpu().numpy(); dn = done.cpu().numpy()
        for e, o in enumerate(orcs):
            _, r, d, _ = o.step(a[e], render=False)
            assert np.array_equal(r, rw[e]) and bool(d) == bool(dn[e]), f"step {k} env {e}"
    assert_state(env, list(enumerate(orcs)), "defaults")
    env.close()
