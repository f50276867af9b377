"""MI355X: action repeat inside the batched step (VecMultiCarRacing(frame_skip=k) -> include/mcr.h: mcr_step_repeat).

The contract is FrameSkip_k(TimeLimit(env)) per env with the auto-reset outside it.  The reference of every check is the CPU oracle driven the
way gym's frame-skip loop drives an env: up to k steps with the same action, `total += r`, break at done, then the next episode's reset.
An env whose episode ends in sub-step s < k - 1 must show the FIRST observation / state of its next episode, not advanced at all."""
import ctypes
import gc
import os
import warnings

import numpy as np
import pytest

from tests import state_obs_ref as R
from tests.util import Follower, assert_frame, assert_state, device_proxy_ids, drive_actions, luma_np

pytestmark = pytest.mark.gpu

K = 4


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


class _MacroFollower(Follower):
    """Follower that also keeps the episode's return"""

    def new_episode(self):
        super().new_episode()
        self.ret = np.zeros(self.N)


class _Macro:
    """what one macro-step of the followers gave: per follower the ordered f64 reward sum, done, truncated, the sub-step of the ending (-1:
    none), the episode's return and length at the ending, the last sub-step's frame (where asked for) and the sub-steps with a touching pair"""

    def __init__(self, n):
        self.reward = [None] * n
        self.done = np.zeros(n, bool); self.trunc = np.zeros(n, bool); self.end_sub = -np.ones(n, int)
        self.ep_return = [None] * n; self.ep_len = np.zeros(n, int)
        self.obs = [None] * n; self.amb = [None] * n
        self.contacts = 0


def _macro_step(O, fol, actions, k, render_last=False, threads=None):
    """gym's frame-skip loop on every follower: `for _ in range(k): obs, r, done, _ = env.step(a); total += r; if done: break`"""
    m = _Macro(len(fol))
    live = list(range(len(fol)))
    for s in range(k):
        rm = np.full(len(live), int(render_last and s == k - 1), np.uint8)
        o_obs, o_amb, o_rew, o_done = O.step_batch([fol[j].o for j in live], np.ascontiguousarray(actions[live]), rm, threads=threads or os.cpu_count() or 1)
        nxt = []
        for i, j in enumerate(live):
            f = fol[j]
            d, t = f.after_step(bool(o_done[i]))
            m.reward[j] = o_rew[i].copy() if m.reward[j] is None else m.reward[j] + o_rew[i]
            f.ret = f.ret + o_rew[i]
            m.contacts += int(f.o.num_car_contacts() > 0)
            if d:
                m.done[j], m.trunc[j], m.end_sub[j] = True, t, s
                m.ep_return[j], m.ep_len[j] = f.ret.copy(), f.steps
            else:
                nxt.append(j)
                if rm[i]:
                    m.obs[j], m.amb[j] = o_obs[i].copy(), o_amb[i].copy()
        live = nxt
        if not live:
            break
    return m


# ---------------------------------------------------------------------------------------------------------------- 1. parity with the oracle
@pytest.mark.parametrize("max_steps", [85, 86, 87, 88])
def test_macro_step_matches_the_oracles_frame_skip_loop(torch_cuda, oracle, lib, max_steps):
    """B = 4096, N = 2, frame_skip = 4, bench topology (streams = 2, async refill), RGB frames, the driving policy with pile-ups; 14 sampled envs
    against their oracles over three episodes.  The TimeLimit ends every episode in sub-step (max_steps - 1) % 4 of a macro-step: the four
    cases meet every sub-step index, and each case asserts that its own index occurred."""
    torch = torch_cuda
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    from multi_car_racing_amd._lib import McrWarning
    B, N, n_sample, seed = 4096, 2, 14, 700 + max_steps
    per_ep = (max_steps + K - 1) // K                       # macro-steps of an episode that the TimeLimit ends
    gc.collect()                                             # (one phase-word handle per device at a time: no stale ones from earlier tests)
    env = VecMultiCarRacing(B, N, seed=seed, use_random_direction=True, auto_reset=True, max_episode_steps=max_steps, car_contacts=True,
                            async_refill=True, streams=2, frame_skip=K)
    assert env.frame_skip == K
    with warnings.catch_warnings():
        warnings.simplefilter("error", McrWarning)           # (a frozen env, an overflow: the step's own warnings)
        obs = env.reset()
        idx = np.sort(np.random.RandomState(seed).choice(B, n_sample, replace=False)); idx_t = torch.from_numpy(idx).cuda()
        fol = [_MacroFollower(oracle, N, seed, int(g), max_steps) for g in idx]
        o0 = obs[idx_t].cpu().numpy()
        for j, f in enumerate(fol):
            assert_frame(o0[j], f.first_obs, f.first_amb, f"reset env {f.g}", 14)
        gen = torch.Generator(device="cuda"); gen.manual_seed(seed)
        ends = np.zeros(K, int); contacts = 0; episodes = np.zeros(n_sample, int)
        for m in range(3 * per_ep + 1):
            a = drive_actions(torch, gen, B, N, K * m, K * per_ep)
            obs, rew, done, info = env.step(a)
            check = m % 8 == 7 or m % per_ep == per_ep - 1
            a_s = a[idx_t].cpu().numpy()
            rw = rew[idx_t].cpu().numpy(); dn = done[idx_t].cpu().numpy().astype(bool); tr = info["TimeLimit.truncated"][idx_t].cpu().numpy().astype(bool)
            want = _macro_step(oracle, fol, a_s, K, render_last=check)
            contacts += want.contacts
            for j, f in enumerate(fol):
                assert np.array_equal(want.reward[j], rw[j]), f"macro-step {m} env {f.g}: reward {rw[j]} vs the ordered sum {want.reward[j]} (ending in sub-step {want.end_sub[j]})"
                assert want.done[j] == dn[j] and want.trunc[j] == tr[j], f"macro-step {m} env {f.g}: done/trunc {dn[j]}/{tr[j]} vs {want.done[j]}/{want.trunc[j]}"
            ended = np.nonzero(want.done)[0]
            got = obs[idx_t].cpu().numpy() if (check or len(ended)) else None
            if len(ended):
                er = info["episode_return"][idx_t].cpu().numpy(); el = info["episode_length"][idx_t].cpu().numpy()
            for j in ended:
                f = fol[j]
                ends[want.end_sub[j]] += 1; episodes[j] += 1
                assert np.array_equal(er[j], want.ep_return[j]) and el[j] == want.ep_len[j], f"macro-step {m} env {f.g}: episode statistics {er[j]}, {el[j]} vs {want.ep_return[j]}, {want.ep_len[j]}"
                f.new_episode()
                tid, fid = f.o.proxy_ids()
                assert np.array_equal(device_proxy_ids(env, lib, f.g), np.concatenate([tid, fid.ravel()])), f"macro-step {m} env {f.g}: proxy ids of the new episode"
                assert_frame(got[j], f.first_obs, f.first_amb, f"macro-step {m} env {f.g}: first frame after an ending in sub-step {want.end_sub[j]}", 14)
            if check:
                for j, f in enumerate(fol):
                    if not want.done[j]:
                        assert_frame(got[j], want.obs[j], want.amb[j], f"macro-step {m} env {f.g}", 14)
                assert_state(env, zip(idx, (f.o for f in fol)), f"macro-step {m}")          # (a re-spawned env: the new episode's reset state, not advanced)
        print(f"max_steps {max_steps}: endings per sub-step {ends.tolist()}, env-steps of the sample with a touching pair {contacts}")
        assert int(env.debug_counters()[3]) == 0 and env.verdict_mismatches() == 0 and env.status_words()[:5].tolist() == [0] * 5
        env.close()
    assert episodes.min() >= 3, episodes
    assert ends[(max_steps - 1) % K] >= n_sample, f"no endings in sub-step {(max_steps - 1) % K}: {ends}"
    assert contacts > 0, "the driving policy produced no car<->car contacts in the sample"


# ---------------------------------------------------------------------------------------------------------------- 2. frame_skip = 1
def test_frame_skip_1_is_the_plain_step(torch_cuda):
    torch = torch_cuda
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    B, N, seed = 64, 2, 31
    kw = dict(seed=seed, use_random_direction=True, auto_reset=True, max_episode_steps=30, car_contacts=True, async_refill=False, streams=2)
    one, plain = VecMultiCarRacing(B, N, frame_skip=1, **kw), VecMultiCarRacing(B, N, **kw)
    assert one.frame_skip == 1 and plain.frame_skip == 1
    assert torch.equal(one.reset(), plain.reset())
    gen = torch.Generator(device="cuda"); gen.manual_seed(seed)
    for k in range(300):
        a = drive_actions(torch, gen, B, N, k, 30)
        o1, r1, d1, i1 = one.step(a); o0, r0, d0, i0 = plain.step(a)
        assert torch.equal(o1, o0) and torch.equal(r1, r0) and torch.equal(d1, d0) and torch.equal(i1["TimeLimit.truncated"], i0["TimeLimit.truncated"]), f"step {k}"
    s1, s0 = one.get_state(), plain.get_state()
    e1, e0 = one.get_env_state(), plain.get_env_state()
    for k in s0:
        assert np.array_equal(s1[k], s0[k]), k
    for k in e0:
        assert np.array_equal(e1[k], e0[k]), k
    one.close(); plain.close()


# ---------------------------------------------------------------------------------------------------------------- 3. stacks of policy-step frames
def test_stack_holds_policy_step_frames(torch_cuda, oracle):
    """gray, frame_stack = 4, frame_skip = 4: FrameStack(FrameSkip(env)) — the luma of the oracle's frames at the last four macro-step boundaries,
    oldest first, outside the oracle's ambiguity masks; after an ending (TimeLimit 30: sub-step 1) the new episode's first frame four times"""
    torch = torch_cuda
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    B, N, seed, L, ks = 6, 2, 55, 30, 4
    env = VecMultiCarRacing(B, N, seed=seed, use_random_direction=True, auto_reset=True, max_episode_steps=L, car_contacts=True,
                            async_refill=False, streams=2, obs_format="gray", frame_stack=ks, frame_skip=K)
    obs = env.reset().cpu().numpy()
    assert obs.shape == (B, N, ks, 96, 96)
    fol = [_MacroFollower(oracle, N, seed, g, L) for g in range(B)]
    stacks = [[(luma_np(f.first_obs), f.first_amb.copy())] * ks for f in fol]

    def compare(got, what):
        for e in range(B):
            for i, (w, amb) in enumerate(stacks[e]):
                bad = int(((got[e, :, i] != w) & (amb == 0)).sum())
                assert bad == 0, f"{what} env {e} stack frame {i}: {bad} unambiguous pixels differ from the oracle's luma"
    compare(obs, "reset")
    rs = np.random.RandomState(seed)
    w0 = int(env.L.mcr_obs_window(env.h))
    mid_skip = 0
    for m in range(20):
        a = np.stack([rs.uniform(-1, 1, (B, N)), rs.uniform(0, 1, (B, N)), rs.uniform(0, 0.2, (B, N))], -1).astype(np.float32)
        obs, _, done, _ = env.step(torch.from_numpy(a).cuda())
        w1 = int(env.L.mcr_obs_window(env.h))
        assert w1 == w0 % ks + 1, "the ring advances once per macro-step"
        w0 = w1
        want = _macro_step(oracle, fol, a, K, render_last=True)
        assert np.array_equal(done.cpu().numpy().astype(bool), want.done), f"macro-step {m}"
        for e, f in enumerate(fol):
            if want.done[e]:
                mid_skip += int(want.end_sub[e] < K - 1)
                f.new_episode()
                stacks[e] = [(luma_np(f.first_obs), f.first_amb.copy())] * ks
            else:
                stacks[e] = stacks[e][1:] + [(luma_np(want.obs[e]), want.amb[e])]
        compare(obs.cpu().numpy(), f"macro-step {m}")
    assert mid_skip >= 2 * B, mid_skip
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 4. state vectors
def test_state_vector_once_per_macro_step(torch_cuda, oracle, lib):
    """obs = False, state_obs = True: the tensor is the restatement on the oracle's state after each macro-step; rows of envs that ended
    mid-skip (TimeLimit 38: sub-step 1) are the first state of their new episode"""
    torch = torch_cuda
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    L_ = lib.load()
    B, N, seed, limit = 64, 2, 78, 38
    env = VecMultiCarRacing(B, N, seed=seed, use_random_direction=True, auto_reset=True, max_episode_steps=limit, car_contacts=True,
                            async_refill=False, streams=2, obs=False, state_obs=True, frame_skip=K)
    env.reset()
    fol = [_MacroFollower(oracle, N, seed, g, limit, render=False) for g in range(B)]
    rs = np.random.RandomState(6)
    ended = 0
    for m in range(30):
        a = np.stack([rs.uniform(-1, 1, (B, N)), rs.uniform(0, 1, (B, N)), rs.uniform(0, 0.3, (B, N))], -1).astype(np.float32)
        _, rew, done, info = env.step(torch.from_numpy(a).cuda())
        assert info["state"] is env.state
        got = env.state.cpu().numpy(); rw = rew.cpu().numpy(); dn = done.cpu().numpy().astype(bool)
        want = _macro_step(oracle, fol, a, K)
        for g, f in enumerate(fol):
            assert np.array_equal(want.reward[g], rw[g]) and want.done[g] == dn[g], f"macro-step {m} env {g}"
            if want.done[g]:
                f.new_episode(); ended += 1
            if want.done[g] or m % 5 == 4:
                assert np.array_equal(got[g], R.of_oracle(L_, f.o, f.ep)), f"macro-step {m} env {g} (ended in sub-step {want.end_sub[g]}): state row"
    assert ended >= 2 * B
    assert env.status_words()[:5].tolist() == [0] * 5 and int(env.debug_counters()[3]) == 0
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 5. parked is not starved
@pytest.mark.parametrize("streams", [1, 2])
def test_parked_is_not_starved_and_starved_is_still_counted(torch_cuda, oracle, streams):
    """hold_refills, TimeLimit 14 (ends in sub-step 1 of every 4th macro-step).  With a staged episode the parked envs re-spawn in the same
    macro-step: no frozen env-steps, no warning.  Without one they freeze at the macro-step's last sub-step: counted, warned about; and they
    thaw — in a last sub-step, with a first observation — once the host stages again, and follow the oracle from there."""
    torch = torch_cuda
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    from multi_car_racing_amd._lib import McrWarning
    B, N, seed, L = 6, 2, 92, 14
    per_ep = (L + K - 1) // K
    env = VecMultiCarRacing(B, N, seed=seed, use_random_direction=True, auto_reset=True, max_episode_steps=L, car_contacts=True,
                            async_refill=False, streams=streams, frame_skip=K)
    env.reset()                                          # consumes episode 1 and stages episode 2
    env.hold_refills = True
    fol = [_MacroFollower(oracle, N, seed, g, L) for g in range(B)]
    rs = np.random.RandomState(4)

    def step():
        a = np.stack([rs.uniform(-1, 1, (B, N)), rs.uniform(0, 1, (B, N)), rs.uniform(0, 0.2, (B, N))], -1).astype(np.float32)
        obs, rew, done, _ = env.step(torch.from_numpy(a).cuda())
        torch.cuda.synchronize()
        return a, obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy().astype(bool)

    def follow(a, rw, dn, what):
        want = _macro_step(oracle, fol, a, K)
        for j in range(B):
            assert np.array_equal(want.reward[j], rw[j]) and want.done[j] == dn[j], f"{what} env {j}"
        return want

    with warnings.catch_warnings():
        warnings.simplefilter("error", McrWarning)
        for m in range(per_ep):                          # episode 1: ends mid-skip, parked, re-spawned from the staged episode 2
            a, obs, rw, dn = step()
            want = follow(a, rw, dn, f"episode 1 macro-step {m}")
        assert dn.all() and (want.end_sub == (L - 1) % K).all() and (L - 1) % K < K - 1
        for j, f in enumerate(fol):
            f.new_episode()
            assert_frame(obs[j], f.first_obs, f.first_amb, f"re-spawn of a parked env {j}", 14)
        assert_state(env, zip(range(B), (f.o for f in fol)), "after the re-spawn of the parked envs")
        assert int(env.debug_counters()[3]) == 0 and env.status_words()[4] == 0, "a parked env was counted as starved"
        for m in range(per_ep - 1):                      # episode 2 up to the macro-step that ends it
            a, obs, rw, dn = step()
            follow(a, rw, dn, f"episode 2 macro-step {m}")
            assert not dn.any()
    # episode 2's last macro-step: no episode 3 is staged — parked in sub-step 1, starved at the last sub-step, one counted env-step each.  The
    # kernels report that in mapped host memory, which step() reads without synchronising: the warning fires in this step() or in the next one
    with pytest.warns(McrWarning, match="froze"):
        a, obs, rw, dn = step()
        want = follow(a, rw, dn, "episode 2, last macro-step")
        assert want.done.all(), "episode 2 should end by TimeLimit"
        # (the status word is a report, not a count: reports that race may land out of order, mcr_kernels.h mcr_raise)
        assert int(env.debug_counters()[3]) == B and 0 < env.status_words()[4] <= B
        stale = obs.copy()
        for m in range(2):                               # frozen: zero reward, done 0, rows untouched, K env-steps counted per macro-step
            a, obs, rw, dn = step()
            assert (rw == 0).all() and not dn.any() and np.array_equal(obs, stale)
    assert int(env.debug_counters()[3]) == B + 2 * K * B
    env.hold_refills = False
    env._settle_staging(torch.cuda.current_stream())
    a, obs, rw, dn = step()                              # thaw: first observation of episode 3, no reward, not done, not advanced
    assert (rw == 0).all() and not dn.any()
    for j, f in enumerate(fol):
        f.new_episode()
        assert_frame(obs[j], f.first_obs, f.first_amb, f"thaw env {j}", 14)
    assert_state(env, zip(range(B), (f.o for f in fol)), "after thaw")
    for m in range(per_ep - 1):                          # and the episode continues bit-exact
        a, obs, rw, dn = step()
        follow(a, rw, dn, f"episode 3 macro-step {m}")
    assert env.verdict_mismatches() == 0
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 6. batch independence
def test_macro_step_does_not_depend_on_the_batch(torch_cuda):
    """global envs g0 .. g0 + 3 of a B = 4096 handle equal a B = 4 handle at env_offset g0 over 200 macro-steps (TimeLimit 50: endings in sub-step 1)"""
    torch = torch_cuda
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    N, seed, g0 = 2, 17, 1776
    kw = dict(seed=seed, use_random_direction=True, auto_reset=True, max_episode_steps=50, car_contacts=True, frame_skip=K)
    big = VecMultiCarRacing(4096, N, async_refill=True, streams=2, **kw)
    small = VecMultiCarRacing(4, N, env_offset=g0, async_refill=False, streams=1, **kw)
    ob, osm = big.reset(), small.reset()
    assert torch.equal(ob[g0:g0 + 4], osm)
    gen = torch.Generator(device="cuda"); gen.manual_seed(2)
    n_done = 0
    for m in range(200):
        a = drive_actions(torch, gen, 4096, N, K * m, 52)
        ob, rb, db, ib = big.step(a)
        osm, rs_, ds, is_ = small.step(a[g0:g0 + 4].contiguous())
        assert torch.equal(rb[g0:g0 + 4], rs_) and torch.equal(db[g0:g0 + 4], ds) and torch.equal(ib["TimeLimit.truncated"][g0:g0 + 4], is_["TimeLimit.truncated"]), f"macro-step {m}"
        assert torch.equal(ob[g0:g0 + 4], osm), f"macro-step {m}: frames"
        n_done += int(ds.sum().item())
    assert n_done >= 4 * 14
    sb, ss = big.get_state(), small.get_state()
    for k in ss:
        assert np.array_equal(sb[k][g0:g0 + 4], ss[k]), k
    assert int(big.debug_counters()[3]) == 0 and big.status_words()[:5].tolist() == [0] * 5
    big.close(); small.close()


# ---------------------------------------------------------------------------------------------------------------- 7. argument checks
def test_arguments(torch_cuda, lib):
    torch = torch_cuda
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    for kw in (dict(frame_skip=0), dict(frame_skip=17), dict(frame_skip=-1), dict(frame_skip=2, terminal_obs=True)):
        with pytest.raises(ValueError):
            VecMultiCarRacing(4, 2, **kw)
    ERR_ARG, ERR_STATE = -1, -3
    env = VecMultiCarRacing(4, 2, seed=1, async_refill=False, frame_skip=2)
    env.reset()
    with pytest.raises(ValueError):
        env.step(None)
    a = torch.zeros((4, 2, 3), dtype=torch.float32, device="cuda")
    L = env.L
    args = lambda act, k: (env.h, act, k, ctypes.c_void_p(env.obs.data_ptr()), ctypes.c_void_p(env.reward.data_ptr()), ctypes.c_void_p(env.done.data_ptr()), None, None)
    ap = ctypes.c_void_p(a.data_ptr())
    assert L.mcr_step_repeat(*args(None, 2)) == ERR_ARG              # repeat > 1 needs actions
    assert L.mcr_step_repeat(*args(ap, 0)) == ERR_ARG and L.mcr_step_repeat(*args(ap, 17)) == ERR_ARG and L.mcr_step_repeat(*args(ap, -3)) == ERR_ARG
    assert L.mcr_step_repeat(None, ap, 2, None, None, None, None, None) == ERR_ARG
    assert L.mcr_step_repeat(*args(ap, 16)) == 0 and L.mcr_step_repeat(*args(None, 1)) == 0      # the bounds; repeat 1 is mcr_step, action-less step included
    torch.cuda.synchronize()
    env.close()
    term = VecMultiCarRacing(4, 2, seed=1, async_refill=False, terminal_obs=True)
    term.reset()
    targs = (term.h, ap, 2, ctypes.c_void_p(term.obs.data_ptr()), ctypes.c_void_p(term.reward.data_ptr()), ctypes.c_void_p(term.done.data_ptr()), None, None)
    assert term.L.mcr_step_repeat(*targs) == ERR_STATE and b"terminal" in term.L.mcr_last_error()
    term.step(a)                                                     # repeat 1 with terminal observations: as before
    torch.cuda.synchronize()
    term.close()
    # a stacked handle: the check for d_obs is the macro-step's, and a refused macro-step leaves the ring alone
    st = VecMultiCarRacing(4, 2, seed=1, async_refill=False, obs_format="gray", frame_stack=3, frame_skip=2)
    st.reset()
    w0 = int(st.L.mcr_obs_window(st.h))
    assert st.L.mcr_step_repeat(st.h, ap, 2, None, ctypes.c_void_p(st.reward.data_ptr()), ctypes.c_void_p(st.done.data_ptr()), None, None) == ERR_ARG
    st.step(a)
    assert int(st.L.mcr_obs_window(st.h)) == w0 % 3 + 1
    st.close()
