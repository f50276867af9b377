"""MI355X: the state-vector observation (VecMultiCarRacing(state_obs=True), csrc/k_stateobs.h) against its numpy restatement
(tests/state_obs_ref.py) on the CPU oracle's state — BIT-EXACT (np.array_equal): every feature is a fixed sequence of IEEE f64 operations on
state the parity suite already holds bit-equal, rounded to f32 once."""
import numpy as np
import pytest

from tests import state_obs_ref as R
from tests.util import Follower, drive_actions, make_env, oracle_episode, random_actions

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _make(B, N, seed, **kw):
    return make_env(B, N, seed, **{"streams": 1, "state_obs": True, **kw})


def _assert_rows(L, got, orcs, eps, what):
    for e, (o, ep) in enumerate(zip(orcs, eps)):
        want = R.of_oracle(L, o, ep)
        if not np.array_equal(got[e], want):
            bad = np.argwhere(got[e] != want)
            a, f = bad[0]
            raise AssertionError(f"{what} env {e}: {len(bad)} features differ, first car {a} feature {f}: got {got[e][a, f]!r} want {want[a, f]!r}")


@pytest.mark.parametrize("obs", [False, True])
@pytest.mark.parametrize("direction", ["CCW", "CW"])
@pytest.mark.parametrize("N", [1, 2, 3])
def test_state_bit_exact_vs_oracle(torch_cuda, oracle, lib, N, direction, obs):
    """B = 6, contacts on, 200 random-action steps with the oracles in lockstep: after reset and every 20th step the tensor equals the restatement."""
    torch = torch_cuda
    L = lib.load()
    B, seed = 6, 300 + N
    env = _make(B, N, seed, direction=direction, obs=obs)
    assert env.state_shape == (N, R.dim(N)) and env.state.shape == (B, N, R.dim(N)) and env.state.dtype == torch.float32
    env.reset()
    eps = [oracle_episode(oracle, N, seed, e, direction=direction) for e in range(B)]
    orcs = [oracle.OracleEnv(N) for _ in range(B)]
    for o, ep in zip(orcs, eps):
        o.reset(ep, render=False)
    _assert_rows(L, env.state.cpu().numpy(), orcs, eps, "after reset")
    rng = np.random.RandomState(10 + N)
    for k in range(200):
        a = random_actions(rng, B, N, brake_scale=0.3 if k < 150 else 1.0)
        _, rew, _, info = env.step(torch.from_numpy(a).cuda())
        assert info["state"] is env.state
        oracle.step_batch(orcs, a, None, threads=4)
        if k % 20 == 19:
            _assert_rows(L, env.state.cpu().numpy(), orcs, eps, f"step {k}")
    assert env.status_words()[:5].tolist() == [0] * 5
    env.close()
    for o in orcs:
        o.close()


def test_state_of_auto_reset_envs_is_the_new_episodes_first(torch_cuda, oracle, lib):
    """B = 64, TimeLimit 40, 100 steps: in the rows where `done` is set the state is the restatement on a fresh oracle reset of the env's NEXT
    episode; the other rows follow the running episode (checked at the end)."""
    torch = torch_cuda
    L = lib.load()
    B, N, seed, limit = 64, 2, 77, 40
    env = _make(B, N, seed, use_random_direction=True, auto_reset=True, max_episode_steps=limit, obs=False, streams=2)
    env.reset()
    fol = [Follower(oracle, N, seed, g, limit, render=False) for g in range(B)]
    _assert_rows(L, env.state.cpu().numpy(), [f.o for f in fol], [f.ep for f in fol], "after reset")
    rng = np.random.RandomState(5)
    ended = 0
    for k in range(100):
        a = random_actions(rng, B, N, brake_scale=0.3)
        _, _, done, _ = env.step(torch.from_numpy(a).cuda())
        dn = done.cpu().numpy().astype(bool); got = env.state.cpu().numpy()
        _, _, _, o_done = oracle.step_batch([f.o for f in fol], a, None, threads=4)
        for g, f in enumerate(fol):
            f.steps += 1
            d = bool(o_done[g]) or f.steps >= limit
            assert d == dn[g], f"step {k} env {g}: done"
            if d:
                f.new_episode(); ended += 1
                want = R.of_oracle(L, f.o, f.ep)
                assert np.array_equal(got[g], want), f"step {k} env {g}: the re-spawned env's row is not its new episode's first state"
    assert ended >= 2 * B
    _assert_rows(L, env.state.cpu().numpy(), [f.o for f in fol], [f.ep for f in fol], "step 99")
    assert env.status_words()[:5].tolist() == [0] * 5 and int(env.debug_counters()[3]) == 0
    env.close()


def test_state_does_not_depend_on_the_batch(torch_cuda):
    """env g at B = 64 equals env g at B = 4 after 50 steps"""
    torch = torch_cuda
    N, seed = 2, 9
    big, small = _make(64, N, seed, obs=False, streams=2), _make(4, N, seed, obs=False)
    big.reset(); small.reset()
    assert torch.equal(big.state[:4], small.state)
    rng = np.random.RandomState(1)
    for k in range(50):
        a = torch.from_numpy(random_actions(rng, 64, N, brake_scale=0.3)).cuda()
        big.step(a); small.step(a[:4].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(big.state[:4], small.state) and bool((big.state[:4] != 0).any())
    big.close(); small.close()


def test_refresh_state(torch_cuda, oracle, lib):
    """before reset() every row is zero; after set_bodies() with shifted poses refresh_state() gives the restatement on the oracle with the same set_body calls"""
    torch = torch_cuda
    L = lib.load()
    B, N, seed = 4, 2, 41
    env = _make(B, N, seed, obs=False)
    env.state.fill_(1.0)
    st = env.refresh_state(); torch.cuda.synchronize()
    assert st is env.state and not bool(st.any()), "rows of envs that were never reset must be zeros"
    env.reset()
    eps = [oracle_episode(oracle, N, seed, e) for e in range(B)]
    orcs = [oracle.OracleEnv(N) for _ in range(B)]
    for o, ep in zip(orcs, eps):
        o.reset(ep, render=False)
    rng = np.random.RandomState(2)
    for k in range(10):
        a = random_actions(rng, B, N, brake_scale=0.2)
        env.step(torch.from_numpy(a).cuda()); oracle.step_batch(orcs, a, None, threads=4)
    bodies = env.get_state()["bodies"].copy()
    for e in range(B):
        bodies[e, :, :, 0] += np.float32(1.5 + e); bodies[e, :, :, 1] -= np.float32(0.75); bodies[e, 1, :, 3] += np.float32(2.0)
        for c in range(N):
            for b in range(5):
                orcs[e].set_body(c, b, bodies[e, c, b])
    before = env.state.clone()
    env.set_bodies(bodies)
    assert torch.equal(env.state, before), "set_bodies leaves the tensor alone: refresh_state() is the caller's call"
    env.refresh_state()
    got = env.state.cpu().numpy()
    assert not np.array_equal(got, before.cpu().numpy())
    _assert_rows(L, got, orcs, eps, "after set_bodies + refresh_state")
    env.close()
    nostate = _make(B, N, seed, obs=False, state_obs=False)
    assert nostate.state is None and nostate.state_shape is None
    with pytest.raises(lib.McrError):
        nostate.refresh_state()
    assert L.mcr_state_obs_now(nostate.h, None) == -3            # MCR_ERR_STATE: no buffer set
    assert L.mcr_set_state_obs(nostate.h, None, 17, 5) == -1 and L.mcr_set_state_obs(nostate.h, None, 6, 0) == -1 and L.mcr_set_state_obs(nostate.h, None, 6, 65) == -1
    nostate.close()


def _touching_policy(torch, gen, B, N, k):
    """test_gpu_world's driving policy (the cars of an env steer into each other, then the even ones brake) in every 8th env; the others drive
    straight at half throttle.  Pile-ups in EVERY env at once are not used here: the single-stream step packs 64 / G envs on a wavefront that
    share one LDS pool of contact constraints, which then overflows (status word 2, a documented capacity deviation of that path) — and the
    single-stream handle is this test's reference."""
    a = drive_actions(torch, gen, B, N, k)
    calm = (torch.arange(B, device="cuda") % 8) != 0
    a[calm, :, 0] = 0.0; a[calm, :, 1] = 0.5; a[calm, :, 2] = 0.0
    return a


@pytest.mark.parametrize("graph", [True, False])
def test_state_is_the_same_on_every_step_path(torch_cuda, lib, graph):
    """streams=2 (three-chain step: contact chain, deferred envs, deferred flag scans), replayed as a graph or launched plainly, against the
    single-stream step: identical tensors step by step over 60 steps of a policy that makes cars touch"""
    torch = torch_cuda
    B, N, seed = 64, 2, 600
    multi = _make(B, N, seed, use_random_direction=True, obs=False, streams=2, graph=graph)
    single = _make(B, N, seed, use_random_direction=True, obs=False, streams=1)
    multi.reset(); single.reset()
    assert torch.equal(multi.state, single.state)
    gen = torch.Generator(device="cuda"); gen.manual_seed(seed)
    cnt = np.zeros(B, np.int32); contacts = 0
    for k in range(60):
        a = _touching_policy(torch, gen, B, N, k)
        multi.step(a); single.step(a)
        assert torch.equal(multi.state, single.state), f"step {k}"
        if k % 5 == 4:
            lib.check(multi.L.mcr_debug_read_contact_counts(multi.h, lib.ptr(cnt))); contacts += int((cnt > 0).sum())
    print(f"env-steps sampled with a touching car<->car pair: {contacts}; envs deferred / resumed / routed to the contact chain: {multi.debug_counters()[:3].tolist()}")
    assert contacts > 0, "the policy produced no car<->car contacts"
    assert multi.status_words()[:5].tolist() == [0] * 5 and single.status_words()[:5].tolist() == [0] * 5 and multi.verdict_mismatches() == 0
    multi.close(); single.close()


def test_state_obs_changes_nothing_else(torch_cuda):
    """reward / done / obs over 100 steps are identical with state_obs=False and state_obs=True"""
    torch = torch_cuda
    B, N, seed = 8, 2, 13
    on, off = _make(B, N, seed, obs=True, state_obs=True), _make(B, N, seed, obs=True, state_obs=False)
    assert torch.equal(on.reset(), off.reset())
    rng = np.random.RandomState(3)
    for k in range(100):
        a = torch.from_numpy(random_actions(rng, B, N, brake_scale=0.3)).cuda()
        o1, r1, d1, i1 = on.step(a); o0, r0, d0, i0 = off.step(a)
        assert "state" in i1 and "state" not in i0
        assert torch.equal(o1, o0) and torch.equal(r1, r0) and torch.equal(d1, d0), f"step {k}"
    on.close(); off.close()
