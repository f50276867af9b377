"""MI355X: the range-finder observation (VecMultiCarRacing(range_obs=True), csrc/k_rangeobs.h) against its numpy restatement
(tests/range_obs_ref.py) on the CPU oracle's state — BIT-EXACT (np.array_equal): every range is a fixed sequence of IEEE f64 operations on
state the parity suite already holds bit-equal, rounded to f32 once; the kernel's pre-test, its culling and its reduction order must not
change a bit."""
import math

import numpy as np
import pytest

from tests import range_obs_ref as R
from tests import state_obs_ref as S
from tests.util import Follower, make_env, oracle_episode, oracles, random_actions

pytestmark = pytest.mark.gpu

FULL_CIRCLE = tuple(np.linspace(-math.pi, math.pi, 24, endpoint=False).tolist())


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _make(B, N, seed, **kw):
    return make_env(B, N, seed, **{"streams": 1, "range_obs": True, "obs": False, **kw})


def _assert_ranges(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} ranges differ, first at (car, channel, ray) {i}: got {got[i]!r} want {want[i]!r}")


def _assert_rows(L, env, orcs, eps, what):
    got = env.ranges.cpu().numpy()
    for e, (o, ep) in enumerate(zip(orcs, eps)):
        _assert_ranges(got[e], R.of_oracle(L, o, ep, env.range_dirs, env.range_max), f"{what} env {e}")


# ------------------------------------------------------------------------------------------------------------ the oracle's run, made once
_RUNS = {}
LOCKSTEP_B, LOCKSTEP_STEPS = 6, 200


def _lockstep_run(oracle, N, direction):
    """B = 6 oracles through reset and 200 random-action steps: (seed, episodes, actions [200, B, N, 3], {checkpoint: (bodies [B], positions [B])}),
    checkpoints -1 (after reset) and every 20th step — shared by every (rays, max_range) case of the same (N, direction)"""
    key = (N, direction)
    if key not in _RUNS:
        B, seed = LOCKSTEP_B, 300 + N
        eps = [oracle_episode(oracle, N, seed, e, direction=direction) for e in range(B)]
        orcs = [oracle.OracleEnv(N) for _ in range(B)]
        for o, ep in zip(orcs, eps):
            o.reset(ep, render=False)
        snap = lambda: ([o.state()["bodies"].copy() for o in orcs], [o.positions().copy() for o in orcs])
        points = {-1: snap()}
        rng = np.random.RandomState(10 + N)
        actions = np.stack([random_actions(rng, B, N, brake_scale=0.3 if k < 150 else 1.0) for k in range(LOCKSTEP_STEPS)])
        for k in range(LOCKSTEP_STEPS):
            oracle.step_batch(orcs, actions[k], None, threads=4)
            if k % 20 == 19:
                points[k] = snap()
        for o in orcs:
            o.close()
        _RUNS[key] = (seed, eps, actions, points)
    return _RUNS[key]


def _lockstep(torch, oracle, lib, N, direction, **kw):
    L = lib.load()
    seed, eps, actions, points = _lockstep_run(oracle, N, direction)
    B = LOCKSTEP_B
    env = _make(B, N, seed, direction=direction, **kw)
    Rn = len(env.range_angles)
    assert env.range_shape == (N, 2, Rn) and env.ranges.shape == (B, N, 2, Rn) and env.ranges.dtype == torch.float32
    assert env.range_dirs.shape == (Rn, 2) and env.range_dirs.dtype == np.float32

    def compare(k, what):
        got = env.ranges.cpu().numpy()
        bodies, pos = points[k]
        for e in range(B):
            want = R.ranges(L, bodies[e], pos[e], eps[e]["track"], env.range_dirs, env.range_max)
            _assert_ranges(got[e], want, f"{what} env {e}")
        return got

    env.reset()
    got = compare(-1, "after reset")              # the cars sit at tile 0: the wrap segments T-1 -> 0 are the nearest ones
    assert (got[:, :, 0] > 0).all() and (got <= np.float32(env.range_max)).all()
    if N == 1:
        assert (got[:, :, 1] == np.float32(env.range_max)).all()
    for k in range(LOCKSTEP_STEPS):
        _, _, _, info = env.step(torch.from_numpy(actions[k]).cuda())
        assert info["ranges"] is env.ranges
        if k % 20 == 19:
            compare(k, f"step {k}")
    assert env.status_words()[:5].tolist() == [0] * 5
    env.close()


@pytest.mark.parametrize("rays,max_range", [(1, 100.0), (19, 25.0), (32, 400.0)])
@pytest.mark.parametrize("direction", ["CCW", "CW"])
@pytest.mark.parametrize("N", [1, 2, 3])
def test_ranges_bit_exact_vs_oracle(torch_cuda, oracle, lib, N, direction, rays, max_range):
    """B = 6, contacts on, 200 random-action steps with the oracles in lockstep: after reset and every 20th step the tensor equals the
    restatement.  max_range 25 culls most of the track and clamps most rays; 400 reaches the whole track."""
    _lockstep(torch_cuda, oracle, lib, N, direction, range_rays=rays, range_max=max_range)


def test_ranges_full_circle_bit_exact_vs_oracle(torch_cuda, oracle, lib):
    """the same run with explicit angles all around the car (rays that look backwards and at the opponent behind)"""
    _lockstep(torch_cuda, oracle, lib, 2, "CCW", range_angles=FULL_CIRCLE, range_max=100.0)


def test_ranges_of_auto_reset_envs_are_the_new_episodes_first(torch_cuda, oracle, lib):
    """B = 64, TimeLimit 40, 100 steps: in the rows where `done` is set the tensor is the restatement on a fresh oracle reset of the env's NEXT
    episode; the other rows follow the running episode (all rows checked at the end)."""
    torch = torch_cuda
    L = lib.load()
    B, N, seed, limit = 64, 2, 77, 40
    env = _make(B, N, seed, use_random_direction=True, auto_reset=True, max_episode_steps=limit, streams=2)
    env.reset()
    fol = [Follower(oracle, N, seed, g, limit, render=False) for g in range(B)]
    _assert_rows(L, env, [f.o for f in fol], [f.ep for f in fol], "after reset")
    rng = np.random.RandomState(5)
    ended = 0
    for k in range(100):
        a = random_actions(rng, B, N, brake_scale=0.3)
        _, _, done, _ = env.step(torch.from_numpy(a).cuda())
        dn = done.cpu().numpy().astype(bool); got = env.ranges.cpu().numpy()
        _, _, _, o_done = oracle.step_batch([f.o for f in fol], a, None, threads=4)
        for g, f in enumerate(fol):
            f.steps += 1
            d = bool(o_done[g]) or f.steps >= limit
            assert d == dn[g], f"step {k} env {g}: done"
            if d:
                f.new_episode(); ended += 1
                _assert_ranges(got[g], R.of_oracle(L, f.o, f.ep, env.range_dirs, env.range_max), f"step {k} env {g}: the re-spawned env's row against its new episode's first state")
    assert ended >= 2 * B
    _assert_rows(L, env, [f.o for f in fol], [f.ep for f in fol], "step 99")
    assert env.status_words()[:5].tolist() == [0] * 5 and int(env.debug_counters()[3]) == 0
    env.close()
    for f in fol:
        f.o.close()


_TAIL_REF = {}


def _tail_reference(oracle, L, dirs, max_range):
    """B = 8 followers, TimeLimit 12, reset + 30 random-action steps, made once for both cases of the test below: the actions [30, B, N, 3],
    `done` [30, B] and, after reset (row 0) and after every step, the restatements of every env's ranges and state rows — those of an env
    that ended in the step on the fresh reset of its next episode"""
    if not _TAIL_REF:
        B, N, seed, limit, steps = 8, 2, 123, 12, 30
        fol = [Follower(oracle, N, seed, g, limit, render=False) for g in range(B)]
        rows = lambda: (np.stack([R.of_oracle(L, f.o, f.ep, dirs, max_range) for f in fol]), np.stack([S.of_oracle(L, f.o, f.ep) for f in fol]))
        rng = np.random.RandomState(6)
        actions = np.stack([random_actions(rng, B, N, brake_scale=0.3) for _ in range(steps)])
        done, ranges, state = np.zeros((steps, B), bool), [None] * (steps + 1), [None] * (steps + 1)
        ranges[0], state[0] = rows()
        for k in range(steps):
            _, _, _, o_done = oracle.step_batch([f.o for f in fol], actions[k], None, threads=4)
            for g, f in enumerate(fol):
                f.steps += 1
                done[k, g] = bool(o_done[g]) or f.steps >= limit
                if done[k, g]:
                    f.new_episode()
            ranges[k + 1], state[k + 1] = rows()
        for f in fol:
            f.o.close()
        _TAIL_REF.update(seed=seed, limit=limit, actions=actions, done=done, ranges=np.stack(ranges), state=np.stack(state), dirs=np.array(dirs), max_range=max_range)
    assert np.array_equal(_TAIL_REF["dirs"], dirs) and _TAIL_REF["max_range"] == max_range
    return _TAIL_REF


@pytest.mark.parametrize("graph", [False, True])
def test_ranges_and_state_behind_a_replayed_step_graph_with_auto_reset(torch_cuda, oracle, lib, graph):
    """B = 8, N = 2, streams=2, TimeLimit 12, 30 steps, the step launched plainly or replayed from the handle's step graph (the replay-hit
    branch from the third step on, once both parities are captured): after reset and after EVERY step every row of `ranges` and of `state`
    is the restatement on the oracle — for an env whose `done` is set, on the fresh reset of its next episode.  `done` agrees with the
    followers every step and every env ends twice at the limit, so the re-spawned rows are really compared."""
    torch = torch_cuda
    L = lib.load()
    B, N = 8, 2
    env = _make(B, N, 123, use_random_direction=True, auto_reset=True, max_episode_steps=12, streams=2, state_obs=True, graph=graph)
    ref = _tail_reference(oracle, L, env.range_dirs, env.range_max)       # (the handle's ray table: the same for both cases, checked there)
    assert (ref["seed"], ref["limit"]) == (123, 12)

    def compare(row, what):
        got_r, got_s = env.ranges.cpu().numpy(), env.state.cpu().numpy()
        for e in range(B):
            _assert_ranges(got_r[e], ref["ranges"][row, e], f"{what} env {e}")
            assert np.array_equal(got_s[e], ref["state"][row, e]), f"{what} env {e}: state row"

    env.reset()
    compare(0, "after reset")
    a = torch.empty((B, N, 3), dtype=torch.float32, device="cuda")       # ONE action buffer: a graph is replayed only while no argument changes
    for k in range(30):
        a.copy_(torch.from_numpy(ref["actions"][k]))
        _, _, done, _ = env.step(a)
        assert np.array_equal(done.cpu().numpy().astype(bool), ref["done"][k]), f"step {k}: done"
        compare(k + 1, f"step {k}")
    assert int(ref["done"].sum()) >= 16
    assert env.status_words()[:5].tolist() == [0] * 5
    env.close()


def test_ranges_do_not_depend_on_the_batch(torch_cuda):
    """env g at B = 64 equals env g at B = 4 after 50 steps, and is non-zero"""
    torch = torch_cuda
    N, seed = 2, 9
    big, small = _make(64, N, seed, streams=2), _make(4, N, seed)
    big.reset(); small.reset()
    assert torch.equal(big.ranges[:4], small.ranges)
    rng = np.random.RandomState(1)
    for k in range(50):
        a = torch.from_numpy(random_actions(rng, 64, N, brake_scale=0.3)).cuda()
        big.step(a); small.step(a[:4].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(big.ranges[:4], small.ranges) and bool((big.ranges[:4] != 0).all())
    big.close(); small.close()


def test_refresh_ranges(torch_cuda, oracle, lib):
    """before reset() every row is zero; after set_bodies() with shifted poses refresh_ranges() gives the restatement on the oracle with the
    same set_body calls; a handle made without the keyword has no tensor, no info entry and refuses refresh_ranges()"""
    torch = torch_cuda
    L = lib.load()
    B, N, seed = 4, 2, 41
    env = _make(B, N, seed)
    env.ranges.fill_(1.0)
    t = env.refresh_ranges(); torch.cuda.synchronize()
    assert t is env.ranges and not bool(t.any()), "rows of envs that were never reset must be zeros"
    env.reset()
    eps = [oracle_episode(oracle, N, seed, e) for e in range(B)]
    orcs = oracles(oracle, B, N, seed)
    rng = np.random.RandomState(2)
    for k in range(10):
        a = random_actions(rng, B, N, brake_scale=0.2)
        env.step(torch.from_numpy(a).cuda()); oracle.step_batch(orcs, a, None, threads=4)
    bodies = env.get_state()["bodies"].copy()
    for e in range(B):
        bodies[e, :, :, 0] += np.float32(1.5 + e); bodies[e, :, :, 1] -= np.float32(0.75)
        bodies[e, 1, :, 2] += np.float32(0.3)                  # (every body of car 1 by the same angle about its own centre: the hull's heading turns)
        for c in range(N):
            for b in range(5):
                orcs[e].set_body(c, b, bodies[e, c, b])
    before = env.ranges.clone()
    env.set_bodies(bodies)
    assert torch.equal(env.ranges, before), "set_bodies leaves the tensor alone: refresh_ranges() is the caller's call"
    env.refresh_ranges()
    assert not torch.equal(env.ranges, before)
    _assert_rows(L, env, orcs, eps, "after set_bodies + refresh_ranges")
    env.close()
    for o in orcs:
        o.close()
    plain = _make(B, N, seed, range_obs=False)
    assert plain.ranges is None and plain.range_shape is None and plain.range_dirs is None
    with pytest.raises(lib.McrError):
        plain.refresh_ranges()
    assert L.mcr_range_obs_now(plain.h, None) == -3              # MCR_ERR_STATE: no buffer set
    plain.reset()
    _, _, _, info = plain.step(torch.zeros((B, N, 3), device="cuda"))
    assert "ranges" not in info
    plain.close()


def test_ranges_once_per_macro_step(torch_cuda, oracle, lib):
    """frame_skip = 4: the tensor is the restatement on the oracle's state after each macro-step (four oracle steps with the same actions)"""
    torch = torch_cuda
    L = lib.load()
    B, N, seed, K = 6, 2, 52, 4
    env = _make(B, N, seed, frame_skip=K)
    env.reset()
    eps = [oracle_episode(oracle, N, seed, e) for e in range(B)]
    orcs = oracles(oracle, B, N, seed)
    rng = np.random.RandomState(8)
    for m in range(12):
        a = random_actions(rng, B, N, brake_scale=0.2)
        _, _, done, info = env.step(torch.from_numpy(a).cuda())
        for _ in range(K):
            oracle.step_batch(orcs, a, None, threads=4)
        assert not bool(done.any())
        if m % 3 == 2:
            _assert_rows(L, env, orcs, eps, f"macro-step {m}")
    assert env.status_words()[:5].tolist() == [0] * 5
    env.close()
    for o in orcs:
        o.close()


def test_ranges_of_clones_and_restored_envs(torch_cuda, oracle, lib):
    """clone_envs: the destination rows equal the source rows at once (no refresh_ranges); load_states: the rows are the restatement of the
    restored state"""
    torch = torch_cuda
    L = lib.load()
    B, N, seed = 8, 2, 61
    env = _make(B, N, seed)
    env.reset()
    eps = [oracle_episode(oracle, N, seed, e) for e in range(B)]
    orcs = oracles(oracle, B, N, seed)
    rng = np.random.RandomState(4)

    def steps(n):
        for _ in range(n):
            a = random_actions(rng, B, N, brake_scale=0.2)
            env.step(torch.from_numpy(a).cuda()); oracle.step_batch(orcs, a, None, threads=4)

    steps(30)
    snap = env.save_states()
    at_snap = env.ranges.clone()
    _assert_rows(L, env, orcs, eps, "step 30")
    a = random_actions(rng, B, N, brake_scale=0.2)
    for _ in range(25):
        env.step(torch.from_numpy(a).cuda())                    # (the oracles stay at the snapshot)
    assert not torch.equal(env.ranges, at_snap)
    env.ranges.fill_(-1.0)
    env.load_states(snap)
    assert torch.equal(env.ranges, at_snap)
    _assert_rows(L, env, orcs, eps, "after load_states")
    steps(5)
    _assert_rows(L, env, orcs, eps, "5 steps after load_states")
    src, dst = [0, 0, 1], [5, 6, 7]
    assert not torch.equal(env.ranges[dst], env.ranges[src])
    env.clone_envs(src, dst)
    assert torch.equal(env.ranges[dst], env.ranges[src]) and bool((env.ranges[dst] != 0).all())
    _assert_rows(L, env, orcs[:5], eps[:5], "after clone_envs: the other envs")
    env.close()
    for o in orcs:
        o.close()


def test_ranges_beside_state_obs_and_scripted_agents(torch_cuda, oracle, lib):
    """state_obs=True and scripted_agents=(1,) on the same handle: over 60 steps both tensors stay bit-exact (the oracle is driven by
    info["actions"], what the step applied), and `state` equals that of a handle created without range_obs"""
    torch = torch_cuda
    L = lib.load()
    B, N, seed = 6, 2, 88
    both = _make(B, N, seed, state_obs=True, scripted_agents=(1,))
    plain = _make(B, N, seed, state_obs=True, scripted_agents=(1,), range_obs=False)
    both.reset(); plain.reset()
    eps = [oracle_episode(oracle, N, seed, e) for e in range(B)]
    orcs = oracles(oracle, B, N, seed)
    rng = np.random.RandomState(12)
    for k in range(60):
        a = torch.from_numpy(random_actions(rng, B, N, brake_scale=0.2)).cuda()
        _, r1, d1, info = both.step(a)
        _, r0, d0, info0 = plain.step(a)
        assert "ranges" in info and "ranges" not in info0
        assert torch.equal(info["state"], info0["state"]) and torch.equal(r1, r0) and torch.equal(d1, d0), f"step {k}"
        oracle.step_batch(orcs, info["actions"].cpu().numpy(), None, threads=4)
        if k % 10 == 9:
            _assert_rows(L, both, orcs, eps, f"step {k}")
            st = both.state.cpu().numpy()
            for e, (o, ep) in enumerate(zip(orcs, eps)):
                assert np.array_equal(st[e], S.of_oracle(L, o, ep)), f"step {k} env {e}: state row"
    assert both.status_words()[:5].tolist() == [0] * 5
    both.close(); plain.close()
    for o in orcs:
        o.close()
