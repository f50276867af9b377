"""MI355X: the scripted drivers (VecMultiCarRacing(scripted_agents=..., driver_params=...), csrc/k_driver.h) against their float64 restatement
(tests/driver_ref.py) on the CPU oracle's state — BIT-EXACT (np.array_equal): an action is a fixed sequence of IEEE f64 operations on state
the parity suite already holds bit-equal, rounded to f32 once.  tests/test_driver_scenario.py holds the conditions the closed loops rest on."""
import numpy as np
import pytest

from tests import driver_ref as D
from tests.util import STATE_ARRAYS, Follower, assert_state, make_env, oracle_episode, random_actions

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _rows(N):
    """parameter rows that differ per car: L1 != L2, a non-zero offset, another speed, and K_c = 0 in the last row"""
    q = D.default_params(N)
    for a in range(N):
        q[a, D.L1] = 3 + a; q[a, D.L2] = 10 + 2 * a
        q[a, D.OFFSET] = (1.5, -2.0, 0.75)[a % 3]
        q[a, D.V_MAX] = (60.0, 45.0, 70.0)[a % 3]
    q[N - 1, D.K_C] = 0.0
    return q


def _make(B, N, seed, **kw):
    return make_env(B, N, seed, **{"streams": 1, "obs": False, **kw})


def _want(L, orcs, eps, prm):
    return np.stack([D.of_oracle(L, o, ep, prm) for o, ep in zip(orcs, eps)])


def _assert_actions(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        e, a, c = bad[0]
        raise AssertionError(f"{what}: {len(bad)} action components differ, first env {e} car {a} component {c}: got {got[e, a, c]!r} want {want[e, a, c]!r}")


def _oracles(oracle, B, N, seed, **kw):
    eps = [oracle_episode(oracle, N, seed, e, **kw) for e in range(B)]
    orcs = [oracle.OracleEnv(N) for _ in range(B)]
    for o, ep in zip(orcs, eps):
        o.reset(ep, render=False)
    return orcs, eps


# ---------------------------------------------------------------------------------------------------------------- 1. bit-exact closed loop
@pytest.mark.parametrize("direction", ["CCW", "CW"])
@pytest.mark.parametrize("N", [1, 2, 3])
def test_closed_loop_bit_exact_vs_oracle(torch_cuda, oracle, lib, N, direction):
    """B = 6, every car scripted, 200 steps with the oracles in lockstep: the actions of every step equal the restatement on the oracle's
    state before the step (which the oracle is then stepped with); the state at the end is the oracle's"""
    torch = torch_cuda
    L = lib.load()
    B, seed = 6, 520 + N
    prm = _rows(N)
    env = _make(B, N, seed, direction=direction, scripted_agents=range(N), driver_params=prm)
    assert np.array_equal(env.driver_params, prm) and env.scripted_agents == tuple(range(N))
    assert env.actions.shape == (B, N, 3) and env.actions.dtype == torch.float32
    env.reset()
    orcs, eps = _oracles(oracle, B, N, seed, direction=direction)
    rng = np.random.RandomState(N)
    moved = 0.0
    for k in range(200):
        want = _want(L, orcs, eps, prm)
        ignored = torch.from_numpy(random_actions(rng, B, N)).cuda()          # every car is scripted: the caller's rows are ignored
        _, _, _, info = env.step(ignored)
        assert info["actions"] is env.actions
        _assert_actions(info["actions"].cpu().numpy(), want, f"step {k}")
        oracle.step_batch(orcs, want, None, threads=4)
        moved = max(moved, float(np.abs(want[..., 0]).max()))
    assert moved > 0.05, "the cars never steered"
    assert_state(env, enumerate(orcs), "after 200 steps")
    assert env.status_words()[:5].tolist() == [0] * 5
    env.close()
    for o in orcs:
        o.close()


# ---------------------------------------------------------------------------------------------------------------- 2. mixed cars
def test_scripted_opponent_beside_a_callers_car(torch_cuda, oracle, lib):
    """N = 2, car 1 scripted, random actions for car 0, 100 steps: car 0's rows of info["actions"] are bitwise the caller's, car 1's the
    restatement, the caller's tensor is unchanged, and reward / done / state equal those of a handle without drivers stepped with the same tensor"""
    torch = torch_cuda
    L = lib.load()
    B, N, seed = 6, 2, 531
    prm = _rows(N)
    env = _make(B, N, seed, scripted_agents=(1,), driver_params=prm)
    plain = _make(B, N, seed)
    assert plain.actions is None and plain.driver_params is None
    env.reset(); plain.reset()
    orcs, eps = _oracles(oracle, B, N, seed)
    rng = np.random.RandomState(7)
    for k in range(100):
        a = random_actions(rng, B, N, brake_scale=0.3)
        want = _want(L, orcs, eps, prm); want[:, 0] = a[:, 0]
        mine = torch.from_numpy(a).cuda(); keep = mine.clone()
        _, rew, done, info = env.step(mine)
        got = info["actions"]
        assert torch.equal(mine, keep), f"step {k}: the caller's tensor was written"
        assert torch.equal(got[:, 0].view(torch.int32), mine[:, 0].view(torch.int32)), f"step {k}: car 0's rows are not bitwise the caller's"
        _assert_actions(got.cpu().numpy(), want, f"step {k}")
        _, rew0, done0, info0 = plain.step(got.clone())
        assert "actions" not in info0
        assert torch.equal(rew, rew0) and torch.equal(done, done0), f"step {k}"
        oracle.step_batch(orcs, want, None, threads=4)
    s1, s0 = env.get_state(), plain.get_state()
    for key in STATE_ARRAYS:
        assert np.array_equal(s1[key], s0[key]), key
    e1, e0 = env.get_env_state(), plain.get_env_state()
    for key in e1:
        assert np.array_equal(e1[key], e0[key]), key
    assert_state(env, enumerate(orcs), "after 100 steps")
    env.close(); plain.close()


# ---------------------------------------------------------------------------------------------------------------- 3. auto-reset
def test_action_after_done_comes_from_the_new_episode(torch_cuda, oracle, lib):
    """B = 64, N = 2, TimeLimit 40, random direction, 100 steps with followers: every step's actions are the restatement on the followers'
    states — for an env that re-spawned in the last step that is the first state of its NEW episode"""
    torch = torch_cuda
    L = lib.load()
    B, N, seed, limit = 64, 2, 540, 40
    prm = _rows(N)
    env = _make(B, N, seed, use_random_direction=True, auto_reset=True, max_episode_steps=limit, streams=2, scripted_agents=(0, 1), driver_params=prm)
    env.reset()
    fol = [Follower(oracle, N, seed, g, limit, render=False) for g in range(B)]
    zeros = torch.zeros((B, N, 3), device="cuda")
    ended = 0; fresh = np.zeros(B, bool); checked_fresh = 0
    for k in range(100):
        want = _want(L, [f.o for f in fol], [f.ep for f in fol], prm)
        _, _, done, info = env.step(zeros)
        _assert_actions(info["actions"].cpu().numpy(), want, f"step {k}")
        checked_fresh += int(fresh.sum())
        dn = done.cpu().numpy().astype(bool)
        _, _, _, o_done = oracle.step_batch([f.o for f in fol], want, None, threads=4)
        for g, f in enumerate(fol):
            d, _ = f.after_step(bool(o_done[g]))
            assert d == dn[g], f"step {k} env {g}: done"
            fresh[g] = d
            if d:
                f.new_episode(); ended += 1
    assert ended >= 2 * B and checked_fresh >= B
    assert env.status_words()[:5].tolist() == [0] * 5 and int(env.debug_counters()[3]) == 0
    env.close()
    for f in fol:
        f.o.close()


# ---------------------------------------------------------------------------------------------------------------- 4. frame skip
def test_one_evaluation_per_macro_step(torch_cuda, oracle, lib):
    """frame_skip = 4, B = 6, N = 2, 50 macro-steps: the controller is evaluated once per step() call, from the state before the macro-step;
    the oracle's frame-skip loop holds that action for the four env steps; rewards (ordered f64 sums) and states equal the oracle's"""
    torch = torch_cuda
    L = lib.load()
    B, N, seed, K = 6, 2, 550, 4
    prm = _rows(N)
    env = _make(B, N, seed, frame_skip=K, scripted_agents=(0, 1), driver_params=prm)
    env.reset()
    orcs, eps = _oracles(oracle, B, N, seed)
    zeros = torch.zeros((B, N, 3), device="cuda")
    for m in range(50):
        want = _want(L, orcs, eps, prm)
        _, rew, done, info = env.step(zeros)
        _assert_actions(info["actions"].cpu().numpy(), want, f"macro-step {m}")
        total = None
        for s in range(K):
            _, _, r, d = oracle.step_batch(orcs, want, None, threads=4)
            assert not d.any(), "an episode ended: the scenario is meant to stay inside one"
            total = r.copy() if total is None else total + r
        assert np.array_equal(rew.cpu().numpy(), total), f"macro-step {m}: rewards"
        assert not bool(done.any())
    assert_state(env, enumerate(orcs), "after 50 macro-steps")
    assert env.status_words()[:5].tolist() == [0] * 5
    env.close()
    for o in orcs:
        o.close()


# ---------------------------------------------------------------------------------------------------------------- 5. step paths
def _crowding_policy(torch, B, N, k):
    """deterministic actions for car 0 under which the scripted car 1 meets it (measured on the oracle, seed 600, 60 steps: car<->car contacts
    in 15 of 64 envs, env 2 among them): in every 8th env car 0 pulls to one side at full throttle for 40 steps and then brakes; elsewhere it
    drives straight at half throttle — and is caught by the scripted car where it spawned in front of it"""
    a = torch.zeros((B, N, 3), device="cuda")
    a[:, 0, 1] = 0.5
    hot = (torch.arange(B, device="cuda") % 8) == 0
    if k < 40:
        a[hot, 0, 0] = 0.12; a[hot, 0, 1] = 1.0
    else:
        a[hot, 0, 1] = 0.0; a[hot, 0, 2] = 0.9
    return a


@pytest.mark.parametrize("graph", [True, False])
def test_actions_are_the_same_on_every_step_path(torch_cuda, lib, graph):
    """streams=2 (three-chain step), replayed as a graph or launched plainly, against the single-stream step at B = 64, and env g at B = 64
    against env g at B = 4: identical `actions` step by step over 60 steps of a policy that makes the cars touch"""
    torch = torch_cuda
    B, N, seed = 64, 2, 600
    kw = dict(use_random_direction=True, scripted_agents=(1,))
    multi = _make(B, N, seed, streams=2, graph=graph, **kw)
    single = _make(B, N, seed, streams=1, **kw)
    small = _make(4, N, seed, streams=1, **kw)
    assert np.array_equal(multi.driver_params, D.default_params(N))
    for e in (multi, single, small):
        e.reset()
    cnt = np.zeros(B, np.int32); contacts = 0
    for k in range(60):
        a = _crowding_policy(torch, B, N, k)
        multi.step(a); single.step(a); small.step(a[:4].contiguous())
        assert torch.equal(multi.actions, single.actions), f"step {k}"
        assert torch.equal(single.actions[:4], small.actions), f"step {k}: env g at B = 64 against env g at B = 4"
        assert torch.equal(multi.actions[:, 0], a[:, 0])
        if k % 5 == 4:
            lib.check(multi.L.mcr_debug_read_contact_counts(multi.h, lib.ptr(cnt))); contacts += int((cnt > 0).sum())
    print(f"env-steps sampled with a touching car<->car pair: {contacts}")
    assert contacts > 0, "the policy produced no car<->car contacts"
    assert bool((multi.actions[:, 1] != 0).any())
    sm, ss = multi.get_state(), single.get_state()
    for key in STATE_ARRAYS:
        assert np.array_equal(sm[key], ss[key]), key
    assert multi.status_words()[:5].tolist() == [0] * 5 and single.status_words()[:5].tolist() == [0] * 5 and multi.verdict_mismatches() == 0
    multi.close(); single.close(); small.close()


# ---------------------------------------------------------------------------------------------------------------- 6. expert_actions()
def test_expert_actions(torch_cuda, oracle, lib):
    """zeros before reset(); after reset() and after set_bodies() with shifted poses the restatement for EVERY car (scripted or not); state and
    `actions` stay as they are; a handle without driver keywords raises McrError"""
    torch = torch_cuda
    L = lib.load()
    B, N, seed = 4, 3, 560
    prm = _rows(N)
    env = _make(B, N, seed, scripted_agents=(2,), driver_params=prm)
    out = torch.full((B, N, 3), 7.0, device="cuda")
    assert env.expert_actions(out=out) is out
    assert not bool(out.any()), "rows of envs that were never reset must be zeros"
    env.reset()
    orcs, eps = _oracles(oracle, B, N, seed)
    _assert_actions(env.expert_actions().cpu().numpy(), _want(L, orcs, eps, prm), "after reset")
    rng = np.random.RandomState(3)
    for k in range(10):
        a = random_actions(rng, B, N, brake_scale=0.2)
        want = _want(L, orcs, eps, prm); a[:, 2] = want[:, 2]
        env.step(torch.from_numpy(a).cuda()); oracle.step_batch(orcs, a, None, threads=4)
    bodies = env.get_state()["bodies"].copy()
    for e in range(B):
        bodies[e, :, :, 0] += np.float32(1.5 + e); bodies[e, :, :, 1] -= np.float32(0.75); bodies[e, 1, :, 3] += np.float32(2.0)
        for c in range(N):
            for b in range(5):
                orcs[e].set_body(c, b, bodies[e, c, b])
    env.set_bodies(bodies)
    before_actions = env.actions.clone(); before_state = env.get_state()
    got = env.expert_actions()
    assert got is not env.actions and got.data_ptr() != env.actions.data_ptr()
    _assert_actions(got.cpu().numpy(), _want(L, orcs, eps, prm), "after set_bodies")
    assert torch.equal(env.actions, before_actions), "expert_actions() wrote the step's buffer"
    after = env.get_state()
    for key in STATE_ARRAYS:
        assert np.array_equal(before_state[key], after[key]), key
    with pytest.raises(ValueError):
        env.expert_actions(out=torch.zeros((B, N, 2), device="cuda"))
    env.close()
    # labels only: driver_params without scripted cars — no merged buffer, the step applies the caller's tensor
    labels = _make(B, N, seed, driver_params={})
    assert labels.actions is None and labels.scripted_agents == () and np.array_equal(labels.driver_params, D.default_params(N))
    labels.reset()
    _, _, _, info = labels.step(torch.zeros((B, N, 3), device="cuda"))
    assert "actions" not in info and bool(labels.expert_actions().any())
    labels.close()
    plain = _make(B, N, seed)
    with pytest.raises(lib.McrError):
        plain.expert_actions()
    assert L.mcr_driver_actions(plain.h, None, 0, None, None) == -3          # MCR_ERR_STATE: mcr_set_drivers was never called
    plain.close()
    for o in orcs:
        o.close()


# ---------------------------------------------------------------------------------------------------------------- 7. snapshots
def test_clones_drive_like_their_source(torch_cuda):
    """clone_envs([0] * 3, [1, 2, 3]) and one step: the clones' rows of `actions` and their next states equal the source's — nothing but
    the env's state feeds the controller"""
    torch = torch_cuda
    B, N, seed = 4, 2, 570
    env = _make(B, N, seed, scripted_agents=(0, 1), driver_params=_rows(N))
    env.reset()
    zeros = torch.zeros((B, N, 3), device="cuda")
    for k in range(30):
        env.step(zeros)
    assert not torch.equal(env.actions[0], env.actions[1])
    env.clone_envs([0] * 3, [1, 2, 3])
    env.step(zeros)
    st = env.get_state()
    for e in (1, 2, 3):
        assert torch.equal(env.actions[e], env.actions[0]), f"clone {e}: actions"
        for key in STATE_ARRAYS:
            assert np.array_equal(st[key][e], st[key][0]), f"clone {e}: {key}"
    assert bool(env.actions[0].any())
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 8. a lap on the device
def test_a_lap_on_the_device(torch_cuda):
    """the run tests/test_driver_scenario.py holds on the oracle (tests/driver_ref.py: DRIVER_LAP = seed, env, step): B = 2, N = 1, TimeLimit 1000, the car scripted with the defaults —
    `done` without `truncated` is raised for that env at exactly the recorded step, with every tile visited"""
    torch = torch_cuda
    seed, g, lap_step = D.DRIVER_LAP
    B, N = 2, 1
    assert g < B
    env = _make(B, N, seed, use_random_direction=True, max_episode_steps=D.SCENARIO_TIME_LIMIT, scripted_agents=(0,))
    env.reset()
    zeros = torch.zeros((B, N, 3), device="cuda")
    flags = torch.zeros((lap_step, 2, B), dtype=torch.uint8, device="cuda")
    for k in range(lap_step):
        _, _, done, info = env.step(zeros)
        flags[k, 0] = done; flags[k, 1] = info["TimeLimit.truncated"]
    f = flags.cpu().numpy()
    first = np.nonzero(f[:, 0, g])[0]
    assert len(first) and first[0] == lap_step - 1, f"env {g}: done first raised at steps {first[:4] + 1}, recorded {lap_step}"
    assert f[lap_step - 1, 1, g] == 0, "the lap's done is marked truncated"
    es = env.get_env_state()
    assert int(es["tile_visited_count"][g, 0]) == int(es["num_tiles"][g]) > 200
    assert env.status_words()[:5].tolist() == [0] * 5
    env.close()
