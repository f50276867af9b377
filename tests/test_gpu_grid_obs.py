"""MI355X: the grid observation (VecMultiCarRacing(grid_obs=True), csrc/k_gridobs.h) against its numpy restatement (tests/grid_obs_ref.py) on
the CPU oracle's state — BYTE-EXACT (np.array_equal): every cell is a fixed sequence of IEEE f64 operations on state the parity suite already
holds bit-equal, and on the oracle's own per-tile visit bits; the kernel's culling, its float32 prefilter and its search order must not
change a bit."""
import numpy as np
import pytest

from tests import grid_obs_ref as G
from tests import state_obs_ref as S
from tests.util import Follower, make_env, oracle_episode, oracles, random_actions

pytestmark = pytest.mark.gpu

SMALL = dict(grid_shape=(16, 16), grid_cell=3.0)        # the same 48 x 48 window in a quarter of the cells: the restatement is the slow side


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _make(B, N, seed, **kw):
    return make_env(B, N, seed, **{"streams": 1, "grid_obs": True, "obs": False, **kw})


def _geom(env):
    return env.grid_shape[1], env.grid_shape[2], env.grid_cell, env.grid_origin


def _assert_grid(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} cells differ, first at (car, row, col) {i}: got {got[i]} want {want[i]}")


def _assert_rows(L, env, orcs, eps, what):
    got = env.grid.cpu().numpy()
    for e, (o, ep) in enumerate(zip(orcs, eps)):
        _assert_grid(got[e], G.of_oracle(L, o, ep, *_geom(env)), f"{what} env {e}")


# ------------------------------------------------------------------------------------------------------------ the oracle's run, made once
_RUNS = {}
LOCKSTEP_B, LOCKSTEP_STEPS = 6, 200


def _lockstep_run(oracle, N, direction):
    """B = 6 oracles through reset and 200 random-action steps: (seed, episodes, actions [200, B, N, 3], {checkpoint: (bodies, positions,
    visited) per env}), checkpoints -1 (after reset) and every 20th step"""
    key = (N, direction)
    if key not in _RUNS:
        B, seed = LOCKSTEP_B, 400 + N
        eps = [oracle_episode(oracle, N, seed, e, direction=direction) for e in range(B)]
        orcs = [oracle.OracleEnv(N) for _ in range(B)]
        for o, ep in zip(orcs, eps):
            o.reset(ep, render=False)
        snap = lambda: [(o.state()["bodies"].copy(), o.positions().copy(), o.env_state()["visited"].copy()) for o in orcs]
        points = {-1: snap()}
        rng = np.random.RandomState(30 + N)
        actions = np.stack([random_actions(rng, B, N, brake_scale=0.3 if k < 150 else 1.0) for k in range(LOCKSTEP_STEPS)])
        for k in range(LOCKSTEP_STEPS):
            oracle.step_batch(orcs, actions[k], None, threads=4)
            if k % 20 == 19:
                points[k] = snap()
        for o in orcs:
            o.close()
        _RUNS[key] = (seed, eps, actions, points)
    return _RUNS[key]


@pytest.mark.parametrize("direction", ["CCW", "CW"])
@pytest.mark.parametrize("N", [1, 2, 3])
def test_grid_byte_exact_vs_oracle(torch_cuda, oracle, lib, N, direction):
    """B = 6, contacts on, 200 random-action steps with the oracles in lockstep: after reset and every 20th step the tensor equals the
    restatement on the oracle's bodies and visit bits"""
    torch = torch_cuda
    L = lib.load()
    seed, eps, actions, points = _lockstep_run(oracle, N, direction)
    B = LOCKSTEP_B
    env = _make(B, N, seed, direction=direction)
    assert env.grid_shape == (N, 32, 32) and env.grid.shape == (B, N, 32, 32) and env.grid.dtype == torch.uint8
    assert env.grid_cell == 1.5 and env.grid_origin == (24.0, 16.0)

    def compare(k, what):
        got = env.grid.cpu().numpy()
        for e in range(B):
            bodies, pos, visited = points[k][e]
            _assert_grid(got[e], G.grid(L, bodies, pos, eps[e]["track"], visited, *_geom(env)), f"{what} env {e}")
        return got

    env.reset()
    got = compare(-1, "after reset")
    road, fresh = (got & G.GRID_ROAD) != 0, (got & G.GRID_FRESH) != 0
    assert road.any() and (fresh <= road).all() and fresh.sum() > 0.5 * road.sum(), "a fresh episode: all but the spawn tiles is FRESH"
    assert N > 1 or not (got & G.GRID_TAKEN).any()
    planes = env.grid_planes().cpu().numpy()
    assert planes.shape == (B, N, 4, 32, 32) and planes.dtype == np.float32
    for b in range(4):
        assert np.array_equal(planes[:, :, b], ((got >> b) & 1).astype(np.float32))
    seen = 0
    for k in range(LOCKSTEP_STEPS):
        _, _, _, info = env.step(torch.from_numpy(actions[k]).cuda())
        assert info["grid"] is env.grid
        if k % 20 == 19:
            seen |= int(np.bitwise_or.reduce(compare(k, f"step {k}"), axis=None))
    need = G.GRID_ROAD | G.GRID_FRESH | (G.GRID_TAKEN if N > 1 else 0)
    assert seen & need == need and not seen & 0xf0, f"bits seen at the checkpoints: {seen:#x}"
    assert env.status_words()[:5].tolist() == [0] * 5
    env.close()


def test_grid_of_auto_reset_envs_is_the_new_episodes_first(torch_cuda, oracle, lib):
    """B = 64, TimeLimit 40, streams=2, 100 steps: in the rows where `done` is set the tensor is the restatement on a fresh oracle reset of
    the env's NEXT episode (its visit bits: the tiles the cars spawned on); all rows are checked at the end"""
    torch = torch_cuda
    L = lib.load()
    B, N, seed, limit = 64, 2, 79, 40
    env = _make(B, N, seed, use_random_direction=True, auto_reset=True, max_episode_steps=limit, streams=2, **SMALL)
    env.reset()
    fol = [Follower(oracle, N, seed, g, limit, render=False) for g in range(B)]
    _assert_rows(L, env, [f.o for f in fol], [f.ep for f in fol], "after reset")
    rng = np.random.RandomState(5)
    ended = 0
    for k in range(100):
        a = random_actions(rng, B, N, brake_scale=0.3)
        _, _, done, _ = env.step(torch.from_numpy(a).cuda())
        dn = done.cpu().numpy().astype(bool); got = env.grid.cpu().numpy()
        _, _, _, o_done = oracle.step_batch([f.o for f in fol], a, None, threads=4)
        for g, f in enumerate(fol):
            f.steps += 1
            d = bool(o_done[g]) or f.steps >= limit
            assert d == dn[g], f"step {k} env {g}: done"
            if d:
                f.new_episode(); ended += 1
                _assert_grid(got[g], G.of_oracle(L, f.o, f.ep, *_geom(env)), f"step {k} env {g}: the re-spawned env's row against its new episode's first state")
    assert ended >= 2 * B
    _assert_rows(L, env, [f.o for f in fol], [f.ep for f in fol], "step 99")
    assert env.status_words()[:5].tolist() == [0] * 5 and int(env.debug_counters()[3]) == 0
    env.close()
    for f in fol:
        f.o.close()


_TAIL_REF = {}


def _tail_reference(oracle, L, geom):
    """B = 8 followers, TimeLimit 12, reset + 30 random-action steps, made once for both cases of the test below: actions, `done` and, after
    reset (row 0) and after every step, the restatement of every env's grid — that of an env that ended in the step on its next episode"""
    if not _TAIL_REF:
        B, N, seed, limit, steps = 8, 2, 125, 12, 30
        fol = [Follower(oracle, N, seed, g, limit, render=False) for g in range(B)]
        rows = lambda: np.stack([G.of_oracle(L, f.o, f.ep, *geom) for f in fol])
        rng = np.random.RandomState(6)
        actions = np.stack([random_actions(rng, B, N, brake_scale=0.3) for _ in range(steps)])
        done, grids = np.zeros((steps, B), bool), [rows()]
        for k in range(steps):
            _, _, _, o_done = oracle.step_batch([f.o for f in fol], actions[k], None, threads=4)
            for g, f in enumerate(fol):
                f.steps += 1
                done[k, g] = bool(o_done[g]) or f.steps >= limit
                if done[k, g]:
                    f.new_episode()
            grids.append(rows())
        for f in fol:
            f.o.close()
        _TAIL_REF.update(actions=actions, done=done, grids=np.stack(grids), geom=geom)
    assert _TAIL_REF["geom"] == geom
    return _TAIL_REF


@pytest.mark.parametrize("graph", [False, True])
def test_grid_behind_a_replayed_step_graph_with_auto_reset(torch_cuda, oracle, lib, graph):
    """B = 8, N = 2, streams=2, TimeLimit 12, 30 steps, the step launched plainly or replayed from the handle's step graph: after reset and
    after EVERY step every row is the restatement — the kernel runs behind the step, outside the graph"""
    torch = torch_cuda
    L = lib.load()
    B, N = 8, 2
    env = _make(B, N, 125, use_random_direction=True, auto_reset=True, max_episode_steps=12, streams=2, graph=graph, **SMALL)
    ref = _tail_reference(oracle, L, _geom(env))
    env.reset()
    assert np.array_equal(env.grid.cpu().numpy(), ref["grids"][0]), "after reset"
    a = torch.empty((B, N, 3), dtype=torch.float32, device="cuda")       # ONE action buffer: a graph is replayed only while no argument changes
    for k in range(30):
        a.copy_(torch.from_numpy(ref["actions"][k]))
        _, _, done, _ = env.step(a)
        assert np.array_equal(done.cpu().numpy().astype(bool), ref["done"][k]), f"step {k}: done"
        got = env.grid.cpu().numpy()
        for e in range(B):
            _assert_grid(got[e], ref["grids"][k + 1, e], f"step {k} env {e}")
    assert int(ref["done"].sum()) >= 16
    assert env.status_words()[:5].tolist() == [0] * 5
    env.close()


def test_grid_once_per_macro_step(torch_cuda, oracle, lib):
    """frame_skip = 4: the tensor is the restatement on the oracle's state after each macro-step (four oracle steps with the same actions)"""
    torch = torch_cuda
    L = lib.load()
    B, N, seed, K = 6, 2, 52, 4
    env = _make(B, N, seed, frame_skip=K, **SMALL)
    env.reset()
    eps = [oracle_episode(oracle, N, seed, e) for e in range(B)]
    orcs = oracles(oracle, B, N, seed)
    rng = np.random.RandomState(8)
    for m in range(12):
        a = random_actions(rng, B, N, brake_scale=0.2)
        _, _, done, _ = env.step(torch.from_numpy(a).cuda())
        for _ in range(K):
            oracle.step_batch(orcs, a, None, threads=4)
        assert not bool(done.any())
        if m % 3 == 2:
            _assert_rows(L, env, orcs, eps, f"macro-step {m}")
    assert env.status_words()[:5].tolist() == [0] * 5
    env.close()
    for o in orcs:
        o.close()


def test_grid_of_clones_and_restored_envs(torch_cuda, oracle, lib):
    """clone_envs: the destination rows equal the source rows at once (no refresh_grid); load_states: the rows are the restatement of the
    restored state — visit bits included, which travel in the state blob"""
    torch = torch_cuda
    L = lib.load()
    B, N, seed = 8, 2, 61
    env = _make(B, N, seed, **SMALL)
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
    at_snap = env.grid.clone()
    _assert_rows(L, env, orcs, eps, "step 30")
    a = random_actions(rng, B, N, brake_scale=0.2)
    for _ in range(25):
        env.step(torch.from_numpy(a).cuda())                    # (the oracles stay at the snapshot)
    assert not torch.equal(env.grid, at_snap)
    env.grid.fill_(0xff)
    env.load_states(snap)
    assert torch.equal(env.grid, at_snap)
    steps(5)
    _assert_rows(L, env, orcs, eps, "5 steps after load_states")
    src, dst = [0, 0, 1], [5, 6, 7]
    assert not torch.equal(env.grid[dst], env.grid[src])
    env.clone_envs(src, dst)
    assert torch.equal(env.grid[dst], env.grid[src]) and bool(env.grid[dst].any())
    _assert_rows(L, env, orcs[:5], eps[:5], "after clone_envs: the other envs")
    env.close()
    for o in orcs:
        o.close()


def test_grid_beside_the_other_observations_and_scripted_agents(torch_cuda, oracle, lib):
    """state_obs, range_obs and scripted_agents=(1,) on the same handle: over 60 steps the grid stays byte-exact (the oracle is driven by
    info["actions"], what the step applied), and rewards, `done`, `state` and `ranges` equal those of a handle created without grid_obs"""
    torch = torch_cuda
    L = lib.load()
    B, N, seed = 6, 2, 88
    both = _make(B, N, seed, state_obs=True, range_obs=True, scripted_agents=(1,), **SMALL)
    plain = _make(B, N, seed, state_obs=True, range_obs=True, scripted_agents=(1,), grid_obs=False)
    both.reset(); plain.reset()
    eps = [oracle_episode(oracle, N, seed, e) for e in range(B)]
    orcs = oracles(oracle, B, N, seed)
    rng = np.random.RandomState(12)
    for k in range(60):
        a = torch.from_numpy(random_actions(rng, B, N, brake_scale=0.2)).cuda()
        _, r1, d1, info = both.step(a)
        _, r0, d0, info0 = plain.step(a)
        assert "grid" in info and "grid" not in info0
        assert torch.equal(info["state"], info0["state"]) and torch.equal(info["ranges"], info0["ranges"]) and torch.equal(r1, r0) and torch.equal(d1, d0), f"step {k}"
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


def test_refresh_grid(torch_cuda, oracle, lib):
    """before reset() every row is zero; after set_bodies() with shifted poses refresh_grid() gives the restatement on the oracle with the
    same set_body calls; a handle made without the keyword has no tensor, no info entry and refuses refresh_grid()"""
    torch = torch_cuda
    L = lib.load()
    B, N, seed = 4, 2, 41
    env = _make(B, N, seed, grid_shape=(33, 17), grid_origin=(20.3, 8.7))
    env.grid.fill_(0xff)
    t = env.refresh_grid(); torch.cuda.synchronize()
    assert t is env.grid and not bool(t.any()), "rows of envs that were never reset must be zeros"
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
        bodies[e, 1, :, 2] += np.float32(0.3)
        for c in range(N):
            for b in range(5):
                orcs[e].set_body(c, b, bodies[e, c, b])
    before = env.grid.clone()
    env.set_bodies(bodies)
    assert torch.equal(env.grid, before), "set_bodies leaves the tensor alone: refresh_grid() is the caller's call"
    env.refresh_grid()
    assert not torch.equal(env.grid, before)
    _assert_rows(L, env, orcs, eps, "after set_bodies + refresh_grid")
    env.close()
    for o in orcs:
        o.close()
    plain = _make(B, N, seed, grid_obs=False)
    assert plain.grid is None and plain.grid_shape is None and plain.grid_cell is None and plain.grid_origin is None
    with pytest.raises(lib.McrError):
        plain.refresh_grid()
    with pytest.raises(lib.McrError):
        plain.grid_planes()
    assert L.mcr_grid_obs_now(plain.h, None) == -3               # MCR_ERR_STATE: no buffer set
    plain.reset()
    _, _, _, info = plain.step(torch.zeros((B, N, 3), device="cuda"))
    assert "grid" not in info
    plain.close()
