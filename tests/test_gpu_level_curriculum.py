"""MI355X: level curricula — per-level episode statistics (VecMultiCarRacing(level_stats=True), csrc/k_levelstats.h) against the host
accumulator of tests/level_stats_ref.py, bit for bit, and weighted level sampling (level_order="weighted", csrc/k_pool.h) against a
host-staged control (the construction of tests/test_gpu_level_pool.py: a handle without `levels`, async_refill=False, whose `_generate`
hands out the pool rows the definition prescribes).

TimeLimit 7 throughout: the envs end in phase, so many envs add to the same stats row in the same step — where the order of the additions
shows in the last bits.  (test_stats_with_staggered_endings_at_B_2118 puts them out of phase on purpose; the kernel alone, on synthetic rows
at every batch size and ending pattern: tests/test_gpu_level_stats_kernel.py.)"""
import ctypes

import numpy as np
import pytest

from tests import level_stats_ref as ref
from tests.util import random_actions

pytestmark = pytest.mark.gpu

MCR_OK, MCR_ERR_ARG, MCR_ERR_STATE = 0, -1, -3
SEED = 23


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


_POOLS = {}


def _pool(N, K=3):
    """the K levels every test here plays (generated once per N; read-only)"""
    if (N, K) not in _POOLS:
        from multi_car_racing_amd.levels import make_levels
        blobs, info = make_levels(K, N, SEED, 2)
        blobs.setflags(write=False); info.setflags(write=False)
        _POOLS[(N, K)] = (blobs, info)
    return _POOLS[(N, K)]


def _env(B, N, K=3, **kw):
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    kw.setdefault("streams", 1); kw.setdefault("max_episode_steps", 7); kw.setdefault("seed", SEED)
    return VecMultiCarRacing(B, N, levels=np.array(_pool(N, K)[0]), **kw)


def _bits(t):
    return t.cpu().numpy().view(np.uint64)


def _act(torch, env, rng):
    return torch.from_numpy(random_actions(rng, env.B, env.N, 0.2)).to(env.device)


class _Tracked:
    """an env with level_stats=True and the host accumulator fed with its per-step host copies; step() compares after every step"""

    def __init__(self, torch, env, rng_seed=3):
        self.torch, self.env, self.rng = torch, env, np.random.RandomState(rng_seed)
        self.acc = ref.LevelStats(env.num_levels, env.N)
        self.k = 0
        self.done_rows = 0
        assert env.level_stats.shape == (env.num_levels + 1, 3 + 2 * env.N) and env.level_stats.dtype == torch.float64
        assert env.finished_level.shape == (env.B,) and env.finished_level.dtype == torch.int32
        assert env.level_stats_now() is env.level_stats and not env.level_stats.any()

    def step(self, actions=None):
        env = self.env
        before = env.level.cpu().numpy().copy()
        a = _act(self.torch, env, self.rng) if actions is None else actions
        _, _, done, info = env.step(a)
        assert info["finished_level"] is env.finished_level
        d = done.cpu().numpy()
        want = self.acc.step(before, d, env.truncated.cpu().numpy(), env.episode_return.cpu().numpy(), env.episode_length.cpu().numpy())
        got = env.finished_level.cpu().numpy()
        assert np.array_equal(got, want), f"step {self.k}: finished_level {got.tolist()} != {want.tolist()}"
        have, ours = _bits(env.level_stats), self.acc.array().view(np.uint64)
        assert np.array_equal(have, ours), (f"step {self.k}: level_stats differs in {int((have != ours).sum())} of {have.size} values\n"
                                            f"{env.level_stats.cpu().numpy()}\n{self.acc.array()}")
        self.k += 1
        self.done_rows += int((d != 0).sum())
        return d != 0


@pytest.mark.parametrize("B,N,K,kw", [(5, 2, 3, {}), (70, 1, 3, dict(obs=False)), (70, 1, 6, dict(obs=False))],
                         ids=["B5_N2_K3", "B70_N1_K3", "B70_N1_K6"])
def test_stats_match_the_host_accumulator_bit_for_bit(torch_cuda, B, N, K, kw):
    """B = 70 crosses a 64-lane boundary and puts ~23 (K = 3) envs into one row in the step in which all envs end; K = 6: seven rows, not a
    multiple of the four wavefronts of a workgroup"""
    env = _env(B, N, K, level_stats=True, **kw)
    t = _Tracked(torch_cuda, env)
    env.reset()
    for _ in range(23):
        t.step()
    s = env.level_stats.cpu().numpy()
    episodes, ret_sum = env.rollout_stats()
    assert t.done_rows == 3 * B and s[:, 0].sum() == episodes == 3 * B          # steps 6, 13, 20: every env, the TimeLimit
    assert s[:K, 0].sum() == episodes and (s[K] == 0).all()                        # nothing unattributed
    assert (s[:, 1] == s[:, 0]).all() and (s[:, 2] == 7 * s[:, 0]).all()           # all truncated, 7 steps each
    assert (s[:K, 0] > 0).sum() >= 2
    assert abs(s[:, 3:3 + N].sum() - ret_sum) <= 1e-9 * max(1.0, abs(ret_sum))     # (rollout_stats adds with atomics: not bit-exact)
    env.close()


@pytest.mark.parametrize("N", [3, 8])
def test_stats_with_many_cars(torch_cuda, N):
    """B5_N2_K3 above at the car counts whose columns (C = 9, C = 19) a rollout had never stored"""
    B, K = 5, 3
    env = _env(B, N, K, level_stats=True, obs=False)
    t = _Tracked(torch_cuda, env)
    env.reset()
    for _ in range(16):
        t.step()
    s = env.level_stats.cpu().numpy()
    assert s.shape == (K + 1, 3 + 2 * N) and t.done_rows == 2 * B == s[:, 0].sum() == env.rollout_stats()[0]
    assert (s[K] == 0).all() and (s[:, 2] == 7 * s[:, 0]).all() and (s[:K, 3 + N:][s[:K, 0] > 0] > 0).all()      # every car's square column took something
    env.close()


@pytest.mark.parametrize("streams", [1, 2])
def test_stats_at_the_bench_level_count(torch_cuda, streams):
    """B = 1100, K = 256 (the pool: one level row tiled, as test_set_level_weights does): 257 wavefronts, `done` rows the step itself wrote,
    one full round on the row pass's 16-byte path plus a tail of 76; streams=2 is the default topology"""
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    B, K = 1100, 256
    blobs = np.tile(_pool(1)[0][:1], (K, 1))
    env = VecMultiCarRacing(B, 1, seed=SEED, levels=blobs, level_stats=True, obs=False, streams=streams, max_episode_steps=7)
    t = _Tracked(torch_cuda, env)
    env.reset()
    for k in range(15):
        d = t.step()
        assert d.all() == d.any() == (k % 7 == 6)
    s = env.level_stats.cpu().numpy()
    assert t.done_rows == 2 * B == s[:K, 0].sum() and (s[K] == 0).all() and (s[:K, 0] > 0).sum() > K // 2
    env.close()


def test_stats_with_staggered_endings_at_B_2118(torch_cuda):
    """B = 2118 — two full rounds of the row pass and a tail of 70 — with `done` rows the step wrote.  All envs reach the TimeLimit together
    in step 6; reset_envs() on three subsets behind steps 7, 8 and 9 then puts them out of phase for good (an env reset behind step k ends in
    step k + 7): envs 0 .. 1022 end in steps 13, 20, 27, the tail (>= 2048) in 14, 21, 28, envs 1025 .. 2047 in 15, 22, 29 and the pair
    {1023, 1024} — the last env of round 0 and the first of round 1 — in step 16 and 23.  The step kinds this was built for are asserted."""
    torch = torch_cuda
    B, K = 2118, 3
    env = _env(B, 1, K, level_stats=True, obs=False)
    t = _Tracked(torch, env, rng_seed=5)
    env.reset()
    e = np.arange(B)
    groups = {7: e >= 2048, 8: (e >= 1025) & (e < 2048), 9: (e == 1023) | (e == 1024)}
    kinds = set()
    for k in range(30):
        d = t.step()
        if not d.any():
            kinds.add("none")
        elif d.all():
            kinds.add("all")
        elif not d[:2048].any():
            kinds.add("tail_only")
        elif np.array_equal(np.flatnonzero(d), [1023, 1024]):
            kinds.add("pair_1023_1024")
        elif d[1024:2048].any() and not d[:1024].any():
            kinds.add("round_1_not_round_0")
        elif d[:1024].any() and not d[1024:].any():
            kinds.add("round_0_only")
        if k in groups:
            env.reset_envs(torch.from_numpy(groups[k].astype(np.uint8)).to(env.device))
    assert kinds == {"none", "all", "tail_only", "pair_1023_1024", "round_1_not_round_0", "round_0_only"}, kinds
    s = env.level_stats.cpu().numpy()
    assert s[:, 0].sum() == t.done_rows and (s[K] == 0).all() and (s[:K, 0] > 0).all()
    env.close()


FEATURES = {
    "frame_skip": dict(kw=dict(frame_skip=4), steps=8, ends=4),                    # a macro-step counts once
    "graph_two_streams": dict(kw=dict(graph=True, streams=2), steps=16, ends=2),
    "state_obs": dict(kw=dict(state_obs=True), steps=16, ends=2),
    "terminal_obs": dict(kw=dict(terminal_obs=True), steps=16, ends=2),
}


@pytest.mark.parametrize("feature", list(FEATURES))
def test_stats_with_the_other_features(torch_cuda, feature):
    c = FEATURES[feature]
    env = _env(4, 2, 3, level_stats=True, **c["kw"])
    t = _Tracked(torch_cuda, env)
    env.reset()
    for _ in range(c["steps"]):
        t.step()
    assert t.done_rows == c["ends"] * 4 and env.level_stats[:, 0].sum().item() == env.rollout_stats()[0] == t.done_rows
    env.close()


def test_stats_without_auto_reset_count_every_reported_done(torch_cuda):
    """auto_reset=False: an env stepped past its end reports `done` again, and counts again, until reset_envs() — the documented rule"""
    torch = torch_cuda
    env = _env(4, 2, 3, level_stats=True, auto_reset=False, max_episode_steps=5)
    t = _Tracked(torch, env, rng_seed=4)
    env.reset()
    resets = installs = 0
    for k in range(14):
        d = t.step()
        if d.any():                                        # all four hit the TimeLimit together: reset two now, two a step later
            m = d & (np.arange(4) % 2 == (resets % 2))
            env.reset_envs(torch.from_numpy(m.astype(np.uint8)).to(env.device))
            resets += 1; installs += int(m.sum())
    s = env.level_stats.cpu().numpy()
    assert resets >= 3 and s[:, 0].sum() == t.done_rows > installs and (s[3] == 0).all()
    env.close()


def test_snapshots_unattributed_row_and_clones(torch_cuda):
    """load_states leaves `level` at -1: that episode lands in row K and finished_level == K; a clone's episode counts for the source's level"""
    torch = torch_cuda
    B, N, K = 4, 2, 3
    env = _env(B, N, K, level_stats=True, level_order="cycle")
    t = _Tracked(torch, env, rng_seed=8)
    env.reset()
    assert env.level.cpu().numpy().tolist() == [0, 1, 2, 0]
    for _ in range(3):
        t.step()
    env.clone_envs([0], [2])
    env.load_states(env.save_states([1]), [3])
    assert env.level.cpu().numpy().tolist() == [0, 1, 0, -1]
    for _ in range(4):
        d = t.step()
    assert d.all() and env.finished_level.cpu().numpy().tolist() == [0, 1, 0, K]
    s = env.level_stats.cpu().numpy()
    assert s[:, 0].tolist() == [2.0, 1.0, 0.0, 1.0] and s[K, 2] == 7.0
    assert env.level.cpu().numpy().tolist() == [1, 2, 0, 1]       # the targets' own next levels (test_gpu_level_pool.py)
    for _ in range(7):
        d = t.step()
    assert d.all() and env.finished_level.cpu().numpy().tolist() == [1, 2, 0, 1]
    env.close()


def test_reset_level_stats_zeroes_in_stream_order(torch_cuda):
    env = _env(5, 2, 3, level_stats=True)
    t = _Tracked(torch_cuda, env)
    env.reset()
    for _ in range(8):
        t.step()
    assert env.level_stats[:, 0].sum().item() == 5
    env.reset_level_stats(); t.acc.reset()                 # enqueued behind step 7, in front of step 8: no synchronisation in between
    for _ in range(8):
        t.step()
    assert env.level_stats[:, 0].sum().item() == 5 and not env.level_stats[3].any()
    env.close()


@pytest.mark.parametrize("order", ["random", "cycle"])
def test_random_and_cycle_are_unchanged_by_level_stats(torch_cuda, order):
    torch = torch_cuda
    on, off = _env(5, 2, 3, level_order=order, level_stats=True), _env(5, 2, 3, level_order=order)
    assert off.level_stats is None and off.finished_level is None and off.level_cdf is None
    on.reset(); off.reset()
    rng = np.random.RandomState(3)
    for k in range(16):
        a = _act(torch, on, rng)
        on.step(a); _, _, _, info = off.step(a)
        assert "finished_level" not in info
        for name in ("reward", "done", "truncated", "level", "episode_return", "obs"):
            assert np.array_equal(getattr(on, name).cpu().numpy(), getattr(off, name).cpu().numpy()), f"step {k}: {name}"
    with pytest.raises(Exception):
        off.reset_level_stats()
    with pytest.raises(Exception):
        off.set_level_weights([1, 1, 1])
    on.close(); off.close()


# ------------------------------------------------------------------ weighted sampling
class _Cdf:
    """the CDF in force, as the host sees it (the control's _generate reads it when it stages an episode)"""

    def __init__(self, K):
        self.now = ref.cdf(np.ones(K))[0]

    def set(self, w):
        self.now, fell_back = ref.cdf(w)
        assert not fell_back


def _make_weighted_pair(torch, B, N, K, cdf, env_offset=0, control=True, **kw):
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    kw.setdefault("streams", 1); kw.setdefault("max_episode_steps", 7)
    common = dict(seed=SEED, env_offset=env_offset, **kw)
    blobs, _ = _pool(N, K)
    pool = VecMultiCarRacing(B, N, levels=np.array(blobs), level_order="weighted", **common)
    if not control:
        return pool, None
    ctl = VecMultiCarRacing(B, N, async_refill=False, **common)
    counter = np.zeros(B, np.int64)
    keep = []

    def generate(ids):
        ids = np.ascontiguousarray(ids, np.int32)
        if len(ids) == 0:
            return None
        rows = torch.empty((len(ids), ctl.slot_bytes), dtype=torch.uint8, pin_memory=True)
        out = rows.numpy()
        for i, e in enumerate(ids):
            out[i] = blobs[ref.weighted_level(SEED, env_offset + int(e), int(counter[e]), cdf.now)]
            counter[e] += 1
        keep.append(rows); del keep[:-4]          # (the staging copies are asynchronous: the rows outlive the call)
        return out

    ctl._generate = generate
    return pool, ctl


def test_weighted_rollout_parity_with_the_host_staged_control(torch_cuda):
    """B = 5, N = 2, K = 3, weights [1, 0, 3] before reset(), [0, 1, 0] from step 10 on.  Episode k of an env is staged — and drawn — when
    episode k - 1 is installed: k = 0, 1 around reset(), k = 2 behind step 6, k = 3 behind step 13 (the first draw under the new weights),
    installed by step 20.  So level 1 is never played before step 20 and always from then on: the one-episode lag."""
    torch = torch_cuda
    from multi_car_racing_amd import levels
    B, N, K = 5, 2, 3
    cdf = _Cdf(K)
    pool, ctl = _make_weighted_pair(torch, B, N, K, cdf)
    assert _bits(pool.level_cdf).tolist() == cdf.now.view(np.uint64).tolist()      # a new handle draws uniformly
    old = ref.cdf([1, 0, 3])[0]; new = ref.cdf([0, 1, 0])[0]
    pool.set_level_weights([1, 0, 3]); cdf.set([1, 0, 3])
    assert _bits(pool.level_cdf).tolist() == old.view(np.uint64).tolist()
    op, oc = pool.reset(), ctl.reset()
    assert np.array_equal(op.cpu().numpy(), oc.cpu().numpy())
    ordinal = np.zeros(B, np.int64)

    def want_levels():
        return [ref.weighted_level(SEED, e, int(ordinal[e]), old if ordinal[e] <= 2 else new) for e in range(B)]

    assert pool.level.cpu().numpy().tolist() == want_levels()
    assert [levels.weighted_level(SEED, e, 0, old) for e in range(B)] == want_levels()
    rng = np.random.RandomState(3)
    for k in range(30):
        if k == 10:
            pool.set_level_weights(np.array([0.0, 1.0, 0.0], np.float32)); cdf.set([0, 1, 0])
        a = _act(torch, pool, rng)
        _, _, done, info = pool.step(a); ctl.step(a)
        for name in ("reward", "done", "truncated", "episode_return", "episode_length", "obs"):
            g, w = getattr(pool, name).cpu().numpy(), getattr(ctl, name).cpu().numpy()
            assert np.array_equal(g, w), f"step {k}: {name}"
        d = done.cpu().numpy() != 0
        assert d.all() == d.any() == (k % 7 == 6)
        ordinal[d] += 1
        lv = pool.level.cpu().numpy().tolist()
        assert info["level"] is pool.level and lv == want_levels(), f"step {k}: level"
        if k < 20:
            assert 1 not in lv, f"step {k}: level 1 (weight 0) is played: {lv}"        # steps 13 .. 19: still the old weights' draw (the lag)
        else:
            assert lv == [1] * B, f"step {k}: {lv}"
    sp, sc = pool.get_state(), ctl.get_state()
    for key in sp:
        assert np.array_equal(sp[key], sc[key]), f"get_state()[{key!r}]"
    assert int(pool.status_words()[4]) == 0 and pool.episodes_generated == K
    pool.close(); ctl.close()


def test_weighted_batch_independence(torch_cuda):
    """two handles of B = 3 with env_offset 0 and 3 reproduce one handle of B = 6 under the same sequence of weights"""
    torch = torch_cuda
    N, K = 2, 3
    cdf = _Cdf(K)
    envs = [_make_weighted_pair(torch, b, N, K, cdf, env_offset=off, control=False)[0] for b, off in ((6, 0), (3, 0), (3, 3))]
    whole, lo, hi = envs
    for e in envs:
        e.set_level_weights([1, 0, 3])
    ow = whole.reset().cpu().numpy()
    assert np.array_equal(ow[:3], lo.reset().cpu().numpy()) and np.array_equal(ow[3:], hi.reset().cpu().numpy())
    rng = np.random.RandomState(6)
    seen = set()
    for k in range(24):
        if k == 3:
            for e in envs:
                e.set_level_weights([2, 5, 1])
        a = random_actions(rng, 6, N, 0.2)
        whole.step(torch.from_numpy(a).to(whole.device)); lo.step(torch.from_numpy(a[:3]).to(whole.device)); hi.step(torch.from_numpy(a[3:]).to(whole.device))
        for name in ("reward", "done", "level", "episode_return"):
            w = getattr(whole, name).cpu().numpy()
            assert np.array_equal(w[:3], getattr(lo, name).cpu().numpy()) and np.array_equal(w[3:], getattr(hi, name).cpu().numpy()), f"step {k}: {name}"
        seen |= set(whole.level.cpu().numpy().tolist())
    assert len(seen) > 1
    for e in envs:
        e.close()


def test_set_level_weights(torch_cuda, lib):
    torch = torch_cuda
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    L = lib.load()
    K = 300
    blobs = np.tile(_pool(1)[0][:1], (K, 1))                # 300 rows of one track: the CDF kernel does not care
    env = VecMultiCarRacing(4, 1, seed=SEED, levels=blobs, level_order="weighted", obs=False, streams=1, max_episode_steps=7)
    uniform = ref.cdf(np.ones(K))[0]
    assert _bits(env.level_cdf).tolist() == uniform.view(np.uint64).tolist()
    # check=True: ValueError, nothing changed
    for bad in ([1.0] * (K - 1), [-1.0] + [1.0] * (K - 1), [float("nan")] + [1.0] * (K - 1), [float("inf")] + [1.0] * (K - 1), [0.0] * K,
                torch.zeros(K, dtype=torch.float64, device=env.device), torch.ones(K, dtype=torch.int32, device=env.device),
                torch.ones(K + 1, dtype=torch.float32, device=env.device)):
        with pytest.raises(ValueError):
            env.set_level_weights(bad)
    assert _bits(env.level_cdf).tolist() == uniform.view(np.uint64).tolist()
    # K = 300 (five rounds of the kernel's 64, the last one partial), magnitudes spread, zeros inside: the device CDF, bit for bit
    rng = np.random.RandomState(9)
    w = 10.0 ** rng.uniform(-12, 12, K) * (rng.rand(K) < 0.8)
    want, fb = ref.cdf(w)
    for given in (w, torch.from_numpy(w).to(env.device)):
        env.set_level_weights(np.ones(K))
        flag = env.set_level_weights(given)
        assert not fb and int(flag.item()) == 0 and _bits(env.level_cdf).tolist() == want.view(np.uint64).tolist()
    # check=False with what check=True refuses: cleaned on the device like ref.cdf cleans it
    dirty = w.copy(); dirty[3] = float("nan"); dirty[64] = -2.0; dirty[299] = float("inf")
    flag = env.set_level_weights(torch.from_numpy(dirty).to(env.device), check=False)
    assert int(flag.item()) == 0 and _bits(env.level_cdf).tolist() == ref.cdf(dirty)[0].view(np.uint64).tolist()
    # an all-zero device tensor, check=False: flag 1, the uniform CDF — and the rollout draws as a new handle does
    flag = env.set_level_weights(torch.zeros(K, dtype=torch.float32, device=env.device), check=False)
    assert flag.dtype == torch.int32 and flag.shape == (1,) and int(flag.item()) == 1
    assert _bits(env.level_cdf).tolist() == uniform.view(np.uint64).tolist()
    env.reset()
    assert env.level.cpu().numpy().tolist() == [ref.weighted_level(SEED, e, 0, uniform) for e in range(4)]
    # state errors
    cdf_buf = torch.zeros(K, dtype=torch.float64, device=env.device); staged = torch.zeros(4, dtype=torch.int32, device=env.device)
    c, s = ctypes.c_void_p(cdf_buf.data_ptr()), ctypes.c_void_p(staged.data_ptr())
    assert L.mcr_set_level_sampler(env.h, c, s) == MCR_ERR_STATE and b"after the first mcr_reset" in L.mcr_last_error()
    assert L.mcr_set_level_sampler(env.h, None, s) == MCR_ERR_ARG and L.mcr_set_level_sampler(env.h, c, None) == MCR_ERR_ARG
    env.close()
    plain = VecMultiCarRacing(2, 1, seed=SEED, async_refill=False, obs=False, streams=1)
    assert L.mcr_set_level_sampler(plain.h, c, s) == MCR_ERR_STATE and L.mcr_level_weights(plain.h, c, None, None) == MCR_ERR_STATE
    assert L.mcr_set_level_stats(plain.h, s, c) == MCR_ERR_STATE and L.mcr_set_level_stats(plain.h, None, None) == MCR_OK
    plain.close()
    cyc = VecMultiCarRacing(2, 1, seed=SEED, levels=np.array(_pool(1)[0]), level_order="cycle", obs=False, streams=1)
    assert L.mcr_set_level_sampler(cyc.h, c, s) == MCR_ERR_STATE and L.mcr_level_weights(cyc.h, c, None, None) == MCR_ERR_STATE
    cyc.close()
