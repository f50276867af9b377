"""MI355X: level pools (VecMultiCarRacing(levels=...), include/mcr.h: mcr_set_episode_pool, csrc/k_pool.h) against the host-staged path.

The yardstick is the code that existed before the feature: a CONTROL handle created without `levels` and with async_refill=False, whose
`_generate` is replaced by a function that hands out pool rows in the order mcr_pool_level prescribes — a per-env episode counter that
starts at 0 — so that the host stages, episode by episode, what the pool handle's kernel must copy by itself."""
import ctypes

import numpy as np
import pytest

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


def _want_level(env_offset, e, k, K, order):
    from multi_car_racing_amd.levels import pool_level
    return pool_level(SEED, env_offset + e, k, K, order)


def _make_pair(torch, B, N, order, K=3, env_offset=0, control=True, **kw):
    """(pool handle, control handle or None).  The control's _generate(ids) returns the pool rows mcr_pool_level prescribes."""
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    kw.setdefault("streams", 1)
    common = dict(seed=SEED, env_offset=env_offset, **kw)
    pool = VecMultiCarRacing(B, N, levels=K, level_order=order, **common)
    blobs, info = _pool(N, K)
    assert np.array_equal(pool._pool_np, blobs) and np.array_equal(pool.level_info, info)
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
            out[i] = blobs[_want_level(env_offset, int(e), int(counter[e]), K, order)]
            counter[e] += 1
        keep.append(rows); del keep[:-4]          # (the staging copies are asynchronous: the rows outlive the call)
        return out

    ctl._generate = generate
    return pool, ctl


class _Ordinals:
    """which episode (0: the first) each env of a rollout is in: + 1 per reset and per auto-reset"""

    def __init__(self, B, env_offset, K, order):
        self.k = np.full(B, -1, np.int64); self.B, self.off, self.K, self.order = B, env_offset, K, order

    def installed(self, mask):
        self.k[np.asarray(mask, bool)] += 1

    def levels(self):
        return np.array([_want_level(self.off, e, int(self.k[e]), self.K, self.order) if self.k[e] >= 0 else -1 for e in range(self.B)], np.int32)


def _same(a, b, what):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert a.shape == b.shape and np.array_equal(a, b), f"{what}: differs in {int((a != b).sum())} of {a.size} values"


def _compare_step(pool, ctl, k, extra=()):
    for name in ("reward", "done", "truncated", "episode_return", "episode_length") + tuple(extra):
        _same(getattr(pool, name), getattr(ctl, name), f"step {k}: {name}")
    if pool.obs is not None:
        _same(pool.obs, ctl.obs, f"step {k}: obs")


def _compare_terminal(pool, ctl, k):
    n = int(pool.terminal_count.item())
    assert n == int(ctl.terminal_count.item()), f"step {k}: terminal_count"
    ip, ic = pool.terminal_env_ids[:n].cpu().numpy(), ctl.terminal_env_ids[:n].cpu().numpy()
    op, oc = np.argsort(ip), np.argsort(ic)               # (entries are appended in the order the envs end in: by env id)
    assert np.array_equal(ip[op], ic[oc]), f"step {k}: terminal_env_ids"
    fp, fc = pool.terminal_obs[:n].cpu().numpy()[op], ctl.terminal_obs[:n].cpu().numpy()[oc]
    assert np.array_equal(fp, fc), f"step {k}: terminal frames differ for envs {ip[op][[(a != b).any() for a, b in zip(fp, fc)]]}"
    return n


def _compare_state(pool, ctl):
    sp, sc = pool.get_state(), ctl.get_state()
    for key in sp:
        assert np.array_equal(sp[key], sc[key]), f"get_state()[{key!r}]"
    ep, ec = pool.get_env_state(), ctl.get_env_state()
    for key in ep:
        assert np.array_equal(ep[key], ec[key]), f"get_env_state()[{key!r}]"


def _healthy(pool, K):
    """never starved: status word 4, the frozen env-step counter; nothing generated after the pool; every env staged"""
    assert int(pool.status_words()[4]) == 0 and int(pool.debug_counters()[3]) == 0
    assert pool.episodes_generated == K and pool._worker is None and not pool._svc
    rec = np.zeros((pool.B, 12), np.int32)
    assert pool.L.mcr_debug_read_env_records(pool.h, rec.ctypes.data_as(ctypes.c_void_p), rec.nbytes) == MCR_OK
    assert (rec[:, 4] == 1).all(), f"staged_ready: {rec[:, 4]}"          # (word 4 of the record: mcr_common.h McrEnvState)


def _rollout(torch, pool, ctl, steps, order, K=3, extra=(), terminal=False, reset_at=None, frame_skip=1):
    B, N = pool.B, pool.N
    ordn = _Ordinals(B, pool.env_offset, K, order)
    _same(pool.reset(), ctl.reset(), "reset obs") if pool.obs is not None else (pool.reset(), ctl.reset())
    ordn.installed(np.ones(B, bool))
    assert np.array_equal(pool.level.cpu().numpy(), ordn.levels()), "level after reset()"
    rng = np.random.RandomState(3)
    ended = terminals = 0
    for k in range(steps):
        if reset_at is not None and k == reset_at:
            pool.reset(); ctl.reset(); ordn.installed(np.ones(B, bool))
            assert np.array_equal(pool.level.cpu().numpy(), ordn.levels()), "level after the second reset()"
        a = torch.from_numpy(random_actions(rng, B, N, 0.2)).to(pool.device)
        _, _, done, info = pool.step(a); ctl.step(a)
        _compare_step(pool, ctl, k, extra)
        if terminal:
            terminals += _compare_terminal(pool, ctl, k)
        d = done.cpu().numpy() != 0
        ended += int(d.sum())
        if pool.auto_reset:
            ordn.installed(d)
        assert info["level"] is pool.level and np.array_equal(pool.level.cpu().numpy(), ordn.levels()), f"step {k}: level"
    _compare_state(pool, ctl)
    _healthy(pool, K)
    return ended, terminals, ordn


@pytest.mark.parametrize("order", ["random", "cycle"])
def test_rollout_parity_with_the_host_staged_control(torch_cuda, order):
    """N=2, B=5, K=3, TimeLimit 7, 40 steps: five episodes per env, every output bit-identical with the control's each step"""
    pool, ctl = _make_pair(torch_cuda, 5, 2, order, max_episode_steps=7)
    ended, _, ordn = _rollout(torch_cuda, pool, ctl, 40, order)
    assert ended == 5 * 5 and (ordn.k == 5).all()
    ep = pool.current_episode(1)                           # the host copy of the level env 1 is in
    assert ep["T"] == int(pool.level_info[int(pool.level[1].item()), 0]) == int(pool.get_env_state()["num_tiles"][1])
    pool.close(); ctl.close()


def test_group_boundary_and_full_reset(torch_cuda):
    """B=70 crosses the scanning workgroups' boundaries (16 envs each: four full groups and one of 6; env 64 and up live past a wavefront's
    64 lanes), physics only, with a reset() of all envs mid-run"""
    pool, ctl = _make_pair(torch_cuda, 70, 1, "random", obs=False, max_episode_steps=7)
    ended, _, ordn = _rollout(torch_cuda, pool, ctl, 20, "random", reset_at=10)
    assert ended == 70 * 2 and (ordn.k == 3).all()         # reset, 7 steps, [3 steps] reset, 7 steps
    assert len(set(pool.level.cpu().numpy().tolist())) == 3
    pool.close(); ctl.close()


FEATURES = {
    "terminal_obs": dict(kw=dict(terminal_obs=True, max_episode_steps=7), steps=16, terminal=True),
    "frame_skip": dict(kw=dict(frame_skip=4, max_episode_steps=7), steps=8),
    "gray_stack": dict(kw=dict(obs_format="gray", frame_stack=4, max_episode_steps=9), steps=20),
    "state_obs": dict(kw=dict(state_obs=True, max_episode_steps=7), steps=16, extra=("state",)),
    "graph_two_streams": dict(kw=dict(graph=True, streams=2, max_episode_steps=7), steps=16),
}


@pytest.mark.parametrize("feature", list(FEATURES))
def test_with_the_other_features(torch_cuda, feature):
    """B=4, N=2, K=3 against the control.  terminal_obs: the terminal frames read the slot the env just left — the slot the kernel
    overwrites — so a restage that came too early would show in them."""
    c = FEATURES[feature]
    pool, ctl = _make_pair(torch_cuda, 4, 2, "random", **c["kw"])
    ended, terminals, _ = _rollout(torch_cuda, pool, ctl, c["steps"], "random", extra=c.get("extra", ()), terminal=c.get("terminal", False))
    assert ended >= 8
    if c.get("terminal"):
        assert terminals == ended
    pool.close(); ctl.close()


def test_manual_reset_envs(torch_cuda):
    """auto_reset=False: a finished env waits for reset_envs(mask), which installs its staged level; the kernel behind the reset re-stages"""
    torch = torch_cuda
    B, N, K, order = 4, 2, 3, "random"
    pool, ctl = _make_pair(torch, B, N, order, auto_reset=False, max_episode_steps=5)
    ordn = _Ordinals(B, 0, K, order)
    _same(pool.reset(), ctl.reset(), "reset obs"); ordn.installed(np.ones(B, bool))
    rng = np.random.RandomState(4)
    resets = 0
    for k in range(14):
        a = torch.from_numpy(random_actions(rng, B, N, 0.2)).to(pool.device)
        pool.step(a); ctl.step(a)
        _compare_step(pool, ctl, k)
        d = pool.done.cpu().numpy() != 0
        if d.any():                                        # all four hit the TimeLimit together: reset two now, two a step later
            m = d & (np.arange(B) % 2 == (resets % 2))
            mask = torch.from_numpy(m.astype(np.uint8)).to(pool.device)
            _same(pool.reset_envs(mask), ctl.reset_envs(mask), f"step {k}: obs after reset_envs")
            ordn.installed(m); resets += 1
        assert np.array_equal(pool.level.cpu().numpy(), ordn.levels()), f"step {k}: level"
    assert resets >= 3 and ordn.k.max() >= 2
    _compare_state(pool, ctl)
    _healthy(pool, K)
    pool.close(); ctl.close()


def test_batch_independence(torch_cuda):
    """two handles of B=3 with env_offset 0 and 3 reproduce one handle of B=6, step by step"""
    torch = torch_cuda
    N, K, order = 2, 3, "random"
    whole, _ = _make_pair(torch, 6, N, order, control=False, max_episode_steps=7)
    lo, _ = _make_pair(torch, 3, N, order, env_offset=0, control=False, max_episode_steps=7)
    hi, _ = _make_pair(torch, 3, N, order, env_offset=3, control=False, max_episode_steps=7)
    ow = whole.reset().cpu().numpy()
    assert np.array_equal(ow[:3], lo.reset().cpu().numpy()) and np.array_equal(ow[3:], hi.reset().cpu().numpy())
    rng = np.random.RandomState(6)
    for k in range(24):
        a = random_actions(rng, 6, N, 0.2)
        whole.step(torch.from_numpy(a).to(whole.device)); lo.step(torch.from_numpy(a[:3]).to(whole.device)); hi.step(torch.from_numpy(a[3:]).to(whole.device))
        for name in ("obs", "reward", "done", "truncated", "episode_return", "episode_length", "level"):
            w = getattr(whole, name).cpu().numpy()
            assert np.array_equal(w[:3], getattr(lo, name).cpu().numpy()) and np.array_equal(w[3:], getattr(hi, name).cpu().numpy()), f"step {k}: {name}"
    assert len(set(whole.level.cpu().numpy().tolist())) > 1
    for e in (whole, lo, hi):
        _healthy(e, K); e.close()


def test_snapshots_keep_the_targets_levels(torch_cuda):
    """clone_envs copies the `level` rows, load_states sets them to -1; the copies continue bit-identically with their sources until the
    episode ends, then play the TARGET's next prescribed level.  "cycle" with K = 3: env e plays level (e + k) % 3 in episode k, so env 2's
    second level is env 0's first (0) and env 3's second is env 1's first (1): their first states must be those reset() produced."""
    torch = torch_cuda
    B, N, K, order = 4, 2, 3, "cycle"
    pool, _ = _make_pair(torch, B, N, order, control=False, max_episode_steps=7)
    pool.reset()
    first = pool.get_state()["bodies"].copy(); tiles = pool.get_env_state()["num_tiles"].copy()
    assert pool.level.cpu().numpy().tolist() == [0, 1, 2, 0]
    rng = np.random.RandomState(8)

    def act():
        a = random_actions(rng, B, N, 0.2); a[2] = a[0]; a[3] = a[1]
        return torch.from_numpy(a).to(pool.device)

    for _ in range(3):
        pool.step(act())
    pool.clone_envs([0], [2])
    rows = pool.save_states([1])
    pool.load_states(rows, [3])
    assert pool.level.cpu().numpy().tolist() == [0, 1, 0, -1]
    with pytest.raises(Exception):
        pool.current_episode(3)
    for k in range(3, 7):
        obs, rew, done, _ = pool.step(act())
        o, r, d = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()
        assert np.array_equal(r[2], r[0]) and np.array_equal(r[3], r[1]) and d[2] == d[0] and d[3] == d[1], f"step {k}"
        if k < 6:
            assert not d.any() and np.array_equal(o[2], o[0]) and np.array_equal(o[3], o[1]), f"step {k}"
            assert pool.level.cpu().numpy().tolist() == [0, 1, 0, -1]
    assert d.all()                                         # the TimeLimit, copies included (the record's step counter travels with the state)
    assert pool.level.cpu().numpy().tolist() == [1, 2, 0, 1]       # episode 1 of envs 0 .. 3: (e + 1) % 3 — the targets' own, not the sources'
    st = pool.get_state()["bodies"]; nt = pool.get_env_state()["num_tiles"]
    assert np.array_equal(st[2], first[0]) and nt[2] == tiles[0] and np.array_equal(st[3], first[1]) and nt[3] == tiles[1]
    assert not np.array_equal(st[0], st[2])
    _healthy(pool, K)
    pool.close()


def test_errors(torch_cuda, lib):
    torch = torch_cuda
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    L = lib.load()
    blobs, _ = _pool(2)
    dev = torch.zeros(3 * blobs.shape[1] + 64, dtype=torch.uint8, device="cuda")
    level = torch.zeros(2, dtype=torch.int32, device="cuda")
    p, lv = dev.data_ptr(), ctypes.c_void_p(level.data_ptr())
    assert p % 16 == 0

    def set_pool(h, ptr, K, mode):
        return L.mcr_set_episode_pool(h, ctypes.c_void_p(ptr) if ptr else None, K, ctypes.c_uint64(1), ctypes.c_uint32(0), mode, lv)

    plain = VecMultiCarRacing(2, 2, seed=SEED, async_refill=False, streams=1)
    assert set_pool(plain.h, p, 0, 0) == MCR_ERR_ARG and set_pool(plain.h, p, -1, 0) == MCR_ERR_ARG
    assert set_pool(plain.h, p + 8, 3, 0) == MCR_ERR_ARG and b"aligned" in L.mcr_last_error()
    assert set_pool(plain.h, p, 3, 2) == MCR_ERR_ARG and set_pool(plain.h, p, 3, -1) == MCR_ERR_ARG
    assert set_pool(plain.h, 0, 3, 0) == MCR_ERR_ARG and set_pool(None, p, 3, 0) == MCR_ERR_ARG
    plain.reset()
    assert set_pool(plain.h, p, 3, 0) == MCR_ERR_STATE and b"after the first mcr_reset" in L.mcr_last_error()
    ids = np.zeros(1, np.int32); n = L.mcr_poll_consumed(plain.h, lib.ptr(ids), 1, None)
    assert n >= 0                                          # nothing changed for a handle without a pool
    plain.close()

    pool = VecMultiCarRacing(2, 2, seed=SEED, levels=np.array(blobs), streams=1)
    assert pool.level_info is None and pool.num_levels == 3
    ids = np.zeros(2, np.int32); row = np.ascontiguousarray(blobs[:1])
    mt = np.zeros((2, lib.MT_WORDS), np.uint32); pin = torch.empty((2, blobs.shape[1]), dtype=torch.uint8, pin_memory=True)
    for when in ("before", "after"):
        assert L.mcr_stage_episodes(pool.h, lib.ptr(ids), 1, lib.ptr(row), None) == MCR_ERR_STATE and b"level pool" in L.mcr_last_error()
        assert L.mcr_refill_start(pool.h, lib.ptr(mt), lib.ptr(mt), 2, 1, ctypes.c_void_p(pin.data_ptr()), None) == MCR_ERR_STATE
        assert L.mcr_poll_consumed(pool.h, lib.ptr(ids), 2, None) == MCR_ERR_STATE
        if when == "before":
            pool.reset()
    assert pool.level.cpu().numpy().tolist() == [_want_level(0, e, 0, 3, "random") for e in range(2)]
    pool.close()
    with pytest.raises(ValueError):
        VecMultiCarRacing(2, 2, levels=np.zeros((3, 100), np.uint8))
    with pytest.raises(ValueError):
        VecMultiCarRacing(2, 2, levels=3, level_order="shuffle")
    with pytest.raises(ValueError):
        VecMultiCarRacing(2, 2, levels=0)
