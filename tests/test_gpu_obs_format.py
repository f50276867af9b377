"""MI355X: gray and frame-stacked observations drawn by the raster (include/mcr.h: mcr_set_obs_format; vec_env.py obs_format / frame_stack).

Every check holds a gray handle against an RGB twin (same seed, same actions, same episodes): a gray frame is the luma of the twin's RGB frame,
bit for bit — the same raster keys, so no ambiguity mask —, and a stack is what gym's FrameStack(k) builds from those frames on the host side
(first frame k times after a reset or an auto-reset).  Plus terminal stacks, the oracle at B = 4096, and the argument checks."""
import numpy as np
import pytest

from tests.util import luma_np, oracle_episode

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _luma(torch, rgb):
    """OpenCV's COLOR_RGB2GRAY on 8-bit data (the formula of include/mcr.h), on the device"""
    x = rgb.to(torch.int32)
    return ((4899 * x[..., 0] + 9617 * x[..., 1] + 1868 * x[..., 2] + 8192) >> 14).to(torch.uint8)


def _pair(B, N, seed, max_steps, k, **kw):
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    rgb = VecMultiCarRacing(B, N, seed=seed, max_episode_steps=max_steps, **kw)
    gray = VecMultiCarRacing(B, N, seed=seed, max_episode_steps=max_steps, obs_format="gray", frame_stack=k, **kw)
    return rgb, gray


def _actions(torch, g, B, N, gas_floor=0.0):
    a = torch.rand((B, N, 3), generator=g, device="cuda")
    a[..., 0] = a[..., 0] * 2 - 1
    a[..., 1] = gas_floor + (1 - gas_floor) * a[..., 1]
    a[..., 2] *= 0.2
    return a


@pytest.mark.parametrize("streams", [1, 2])
def test_gray_is_luma_of_rgb(torch_cuda, streams):
    torch = torch_cuda
    B, N = 256, 2
    rgb, gray = _pair(B, N, 11, 60, 1, streams=streams)
    assert gray.obs_shape == (N, 96, 96) and rgb.obs_shape == (N, 96, 96, 3)
    o_r, o_g = rgb.reset(), gray.reset()
    assert o_g.shape == (B, N, 96, 96) and o_g.is_contiguous()
    assert torch.equal(o_g, _luma(torch, o_r)), "reset: gray differs from the luma of the RGB twin"
    g = torch.Generator(device="cuda"); g.manual_seed(3)
    n_done = 0
    for k in range(200):
        a = _actions(torch, g, B, N)
        o_r, r_r, d_r, _ = rgb.step(a)
        o_g, r_g, d_g, _ = gray.step(a)
        assert torch.equal(r_r, r_g) and torch.equal(d_r, d_g), f"step {k}: the twins diverged"
        n_done += int(d_r.sum().item())
        if not torch.equal(o_g, _luma(torch, o_r)):
            bad = (o_g != _luma(torch, o_r)).nonzero()[:4].tolist()
            raise AssertionError(f"step {k}: gray differs from the luma of the RGB twin at {bad}")
    assert n_done >= B * 3, "the TimeLimit auto-resets did not happen"
    rgb.close(); gray.close()


def _stack_run(torch, B, N, seed, steps, k, max_steps, resets_at, gas_floor=0.0, **kw):
    rgb, gray = _pair(B, N, seed, max_steps, k, terminal_obs=True, **kw)
    assert gray.obs_shape == (N, k, 96, 96)
    ref = _luma(torch, rgb.reset()).unsqueeze(2).repeat(1, 1, k, 1, 1)      # gym FrameStack: the first frame k times
    assert torch.equal(gray.reset(), ref), "reset: the stack is not the first frame k times"
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    rs = np.random.RandomState(seed)
    n_term = n_mask = 0
    for t in range(steps):
        a = _actions(torch, g, B, N, gas_floor)
        o_r, _, d_r, _ = rgb.step(a)
        o_g, _, d_g, _ = gray.step(a)
        assert torch.equal(d_r, d_g), f"step {t}: the twins diverged"
        assert o_g.shape == (B, N, k, 96, 96)
        y = _luma(torch, o_r)
        prev = ref
        ref = torch.cat([ref[:, :, 1:], y.unsqueeze(2)], 2)
        dn = d_r.bool()
        ref[dn] = y[dn].unsqueeze(2).repeat(1, 1, k, 1, 1)                  # auto-reset: the new episode's first frame k times
        if not torch.equal(o_g, ref):
            bad = (o_g != ref).reshape(B, N, k, -1).any(-1).nonzero()[:6].tolist()
            raise AssertionError(f"step {t}: the stack differs from FrameStack({k}) of the RGB twin's luma at (env, agent, frame) {bad}")
        # terminal stacks: the previous window's last k - 1 frames, then the luma of the RGB twin's terminal frame
        ids_r, fr_r = rgb.terminal_observations()
        ids_g, fr_g = gray.terminal_observations()
        assert sorted(ids_r.tolist()) == sorted(ids_g.tolist()) == dn.nonzero().flatten().tolist()
        if len(ids_g):
            pr, pg = torch.argsort(ids_r), torch.argsort(ids_g)
            ids = ids_g[pg].long()
            want = torch.cat([prev[ids][:, :, 1:], _luma(torch, fr_r[pr]).unsqueeze(2)], 2)
            assert fr_g.shape[1:] == (N, k, 96, 96)
            assert torch.equal(fr_g[pg], want), f"step {t}: terminal stacks of envs {ids.tolist()[:8]} differ"
            n_term += len(ids)
        if t in resets_at:                                                  # reset_envs(mask): masked envs restart, the others keep their stacks
            m = torch.from_numpy((rs.uniform(size=B) < 0.3).astype(np.uint8)).cuda()
            y = _luma(torch, rgb.reset_envs(m))
            o_g = gray.reset_envs(m)
            mb = m.bool()
            ref[mb] = y[mb].unsqueeze(2).repeat(1, 1, k, 1, 1)
            assert torch.equal(o_g, ref), f"reset_envs at step {t}: the stacks differ"
            n_mask += int(mb.sum().item())
    rgb.close(); gray.close()
    return n_term, n_mask


# (37 steps per episode: the TimeLimit endings meet every ring head j; the masked resets land on heads 2 and 3, whose first frames need
# their copies in slots 1 .. j - 1 written a step later)
@pytest.mark.parametrize("graph", [False, True])
def test_stack_equals_framestack(torch_cuda, graph):
    n_term, n_mask = _stack_run(torch_cuda, 256, 2, 5, 160, 4, 37, resets_at={42, 95, 131}, graph=graph)
    assert n_term >= 256 * 3 and n_mask > 0


def test_stack_equals_framestack_contact_chain(torch_cuda):
    """N = 8, full gas: cars run into each other, and envs that re-spawn in the contact chain draw their first frames there"""
    n_term, n_mask = _stack_run(torch_cuda, 128, 8, 9, 90, 4, 29, resets_at={50}, gas_floor=0.8)
    assert n_term >= 128 * 2


def test_oracle_gray_stack(torch_cuda, oracle):
    """B = 4096, gray k = 4, 50 steps: sampled envs' stacks are the luma of the oracle's last four frames outside its ambiguity masks"""
    torch = torch_cuda
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    O = oracle
    B, N, k, seed, steps = 4096, 2, 4, 21, 50
    env = VecMultiCarRacing(B, N, seed=seed, use_random_direction=False, obs_format="gray", frame_stack=k)
    env.reset()
    sample = [0, 1, 1777, 4095]
    orcs = []
    for e in sample:
        o = O.OracleEnv(N)
        o.reset(oracle_episode(O, N, seed, e))
        orcs.append(o)
    rng = np.random.RandomState(1)
    want = {e: [] for e in sample}
    for t in range(steps):
        a = rng.uniform(0, 1, (B, N, 3)).astype(np.float32)
        a[..., 0] = a[..., 0] * 2 - 1
        a[..., 2] *= 0.2
        obs, _, done, _ = env.step(torch.from_numpy(a).cuda())
        for e, o in zip(sample, orcs):
            oo, _, d, _ = o.step(a[e], render=t >= steps - k)
            assert not d
            if t >= steps - k:
                want[e].append((luma_np(oo), o.last_amb.copy()))
    assert not bool(done.any().item())
    got = obs.cpu().numpy()
    for e in sample:
        for i, (w, amb) in enumerate(want[e]):
            bad = int(((got[e, :, i] != w) & (amb == 0)).sum())
            assert bad == 0, f"env {e} stack frame {i}: {bad} unambiguous pixels differ from the oracle's luma"
    env.close()


def test_arguments(torch_cuda):
    from multi_car_racing_amd import _lib
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    torch = torch_cuda
    for kw in (dict(obs_format="rgb", frame_stack=2), dict(obs_format="gray", frame_stack=0), dict(obs_format="gray", frame_stack=9),
               dict(obs_format="bgr"), dict(obs_format="gray", obs=False), dict(obs_format="gray", frame_stack=2, obs=False),
               dict(obs_format="gray", frame_stack=4, max_episode_steps=3)):
        with pytest.raises(ValueError):
            VecMultiCarRacing(4, 2, **kw)
    ERR_ARG, ERR_STATE = -1, -3
    L = _lib.load()
    import ctypes
    for obs_enabled in (1, 0):
        cfg = _lib.Config(4, 2, 0, obs_enabled, 1, 1, 0, 1, 1000, 1, 0.25, 0, 0)
        h = ctypes.c_void_p()
        _lib.check(L.mcr_create(ctypes.byref(cfg), ctypes.byref(h)), "mcr_create")
        if obs_enabled:
            for fmt, st in ((2, 1), (-1, 1), (_lib.OBS_RGB, 2), (_lib.OBS_GRAY, 0), (_lib.OBS_GRAY, 9)):
                assert L.mcr_set_obs_format(h, fmt, st) == ERR_ARG, (fmt, st)
            assert L.mcr_obs_bytes_per_view(h) == 27648 and L.mcr_obs_window(h) == 0
            assert L.mcr_set_obs_format(h, _lib.OBS_GRAY, 1) == 0 and L.mcr_obs_bytes_per_view(h) == 9216 and L.mcr_obs_window(h) == 0
            assert L.mcr_set_obs_format(h, _lib.OBS_GRAY, 3) == 0 and L.mcr_obs_bytes_per_view(h) == 6 * 9216 and L.mcr_obs_window(h) == 3
            assert L.mcr_set_obs_format(h, _lib.OBS_RGB, 1) == 0 and L.mcr_obs_bytes_per_view(h) == 27648
        else:
            assert L.mcr_set_obs_format(h, _lib.OBS_GRAY, 1) == ERR_STATE
        L.mcr_destroy(h)
    env = VecMultiCarRacing(4, 2, seed=1, obs_format="gray", frame_stack=3, async_refill=False)
    env.reset()
    assert env.L.mcr_set_obs_format(env.h, _lib.OBS_GRAY, 2) == ERR_STATE          # after the first reset
    assert env.L.mcr_set_obs_format(env.h, _lib.OBS_RGB, 1) == ERR_STATE
    a = torch.zeros((4, 2, 3), dtype=torch.float32, device="cuda")
    # a stacked handle refuses a step without an observation buffer (the ring would get a hole)
    assert env.L.mcr_step(env.h, ctypes.c_void_p(a.data_ptr()), None, ctypes.c_void_p(env.reward.data_ptr()), ctypes.c_void_p(env.done.data_ptr()),
                          None, None) == ERR_ARG
    w0 = int(env.L.mcr_obs_window(env.h))
    env.step(a)
    assert int(env.L.mcr_obs_window(env.h)) == w0 % 3 + 1                     # the refused step did not advance the head
    env.close()
