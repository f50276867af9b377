"""MI355X: the stepping loop of tools/costlib.py (action_stream + preroll + timed_steps) against a literal restatement of the loop every
tools/*_cost.py carried before they shared it — two handles with the same keywords must end bit-equal — and one tool end to end."""
import json
import os
import subprocess
import sys
import time
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)

W, K = 4, 40                                                 # K > 2 * LOOKAHEAD: the query() poll of the fence is reached


def _make(B):
    """levels=4: no host thread has a say in the result; max_episode_steps=24: episodes end inside the run"""
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                      # (a second handle of a process orders its streams with events: the same results)
        env = VecMultiCarRacing(B, 2, seed=0, obs=False, auto_reset=True, use_random_direction=True, streams=2, levels=4, max_episode_steps=24)
    env.reset()
    return env


def reference_loop(torch, env, L, W, K, actions="random", calls=1):
    """tools/state_obs_cost.py's loop as it stood before tools/costlib.py, `L` a parameter; actions="drive" adds tools/contact_obs_cost.py's
    three in-place lines, calls=2 is tools/frame_skip_cost.py's parent leg (step() twice per policy step with the same actions)"""
    B, N = env.B, env.N
    dev = env.device
    g = torch.Generator(device=dev); g.manual_seed(1234)
    ACT_BLOCK = 16
    act = [torch.empty((ACT_BLOCK, B, N, 3), dtype=torch.float32, device=dev) for _ in range(2)]
    tstep = [0]

    def next_actions():
        t = tstep[0]; tstep[0] += 1
        blk, j = divmod(t, ACT_BLOCK)
        if j == 0:
            env.synth_actions(t, seed=1234, out=act[blk & 1], steps=ACT_BLOCK)
            if actions == "drive":
                a = act[blk & 1]
                a[..., 0].mul_(0.1); a[..., 1].fill_(1.0); a[..., 2].zero_()
        return act[blk & 1][j]

    def policy_step():
        a = next_actions()
        for _ in range(calls):
            env.step(a)
    ids = torch.randperm(B, device=dev, generator=g)
    for j in range(L):
        policy_step()
        msk = ((ids * L) // B == j).to(torch.uint8)
        if bool(msk.any()):
            env.reset_envs(msk)
    for k in range(W):
        policy_step()
    env.wait_refills()
    torch.cuda.synchronize()
    LOOKAHEAD = 16; FENCE = LOOKAHEAD // 4
    evs = [torch.cuda.Event(blocking=True) for _ in range(4)]
    t0 = time.perf_counter()
    for k in range(K):
        policy_step()
        if k % FENCE == FENCE - 1:
            j = (k // FENCE) % 4
            if k >= LOOKAHEAD:
                while not evs[j].query():
                    time.sleep(1e-4)
            evs[j].record()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def shared_loop(env, L, W, K, actions="random", calls=1):
    import costlib
    next_actions = costlib.action_stream(env, mode=actions)
    if calls == 1:
        step = lambda: env.step(next_actions())
    else:
        def step():
            a = next_actions()
            for _ in range(calls):
                env.step(a)
    costlib.preroll(env, step, stagger_steps=L, warmup=W)
    return costlib.timed_steps(step, K)


def _readout(torch, env):
    torch.cuda.synchronize()
    out = {k: getattr(env, k).cpu().numpy().copy() for k in ("reward", "done", "truncated", "episode_return", "episode_length", "level")}
    out.update({"state." + k: v for k, v in env.get_env_state().items()})
    out["rollout_stats"] = np.array(env.rollout_stats())
    out["_step_idx"] = np.array(env._step_idx)
    out["status"] = env.status_words()[:5].copy()
    return out


@pytest.mark.parametrize("B, L, actions, calls", [
    (64, 16, "random", 1),        # every pre-roll step resets four envs
    (8, 16, "random", 1),         # half the pre-roll steps have an empty mask: `if msk.any()` not taken
    (64, 16, "drive", 1),
    (64, 8, "random", 2),         # frame_skip_cost.py's parent leg, k = 2, L = 8 policy steps
])
def test_shared_loop_is_the_parents_loop(B, L, actions, calls):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    got = []
    for loop in (lambda e: reference_loop(torch, e, L, W, K, actions, calls), lambda e: shared_loop(e, L, W, K, actions, calls)):
        env = _make(B)
        try:
            assert loop(env) > 0.0
            got.append(_readout(torch, env))
        finally:
            env.close()
    ref, new = got
    assert sorted(ref) == sorted(new)
    (episodes, returns), (episodes_new, returns_new) = ref.pop("rollout_stats"), new.pop("rollout_stats")
    for k in ref:
        assert ref[k].dtype == new[k].dtype and ref[k].tobytes() == new[k].tobytes(), k
    assert int(ref["_step_idx"]) == int(new["_step_idx"]) == calls * (L + W + K)
    assert not ref["status"].any() and not new["status"].any()
    assert episodes == episodes_new and episodes > 0         # (episodes did end inside the run: the comparison covers re-spawns)
    # The sum of returns is the one read-out that is not a function of the rollout alone: k_dynamics adds every ended episode's return per
    # car with an f64 atomicAdd, in the order the hardware serves the lanes, so two runs of the SAME loop differ in its last bit now and then
    # (measured: 2 of 48 runs at B = 64, L = 8, two steps per call; every other read-out identical in all 48).  Both figures are sums of the
    # same n = 2 * episodes terms in two orders: each is within (n - 1) * 2^-53 * sum|x| of the exact sum, and |x| <= 1000 + 0.1 * 24 (all
    # tiles of a track are worth 1000, a step costs 0.1, an episode here has at most 24 steps).
    n = 2 * episodes
    assert abs(returns - returns_new) <= 2 * (n - 1) * 2.0 ** -53 * n * (1000 + 0.1 * 24)


def test_state_obs_cost_end_to_end(tmp_path):
    out = tmp_path / "cost.json"
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(TOOLS, "state_obs_cost.py"), "--envs", "64", "--steps", "48", "--warmup", "4",
           "--repeats", "1", "--configs", "0", "--child-timeout", "120", "--out", str(out)]
    pr = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert pr.returncode == 0, pr.stdout[-4000:]
    with open(out) as f:
        rec = json.load(f)
    assert [r["which"] for r in rec["runs"]] == ["off", "on"]
    assert rec["runs"][1]["state_written"] is True
    assert list(rec["summary"]) == ["obs=0 off", "obs=0 on"]
