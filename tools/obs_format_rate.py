"""Rate of the observation formats (include/mcr.h: mcr_set_obs_format) at B = 4096, N = 2 with bench.py's loop shape: synthetic device
actions, auto-reset, the native refill service, TimeLimit phases spread before timing, the host at most 16 steps ahead of the GPU.
One JSON line per leg:
  a  rgb                        what bench.py measures
  b  rgb + torch post-processing the same luma integers, then a k = 4 FrameStack by torch.cat (first frame k times where `done`)
  c  gray, k = 1                the raster writes luma
  d  gray, k = 4                ... into the ring of 2k frames per view
env_steps_per_s over the timed steps, raster_us: the main raster launch's dispatch duration (mcr_timing, every 8th step).

    python tools/obs_format_rate.py [--steps 2000] [--warmup 200] [--legs abcd]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def luma(torch, rgb):
    x = rgb.to(torch.int32)
    return ((4899 * x[..., 0] + 9617 * x[..., 1] + 1868 * x[..., 2] + 8192) >> 14).to(torch.uint8)


def run_leg(leg, B, N, K, W, stagger):
    import torch
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    fmt, k = {"a": ("rgb", 1), "b": ("rgb", 1), "c": ("gray", 1), "d": ("gray", 4)}[leg]
    env = VecMultiCarRacing(B, N, seed=0, use_random_direction=True, obs_format=fmt, frame_stack=k)
    env.reset()
    dev = env.device
    ACT_BLOCK = 16
    act = [torch.empty((ACT_BLOCK, B, N, 3), dtype=torch.float32, device=dev) for _ in range(2)]
    tstep = [0]

    def next_actions():
        t = tstep[0]; tstep[0] += 1
        blk, j = divmod(t, ACT_BLOCK)
        if j == 0:
            env.synth_actions(t, seed=0, out=act[blk & 1], steps=ACT_BLOCK)
        return act[blk & 1][j]

    stack = [None]

    def step():
        obs, rew, done, info = env.step(next_actions())
        if leg == "b":                                   # what a user does with the RGB frames to get gym's gray FrameStack(4)
            y = luma(torch, obs).unsqueeze(2)
            if stack[0] is None:
                stack[0] = y.repeat(1, 1, 4, 1, 1)
            s = torch.cat([stack[0][:, :, 1:], y], 2)
            stack[0] = torch.where(done.bool()[:, None, None, None, None], y.expand_as(s), s)
        return obs

    g = torch.Generator(device=dev); g.manual_seed(1234)
    if stagger:                                          # spread the TimeLimit phases (bench.py --stagger 1)
        L = 1000
        ids = torch.randperm(B, device=dev, generator=g)
        for j in range(L):
            step()
            msk = ((ids * L) // B == j).to(torch.uint8)
            if bool(msk.any()):
                env.reset_envs(msk)
                stack[0] = None
    for _ in range(W):
        step()
    env.wait_refills()
    env.timing(0)
    torch.cuda.synchronize()
    LOOKAHEAD, FENCE, TIME_EVERY = 16, 4, 8
    evs = [torch.cuda.Event(blocking=True) for _ in range(4)]
    t0 = time.perf_counter()
    for i in range(K):
        env.timing(4 if i % TIME_EVERY == 0 else 0)
        step()
        if i % FENCE == FENCE - 1:
            j = (i // FENCE) % 4
            if i >= LOOKAHEAD:
                while not evs[j].query():
                    time.sleep(1e-4)
            evs[j].record()
    torch.cuda.synchronize()
    env.wait_refills()
    elapsed = time.perf_counter() - t0
    ms, n = env.timing_read()
    env.timing(0)
    frozen = int(env.debug_counters()[3])
    env.close()
    name = {"a": "a_rgb", "b": "b_rgb_plus_torch_gray_stack4", "c": "c_gray_k1", "d": "d_gray_k4"}[leg]
    return {"leg": name, "B": B, "N": N, "steps": K, "env_steps_per_s": round(B * K / elapsed, 1), "step_ms": round(1e3 * elapsed / K, 4),
            "raster_us": round(1e3 * ms[2] / max(1, n[2]), 2), "raster_launches_timed": int(n[2]), "frozen_env_steps": frozen,
            "obs_bytes_per_view": 96 * 96 * 3 if leg in "ab" else 96 * 96 * (2 * 4 if leg == "d" else 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--agents", type=int, default=2)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--stagger", type=int, default=1)
    ap.add_argument("--legs", default="abcd")
    args = ap.parse_args()
    for leg in args.legs:
        print(json.dumps(run_leg(leg, args.envs, args.agents, args.steps, args.warmup, args.stagger)), flush=True)


if __name__ == "__main__":
    main()
