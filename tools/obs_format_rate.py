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
import time

import costlib


def luma(torch, rgb):
    x = rgb.to(torch.int32)
    return ((4899 * x[..., 0] + 9617 * x[..., 1] + 1868 * x[..., 2] + 8192) >> 14).to(torch.uint8)


def run_leg(leg, B, N, K, W, stagger):
    torch, VecMultiCarRacing = costlib.import_tree(costlib.ROOT)
    fmt, k = {"a": ("rgb", 1), "b": ("rgb", 1), "c": ("gray", 1), "d": ("gray", 4)}[leg]
    env = VecMultiCarRacing(B, N, seed=0, use_random_direction=True, obs_format=fmt, frame_stack=k)
    env.reset()
    next_actions = costlib.action_stream(env, seed=0)
    stack = [None]
    TIME_EVERY = 8
    timed = [None]                                       # the timed region's step counter (None in front of it: no launch is timed)

    def step():
        if timed[0] is not None:
            env.timing(4 if timed[0] % TIME_EVERY == 0 else 0); timed[0] += 1
        obs, rew, done, info = env.step(next_actions())
        if leg == "b":                                   # what a user does with the RGB frames to get gym's gray FrameStack(4)
            y = luma(torch, obs).unsqueeze(2)
            if stack[0] is None:
                stack[0] = y.repeat(1, 1, 4, 1, 1)
            s = torch.cat([stack[0][:, :, 1:], y], 2)
            stack[0] = torch.where(done.bool()[:, None, None, None, None], y.expand_as(s), s)

    def drop_stack():
        stack[0] = None
    # spread the TimeLimit phases (bench.py --stagger 1)
    costlib.preroll(env, step, stagger_steps=1000 if stagger else 0, warmup=W, after_reset=drop_stack)
    env.timing(0)
    timed[0] = 0
    t0 = time.perf_counter()                             # the tool's own clock: its time includes the wait_refills() behind the loop
    costlib.fenced_steps(step, K)
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


def parser():
    ap = argparse.ArgumentParser()
    costlib.add_common_args(ap, steps=2000, warmup=200, child_timeout=None)
    ap.add_argument("--stagger", type=int, default=1)
    ap.add_argument("--legs", default="abcd")
    return ap


def main():
    args = parser().parse_args()
    for leg in args.legs:
        print(json.dumps(run_leg(leg, args.envs, args.agents, args.steps, args.warmup, args.stagger)), flush=True)


if __name__ == "__main__":
    main()
