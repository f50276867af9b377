#!/usr/bin/env python
"""What the level curricula (VecMultiCarRacing(level_stats=True) / level_order="weighted"; csrc/k_levelstats.h, csrc/k_pool.h) cost a rollout,
and that they cost nothing when off.

bench.py's stepping loop (B = 4096, N = 2, levels=256; device-side synthetic actions, the staggered TimeLimit pre-roll, a warm-up, K timed
steps with the host at most 16 steps ahead), physics only and with RGB observations, for four builds / settings, alternating, each in a
fresh child process under its own time limit:
  parent    the parent commit's tree (--parent-tree DIR: a checkout of it, built in place): levels=256, level_order="random"
  off       this tree, the same call: no new keyword, no new launch
  stats     this tree, level_stats=True
  weighted  this tree, level_order="weighted" (uniform weights until step 0 of the timed window, then a fixed non-uniform vector)
The spread of the repeated `parent` runs is the noise `off` is held against (1); `stats` and `weighted` are held against `off` (2).
Prints one JSON line per run and a summary of medians; --out FILE keeps them.

    python tools/level_stats_cost.py --parent-tree build/parent --repeats 3 --out profiles/level_stats_cost.json

(3) kernel durations come from a trace run of their own — one worker, both features on, next to k_pool_restage, k_stateobs and k_flags:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/level_stats_cost.py --worker both --state-obs 1 --steps 300            # steady state
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/level_stats_cost.py --worker both --state-obs 1 --stagger 0 --warmup 0 --steps 1000
                                                                  # no stagger: step 999 of the window is the one in which all 4096 envs end

A child that fails ends the whole measurement: nothing more is started on the device."""
import argparse
import json
import sys

import costlib

WORKERS = ["parent", "off", "stats", "weighted", "both"]


def worker(args):
    torch, VecMultiCarRacing = costlib.import_tree(args.parent_tree if args.worker == "parent" else costlib.ROOT)
    B, N, K = args.envs, args.agents, args.steps
    kw = {}
    if args.worker in ("stats", "both"):
        kw["level_stats"] = True
    if args.worker in ("weighted", "both"):
        kw["level_order"] = "weighted"
    if args.state_obs:
        kw["state_obs"] = True
    env = VecMultiCarRacing(B, N, seed=0, obs=bool(args.obs), auto_reset=True, use_random_direction=True, streams=2, levels=args.levels, **kw)
    env.reset()
    next_actions = costlib.action_stream(env)
    step = lambda: env.step(next_actions())
    # (preroll's wait_refills() in front of the timed region, which this tool alone did without, returns at once here: with a level pool —
    # and this tool always has one — there is neither a refill service nor a queue to wait for)
    costlib.preroll(env, step, stagger_steps=1000 if args.stagger else 0, warmup=args.warmup)
    if "level_order" in kw:                             # device weights, no synchronisation: what a learner's update would enqueue
        env.set_level_weights(1.0 + torch.arange(args.levels, dtype=torch.float64, device=env.device) % 7, check=False)
        torch.cuda.synchronize()                        # (the tool's own: the upload is drained before the clock starts)
    elapsed = costlib.timed_steps(step, K)
    episodes, _ = env.rollout_stats()
    counted = None if getattr(env, "level_stats", None) is None else float(env.level_stats[:, 0].sum().item())
    levels_seen = int(torch.unique(env.level).numel())
    env.close()
    print("RESULT " + json.dumps(dict(which=args.worker, obs=args.obs, stagger=args.stagger, envs=B, agents=N, steps=K, elapsed_s=elapsed,
                                      env_steps_per_s=B * K / elapsed, episodes_finished=episodes, episodes_in_level_stats=counted,
                                      levels_in_play=levels_seen)), flush=True)


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worker", choices=WORKERS, default=None, help="run ONE measurement in this process")
    ap.add_argument("--stagger", type=int, default=1, help="1: bench.py's staggered pre-roll; 0: all envs in phase (they all end in step 999, 1999, ...)")
    ap.add_argument("--obs", type=int, default=1, help="worker: 1 RGB observations, 0 physics only")
    ap.add_argument("--state-obs", type=int, default=0, help="worker: 1 adds state_obs=True (k_stateobs in the same trace)")
    ap.add_argument("--levels", type=int, default=256)
    ap.add_argument("--obs-settings", default="0,1", help="obs settings to measure: 0 physics only, 1 RGB")
    costlib.add_common_args(ap)
    return ap


def summarise(runs, which):
    summary = {}
    for obs in sorted({r["obs"] for r in runs}):
        for w in which:
            summary[f"obs={obs} {w}"] = costlib.median_triple(r["env_steps_per_s"] for r in runs if r["obs"] == obs and r["which"] == w)
        base = summary[f"obs={obs} off"]["median"]
        for w in which:
            summary[f"obs={obs} {w}"]["vs_off_pct"] = round(100.0 * (summary[f"obs={obs} {w}"]["median"] - base) / base, 2)
    return summary


def main():
    args = parser().parse_args()
    if args.worker:
        return worker(args)
    which = (["parent"] if args.parent_tree else []) + ["off", "stats", "weighted"]
    tail = ["--envs", str(args.envs), "--agents", str(args.agents), "--steps", str(args.steps), "--warmup", str(args.warmup)] \
        + (["--parent-tree", args.parent_tree] if args.parent_tree else [])
    # alternating: a drift of the machine hits all alike
    jobs = [(f"{w} obs={obs}", ["--worker", w, "--obs", str(obs), "--stagger", str(args.stagger), "--levels", str(args.levels)] + tail, rep)
            for obs in [int(v) for v in args.obs_settings.split(",")] for rep in range(args.repeats) for w in which]
    runs = costlib.run_children(__file__, jobs, args.child_timeout)
    if runs is None:
        return 1
    summary = summarise(runs, which)
    costlib.finish(dict(steps=args.steps, envs=args.envs, agents=args.agents, levels=args.levels, stagger=args.stagger, runs=runs, summary=summary), summary, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
