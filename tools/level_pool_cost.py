#!/usr/bin/env python
"""What a level pool (VecMultiCarRacing(levels=K), csrc/k_pool.h) costs or saves a rollout, and that the feature costs nothing when off.

bench.py's stepping loop at its default configuration (B = 4096, N = 2, RGB observations; device-side synthetic actions, a warm-up, K timed
steps with the host at most 16 steps ahead) for three builds / settings, alternating, each in a fresh child process under its own time limit:
  parent   the parent commit's tree (--parent-tree DIR: a checkout of it, built in place), which has no `levels` keyword
  default  this tree, the host-staged path (the refill service generates and stages every episode)
  pool     this tree, levels=256: the device re-stages from the resident pool, no host work per step
in two phases: stagger=1 — bench.py's staggered TimeLimit pre-roll, ~4 envs re-spawn per step — and stagger=0 — every env in phase, so the
timed window holds the step in which all B envs re-spawn at once (the kernel's mass case).  Every run also reports the process's CPU-seconds
per wall-second over the timed window (all threads: the stepping thread, the refill service, the generators).  The spread of the repeated
`parent` runs is the noise `default` is held against.  Prints one JSON line per run and a summary; --out FILE keeps them.

    python tools/level_pool_cost.py --parent-tree build/parent --repeats 3 --out profiles/level_pool_cost.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/level_pool_cost.py --worker pool --steps 300      # the kernel's duration

A child that fails ends the whole measurement: nothing more is started on the device."""
import argparse
import json
import resource
import sys

import costlib


def worker(args):
    torch, VecMultiCarRacing = costlib.import_tree(args.parent_tree if args.worker == "parent" else costlib.ROOT)
    B, N, K = args.envs, args.agents, args.steps
    kw = {"levels": args.levels} if args.worker == "pool" else {}
    env = VecMultiCarRacing(B, N, seed=0, obs=True, auto_reset=True, use_random_direction=True, streams=2, async_refill=True, **kw)
    env.reset()
    next_actions = costlib.action_stream(env)
    step = lambda: env.step(next_actions())
    costlib.preroll(env, step, stagger_steps=1000 if args.stagger else 0, warmup=args.warmup)
    ru0 = resource.getrusage(resource.RUSAGE_SELF)
    elapsed = costlib.timed_steps(step, K)
    ru1 = resource.getrusage(resource.RUSAGE_SELF)
    cpu_s = (ru1.ru_utime - ru0.ru_utime) + (ru1.ru_stime - ru0.ru_stime)
    env.wait_refills()
    frozen = int(env.debug_counters()[3]); status = env.status_words()[:5].tolist()
    episodes, _ = env.rollout_stats()
    generated = int(env.episodes_generated)
    levels_seen = None if getattr(env, "level", None) is None else int(torch.unique(env.level).numel())
    env.close()
    print("RESULT " + json.dumps(dict(which=args.worker, stagger=args.stagger, envs=B, agents=N, steps=K, elapsed_s=elapsed, env_steps_per_s=B * K / elapsed,
                                      cpu_s_per_wall_s=cpu_s / elapsed, frozen_env_steps=frozen, status=status, episodes_finished=episodes,
                                      episodes_generated=generated, levels_in_play=levels_seen)), flush=True)


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worker", choices=["parent", "default", "pool"], default=None, help="run ONE measurement in this process")
    ap.add_argument("--stagger", type=int, default=1, help="1: bench.py's staggered pre-roll; 0: all envs in phase (the timed window holds the mass re-spawn)")
    ap.add_argument("--levels", type=int, default=256)
    ap.add_argument("--phases", default="1,0", help="stagger settings to measure")
    costlib.add_common_args(ap)
    return ap


def summarise(runs, which):
    summary = {}
    for stagger in sorted({r["stagger"] for r in runs}, reverse=True):
        for w in which:
            mine = [r for r in runs if r["stagger"] == stagger and r["which"] == w]
            c = sorted(r["cpu_s_per_wall_s"] for r in mine)
            summary[f"stagger={stagger} {w}"] = dict(costlib.median_triple(r["env_steps_per_s"] for r in mine), cpu_s_per_wall_s_median=round(c[len(c) // 2], 3))
    return summary


def main():
    args = parser().parse_args()
    if args.worker:
        return worker(args)
    which = (["parent"] if args.parent_tree else []) + ["default", "pool"]
    tail = ["--envs", str(args.envs), "--agents", str(args.agents), "--steps", str(args.steps), "--warmup", str(args.warmup)] \
        + (["--parent-tree", args.parent_tree] if args.parent_tree else [])
    # alternating: a drift of the machine hits all three alike
    jobs = [(f"{w} stagger={stagger}", ["--worker", w, "--stagger", str(stagger), "--levels", str(args.levels)] + tail, rep)
            for stagger in [int(v) for v in args.phases.split(",")] for rep in range(args.repeats) for w in which]
    runs = costlib.run_children(__file__, jobs, args.child_timeout)
    if runs is None:
        return 1
    summary = summarise(runs, which)
    costlib.finish(dict(steps=args.steps, envs=args.envs, agents=args.agents, levels=args.levels, runs=runs, summary=summary), summary, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
