#!/usr/bin/env python
"""What the state-vector observation (VecMultiCarRacing(state_obs=True), csrc/k_stateobs.h) costs a rollout.

bench.py's stepping loop (device-side synthetic actions, the staggered TimeLimit pre-roll, a warm-up, K timed steps with the host at most
16 steps ahead) for three builds / settings, alternating, each in a fresh child process under its own time limit:
  parent   the parent commit's tree (--parent-tree DIR: a checkout of it, built in place), which has no state_obs keyword
  off      this tree, state_obs=False
  on       this tree, state_obs=True
at two configurations: BASELINE configs[4] (B = 4096, N = 2, obs = False) and configs[1] (the same with RGB observations).  The spread of the
repeated `parent` runs is the noise `off` is held against.  Prints one JSON line per run and a summary; --out FILE keeps them.

    python tools/state_obs_cost.py --parent-tree build/parent --repeats 3 --out profiles/state_obs_cost.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/state_obs_cost.py --worker on --obs 0 --steps 300      # the kernel's duration

A child that fails ends the whole measurement: nothing more is started on the device."""
import argparse
import json
import sys

import costlib


def worker(args):
    torch, VecMultiCarRacing = costlib.import_tree(args.parent_tree if args.worker == "parent" else costlib.ROOT)
    B, N, K = args.envs, args.agents, args.steps
    kw = {} if args.worker == "parent" else {"state_obs": args.worker == "on"}
    env = VecMultiCarRacing(B, N, seed=0, obs=bool(args.obs), auto_reset=True, use_random_direction=True, streams=2, async_refill=True, **kw)
    env.reset()
    next_actions = costlib.action_stream(env)
    step = lambda: env.step(next_actions())
    costlib.preroll(env, step, warmup=args.warmup)
    elapsed = costlib.timed_steps(step, K)
    env.wait_refills()
    frozen = int(env.debug_counters()[3]); status = env.status_words()[:5].tolist()
    nz = None if getattr(env, "state", None) is None else bool((env.state != 0).any().item())
    env.close()
    print("RESULT " + json.dumps(dict(which=args.worker, obs=args.obs, envs=B, agents=N, steps=K, elapsed_s=elapsed, env_steps_per_s=B * K / elapsed,
                                      frozen_env_steps=frozen, status=status, state_written=nz)), flush=True)


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worker", choices=["parent", "off", "on"], default=None, help="run ONE measurement in this process")
    ap.add_argument("--obs", type=int, default=0)
    ap.add_argument("--configs", default="0,1", help="obs settings to measure: 0 = BASELINE configs[4], 1 = configs[1]")
    costlib.add_common_args(ap)
    return ap


def summarise(runs, which):
    summary = {}
    for obs in sorted({r["obs"] for r in runs}):
        for w in which:
            summary[f"obs={obs} {w}"] = costlib.median_triple(r["env_steps_per_s"] for r in runs if r["obs"] == obs and r["which"] == w)
    return summary


def main():
    args = parser().parse_args()
    if args.worker:
        return worker(args)
    which = (["parent"] if args.parent_tree else []) + ["off", "on"]
    tail = ["--envs", str(args.envs), "--agents", str(args.agents), "--steps", str(args.steps), "--warmup", str(args.warmup)] \
        + (["--parent-tree", args.parent_tree] if args.parent_tree else [])
    # alternating: a drift of the machine hits all three alike
    jobs = [(f"{w} obs={obs}", ["--worker", w, "--obs", str(obs)] + tail, rep)
            for obs in [int(v) for v in args.configs.split(",")] for rep in range(args.repeats) for w in which]
    runs = costlib.run_children(__file__, jobs, args.child_timeout)
    if runs is None:
        return 1
    summary = summarise(runs, which)
    costlib.finish(dict(steps=args.steps, envs=args.envs, agents=args.agents, runs=runs, summary=summary), summary, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
