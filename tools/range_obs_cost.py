#!/usr/bin/env python
"""What the range-finder observation (VecMultiCarRacing(range_obs=True), csrc/k_rangeobs.h) costs a rollout.

bench.py's stepping loop (device-side synthetic actions, the staggered TimeLimit pre-roll, a warm-up, K timed steps with the host at most
16 steps ahead) for three builds / settings, alternating, each in a fresh child process under its own time limit:
  parent   the parent commit's tree (--parent-tree DIR: a checkout of it, built in place), which has no range_obs keyword
  off      this tree, range_obs=False
  on       this tree, range_obs=True (the default 19 rays over a half circle, range_max 100)
at two configurations: BASELINE configs[4] (B = 4096, N = 2, obs = False) and configs[1] (the same with RGB observations).  The spread of the
repeated `parent` runs is the noise `off` is held against (the summary says whether `off`'s median lies within it).  Prints one JSON line per
run and a summary; --out FILE keeps them.

    python tools/range_obs_cost.py --parent-tree build/parent --repeats 3 --out profiles/range_obs_cost.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/range_obs_cost.py --worker on --obs 0 --steps 300      # k_rangeobs' duration; with
                                                                            # --state-obs 1 next to k_stateobs' in the same trace
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/range_obs_cost.py --worker off --obs 0 --steps 300     # no k_rangeobs launch

A child that fails ends the whole measurement: nothing more is started on the device."""
import argparse
import json
import sys

import costlib


def worker(args):
    torch, VecMultiCarRacing = costlib.import_tree(args.parent_tree if args.worker == "parent" else costlib.ROOT)
    B, N, K = args.envs, args.agents, args.steps
    kw = {} if args.worker == "parent" else {"range_obs": args.worker == "on"}
    if args.state_obs:
        kw["state_obs"] = True
    env = VecMultiCarRacing(B, N, seed=0, obs=bool(args.obs), auto_reset=True, use_random_direction=True, streams=2, async_refill=True, **kw)
    env.reset()
    next_actions = costlib.action_stream(env)
    step = lambda: env.step(next_actions())
    costlib.preroll(env, step, warmup=args.warmup)
    elapsed = costlib.timed_steps(step, K)
    env.wait_refills()
    frozen = int(env.debug_counters()[3]); status = env.status_words()[:5].tolist()
    nz = None if getattr(env, "ranges", None) is None else bool((env.ranges != 0).any().item())
    env.close()
    print("RESULT " + json.dumps(dict(which=args.worker, obs=args.obs, envs=B, agents=N, steps=K, elapsed_s=elapsed, env_steps_per_s=B * K / elapsed,
                                      frozen_env_steps=frozen, status=status, ranges_written=nz)), flush=True)


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worker", choices=["parent", "off", "on"], default=None, help="run ONE measurement in this process")
    ap.add_argument("--obs", type=int, default=0)
    ap.add_argument("--state-obs", type=int, default=0, help="1: state_obs=True as well (kernel traces: k_stateobs beside k_rangeobs)")
    ap.add_argument("--configs", default="0,1", help="obs settings to measure: 0 = BASELINE configs[4], 1 = configs[1]")
    costlib.add_common_args(ap)
    return ap


def summarise(runs, which):
    summary = {}
    for obs in sorted({r["obs"] for r in runs}):
        for w in which:
            summary[f"obs={obs} {w}"] = costlib.median_triple(r["env_steps_per_s"] for r in runs if r["obs"] == obs and r["which"] == w)
    for obs in sorted({r["obs"] for r in runs}):         # `off` against the parent's own run-to-run spread
        pa, of = summary.get(f"obs={obs} parent"), summary.get(f"obs={obs} off")
        if pa and of:
            of["vs_parent_median_pct"] = round(100.0 * (of["median"] - pa["median"]) / pa["median"], 2)
            # the off-path yardstick, ONE-sided: no slower than the parent's slowest run (grid_obs_cost.py has the same; end_rules_cost.py's
            # `off inside parent range` is two-sided: slowest <= median <= fastest)
            of["within_parent_spread"] = bool(of["median"] >= pa["runs"][0])
        on = summary.get(f"obs={obs} on")
        if on and of:
            on["vs_off_median_pct"] = round(100.0 * (on["median"] - of["median"]) / of["median"], 2)
    return summary


def main():
    args = parser().parse_args()
    if args.worker:
        return worker(args)
    which = (["parent"] if args.parent_tree else []) + ["off", "on"]
    tail = ["--envs", str(args.envs), "--agents", str(args.agents), "--steps", str(args.steps), "--warmup", str(args.warmup)] \
        + (["--parent-tree", args.parent_tree] if args.parent_tree else [])
    # alternating: a drift of the machine hits all three alike
    jobs = [(f"{w} obs={obs}", ["--worker", w, "--obs", str(obs), "--state-obs", str(args.state_obs)] + tail, rep)
            for obs in [int(v) for v in args.configs.split(",")] for rep in range(args.repeats) for w in which]
    runs = costlib.run_children(__file__, jobs, args.child_timeout)
    if runs is None:
        return 1
    summary = summarise(runs, which)
    costlib.finish(dict(steps=args.steps, envs=args.envs, agents=args.agents, runs=runs, summary=summary), summary, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
