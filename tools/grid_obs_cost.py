#!/usr/bin/env python
"""What the grid observation (VecMultiCarRacing(grid_obs=True), csrc/k_gridobs.h) costs a rollout — and whether it is cheaper than the pixels
it can replace.

bench.py's stepping loop (device-side synthetic actions, the staggered TimeLimit pre-roll, a warm-up, K timed steps with the host at most
16 steps ahead) for three builds / settings, alternating, each in a fresh child process under its own time limit:
  parent   the parent commit's tree (--parent-tree DIR: a checkout of it, built in place), which has no grid_obs keyword
  off      this tree, grid_obs=False
  on       this tree, grid_obs=True (the defaults: 32 x 32 cells of 1.5, the car a quarter from the bottom)
at two configurations: BASELINE configs[4] (B = 4096, N = 2, obs = False) and configs[1] (the same with RGB observations).  The spread of the
repeated `parent` runs is the noise `off` is held against (the summary says whether `off`'s median lies within it), and `obs=0 on` — the grid
INSTEAD of the frame — is compared with `obs=1 parent`, the frame it can replace.  Prints one JSON line per run and a summary; --out FILE
keeps them.

    python tools/grid_obs_cost.py --parent-tree build/parent --repeats 3 --out profiles/grid_obs_cost.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/grid_obs_cost.py --worker on --obs 1 --others 1 --steps 300     # k_gridobs beside k_view,
                                                                            # k_rangeobs, k_stateobs and k_flags in one trace
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/grid_obs_cost.py --worker off --obs 1 --others 1 --steps 300    # no k_gridobs launch

A child that fails ends the whole measurement: nothing more is started on the device."""
import argparse
import json
import sys

import costlib


def worker(args):
    torch, VecMultiCarRacing = costlib.import_tree(args.parent_tree if args.worker == "parent" else costlib.ROOT)
    B, N, K = args.envs, args.agents, args.steps
    kw = {} if args.worker == "parent" else {"grid_obs": args.worker == "on"}
    if args.others:
        kw.update(state_obs=True, range_obs=True)
    env = VecMultiCarRacing(B, N, seed=0, obs=bool(args.obs), auto_reset=True, use_random_direction=True, streams=2, async_refill=True, **kw)
    env.reset()
    next_actions = costlib.action_stream(env)
    step = lambda: env.step(next_actions())
    costlib.preroll(env, step, stagger_steps=args.stagger, warmup=args.warmup)
    elapsed = costlib.timed_steps(step, K)
    env.wait_refills()
    frozen = int(env.debug_counters()[3]); status = env.status_words()[:5].tolist()
    grid = getattr(env, "grid", None)
    filled = None if grid is None else round(float((grid != 0).float().mean().item()), 4)      # share of cells with anything under them
    env.close()
    print("RESULT " + json.dumps(dict(which=args.worker, obs=args.obs, envs=B, agents=N, steps=K, elapsed_s=elapsed, env_steps_per_s=B * K / elapsed,
                                      frozen_env_steps=frozen, status=status, grid_filled=filled)), flush=True)


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worker", choices=["parent", "off", "on"], default=None, help="run ONE measurement in this process")
    ap.add_argument("--obs", type=int, default=0)
    ap.add_argument("--others", type=int, default=0, help="1: state_obs=True and range_obs=True as well (kernel traces: their kernels beside k_gridobs)")
    ap.add_argument("--stagger", type=int, default=1000, help="steps of the staggered pre-roll (0: none, every env in phase)")
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
            # the off-path yardstick, ONE-sided: no slower than the parent's slowest run (range_obs_cost.py has the same; end_rules_cost.py's
            # `off inside parent range` is two-sided: slowest <= median <= fastest)
            of["within_parent_spread"] = bool(of["median"] >= pa["runs"][0])
        on = summary.get(f"obs={obs} on")
        if on and of:
            on["vs_off_median_pct"] = round(100.0 * (on["median"] - of["median"]) / of["median"], 2)
    grid_only, pixels = summary.get("obs=0 on"), summary.get("obs=1 parent")
    if grid_only and pixels:                             # the grid instead of the frame, against the frame
        grid_only["vs_parent_rgb_median_pct"] = round(100.0 * (grid_only["median"] - pixels["median"]) / pixels["median"], 2)
        grid_only["faster_than_parent_rgb"] = bool(grid_only["median"] > pixels["median"])
    return summary


def main():
    args = parser().parse_args()
    if args.worker:
        return worker(args)
    which = (["parent"] if args.parent_tree else []) + ["off", "on"]
    tail = ["--envs", str(args.envs), "--agents", str(args.agents), "--steps", str(args.steps), "--warmup", str(args.warmup)] \
        + (["--parent-tree", args.parent_tree] if args.parent_tree else [])
    # alternating, the repeats outermost: a drift of the machine hits all of them alike
    jobs = [(f"{w} obs={obs}", ["--worker", w, "--obs", str(obs), "--stagger", str(args.stagger), "--others", str(args.others)] + tail, rep)
            for rep in range(args.repeats) for obs in [int(v) for v in args.configs.split(",")] for w in which]
    runs = costlib.run_children(__file__, jobs, args.child_timeout)
    if runs is None:
        return 1
    summary = summarise(runs, which)
    costlib.finish(dict(steps=args.steps, envs=args.envs, agents=args.agents, runs=runs, summary=summary), summary, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
