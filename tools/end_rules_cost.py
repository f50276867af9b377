#!/usr/bin/env python
"""What early episode ending (VecMultiCarRacing(end_patience=...), csrc/k_endrules.h) costs a rollout — and what it buys.

bench.py's stepping loop (device-side synthetic actions, the staggered TimeLimit pre-roll, a warm-up, K timed steps with the host at most
16 steps ahead) for three builds / settings, alternating, each in a fresh child process under its own time limit:
  parent   the parent commit's tree (--parent-tree DIR: a checkout of it, built in place), which has no end_* keywords
  off      this tree, every end_* keyword at its default
  on       this tree, end_patience=100
at two configurations: B = 4096, N = 2 physics only (`obs0`) and the same with RGB observations (`obs1`).  The yardstick for `off` is the
PARENT: its median must lie inside the range of the parent's own repeated runs of the same session (`off inside parent range` in the
summary).  Every run also reports the figure that motivates the feature: the share of env-steps, under random actions, in which at least
one counted car has a wheel on a tile (state feature 8-11 of k_stateobs, sampled over 256 steps behind the timed region with a state_obs
twin of the same setting) — with and without end_patience=100.  Prints one JSON line per run and a summary; --out FILE keeps them.  Where the
off median lies outside the parent's range the tool prints a FAIL line per configuration and exits with 2 (the file is still written).

    python tools/end_rules_cost.py --parent-tree build/parent --repeats 3 --out profiles/end_rules_cost.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/end_rules_cost.py --worker on --config obs0 --siblings 1 --steps 300     # k_endrules next to k_contactobs / k_stateobs -> profiles/end_rules_kernel_stats.csv
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python bench.py --gpus 1 --steps 100 --warmup 16                                   # feature off: no k_endrules launch -> profiles/end_rules_off_kernel_stats.csv

A child that fails ends the whole measurement: nothing more is started on the device."""
import argparse
import json
import sys

import costlib

CONFIGS = {"obs0": (0, "random"), "obs1": (1, "random")}


def worker(args):
    torch, VecMultiCarRacing = costlib.import_tree(args.parent_tree if args.worker == "parent" else costlib.ROOT)
    B, N, K = args.envs, args.agents, args.steps
    obs, actions = CONFIGS[args.config]
    on = {"end_patience": args.patience} if args.worker == "on" else {}
    kw = dict(on)
    if args.siblings:                                   # (kernel traces) the other per-step derived-output kernels in the same trace: k_contactobs, k_stateobs
        kw.update(state_obs=True, contact_obs=True)
    env = VecMultiCarRacing(B, N, seed=0, obs=bool(obs), auto_reset=True, use_random_direction=True, streams=2, async_refill=True, **kw)
    env.reset()
    next_actions = costlib.action_stream(env)
    step = lambda: env.step(next_actions())
    costlib.preroll(env, step, warmup=args.warmup)
    elapsed = costlib.timed_steps(step, K)
    env.wait_refills()
    frozen = int(env.debug_counters()[3]); status = env.status_words()[:5].tolist()
    forced = None
    if getattr(env, "end_reason", None) is not None:    # (outside the timed region) forced ends per step over 64 more steps
        n = 0
        for k in range(64):
            step()
            n += int((env.end_reason != 0).sum().item())
        forced = n / 64.0
    env.close()
    # (outside the timed region) the share of env-steps with a counted car on the road: a state_obs twin of the same setting, physics only,
    # from reset() through one TimeLimit and 256 sampled steps (the parent has the state vector too: its share is the "without" figure)
    twin = VecMultiCarRacing(B, N, seed=0, obs=False, auto_reset=True, use_random_direction=True, streams=2, async_refill=True, state_obs=True, **on)
    twin.reset()
    twin_actions = costlib.action_stream(twin)          # (the twin's own stream, from step 0: `env` is closed)
    on_road = total = 0
    for k in range(1000 + 256):
        twin.step(twin_actions())
        if k >= 1000:
            on_road += int((twin.state[:, :, 8:12] != 0).any(dim=2).any(dim=1).sum().item()); total += B
    twin.wait_refills()
    twin.close()
    print("RESULT " + json.dumps(dict(which=args.worker, config=args.config, envs=B, agents=N, steps=K, elapsed_s=elapsed, env_steps_per_s=B * K / elapsed,
                                      frozen_env_steps=frozen, status=status, forced_ends_per_step=forced, on_road_share=on_road / total)), flush=True)


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worker", choices=["parent", "off", "on"], default=None, help="run ONE measurement in this process")
    ap.add_argument("--config", choices=sorted(CONFIGS), default="obs0", help="the worker's configuration")
    ap.add_argument("--siblings", type=int, default=0, help="worker: 1 = also state_obs=True and contact_obs=True (k_stateobs and k_contactobs in the same kernel trace)")
    ap.add_argument("--patience", type=int, default=100, help="end_patience of the `on` runs")
    ap.add_argument("--configs", default="obs0,obs1", help="configurations to measure")
    costlib.add_common_args(ap, child_timeout=240)
    return ap


def summarise(runs, which, configs):
    summary = {}
    for cfg in configs:
        for w in which:
            summary[f"{cfg} {w}"] = costlib.median_triple(r["env_steps_per_s"] for r in runs if r["config"] == cfg and r["which"] == w)
        off = summary[f"{cfg} off"]["median"]
        summary[f"{cfg} on vs off pct"] = round(100.0 * (summary[f"{cfg} on"]["median"] - off) / off, 2)
        if "parent" in which:
            par = summary[f"{cfg} parent"]
            summary[f"{cfg} off vs parent pct"] = round(100.0 * (off - par["median"]) / par["median"], 2)
            # THE off-path condition, TWO-sided: the parent's own run-to-run range, slowest <= median <= fastest (range_obs_cost.py's and
            # grid_obs_cost.py's `within_parent_spread` is one-sided: no slower than the parent's slowest run)
            summary[f"{cfg} off inside parent range"] = bool(par["runs"][0] <= off <= par["runs"][-1])
        for w in which:
            v = sorted(r["on_road_share"] for r in runs if r["config"] == cfg and r["which"] == w)
            summary[f"{cfg} {w} on-road share"] = round(v[len(v) // 2], 4)
    return summary


def verdict(summary, configs):
    """(exit code, FAIL lines): 2 and a line per configuration whose off median lies outside the parent's range, else 0 and none"""
    lines = []
    for cfg in configs:
        if summary.get(f"{cfg} off inside parent range") is False:
            par = summary[f"{cfg} parent"]["runs"]
            off = summary[f"{cfg} off"]["median"]
            lines.append(f"FAIL {cfg}: the off median {off} lies {'below' if off < par[0] else 'above'} the parent's own range {par[0]} .. {par[-1]}")
    return (2 if lines else 0), lines


def main():
    args = parser().parse_args()
    if args.worker:
        return worker(args)
    which = (["parent"] if args.parent_tree else []) + ["off", "on"]
    configs = args.configs.split(",")
    tail = ["--envs", str(args.envs), "--agents", str(args.agents), "--steps", str(args.steps), "--warmup", str(args.warmup)] \
        + (["--parent-tree", args.parent_tree] if args.parent_tree else [])
    # alternating: a drift of the machine hits all three alike
    jobs = [(f"{w} config={cfg}", ["--worker", w, "--config", cfg, "--patience", str(args.patience)] + tail, rep)
            for cfg in configs for rep in range(args.repeats) for w in which]
    runs = costlib.run_children(__file__, jobs, args.child_timeout)
    if runs is None:
        return 1
    summary = summarise(runs, which, configs)
    costlib.finish(dict(steps=args.steps, envs=args.envs, agents=args.agents, runs=runs, summary=summary), summary, args.out)
    code, lines = verdict(summary, configs)
    for line in lines:
        print(line, flush=True)
    return code


if __name__ == "__main__":
    sys.exit(main())
