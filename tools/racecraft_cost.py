#!/usr/bin/env python
"""What racecraft (VecMultiCarRacing(scripted_agents=(1,), racecraft=True), csrc/k_driver.h: k_driver<true>) costs a rollout, and what it
changes about the workload.

tools/driver_cost.py's loop (device-side synthetic actions, the staggered TimeLimit pre-roll, a warm-up, K timed steps with the host at most
16 steps ahead) for four builds / settings, alternating, each in a fresh child process under its own time limit:
  parent   the parent commit's tree (--parent-tree DIR: a checkout of it, built in place), which has no racecraft keyword; no drivers
  off      this tree without drivers, fed the same pre-made action tensor
  drv      this tree, scripted_agents=(1,), racecraft off: the plain controller (k_driver<false>)
  on       this tree, scripted_agents=(1,), racecraft=True (k_driver<true>)
at two configurations: BASELINE configs[4] (B = 4096, N = 2, obs = False) and configs[1] (the same with RGB observations).  The spread of
the repeated `parent` runs is the noise `off` is held against.  Every run also reports the share of its timed env-steps that went through
the contact chain (mcr_debug_read_counters [2]: contact envs routed to the side stream): `drv` and `on` are different WORKLOADS — an
opponent that rams against one that goes round.  Prints one JSON line per run and a summary; --out FILE keeps them.

    python tools/racecraft_cost.py --parent-tree build/parent --repeats 3 --out profiles/racecraft_cost.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/racecraft_cost.py --worker trace --steps 300    # k_driver<true>, k_driver<false>, k_stateobs in one trace
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/racecraft_cost.py --worker drv --steps 300      # racecraft off: the old instantiation alone

A child that fails ends the whole measurement: nothing more is started on the device."""
import argparse
import json
import sys

import costlib

KW = {"parent": {}, "off": {}, "drv": {"scripted_agents": (1,)}, "on": {"scripted_agents": (1,), "racecraft": True}}


def _rollout(env, K, W):
    next_actions = costlib.action_stream(env)
    step = lambda: env.step(next_actions())
    costlib.preroll(env, step, warmup=W)
    c0 = env.debug_counters()
    elapsed = costlib.timed_steps(step, K)
    env.wait_refills()
    c1 = env.debug_counters()
    return elapsed, int(c1[2]) - int(c0[2]), int(c1[3])


def worker(args):
    torch, VecMultiCarRacing = costlib.import_tree(args.parent_tree if args.worker == "parent" else costlib.ROOT)
    B, N, K, W = args.envs, args.agents, args.steps, args.warmup
    common = dict(seed=0, obs=bool(args.obs), auto_reset=True, use_random_direction=True, streams=2, async_refill=True)
    if args.worker == "trace":                          # for the kernel trace alone: both instantiations and k_stateobs in one process
        for kw in (dict(KW["on"], state_obs=True), KW["drv"]):
            env = VecMultiCarRacing(B, N, **common, **kw)
            env.reset()
            _rollout(env, K, W)
            env.close()
        print("RESULT " + json.dumps(dict(which="trace", steps=K)), flush=True)
        return
    env = VecMultiCarRacing(B, N, **common, **KW[args.worker])
    env.reset()
    elapsed, contact_envs, frozen = _rollout(env, K, W)
    status = env.status_words()[:5].tolist()
    nz = None if getattr(env, "actions", None) is None else bool((env.actions[:, 1] != 0).any().item())
    env.close()
    print("RESULT " + json.dumps(dict(which=args.worker, obs=args.obs, envs=B, agents=N, steps=K, elapsed_s=elapsed, env_steps_per_s=B * K / elapsed,
                                      contact_env_steps=contact_envs, contact_share=contact_envs / float(B * K),
                                      frozen_env_steps=frozen, status=status, driver_rows_written=nz)), flush=True)


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worker", choices=["parent", "off", "drv", "on", "trace"], default=None, help="run ONE measurement in this process")
    ap.add_argument("--obs", type=int, default=0)
    ap.add_argument("--configs", default="0,1", help="obs settings to measure: 0 = BASELINE configs[4], 1 = configs[1]")
    costlib.add_common_args(ap)
    return ap


def summarise(runs, which):
    summary = {}
    for obs in sorted({r["obs"] for r in runs}):
        for w in which:
            mine = [r for r in runs if r["obs"] == obs and r["which"] == w]
            share = sorted(r["contact_share"] for r in mine)
            summary[f"obs={obs} {w}"] = dict(costlib.median_triple(r["env_steps_per_s"] for r in mine), contact_share_median=round(share[len(share) // 2], 5))
    return summary


def main():
    args = parser().parse_args()
    if args.worker:
        return worker(args)
    which = (["parent"] if args.parent_tree else []) + ["off", "drv", "on"]
    tail = ["--envs", str(args.envs), "--agents", str(args.agents), "--steps", str(args.steps), "--warmup", str(args.warmup)] \
        + (["--parent-tree", args.parent_tree] if args.parent_tree else [])
    # alternating: a drift of the machine hits all of them alike
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
