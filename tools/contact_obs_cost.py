#!/usr/bin/env python
"""What the car-contact observation (VecMultiCarRacing(contact_obs=True), csrc/k_contactobs.h) costs a rollout.

bench.py's stepping loop (device-side synthetic actions, the staggered TimeLimit pre-roll, a warm-up, K timed steps with the host at most
16 steps ahead) for three builds / settings, alternating, each in a fresh child process under its own time limit:
  parent   the parent commit's tree (--parent-tree DIR: a checkout of it, built in place), which has no contact_obs keyword
  off      this tree, contact_obs=False
  on       this tree, contact_obs=True
at three configurations: B = 4096, N = 2 physics only (`obs0`), the same with RGB observations (`obs1`), and RGB under bench.py's
`--actions drive` (`drive`: gas 1, no brake, steering noise +-0.1 — cars that run into each other, ~1000 envs with a touching pair at a
time: where the kernel's long path runs).  The spread of the repeated `parent` runs is the noise `off` is held against.  Prints one JSON
line per run and a summary; --out FILE keeps them.

    python tools/contact_obs_cost.py --parent-tree build/parent --repeats 3 --out profiles/contact_obs_cost.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/contact_obs_cost.py --worker on --config obs0 --siblings 1 --steps 300     # the kernel's duration, next to k_stateobs / k_levelstats
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/contact_obs_cost.py --worker on --config drive --siblings 1 --steps 300    # ... with ~1000 envs on its long path
    rocprofv3 --kernel-trace --stats -d DIR -- python bench.py --gpus 1 --steps 100 --warmup 16                            # feature off: no k_contactobs launch

A child that fails ends the whole measurement: nothing more is started on the device."""
import argparse
import json
import sys

import costlib

CONFIGS = {"obs0": (0, "random"), "obs1": (1, "random"), "drive": (1, "drive")}


def worker(args):
    torch, VecMultiCarRacing = costlib.import_tree(args.parent_tree if args.worker == "parent" else costlib.ROOT)
    B, N, K = args.envs, args.agents, args.steps
    obs, actions = CONFIGS[args.config]
    kw = {} if args.worker == "parent" else {"contact_obs": args.worker == "on"}
    if args.siblings:                                   # (kernel traces) the other derived-output kernels in the same trace: k_stateobs, k_levelstats
        kw.update(state_obs=True, levels=256, level_stats=True)
    env = VecMultiCarRacing(B, N, seed=0, obs=bool(obs), auto_reset=True, use_random_direction=True, streams=2, async_refill=True, **kw)
    env.reset()
    next_actions = costlib.action_stream(env, mode=actions)
    step = lambda: env.step(next_actions())
    costlib.preroll(env, step, warmup=args.warmup)
    elapsed = costlib.timed_steps(step, K)
    # (outside the timed region) 32 more steps: envs with a contact per step — the long path's share — by the observation and, as a
    # cross-check on this topology, by the manifold stores' own counts (mcr_debug_read_contact_counts)
    touching = by_store = None
    if getattr(env, "contact_mask", None) is not None:
        import ctypes
        import numpy as np
        touching, by_store = [], []
        counts = np.zeros(B, np.int32)
        for k in range(32):
            step()
            touching.append(int((env.contact_mask != 0).any(dim=1).sum().item()))
            assert env.L.mcr_debug_read_contact_counts(env.h, counts.ctypes.data_as(ctypes.c_void_p)) == 0
            by_store.append(int((counts > 0).sum()))
        assert touching == by_store, f"contact_mask names {touching} touching envs per step, the stores {by_store}"
        touching = sum(touching) / len(touching)
    env.wait_refills()
    frozen = int(env.debug_counters()[3]); status = env.status_words()[:5].tolist()
    env.close()
    print("RESULT " + json.dumps(dict(which=args.worker, config=args.config, envs=B, agents=N, steps=K, elapsed_s=elapsed, env_steps_per_s=B * K / elapsed,
                                      frozen_env_steps=frozen, status=status, envs_touching_per_step=touching)), flush=True)


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worker", choices=["parent", "off", "on"], default=None, help="run ONE measurement in this process")
    ap.add_argument("--config", choices=sorted(CONFIGS), default="obs0", help="the worker's configuration")
    ap.add_argument("--siblings", type=int, default=0, help="worker: 1 = also state_obs=True and levels=256, level_stats=True (k_stateobs and k_levelstats in the same kernel trace)")
    ap.add_argument("--configs", default="obs0,obs1,drive", help="configurations to measure")
    costlib.add_common_args(ap)
    return ap


def summarise(runs, which, configs):
    summary = {}
    for cfg in configs:
        for w in which:
            summary[f"{cfg} {w}"] = costlib.median_triple(r["env_steps_per_s"] for r in runs if r["config"] == cfg and r["which"] == w)
        off = summary[f"{cfg} off"]["median"]
        summary[f"{cfg} on vs off pct"] = round(100.0 * (summary[f"{cfg} on"]["median"] - off) / off, 2)
        if "parent" in which:
            par = summary[f"{cfg} parent"]["median"]
            summary[f"{cfg} off vs parent pct"] = round(100.0 * (off - par) / par, 2)
    return summary


def main():
    args = parser().parse_args()
    if args.worker:
        return worker(args)
    which = (["parent"] if args.parent_tree else []) + ["off", "on"]
    configs = args.configs.split(",")
    tail = ["--envs", str(args.envs), "--agents", str(args.agents), "--steps", str(args.steps), "--warmup", str(args.warmup)] \
        + (["--parent-tree", args.parent_tree] if args.parent_tree else [])
    # alternating: a drift of the machine hits all three alike
    jobs = [(f"{w} config={cfg}", ["--worker", w, "--config", cfg] + tail, rep) for cfg in configs for rep in range(args.repeats) for w in which]
    runs = costlib.run_children(__file__, jobs, args.child_timeout)
    if runs is None:
        return 1
    summary = summarise(runs, which, configs)
    costlib.finish(dict(steps=args.steps, envs=args.envs, agents=args.agents, runs=runs, summary=summary), summary, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
