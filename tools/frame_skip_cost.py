#!/usr/bin/env python
"""What an action repeat costs with and without VecMultiCarRacing(frame_skip=k) (include/mcr.h: mcr_step_repeat).

bench.py's stepping loop (device-side synthetic actions, a staggered TimeLimit pre-roll, a warm-up, timed policy steps with the host at most
16 policy steps ahead), one measurement per fresh child process under its own time limit, alternating, medians of --repeats runs:
  (a) parent4 / parent8   the parent commit's tree (--parent-tree DIR: a checkout of it, built in place) calling step() 4 / 8 times per
                          policy step with the same actions, drawing every time — what a user does today (and gets other semantics for:
                          no per-env break, a stack of sub-step frames); the only thing the new path is compared against
  (b) parent1 / skip1     the parent's plain step beside this tree's frame_skip=1; the spread of the repeated parent1 runs is the noise
  (c) skip4 / skip8       this tree, frame_skip=4 / 8
at two configurations: B = 4096, N = 2 with RGB observations (`rgb`) and with gray observations, frame_stack=4 (`gray4`).  Reports
policy-steps/s and env-steps/s (= envs x env steps per policy step x policy-steps/s).  Prints one JSON line per run and a summary; --out FILE
keeps them.

    python tools/frame_skip_cost.py --parent-tree build/parent --repeats 3 --out profiles/frame_skip_cost.json

A child that fails ends the whole measurement: nothing more is started on the device."""
import argparse
import json
import sys

import costlib

WORKERS = {"parent1": ("parent", 1), "parent4": ("parent", 4), "parent8": ("parent", 8), "skip1": ("this", 1), "skip4": ("this", 4), "skip8": ("this", 8)}
CONFIGS = {"rgb": dict(obs_format="rgb", frame_stack=1), "gray4": dict(obs_format="gray", frame_stack=4)}


def worker(args):
    side, k = WORKERS[args.worker]
    torch, VecMultiCarRacing = costlib.import_tree(args.parent_tree if side == "parent" else costlib.ROOT)
    B, N = args.envs, args.agents
    kw = dict(CONFIGS[args.config])
    if side == "this":
        kw["frame_skip"] = k
    env = VecMultiCarRacing(B, N, seed=0, obs=True, auto_reset=True, use_random_direction=True, streams=2, async_refill=True, **kw)
    env.reset()
    calls = k if side == "parent" else 1                # step() calls per policy step
    next_actions = costlib.action_stream(env)

    def policy_step():
        a = next_actions()
        for _ in range(calls):
            env.step(a)
    # bench.py's stagger in policy steps: every env reset once, at a step of its own, before anything is timed
    costlib.preroll(env, policy_step, stagger_steps=(1000 + k - 1) // k, warmup=max(1, args.warmup // k))
    K = max(1, args.steps // k)                         # timed policy steps
    elapsed = costlib.timed_steps(policy_step, K)
    env.wait_refills()
    frozen = int(env.debug_counters()[3]); status = env.status_words()[:5].tolist()
    env.close()
    print("RESULT " + json.dumps(dict(which=args.worker, config=args.config, envs=B, agents=N, env_steps_per_policy_step=k, policy_steps=K, elapsed_s=elapsed,
                                      policy_steps_per_s=K / elapsed, env_steps_per_s=B * K * k / elapsed, frozen_env_steps=frozen, status=status)), flush=True)


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worker", choices=sorted(WORKERS), default=None, help="run ONE measurement in this process")
    ap.add_argument("--config", choices=sorted(CONFIGS), default="rgb")
    ap.add_argument("--configs", default="rgb,gray4")
    costlib.add_common_args(ap, steps=2000)             # timed ENV steps per run (policy steps: steps // k)
    return ap


def summarise(runs, which, configs):
    summary = {}
    for cfg in configs:
        for w in which:
            sel = [r for r in runs if r["config"] == cfg and r["which"] == w]
            t = costlib.median_triple(r["env_steps_per_s"] for r in sel); p = sorted(r["policy_steps_per_s"] for r in sel)
            summary[f"{cfg} {w}"] = dict(env_steps_per_s_runs=t["runs"], env_steps_per_s_median=t["median"],
                                         policy_steps_per_s_median=round(p[len(p) // 2], 1), spread_pct=t["spread_pct"])
    return summary


def main():
    args = parser().parse_args()
    if args.worker:
        return worker(args)
    which = [w for w in ("parent1", "skip1", "parent4", "skip4", "parent8", "skip8") if args.parent_tree or not w.startswith("parent")]
    configs = args.configs.split(",")
    tail = ["--envs", str(args.envs), "--agents", str(args.agents), "--steps", str(args.steps), "--warmup", str(args.warmup)] \
        + (["--parent-tree", args.parent_tree] if args.parent_tree else [])
    # alternating: a drift of the machine hits all of them alike
    jobs = [(f"{w} config={cfg}", ["--worker", w, "--config", cfg] + tail, rep) for cfg in configs for rep in range(args.repeats) for w in which]
    runs = costlib.run_children(__file__, jobs, args.child_timeout)
    if runs is None:
        return 1
    summary = summarise(runs, which, configs)
    costlib.finish(dict(env_steps_timed=args.steps, envs=args.envs, agents=args.agents, runs=runs, summary=summary), summary, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
