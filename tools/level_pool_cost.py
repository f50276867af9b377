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
import os
import resource
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worker(args):
    tree = os.path.abspath(args.parent_tree) if args.worker == "parent" else ROOT
    sys.path.insert(0, tree)
    import torch
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    import multi_car_racing_amd
    assert os.path.abspath(os.path.dirname(os.path.dirname(multi_car_racing_amd.__file__))) == tree, "the package did not come from the tree asked for"
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path to time"
    B, N, K, W = args.envs, args.agents, args.steps, args.warmup
    kw = {"levels": args.levels} if args.worker == "pool" else {}
    env = VecMultiCarRacing(B, N, seed=0, obs=True, auto_reset=True, use_random_direction=True, streams=2, async_refill=True, **kw)
    env.reset()
    dev = env.device
    g = torch.Generator(device=dev); g.manual_seed(1234)
    ACT_BLOCK = 16
    act = [torch.empty((ACT_BLOCK, B, N, 3), dtype=torch.float32, device=dev) for _ in range(2)]
    tstep = [0]

    def next_actions():
        t = tstep[0]; tstep[0] += 1
        blk, j = divmod(t, ACT_BLOCK)
        if j == 0:
            env.synth_actions(t, seed=1234, out=act[blk & 1], steps=ACT_BLOCK)
        return act[blk & 1][j]
    L = 1000                                            # bench.py's stagger: every env reset once, at a step of its own, before anything is timed
    ids = torch.randperm(B, device=dev, generator=g)
    for j in range(L if args.stagger else 0):
        env.step(next_actions())
        msk = ((ids * L) // B == j).to(torch.uint8)
        if bool(msk.any()):
            env.reset_envs(msk)
    for k in range(W):
        env.step(next_actions())
    env.wait_refills()
    torch.cuda.synchronize()
    LOOKAHEAD = 16; FENCE = LOOKAHEAD // 4
    evs = [torch.cuda.Event(blocking=True) for _ in range(4)]
    ru0 = resource.getrusage(resource.RUSAGE_SELF)
    t0 = time.perf_counter()
    for k in range(K):
        env.step(next_actions())
        if k % FENCE == FENCE - 1:
            j = (k // FENCE) % 4
            if k >= LOOKAHEAD:
                while not evs[j].query():
                    time.sleep(1e-4)
            evs[j].record()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worker", choices=["parent", "default", "pool"], default=None, help="run ONE measurement in this process")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit (omit: the `parent` runs are left out)")
    ap.add_argument("--stagger", type=int, default=1, help="1: bench.py's staggered pre-roll; 0: all envs in phase (the timed window holds the mass re-spawn)")
    ap.add_argument("--levels", type=int, default=256)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--agents", type=int, default=2)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--phases", default="1,0", help="stagger settings to measure")
    ap.add_argument("--child-timeout", type=int, default=150)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    which = (["parent"] if args.parent_tree else []) + ["default", "pool"]
    runs = []
    for stagger in [int(v) for v in args.phases.split(",")]:
        for rep in range(args.repeats):
            for w in which:                              # alternating: a drift of the machine hits all three alike
                cmd = [sys.executable, os.path.abspath(__file__), "--worker", w, "--stagger", str(stagger), "--levels", str(args.levels), "--envs", str(args.envs), "--agents", str(args.agents),
                       "--steps", str(args.steps), "--warmup", str(args.warmup)] + (["--parent-tree", args.parent_tree] if args.parent_tree else [])
                pr = subprocess.run(["timeout", "-k", "10", str(args.child_timeout)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                line = [l for l in pr.stdout.splitlines() if l.startswith("RESULT ")]
                if pr.returncode != 0 or not line:
                    print(pr.stdout[-4000:])
                    print(f"child {w} stagger={stagger} ended with {pr.returncode}: nothing more is started", flush=True)
                    return 1
                r = json.loads(line[-1][7:]); r["repeat"] = rep
                runs.append(r); print(json.dumps(r), flush=True)
    summary = {}
    for stagger in sorted({r["stagger"] for r in runs}, reverse=True):
        for w in which:
            mine = [r for r in runs if r["stagger"] == stagger and r["which"] == w]
            v = sorted(r["env_steps_per_s"] for r in mine); c = sorted(r["cpu_s_per_wall_s"] for r in mine)
            summary[f"stagger={stagger} {w}"] = dict(runs=[round(x) for x in v], median=round(v[len(v) // 2]), spread_pct=round(100.0 * (v[-1] - v[0]) / v[len(v) // 2], 2),
                                                     cpu_s_per_wall_s_median=round(c[len(c) // 2], 3))
    out = dict(steps=args.steps, envs=args.envs, agents=args.agents, levels=args.levels, runs=runs, summary=summary)
    print("SUMMARY " + json.dumps(summary, indent=1), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
