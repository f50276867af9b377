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
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKERS = ["parent", "off", "stats", "weighted", "both"]


def worker(args):
    tree = os.path.abspath(args.parent_tree) if args.worker == "parent" else ROOT
    sys.path.insert(0, tree)
    import torch
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    import multi_car_racing_amd
    assert os.path.abspath(os.path.dirname(os.path.dirname(multi_car_racing_amd.__file__))) == tree, "the package did not come from the tree asked for"
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path to time"
    B, N, K, W = args.envs, args.agents, args.steps, args.warmup
    kw = {}
    if args.worker in ("stats", "both"):
        kw["level_stats"] = True
    if args.worker in ("weighted", "both"):
        kw["level_order"] = "weighted"
    if args.state_obs:
        kw["state_obs"] = True
    env = VecMultiCarRacing(B, N, seed=0, obs=bool(args.obs), auto_reset=True, use_random_direction=True, streams=2, levels=args.levels, **kw)
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
    if "level_order" in kw:                             # device weights, no synchronisation: what a learner's update would enqueue
        env.set_level_weights(1.0 + torch.arange(args.levels, dtype=torch.float64, device=dev) % 7, check=False)
    torch.cuda.synchronize()
    LOOKAHEAD = 16; FENCE = LOOKAHEAD // 4
    evs = [torch.cuda.Event(blocking=True) for _ in range(4)]
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
    episodes, _ = env.rollout_stats()
    counted = None if getattr(env, "level_stats", None) is None else float(env.level_stats[:, 0].sum().item())
    levels_seen = int(torch.unique(env.level).numel())
    env.close()
    print("RESULT " + json.dumps(dict(which=args.worker, obs=args.obs, stagger=args.stagger, envs=B, agents=N, steps=K, elapsed_s=elapsed,
                                      env_steps_per_s=B * K / elapsed, episodes_finished=episodes, episodes_in_level_stats=counted,
                                      levels_in_play=levels_seen)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worker", choices=WORKERS, default=None, help="run ONE measurement in this process")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit (omit: the `parent` runs are left out)")
    ap.add_argument("--stagger", type=int, default=1, help="1: bench.py's staggered pre-roll; 0: all envs in phase (they all end in step 999, 1999, ...)")
    ap.add_argument("--obs", type=int, default=1, help="worker: 1 RGB observations, 0 physics only")
    ap.add_argument("--state-obs", type=int, default=0, help="worker: 1 adds state_obs=True (k_stateobs in the same trace)")
    ap.add_argument("--levels", type=int, default=256)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--agents", type=int, default=2)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--obs-settings", default="0,1", help="obs settings to measure: 0 physics only, 1 RGB")
    ap.add_argument("--child-timeout", type=int, default=150)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    which = (["parent"] if args.parent_tree else []) + ["off", "stats", "weighted"]
    runs = []
    for obs in [int(v) for v in args.obs_settings.split(",")]:
        for rep in range(args.repeats):
            for w in which:                              # alternating: a drift of the machine hits all alike
                cmd = [sys.executable, os.path.abspath(__file__), "--worker", w, "--obs", str(obs), "--stagger", str(args.stagger), "--levels", str(args.levels),
                       "--envs", str(args.envs), "--agents", str(args.agents), "--steps", str(args.steps), "--warmup", str(args.warmup)]
                cmd += ["--parent-tree", args.parent_tree] if args.parent_tree else []
                pr = subprocess.run(["timeout", "-k", "10", str(args.child_timeout)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                line = [l for l in pr.stdout.splitlines() if l.startswith("RESULT ")]
                if pr.returncode != 0 or not line:
                    print(pr.stdout[-4000:])
                    print(f"child {w} obs={obs} ended with {pr.returncode}: nothing more is started", flush=True)
                    return 1
                r = json.loads(line[-1][7:]); r["repeat"] = rep
                runs.append(r); print(json.dumps(r), flush=True)
    summary = {}
    for obs in sorted({r["obs"] for r in runs}):
        for w in which:
            v = sorted(r["env_steps_per_s"] for r in runs if r["obs"] == obs and r["which"] == w)
            summary[f"obs={obs} {w}"] = dict(runs=[round(x) for x in v], median=round(v[len(v) // 2]), spread_pct=round(100.0 * (v[-1] - v[0]) / v[len(v) // 2], 2))
        base = summary[f"obs={obs} off"]["median"]
        for w in which:
            summary[f"obs={obs} {w}"]["vs_off_pct"] = round(100.0 * (summary[f"obs={obs} {w}"]["median"] - base) / base, 2)
    out = dict(steps=args.steps, envs=args.envs, agents=args.agents, levels=args.levels, stagger=args.stagger, runs=runs, summary=summary)
    print("SUMMARY " + json.dumps(summary, indent=1), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
