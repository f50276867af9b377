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
import os
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
    kw = {} if args.worker == "parent" else {"grid_obs": args.worker == "on"}
    if args.others:
        kw.update(state_obs=True, range_obs=True)
    env = VecMultiCarRacing(B, N, seed=0, obs=bool(args.obs), auto_reset=True, use_random_direction=True, streams=2, async_refill=True, **kw)
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
    L = args.stagger                                    # bench.py's stagger: every env reset once, at a step of its own, before anything is timed
    ids = torch.randperm(B, device=dev, generator=g)
    for j in range(L):
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
    env.wait_refills()
    frozen = int(env.debug_counters()[3]); status = env.status_words()[:5].tolist()
    grid = getattr(env, "grid", None)
    filled = None if grid is None else round(float((grid != 0).float().mean().item()), 4)      # share of cells with anything under them
    env.close()
    print("RESULT " + json.dumps(dict(which=args.worker, obs=args.obs, envs=B, agents=N, steps=K, elapsed_s=elapsed, env_steps_per_s=B * K / elapsed,
                                      frozen_env_steps=frozen, status=status, grid_filled=filled)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worker", choices=["parent", "off", "on"], default=None, help="run ONE measurement in this process")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit (omit: the `parent` runs are left out)")
    ap.add_argument("--obs", type=int, default=0)
    ap.add_argument("--others", type=int, default=0, help="1: state_obs=True and range_obs=True as well (kernel traces: their kernels beside k_gridobs)")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--agents", type=int, default=2)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--stagger", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--configs", default="0,1", help="obs settings to measure: 0 = BASELINE configs[4], 1 = configs[1]")
    ap.add_argument("--child-timeout", type=int, default=150)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    which = (["parent"] if args.parent_tree else []) + ["off", "on"]
    runs = []
    for rep in range(args.repeats):
        for obs in [int(v) for v in args.configs.split(",")]:
            for w in which:                              # alternating: a drift of the machine hits all of them alike
                cmd = [sys.executable, os.path.abspath(__file__), "--worker", w, "--obs", str(obs), "--envs", str(args.envs), "--agents", str(args.agents),
                       "--steps", str(args.steps), "--warmup", str(args.warmup), "--stagger", str(args.stagger), "--others", str(args.others)]
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
    for obs in sorted({r["obs"] for r in runs}):         # `off` against the parent's own run-to-run spread
        pa, of = summary.get(f"obs={obs} parent"), summary.get(f"obs={obs} off")
        if pa and of:
            of["vs_parent_median_pct"] = round(100.0 * (of["median"] - pa["median"]) / pa["median"], 2)
            of["within_parent_spread"] = bool(of["median"] >= pa["runs"][0])      # no slower than the parent's slowest run
        on = summary.get(f"obs={obs} on")
        if on and of:
            on["vs_off_median_pct"] = round(100.0 * (on["median"] - of["median"]) / of["median"], 2)
    grid_only, pixels = summary.get("obs=0 on"), summary.get("obs=1 parent")
    if grid_only and pixels:                             # the grid instead of the frame, against the frame
        grid_only["vs_parent_rgb_median_pct"] = round(100.0 * (grid_only["median"] - pixels["median"]) / pixels["median"], 2)
        grid_only["faster_than_parent_rgb"] = bool(grid_only["median"] > pixels["median"])
    out = dict(steps=args.steps, envs=args.envs, agents=args.agents, runs=runs, summary=summary)
    print("SUMMARY " + json.dumps(summary, indent=1), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
