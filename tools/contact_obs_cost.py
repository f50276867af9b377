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
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"obs0": (0, "random"), "obs1": (1, "random"), "drive": (1, "drive")}


def worker(args):
    tree = os.path.abspath(args.parent_tree) if args.worker == "parent" else ROOT
    sys.path.insert(0, tree)
    import torch
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    import multi_car_racing_amd
    assert os.path.abspath(os.path.dirname(os.path.dirname(multi_car_racing_amd.__file__))) == tree, "the package did not come from the tree asked for"
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path to time"
    B, N, K, W = args.envs, args.agents, args.steps, args.warmup
    obs, actions = CONFIGS[args.config]
    kw = {} if args.worker == "parent" else {"contact_obs": args.worker == "on"}
    if args.siblings:                                   # (kernel traces) the other derived-output kernels in the same trace: k_stateobs, k_levelstats
        kw.update(state_obs=True, levels=256, level_stats=True)
    env = VecMultiCarRacing(B, N, seed=0, obs=bool(obs), auto_reset=True, use_random_direction=True, streams=2, async_refill=True, **kw)
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
            if actions == "drive":                      # bench.py --actions drive
                a = act[blk & 1]
                a[..., 0].mul_(0.1); a[..., 1].fill_(1.0); a[..., 2].zero_()
        return act[blk & 1][j]
    L = 1000                                            # bench.py's stagger: every env reset once, at a step of its own, before anything is timed
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
    # (outside the timed region) 32 more steps: envs with a contact per step — the long path's share — by the observation and, as a
    # cross-check on this topology, by the manifold stores' own counts (mcr_debug_read_contact_counts)
    touching = by_store = None
    if getattr(env, "contact_mask", None) is not None:
        import ctypes
        import numpy as np
        touching, by_store = [], []
        counts = np.zeros(B, np.int32)
        for k in range(32):
            env.step(next_actions())
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worker", choices=["parent", "off", "on"], default=None, help="run ONE measurement in this process")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit (omit: the `parent` runs are left out)")
    ap.add_argument("--config", choices=sorted(CONFIGS), default="obs0", help="the worker's configuration")
    ap.add_argument("--siblings", type=int, default=0, help="worker: 1 = also state_obs=True and levels=256, level_stats=True (k_stateobs and k_levelstats in the same kernel trace)")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--agents", type=int, default=2)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--configs", default="obs0,obs1,drive", help="configurations to measure")
    ap.add_argument("--child-timeout", type=int, default=150)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    which = (["parent"] if args.parent_tree else []) + ["off", "on"]
    runs = []
    for cfg in args.configs.split(","):
        for rep in range(args.repeats):
            for w in which:                              # alternating: a drift of the machine hits all three alike
                cmd = [sys.executable, os.path.abspath(__file__), "--worker", w, "--config", cfg, "--envs", str(args.envs), "--agents", str(args.agents),
                       "--steps", str(args.steps), "--warmup", str(args.warmup)] + (["--parent-tree", args.parent_tree] if args.parent_tree else [])
                pr = subprocess.run(["timeout", "-k", "10", str(args.child_timeout)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                line = [l for l in pr.stdout.splitlines() if l.startswith("RESULT ")]
                if pr.returncode != 0 or not line:
                    print(pr.stdout[-4000:])
                    print(f"child {w} config={cfg} ended with {pr.returncode}: nothing more is started", flush=True)
                    return 1
                r = json.loads(line[-1][7:]); r["repeat"] = rep
                runs.append(r); print(json.dumps(r), flush=True)
    summary = {}
    for cfg in args.configs.split(","):
        for w in which:
            v = sorted(r["env_steps_per_s"] for r in runs if r["config"] == cfg and r["which"] == w)
            summary[f"{cfg} {w}"] = dict(runs=[round(x) for x in v], median=round(v[len(v) // 2]), spread_pct=round(100.0 * (v[-1] - v[0]) / v[len(v) // 2], 2))
        off = summary[f"{cfg} off"]["median"]
        summary[f"{cfg} on vs off pct"] = round(100.0 * (summary[f"{cfg} on"]["median"] - off) / off, 2)
        if args.parent_tree:
            par = summary[f"{cfg} parent"]["median"]
            summary[f"{cfg} off vs parent pct"] = round(100.0 * (off - par) / par, 2)
    out = dict(steps=args.steps, envs=args.envs, agents=args.agents, runs=runs, summary=summary)
    print("SUMMARY " + json.dumps(summary, indent=1), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
