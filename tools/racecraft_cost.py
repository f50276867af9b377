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
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = {"parent": {}, "off": {}, "drv": {"scripted_agents": (1,)}, "on": {"scripted_agents": (1,), "racecraft": True}}


def _rollout(torch, env, B, N, K, W, timed=True):
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
    for j in range(L):
        env.step(next_actions())
        msk = ((ids * L) // B == j).to(torch.uint8)
        if bool(msk.any()):
            env.reset_envs(msk)
    for k in range(W):
        env.step(next_actions())
    env.wait_refills()
    torch.cuda.synchronize()
    c0 = env.debug_counters()
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
    c1 = env.debug_counters()
    return elapsed, int(c1[2]) - int(c0[2]), int(c1[3])


def worker(args):
    tree = os.path.abspath(args.parent_tree) if args.worker == "parent" else ROOT
    sys.path.insert(0, tree)
    import torch
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    import multi_car_racing_amd
    assert os.path.abspath(os.path.dirname(os.path.dirname(multi_car_racing_amd.__file__))) == tree, "the package did not come from the tree asked for"
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path to time"
    B, N, K, W = args.envs, args.agents, args.steps, args.warmup
    common = dict(seed=0, obs=bool(args.obs), auto_reset=True, use_random_direction=True, streams=2, async_refill=True)
    if args.worker == "trace":                          # for the kernel trace alone: both instantiations and k_stateobs in one process
        for kw in (dict(KW["on"], state_obs=True), KW["drv"]):
            env = VecMultiCarRacing(B, N, **common, **kw)
            env.reset()
            _rollout(torch, env, B, N, K, W)
            env.close()
        print("RESULT " + json.dumps(dict(which="trace", steps=K)), flush=True)
        return
    env = VecMultiCarRacing(B, N, **common, **KW[args.worker])
    env.reset()
    elapsed, contact_envs, frozen = _rollout(torch, env, B, N, K, W)
    status = env.status_words()[:5].tolist()
    nz = None if getattr(env, "actions", None) is None else bool((env.actions[:, 1] != 0).any().item())
    env.close()
    print("RESULT " + json.dumps(dict(which=args.worker, obs=args.obs, envs=B, agents=N, steps=K, elapsed_s=elapsed, env_steps_per_s=B * K / elapsed,
                                      contact_env_steps=contact_envs, contact_share=contact_envs / float(B * K),
                                      frozen_env_steps=frozen, status=status, driver_rows_written=nz)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worker", choices=["parent", "off", "drv", "on", "trace"], default=None, help="run ONE measurement in this process")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit (omit: the `parent` runs are left out)")
    ap.add_argument("--obs", type=int, default=0)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--agents", type=int, default=2)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--configs", default="0,1", help="obs settings to measure: 0 = BASELINE configs[4], 1 = configs[1]")
    ap.add_argument("--child-timeout", type=int, default=150)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    which = (["parent"] if args.parent_tree else []) + ["off", "drv", "on"]
    runs = []
    for obs in [int(v) for v in args.configs.split(",")]:
        for rep in range(args.repeats):
            for w in which:                              # alternating: a drift of the machine hits all of them alike
                cmd = [sys.executable, os.path.abspath(__file__), "--worker", w, "--obs", str(obs), "--envs", str(args.envs), "--agents", str(args.agents),
                       "--steps", str(args.steps), "--warmup", str(args.warmup)] + (["--parent-tree", args.parent_tree] if args.parent_tree else [])
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
            mine = [r for r in runs if r["obs"] == obs and r["which"] == w]
            v = sorted(r["env_steps_per_s"] for r in mine)
            share = sorted(r["contact_share"] for r in mine)
            summary[f"obs={obs} {w}"] = dict(runs=[round(x) for x in v], median=round(v[len(v) // 2]), spread_pct=round(100.0 * (v[-1] - v[0]) / v[len(v) // 2], 2),
                                             contact_share_median=round(share[len(share) // 2], 5))
    out = dict(steps=args.steps, envs=args.envs, agents=args.agents, runs=runs, summary=summary)
    print("SUMMARY " + json.dumps(summary, indent=1), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
