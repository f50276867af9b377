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
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKERS = {"parent1": ("parent", 1), "parent4": ("parent", 4), "parent8": ("parent", 8), "skip1": ("this", 1), "skip4": ("this", 4), "skip8": ("this", 8)}
CONFIGS = {"rgb": dict(obs_format="rgb", frame_stack=1), "gray4": dict(obs_format="gray", frame_stack=4)}


def worker(args):
    side, k = WORKERS[args.worker]
    tree = os.path.abspath(args.parent_tree) if side == "parent" else ROOT
    sys.path.insert(0, tree)
    import torch
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    import multi_car_racing_amd
    assert os.path.abspath(os.path.dirname(os.path.dirname(multi_car_racing_amd.__file__))) == tree, "the package did not come from the tree asked for"
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path to time"
    B, N = args.envs, args.agents
    kw = dict(CONFIGS[args.config])
    if side == "this":
        kw["frame_skip"] = k
    env = VecMultiCarRacing(B, N, seed=0, obs=True, auto_reset=True, use_random_direction=True, streams=2, async_refill=True, **kw)
    env.reset()
    calls = k if side == "parent" else 1                # step() calls per policy step
    dev = env.device
    g = torch.Generator(device=dev); g.manual_seed(1234)
    ACT_BLOCK = 16
    act = [torch.empty((ACT_BLOCK, B, N, 3), dtype=torch.float32, device=dev) for _ in range(2)]
    tstep = [0]

    def policy_step():
        t = tstep[0]; tstep[0] += 1
        blk, j = divmod(t, ACT_BLOCK)
        if j == 0:
            env.synth_actions(t, seed=1234, out=act[blk & 1], steps=ACT_BLOCK)
        a = act[blk & 1][j]
        for _ in range(calls):
            env.step(a)
    P = (1000 + k - 1) // k                             # bench.py's stagger in policy steps: every env reset once, at a step of its own, before anything is timed
    ids = torch.randperm(B, device=dev, generator=g)
    for j in range(P):
        policy_step()
        msk = ((ids * P) // B == j).to(torch.uint8)
        if bool(msk.any()):
            env.reset_envs(msk)
    for _ in range(max(1, args.warmup // k)):
        policy_step()
    env.wait_refills()
    torch.cuda.synchronize()
    K = max(1, args.steps // k)                         # timed policy steps
    LOOKAHEAD = 16; FENCE = LOOKAHEAD // 4
    evs = [torch.cuda.Event(blocking=True) for _ in range(4)]
    t0 = time.perf_counter()
    for i in range(K):
        policy_step()
        if i % FENCE == FENCE - 1:
            j = (i // FENCE) % 4
            if i >= LOOKAHEAD:
                while not evs[j].query():
                    time.sleep(1e-4)
            evs[j].record()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    env.wait_refills()
    frozen = int(env.debug_counters()[3]); status = env.status_words()[:5].tolist()
    env.close()
    print("RESULT " + json.dumps(dict(which=args.worker, config=args.config, envs=B, agents=N, env_steps_per_policy_step=k, policy_steps=K, elapsed_s=elapsed,
                                      policy_steps_per_s=K / elapsed, env_steps_per_s=B * K * k / elapsed, frozen_env_steps=frozen, status=status)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worker", choices=sorted(WORKERS), default=None, help="run ONE measurement in this process")
    ap.add_argument("--config", choices=sorted(CONFIGS), default="rgb")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit (omit: the parent runs are left out)")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--agents", type=int, default=2)
    ap.add_argument("--steps", type=int, default=2000, help="timed ENV steps per run (policy steps: steps // k)")
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--configs", default="rgb,gray4")
    ap.add_argument("--child-timeout", type=int, default=150)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    which = [w for w in ("parent1", "skip1", "parent4", "skip4", "parent8", "skip8") if args.parent_tree or not w.startswith("parent")]
    runs = []
    for cfg in args.configs.split(","):
        for rep in range(args.repeats):
            for w in which:                              # alternating: a drift of the machine hits all of them alike
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
            sel = [r for r in runs if r["config"] == cfg and r["which"] == w]
            v = sorted(r["env_steps_per_s"] for r in sel); p = sorted(r["policy_steps_per_s"] for r in sel)
            summary[f"{cfg} {w}"] = dict(env_steps_per_s_runs=[round(x) for x in v], env_steps_per_s_median=round(v[len(v) // 2]),
                                         policy_steps_per_s_median=round(p[len(p) // 2], 1), spread_pct=round(100.0 * (v[-1] - v[0]) / v[len(v) // 2], 2))
    out = dict(env_steps_timed=args.steps, envs=args.envs, agents=args.agents, runs=runs, summary=summary)
    print("SUMMARY " + json.dumps(summary, indent=1), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
