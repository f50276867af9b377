#!/usr/bin/env python
"""What the batched device-side snapshots (mcr_save_states / mcr_load_states / mcr_copy_states, csrc/k_envcopy.h) cost at B = 4096, N = 2.

Four operations — save all envs, load all envs, clone 64 sources x 63 destinations (n = 4032), clone n = 64 — each timed with device events
around `--inner` back-to-back calls (the launch latency of the first is in the sample, amortised), warmed, the median of `--samples` samples.
Beside each figure, measured in the same run:
  (a) memcpy     a device-to-device copy of the same number of bytes (torch's copy_ of a contiguous uint8 tensor: hipMemcpyAsync) — the
                 yardstick for the kernel; `fraction_of_memcpy` = memcpy time / kernel time
  (b) host path  the per-env calls the feature replaces, get_state_blob / set_state_blob over 64 envs, wall time per env
Bytes: n x mcr_state_blob_bytes is the payload; a copy reads and writes it once, so bytes/s figures are 2 x payload / time for the kernel
and the memcpy alike.  Writes one JSON file (--out, default profiles/state_copy_cost.json) and prints it.

    python tools/state_copy_cost.py
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/state_copy_cost.py --samples 3      # the kernels' own durations"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--agents", type=int, default=2)
    ap.add_argument("--presteps", type=int, default=32)
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "state_copy_cost.json"))
    args = ap.parse_args()
    import torch
    from multi_car_racing_amd import _lib
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path to time"
    B, N = args.envs, args.agents
    assert B >= 64 * 64, "the 64 x 63 clone needs 4096 envs"
    env = VecMultiCarRacing(B, N, seed=0, obs=False, auto_reset=False, use_random_direction=True, streams=2, async_refill=False)
    env.reset()
    for t in range(args.presteps):
        env.step(env.synth_actions(t, seed=1234))
    dev, L, vp = env.device, env.L, ctypes.c_void_p
    st = torch.cuda.current_stream(dev)
    stream = vp(st.cuda_stream)
    nbytes, pitch = int(L.mcr_state_blob_bytes(env.h)), env.state_blob_pitch
    blobs = torch.empty((B, pitch), dtype=torch.uint8, device=dev)
    scratch = torch.empty_like(blobs)
    fan_src = torch.arange(64, dtype=torch.int32, device=dev).repeat_interleave(63)                 # sources 0..63, 63 destinations each
    fan_dst = torch.arange(64, 64 + 64 * 63, dtype=torch.int32, device=dev)
    few_src = torch.arange(64, dtype=torch.int32, device=dev); few_dst = few_src + 64

    def save_all():
        _lib.check(L.mcr_save_states(env.h, None, B, vp(blobs.data_ptr()), stream), "mcr_save_states")

    def load_all():
        _lib.check(L.mcr_load_states(env.h, None, B, vp(blobs.data_ptr()), None, stream), "mcr_load_states")

    def clone(src, dst):
        return lambda: _lib.check(L.mcr_copy_states(env.h, vp(src.data_ptr()), vp(dst.data_ptr()), int(src.numel()), stream), "mcr_copy_states")

    def memcpy(n):
        return lambda: scratch[:n].copy_(blobs[:n])

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        us = []
        for _ in range(args.samples):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            for _ in range(args.inner):
                fn()
            b.record(st)
            b.synchronize()
            us.append(a.elapsed_time(b) * 1000.0 / args.inner)
        return statistics.median(us), min(us), max(us)

    save_all(); torch.cuda.synchronize()                                  # `blobs` holds valid rows before anything loads them
    ops = [("save_all", save_all, B), ("load_all", load_all, B), ("clone_64x63", clone(fan_src, fan_dst), 64 * 63), ("clone_64", clone(few_src, few_dst), 64)]
    result = dict(envs=B, agents=N, blob_bytes=nbytes, pitch=pitch, samples=args.samples, inner=args.inner, device=torch.cuda.get_device_name(dev), ops={})
    for name, fn, n in ops:
        k_us, k_lo, k_hi = timed(fn)
        m_us, m_lo, m_hi = timed(memcpy(n))
        payload = n * nbytes
        result["ops"][name] = dict(n=n, payload_bytes=payload, kernel_us=round(k_us, 2), kernel_us_range=[round(k_lo, 2), round(k_hi, 2)],
                                   kernel_bytes_per_s=round(2 * payload / (k_us * 1e-6)), memcpy_us=round(m_us, 2), memcpy_us_range=[round(m_lo, 2), round(m_hi, 2)],
                                   memcpy_bytes_per_s=round(2 * n * pitch / (m_us * 1e-6)), fraction_of_memcpy=round(m_us / k_us, 3))
    # (b) the per-env host path over 64 envs
    torch.cuda.synchronize()
    t0 = time.perf_counter(); host = [env.get_state_blob(e) for e in range(64)]; t_get = (time.perf_counter() - t0) / 64
    t0 = time.perf_counter()
    for e in range(64):
        env.set_state_blob(e, host[e])
    t_set = (time.perf_counter() - t0) / 64
    result["host_path"] = dict(envs=64, get_state_blob_us_per_env=round(t_get * 1e6, 1), set_state_blob_us_per_env=round(t_set * 1e6, 1))
    for name, per_env in (("save_all", t_get), ("load_all", t_set)):
        o = result["ops"][name]
        o["host_path_us_scaled"] = round(per_env * 1e6 * o["n"], 1); o["speedup_over_host_path"] = round(per_env * 1e6 * o["n"] / o["kernel_us"], 1)
    status = env.status_words()[:5].tolist()
    env.close()
    result["status"] = status
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
