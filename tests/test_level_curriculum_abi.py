"""CPU: the level curricula's C ABI (include/mcr.h: mcr_level_cdf, mcr_pool_level_weighted, mcr_set_level_sampler, mcr_level_weights,
mcr_set_level_stats, mcr_level_stats_dim) and its Python wrappers against the restatement in tests/level_stats_ref.py — no GPU needed."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import level_stats_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MCR_ERR_ARG = -1
NEW = {
    "mcr_level_cdf": r"\bint\s+mcr_level_cdf\s*\(\s*const\s+double\s*\*\s*w\s*,\s*int\s+K\s*,\s*double\s*\*\s*cdf_out\s*\)",
    "mcr_pool_level_weighted": r"\bint32_t\s+mcr_pool_level_weighted\s*\(\s*uint64_t\s+seed\s*,\s*uint32_t\s+global_env\s*,\s*uint32_t\s+episode\s*,"
                               r"\s*const\s+double\s*\*\s*cdf\s*,\s*int32_t\s+K\s*\)",
    "mcr_set_level_sampler": r"\bint\s+mcr_set_level_sampler\s*\(\s*mcr_env\s*\*\s*h\s*,\s*double\s*\*\s*d_cdf\s*,\s*int32_t\s*\*\s*d_staged_level\s*\)",
    "mcr_level_weights": r"\bint\s+mcr_level_weights\s*\(\s*mcr_env\s*\*\s*h\s*,\s*const\s+double\s*\*\s*d_weights\s*,\s*int32_t\s*\*\s*d_fell_back\s*,\s*void\s*\*\s*stream\s*\)",
    "mcr_set_level_stats": r"\bint\s+mcr_set_level_stats\s*\(\s*mcr_env\s*\*\s*h\s*,\s*int32_t\s*\*\s*d_finished_level\s*,\s*double\s*\*\s*d_stats\s*\)",
    "mcr_level_stats_dim": r"\bint\s+mcr_level_stats_dim\s*\(\s*int\s+num_agents\s*\)",
    "mcr_debug_level_stats": r"\bint\s+mcr_debug_level_stats\s*\(\s*const\s+uint8_t\s*\*\s*d_done\s*,\s*const\s+uint8_t\s*\*\s*d_trunc\s*,"
                             r"\s*const\s+double\s*\*\s*d_ep_return\s*,\s*const\s+int32_t\s*\*\s*d_ep_len\s*,\s*const\s+int32_t\s*\*\s*d_level\s*,"
                             r"\s*int\s+num_envs\s*,\s*int\s+num_agents\s*,\s*int\s+K\s*,\s*int32_t\s*\*\s*d_finished\s*,\s*double\s*\*\s*d_stats\s*,"
                             r"\s*void\s*\*\s*stream\s*\)",
}


def _c_cdf(L, lib, w):
    w = np.ascontiguousarray(w, np.float64)
    out = np.full(len(w), -7.0)
    rc = L.mcr_level_cdf(lib.ptr(w), len(w), lib.ptr(out))
    assert rc in (0, 1)
    return out, bool(rc)


def _c_level(L, lib, seed, g, k, cdf):
    cdf = np.ascontiguousarray(cdf, np.float64)
    return int(L.mcr_pool_level_weighted(ctypes.c_uint64(seed), ctypes.c_uint32(g), ctypes.c_uint32(k), lib.ptr(cdf), len(cdf)))


def _same_bits(a, b):
    return a.dtype == b.dtype == np.float64 and a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_symbols_declared_and_exported(lib):
    L = lib.load()
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcr.h")).read(), flags=re.S)
    exported = {ln.split()[-1] for ln in subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True,
                                                         text=True).stdout.splitlines() if " T " in ln}
    for name, decl in NEW.items():
        assert re.search(decl, code), f"{name} is not declared in include/mcr.h as the issue states it"
        assert name in exported and hasattr(L, name), f"{name} is not exported by libmcr_hip.so"
        assert name in lib.SYMBOLS
    # the whole header against the whole export table
    declared = set(re.findall(r"\b(mcr_[a-z0-9_]+)\s*\(", code))
    assert {s for s in exported if s.startswith("mcr_")} == declared


def test_level_cdf_matches_the_python_loop_bit_for_bit(lib):
    L = lib.load()
    rng = np.random.RandomState(5)
    for _ in range(300):
        K = int(rng.randint(1, 5001))
        w = 10.0 ** rng.uniform(-300, 300, K) if rng.rand() < 0.5 else 10.0 ** rng.uniform(-300, 300) * rng.uniform(0, 1, K)
        got, fb = _c_cdf(L, lib, w)
        want, wfb = ref.cdf(w)
        assert fb == wfb and _same_bits(got, want), f"K = {K}"
        if not fb:
            assert got[-1] == 1.0 and (np.diff(got) >= 0).all() and (got >= 0).all()
    # a sum that overflows: not finite, so uniform
    got, fb = _c_cdf(L, lib, [1e308, 1e308, 1.0])
    assert fb and _same_bits(got, ref.cdf([1e308, 1e308, 1.0])[0]) and _same_bits(got, np.array([1 / 3, 2 / 3, 1.0]))


def test_level_cdf_sanitises_and_falls_back(lib):
    L = lib.load()
    nan, inf = float("nan"), float("inf")
    # not finite or negative: counts as 0
    for w, clean in (([1.0, nan, 2.0], [1.0, 0.0, 2.0]), ([inf, 1.0, 3.0], [0.0, 1.0, 3.0]), ([-inf, 2.0], [0.0, 2.0]),
                     ([-1.0, 4.0, -0.0, 1.0], [0.0, 4.0, 0.0, 1.0]), ([nan, inf, -2.0, 5.0], [0.0, 0.0, 0.0, 5.0])):
        got, fb = _c_cdf(L, lib, w)
        want, wfb = ref.cdf(w)
        assert not fb and not wfb and _same_bits(got, want) and _same_bits(got, ref.cdf(clean)[0]), w
    # nothing left: the uniform CDF, flag set
    for w in ([0.0, 0.0, 0.0], [nan, nan], [-1.0, -2.0, -3.0, -4.0], [inf, -inf, nan, 0.0, -0.0], [0.0]):
        got, fb = _c_cdf(L, lib, w)
        want, wfb = ref.cdf(w)
        K = len(w)
        assert fb and wfb and _same_bits(got, want) and _same_bits(got, np.array([float(j + 1) / float(K) for j in range(K)])), w
    # K = 1
    for w in ([3.5], [1e-300], [1e300]):
        got, fb = _c_cdf(L, lib, w)
        assert not fb and got.tolist() == [1.0]
    # all-ones == the initial (uniform) CDF, bit for bit
    for K in (1, 2, 3, 7, 256, 300, 4999):
        got, fb = _c_cdf(L, lib, np.ones(K))
        zero, zfb = _c_cdf(L, lib, np.zeros(K))
        assert not fb and zfb and _same_bits(got, zero) and _same_bits(got, ref.cdf(np.ones(K))[0])
    # bad arguments
    one = np.ones(2)
    assert L.mcr_level_cdf(None, 2, lib.ptr(one)) == MCR_ERR_ARG and L.mcr_level_cdf(lib.ptr(one), 2, None) == MCR_ERR_ARG
    assert L.mcr_level_cdf(lib.ptr(one), 0, lib.ptr(one)) == MCR_ERR_ARG and L.mcr_level_cdf(lib.ptr(one), -1, lib.ptr(one)) == MCR_ERR_ARG


def test_weighted_level_matches_the_restatement(lib):
    L = lib.load()
    rng = np.random.RandomState(6)
    for _ in range(300):
        seed = int(rng.randint(0, 2 ** 32)) << 32 | int(rng.randint(0, 2 ** 32))
        g = int(rng.randint(0, 2 ** 32)); k = int(rng.randint(0, 2 ** 32)); K = int(rng.randint(1, 400))
        w = rng.uniform(0, 1, K) * (rng.rand(K) < 0.6)          # ~40 % zero weights
        if not w.any():
            w[int(rng.randint(K))] = 1.0
        c, fb = ref.cdf(w)
        assert not fb
        v = _c_level(L, lib, seed, g, k, c)
        assert 0 <= v < K and v == ref.weighted_level(seed, g, k, c), (seed, g, k, K)
        assert w[v] > 0, "a zero-weight level was drawn"
        # one positive weight: always that level
        j = int(rng.randint(K)); single = np.zeros(K); single[j] = float(rng.uniform(1e-9, 1e9))
        assert _c_level(L, lib, seed, g, k, ref.cdf(single)[0]) == j
    # the uniform is the top 53 bits of mode 0's hash: under the uniform CDF of K = 2**m levels the draw is the hash's top m bits
    for g in range(8):
        x = ref._mix64(ref._mix64((9 + 0x9e3779b97f4a7c15 * ((3 << 32) | g)) & ref.M64))
        assert ref.uniform(9, g, 3) == (x >> 11) / 2.0 ** 53 and 0.0 <= ref.uniform(9, g, 3) < 1.0
        assert _c_level(L, lib, 9, g, 3, ref.cdf(np.ones(16))[0]) == x >> 60
    # bad arguments
    c = np.ones(1)
    assert L.mcr_pool_level_weighted(ctypes.c_uint64(0), 0, 0, None, 3) == MCR_ERR_ARG
    assert L.mcr_pool_level_weighted(ctypes.c_uint64(0), 0, 0, lib.ptr(c), 0) == MCR_ERR_ARG


@pytest.mark.parametrize("seed", [0, 23])
@pytest.mark.parametrize("weights", [[1, 2, 3, 4], [0, 1, 0, 3], [1e-3, 1, 1, 1]])
def test_frequencies_follow_the_weights(lib, seed, weights):
    """n = 20 000 draws (g in 0..1999, k in 0..9): every level's share within 4 sigma, sigma = sqrt(p (1 - p) / n), of its weight share;
    a zero-weight level gets exactly 0.  (Worst case over these inputs, from the hash's restatement: 1.81 sigma.)"""
    L = lib.load()
    c, fb = _c_cdf(L, lib, np.array(weights, np.float64))
    assert not fb
    K, n = len(weights), 2000 * 10
    counts = np.zeros(K, np.int64)
    for g in range(2000):
        for k in range(10):
            counts[_c_level(L, lib, seed, g, k, c)] += 1
    assert counts.sum() == n
    total = float(sum(weights))
    worst = 0.0
    for j in range(K):
        p = weights[j] / total
        if p == 0:
            assert counts[j] == 0, f"level {j} has weight 0 and was drawn {counts[j]} times"
            continue
        sigma = math.sqrt(p * (1 - p) / n)
        dev = abs(counts[j] / n - p) / sigma
        worst = max(worst, dev)
        print(f"seed {seed} weights {weights} level {j}: share {counts[j] / n:.5f} want {p:.5f} = {dev:.2f} sigma")
        assert dev <= 4.0, f"level {j}: share {counts[j] / n:.5f}, weight share {p:.5f}: {dev:.2f} sigma"


def test_python_wrappers_and_validation(lib):
    from multi_car_racing_amd import levels
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    c, fb = levels.level_cdf([1, 0, 3])
    assert not fb and _same_bits(c, ref.cdf([1, 0, 3])[0])
    c0, fb0 = levels.level_cdf([0, 0])
    assert fb0 and c0.tolist() == [0.5, 1.0]
    for g in range(5):
        for k in range(4):
            assert levels.weighted_level(13, g, k, c) == ref.weighted_level(13, g, k, c) != 1
    with pytest.raises(ValueError):
        levels.pool_level(0, 0, 0, 3, order="weighted")
    assert "weighted" not in lib.LEVEL_ORDER and sorted(lib.LEVEL_ORDER.values()) == [0, 1]        # no third ABI mode
    with pytest.raises(ValueError):
        levels.level_cdf([])
    # set_level_weights(check=True)'s host validation
    assert levels.check_weights([1, 0, 2.5], 3).tolist() == [1.0, 0.0, 2.5]
    for bad in ([1, 2], [1, 2, 3, 4], [[1, 2, 3]], [1, -1, 2], [1, float("nan"), 2], [1, float("inf"), 2], [0, 0, 0], [1e308, 1e308, 1e308]):
        with pytest.raises(ValueError):
            levels.check_weights(bad, 3)
    # keyword validation comes before anything is created (no device needed)
    with pytest.raises(ValueError):
        VecMultiCarRacing(2, 2, level_stats=True)
    with pytest.raises(ValueError):
        VecMultiCarRacing(2, 2, levels=3, level_order="shuffle", level_stats=True)


def test_abi_errors_that_need_no_device(lib):
    L = lib.load()
    buf = np.zeros(8)
    p = lib.ptr(buf)
    assert L.mcr_set_level_sampler(None, p, p) == MCR_ERR_ARG
    assert L.mcr_level_weights(None, p, None, None) == MCR_ERR_ARG
    assert L.mcr_set_level_stats(None, p, p) == MCR_ERR_ARG
    assert L.mcr_level_stats_dim(0) == MCR_ERR_ARG and L.mcr_level_stats_dim(9) == MCR_ERR_ARG
    assert [L.mcr_level_stats_dim(n) for n in range(1, 9)] == [3 + 2 * n for n in range(1, 9)]
    # mcr_pool_level keeps its two modes: "weighted" is no third one
    assert L.mcr_pool_level(ctypes.c_uint64(0), 0, 0, 4, 2) == MCR_ERR_ARG


def test_debug_level_stats_argument_errors(lib):
    """mcr_debug_level_stats refuses a NULL required pointer, num_envs < 1, num_agents outside 1..8 and K < 1 with MCR_ERR_ARG and a message —
    before any HIP call: this box has no device, and the pointers are host memory no launch could take"""
    L = lib.load()
    assert lib.SYMBOLS["mcr_debug_level_stats"] == (ctypes.c_int, [ctypes.c_void_p] * 5 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 3)
    buf = np.zeros(64)
    p = lib.ptr(buf)
    good = dict(done=p, trunc=p, ret=p, len=p, level=p, B=4, N=2, K=3, fin=p, stats=p)

    def call(**kw):
        a = dict(good, **kw)
        L.mcr_level_stats_dim(1)                               # (an OK call does not touch the message: put a known one there first)
        assert L.mcr_level_stats_dim(0) == MCR_ERR_ARG and b"mcr_level_stats_dim" in L.mcr_last_error()
        return L.mcr_debug_level_stats(a["done"], a["trunc"], a["ret"], a["len"], a["level"], a["B"], a["N"], a["K"], a["fin"], a["stats"], None)

    for name in ("done", "ret", "len", "level", "fin", "stats"):
        assert call(**{name: None}) == MCR_ERR_ARG, name
        assert b"mcr_debug_level_stats" in L.mcr_last_error() and b"null" in L.mcr_last_error(), name
    for kw in (dict(B=0), dict(B=-5), dict(N=0), dict(N=9), dict(N=-1), dict(K=0), dict(K=-1)):
        assert call(**kw) == MCR_ERR_ARG, kw
        assert b"mcr_debug_level_stats" in L.mcr_last_error() and b"num_agents 1..8" in L.mcr_last_error(), kw
    # (d_trunc alone may be NULL: with every other argument good that call launches, which is the GPU tests' business)
    assert call(trunc=None, K=0) == MCR_ERR_ARG and b"K >= 1" in L.mcr_last_error()
