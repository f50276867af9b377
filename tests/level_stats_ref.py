"""Host restatement of the level curricula (include/mcr.h: mcr_set_level_sampler, mcr_set_level_stats): the CDF of a weight vector, the
weighted level draw and the per-level episode statistics, in float64 on Python floats / ints — no GPU, no library.

Every operation is written out in the order the definition fixes: the CDF's running sum is an explicit loop in index order, the statistics
add per row and column in step order and within a step in ascending env index, one f64 add each (Python floats are IEEE binary64 and
`x * x` then `+` is a multiply and an add, never an FMA)."""
import math

import numpy as np

M64 = (1 << 64) - 1


def _mix64(x):
    """splitmix64's finaliser (csrc/mcr_common.h: mcr_mix64) on Python ints"""
    x ^= x >> 30; x = (x * 0xbf58476d1ce4e5b9) & M64
    x ^= x >> 27; x = (x * 0x94d049bb133111eb) & M64
    return x ^ (x >> 31)


def uniform(seed, g, k):
    """the f64 uniform in [0, 1) of (seed, global env g, episode ordinal k): the top 53 bits of "random"'s hash, exactly"""
    x = _mix64(_mix64((seed + 0x9e3779b97f4a7c15 * ((k << 32) | g)) & M64))
    return float(x >> 11) * 2.0 ** -53


def cdf(weights):
    """(cdf float64 [K], fell_back): a weight that is not finite or is negative counts as 0, S_j is the running sum in index order,
    cdf[j] = S_j / S_{K-1}; S_{K-1} zero or not finite: the uniform CDF (j + 1) / K and fell_back"""
    w = [float(x) for x in np.asarray(weights, np.float64)]
    K = len(w)
    sums, S = [], 0.0
    for x in w:
        S = S + (x if (math.isfinite(x) and x >= 0.0) else 0.0)
        sums.append(S)
    if S == 0.0 or not math.isfinite(S):
        return np.array([float(j + 1) / float(K) for j in range(K)], np.float64), True
    return np.array([s / S for s in sums], np.float64), False


def weighted_level(seed, g, k, cdf_):
    """the smallest j with u < cdf[j], K - 1 if there is none (a linear scan: the definition, not the kernel's binary search)"""
    u = uniform(seed, g, k)
    for j, c in enumerate(cdf_):
        if u < float(c):
            return j
    return len(cdf_) - 1


class LevelStats:
    """the accumulator behind `vec.level_stats`: feed it the host copies of one step() — the `level` rows from BEFORE the step, the step's
    done / truncated rows and the episode_return / episode_length buffers after it.  `start`: the [K + 1][3 + 2N] sums to go on from
    (zeros without; reset() zeroes as the caller of mcr_set_level_stats does).  `truncated=None` in step(): nothing was truncated."""

    def __init__(self, K, N, start=None):
        self.K, self.N = K, N
        self.stats = [[0.0] * (3 + 2 * N) for _ in range(K + 1)]
        if start is not None:
            start = np.asarray(start, np.float64)
            assert start.shape == (K + 1, 3 + 2 * N)
            self.stats = [[float(x) for x in row] for row in start]
        self.finished = None

    def reset(self):
        self.stats = [[0.0] * (3 + 2 * self.N) for _ in range(self.K + 1)]

    def step(self, level_before, done, truncated, episode_return, episode_length):
        B, N, K = len(done), self.N, self.K
        fin = np.full(B, -1, np.int32)
        for e in range(B):                                 # ascending env index
            if not done[e]:
                continue
            lv = int(level_before[e])
            r = lv if 0 <= lv < K else K
            fin[e] = r
            row = self.stats[r]
            row[0] = row[0] + 1.0
            row[1] = row[1] + (1.0 if (truncated is not None and truncated[e]) else 0.0)
            row[2] = row[2] + float(int(episode_length[e]))
            for a in range(N):
                x = float(episode_return[e][a])
                row[3 + a] = row[3 + a] + x
                sq = x * x
                row[3 + N + a] = row[3 + N + a] + sq
        self.finished = fin
        return fin

    def array(self):
        return np.array(self.stats, np.float64)
