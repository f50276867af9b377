"""Level pools: a finite set of K tracks for VecMultiCarRacing(levels=...) — procgen's `num_levels`.  Nothing here needs a GPU.

Level j of `make_levels(K, num_agents, seed)` is the FIRST episode that the env with global index j would get under `seed` on the default
(host-staged) path: track stream RandomState(seed + j), draw stream RandomState((seed + j + 2**31) % 2**32) (vec_env.py's docstring), through the
same bit-exact generator (include/mcr.h: mcr_mt_seed, mcr_episodes_generate).  So a pool is a prefix-stable list — the first K levels do not
depend on how many are made — and level j can be compared with what env j of an ordinary handle plays first.

Which level an env plays in which episode is `pool_level` (include/mcr.h: mcr_pool_level), the function the device evaluates when it
re-stages an env (csrc/k_pool.h): a pure function of (seed, global env index, episode ordinal), independent of batch size and sharding.

Curricula (`level_order="weighted"`, include/mcr.h: mcr_set_level_sampler): `level_cdf(weights)` is the CDF that
VecMultiCarRacing.set_level_weights builds on the device and `weighted_level(seed, g, k, cdf)` the level it gives — the same hash as
"random", mapped through the CDF in force when the episode was STAGED, one episode before the env plays it.  `pool_level` cannot answer for
"weighted": it has no CDF.
"""
import ctypes

import numpy as np

from . import _lib


def make_levels(K, num_agents=2, seed=0, direction_mode=2, threads=None):
    """K episode blobs and their info rows: (uint8 [K, episode_bytes], int32 [K, 12]: T, P, retries, cw, car_order[8]).
    direction_mode: 0 'CCW', 1 'CW', 2 drawn per level (mcr_episodes_generate)."""
    K = int(K)
    if K < 1:
        raise ValueError(f"a level pool needs K >= 1 levels, got {K}")
    if not 1 <= int(num_agents) <= _lib.MAX_AGENTS:
        raise ValueError(f"num_agents must be 1..{_lib.MAX_AGENTS}, got {num_agents}")
    if int(direction_mode) not in (0, 1, 2):
        raise ValueError(f"direction_mode must be 0 (CCW), 1 (CW) or 2 (random), got {direction_mode}")
    L = _lib.load()
    mt_track = np.zeros((K, _lib.MT_WORDS), np.uint32)
    mt_draw = np.zeros((K, _lib.MT_WORDS), np.uint32)
    for j in range(K):
        g = (int(seed) + j) % 2 ** 32
        L.mcr_mt_seed(_lib.ptr(mt_track[j]), ctypes.c_uint32(g))
        L.mcr_mt_seed(_lib.ptr(mt_draw[j]), ctypes.c_uint32((g + 2 ** 31) % 2 ** 32))
    blobs = np.zeros((K, _lib.episode_bytes()), np.uint8)
    info = np.zeros((K, 12), np.int32)
    threads = max(1, min(int(threads or _lib.effective_cpus()), K))
    _lib.check(L.mcr_episodes_generate(_lib.ptr(mt_track), _lib.ptr(mt_draw), K, int(num_agents), int(direction_mode),
                                       _lib.ptr(blobs), _lib.ptr(info), threads), "mcr_episodes_generate")
    return blobs, info


def from_tracks(tracks, num_agents=2, direction="CCW", car_order=None):
    """Episode blobs of the caller's own tracks (include/mcr.h: mcr_episode_from_track): uint8 [K, episode_bytes] for `levels=`.
    tracks: K arrays [T, 4] float64, rows (alpha, beta, x, y) — beta the heading of the tile's edge, the track running along (-sin beta, cos beta);
    direction: 'CCW' / 'CW', or one per track; car_order: the grid order of the cars (default 0 .. num_agents-1)."""
    tracks = list(tracks)
    if len(tracks) < 1:
        raise ValueError("from_tracks needs at least one track")
    N = int(num_agents)
    if not 1 <= N <= _lib.MAX_AGENTS:
        raise ValueError(f"num_agents must be 1..{_lib.MAX_AGENTS}, got {num_agents}")
    dirs = [direction] * len(tracks) if isinstance(direction, str) else list(direction)
    if len(dirs) != len(tracks) or any(d not in ("CCW", "CW") for d in dirs):
        raise ValueError("direction must be 'CCW' or 'CW', or one of them per track")
    order = np.ascontiguousarray(np.arange(N) if car_order is None else car_order, dtype=np.int32)
    if order.shape != (N,):
        raise ValueError(f"car_order must have shape [{N}], got {list(order.shape)}")
    L = _lib.load()
    blobs = np.zeros((len(tracks), _lib.episode_bytes()), np.uint8)
    for j, (tr, d) in enumerate(zip(tracks, dirs)):
        tr = np.ascontiguousarray(tr, dtype=np.float64)
        if tr.ndim != 2 or tr.shape[1] != 4:
            raise ValueError(f"track {j} must have shape [T, 4] (alpha, beta, x, y), got {list(tr.shape)}")
        rc = L.mcr_episode_from_track(_lib.ptr(tr), len(tr), N, int(d == "CW"), _lib.ptr(order), _lib.ptr(blobs[j]), None)
        if rc != 0:
            raise ValueError(f"track {j}: T must be 20..{_lib.TILE_CAP}, every entry finite, and tiles plus kerbs at most {_lib.QUAD_CAP} (T = {len(tr)})")
    return blobs


def pool_level(seed, global_env, episode, K, order="random"):
    """the pool row that the env with global index `global_env` plays in its `episode`-th episode (0: the first)"""
    if order == "weighted":
        raise ValueError("pool_level: the level of a weighted pool depends on the CDF in force when it was staged: use weighted_level(seed, g, k, cdf)")
    r = int(_lib.load().mcr_pool_level(ctypes.c_uint64(int(seed) % 2 ** 64), ctypes.c_uint32(int(global_env)), ctypes.c_uint32(int(episode)),
                                       int(K), _lib.LEVEL_ORDER[order]))
    if r < 0:
        raise ValueError(f"pool_level: K must be >= 1, got {K}")
    return r


def level_cdf(weights):
    """(cdf float64 [K], fell_back bool) of a weight vector (include/mcr.h: mcr_level_cdf): a weight that is not finite or is negative counts
    as 0, the running sum goes in index order, and a total that is 0 or not finite gives the uniform CDF with fell_back set."""
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.ndim != 1 or len(w) < 1:
        raise ValueError("level_cdf: weights must be a 1-D sequence of K >= 1 values")
    cdf = np.zeros(len(w), np.float64)
    return cdf, bool(_lib.check(_lib.load().mcr_level_cdf(_lib.ptr(w), len(w), _lib.ptr(cdf)), "mcr_level_cdf"))


def weighted_level(seed, global_env, episode, cdf):
    """the pool row that `cdf` (level_cdf) gives the env with global index `global_env` for its `episode`-th episode (0: the first)"""
    c = np.ascontiguousarray(cdf, dtype=np.float64)
    if c.ndim != 1 or len(c) < 1:
        raise ValueError("weighted_level: cdf must be a 1-D sequence of K >= 1 values")
    return int(_lib.load().mcr_pool_level_weighted(ctypes.c_uint64(int(seed) % 2 ** 64), ctypes.c_uint32(int(global_env)),
                                                   ctypes.c_uint32(int(episode)), _lib.ptr(c), len(c)))


def check_weights(weights, K):
    """Host validation of a weight vector for K levels, as set_level_weights(check=True) applies it: float64 [K], every value finite and
    >= 0, sum > 0 and finite.  Returns the float64 array; ValueError otherwise."""
    try:
        w = np.ascontiguousarray(weights, dtype=np.float64)
    except (TypeError, ValueError) as exc:
        raise ValueError(f"level weights must be numbers: {exc}") from None
    if w.ndim != 1 or len(w) != int(K):
        raise ValueError(f"level weights must have shape [{int(K)}], got {list(w.shape)}")
    if not np.isfinite(w).all():
        raise ValueError("level weights must be finite")
    if (w < 0).any():
        raise ValueError("level weights must be >= 0")
    if level_cdf(w)[1]:
        raise ValueError("level weights must have a finite sum > 0")
    return w
