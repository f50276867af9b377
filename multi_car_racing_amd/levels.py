"""Level pools: a finite set of K tracks for VecMultiCarRacing(levels=...) — procgen's `num_levels`.  Nothing here needs a GPU.

Level j of `make_levels(K, num_agents, seed)` is the FIRST episode that the env with global index j would get under `seed` on the default
(host-staged) path: track stream RandomState(seed + j), draw stream RandomState((seed + j + 2**31) % 2**32) (vec_env.py's docstring), through the
same bit-exact generator (include/mcr.h: mcr_mt_seed, mcr_episodes_generate).  So a pool is a prefix-stable list — the first K levels do not
depend on how many are made — and level j can be compared with what env j of an ordinary handle plays first.

Which level an env plays in which episode is `pool_level` (include/mcr.h: mcr_pool_level), the function the device evaluates when it
re-stages an env (csrc/k_pool.h): a pure function of (seed, global env index, episode ordinal), independent of batch size and sharding.
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


def pool_level(seed, global_env, episode, K, order="random"):
    """the pool row that the env with global index `global_env` plays in its `episode`-th episode (0: the first)"""
    r = int(_lib.load().mcr_pool_level(ctypes.c_uint64(int(seed) % 2 ** 64), ctypes.c_uint32(int(global_env)), ctypes.c_uint32(int(episode)),
                                       int(K), _lib.LEVEL_ORDER[order]))
    if r < 0:
        raise ValueError(f"pool_level: K must be >= 1, got {K}")
    return r
