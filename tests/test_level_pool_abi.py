"""CPU: the level pool's C ABI (include/mcr.h: mcr_pool_level / mcr_set_episode_pool) and the pool generator
(multi_car_racing_amd/levels.py) — no GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1


def _mix64(x):
    """splitmix64's finaliser (csrc/mcr_common.h: mcr_mix64) on Python ints"""
    x ^= x >> 30; x = (x * 0xbf58476d1ce4e5b9) & M64
    x ^= x >> 27; x = (x * 0x94d049bb133111eb) & M64
    return x ^ (x >> 31)


def _level(seed, g, k, K, mode):
    """the issue's formula, restated"""
    if mode == 1:
        return (g + k) % K
    return _mix64(_mix64((seed + 0x9e3779b97f4a7c15 * ((k << 32) | g)) & M64)) % K


def _c_level(L, seed, g, k, K, mode):
    return int(L.mcr_pool_level(ctypes.c_uint64(seed), ctypes.c_uint32(g), ctypes.c_uint32(k), K, mode))


def test_symbols_exported_and_declared(lib):
    L = lib.load()
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcr.h")).read(), flags=re.S)
    assert re.search(r"\bint32_t\s+mcr_pool_level\s*\(\s*uint64_t\s+seed\s*,\s*uint32_t\s+global_env\s*,\s*uint32_t\s+episode\s*,\s*int32_t\s+K\s*,\s*int\s+mode\s*\)", code)
    assert re.search(r"\bint\s+mcr_set_episode_pool\s*\(\s*mcr_env\s*\*\s*h\s*,\s*const\s+void\s*\*\s*d_pool\s*,\s*int\s+K\s*,\s*uint64_t\s+seed\s*,\s*uint32_t\s+env_offset\s*,"
                     r"\s*int\s+mode\s*,\s*int32_t\s*\*\s*d_level\s*\)", code)
    for n in ("mcr_pool_level", "mcr_set_episode_pool"):
        assert hasattr(L, n), f"{n} is not exported by libmcr_hip.so"
        assert n in lib.SYMBOLS
    # argument checks that need no device: a NULL handle, a NULL pool
    assert L.mcr_set_episode_pool(None, None, 3, ctypes.c_uint64(0), ctypes.c_uint32(0), 0, None) == -1


def test_pool_level_is_a_pure_function_in_range(lib):
    L = lib.load()
    rng = np.random.RandomState(11)
    for _ in range(300):
        seed = int(rng.randint(0, 2 ** 32)) << 32 | int(rng.randint(0, 2 ** 32))
        g = int(rng.randint(0, 2 ** 32)); k = int(rng.randint(0, 2 ** 32)); K = int(rng.randint(1, 5000)); mode = int(rng.randint(0, 2))
        v = _c_level(L, seed, g, k, K, mode)
        assert 0 <= v < K and v == _c_level(L, seed, g, k, K, mode)
        assert v == _level(seed, g, k, K, mode), (seed, g, k, K, mode)
    # small arguments, as a rollout uses them; K = 1; the cycle
    for seed in (0, 1, 7, 2 ** 63 + 5):
        for g in range(6):
            for k in range(5):
                for K in (1, 2, 3, 256):
                    assert _c_level(L, seed, g, k, K, 0) == _level(seed, g, k, K, 0)
                    assert _c_level(L, seed, g, k, K, 1) == (g + k) % K
                assert _c_level(L, seed, g, k, 1, 0) == 0
    assert _c_level(L, 3, 2 ** 32 - 1, 2 ** 32 - 1, 7, 1) == (2 ** 33 - 2) % 7         # the sum does not wrap
    # mode 0 spreads: 4096 envs over 256 levels in one episode use (nearly) all of them, and an env's levels change with the episode
    first = [_c_level(L, 5, g, 0, 256, 0) for g in range(4096)]
    assert len(set(first)) >= 250
    assert len({_c_level(L, 5, 9, k, 256, 0) for k in range(64)}) >= 50
    # errors: K < 1, a bad mode
    assert _c_level(L, 0, 0, 0, 0, 0) == -1 and _c_level(L, 0, 0, 0, -3, 1) == -1 and _c_level(L, 0, 0, 0, 4, 2) == -1 and _c_level(L, 0, 0, 0, 4, -1) == -1


def test_python_pool_level_wraps_the_c_function(lib):
    from multi_car_racing_amd import levels
    L = lib.load()
    for order, mode in (("random", 0), ("cycle", 1)):
        for g, k, K in ((0, 0, 3), (5, 2, 3), (4099, 17, 256)):
            assert levels.pool_level(13, g, k, K, order) == _c_level(L, 13, g, k, K, mode)
    with pytest.raises(ValueError):
        levels.pool_level(0, 0, 0, 0)


def test_make_levels_is_deterministic_and_prefix_stable(lib):
    from multi_car_racing_amd import levels
    b5, i5 = levels.make_levels(5, 2, 40, 2)
    b5b, i5b = levels.make_levels(5, 2, 40, 2, threads=1)
    b3, i3 = levels.make_levels(3, 2, 40, 2)
    assert b5.dtype == np.uint8 and b5.shape == (5, lib.episode_bytes()) and i5.shape == (5, 12) and i5.dtype == np.int32
    assert np.array_equal(b5, b5b) and np.array_equal(i5, i5b)
    assert np.array_equal(b5[:3], b3) and np.array_equal(i5[:3], i3)
    assert len({b.tobytes() for b in b5}) == 5                     # five different tracks
    assert not np.array_equal(levels.make_levels(2, 2, 41, 2)[0][0], b5[0])
    assert np.array_equal(levels.make_levels(2, 2, 41, 2)[0][0], b5[1])        # level j of seed s = level 0 of seed s + j
    with pytest.raises(ValueError):
        levels.make_levels(0, 2, 0)


@pytest.mark.parametrize("N,direction_mode", [(1, 0), (2, 2), (3, 1)])
def test_level_j_is_the_first_episode_of_global_env_j(lib, N, direction_mode):
    """row j = what the per-env path (vec_env.py: _generate) produces first for the env whose streams are seeded with seed + j"""
    from multi_car_racing_amd import levels
    L = lib.load()
    seed, K = 2 ** 32 - 2, 4                                        # (the seeds wrap at 2**32, as the env's do)
    blobs, info = levels.make_levels(K, N, seed, direction_mode)
    for j in range(K):
        g = (seed + j) % 2 ** 32
        mt_t = np.zeros(lib.MT_WORDS, np.uint32); mt_d = np.zeros(lib.MT_WORDS, np.uint32)
        L.mcr_mt_seed(lib.ptr(mt_t), ctypes.c_uint32(g)); L.mcr_mt_seed(lib.ptr(mt_d), ctypes.c_uint32((g + 2 ** 31) % 2 ** 32))
        blob = np.zeros(lib.episode_bytes(), np.uint8); row = np.zeros(12, np.int32)
        assert L.mcr_episodes_generate(lib.ptr(mt_t), lib.ptr(mt_d), 1, N, direction_mode, lib.ptr(blob), lib.ptr(row), 1) == 0
        assert np.array_equal(blobs[j], blob) and np.array_equal(info[j], row), f"level {j}"
        ep = lib.unpack_episode(blobs[j])
        assert ep["T"] == info[j, 0] and ep["P"] == info[j, 1] and bool(info[j, 3]) == ep["cw"]
        if direction_mode != 2:
            assert ep["cw"] == (direction_mode == 1)
