"""The state-vector observation of csrc/k_stateobs.h restated in numpy float64 (a helper, not a test): the same IEEE operations in the same
order, one rounding to float32 at the end, so that the kernel's rows can be compared with np.array_equal.

Inputs are what an oracle env hands out — state(), env_state(), positions() — its episode (oracle.new_episode: track rows (alpha, beta, x, y),
direction) and the build's sinf/cosf spec evaluated on the host (mcr_sincos_host)."""
import ctypes
import math

import numpy as np

BASE = 18


def dim(N, K=6):
    return BASE + 2 * K + 4 * (N - 1)


def sincos_host(L, a):
    """(s, c) = mcr_sincosf(a) as float32 values (L: the loaded libmcr_hip.so)"""
    s, c = ctypes.c_float(), ctypes.c_float()
    L.mcr_sincos_host(ctypes.c_float(float(a)), ctypes.byref(s), ctypes.byref(c))
    return np.float32(s.value), np.float32(c.value)


def nearest_tile(tx, ty, px, py):
    """argmin over the tiles of dx dx + dy dy in f64, lowest index among ties"""
    dx = px - tx; dy = py - ty
    return int(np.argmin(dx * dx + dy * dy))


def features(L, bodies, wheels, on_road, tvc, positions, track, cw, K=6, stride=5):
    """bodies [N,5,6] f32, wheels [N,4,5] f64, on_road [N,4], tvc [N], positions [N,2] f32, track [T,4] f64 rows (alpha, beta, x, y) -> [N, F] f32"""
    N = bodies.shape[0]
    T = len(track)
    f64 = np.float64
    tx = np.ascontiguousarray(track[:, 2], f64); ty = np.ascontiguousarray(track[:, 3], f64)
    sgn = f64(-1.0 if cw else 1.0)
    d = -1 if cw else 1
    out = np.zeros((N, dim(N, K)), np.float32)
    pos = positions.astype(f64)
    for a in range(N):
        px, py = pos[a, 0], pos[a, 1]
        vx, vy = f64(bodies[a, 0, 3]), f64(bodies[a, 0, 4])
        s32, c32 = sincos_host(L, bodies[a, 0, 2])
        s, c = f64(s32), f64(c32)
        fx, fy, rx, ry = -s, c, c, s
        i = nearest_tile(tx, ty, px, py)
        C, S = f64(math.cos(track[i, 1])), f64(math.sin(track[i, 1]))       # the slot stores libm's cos / sin of beta
        dx, dy = px - tx[i], py - ty[i]
        row = np.zeros(out.shape[1], f64)
        row[0] = vx * fx + vy * fy
        row[1] = vx * rx + vy * ry
        row[2] = f64(bodies[a, 0, 5])
        row[3:7] = wheels[a, :, 4]
        row[7] = f64(bodies[a, 1, 2]) - f64(bodies[a, 0, 2])
        row[8:12] = (np.asarray(on_road[a]) != 0).astype(f64)
        row[12] = f64(int(tvc[a])) / f64(T)
        row[13] = dx * C + dy * S
        row[14] = -dx * S + dy * C
        row[15] = sgn * (c * C + s * S)
        row[16] = sgn * (s * C - c * S)
        row[17] = sgn
        for m in range(1, K + 1):
            t = (i + d * m * stride) % T
            ux, uy = tx[t] - px, ty[t] - py
            row[BASE + 2 * (m - 1)] = ux * fx + uy * fy
            row[BASE + 2 * (m - 1) + 1] = ux * rx + uy * ry
        o = BASE + 2 * K
        for j in range(N):
            if j == a:
                continue
            ux, uy = pos[j, 0] - px, pos[j, 1] - py
            wx, wy = f64(bodies[j, 0, 3]) - vx, f64(bodies[j, 0, 4]) - vy
            row[o] = ux * fx + uy * fy; row[o + 1] = ux * rx + uy * ry
            row[o + 2] = wx * fx + wy * fy; row[o + 3] = wx * rx + wy * ry
            o += 4
        out[a] = row.astype(np.float32)
    return out


def of_oracle(L, o, ep, K=6, stride=5):
    """the rows [N, F] of oracle env `o` playing episode `ep`"""
    st = o.state(); es = o.env_state()
    return features(L, st["bodies"], st["wheels"], st["on_road"], es["tile_visited_count"], o.positions(), ep["track"],
                    ep["direction"] == "CW", K, stride)
