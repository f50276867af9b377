"""The scripted driver of csrc/k_driver.h restated in float64 (a helper, not a test): the same IEEE operations in the same order, one rounding
to float32 at the end, so that the kernel's actions can be compared with np.array_equal.  Python floats are IEEE doubles and `a * b + c * d`
is evaluated as written (no contraction), which is all the recipe needs.

Inputs are what an oracle env hands out — state(), positions() — its episode (oracle.new_episode: track rows (alpha, beta, x, y), direction),
the build's sinf/cosf spec evaluated on the host (mcr_sincos_host) for the hull, and math.cos / math.sin of beta for the slot's values."""
import math

import numpy as np

from tests.state_obs_ref import nearest_tile, sincos_host

PARAMS = 10
L1, L2, V_MAX, K_S, K_C, K_G, K_B, OFFSET, GAS_MAX, BRAKE_MAX = range(PARAMS)
DEFAULTS = (4.0, 12.0, 70.0, 8.0, 20.0, 0.2, 0.1, 0.0, 1.0, 0.8)


# The closed-loop scenario of tests/test_driver_scenario.py, which holds it to its conditions on the oracle: N = 1, global envs SCENARIO_ENVS of
# SCENARIO_SEED, random direction, the defaults, TimeLimit SCENARIO_TIME_LIMIT.  DRIVER_LAP is the run tests/test_gpu_driver.py repeats on the
# device: (seed, global env, the step — counted from 1 — in which `done` is raised by lap completion).
SCENARIO_SEED = 500
SCENARIO_ENVS = tuple(range(6))
SCENARIO_TIME_LIMIT = 1000
DRIVER_LAP = (500, 0, 832)


def default_params(N):
    return np.tile(np.asarray(DEFAULTS, np.float32), (N, 1))


def _clamp(v, lo, hi):
    """two comparisons; a NaN passes through (the caller has already replaced a non-finite value)"""
    if v < lo:
        v = lo
    if v > hi:
        v = hi
    return v


def _finite(v):
    return math.isfinite(v)


def _div(a, b):
    """IEEE division (Python raises where IEEE returns inf / nan)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def car_action(px, py, s, c, vx, vy, i, tx, ty, tc, ts, cw, prm):
    """one car: px, py, s, c, vx, vy float64 (widened float32 values), i the nearest track point, tx / ty / tc / ts the track's float64 arrays,
    prm the car's float32 parameter row -> [3] float32"""
    T = len(tx)
    sgn = -1.0 if cw else 1.0
    d = -1 if cw else 1
    fx, fy, rx, ry = -s, c, c, s
    q = [float(v) for v in np.asarray(prm, np.float32)]
    vf = vx * fx + vy * fy
    so = sgn * q[OFFSET]

    def kappa(m):
        t = (i + d * m) % T
        ux = (float(tx[t]) + so * float(tc[t])) - px
        uy = (float(ty[t]) + so * float(ts[t])) - py
        x = ux * fx + uy * fy
        y = ux * rx + uy * ry
        den = x * x + y * y
        return 0.0 if den == 0.0 else _div(2.0 * y, den)

    k1 = kappa(int(q[L1])); k2 = kappa(int(q[L2]))
    with np.errstate(all="ignore"):
        rs = float(np.float64(q[K_S]) * np.float64(k1))
        vstar = _div(q[V_MAX], float(np.float64(1.0) + np.float64(q[K_C]) * np.float64(abs(k2))))
        e = float(np.float64(vstar) - np.float64(vf))
        rg = float(np.float64(q[K_G]) * np.float64(e))
        rb = float(np.float64(-q[K_B]) * np.float64(e))
    steer = _clamp(rs, -1.0, 1.0) if _finite(rs) else 0.0
    gas = _clamp(rg, 0.0, q[GAS_MAX]) if _finite(k2) and _finite(rg) else 0.0
    brake = _clamp(rb, 0.0, q[BRAKE_MAX]) if _finite(k2) and _finite(rb) else 0.0
    return np.array([steer, gas, brake], np.float64).astype(np.float32)


def track_arrays(track):
    """track [T,4] f64 rows (alpha, beta, x, y) -> (x, y, cos beta, sin beta) as the episode slot holds them (libm's cos / sin of beta)"""
    f64 = np.float64
    return (np.ascontiguousarray(track[:, 2], f64), np.ascontiguousarray(track[:, 3], f64),
            np.array([math.cos(b) for b in track[:, 1]], f64), np.array([math.sin(b) for b in track[:, 1]], f64))


def actions(L, bodies, positions, arrays, cw, params):
    """bodies [N,5,6] f32, positions [N,2] f32, arrays = track_arrays(track), params [N,10] f32 -> [N,3] f32: every car's action"""
    N = bodies.shape[0]
    f64 = np.float64
    tx, ty, tc, ts = arrays
    out = np.zeros((N, 3), np.float32)
    for a in range(N):
        px, py = f64(positions[a, 0]), f64(positions[a, 1])
        s32, c32 = sincos_host(L, bodies[a, 0, 2])
        i = nearest_tile(tx, ty, px, py)
        out[a] = car_action(float(px), float(py), float(s32), float(c32), float(bodies[a, 0, 3]), float(bodies[a, 0, 4]), i, tx, ty, tc, ts, cw, params[a])
    return out


def of_oracle(L, o, ep, params):
    """the actions [N, 3] of oracle env `o` playing episode `ep`"""
    if "_driver_arrays" not in ep:
        ep["_driver_arrays"] = track_arrays(ep["track"])
    return actions(L, o.state()["bodies"], o.positions(), ep["_driver_arrays"], ep["direction"] == "CW", np.asarray(params, np.float32))
