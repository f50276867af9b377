"""Synthetic pose sets for racecraft (csrc/k_driver.h, k_driver<true>; a helper, not a test), on the tracks and the `Rig` of
tests/obs_cases.py: each set is named for the branch of the definition it is built to take for CAR 0, and
tests/test_racecraft_cases.py holds it to that branch through racecraft_ref.branches without a GPU; tests/test_gpu_racecraft_kernel.py
runs the kernel on the same bodies.

A pose is (tile offset from the env's anchor along the driving direction, metres along the track's tangent, lateral position — positive to
the right of the driving direction — and forward speed); the car heads down the track.  On the circles a lateral displacement is radial,
so the nearest point stays the anchor's.  The other cars of a set ("fillers") stand in pairs behind car 0, beyond every look-ahead.
The parameter rows of a set hold for every env of the handle (they travel by value with the launch): SETS[name] = (poses, overrides of the
racecraft row)."""
import math

import numpy as np

from tests import driver_ref as D
from tests import obs_cases as C
from tests import racecraft_ref as R
from tests.util import hull_positions

f32 = np.float32
NS = (2, 4, 8)


def tracks(lib):
    return C.driver_tracks(lib)


def anchor(e, T, seam=False):
    """the tile car 0 stands on: away from the index seam, or two tiles in front of it (a leader three tiles on is across it)"""
    if seam:
        return T - 2 if e % 2 == 0 else 1          # (tracks come in pairs CCW, CW: the CCW car looks from T - 2 to 1, the CW car from 1 to T - 2)
    return (5 + 3 * e) % T


def pose(rows, cw, i0, off, along, lat, speed, turn=0.0):
    """(px, py, angle, vx, vy) of a car `off` tiles down the track from tile i0, `along` further along that tile's tangent, `lat` to the right"""
    T = len(rows); d = -1 if cw else 1; sgn = -1.0 if cw else 1.0
    i = (i0 + d * off) % T
    b = float(rows[i, 1])
    h = b - (math.pi if cw else 0.0) + turn
    tx, ty = -math.sin(b) * d, math.cos(b) * d                  # the driving direction at tile i
    px = float(rows[i, 2]) + sgn * lat * math.cos(b) + along * tx
    py = float(rows[i, 3]) + sgn * lat * math.sin(b) + along * ty
    return px, py, h, -math.sin(h) * speed, math.cos(h) * speed


def fillers(n):
    """n cars in pairs behind car 0: (off, along, lat, speed)"""
    return [(-(1 + k // 2), 0.0, 3.0 if k % 2 else -3.0, 5.0 + k) for k in range(n)]


def _G(T, look):
    return min(int(look), (T - 1) // 2)


# name -> (car 0, the cars that matter besides it, racecraft overrides, seam) — each car (off, along, lat, speed), `off` may be a function of T
SETS = {
    "queue":          None,                                                                    # built below: every car has the next one ahead
    "seam":           ((0, 0.0, -0.5, 30.0), [(3, 0.0, 0.0, 10.0)], {}, True),
    "clamp_in":       ((0, 0.0, 0.0, 30.0), [(lambda T: _G(T, 64), 0.0, 0.0, 10.0)], {"look": 64.0}, False),
    "clamp_out":      ((0, 0.0, 0.0, 30.0), [(lambda T: _G(T, 64) + 1, 0.0, 0.0, 10.0)], {"look": 64.0}, False),
    "behind":         ((0, 0.0, 0.0, 30.0), [(-2, 0.0, 0.0, 40.0)], {}, False),
    "twins":          ((0, 0.0, -0.5, 30.0), [(3, 0.0, 0.0, 35.0), (3, 0.0, 0.0, 38.0)], {}, False),          # (caps 35 / 38 - 2 (16 - gap): inside the brake's range)
    "tile_ahead":     ((0, 0.0, -0.5, 30.0), [(0, 1.0, 0.0, 10.0)], {}, False),
    "tile_behind":    ((0, 0.0, -0.5, 30.0), [(0, -1.0, 0.0, 10.0)], {}, False),
    "step_left":      ((0, 0.0, -0.5, 30.0), [(3, 0.0, 0.0, 25.0)], {}, False),
    "step_right":     ((0, 0.0, 0.5, 30.0), [(3, 0.0, 0.0, 25.0)], {}, False),
    "step_flipped":   ((0, 0.0, -2.0, 30.0), [(3, 0.0, -1.0, 25.0)], {}, False),
    "step_refused":   ((0, 0.0, -0.5, 30.0), [(3, 0.0, 0.0, 25.0)], {"off_max": 1.0}, False),
    "follow_zero":    ((0, 0.0, 0.0, 30.0), [(2, 0.0, 0.0, 0.0)], {}, False),
    "w_off_above":    ((0, 0.0, "w_off+", 30.0), [], {}, False),
    "w_off_below":    ((0, 0.0, "w_off-", 30.0), [], {}, False),
    "other_nonfinite": ((0, 0.0, -0.5, 30.0), [(3, 0.0, "nonfinite", 10.0)], {}, False),
    "self_nonfinite": ((0, 0.0, "nonfinite", 30.0), [(3, 0.0, 0.0, 10.0)], {}, False),
}
QUEUE_LATS = (0.0, 0.5, -3.8, 0.0, 3.9, -0.25, 1.0, 0.0)


def rc_rows(N, name):
    rows = R.default_params(N)
    over = {} if SETS[name] is None else SETS[name][2]
    for k, v in over.items():
        rows[:, R.NAMES.index(k)] = f32(v)
    return rows


def drv_rows(N):
    """car 0 the defaults; the others rows of their own (look-aheads, offsets, speeds)"""
    p = D.default_params(N)
    for a in range(1, N):
        p[a, D.L1] = (1, 4, 64)[a % 3]; p[a, D.L2] = (64, 1, 4)[(a // 2) % 3]
        p[a, D.OFFSET] = (1.0, -1.0, 0.0)[a % 3]; p[a, D.V_MAX] = 20.0 + 9.0 * a
    return np.ascontiguousarray(p, f32)


def _lat0(L, body, rows, cw):
    pos = hull_positions(L, body[None])
    return R.cars_of(L, body[None], pos, D.track_arrays(rows), cw)[0]["lat"]


def _at_w_off(L, base, rows, cw, i0, above, speed):
    """car 0 with lat_0 on one side of the default w_off, ONE float32 step of its hull centre from the other side: `above` -> the smallest
    lat_0 > w_off along that walk, else the value one step before it (<= w_off)"""
    w = float(f32(R.DEFAULTS[R.W_OFF]))
    b = C.place(L, base, *pose(rows, cw, i0, 0, 0.0, w, speed))
    sgn = -1.0 if cw else 1.0
    beta = float(rows[i0, 1])
    k = 0 if abs(math.cos(beta)) >= abs(math.sin(beta)) else 1          # walk the hull centre's larger radial component
    up = f32(np.inf) if sgn * (math.cos(beta), math.sin(beta))[k] > 0 else f32(-np.inf)

    def step(body, to):
        nb = body.copy()
        delta = np.nextafter(nb[0, k], to) - nb[0, k]
        nb[:, k] += delta; nb[0, k] = np.nextafter(body[0, k], to)
        return nb
    for _ in range(64):                     # back to lat <= w_off ...
        if _lat0(L, b, rows, cw) <= w:
            break
        b = step(b, -up)
    for _ in range(64):                     # ... then up to the first lat > w_off
        nb = step(b, up)
        if _lat0(L, nb, rows, cw) > w:
            return nb if above else b
        b = nb
    raise AssertionError("no float32 step across w_off found")


def pose_sets(L, trks, N, base):
    """{name: bodies [B, N, 5, 6] f32} for the sets that exist at this N (twins needs three cars) — base: the rig's get_state()["bodies"],
    or zeros on a box without a device (only the hulls' rows are read)"""
    B = len(trks)
    out = {}
    for name, spec in SETS.items():
        if name == "twins" and N < 3:
            continue
        bodies = np.zeros((B, N, 5, 6), f32)
        for e, (_, rows, cw) in enumerate(trks):
            T = len(rows)
            if spec is None:
                cars = [(k, 0.0, QUEUE_LATS[k], 30.0 - 3.0 * k) for k in range(N)]      # (one tile apart: on 20 tiles eight cars stay inside half a lap)
                i0 = anchor(e, T)
            else:
                car0, others, _, seam = spec
                others = others[:N - 1]
                cars = [car0] + list(others) + fillers(N - 1 - len(others))
                i0 = anchor(e, T, seam)
            for a, (off, along, lat, speed) in enumerate(cars):
                off = off(T) if callable(off) else off
                if lat in ("w_off+", "w_off-"):
                    bodies[e, a] = _at_w_off(L, base[e, a], rows, cw, i0, lat == "w_off+", speed)
                    continue
                bad = lat == "nonfinite"
                px, py, h, vx, vy = pose(rows, cw, i0, off, along, 0.0 if bad else lat, speed)
                if bad:                      # NaN position, inf position, inf velocity, NaN angle — by env
                    kind = e % 4
                    px = float("nan") if kind == 0 else px
                    py = float("-inf") if kind == 1 else py
                    vx = float("inf") if kind == 2 else vx
                    h = float("nan") if kind == 3 else h
                bodies[e, a] = C.place(L, base[e, a], px, py, h, vx, vy)
        out[name] = bodies
    return out


def ref_actions(L, trks, bodies, drv, rc, rc_mask, reports=None):
    """[B, N, 3] f32: the restatement on the bodies of one set; reports: a list that receives each env's per-car branches"""
    pos = hull_positions(L, bodies)
    out = []
    with np.errstate(all="ignore"):
        for e, (_, rows, cw) in enumerate(trks):
            reps = []
            out.append(R.actions(L, bodies[e], pos[e], D.track_arrays(rows), cw, drv, rc, rc_mask, reps))
            if reports is not None:
                reports.append(reps)
    return np.stack(out)


# what car 0's branches must say, per set: a predicate over (branches dict, env index, track, cw)
def expect(name, rep, N):
    lead = rep["leader"]
    none = not (rep["step_left"] or rep["step_right"] or rep["step_refused"])
    return {
        "queue": lead == 1,
        "seam": lead == 1 and rep["step_left"],
        "clamp_in": lead == 1,
        "clamp_out": lead is None,
        "behind": lead is None,
        "twins": lead == 1,
        "tile_ahead": lead == 1,
        "tile_behind": lead is None,
        "step_left": lead == 1 and rep["step_left"] and not rep["step_flipped"],
        "step_right": lead == 1 and rep["step_right"] and not rep["step_flipped"],
        "step_flipped": lead == 1 and rep["step_flipped"] and rep["step_right"],
        "step_refused": lead == 1 and rep["step_refused"],
        "follow_zero": lead == 1 and rep["follow"] and rep["follow_zero"],
        "w_off_above": lead is None and rep["off_road"],
        "w_off_below": lead is None and not rep["off_road"],
        "other_nonfinite": lead is None and rep["ignored"] >= 1 and none and not rep["self_nonfinite"],
        "self_nonfinite": rep["self_nonfinite"] and lead is None,
    }[name]
