"""The racecraft controller of csrc/k_driver.h (k_driver<true>) restated in float64 (a helper, not a test), on top of tests/driver_ref.py:
the same IEEE operations in the same order, one rounding to float32 at the end, so that the kernel's actions can be compared bit for bit.
`actions` / `of_oracle` have driver_ref's shape plus the racecraft rows and mask; `branches` reports which rules fired for one car."""
import math

import numpy as np

from tests import driver_ref as D
from tests.state_obs_ref import nearest_tile, sincos_host

PARAMS = 8
LOOK, W_BLOCK, W_PASS, OFF_MAX, D_SAFE, K_F, W_OFF, V_OFF = range(PARAMS)
NAMES = ("look", "w_block", "w_pass", "off_max", "d_safe", "K_f", "w_off", "v_off")
DEFAULTS = (24.0, 3.5, 4.25, 4.5, 16.0, 2.0, 7.5, 15.0)
LOOK_MAX = 64

# the keys of branches(): "leader" is the leader's car index or None, the others are booleans
BRANCHES = ("self_nonfinite", "leader", "step_left", "step_right", "step_flipped", "step_refused", "follow", "follow_zero", "off_road", "ignored")


def default_params(N):
    return np.tile(np.asarray(DEFAULTS, np.float32), (N, 1))


def _counts(px, py, s, c, vx, vy):
    return all(math.isfinite(v) for v in (px, py, s, c, vx, vy))


def cars_of(L, bodies, positions, arrays, cw):
    """per car the kernel's per-lane record: dict(px, py, s, c, vx, vy, i, lat, counts) — every value a Python float (IEEE f64)"""
    tx, ty, tc, ts = arrays
    sgn = -1.0 if cw else 1.0
    out = []
    for a in range(bodies.shape[0]):
        px, py = float(positions[a, 0]), float(positions[a, 1])
        s32, c32 = sincos_host(L, bodies[a, 0, 2])
        with np.errstate(all="ignore"):
            i = nearest_tile(tx, ty, np.float64(px), np.float64(py))
            lat = float(np.float64(sgn) * ((np.float64(px) - tx[i]) * tc[i] + (np.float64(py) - ty[i]) * ts[i]))
        vx, vy = float(bodies[a, 0, 3]), float(bodies[a, 0, 4])
        out.append(dict(px=px, py=py, s=float(s32), c=float(c32), vx=vx, vy=vy, i=i, lat=lat, counts=_counts(px, py, float(s32), float(c32), vx, vy)))
    return out


def car_action(cars, a, arrays, cw, prm, rc, report=None):
    """car a with racecraft row rc ([8] f32) and driver row prm ([10] f32) among `cars` (cars_of) -> [3] float32; report: a dict that
    receives the branches"""
    tx, ty, tc, ts = arrays
    T = len(tx)
    sgn = -1.0 if cw else 1.0
    d = -1 if cw else 1
    me = cars[a]
    q = [float(v) for v in np.asarray(prm, np.float32)]
    w = [float(v) for v in np.asarray(rc, np.float32)]
    rep = dict(self_nonfinite=not me["counts"], leader=None, step_left=False, step_right=False, step_flipped=False, step_refused=False,
               follow=False, follow_zero=False, off_road=False, ignored=sum(1 for b, cb in enumerate(cars) if b != a and not cb["counts"]))
    if report is not None:
        report.update(rep)
    px, py, s, c, vx, vy, i = me["px"], me["py"], me["s"], me["c"], me["vx"], me["vy"], me["i"]
    if not me["counts"]:                     # a car that does not count gets the plain controller (which zeroes what a non-finite value enters)
        return D.car_action(px, py, s, c, vx, vy, i, tx, ty, tc, ts, cw, prm)
    fx, fy, rx, ry = -s, c, c, s
    vf = vx * fx + vy * fy
    G = min(min(max(int(w[LOOK]), 1), LOOK_MAX), (T - 1) // 2)
    # the leader: smallest x among the counting cars within G tiles ahead with x > 0, lowest index among equals
    lead = None; lx = ly = lvb = 0.0
    for b, cb in enumerate(cars):
        if b == a or not cb["counts"]:
            continue
        g = ((cb["i"] - i) * d) % T
        ux, uy = cb["px"] - px, cb["py"] - py
        x = ux * fx + uy * fy
        y = ux * rx + uy * ry
        vb = cb["vx"] * fx + cb["vy"] * fy
        if g <= G and x > 0.0 and (lead is None or x < lx):
            lead, lx, ly, lvb = b, x, y, vb
    o = q[D.OFFSET]
    cap = None
    if lead is not None:
        rep["leader"] = lead
        ll = cars[lead]["lat"]
        if abs(ll - o) < w[W_BLOCK]:
            left, right = ll - w[W_PASS], ll + w[W_PASS]
            lo, hi = -w[OFF_MAX], w[OFF_MAX]
            go_left = me["lat"] < ll
            first, second = (left, right) if go_left else (right, left)
            if lo <= first <= hi:
                o = first; rep["step_left" if go_left else "step_right"] = True
            elif lo <= second <= hi:
                o = second; rep["step_flipped"] = True; rep["step_right" if go_left else "step_left"] = True
            else:
                rep["step_refused"] = True
        if abs(ly) < w[W_BLOCK]:
            cap = lvb + w[K_F] * (lx - w[D_SAFE])
            if cap < 0.0:
                cap = 0.0; rep["follow_zero"] = True
    so = sgn * o

    def kappa(m):
        t = (i + d * m) % T
        ux = (float(tx[t]) + so * float(tc[t])) - px
        uy = (float(ty[t]) + so * float(ts[t])) - py
        x = ux * fx + uy * fy
        y = ux * rx + uy * ry
        den = x * x + y * y
        return 0.0 if den == 0.0 else D._div(2.0 * y, den)

    k1 = kappa(int(q[D.L1])); k2 = kappa(int(q[D.L2]))
    with np.errstate(all="ignore"):
        rs = float(np.float64(q[D.K_S]) * np.float64(k1))
        vstar = D._div(q[D.V_MAX], float(np.float64(1.0) + np.float64(q[D.K_C]) * np.float64(abs(k2))))
        if cap is not None and cap < vstar:
            vstar = cap; rep["follow"] = True
        if abs(me["lat"]) > w[W_OFF] and w[V_OFF] < vstar:
            vstar = w[V_OFF]; rep["off_road"] = True
        e = float(np.float64(vstar) - np.float64(vf))
        rg = float(np.float64(q[D.K_G]) * np.float64(e))
        rb = float(np.float64(-q[D.K_B]) * np.float64(e))
    if report is not None:
        report.update(rep)
    steer = D._clamp(rs, -1.0, 1.0) if D._finite(rs) else 0.0
    gas = D._clamp(rg, 0.0, q[D.GAS_MAX]) if D._finite(k2) and D._finite(rg) else 0.0
    brake = D._clamp(rb, 0.0, q[D.BRAKE_MAX]) if D._finite(k2) and D._finite(rb) else 0.0
    return np.array([steer, gas, brake], np.float64).astype(np.float32)


def actions(L, bodies, positions, arrays, cw, params, rc_params, rc_mask, reports=None):
    """bodies [N,5,6] f32, positions [N,2] f32, arrays = driver_ref.track_arrays(track), params [N,10] f32, rc_params [N,8] f32, rc_mask:
    bit a = car a races -> [N,3] f32: every car's action (a car outside rc_mask: driver_ref's).  reports: a list that receives one
    branches dict per car (None for a car outside the mask)"""
    N = bodies.shape[0]
    tx, ty, tc, ts = arrays
    cars = cars_of(L, bodies, positions, arrays, cw)
    out = np.zeros((N, 3), np.float32)
    for a in range(N):
        me = cars[a]
        rep = None
        if (rc_mask >> a) & 1:
            rep = {}
            out[a] = car_action(cars, a, arrays, cw, params[a], rc_params[a], rep)
        else:
            out[a] = D.car_action(me["px"], me["py"], me["s"], me["c"], me["vx"], me["vy"], me["i"], tx, ty, tc, ts, cw, params[a])
        if reports is not None:
            reports.append(rep)
    return out


def branches(L, bodies, positions, arrays, cw, params, rc_params, a):
    """which rules fired for car a (racing): dict over BRANCHES"""
    rep = {}
    car_action(cars_of(L, bodies, positions, arrays, cw), a, arrays, cw, params[a], rc_params[a], rep)
    return rep


def _arrays(ep):
    if "_driver_arrays" not in ep:
        ep["_driver_arrays"] = D.track_arrays(ep["track"])
    return ep["_driver_arrays"]


def of_oracle(L, o, ep, params, rc_params, rc_mask, reports=None):
    """the actions [N, 3] of oracle env `o` playing episode `ep`"""
    return actions(L, o.state()["bodies"], o.positions(), _arrays(ep), ep["direction"] == "CW", np.asarray(params, np.float32),
                   np.asarray(rc_params, np.float32), rc_mask, reports)


def branches_of_oracle(L, o, ep, params, rc_params, a):
    return branches(L, o.state()["bodies"], o.positions(), _arrays(ep), ep["direction"] == "CW", np.asarray(params, np.float32),
                    np.asarray(rc_params, np.float32), a)
