"""The range-finder observation of csrc/k_rangeobs.h restated in numpy float64 (a helper, not a test): the same IEEE operations in the same
order, one rounding to float32 at the end, so that the kernel's tensor can be compared with np.array_equal.  (The kernel's division-free
pre-test, its parking of candidates and its culling are not restated: they must not change a value.)

Inputs are what an oracle env hands out — state(), positions() — its episode (oracle.new_episode: track rows (alpha, beta, x, y)) and the
build's sinf/cosf spec evaluated on the host (mcr_sincos_host)."""
import math

import numpy as np

from tests.state_obs_ref import sincos_host

f64 = np.float64
SIZE = 0.02
TRACK_WIDTH = 40 / 6.0
# gym car_dynamics.py HULL_POLY1..4
HULL_POLY = (
    [(-60, +130), (+60, +130), (+60, +110), (-60, +110)],
    [(-15, +120), (+15, +120), (+20, +20), (-20, 20)],
    [(+25, +20), (+50, -10), (+50, -40), (+20, -90), (-20, -90), (-50, -40), (-50, -10), (-25, +20)],
    [(-50, -120), (+50, -120), (+50, -90), (-50, -90)],
)


def set_order(pts):
    """the vertex order b2PolygonShape::Set gives a convex polygon: counter-clockwise from the right-most vertex (the lower one on a tie)"""
    pts = [tuple(p) for p in pts]
    area2 = sum(pts[i][0] * pts[(i + 1) % len(pts)][1] - pts[(i + 1) % len(pts)][0] * pts[i][1] for i in range(len(pts)))
    if area2 < 0:
        pts = pts[::-1]
    start = max(range(len(pts)), key=lambda i: (pts[i][0], -pts[i][1]))
    return pts[start:] + pts[:start]


def hull_polygons():
    """the four hull fixture polygons: float32 body-frame vertices [n, 2] each — gym's (x * SIZE, y * SIZE) as Box2D stores them, in Set's order"""
    return [np.array([(np.float32(x * SIZE), np.float32(y * SIZE)) for x, y in set_order(poly)], np.float32) for poly in HULL_POLY]


def default_dirs(rays=19, fov=math.pi):
    """(angles f64, dirs f32 [R, 2]) as VecMultiCarRacing(range_rays=, range_fov=) builds them"""
    ang = np.linspace(-fov / 2, fov / 2, rays) if rays > 1 else np.zeros(1, f64)
    return ang, np.stack([np.cos(ang), np.sin(ang)], axis=1).astype(np.float32)


def ray_segments(px, py, ux, uy, ax, ay, bx, by, max_range):
    """min(max_range, min over the hits of t) of the ray p + t u against the segments A[i] -> B[i] (f64 arrays); f64"""
    if len(ax) == 0:
        return f64(max_range)
    ex, ey = bx - ax, by - ay
    wx, wy = ax - px, ay - py
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        den = ux * ey - uy * ex
        t = (wx * ey - wy * ex) / den
        q = (wx * uy - wy * ux) / den
        hit = (den != 0) & (t >= 0) & (q >= 0) & (q <= 1)
    return min(f64(max_range), t[hit].min()) if hit.any() else f64(max_range)


def border_segments(track):
    """the 2 T border segments of a track [T, 4] (alpha, beta, x, y): (ax, ay, bx, by) f64, L_j -> L_i then R_j -> R_i, j = (i - 1) mod T"""
    tx = np.ascontiguousarray(track[:, 2], f64); ty = np.ascontiguousarray(track[:, 3], f64)
    C = np.array([math.cos(b) for b in track[:, 1]], f64); S = np.array([math.sin(b) for b in track[:, 1]], f64)   # the slot stores libm's
    W = f64(40 / 6.0)
    lx, ly, rx, ry = tx - W * C, ty - W * S, tx + W * C, ty + W * S
    j = (np.arange(len(tx)) - 1) % len(tx)
    return (np.concatenate([lx[j], rx[j]]), np.concatenate([ly[j], ry[j]]), np.concatenate([lx, rx]), np.concatenate([ly, ry]))


def hull_segments(pxj, pyj, sj, cj):
    """the world-frame edges of one car's four hull polygons, closing edges included: (ax, ay, bx, by) f64"""
    A, B = [], []
    for poly in hull_polygons():
        v = poly.astype(f64)
        wx = pxj + (cj * v[:, 0] - sj * v[:, 1]); wy = pyj + (sj * v[:, 0] + cj * v[:, 1])
        w = np.stack([wx, wy], axis=1)
        A.append(w); B.append(np.roll(w, -1, axis=0))
    A = np.concatenate(A); B = np.concatenate(B)
    return A[:, 0], A[:, 1], B[:, 0], B[:, 1]


def ranges(L, bodies, positions, track, dirs, max_range):
    """bodies [N,5,6] f32, positions [N,2] f32, track [T,4] f64, dirs [R,2] f32 -> [N, 2, R] f32"""
    N = bodies.shape[0]
    dirs = np.asarray(dirs, np.float32)
    R = len(dirs)
    max_range = f64(np.float32(max_range))
    pos = positions.astype(f64)
    sc = [sincos_host(L, bodies[a, 0, 2]) for a in range(N)]
    border = border_segments(track)
    hulls = [hull_segments(pos[j, 0], pos[j, 1], f64(sc[j][0]), f64(sc[j][1])) for j in range(N)]
    out = np.zeros((N, 2, R), np.float32)
    for a in range(N):
        px, py = pos[a, 0], pos[a, 1]
        s, c = f64(sc[a][0]), f64(sc[a][1])
        fx, fy, rx, ry = -s, c, c, s
        others = [hulls[j] for j in range(N) if j != a]
        opp = tuple(np.concatenate([h[i] for h in others]) for i in range(4)) if others else None
        for k in range(R):
            ck, sk = f64(dirs[k, 0]), f64(dirs[k, 1])
            ux, uy = ck * fx + sk * rx, ck * fy + sk * ry
            out[a, 0, k] = np.float32(ray_segments(px, py, ux, uy, *border, max_range))
            out[a, 1, k] = np.float32(ray_segments(px, py, ux, uy, *opp, max_range)) if opp else np.float32(max_range)
    return out


def of_oracle(L, o, ep, dirs, max_range):
    """the tensor [N, 2, R] of oracle env `o` playing episode `ep`"""
    return ranges(L, o.state()["bodies"], o.positions(), ep["track"], dirs, max_range)
