"""Synthetic tracks and poses for the derived-observation kernels (a helper, not a test): csrc/k_stateobs.h, k_rangeobs.h, k_driver.h and
the search they share, k_nearest.h, driven through their own launches on inputs no rollout reaches — tests/test_gpu_state_obs_kernel.py,
test_gpu_range_obs_kernel.py, test_gpu_driver_kernel.py.

Everything is generated in float64 from fixed formulas and seeds; the same arrays go to levels.from_tracks (what the device holds) and to
the host restatements (tests/state_obs_ref.py, range_obs_ref.py, driver_ref.py).  A `Rig` is one handle whose env e plays track e
(`levels=` the blobs, level_order="cycle"), obs=False, streams=1, reset once, optionally stepped a little so that the cars' wheel speeds,
steering angles and on-road bits differ — and then never stepped again: every case is set_bodies(poses) and a refresh, so teleported cars
(overlapping, off the playfield, NaN) never meet the solver.

The host-side conditions on the inputs (ties that are exact, a ray through a vertex, cars 4-7 being somebody's nearest hit, ...) are
functions of the restatements alone; tests/test_obs_cases.py holds them without a GPU."""
import math

import numpy as np

from tests import driver_ref, range_obs_ref, state_obs_ref
from tests.util import hull_positions, rigid_teleport

f64 = np.float64
W = f64(40 / 6.0)                    # TRACK_WIDTH: a border vertex is (x -+ W cos beta, y -+ W sin beta)
CIRCLE_T = (20, 63, 64, 65, 128, 321, 448, 449, 511, 512)
LATTICE_W, LATTICE_H = 2, 40         # cells of 4.0: T = 2 (W + H) = 84
TRUNCATED_T = 100


# ------------------------------------------------------------------------------------------------------------------------------ tracks
def circle(T, step=3.5):
    """T points `step` apart on a circle round the origin, walked counter-clockwise; beta the tangent heading (a track runs along
    (-sin beta, cos beta))"""
    r = T * step / (2 * math.pi)
    th = 2 * math.pi * np.arange(T) / T
    return np.ascontiguousarray(np.stack([th, th, r * np.cos(th), r * np.sin(th)], axis=1), f64)


def lattice_loop(x0=0.0):
    """A rectangle of LATTICE_W x LATTICE_H cells of 4.0 walked counter-clockwise from its lower right corner, one point per lattice node:
    up the right side (beta 0), along the top (pi / 2), down the left side (pi), along the bottom (-pi / 2); x shifted by x0.
    T = 84: tile y (right side, (8, 4 y)) and tile 82 - y (left side, (0, 4 y)) lie 8 apart — y = 9 gives the pair 9 and 73, 64 apart in
    index (one lane of the search), every other y a pair in two lanes."""
    w, h = LATTICE_W, LATTICE_H
    pts = [(4.0 * w, 4.0 * i, 0.0) for i in range(h)] + [(4.0 * (w - i), 4.0 * h, math.pi / 2) for i in range(w)]
    pts += [(0.0, 4.0 * (h - i), math.pi) for i in range(h)] + [(4.0 * i, 0.0, -math.pi / 2) for i in range(w)]
    a = np.array(pts, f64)
    return np.ascontiguousarray(np.stack([np.arange(len(a)) * (2 * math.pi / len(a)), a[:, 2], a[:, 0] + f64(x0), a[:, 1]], axis=1), f64)


def border_loop():
    """lattice_loop shifted by x0 = W: its left side's points are (W, y) with cos beta = -1 exactly, so that side's RIGHT border vertices are
    (W - W, y + W sin pi) = (0, y) exactly for y >= 8 — a border a float32 pose can stand on, and whose vertices a ray can go through"""
    return lattice_loop(float(W))


def truncated_track(lib, seed=77):
    """the first TRUNCATED_T points of a generated lap: the wrap segment T-1 -> 0 is then hundreds of units long"""
    from multi_car_racing_amd import levels
    blobs, _ = levels.make_levels(1, 1, seed, direction_mode=0, threads=1)
    ep = lib.unpack_episode(np.ascontiguousarray(blobs[0]))
    rows = np.stack([ep["alpha"], ep["track"][:, 2], ep["track"][:, 0], ep["track"][:, 1]], axis=1)
    return np.ascontiguousarray(rows[:TRUNCATED_T], f64)


def all_tracks(lib):
    """[(name, rows [T, 4], cw)]: every track in both directions"""
    base = [(f"circle{T}", circle(T)) for T in CIRCLE_T] + [("lattice", lattice_loop()), ("border", border_loop()), ("truncated", truncated_track(lib))]
    return [(name, rows, cw) for name, rows in base for cw in (False, True)]


def driver_tracks(lib):
    return [t for t in all_tracks(lib) if t[0] in ("circle20", "circle64", "circle65", "circle512")]


# ------------------------------------------------------------------------------------------------------------------------------ poses
def centre_for(L, px, py, angle):
    """the float32 hull centre c with hull_positions(c, angle) == (px, py) where one exists among c's neighbours (angle 0: always), else the
    nearest one"""
    f32 = np.float32
    probe = np.zeros((1, 5, 6), f32); probe[0, 0, 2] = f32(angle)
    off = hull_positions(L, probe)[0].astype(f64)                 # -R(a) lc
    out = []
    for want, o in ((px, off[0]), (py, off[1])):
        c0 = f32(f64(want) - o)
        if not np.isfinite(c0):
            out.append(c0); continue
        cands = [c0]
        for _ in range(3):
            cands = [np.nextafter(cands[0], f32(-np.inf))] + cands + [np.nextafter(cands[-1], f32(np.inf))]
        good = [c for c in cands if f32(c + f32(o)) == f32(want)]
        out.append(good[0] if good else c0)
    return out[0], out[1]


def place(L, base, px, py, angle, vx=None, vy=None):
    """one car's bodies [5, 6] moved so that the hull's body origin is (px, py) and its angle `angle` (the wheels keep their offsets from the
    hull's centre and their angles relative to the hull: no kernel under test reads a wheel's position); hull velocity (vx, vy) if given"""
    b = np.array(base, np.float32, copy=True)
    a32 = np.float32(angle)
    cx, cy = centre_for(L, px, py, a32)
    with np.errstate(all="ignore"):
        b[1:, 0] += cx - b[0, 0]; b[1:, 1] += cy - b[0, 1]; b[1:, 2] += a32 - b[0, 2]
    b[0, 0], b[0, 1], b[0, 2] = cx, cy, a32
    if vx is not None:
        b[0, 3], b[0, 4] = np.float32(vx), np.float32(vy)
    return b


def _scatter(rng, rows, N):
    """each car within +-8 of a random tile, random heading (beyond +-pi too) and velocity"""
    i = rng.randint(0, len(rows), N)
    return [(rows[i[a], 2] + rng.uniform(-8, 8), rows[i[a], 3] + rng.uniform(-8, 8), rng.uniform(-7, 7), rng.normal(0, 10), rng.normal(0, 10)) for a in range(N)]


def _centroid(rows):
    return float(rows[:, 2].mean()), float(rows[:, 3].mean())


# lattice poses at angle 0 and what ties there, in lattice_loop's indices: (x, y, tied tiles)
LATTICE_TIES = [
    (4.0, 36.0, (9, 73)),                # one lane: i and i + 64
    (4.0, 38.0, (9, 10, 72, 73)),        # four tiles, two of them one lane's
    (4.0, 34.0, (8, 9, 73, 74)),
    (8.0, 38.0, (9, 10)),                # neighbours: two lanes
    (4.0, 20.0, (5, 77)),                # across the loop: two lanes (5 and 13), the lowest index in the lower lane ...
    (4.0, 120.0, (30, 52)),
    (0.0, 50.0, (69, 70)),
    (4.0, 40.0, (10, 72)),               # ... and in the higher one (lanes 10 and 8)
]
OFFSETS = [(0.0, 0.0), (1e-6, 0.0), (0.0, -1e-6), (3e-5, 2e-5), (-1e-3, 1e-3), (0.5, 0.0), (0.0, 0.0), (-2e-7, 0.0)]


def pose_sets(L, tracks, N, base):
    """{name: bodies [B, N, 5, 6] f32} — base: get_state()["bodies"] of the rig"""
    B = len(tracks)
    sets = {}

    def build(fn, seed):
        out = np.zeros((B, N, 5, 6), np.float32)
        for e, (name, rows, cw) in enumerate(tracks):
            rng = np.random.RandomState(seed * 1000 + e)
            poses = fn(e, name, rows, cw, rng)
            if poses is None:
                poses = _scatter(rng, rows, N)
            for a, (px, py, ang, vx, vy) in enumerate(poses):
                out[e, a] = place(L, base[e, a], px, py, ang, vx, vy)
        return out

    sets["scatter"] = build(lambda e, name, rows, cw, rng: None, 1)
    sets["scatter2"] = build(lambda e, name, rows, cw, rng: None, 2)

    def centre(e, name, rows, cw, rng):
        cx, cy = _centroid(rows) if not name.startswith("circle") else (0.0, 0.0)
        return [(cx + OFFSETS[a][0], cy + OFFSETS[a][1], rng.uniform(-3, 3), rng.normal(0, 5), rng.normal(0, 5)) for a in range(N)]
    sets["centre"] = build(centre, 3)

    def ties(e, name, rows, cw, rng):
        if name not in ("lattice", "border"):
            return None
        x0 = float(W) if name == "border" else 0.0       # (on the shifted loop the distances are no longer exact: the poses are just close calls)
        return [(LATTICE_TIES[(a + e) % len(LATTICE_TIES)][0] + x0, LATTICE_TIES[(a + e) % len(LATTICE_TIES)][1], 0.0, rng.normal(0, 5), rng.normal(0, 5)) for a in range(N)]
    sets["ties"] = build(ties, 4)

    def border(e, name, rows, cw, rng):
        """on the border x = 0 of border_loop (t = 0; with the ray straight ahead also den == 0), beside a vertex of it, and 5 to its left at
        a vertex's height (the rays (0, +-1) of a direction table then pass through that vertex)"""
        if name == "lattice":                            # den == 0 against every vertical segment; no pose on a border here
            return [(4.0 + 0.25 * a, 30.0 + 6.0 * a, 0.0, 1.0, 2.0) for a in range(N)]
        if name != "border":
            return None
        spots = [(0.0, 42.0), (-5.0, 48.0), (0.0, 60.0), (-5.0, 100.0), (0.0, 33.5), (5.0, 64.0), (-5.0, 12.0), (0.0, 150.0)]
        return [(spots[(a + e) % 8][0], spots[(a + e) % 8][1], 0.0, rng.normal(0, 5), rng.normal(0, 5)) for a in range(N)]
    sets["border"] = build(border, 5)

    def far(e, name, rows, cw, rng):
        cx, cy = _centroid(rows)
        spots = [(5e3, 0.0), (0.0, -1e5), (-5e3, 5e3), (1e5, 1e5), (0.0, 5e3), (-1e5, 3.0), (5e3, -5e3), (7.0, 1e5)]
        return [(cx + spots[(a + e) % 8][0], cy + spots[(a + e) % 8][1], rng.uniform(-3, 3), rng.normal(0, 5), rng.normal(0, 5)) for a in range(N)]
    sets["far"] = build(far, 6)

    def nonfinite(e, name, rows, cw, rng):
        poses = _scatter(rng, rows, N)
        a_nan = e % N
        poses[a_nan] = (float("nan"), poses[a_nan][1], poses[a_nan][2], 1.0, 2.0)
        if N > 1:
            a_inf = (e + 1) % N
            poses[a_inf] = (poses[a_inf][0], float("inf") if e % 2 else float("-inf"), poses[a_inf][2], 1.0, 2.0)
        return poses
    sets["nonfinite"] = build(nonfinite, 7)

    def close(e, name, rows, cw, rng):
        """even envs: a ring of radius 6 round a track point, every car looking at the ring's centre past its neighbours; odd envs: a line
        astern, 5.5 apart, all looking down the line"""
        i = rng.randint(0, len(rows)); x0, y0 = rows[i, 2], rows[i, 3]
        if e % 2 == 0:
            out = []
            for a in range(N):
                ph = 2 * math.pi * a / max(N, 1)
                # forward axis (-sin ang, cos ang) = towards the centre: ang = ph + pi / 2
                out.append((x0 + 6 * math.cos(ph), y0 + 6 * math.sin(ph), ph + math.pi / 2 + 0.1 * a, rng.normal(0, 5), rng.normal(0, 5)))
            return out
        ang = rng.uniform(-3, 3)
        return [(x0 - math.sin(ang) * 5.5 * a, y0 + math.cos(ang) * 5.5 * a, ang + (math.pi if a % 3 == 2 else 0.0), rng.normal(0, 5), rng.normal(0, 5)) for a in range(N)]
    sets["close"] = build(close, 8)

    def graze(e, name, rows, cw, rng):
        """all at angle 0 round car 0 at (20, 0): rays (0, +-1) of a direction table, i.e. u = (+-1, 0), that end on a CORNER of car 0's front
        polygon (+-1.2, 2.2) .. (+-1.2, 2.6) — q is exactly 1 (or 0) on the polygon's side edge and the edge round the corner is collinear
        (den == 0), so the side edge alone holds the hit"""
        lo, hi, half = float(np.float32(110 * 0.02)), float(np.float32(130 * 0.02)), float(np.float32(60 * 0.02))
        spots = [(20.0, 0.0), (10.0, lo), (10.0, hi), (30.0, lo), (30.0, hi), (20.0 - half, -8.0), (20.0 + half, 9.0), (12.0, 1.0)]
        return [(spots[a][0], spots[a][1], 0.0, rng.normal(0, 5), rng.normal(0, 5)) for a in range(N)]
    sets["graze"] = build(graze, 10)

    def start(e, name, rows, cw, rng):
        """near tile 0: a look-ahead of 64 wraps in either direction"""
        T = len(rows)
        idx = [[0, 1, T - 1, 2, T - 2, 0, 3, T - 3][(a + e // 2) % 8] for a in range(N)]      # (e // 2: both directions of a track get the same tiles)
        return [(rows[i, 2] + rng.uniform(-1, 1), rows[i, 3] + rng.uniform(-1, 1), rows[i, 1] - (math.pi if cw else 0.0) + rng.uniform(-0.3, 0.3),
                 rng.normal(0, 10), rng.normal(0, 10)) for i in idx]
    sets["start"] = build(start, 9)
    return sets


# ------------------------------------------------------------------------------------------------------------------------------ restatements
def state_ref(L, tracks, st, tvc, K, stride):
    """[B, N, F] f32 of state_obs_ref.features on get_state() arrays `st`, hull_positions and the track rows"""
    pos = hull_positions(L, st["bodies"])
    with np.errstate(all="ignore"):
        return np.stack([state_obs_ref.features(L, st["bodies"][e], st["wheels"][e], st["on_road"][e], tvc[e], pos[e], rows, cw, K, stride)
                         for e, (_, rows, cw) in enumerate(tracks)])


def range_ref(L, tracks, bodies, dirs, max_range):
    pos = hull_positions(L, bodies)
    with np.errstate(all="ignore"):
        return np.stack([range_obs_ref.ranges(L, bodies[e], pos[e], rows, dirs, max_range) for e, (_, rows, _) in enumerate(tracks)])


def driver_ref_actions(L, tracks, bodies, params):
    pos = hull_positions(L, bodies)
    with np.errstate(all="ignore"):
        return np.stack([driver_ref.actions(L, bodies[e], pos[e], driver_ref.track_arrays(rows), cw, np.asarray(params, np.float32))
                         for e, (_, rows, cw) in enumerate(tracks)])


def tied_tiles(rows, px, py):
    """(indices of the tiles at the minimal f64 distance dx dx + dy dy from (px, py), the restatement's choice)"""
    tx = np.ascontiguousarray(rows[:, 2], f64); ty = np.ascontiguousarray(rows[:, 3], f64)
    dx = f64(px) - tx; dy = f64(py) - ty
    dd = dx * dx + dy * dy
    return np.nonzero(dd == dd.min())[0], state_obs_ref.nearest_tile(tx, ty, f64(px), f64(py))


def ray_table(L, body, pos, rows, dirs):
    """every ray of one car against the 2 T border segments, the recipe's values: (t, q, den, hit) [R, 2 T] f64 / bool — segment s < T is tile
    s's left one, s >= T tile s - T's right one"""
    s32, c32 = state_obs_ref.sincos_host(L, body[0, 2])
    s, c = f64(s32), f64(c32)
    fx, fy, rx, ry = -s, c, c, s
    ax, ay, bx, by = range_obs_ref.border_segments(rows)
    ex, ey = bx - ax, by - ay
    wx, wy = ax - f64(pos[0]), ay - f64(pos[1])
    out = []
    with np.errstate(all="ignore"):
        for k in range(len(dirs)):
            ck, sk = f64(np.float32(dirs[k][0])), f64(np.float32(dirs[k][1]))
            ux, uy = ck * fx + sk * rx, ck * fy + sk * ry
            den = ux * ey - uy * ex
            t = (wx * ey - wy * ex) / den
            q = (wx * uy - wy * ux) / den
            out.append((t, q, den, (den != 0) & (t >= 0) & (q >= 0) & (q <= 1)))
    return tuple(np.stack([o[i] for o in out]) for i in range(4))


def hull_ray_table(L, bodies, pos, a, j, direction):
    """one ray of car a against the edges of car j's hull: (t, q, den, hit) [20] f64 / bool, the recipe's values"""
    sa, ca = (f64(v) for v in state_obs_ref.sincos_host(L, bodies[a, 0, 2]))
    sj, cj = (f64(v) for v in state_obs_ref.sincos_host(L, bodies[j, 0, 2]))
    p = pos.astype(f64)
    ax, ay, bx, by = range_obs_ref.hull_segments(p[j, 0], p[j, 1], sj, cj)
    fx, fy, rx, ry = -sa, ca, ca, sa
    ck, sk = f64(np.float32(direction[0])), f64(np.float32(direction[1]))
    ux, uy = ck * fx + sk * rx, ck * fy + sk * ry
    ex, ey = bx - ax, by - ay
    wx, wy = ax - p[a, 0], ay - p[a, 1]
    with np.errstate(all="ignore"):
        den = ux * ey - uy * ex
        t = (wx * ey - wy * ex) / den
        q = (wx * uy - wy * ux) / den
    return t, q, den, (den != 0) & (t >= 0) & (q >= 0) & (q <= 1)


def nearest_car(L, bodies, pos, a, dirs, max_range):
    """per ray of car a: the car whose hull holds the nearest hit within max_range, or -1 — from range_obs_ref's pieces"""
    N = bodies.shape[0]
    sc = [state_obs_ref.sincos_host(L, bodies[j, 0, 2]) for j in range(N)]
    p = pos.astype(f64)
    s, c = f64(sc[a][0]), f64(sc[a][1])
    fx, fy, rx, ry = -s, c, c, s
    out = np.full(len(dirs), -1)
    for k in range(len(dirs)):
        ck, sk = f64(np.float32(dirs[k][0])), f64(np.float32(dirs[k][1]))
        ux, uy = ck * fx + sk * rx, ck * fy + sk * ry
        best = f64(np.float32(max_range))
        for j in range(N):
            if j == a:
                continue
            t = range_obs_ref.ray_segments(p[a, 0], p[a, 1], ux, uy, *range_obs_ref.hull_segments(p[j, 0], p[j, 1], f64(sc[j][0]), f64(sc[j][1])), max_range)
            if t < best:
                best, out[k] = t, j
    return out


# ------------------------------------------------------------------------------------------------------------------------------ the handle
WARMUP_STEPS = 20
SPREAD_ODD = 14.0


def spread_bodies(tracks, N, bodies):
    """the spawn poses [B, N, 5, 6] re-placed so that the warm-up steps leave the cars of an env with different on-road bits: an even car c
    stands on the centre line at track point (10 + 3 c) mod T, away from the seam, looking down the track; an odd car is moved rigidly
    SPREAD_ODD — twice the road's half-width — away from its track's centroid, off the road"""
    st = np.array(bodies, np.float32, copy=True)
    for e, (_, rows, cw) in enumerate(tracks):
        cx, cy = _centroid(rows)
        for c in range(N):
            if c % 2 == 0:
                i = (10 + 3 * c) % len(rows)
                st[e, c] = rigid_teleport(st[e, c], rows[i, 2], rows[i, 3], rows[i, 1] - (math.pi if cw else 0.0))
                continue
            d = np.array([st[e, c, 0, 0] - cx, st[e, c, 0, 1] - cy], np.float64)
            d *= SPREAD_ODD / max(np.hypot(*d), 1e-9)
            st[e, c, :, 0] += np.float32(d[0]); st[e, c, :, 1] += np.float32(d[1])
    return st


def warmup_actions(B, N):
    """per-car distinct gas and steering (|steer| < 0.4: below the steering joint's limit)"""
    a = np.zeros((B, N, 3), np.float32)
    for c in range(N):
        a[:, c, 0] = (-1) ** c * (0.05 + 0.04 * c); a[:, c, 1] = 0.15 + 0.1 * c
    return a


def oracle_warmup(O, rows, cw, N, steps=WARMUP_STEPS):
    """The host twin of a Rig(spread=True, steps=...) env on track `rows`: an oracle env on the same tiles and spawn poses (car order 0 .. N-1,
    as levels.from_tracks), spread and stepped alike.  Returns its state() — bit for bit what the rig's get_state() row holds."""
    T = len(rows)
    c, s = np.array([math.cos(b) for b in rows[:, 1]]), np.array([math.sin(b) for b in rows[:, 1]])
    x, y = rows[:, 2], rows[:, 3]
    j = (np.arange(T) - 1) % T
    poly = np.stack([np.stack([x - W * c, y - W * s], 1), np.stack([x + W * c, y + W * s], 1),
                     np.stack([x[j] + W * c[j], y[j] + W * s[j]], 1), np.stack([x[j] - W * c[j], y[j] - W * s[j]], 1)], 1)
    ep = dict(track=rows, poly=poly, color=np.full((T, 3), 0.4), tile_of_quad=np.arange(T, dtype=np.int32), direction="CW" if cw else "CCW",
              car_order=list(range(N)), poses=O.spawn_poses(rows, list(range(N)), cw))
    o = O.OracleEnv(N)
    try:
        o.reset(ep, render=False)
        b = spread_bodies([(None, rows, cw)], N, o.state()["bodies"][None])[0]
        for car in range(N):
            for k in range(5):
                o.set_body(car, k, b[car, k])
        a = warmup_actions(1, N)[0]
        for _ in range(steps):
            o.step(a, render=False)
        return o.state()
    finally:
        o.close()


GUARD = 64                     # float32 words in front of and behind a tensor under test
SENTINEL = np.float32(-7.25e11)


class Rig:
    """One handle on `tracks` (env e plays track e) with the observation under test on — observe: "state", "range", "driver", "pixels" (obs=True:
    the raster is under test, tests/test_gpu_view_kernel.py; env_kw: further settings of the handle, e.g. obs_format) or None (no
    derived observation: the step's own bookkeeping is under test, tests/test_gpu_flags_kernel.py); the tests
    point it at buffers of their own through the C ABI.  The buffer of the last launch stays referenced here (`held`), and the driver's
    registered action buffer (`scratch`) lives as long as the rig: the handle never holds a pointer to freed memory."""

    def __init__(self, lib, tracks, N, observe, steps=0, env_offset=0, every=None, spread=False, **env_kw):
        import torch
        from multi_car_racing_amd import levels
        from tests.util import make_env
        self.lib, self.L, self.torch, self.N = lib, lib.load(), torch, N
        every = tracks if every is None else every               # the pool: env e of a handle with env_offset o plays every[(o + e) % K]
        self.B = len(tracks)
        self.held = self.scratch = None
        on = {"state": dict(state_obs=True), "range": dict(range_obs=True), "driver": dict(driver_params={}), "pixels": env_kw, None: {}}[observe]
        self.tracks = tracks
        blobs = np.concatenate([levels.from_tracks([rows], N, "CW" if cw else "CCW") for _, rows, cw in every])
        self.env = make_env(self.B, N, 0, levels=blobs, level_order="cycle", obs=observe == "pixels", streams=1, env_offset=env_offset, **on)
        self.env.reset()
        if spread:
            self.env.set_bodies(spread_bodies(tracks, N, self.env.get_state()["bodies"]))
        if steps:
            act = torch.from_numpy(warmup_actions(self.B, N)).to(self.env.device)
            for _ in range(steps):
                self.env.step(act)
            torch.cuda.synchronize()
        self.base = self.env.get_state()
        self.tvc = self.env.get_env_state()["tile_visited_count"]

    def close(self):
        self.env.close()

    def guarded(self, n):
        """(whole tensor with GUARD sentinel words on either side of n float32 words, the view of the n words)"""
        whole = self.torch.full((n + 2 * GUARD,), float(SENTINEL), dtype=self.torch.float32, device=self.env.device)
        self.held = whole
        return whole, whole[GUARD:GUARD + n]

    @staticmethod
    def guards_intact(whole):
        h = whole.cpu().numpy()
        return bool((h[:GUARD] == SENTINEL).all() and (h[-GUARD:] == SENTINEL).all())

    def set_bodies(self, bodies):
        """teleport; returns get_state() (what the restatements read)"""
        self.env.set_bodies(bodies)
        st = self.env.get_state()
        assert np.array_equal(st["bodies"].view(np.uint32), np.ascontiguousarray(bodies, np.float32).view(np.uint32))
        return st
