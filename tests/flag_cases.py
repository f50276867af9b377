"""Synthetic tracks and poses for the backward / on-grass scans (a helper, not a test): csrc/k_flags.h driven through mcr_flags_now on inputs
no rollout reaches — tests/test_gpu_flags_kernel.py — and the conditions those inputs must hold, which tests/test_flag_cases.py checks on
the host from tests/flags_ref.py alone.

Tracks: tests/obs_cases.py's (circles of 20 .. 512 tiles, the lattice and border loops, a truncated lap) plus
  wiggle     T = 512, four-fold symmetric, right- and left-hand bends whose kerbs bring road_poly to MCR_QUAD_CAP = 768 entries exactly:
             all 48 blocks in use; the loop starts in a right-hand bend, so tile 0 carries a kerb (its previous tile is T - 1)
  scs        a stadium, straight - curve - straight: kerb runs that start and end inside a block; two kerb edges are moved onto float32
             coordinates (snap_edge), so that a float32 pose can stand exactly on a kerb's edge with its tile and on its outer edge
  spur       T = 44, P = 49: block 3 holds ONE entry, the kerb of tile 43, whose tile ended block 2.  A pose in that kerb is 5 from the tip of a
             straight (tile 31, the last entry of block 1) and 7.4 from tiles 42 / 43: the box of the kerb-only block is no bound for a track point
  lap        one generated lap, whole
  seam       T = 256, four-fold symmetric, turned so that a right-hand bend lies across the seam.  The kerb flags are spread IN PLACE over
             wrapped indices (:305-307): tile 0, part of four turns, flags tiles T - 3 .. T - 1 early, and T - 3, read again later in the
             same loop, hands the flag on to T - 6 .. T - 4 — straight tiles.  Their kerbs have side = sign(0) = 0: all four vertices lie on
             the centre line, nothing is inside them, and the ground where a kerb of side +1 or -1 would lie is grass
  columns    T = 80, no kerbs, every block's box within reach of the pose (1, 28): tiles 8 at (0, 28) and 72 at (2, 28) tie exactly, 64 apart —
             entry 8 of blocks 0 and 4, the same lane in the first and the second trip of the block loop
each in both directions.

Pose sets: `cases(...)` gives every track a list of cases (px, py, angle, vx, vy, tag) per set; `assign` deals them to the cars of a batch,
the N cars of an env taking consecutive cases, rotated per env and per round, so that `rounds(...)` rounds run every case of every track."""
import math

import numpy as np

from tests import flags_ref as R
from tests import obs_cases as C
from tests.util import hull_positions

f32, f64 = np.float32, np.float64
W, KW = R.TRACK_WIDTH, R.TRACK_WIDTH + R.BORDER
QBLK, QUAD_CAP = 16, 768
SETS = ("scatter", "ties", "edges", "kerb_only", "culling", "far", "heading_slow", "heading_fast", "heading_speed", "heading_wrap")
SPUR_TIP = 31
FAR = (1e3, 1e6, 1e15, 3e17, 1e18, 3e18, 1e19, 1e20, float(np.finfo(f32).max))


# ------------------------------------------------------------------------------------------------------------------------------ tracks
def walk(dbeta, step=3.5):
    """rows of a walk: beta[i] = sum of dbeta[..i], point i = point i - 1 + step (-sin beta[i], cos beta[i]); centred on its centroid"""
    beta = np.cumsum(np.asarray(dbeta, f64))
    x = np.cumsum(-step * np.sin(beta)); y = np.cumsum(step * np.cos(beta))
    T = len(beta)
    return np.ascontiguousarray(np.stack([np.arange(T) * (2 * math.pi / T), beta, x - x.mean(), y - y.mean()], axis=1), f64)


def wiggle():
    """per quarter: 24 tiles to the right, 32 straight, 40 to the left by 0.1 each, 32 straight — a quarter turn in all, 64 kerbs"""
    right = (40 * 0.1 - math.pi / 2) / 24
    return walk(([-right] * 24 + [0.0] * 32 + [0.1] * 40 + [0.0] * 32) * 4)


def snap_edge(rows, t, w, X, Y):
    """move tiles t and t - 1 along x so that x + w cos(beta) == X exactly for both: the edge between their vertices at signed offset w is
    the vertical line x == X, and tile t along y so that its vertex is (X, Y) exactly.  False (nothing moved) where no such coordinates exist."""
    def solve(target, prod):
        """v with v + prod == target exactly: target - prod or one of its neighbours"""
        v = [target - prod]
        for _ in range(4):
            v = [np.nextafter(v[0], -np.inf)] + v + [np.nextafter(v[-1], np.inf)]
        return next((float(c) for c in v if c + prod == target), None)
    xs = [solve(X, w * math.cos(rows[k, 1])) for k in (t, t - 1)]
    y = solve(Y, w * math.sin(rows[t, 1]))
    if None in xs or y is None:          # (the sums' grid is finer than the coordinate's: not every target can be met)
        return False
    rows[t, 2], rows[t - 1, 2], rows[t, 3] = xs[0], xs[1], y
    return True


SCS_INNER, SCS_OUTER = 13, 19          # the tiles whose kerb edges are snapped (both in the first curve, both kerbed, as their predecessors)


def scs():
    rows = walk([0.0] * 10 + [math.pi / 32] * 32 + [0.0] * 20 + [math.pi / 32] * 32 + [0.0] * 10)
    # the tiles to be moved get coordinates below 0, their vertices (further left and down) larger ones in magnitude: a vertex's grid of
    # float64 values is then no finer than the coordinate's, and every target can be met
    rows[:, 2] -= rows[SCS_INNER - 1, 2] + 1.0; rows[:, 3] -= rows[SCS_OUTER, 3] + 1.0
    for t, w in ((SCS_INNER, -W), (SCS_OUTER, -KW)):     # a left-hand curve: side = sign(beta[t - 1] - beta[t]) = -1
        vx = rows[t, 2] + w * math.cos(rows[t, 1]); vy = rows[t, 3] + w * math.sin(rows[t, 1])
        assert snap_edge(rows, t, w, round(vx * 8) / 8, round(vy * 8) / 8)
    return rows


def scs_edges(rows):
    """[(X, y0, y1)] of the two snapped edges: x == X from tile t - 1's vertex (y0) to tile t's (y1, a float32 value)"""
    out = []
    for t, w in ((SCS_INNER, -W), (SCS_OUTER, -KW)):
        X = rows[t, 2] + w * math.cos(rows[t, 1])
        out.append((X, rows[t - 1, 3] + w * math.sin(rows[t - 1, 1]), rows[t, 3] + w * math.sin(rows[t, 1])))
    return out


def spur():
    y0 = 3.5 * SPUR_TIP
    pts = [(0.0, 3.5 * i, 0.0) for i in range(SPUR_TIP + 1)]
    pts += [(-3.5 * (k + 1), y0 - 8.0, -1.5 * math.pi) for k in range(6)]
    pts += [(7.4, y0 + 5.0 - 1.75 + 3.5 * (5 - j), -math.pi + 0.1 * (5 - j)) for j in range(6)]      # (beta below 0: the seam's turn 0 - beta[43] opposes the bend's)
    a = np.array(pts, f64)
    return np.ascontiguousarray(np.stack([np.arange(len(a)) * (2 * math.pi / len(a)), a[:, 2], a[:, 0], a[:, 1]], axis=1), f64)


SPUR_POSE = (0.0, 3.5 * SPUR_TIP + 5.0)


SEAM_T = 256


def seam():
    """per quarter 8 tiles to the right, 16 straight, 24 to the left by 0.1 each, 16 straight; the list turned by 3, so that the last three
    tiles of the loop and the first five are one right-hand bend"""
    right = (24 * 0.1 - math.pi / 2) / 8
    d = ([-right] * 8 + [0.0] * 16 + [0.1] * 24 + [0.0] * 16) * 4
    return walk(d[3:] + d[:3])


COLUMNS_TIE = (1.0, 28.0, (8, 72))


def columns():
    """tiles 0 .. 15 at (0, 3.5 k), 16 .. 63 on the line x = -12, 64 .. 79 at (2, 3.5 (k - 64)) with beta = pi: the flag tells tile 8 from
    tile 72.  (3.5 apart, as a generated track's tiles: a grid of 8 cars on two overlapping columns stays within the tile event buffer.)"""
    pts = [(0.0, 3.5 * k, 0.0) for k in range(16)] + [(-12.0, 1.0 * (k - 16), 0.0) for k in range(16, 64)] + [(2.0, 3.5 * (k - 64), math.pi) for k in range(64, 80)]
    a = np.array(pts, f64)
    return np.ascontiguousarray(np.stack([np.arange(len(a)) * (2 * math.pi / len(a)), a[:, 2], a[:, 0], a[:, 1]], axis=1), f64)


def generated_lap(lib, seed=78):
    from multi_car_racing_amd import levels
    blobs, _ = levels.make_levels(1, 1, seed, direction_mode=0, threads=1)
    ep = lib.unpack_episode(np.ascontiguousarray(blobs[0]))
    return np.ascontiguousarray(np.stack([ep["alpha"], ep["track"][:, 2], ep["track"][:, 0], ep["track"][:, 1]], axis=1), f64)


def all_tracks(lib):
    """[(name, rows [T, 4], cw)]: obs_cases' tracks and the six above, every one in both directions"""
    more = [("wiggle", wiggle()), ("scs", scs()), ("spur", spur()), ("lap", generated_lap(lib)), ("seam", seam()), ("columns", columns())]
    return C.all_tracks(lib) + [(name, rows, cw) for name, rows in more for cw in (False, True)]


class Geo:
    """what the restatement makes of a track: road_poly, which entry is which, the float32 boxes of the blocks of QBLK entries"""

    def __init__(self, rows):
        self.polys, self.tile, self.owner = R.road_polys(rows)
        self.P = len(self.polys)
        self.entry_of_tile = np.nonzero(self.tile >= 0)[0]
        q = self.polys.astype(f32)
        nb = (self.P + QBLK - 1) // QBLK
        self.boxes = np.array([[q[b * QBLK:(b + 1) * QBLK, :, 0].min(), q[b * QBLK:(b + 1) * QBLK, :, 1].min(),
                                q[b * QBLK:(b + 1) * QBLK, :, 0].max(), q[b * QBLK:(b + 1) * QBLK, :, 1].max()] for b in range(nb)], f32)

    def blocks_holding(self, px, py):
        b = self.boxes
        return np.nonzero((b[:, 0] <= px) & (px <= b[:, 2]) & (b[:, 1] <= py) & (py <= b[:, 3]))[0]

    def block_of_tile(self, t):
        return int(self.entry_of_tile[t]) // QBLK


def scan_lanes(g, px, py):
    """where k_flags' block loop puts road_poly's entries for a car at (px, py) (float32): {entry: (trip, lane)} of the entries of the blocks
    it visits — the kernel's culling in its float32 arithmetic, four visited blocks per trip, 16 lanes per block"""
    one = f32(1.0); px, py = f32(px), f32(py)
    b = g.boxes
    full = (np.arange(len(b)) + 1) * QBLK <= g.P
    with np.errstate(all="ignore"):
        lx = np.maximum(np.maximum(b[:, 0] - px, px - b[:, 2]), f32(0)); ly = np.maximum(np.maximum(b[:, 1] - py, py - b[:, 3]), f32(0))
        hx = np.maximum(np.abs(px - b[:, 0]), np.abs(px - b[:, 2])); hy = np.maximum(np.abs(py - b[:, 1]), np.abs(py - b[:, 3]))
        lb2 = (lx * lx + ly * ly).astype(f32)
        ub2 = np.where(full, (hx * hx + hy * hy).astype(f32), np.finfo(f32).max).min()
        reach = f32(np.sqrt(ub2) * (one + f32(1e-5)) + f32(0.01)) if ub2 < f32(1e30) else f32(1e18)
        visit = np.nonzero(lb2 <= reach * reach)[0]
    out = {}
    for k, blk in enumerate(visit):
        for j in range(QBLK):
            if blk * QBLK + j < g.P:
                out[int(blk) * QBLK + j] = (k // 4, (k % 4) * QBLK + j)
    return out


_geo = {}


def geometry(tracks):
    """[Geo] per track (both directions of a track share one)"""
    out = []
    for name, rows, _ in tracks:
        if name not in _geo:
            _geo[name] = Geo(rows)
        out.append(_geo[name])
    return out


# ------------------------------------------------------------------------------------------------------------------------------ cases
def desired_angle(rows, cw, t):
    d = f64(rows[t, 1]) + (f64(np.pi) if cw else f64(0))
    return float((d + f64(2 * np.pi)) % f64(2 * np.pi))


def ulp_pair(rows, want_low_first):
    """a pose (ox, 0) beside the centre of a circle whose two smallest exact distances differ by one float64 ulp, the nearer tile having the
    lower index (want_low_first) or the higher one: (ox, nearest, runner-up) or None.  ox is a multiple of 2^-50: the hull's origin at
    angle 0 is its centre minus a local centre of 1.5e-9 in x, so it takes every multiple of 2^-53 that small."""
    for k in range(-3000, 3001):
        ox = k * 2.0 ** -50
        d = R.distances(rows, ox, 0.0)
        s = np.unique(d)
        if len(s) < 2 or s[1] != np.nextafter(s[0], np.inf) or (d == s[0]).sum() != 1:
            continue
        i0, i1 = int(np.argmin(d)), int(np.nonzero(d == s[1])[0][0])
        if (i0 < i1) == want_low_first:
            return ox, i0, i1
    return None


def _pick_tiles(rows, n, seed):
    T = len(rows)
    return [(seed * 7 + 3 + k * max(T // n, 1)) % T for k in range(n)]


def _ulps(v):
    v = f32(v)
    lo, hi = np.nextafter(v, f32(-np.inf)), np.nextafter(v, f32(np.inf))
    return float(lo), float(hi)


_cases = {}


def cases(set_name, e, tracks, geos):
    """_make_cases, made once per (set, track, direction)"""
    key = (set_name, e, tracks[e][0], tracks[e][2])
    if key not in _cases:
        _cases[key] = _make_cases(set_name, e, tracks, geos)
    return _cases[key]


def _make_cases(set_name, e, tracks, geos):
    """the cases of track e in pose set `set_name`: [(px, py, angle, vx, vy, tag)] — tag a string; "filler" marks a scatter pose that stands in
    where a track has no case of the kind"""
    name, rows, cw = tracks[e]
    g = geos[e]
    T = len(rows)
    rng = np.random.RandomState(1000 * (SETS.index(set_name) + 11) + e)
    cx, cy = (0.0, 0.0) if name.startswith("circle") else C._centroid(rows)

    def fill(out, n=4):
        return out + [p + ("filler",) for p in C._scatter(rng, rows, max(n - len(out), 0))]

    def v():
        return float(rng.normal(0, 10)), float(rng.normal(0, 10))

    if set_name == "scatter":
        return [p + ("random",) for p in C._scatter(rng, rows, 8)]

    if set_name == "ties":
        out = []
        if name in ("lattice", "border"):
            x0 = float(C.W) if name == "border" else 0.0
            for k, (x, y, tied) in enumerate(C.LATTICE_TIES):
                out.append((x + x0, y, 0.0) + v() + (f"tie {tied}" if name == "lattice" else "close call",))
                out.append((x + x0 + C.OFFSETS[k][0], y + C.OFFSETS[k][1], 0.0) + v() + ("close call",))
            return out
        if name == "columns":
            x, y, tied = COLUMNS_TIE
            return [(x, y, 0.0, 0.0, 0.0, f"tie {tied}"), (x, y, 0.0) + v() + (f"tie {tied}",)] + [(x + ox, y + oy, 0.0) + v() + ("close call",) for ox, oy in C.OFFSETS[1:]]
        out = [(cx + ox, cy + oy, 0.0) + v() + ("centre",) for ox, oy in C.OFFSETS]
        if name.startswith("circle"):
            for low in (True, False):
                hit = ulp_pair(rows, low)
                if hit is not None:
                    out.append((hit[0], 0.0, 0.0) + v() + (f"ulp {hit[1]} {hit[2]}",))
        return out

    if set_name == "edges":
        out = []

        def with_neighbours(x, y, axis, tag):
            lo, hi = _ulps(x if axis == 0 else y)
            out.append((x, y, 0.0) + v() + ("exact " + tag,))
            for nb in (lo, hi):
                out.append(((nb, y) if axis == 0 else (x, nb)) + (0.0,) + v() + ("beside " + tag,))
        if name == "border":
            with_neighbours(8.0, 42.0, 0, "border")          # the left border of the loop's right side is x == 8 exactly
            with_neighbours(8.0, 48.0, 0, "vertex")
            with_neighbours(float(C.W) + 1.0, 100.0, 1, "seam")
        elif name == "lattice":
            with_neighbours(9.0, 20.0, 1, "seam")
            with_neighbours(3.0, 64.0, 1, "seam")
        elif name == "scs":
            (xi, ya, yb), (xo, yc, yd) = scs_edges(rows)
            with_neighbours(xi, float(f32((ya + yb) / 2)), 0, "kerb-tile edge")
            with_neighbours(xi, yb, 0, "kerb-tile vertex")
            with_neighbours(xo, float(f32((yc + yd) / 2)), 0, "kerb outer edge")
            with_neighbours(xo, yd, 0, "kerb outer vertex")
        else:                            # close calls: float32 roundings of a vertex, a seam's midpoint and a border's midpoint
            for t in _pick_tiles(rows, 3, e):
                q = g.polys[g.entry_of_tile[t]]
                out.append((float(f32(q[0, 0])), float(f32(q[0, 1])), 0.0) + v() + ("close call",))
                out.append((float(f32((q[0, 0] + q[1, 0]) / 2)), float(f32((q[0, 1] + q[1, 1]) / 2)), 0.0) + v() + ("close call",))
                out.append((float(f32((q[1, 0] + q[2, 0]) / 2)), float(f32((q[1, 1] + q[2, 1]) / 2)), 0.0) + v() + ("close call",))
        return out

    if set_name == "kerb_only":
        kerbs = np.nonzero(g.tile < 0)[0]
        picks = []
        if len(kerbs):
            picks.append(int(kerbs[0]))                                             # the kerb of the lowest tile (wiggle: tile 0)
            picks += [int(q) for q in kerbs if q % QBLK == 0][:2]                   # first entry of a block: its tile ended the previous one
            picks += [int(q) for q in rng.choice(kerbs, min(6, len(kerbs)), replace=False)]
        out = []
        for q in picks:
            px, py = float(f32(g.polys[q, :, 0].mean())), float(f32(g.polys[q, :, 1].mean()))
            inside = R.within(g.polys, px, py)
            if inside[q] and not inside[g.tile >= 0].any():
                out.append((px, py, float(rng.uniform(-3, 3))) + v() + (f"kerb {q} of tile {g.owner[q]}" + (" block start" if q % QBLK == 0 else ""),))
        # a kerb of side 0 (the seam loop): where it would lie with side +1 and with side -1, beside the tile, and on the segment it is
        for q in [int(q) for q in kerbs if R.kerb_side(rows, int(g.owner[q])) == 0.0]:
            t = int(g.owner[q])
            mx, my = (rows[t, 2] + rows[t - 1, 2]) / 2, (rows[t, 3] + rows[t - 1, 3]) / 2
            c, sn = math.cos(rows[t, 1]), math.sin(rows[t, 1])
            for sd in (1.0, -1.0):
                out.append((mx + sd * (W + R.BORDER / 2) * c, my + sd * (W + R.BORDER / 2) * sn, float(rng.uniform(-3, 3))) + v() + (f"side0 beside {q} of tile {t}",))
            out.append((mx, my, float(rng.uniform(-3, 3))) + v() + (f"side0 on {q} of tile {t}",))
        return fill(out)

    if set_name == "culling":
        out = [(cx, cy, float(rng.uniform(-3, 3))) + v() + ("centroid",)]
        for r in (5.0, 50.0, 500.0, 2000.0):
            t = int(rng.randint(T))
            dx, dy = rows[t, 2] - cx, rows[t, 3] - cy
            n = math.hypot(dx, dy) or 1.0
            out.append((rows[t, 2] + dx / n * (KW + r), rows[t, 3] + dy / n * (KW + r), float(rng.uniform(-3, 3))) + v() + (f"outside {r:g}",))
        found = 0
        for _ in range(400):             # inside some block's box, the nearest track point in a block whose box does not hold the pose
            t = int(rng.randint(T))
            px, py = float(f32(rows[t, 2] + rng.uniform(-12, 12))), float(f32(rows[t, 3] + rng.uniform(-12, 12)))
            holding = g.blocks_holding(px, py)
            if len(holding) and g.block_of_tile(R.track_index(rows, px, py)) not in holding:
                out.append((px, py, 0.0) + v() + ("other block",)); found += 1
                if found == 2:
                    break
        if g.P % QBLK:                   # the nearest tile in the partial last block
            last = [t for t in range(T) if g.block_of_tile(t) == g.P // QBLK]
            if last:
                t = last[len(last) // 2]
                out.append((rows[t, 2] + 0.25, rows[t, 3] - 0.5, float(rng.uniform(-3, 3))) + v() + ("partial block",))
        if name == "spur":
            out.append(SPUR_POSE + (0.0, 0.0, 0.0, "spur"))
        return out

    if set_name == "far":
        out = []
        for k, m in enumerate(FAR):
            sx, sy = (1, -1)[k % 2], (1, -1)[(k // 2) % 2]
            for px, py in ((sx * m, cy), (cx, sy * m), (sx * m, -sy * m)):
                out.append((px, py, float(rng.uniform(-3, 3))) + v() + (f"far {m:g}",))
        t = int(rng.randint(T))
        x, y = rows[t, 2], rows[t, 3]
        for px, py, ang in ((math.inf, y, 0.3), (-math.inf, y, 0.3), (x, math.inf, 0.3), (x, -math.inf, 0.3), (math.nan, y, 0.3), (x, math.nan, 0.3),
                            (x, y, math.nan), (x, y, math.inf), (x, y, -math.inf)):
            out.append((px, py, ang, 0.1, 0.2, "nonfinite"))
        return out

    tiles = _pick_tiles(rows, 2, e)
    if set_name == "heading_slow":       # at rest on a track point: the hull's angle decides
        out = []
        for t in tiles:
            d = desired_angle(rows, cw, t)
            for base in (d + math.pi / 2, d - math.pi / 2):
                a = f32(base)
                for ang in (a, np.nextafter(a, f32(-np.inf)), np.nextafter(a, f32(np.inf))):
                    out.append((rows[t, 2], rows[t, 3], float(ang), 0.0, 0.0, "quarter turn"))
        t = tiles[0]
        for ang in (7.0, -7.0, 20.0, -20.0, float(f32(2 * math.pi)), -float(f32(2 * math.pi))):
            out.append((rows[t, 2], rows[t, 3], ang, 0.0, 0.0, "beyond a turn"))
        return out

    if set_name == "heading_fast":       # axis-aligned velocities: atan2 is exact on any libm
        return [(rows[t, 2], rows[t, 3], float(rng.uniform(-3, 3)), vx, vy, "axis") for t in tiles for vx, vy in ((1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (0.0, -1.0))]

    if set_name == "heading_speed":
        # (0.3, 0.4): the tile whose direction the velocity opposes most safely, the hull looking down the track — the branch decides the flag
        ca = (-math.atan2(0.3, 0.4) + 2 * math.pi) % (2 * math.pi)

        def margin(t):
            raw = abs(desired_angle(rows, cw, t) - ca)
            diff = abs(raw - 2 * math.pi) if raw > math.pi else raw
            return min(diff - math.pi / 2, math.pi - diff)
        t = max(range(T), key=margin)
        d = desired_angle(rows, cw, t)
        a, b = f32(0.3), f32(0.4)
        out = [(rows[t, 2], rows[t, 3], d, float(vx), float(vy), "0.3 0.4")
               for vx, vy in ((a, b), (np.nextafter(a, f32(0)), b), (np.nextafter(a, f32(1)), b), (a, np.nextafter(b, f32(0))), (a, np.nextafter(b, f32(1))))]
        # (0, 0.5) is exactly the threshold — not above it —, its neighbour is: the velocity points along hull angle 0
        t = tiles[0]
        for vy in (0.5, float(np.nextafter(f32(0.5), f32(1))), float(np.nextafter(f32(0.5), f32(0)))):
            out.append((rows[t, 2], rows[t, 3], desired_angle(rows, cw, t) + 2.5, 0.0, vy, "0 0.5"))
        return out

    if set_name == "heading_wrap":       # |desired - car_angle| > pi before the wrap, a small angle after it
        ds = [desired_angle(rows, cw, t) for t in range(T)]
        lo, hi = int(np.argmin(ds)), int(np.argmax(ds))
        out = []
        if ds[lo] < 1.0:
            out.append((rows[lo, 2], rows[lo, 3], -0.4, 0.0, 0.0, "wrap low"))
            out.append((rows[lo, 2], rows[lo, 3], float(rng.uniform(-3, 3)), 1.0, 0.0, "wrap low axis"))      # car_angle 3 pi / 2
        if ds[hi] > 2 * math.pi - 1.0:
            out.append((rows[hi, 2], rows[hi, 3], 0.4, 0.0, 0.0, "wrap high"))
            out.append((rows[hi, 2], rows[hi, 3], float(rng.uniform(-3, 3)), 0.0, 1.0, "wrap high axis"))     # car_angle 0
        return fill(out)
    raise KeyError(set_name)


def rounds(set_name, tracks, geos, N):
    """how many rounds of `assign` run every case of every track"""
    return max((len(cases(set_name, e, tracks, geos)) + N - 1) // N for e in range(len(tracks)))


def assign(L, tracks, geos, N, base, set_name, rnd):
    """(bodies [B, N, 5, 6] f32, tags [B][N]): car a of env e takes case (rnd N + a + e) mod the number of its track's cases"""
    B = len(tracks)
    out = np.zeros((B, N, 5, 6), f32)
    tags = []
    for e in range(B):
        cs = cases(set_name, e, tracks, geos)
        row = []
        for a in range(N):
            px, py, ang, vx, vy, tag = cs[(rnd * N + a + e) % len(cs)]
            out[e, a] = C.place(L, base[e, a], px, py, ang, vx, vy)
            row.append(f"{tag} ({px!r}, {py!r}) angle {ang!r} v ({vx!r}, {vy!r})")
        tags.append(row)
    return out, tags


def reference(L, tracks, geos, bodies):
    """(backward [B, N] u8, on_grass [B, N] u8, index [B, N]) of tests/flags_ref.py on get_state()'s bodies"""
    pos = hull_positions(L, bodies)
    B, N = bodies.shape[:2]
    bw = np.zeros((B, N), np.uint8); og = np.zeros((B, N), np.uint8); ix = np.zeros((B, N), np.int64)
    for e, (_, rows, cw) in enumerate(tracks):
        for a in range(N):
            bw[e, a], og[e, a], ix[e, a] = R.flags(rows, cw, pos[e, a], bodies[e, a, 0, 3:5], bodies[e, a, 0, 2], geos[e].polys)
    return bw, og, ix
