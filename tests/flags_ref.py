"""Host restatement of the backward / on-grass bookkeeping (a helper, not a test): what csrc/k_flags.h computes per car, as a direct reading of
the reference's track set-up (multi_car_racing.py:294-337: kerb flags, tiles, kerbs) and step bookkeeping (:446-495) in plain float64 —
every tile, every polygon, no culling, no bands, no prefilter.

Inputs are what the device holds: the track rows [T, 4] (alpha, beta, x, y) that went into levels.from_tracks, the episode's direction, the
hull's body origin (float32, tests/util.py: hull_positions), the hull's velocity and angle (float32, get_state()).  The polygons' vertices
use math.cos / math.sin of beta, as the host that packs an episode does.

tests/test_flag_cases.py ties this file to the C++ oracle's bookkeeping (which the goldens pin to the reference) on every finite case of
tests/flag_cases.py."""
import math

import numpy as np

f64 = np.float64
SCALE = 6.0
TRACK_WIDTH = 40 / SCALE
BORDER = 8 / SCALE
BORDER_MIN_COUNT = 4
TRACK_TURN_RATE = 0.31
BACKWARD_THRESHOLD = np.pi / 2


def border_flags(rows):
    """border[] of :294-307: a tile carries a kerb when it is one of BORDER_MIN_COUNT consecutive tiles that all turn the same way by more
    than TRACK_TURN_RATE * 0.2, or one of the BORDER_MIN_COUNT - 1 tiles in front of such a tile (negative indices wrap, as Python's do)"""
    T = len(rows)
    beta = [float(b) for b in rows[:, 1]]
    border = [False] * T
    for i in range(T):
        good = True
        oneside = 0
        for neg in range(BORDER_MIN_COUNT):
            beta1 = beta[(i - neg - 0) % T]
            beta2 = beta[(i - neg - 1) % T]
            good &= abs(beta1 - beta2) > TRACK_TURN_RATE * 0.2
            oneside += np.sign(beta1 - beta2)
        good &= abs(oneside) == BORDER_MIN_COUNT
        border[i] = bool(good)
    for i in range(T):
        for neg in range(BORDER_MIN_COUNT):
            border[(i - neg) % T] |= border[i]
    return border


def kerb_side(rows, i):
    """side of :329 for tile i: np.sign(beta2 - beta1), beta2 the previous tile's"""
    return float(np.sign(float(rows[i - 1, 1]) - float(rows[i, 1])))


def road_polys(rows):
    """road_poly of :310-334 in its order — a tile, then its kerb if it has one: (poly [P, 4, 2] f64, tile [P] i32: the tile an entry is, or
    -1 for a kerb, owner [P] i32: the tile an entry was made for)"""
    T = len(rows)
    border = border_flags(rows)
    polys, tile, owner = [], [], []
    for i in range(T):
        _, beta1, x1, y1 = (float(v) for v in rows[i])
        _, beta2, x2, y2 = (float(v) for v in rows[i - 1])
        road1_l = (x1 - TRACK_WIDTH * math.cos(beta1), y1 - TRACK_WIDTH * math.sin(beta1))
        road1_r = (x1 + TRACK_WIDTH * math.cos(beta1), y1 + TRACK_WIDTH * math.sin(beta1))
        road2_l = (x2 - TRACK_WIDTH * math.cos(beta2), y2 - TRACK_WIDTH * math.sin(beta2))
        road2_r = (x2 + TRACK_WIDTH * math.cos(beta2), y2 + TRACK_WIDTH * math.sin(beta2))
        polys.append([road1_l, road1_r, road2_r, road2_l]); tile.append(i); owner.append(i)
        if border[i]:
            side = float(np.sign(beta2 - beta1))
            b1_l = (x1 + side * TRACK_WIDTH * math.cos(beta1), y1 + side * TRACK_WIDTH * math.sin(beta1))
            b1_r = (x1 + side * (TRACK_WIDTH + BORDER) * math.cos(beta1), y1 + side * (TRACK_WIDTH + BORDER) * math.sin(beta1))
            b2_l = (x2 + side * TRACK_WIDTH * math.cos(beta2), y2 + side * TRACK_WIDTH * math.sin(beta2))
            b2_r = (x2 + side * (TRACK_WIDTH + BORDER) * math.cos(beta2), y2 + side * (TRACK_WIDTH + BORDER) * math.sin(beta2))
            polys.append([b1_l, b1_r, b2_r, b2_l]); tile.append(-1); owner.append(i)
    return np.array(polys, f64), np.array(tile, np.int32), np.array(owner, np.int32)


def crosses(poly, px, py):
    """[P, 4] f64: per polygon and edge i -> i + 1 the cross product (x2 - x1)(py - y1) - (y2 - y1)(px - x1), each product and difference
    rounded on its own"""
    a = poly; b = np.roll(poly, -1, axis=1)
    with np.errstate(all="ignore"):
        return (b[:, :, 0] - a[:, :, 0]) * (f64(py) - a[:, :, 1]) - (b[:, :, 1] - a[:, :, 1]) * (f64(px) - a[:, :, 0])


def within(poly, px, py):
    """[P] bool: the point lies strictly inside the polygon — every cross product > 0 or every one < 0 (shapely's Point.within of a convex
    quad: a point on the boundary is not within; NaN is in nothing)"""
    cr = crosses(poly, px, py)
    return (cr > 0).all(axis=1) | (cr < 0).all(axis=1)


def distances(rows, px, py):
    """np.linalg.norm(car_pos - track[:, 2:], ord=2, axis=1) as the oracle pins it: sqrt(dx dx + dy dy) in float64"""
    with np.errstate(all="ignore"):
        dx = f64(px) - np.ascontiguousarray(rows[:, 2], f64); dy = f64(py) - np.ascontiguousarray(rows[:, 3], f64)
        return np.sqrt(dx * dx + dy * dy)


def track_index(rows, px, py):
    """np.argmin: the first minimum; the first NaN if there is one (a row of NaN or of inf gives 0)"""
    return int(np.argmin(distances(rows, px, py)))


def car_angle(vx, vy, angle):
    """(:449-456) -> (car_angle in [0, 2 pi), speed)"""
    vx, vy = float(np.float32(vx)), float(np.float32(vy))
    speed = math.sqrt(vx * vx + vy * vy)
    with np.errstate(all="ignore"):
        a = f64(-math.atan2(vx, vy)) if speed > 0.5 else f64(np.float32(angle))
        return (a + f64(2 * np.pi)) % f64(2 * np.pi), speed


def heading(rows, cw, index, vx, vy, angle):
    """(:474-495) -> (backward, angle_diff after the wrap, angle_diff before it, speed)"""
    ca, speed = car_angle(vx, vy, angle)
    desired = f64(rows[index, 1])
    if cw:
        desired = desired + f64(np.pi)
    with np.errstate(all="ignore"):
        desired = (desired + f64(2 * np.pi)) % f64(2 * np.pi)
        raw = abs(desired - ca)
        diff = abs(raw - 2 * np.pi) if raw > np.pi else raw
    return bool(diff > BACKWARD_THRESHOLD), float(diff), float(raw), speed


def flags(rows, cw, pos, vel, angle, polys=None):
    """(driving_backward, driving_on_grass, track_index) of one car.  pos: the hull's body origin (float32 pair), vel: the hull's velocity,
    angle: the hull's angle; polys: road_polys(rows)[0] if the caller has it"""
    if polys is None:
        polys = road_polys(rows)[0]
    px, py = f64(np.float32(pos[0])), f64(np.float32(pos[1]))
    index = track_index(rows, px, py)
    on_grass = not bool(within(polys, px, py).any())
    backward = heading(rows, cw, index, vel[0], vel[1], angle)[0]
    return backward, on_grass, index
