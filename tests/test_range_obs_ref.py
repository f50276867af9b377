"""CPU: the numpy restatement of the range-finder observation (tests/range_obs_ref.py) against an independent method on oracle episodes —
channel 0 against a MARCH along every ray that tests `point in any tile quad` (no segment intersection anywhere), channel 1 against the
opponent's bounding rectangle."""
import math

import numpy as np
import pytest

from tests import range_obs_ref as R
from tests.util import oracle_episode

H = 0.05                # march step
MAX_RANGE = 60.0
CASES = ((2, 11, "CCW"), (2, 12, "CW"))          # (N, seed, direction): two tracks
# share of the rays (all rays of all on-road cars of CASES, at spawn and after 100 driven steps) whose channel-0 value equals the march's exit
# distance within 2 H, measured on the restatement alone (test_channel0_against_the_march prints it): see that test's docstring
EQUAL_SHARE_MEASURED = 1.0
EQUAL_SHARE_MARGIN = 0.03


def tile_quads(track):
    """[T, 4, 2] f64: the road quad of tile i — L_i, R_i, R_j, L_j with j = i - 1 (multi_car_racing.py:300-307)"""
    tx, ty = track[:, 2], track[:, 3]
    C = np.cos(track[:, 1]); S = np.sin(track[:, 1]); W = R.TRACK_WIDTH
    L = np.stack([tx - W * C, ty - W * S], 1); Rt = np.stack([tx + W * C, ty + W * S], 1)
    return np.stack([L, Rt, np.roll(Rt, 1, axis=0), np.roll(L, 1, axis=0)], axis=1)


def in_any_quad(quads, pts):
    """pts [M, 2] -> [M] bool: inside (or on the edge of) any quad, whichever way it winds"""
    a = quads[None, :, :, :]; b = np.roll(quads, -1, axis=1)[None, :, :, :]
    p = pts[:, None, None, :]
    cr = (b[..., 0] - a[..., 0]) * (p[..., 1] - a[..., 1]) - (b[..., 1] - a[..., 1]) * (p[..., 0] - a[..., 0])     # [M, T, 4]
    return ((cr >= 0).all(-1) | (cr <= 0).all(-1)).any(-1)


def march(quads, px, py, ux, uy):
    """the first marched distance k H, k = 1, 2, .., at which p + k H u lies outside every tile quad; MAX_RANGE if there is none below it"""
    ks = np.arange(1, int(round(MAX_RANGE / H)) + 1) * H
    pts = np.stack([px + ks * ux, py + ks * uy], 1)
    out = ~in_any_quad(quads, pts)
    return float(ks[np.argmax(out)]) if out.any() else MAX_RANGE


def pursuit_actions(o, ep, gas=0.4, lookahead=3):
    """every car follows the centre line (tests/util.py LapRun.drive_actions' controller), so that the cars stay on the road"""
    tr = ep["track"]; T = len(tr); d = -1 if ep["direction"] == "CW" else 1
    b = o.state()["bodies"]
    a = np.zeros((o.N, 3), np.float32)
    for c in range(o.N):
        x, y, ang = float(b[c, 0, 0]), float(b[c, 0, 1]), float(b[c, 0, 2])
        i = int(np.argmin((tr[:, 2] - x) ** 2 + (tr[:, 3] - y) ** 2))
        t = (i + d * lookahead) % T
        want = np.arctan2(-(tr[t, 2] - x), tr[t, 3] - y)
        err = (want - ang + np.pi) % (2 * np.pi) - np.pi
        a[c, 0] = np.float32(np.clip(-2.0 * err, -1.0, 1.0)); a[c, 1] = gas
    return a


@pytest.fixture(scope="module")
def march_rows(lib, oracle):
    """per (case, moment, car, ray): (channel-0 value of the restatement, the march's exit distance), on-road cars only — computed once"""
    L = lib.load()
    _, dirs = R.default_dirs(19)
    rows, cars = [], 0
    for N, seed, direction in CASES:
        ep = oracle_episode(oracle, N, seed, 0, direction=direction)
        quads = tile_quads(ep["track"])
        o = oracle.OracleEnv(N)
        o.reset(ep, render=False)
        for moment in ("spawn", "driven"):
            if moment == "driven":
                for _ in range(100):
                    o.step(pursuit_actions(o, ep), render=False)
            got = R.of_oracle(L, o, ep, dirs, MAX_RANGE)
            assert got.shape == (N, 2, 19) and got.dtype == np.float32
            pos = o.positions().astype(np.float64); bodies = o.state()["bodies"]
            for a in range(N):
                px, py = pos[a]
                if not in_any_quad(quads, np.array([[px, py]]))[0]:
                    continue
                cars += 1
                ang = float(bodies[a, 0, 2])
                f = np.array([-math.sin(ang), math.cos(ang)]); r = np.array([math.cos(ang), math.sin(ang)])
                for k in range(19):
                    u = float(dirs[k, 0]) * f + float(dirs[k, 1]) * r
                    rows.append((N, seed, moment, a, k, float(got[a, 0, k]), march(quads, px, py, u[0], u[1])))
        o.close()
    assert cars >= 6, f"only {cars} of the 8 cars are on the road: the cases do not test what they should"
    return rows


def test_channel0_against_the_march(march_rows):
    """Leaving the union of the road quads crosses a border segment, so for EVERY ray of an on-road car the channel-0 range is at most the
    march's exit distance + H.  It can be SMALLER where the borders fold (k_rangeobs.h's documented limit): on the inside of a bend consecutive
    quads overlap, the inner polyline's segments run through their neighbours' quads, and a ray meets such a segment before it leaves the union.
    Measured on the restatement alone over all 152 rays (2 tracks x spawn / 100 driven steps x 2 cars x 19 rays, every car on the road):
    1.0000 of the rays (152 of 152) agree with the march within 2 H, and range - exit is at most 0.0000 — these cars stand on and drive through
    gentle bends; the share is asserted with a margin of 0.03 below the measured value (EQUAL_SHARE_MEASURED - EQUAL_SHARE_MARGIN).  No ray is skipped."""
    assert len(march_rows) >= 6 * 19
    worst = max(v - ex for *_, v, ex in march_rows)
    equal = sum(abs(v - ex) <= 2 * H for *_, v, ex in march_rows) / len(march_rows)
    print(f"{len(march_rows)} rays: range - exit at most {worst:.4f}; equal within 2 H: {equal:.4f}")
    for N, seed, moment, a, k, v, ex in march_rows:
        assert v <= ex + H, f"seed {seed} {moment} car {a} ray {k}: range {v} beyond the march's exit {ex}"
        assert 0.0 < v <= MAX_RANGE
    assert equal >= EQUAL_SHARE_MEASURED - EQUAL_SHARE_MARGIN, f"only {equal:.4f} of the rays agree with the march within 2 H"


def test_channel1_beside_an_opponent_at_spawn(lib, oracle):
    """Two cars side by side at spawn.  A ray that passes the opponent's hull rectangle x in [-1.2, 1.2], y in [-1.8, 2.6] (its body frame)
    by more than 0.1 on the outside reads max_range; a ray aimed at the opponent's origin reads less than the centre distance.  (The hull's
    fourth polygon reaches y = -2.4, behind that rectangle: a ray can touch it only from behind the opponent's rear axle, where no ray of a
    forward half-circle fan of a car standing BESIDE it points — the test asserts that premise instead of assuming it.)"""
    L = lib.load()
    _, dirs = R.default_dirs(19)
    hits = misses = 0
    for N, seed, direction in CASES:
        ep = oracle_episode(oracle, N, seed, 0, direction=direction)
        o = oracle.OracleEnv(N)
        o.reset(ep, render=False)
        pos = o.positions().astype(np.float64); bodies = o.state()["bodies"]
        got = R.of_oracle(L, o, ep, dirs, MAX_RANGE)
        for a in range(N):
            j = 1 - a
            ang_a, ang_j = float(bodies[a, 0, 2]), float(bodies[j, 0, 2])
            f = np.array([-math.sin(ang_a), math.cos(ang_a)]); r = np.array([math.cos(ang_a), math.sin(ang_a)])
            d = pos[j] - pos[a]; dist = float(np.hypot(*d))
            assert 2.4 < dist < 2 * R.TRACK_WIDTH and abs(float(d @ f)) < 2.0, "the cars do not stand side by side"
            # the ray in the opponent's body frame: x along its right-hand axis, y along its forward axis
            fj = np.array([-math.sin(ang_j), math.cos(ang_j)]); rj = np.array([math.cos(ang_j), math.sin(ang_j)])
            o_loc = np.array([-(d @ rj), -(d @ fj)])
            for k in range(19):
                u = float(dirs[k, 0]) * f + float(dirs[k, 1]) * r
                u_loc = np.array([u @ rj, u @ fj])
                clear = _ray_clears_box(o_loc, u_loc, (-1.2 - 0.1, 1.2 + 0.1), (-1.8 - 0.1, 2.6 + 0.1))
                clear_full = _ray_clears_box(o_loc, u_loc, (-1.2 - 0.1, 1.2 + 0.1), (-2.4 - 0.1, 2.6 + 0.1))
                assert clear == clear_full, "a ray of the fan reaches the rear polygon alone: the rectangle of this test does not bound the hull for it"
                if clear:
                    misses += 1
                    assert got[a, 1, k] == np.float32(MAX_RANGE), f"seed {seed} car {a} ray {k} passes the opponent but reads {got[a, 1, k]}"
                else:
                    hits += int(got[a, 1, k] < MAX_RANGE)
            # a ray aimed at the opponent's origin
            th = math.atan2(float(d @ r), float(d @ f))
            aim = np.array([[math.cos(th), math.sin(th)]], np.float32)
            v = R.of_oracle(L, o, ep, aim, MAX_RANGE)[a, 1, 0]
            assert 0.0 < v < dist and v > dist - 3.0, f"seed {seed} car {a}: aimed at the opponent's origin, range {v}, centre distance {dist}"
        o.close()
    assert hits >= 4 and misses >= 40, f"{hits} rays on the opponent, {misses} past it: the fan does not exercise both outcomes"


def _ray_clears_box(o, u, xr, yr):
    """does the ray o + t u, t >= 0, stay outside the box xr x yr? (slab test)"""
    t0, t1 = 0.0, math.inf
    for oc, uc, (lo, hi) in ((o[0], u[0], xr), (o[1], u[1], yr)):
        if abs(uc) < 1e-12:
            if not lo <= oc <= hi:
                return True
            continue
        ta, tb = (lo - oc) / uc, (hi - oc) / uc
        t0, t1 = max(t0, min(ta, tb)), min(t1, max(ta, tb))
    return t0 > t1


def test_one_car_sees_no_opponent_and_clamps(lib, oracle):
    """N = 1: channel 1 is max_range everywhere; a short max_range clamps channel 0 and never exceeds the long one's values"""
    L = lib.load()
    _, dirs = R.default_dirs(19)
    ep = oracle_episode(oracle, 1, 21, 0)
    o = oracle.OracleEnv(1)
    o.reset(ep, render=False)
    far, near = R.of_oracle(L, o, ep, dirs, 400.0), R.of_oracle(L, o, ep, dirs, 8.0)
    o.close()
    assert (far[0, 1] == np.float32(400.0)).all() and (near[0, 1] == np.float32(8.0)).all()
    assert np.array_equal(near[0, 0], np.minimum(far[0, 0], np.float32(8.0)))
    assert (far[0, 0] < 400.0).all(), "inside a closed track every ray meets a border"
    assert far[0, 0, 0] < R.TRACK_WIDTH * 2 and far[0, 0, 18] < R.TRACK_WIDTH * 2 and far[0, 0, 9] > far[0, 0, 0]      # sideways: the road's width; ahead: farther
