"""CPU: the synthetic tracks and poses of tests/obs_cases.py hold the conditions the GPU kernel tests rest on — from the restatements alone,
no device: exact ties where ties are meant, a pose on a border, a ray through a shared vertex, den == 0, non-finite cars beside finite ones,
cars 4-7 being somebody's nearest hit, and each situation of the range finder's lanes occurring at least once."""
import numpy as np
import pytest

from multi_car_racing_amd import levels
from tests import obs_cases as C
from tests import range_obs_ref
from tests.util import hull_positions

AXES = np.array([(1, 0), (0, 1), (-1, 0), (0, -1)], np.float32)     # at hull angle 0 the rays (0, 1), (1, 0), (0, -1), (-1, 0)


@pytest.fixture(scope="module")
def tracks(lib):
    return C.all_tracks(lib)


def _sets(lib, tracks, N):
    return C.pose_sets(lib.load(), tracks, N, np.zeros((len(tracks), N, 5, 6), np.float32))


def _env(tracks, name, cw=False):
    return next(e for e, t in enumerate(tracks) if t[0] == name and t[2] == cw)


def test_tracks_are_what_they_say(lib, tracks):
    assert len(tracks) == 2 * (len(C.CIRCLE_T) + 3)
    assert [len(t[1]) for t in tracks if t[0].startswith("circle") and not t[2]] == list(C.CIRCLE_T)
    for name, rows, cw in tracks:
        blob = levels.from_tracks([rows], 8, "CW" if cw else "CCW")[0]
        ep = lib.unpack_episode(np.ascontiguousarray(blob))
        assert ep["T"] == len(rows) and ep["cw"] == cw and np.array_equal(ep["track"][:, :2], rows[:, 2:4]), name
    lat = tracks[_env(tracks, "lattice")][1]
    assert len(lat) == 84 and np.array_equal(lat[:, 2:4] % 4.0, np.zeros((84, 2))) and set(np.round(lat[:, 1] / (np.pi / 2)).tolist()) == {0.0, 1.0, 2.0, -1.0}
    tr = tracks[_env(tracks, "truncated")][1]
    assert len(tr) == C.TRUNCATED_T and np.hypot(*(tr[0, 2:4] - tr[-1, 2:4])) > 150.0, "the wrap segment is meant to be long"
    # border_loop: the right border of its left side is x = 0 exactly, its vertices (0, y) exactly
    brows = tracks[_env(tracks, "border")][1]
    ax, ay, bx, by = range_obs_ref.border_segments(brows)
    left = [i for i in range(84) if brows[i, 1] == np.pi and brows[i - 1, 1] == np.pi and brows[i, 3] >= 8]
    assert len(left) > 30
    for i in left:
        assert ax[84 + i] == 0.0 and bx[84 + i] == 0.0 and by[84 + i] == brows[i, 3] and ay[84 + i] == brows[i, 3] + 4.0


@pytest.mark.parametrize("N", [1, 5, 8])
def test_lattice_ties_are_exact_and_the_lowest_index_wins(lib, tracks, N):
    L = lib.load()
    sets = _sets(lib, tracks, N)
    seen = set()
    for cw in (False, True):
        e = _env(tracks, "lattice", cw)
        rows = tracks[e][1]
        pos = hull_positions(L, sets["ties"][e])
        for a in range(N):
            x, y, want = C.LATTICE_TIES[(a + e) % len(C.LATTICE_TIES)]
            assert sets["ties"][e, a, 0, 2] == 0.0 and pos[a].tolist() == [x, y], f"car {a}: hull_positions gives {pos[a].tolist()}, meant ({x}, {y})"
            tied, chosen = C.tied_tiles(rows, pos[a, 0], pos[a, 1])
            assert tuple(tied.tolist()) == want and chosen == min(want)
            seen.add(want)
    if N == 8:
        assert any(len(w) == 2 and w[1] - w[0] == 64 for w in seen), "a tie inside one lane (i, i + 64)"
        assert any(len(w) == 2 and (w[1] - w[0]) % 64 for w in seen), "a tie between two lanes"
        assert any(len(w) == 2 and w[0] % 64 > w[1] % 64 for w in seen) and any(len(w) == 2 and w[0] % 64 < w[1] % 64 for w in seen), \
            "the lowest index in the higher lane, and in the lower one"
        assert any(len(w) == 4 for w in seen)


def test_centre_of_a_circle_is_inside_the_f32_band(lib, tracks):
    """from the centre every tile's float32 distance lies within the search's band of the minimum, and the float32 minimum is not the float64 one"""
    L = lib.load()
    sets = _sets(lib, tracks, 8)
    differ = 0
    for e, (name, rows, cw) in enumerate(tracks):
        if not name.startswith("circle"):
            continue
        pos = hull_positions(L, sets["centre"][e])
        for a in (0, 1, 3):
            dx = pos[a, 0] - rows[:, 2].astype(np.float32); dy = pos[a, 1] - rows[:, 3].astype(np.float32)
            d32 = dx * dx + dy * dy
            band = np.float32(np.sqrt(d32.min()) * np.float32(1 + 1e-5) + np.float32(2e-3))
            assert (d32 <= band * band).all(), name
            differ += int(np.argmin(d32)) != C.tied_tiles(rows, pos[a, 0], pos[a, 1])[1]
    assert differ >= 10


def test_border_vertex_and_collinear_poses(lib, tracks):
    L = lib.load()
    sets = _sets(lib, tracks, 8)
    e = _env(tracks, "border")
    rows = tracks[e][1]; T = len(rows)
    bodies = sets["border"][e]; pos = hull_positions(L, bodies)
    spots = {tuple(pos[a].tolist()): a for a in range(8)}
    assert (0.0, 42.0) in spots and (-5.0, 48.0) in spots and (0.0, 60.0) in spots
    # on the border: the ray to the right meets the segment under the car at t = 0, 0 < q < 1; the ray straight ahead runs along it (den == 0)
    a = spots[(0.0, 42.0)]
    t, q, den, hit = C.ray_table(L, bodies[a], pos[a], rows, AXES)
    on = np.nonzero(hit[1] & (t[1] == 0.0))[0]
    assert len(on) == 1 and on[0] >= T and 0.0 < q[1, on[0]] < 1.0
    assert den[0, on[0]] == 0.0 and np.isnan(t[0, on[0]]) and not hit[0, on[0]]
    # 5 to the left of a vertex: q is exactly 1 on the segment that ends there and exactly 0 on the one that starts there
    a = spots[(-5.0, 48.0)]
    t, q, den, hit = C.ray_table(L, bodies[a], pos[a], rows, AXES)
    ends = np.nonzero(hit[1] & (q[1] == 1.0))[0]; starts = np.nonzero(hit[1] & (q[1] == 0.0))[0]
    assert len(ends) >= 1 and len(starts) >= 1
    en, stt = ends[np.argmin(t[1, ends])], starts[np.argmin(t[1, starts])]
    assert t[1, en] == 5.0 and t[1, stt] == 5.0 and t[1][hit[1]].min() == 5.0, "the nearest hit of the ray IS the vertex, on both segments"
    assert en >= T and stt == en + 1, "neighbouring segments of the right-hand polyline"
    # on the lattice loop a car at angle 0 meets den == 0 on every vertical segment
    e = _env(tracks, "lattice")
    bodies = sets["border"][e]; pos = hull_positions(L, bodies)
    _, _, den, _ = C.ray_table(L, bodies[0], pos[0], tracks[e][1], AXES)
    assert (den[0] == 0.0).sum() >= 2 * 70


def test_a_ray_ends_on_a_hull_corner_with_q_exactly_one(lib, tracks):
    """car 1's ray to the right ends on the lower left corner of car 0's front polygon: q == 1 exactly on the one edge that holds the hit,
    which is the ray's nearest; car 2's on the upper left corner: q == 0 exactly"""
    L = lib.load()
    for N in (2, 5):
        bodies = _sets(lib, tracks, N)["graze"][3]; pos = hull_positions(L, bodies)
        t, q, den, hit = C.hull_ray_table(L, bodies, pos, 1, 0, (0.0, 1.0))
        first = int(np.argmin(np.where(hit, t, np.inf)))
        assert hit[first] and q[first] == 1.0 and (den == 0.0).sum() >= 2 and (t[hit & (np.arange(20) != first)] > t[first] + 0.5).all()
        if N > 2:
            t, q, den, hit = C.hull_ray_table(L, bodies, pos, 2, 0, (0.0, 1.0))
            first = int(np.argmin(np.where(hit, t, np.inf)))
            assert hit[first] and q[first] == 0.0


def test_nonfinite_cars_stand_beside_finite_ones(lib, tracks):
    L = lib.load()
    for N in (1, 2, 8):
        pos = hull_positions(L, _sets(lib, tracks, N)["nonfinite"])
        for e in range(len(tracks)):
            assert np.isnan(pos[e]).any(axis=1).sum() == 1
            assert np.isinf(pos[e]).any(axis=1).sum() == (1 if N > 1 else 0)
            assert np.isfinite(pos[e]).all(axis=1).sum() == max(N - 2, 0)


def test_far_poses_are_beyond_every_range(lib, tracks):
    L = lib.load()
    bodies = _sets(lib, tracks, 2)["far"]
    _, dirs = range_obs_ref.default_dirs(5)
    want = C.range_ref(L, tracks[:6], bodies[:6], dirs, 2000.0)
    assert (want == np.float32(2000.0)).all()


@pytest.mark.parametrize("N", [5, 7, 8])
def test_close_cars_see_each_other_and_cars_4_to_7_are_nearest_hits(lib, tracks, N):
    """(N = 5 and 7: the last car is the only one of its hull-edge slot)"""
    L = lib.load()
    sets = _sets(lib, tracks, N)
    ang = np.linspace(-np.pi, np.pi, 32, endpoint=False)
    dirs = np.stack([np.cos(ang), np.sin(ang)], 1).astype(np.float32)
    for e in (0, 1, 4, 5):
        bodies = sets["close"][e]; pos = hull_positions(L, bodies)
        near = [C.nearest_car(L, bodies, pos, a, dirs, 25.0) for a in range(N)]
        hit_by_somebody = set(int(j) for n in near for j in n if j >= 0)
        assert set(range(4, N)) <= hit_by_somebody, f"env {e}: nearest hits {sorted(hit_by_somebody)}"
        if e % 2 == 0:            # the ring: every car sees several others
            assert all(len(set(n[n >= 0].tolist())) >= 3 for n in near), [sorted(set(n.tolist())) for n in near]


def range_situations(L, tracks, sets, N, dirs, max_range, names):
    """how often each situation of k_rangeobs' lanes occurs over the pose sets `names`: dict of counts"""
    out = dict(clamped=0, unclamped=0, wrap_nearest=0, two_in_a_lane=0, nearest_parked_first=0, nearest_parked_before_another_tile=0)
    mr = np.float64(np.float32(max_range))
    for name in names:
        pos = hull_positions(L, sets[name])
        for e, (tname, rows, cw) in enumerate(tracks):
            T = len(rows)
            for a in range(N):
                if not np.isfinite(pos[e, a]).all():
                    continue
                t, q, den, hit = C.ray_table(L, sets[name][e, a], pos[e, a], rows, dirs)
                for k in range(len(dirs)):
                    h = np.nonzero(hit[k] & (t[k] < mr))[0]
                    if len(h) == 0:
                        out["clamped"] += 1
                        continue
                    out["unclamped"] += 1
                    first = h[np.argmin(t[k, h])]
                    if tname == "truncated" and first % T == 0:
                        out["wrap_nearest"] += 1
                    # two or more hits on DISTINCT tiles of one lane (tiles i and i + 64 k) — a tile's own left and right segment do not count
                    lanes = np.bincount(np.unique(h % T) % 64)
                    if (lanes >= 2).any():
                        out["two_in_a_lane"] += 1
                    # the lane walks its tiles in ascending order, the left segment before the right one: the nearest hit is parked and
                    # another passing segment of the lane arrives behind it — any segment, and one of another tile
                    same = [s for s in h if s != first and (s % T) % 64 == (first % T) % 64]
                    if any(((s % T) // 64, s >= T) > ((first % T) // 64, first >= T) for s in same):
                        out["nearest_parked_first"] += 1
                    if any((s % T) // 64 > (first % T) // 64 for s in same):
                        out["nearest_parked_before_another_tile"] += 1
    return out


def test_each_range_situation_occurs(lib, tracks):
    L = lib.load()
    N = 2
    sets = _sets(lib, tracks, N)
    _, dirs = range_obs_ref.default_dirs(19)
    got = range_situations(L, tracks, sets, N, dirs, 400.0, ("scatter", "scatter2", "centre", "start"))
    assert all(v >= 3 for v in got.values()), got
    got = range_situations(L, tracks, sets, N, dirs, 0.5, ("scatter",))
    assert got["clamped"] >= 100 and got["unclamped"] >= 1, got


@pytest.mark.parametrize("N", [2, 5, 8])
def test_warmup_leaves_the_cars_of_an_env_different(lib, oracle, tracks, N):
    """the oracle twin of the state rig's warm-up (spread_bodies, WARMUP_STEPS steps of warmup_actions): in every env the cars differ in wheel
    speeds and steering angle, and their on-road bits are not all the same"""
    for name, rows, cw in tracks:
        st = C.oracle_warmup(oracle, rows, cw, N)
        assert np.isfinite(st["bodies"]).all() and (np.abs(st["wheels"][:, :, 4]).max(axis=1) > 0).all(), name
        steer = st["bodies"][:, 1, 2].astype(np.float64) - st["bodies"][:, 0, 2].astype(np.float64)
        assert len(set(steer.tolist())) == N and len(set(map(tuple, st["wheels"][:, :, 4].tolist()))) == N, name
        assert len(set(map(tuple, (st["on_road"] != 0).tolist()))) >= 2, f"{name} cw {cw}: on-road bits {st['on_road'].tolist()}"
