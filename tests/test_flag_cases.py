"""CPU: the restatement of the backward / on-grass bookkeeping (tests/flags_ref.py) against the C++ oracle's on every finite case of
tests/flag_cases.py, and the conditions those cases are meant to hold — exact zeros where a pose is meant to stand on an edge, exact ties
and one-ulp gaps where they are meant, poses whose nearest track point lies in another block than the pose, both values of both flags in
every pose set.  No device: tests/test_gpu_flags_kernel.py compares csrc/k_flags.h with the same restatement on the same cases."""
import math

import numpy as np
import pytest

from multi_car_racing_amd import levels
from tests import flag_cases as F
from tests import flags_ref as R
from tests import obs_cases as C
from tests.util import hull_positions

RANDOM_SETS = ("scatter", "ties", "edges", "kerb_only", "culling", "far")      # the sets whose headings and velocities are drawn


@pytest.fixture(scope="module")
def tracks(lib):
    return F.all_tracks(lib)


@pytest.fixture(scope="module")
def geos(tracks):
    return F.geometry(tracks)


@pytest.fixture(scope="module")
def realised(lib, tracks, geos):
    """{set: [per track: [(case, pos f32 [2], vel f32 [2], angle f32)]]}: every case as obs_cases.place puts it into a car's bodies"""
    L = lib.load()
    out = {}
    zero = np.zeros((5, 6), np.float32)
    for s in F.SETS:
        per = []
        for e in range(len(tracks)):
            cs = F.cases(s, e, tracks, geos)
            with np.errstate(all="ignore"):
                bodies = np.stack([C.place(L, zero, *c[:5]) for c in cs])
            pos = hull_positions(L, bodies)
            per.append([(c, pos[i], bodies[i, 0, 3:5], bodies[i, 0, 2]) for i, c in enumerate(cs)])
        out[s] = per
    return out


def _finite(pos, vel, ang):
    return bool(np.isfinite(pos).all() and np.isfinite(vel).all() and np.isfinite(ang))


def test_tracks_are_what_they_say(lib, tracks, geos):
    names = [t[0] for t in tracks if not t[2]]
    assert names[-6:] == ["wiggle", "scs", "spur", "lap", "seam", "columns"] and len(tracks) == 2 * len(names)
    by = {t[0]: (t[1], g) for t, g in zip(tracks, geos)}
    rows, g = by["wiggle"]
    assert len(rows) == 512 and g.P == F.QUAD_CAP and g.owner[1] == 0 and g.tile[1] == -1, "the wiggle loop fills road_poly, tile 0 has a kerb"
    assert math.hypot(*(rows[0, 2:4] - rows[-1, 2:4])) < 3.6, "the wiggle loop closes"
    with pytest.raises(ValueError):                      # one kerb more does not fit: 768 is the largest P from_tracks accepts
        levels.from_tracks([F.walk(([-0.1012] * 24 + [0.0] * 31 + [0.1] * 41 + [0.0] * 32) * 4)], 1)
    rows, g = by["spur"]
    assert len(rows) == 44 and g.P == 49 and g.tile[47] == 43 and g.tile[48] == -1 and g.owner[48] == 43, "block 3 holds the kerb of tile 43 alone"
    rows, g = by["scs"]
    starts = [q for q in range(1, g.P) if g.tile[q] < 0 and g.tile[q - 2] >= 0 and g.tile[q - 1] >= 0]
    assert starts and all(q % F.QBLK not in (0, 1) for q in starts), "kerb runs start inside a block"
    assert len(by["lap"][0]) > 200 and by["lap"][1].P > len(by["lap"][0])
    assert any(g.P % F.QBLK == 0 for g in geos) and any(g.P % F.QBLK == 1 for g in geos) and any(g.P % F.QBLK == 15 for g in geos)


def test_kerb_rule_equals_the_staged_entries(lib, tracks, geos):
    """border[] and road_poly's order of the restatement against what from_tracks stages: the same owners in the same order, the same vertices"""
    for (name, rows, cw), g in zip(tracks, geos):
        ep = lib.unpack_episode(np.ascontiguousarray(levels.from_tracks([rows], 8, "CW" if cw else "CCW")[0]))
        m = ep["quad_meta"]
        assert ep["P"] == g.P and ep["T"] == len(rows), name
        assert np.array_equal((m >> 8) & 0x3ff, np.where(g.tile >= 0, g.tile + 1, 0)), name
        assert np.array_equal(m >> 18, np.where(g.tile < 0, g.owner + 1, 0)), name
        assert np.array_equal(ep["quads"], g.polys.astype(np.float32)), name
        # a kerb of side 0 — a straight tile that the in-place, wrapping spread of the flags reached — only where it is meant: the seam loop
        sides = [R.kerb_side(rows, int(g.owner[q])) for q in np.nonzero(g.tile < 0)[0]]
        assert (0.0 in sides) == (name == "seam"), f"{name}: kerb sides {sorted(set(sides))}"


def test_the_seam_loop_has_kerbs_of_side_zero_beside_others(tracks, geos, realised):
    """tiles T - 6 .. T - 4 of the seam loop are straight and carry kerbs: side 0, every vertex on the centre line, next to the kerb of tile
    T - 3 whose side is not 0.  The `side0 beside` poses lie where such a kerb would be with side +1 / -1 — inside that polygon, off every
    polygon there is: on the grass; the `side0 on` poses lie on the degenerate kerb, every cross product with it 0, on the road through a tile."""
    beside = on = 0
    for e, ((name, rows, cw), g) in enumerate(zip(tracks, geos)):
        if name != "seam":
            continue
        T = len(rows)
        kerb_of = {int(g.owner[q]): int(q) for q in np.nonzero(g.tile < 0)[0]}
        zero = sorted(t for t in kerb_of if R.kerb_side(rows, t) == 0.0)
        assert zero == [T - 6, T - 5, T - 4] and T - 3 in kerb_of and R.kerb_side(rows, T - 3) != 0.0, zero
        for t in zero:
            q = g.polys[kerb_of[t]]
            assert np.array_equal(q[0], q[1]) and np.array_equal(q[2], q[3]) and np.array_equal(q[0], rows[t, 2:4]) and np.array_equal(q[2], rows[t - 1, 2:4])
        for c, pos, vel, ang in realised["kerb_only"][e]:
            if not c[5].startswith("side0"):
                continue
            q, t = int(c[5].split()[2]), int(c[5].split()[-1])
            inside = R.within(g.polys, pos[0], pos[1])
            if c[5].startswith("side0 beside"):
                would = []
                for sd in (1.0, -1.0):
                    w0, w1 = sd * R.TRACK_WIDTH, sd * (R.TRACK_WIDTH + R.BORDER)
                    v = [(rows[k, 2] + w * np.cos(rows[k, 1]), rows[k, 3] + w * np.sin(rows[k, 1])) for k, w in ((t, w0), (t, w1), (t - 1, w1), (t - 1, w0))]
                    would.append(bool(R.within(np.array([v]), pos[0], pos[1])[0]))
                assert sum(would) == 1 and not inside.any(), f"{c}: inside the kerb of side +1 / -1 {would}, inside entries {np.nonzero(inside)[0].tolist()}"
                beside += 1
            else:
                cr = R.crosses(g.polys[q:q + 1], np.float64(pos[0]), np.float64(pos[1]))[0]       # (two edges have no length; the pose is a float32 rounding of the midpoint)
                assert (cr == 0.0).sum() >= 2 and (np.abs(cr) < 1e-3).all() and not inside[q]
                assert inside.any() and (g.tile[inside] >= 0).all(), f"{c}"
                on += 1
    assert beside == 2 * 2 * 3 and on == 2 * 3


def test_restatement_equals_the_oracle(oracle, tracks, geos, realised):
    """every finite case of every set: flags_ref.flags == orc_set_track + orc_set_hull_pose + orc_bookkeeping, the oracle holding the
    restatement's road_poly, kerbs included"""
    n = 0
    for e, ((name, rows, cw), g) in enumerate(zip(tracks, geos)):
        ep = dict(track=rows, poly=g.polys, color=np.full((g.P, 3), 0.4), tile_of_quad=g.tile, direction="CW" if cw else "CCW",
                  car_order=[0], poses=oracle.spawn_poses(rows, [0], cw))
        o = oracle.OracleEnv(1)
        try:
            o.reset_nostep(ep)
            for s in F.SETS:
                for c, pos, vel, ang in realised[s][e]:
                    if not _finite(pos, vel, ang):
                        continue
                    o.set_hull_pose(0, pos[0], pos[1], vel[0], vel[1], ang)
                    o.bookkeeping()
                    es = o.env_state()
                    bw, og, _ = R.flags(rows, cw, pos, vel, ang, g.polys)
                    assert (bool(es["driving_backward"][0]), bool(es["driving_on_grass"][0])) == (bw, og), f"{name} cw {cw} set {s} case {c}"
                    n += 1
        finally:
            o.close()
    assert n > 3000


def test_edges_hold_exact_zeros(tracks, geos, realised):
    """every deliberate `edges` case has a cross product that is exactly 0.0 and is within none of the polygons it touches; its neighbours
    stand one float32 step to either side"""
    seen = set()
    for e, ((name, rows, cw), g) in enumerate(zip(tracks, geos)):
        for c, pos, vel, ang in realised["edges"][e]:
            tag = c[5]
            cr = R.crosses(g.polys, np.float64(pos[0]), np.float64(pos[1]))
            if tag.startswith("exact"):
                assert (pos[0], pos[1]) == (np.float32(c[0]), np.float32(c[1])), f"{name} {c}: the hull stands at {pos.tolist()}"
                assert (cr == 0.0).any(), f"{name} {c}"
                zero_polys = np.nonzero((cr == 0.0).any(axis=1))[0]
                assert not R.within(g.polys[zero_polys], pos[0], pos[1]).any()
                if "kerb" in tag:
                    assert (g.tile[zero_polys] < 0).any(), f"{name} {c}: no kerb's edge"
                if "kerb-tile" in tag:
                    assert (g.tile[zero_polys] >= 0).any(), f"{name} {c}: no tile's edge"
                seen.add(tag)
    assert seen == {"exact border", "exact vertex", "exact seam", "exact kerb-tile edge", "exact kerb-tile vertex", "exact kerb outer edge", "exact kerb outer vertex"}
    # the neighbours of an exact case: one float32 step to either side, and the on-grass verdict differs somewhere
    flips = held = 0
    for e, ((name, rows, cw), g) in enumerate(zip(tracks, geos)):
        cs = realised["edges"][e]
        for i, (c, pos, vel, ang) in enumerate(cs):
            if not c[5].startswith("exact"):
                continue
            axis = 0 if cs[i + 1][0][1] == c[1] else 1
            lo, hi = cs[i + 1][1][axis], cs[i + 2][1][axis]
            assert lo < pos[axis] < hi and (lo, hi) == tuple(np.float32(v) for v in F._ulps(pos[axis])), f"{name} {c}: neighbours {lo!r} {hi!r}"
            grass = [not R.within(g.polys, p[0], p[1]).any() for p in (cs[i + 1][1], pos, cs[i + 2][1])]
            held += not grass[1]             # (on an edge, yet on the road: another polygon holds the pose strictly)
            flips += grass[1] and len(set(grass)) > 1
    assert flips >= 8 and held >= 2, (flips, held)


def test_ties_are_exact_and_ulp_pairs_are_one_ulp_apart(tracks, geos, realised):
    kinds = set()
    for e, ((name, rows, cw), g) in enumerate(zip(tracks, geos)):
        for c, pos, vel, ang in realised["ties"][e]:
            tag = c[5]
            d = R.distances(rows, np.float64(pos[0]), np.float64(pos[1]))
            if tag.startswith("tie"):
                tied = tuple(np.nonzero(d == d.min())[0].tolist())
                assert repr(tied) == tag[4:] and len(tied) >= 2 and R.track_index(rows, pos[0], pos[1]) == min(tied), f"{name} {c}: {tied}"
                kinds.add("tie")
                # where the kernel's block loop meets the tied tiles: (trip, lane) of the lowest and of another one
                lanes = F.scan_lanes(g, pos[0], pos[1])
                where = [lanes[int(g.entry_of_tile[t])] for t in tied]
                for (tr, ln) in where[1:]:
                    if ln == where[0][1] and tr != where[0][0]:
                        kinds.add("tie in one lane across trips")
                    if ln // 16 != where[0][1] // 16 and tr == where[0][0]:
                        kinds.add("tie across 16-lane groups")
                    if ln // 16 == where[0][1] // 16 and ln != where[0][1] and tr == where[0][0]:
                        kinds.add("tie inside a 16-lane group")
            elif tag.startswith("ulp"):
                i0, i1 = (int(v) for v in tag.split()[1:])
                assert (pos[0], pos[1]) == (np.float32(c[0]), np.float32(0.0)), f"{name} {c}: the hull stands at {pos.tolist()}"
                s = np.unique(d)
                assert d[i0] == s[0] and d[i1] == s[1] and s[1] == np.nextafter(s[0], np.inf) and (d == s[0]).sum() == 1, f"{name} {c}"
                assert R.track_index(rows, pos[0], pos[1]) == i0
                kinds.add("ulp low first" if i0 < i1 else "ulp high first")
    assert kinds == {"tie", "ulp low first", "ulp high first", "tie in one lane across trips", "tie across 16-lane groups", "tie inside a 16-lane group"}, kinds


def test_culling_cases_are_what_they_say(tracks, geos, realised):
    other = partial = 0
    for e, ((name, rows, cw), g) in enumerate(zip(tracks, geos)):
        for c, pos, vel, ang in realised["culling"][e]:
            tag = c[5]
            near = R.track_index(rows, pos[0], pos[1])
            if tag == "other block":
                holding = g.blocks_holding(pos[0], pos[1])
                assert len(holding) and g.block_of_tile(near) not in holding, f"{name} {c}"
                other += 1
            elif tag == "partial block":
                assert g.block_of_tile(near) == g.P // F.QBLK and g.P % F.QBLK, f"{name} {c}"
                partial += 1
            elif tag == "spur":
                # 5 from the tip of the straight, whose block's box ends there; further from every other track point; and the box of the
                # kerb-only last block lies within 2 of the pose: its far corner is nearer than the nearest track point
                assert near == F.SPUR_TIP and g.block_of_tile(near) == 1 and R.distances(rows, pos[0], pos[1])[near] == 5.0
                b = g.boxes[3]
                far = math.hypot(max(abs(pos[0] - b[0]), abs(pos[0] - b[2])), max(abs(pos[1] - b[1]), abs(pos[1] - b[3])))
                b1 = g.boxes[1]
                assert far < 2.0 and pos[1] - b1[3] == 5.0 and b1[0] <= pos[0] <= b1[2]
                assert R.within(g.polys, pos[0], pos[1]).nonzero()[0].tolist() == [48], "on the road through the kerb of tile 43 alone"
    assert other >= 20 and partial >= 20


def test_kerb_only_cases_are_on_the_road_through_a_kerb(tracks, geos, realised):
    kerb0 = block_start = n = 0
    for e, ((name, rows, cw), g) in enumerate(zip(tracks, geos)):
        for c, pos, vel, ang in realised["kerb_only"][e]:
            if not c[5].startswith("kerb"):
                continue
            inside = np.nonzero(R.within(g.polys, pos[0], pos[1]))[0]
            assert len(inside) and (g.tile[inside] < 0).all(), f"{name} {c}: inside {inside.tolist()}"
            n += 1
            kerb0 += int((g.owner[inside] == 0).any())
            block_start += int(any(q % F.QBLK == 0 and g.tile[q - 1] == g.owner[q] for q in inside))
    assert n >= 60 and kerb0 >= 2 and block_start >= 4, (n, kerb0, block_start)


def test_both_flags_take_both_values_in_every_set(tracks, geos, realised):
    for s in F.SETS:
        bw, og = set(), set()
        for e, ((name, rows, cw), g) in enumerate(zip(tracks, geos)):
            for c, pos, vel, ang in realised[s][e]:
                if s == "kerb_only" and not c[5].startswith("kerb"):
                    continue
                with np.errstate(all="ignore"):
                    b, o, _ = R.flags(rows, cw, pos, vel, ang, g.polys)
                bw.add(b); og.add(o)
        assert bw == {False, True}, f"{s}: backward {bw}"
        # (a kerb-only pose is on the road by construction; the far poses include 1e3 off the centroid only: all on grass)
        assert og == ({False} if s == "kerb_only" else {True} if s == "far" else {False, True}), f"{s}: on grass {og}"


def test_heading_cases_decide_what_they_are_meant_to(tracks, geos, realised):
    quarter = wraps = speed = axis_exact = 0
    for e, ((name, rows, cw), g) in enumerate(zip(tracks, geos)):
        per = {}
        for s in ("heading_slow", "heading_fast", "heading_speed", "heading_wrap"):
            for c, pos, vel, ang in realised[s][e]:
                near = R.track_index(rows, pos[0], pos[1])
                bw, diff, raw, sp = R.heading(rows, cw, near, vel[0], vel[1], ang)
                per.setdefault((s, c[5]), []).append((bw, diff, raw, sp))
        # the hull angle and its two float32 neighbours straddle the quarter turn
        q = per[("heading_slow", "quarter turn")]
        for i in range(0, len(q), 3):
            quarter += len({b for b, _, _, _ in q[i:i + 3]}) == 2
            assert all(abs(d - math.pi / 2) < 1e-6 and s == 0.0 for _, d, _, s in q[i:i + 3])
        sp = per[("heading_speed", "0.3 0.4")]
        assert {s > 0.5 for _, _, _, s in sp} == {False, True} and all(abs(s - 0.5) < 1e-7 for _, _, _, s in sp)
        speed += len({b for b, _, _, _ in sp}) == 2
        assert [s > 0.5 for _, _, _, s in per[("heading_speed", "0 0.5")]] == [False, True, False] and per[("heading_speed", "0 0.5")][0][3] == 0.5
        for tag in ("wrap low", "wrap high", "wrap low axis", "wrap high axis"):
            for bw, diff, raw, _ in per.get(("heading_wrap", tag), []):
                assert raw > math.pi, f"{name} {tag}"
                wraps += bw != (raw > math.pi / 2)
        axis_exact += sum(d in (0.0, math.pi / 2, math.pi) for _, d, _, _ in per[("heading_fast", "axis")])
    assert quarter >= 2 * len(tracks) and speed >= len(tracks) - 4 and wraps >= len(tracks) and axis_exact >= 8, (quarter, speed, wraps, axis_exact)


def test_random_headings_keep_clear_of_the_thresholds(tracks, geos, realised):
    """wherever a heading or a velocity is drawn, |diff - pi / 2|, |diff - pi| (before the wrap) and |speed - 0.5| stay above 1e-9: a last-ulp
    difference between two atan2 cannot decide a case.  The deliberate threshold cases use the hull's angle or axis-aligned velocities."""
    worst = math.inf
    for s in F.SETS:
        for e, ((name, rows, cw), g) in enumerate(zip(tracks, geos)):
            for c, pos, vel, ang in realised[s][e]:
                if not _finite(pos, vel, ang) or (s in RANDOM_SETS and not vel.any()):      # (the deliberate cases at rest — spur, columns — : hull angle 0 against beta 0 or pi, no atan2)
                    continue
                fast_general = math.hypot(float(vel[0]), float(vel[1])) > 0.5 and vel[0] != 0 and vel[1] != 0
                if s not in RANDOM_SETS and not fast_general:
                    continue
                near = R.track_index(rows, pos[0], pos[1])
                _, diff, raw, sp = R.heading(rows, cw, near, vel[0], vel[1], ang)
                m = min(abs(diff - math.pi / 2), abs(raw - math.pi))
                if s in RANDOM_SETS:
                    m = min(m, abs(sp - 0.5))
                assert m > 1e-9, f"{name} cw {cw} set {s} case {c}: margin {m!r}"
                worst = min(worst, m)
    assert worst > 1e-9
