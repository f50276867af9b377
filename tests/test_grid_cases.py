"""CPU: the inputs of tests/test_gpu_grid_obs_kernel.py (tests/grid_cases.py) held to the situations they are there for, from the
restatement (tests/grid_obs_ref.py) alone — no GPU.  A pose set that stopped producing its situation would leave the kernel test green and
blind."""
import numpy as np
import pytest

from tests import grid_cases as GC
from tests import grid_obs_ref as G
from tests.util import hull_positions

ROAD, FRESH, TAKEN, CAR = G.GRID_ROAD, G.GRID_FRESH, G.GRID_TAKEN, G.GRID_CAR


@pytest.fixture(scope="module")
def L(lib):
    return lib.load()


def _sets(lib, L, N, names=None):
    tracks = GC.tracks_for(lib, N)
    if names is not None:
        tracks = [t for t in tracks if t[0] in names]
    base = np.zeros((len(tracks), N, 5, 6), np.float32)
    return tracks, GC.pose_sets(L, tracks, N, base), GC.flag_sets(tracks, N)


def _env(tracks, name, cw=None):
    return next(e for e, t in enumerate(tracks) if t[0] == name and (cw is None or t[2] == cw))


def test_centres_exactly_on_an_edge_and_one_float32_beside_it(lib, L):
    """border_loop, cell 1, heading 0, p.x = 0.5: the 32 centres of column 15 have x == 0, the border — in nothing; with p.x one float32 up
    they are road, one down they are grass: the three poses differ exactly there, inside any float32 test's band"""
    N = 3
    tracks, sets, flags = _sets(lib, L, N, ("border",))
    bodies = sets["edge"]; pos = hull_positions(L, bodies)
    H, W, cell, origin = GC.CONFIGS["pow2"]
    seen = set()
    for e, (name, rows, cw) in enumerate(tracks):
        poly = GC.road_polys(name, rows)[0]
        g = G.grid(L, bodies[e], pos[e], rows, flags["clear"][e], H, W, cell, origin)
        for a in range(N):
            qx, qy = G.centres(L, bodies[e, a], pos[e, a], H, W, cell, origin)
            v = GC.edge_variant(e, a); seen.add(v)
            col = g[a][:, 15] & ROAD
            if v == 0:
                assert int((qx == 0.0).sum()) == 32 and (qx[:, 15] == 0.0).all()
                assert int(GC.on_edge(poly, qx, qy).sum()) >= 32, "centres exactly on an edge"
                assert not col.any(), "a centre on the border is in nothing"
            elif v == 1:
                assert (qx[:, 15] > 0).all() and (qx[:, 15] < 1e-7).all() and col.all(), "one float32 to the right: road"
            else:
                assert (qx[:, 15] < 0).all() and (qx[:, 15] > -1e-7).all() and not col.any(), "one float32 to the left: grass"
            assert (g[a][:, 16] & ROAD).all() and not (g[a][:, 14] & ROAD).any()
    assert seen == {0, 1, -1}


def test_dense_and_all_entries_and_no_candidate(lib, L):
    N = 2
    tracks, sets, flags = _sets(lib, L, N, ("c512q", "wiggle"))
    pos = hull_positions(L, sets["dense"])
    e = _env(tracks, "c512q")
    H, W, cell, origin = GC.CONFIGS["default"]
    qx, qy = G.centres(L, sets["dense"][e, 0], pos[e, 0], H, W, cell, origin)
    n = int((G.containing(GC.road_polys("c512q", tracks[e][1])[0], qx, qy) > 0).sum())
    assert n >= 150, f"{n} polygons hold a cell centre"
    e = _env(tracks, "wiggle")
    meets = GC.view_box_meets(L, sets["dense"][e, 0], pos[e, 0], tracks[e][1], "wiggle", "big")
    assert len(meets) == 768 and meets.all(), "the 64 x 64 grid of 6.0 over wiggle's centroid meets every one of the 768 entries"
    far = hull_positions(L, sets["far"])
    for e, (name, rows, _) in enumerate(tracks):
        for a in range(N):
            assert not GC.view_box_meets(L, sets["far"][e, a], far[e, a], rows, name, "default").any(), "a view with no candidate at all"


def test_every_bit_set_and_clear_in_every_shape_and_kerb_only_cells(lib, L):
    N = 2
    names = ("wiggle", "circle20", "border", "c512q")
    tracks, sets, flags = _sets(lib, L, N, names)
    seen = {c: [0, 0xff] for c in GC.CONFIGS}
    kerb_only = 0
    for config, poses, bits, _ in GC.CASES:
        if poses in ("far", "nonfinite"):
            continue
        envs = [e for e, t in enumerate(tracks) if config != "big" or t[0] in GC.BIG_TRACKS]
        for g in GC.reference(L, tracks, sets[poses], flags[bits], config, envs).values():
            seen[config][0] |= int(np.bitwise_or.reduce(g, axis=None)); seen[config][1] &= int(np.bitwise_and.reduce(g, axis=None))
            if bits == "clear":
                kerb_only += int((g == ROAD).sum())                # (no visit bit set: a tile cell is FRESH, so ROAD alone is a kerb)
    for config, (any_set, all_set) in seen.items():
        assert any_set == ROAD | FRESH | TAKEN | CAR and all_set == 0, f"{config}: bits set somewhere {any_set:#x}, set everywhere {all_set:#x}"
    assert kerb_only >= 10, "kerb-only cells"


def test_cars_4_to_7_set_bit_3_and_a_car_overlaps_the_viewer(lib, L):
    N = 8
    tracks, sets, flags = _sets(lib, L, N, ("circle128", "lattice"))
    H, W, cell, origin = GC.CONFIGS["default"]
    bodies = sets["close"]; pos = hull_positions(L, bodies)
    hits = 0
    for e in range(len(tracks)):
        for a in range(4):                                          # a viewer among cars 0 .. 3: a cell under a hull of cars 4 .. 7
            qx, qy = G.centres(L, bodies[e, a], pos[e, a], H, W, cell, origin)
            for j in range(4, 8):
                hits += sum(int(G.within_matrix(hp[None], qx, qy).any()) for hp in G.hull_world_polygons(L, bodies[e, j], pos[e, j]))
    assert hits >= 4, "cars 4..7 under somebody's grid"
    bodies = sets["overlap"]; pos = hull_positions(L, bodies)
    for e, (name, rows, _) in enumerate(tracks):
        g = G.grid(L, bodies[e], pos[e], rows, flags["clear"][e], H, W, cell, origin)
        near = g[:, int(origin[0]) - 2:int(origin[0]) + 2, int(origin[1]) - 2:int(origin[1]) + 2]
        assert all((near[a] & CAR).any() for a in range(N)), "another car's hull lies across the viewer's own origin"
