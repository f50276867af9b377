"""CPU: the grid observation's numpy restatement (tests/grid_obs_ref.py) pinned independently of the kernel — against the oracle's own
driving_on_grass and visit bits on rollouts, against flags_ref's single-point predicate, and against an even-odd crossing test written here."""
import math

import numpy as np
import pytest

from tests import flags_ref
from tests import grid_obs_ref as G
from tests.util import oracle_episode

ROAD, FRESH, TAKEN, CAR = G.GRID_ROAD, G.GRID_FRESH, G.GRID_TAKEN, G.GRID_CAR


@pytest.fixture(scope="module")
def L(lib):
    return lib.load()


def _weave(N, k):
    """every car accelerates and weaves ever wider: onto the grass and back"""
    a = np.zeros((N, 3), np.float32)
    for c in range(N):
        a[c, 0] = 0.9 * math.sin(0.11 * k + 1.3 * c) * min(1.0, k / 30.0)
        a[c, 1] = 0.6 if k < 45 else 0.15
    return a


@pytest.mark.parametrize("N", [1, 2, 3])
def test_own_cell_is_road_iff_the_oracle_is_not_on_grass_and_bits_follow_visited(oracle, L, N):
    """With origin (i + 0.5, j + 0.5) cell (i, j)'s centre is the hull's origin: bit 0 there is 1 - driving_on_grass after every step past
    the first (the flag is computed inside step, from the pose the step ended with).  After reset and later a cell is FRESH for car a and
    TAKEN for car b exactly as `visited` says for the tiles that contain it — after reset that is two tiles per car, the ones it spawned on."""
    ep = oracle_episode(oracle, N, 900 + N, 0)
    o = oracle.OracleEnv(N)
    o.reset(ep, render=False)
    rows = ep["track"]
    polys = flags_ref.road_polys(rows)
    poly, tile, _ = polys
    H, W, cell = 9, 8, 2.5
    origin = (5.5, 3.5)                                           # cell (5, 3)'s centre is p

    def bits_follow_visited(g, what):
        es, st, pos = o.env_state(), o.state(), o.positions()
        visited = es["visited"].astype(np.int64)
        for a in range(N):
            qx, qy = G.centres(L, st["bodies"][a], pos[a], H, W, cell, origin)
            for i in range(H):
                for j in range(W):
                    inside = flags_ref.within(poly, qx[i, j], qy[i, j])           # the single-point predicate the flags are pinned with
                    tiles = tile[inside & (tile >= 0)]
                    fresh = any(not (visited[t] >> a) & 1 for t in tiles)
                    taken = any(visited[t] & ((1 << N) - 1) & ~(1 << a) for t in tiles)
                    want = (ROAD if inside.any() else 0) | (FRESH if fresh else 0) | (TAKEN if taken else 0)
                    assert g[a, i, j] & 7 == want, f"{what} car {a} cell ({i}, {j})"

    # the first state of an episode: reset's own action-less step has put every car's wheels on the tiles it stands on (the reference marks
    # them visited and pays for them, :113-120) — those and no others; everything else on a tile is FRESH, and TAKEN only under a neighbour
    g = G.of_oracle(L, o, ep, H, W, cell, origin)
    bits_follow_visited(g, "after reset")
    v0 = o.env_state()["visited"]
    assert 1 <= int((v0 != 0).sum()) <= 2 * N and o.env_state()["tile_visited_count"].tolist() == [2] * N
    assert (g & FRESH).any() and (N > 1 or not (g & TAKEN).any())
    seen = set()
    for k in range(70):
        o.step(_weave(N, k), render=False)
        es = o.env_state()
        g = G.grid(L, o.state()["bodies"], o.positions(), rows, es["visited"], H, W, cell, origin, polys=polys)
        if k >= 1:
            for a in range(N):
                assert int(g[a, 5, 3] & ROAD) == 1 - int(es["driving_on_grass"][a]), f"step {k} car {a}"
                seen.add(int(es["driving_on_grass"][a]))
        if k % 10 == 9:
            bits_follow_visited(g, f"step {k}")
    assert seen == {0, 1}, "the cars were driven onto the grass and back"
    assert int((o.env_state()["visited"] != 0).sum()) > 2 * N, "tiles were visited on the way"
    o.close()


def _even_odd(pts, x, y):
    """is (x, y) inside the polygon by the crossing-number rule"""
    inside = False
    n = len(pts)
    for k in range(n):
        (x1, y1), (x2, y2) = pts[k], pts[(k + 1) % n]
        if (y1 > y) != (y2 > y) and x < x1 + (y - y1) * (x2 - x1) / (y2 - y1):
            inside = not inside
    return inside


def _edge_distance(pts, x, y):
    d = math.inf
    n = len(pts)
    for k in range(n):
        (x1, y1), (x2, y2) = pts[k], pts[(k + 1) % n]
        ex, ey = x2 - x1, y2 - y1
        t = min(1.0, max(0.0, ((x - x1) * ex + (y - y1) * ey) / (ex * ex + ey * ey)))
        d = min(d, math.hypot(x - (x1 + t * ex), y - (y1 + t * ey)))
    return d


def test_car_bit_against_an_even_odd_crossing_test(oracle, L):
    """bit 3 on the oracle's spawn grid of three cars, a fine grid over the neighbours: equal to the crossing-number rule on every cell
    farther than 1e-6 from every hull edge"""
    N = 3
    ep = oracle_episode(oracle, N, 77, 0)
    o = oracle.OracleEnv(N)
    o.reset(ep, render=False)
    st, pos = o.state(), o.positions()
    H, W, cell, origin = 40, 40, 0.5, (20.0, 20.0)
    g = G.of_oracle(L, o, ep, H, W, cell, origin)
    checked = hits = 0
    for a in range(N):
        qx, qy = G.centres(L, st["bodies"][a], pos[a], H, W, cell, origin)
        hulls = [hp for j in range(N) if j != a for hp in G.hull_world_polygons(L, st["bodies"][j], pos[j])]
        for i in range(H):
            for j in range(W):
                x, y = float(qx[i, j]), float(qy[i, j])
                if min(_edge_distance(hp.tolist(), x, y) for hp in hulls) <= 1e-6:
                    continue
                want = any(_even_odd(hp.tolist(), x, y) for hp in hulls)
                assert bool(g[a, i, j] & CAR) == want, f"car {a} cell ({i}, {j})"
                checked += 1; hits += want
    assert checked > 0.99 * N * H * W and hits >= 20
    o.close()


def test_many_point_cross_products_are_flags_refs(L):
    """grid_obs_ref.crosses / within_matrix on many points against flags_ref.crosses / within on each of them, NaN and inf included"""
    rng = np.random.RandomState(3)
    from tests import obs_cases as C
    poly = flags_ref.road_polys(C.circle(64))[0]
    px = np.concatenate([rng.uniform(-45, 45, 60), [np.nan, np.inf, 0.0, poly[3, 0, 0]]])
    py = np.concatenate([rng.uniform(-45, 45, 60), [1.0, 2.0, -np.inf, poly[3, 0, 1]]])
    cr = G.crosses(poly, px, py)
    w = G.within_matrix(poly, px, py)
    for k in range(len(px)):
        one = flags_ref.crosses(poly, px[k], py[k])
        assert np.array_equal(cr[k], one, equal_nan=True)
        assert np.array_equal(w[k], flags_ref.within(poly, px[k], py[k]))
    assert w[:60].any() and not w[60:].any(), "NaN, inf and a vertex are in nothing"
