"""The grid observation of csrc/k_gridobs.h restated in numpy float64 (a helper, not a test): every cell centre against every polygon — the
same IEEE operations in the same order, no culling, no float32, no bands — so that the kernel's tensor can be compared with np.array_equal.

Inputs are what an oracle env hands out — state(), positions(), env_state()["visited"] — its episode (oracle.new_episode: track rows
(alpha, beta, x, y)) and the build's sinf/cosf spec evaluated on the host (mcr_sincos_host).  The road polygons are flags_ref.road_polys
(math.cos / math.sin of beta, as the host that packs an episode computes them), the predicate is flags_ref.crosses' / within's (restated for many points: `crosses` below; tests/test_grid_obs_ref.py pins the two
to each other), the hull polygons are
range_obs_ref.hull_segments'."""
import numpy as np

from tests import flags_ref, range_obs_ref
from tests.state_obs_ref import sincos_host

f64 = np.float64
GRID_ROAD, GRID_FRESH, GRID_TAKEN, GRID_CAR = 1, 2, 4, 8
CHUNK = 256                          # cells per batch of cross products


def default_origin(H, W):
    return (0.75 * H, 0.5 * W)


def centres(L, body, pos, H, W, cell, origin):
    """(qx, qy) [H, W] f64: the cell centres of the car with bodies row `body` [5, 6] f32 and body origin `pos` (f32 pair)"""
    s32, c32 = sincos_host(L, body[0, 2])
    s, c = f64(s32), f64(c32)
    fx, fy, rx, ry = -s, c, c, s
    cell = f64(np.float32(cell)); orow = f64(np.float32(origin[0])); ocol = f64(np.float32(origin[1]))
    i = np.arange(H, dtype=f64)[:, None]; j = np.arange(W, dtype=f64)[None, :]
    with np.errstate(all="ignore"):
        u = (orow - (i + 0.5)) * cell
        v = ((j + 0.5) - ocol) * cell
        qx = f64(np.float32(pos[0])) + (u * fx + v * rx)
        qy = f64(np.float32(pos[1])) + (u * fy + v * ry)
    return qx, qy


def crosses(polys, fx, fy):
    """[cells, P, n] f64: flags_ref.crosses' expression — (x2 - x1)(py - y1) - (y2 - y1)(px - x1), each product and difference rounded on its
    own — for many points at once (fx, fy [cells] f64) and polygons of any vertex count [P, n, 2]"""
    a = polys[None]; b = np.roll(polys, -1, axis=1)[None]
    px = np.asarray(fx, f64).reshape(-1, 1, 1); py = np.asarray(fy, f64).reshape(-1, 1, 1)
    with np.errstate(all="ignore"):
        return (b[..., 0] - a[..., 0]) * (py - a[..., 1]) - (b[..., 1] - a[..., 1]) * (px - a[..., 0])


def within_matrix(polys, qx, qy):
    """[H * W, P] bool: cell centre (row-major) strictly within polygon p of `polys` [P, n, 2] — every cross product > 0 or every one < 0"""
    fx, fy = qx.reshape(-1), qy.reshape(-1)
    out = np.zeros((len(fx), len(polys)), bool)
    for lo in range(0, len(fx), CHUNK):
        cr = crosses(polys, fx[lo:lo + CHUNK], fy[lo:lo + CHUNK])
        with np.errstate(all="ignore"):
            out[lo:lo + CHUNK] = (cr > 0).all(axis=2) | (cr < 0).all(axis=2)
    return out


def containing(polys, qx, qy):
    """[P] int: how many cell centres each polygon strictly contains"""
    return within_matrix(polys, qx, qy).sum(axis=0)


def hull_world_polygons(L, body, pos):
    """the four hull polygons of one car in world space: [n, 2] f64 each, in the stored vertex order"""
    s32, c32 = sincos_host(L, body[0, 2])
    ax, ay, _, _ = range_obs_ref.hull_segments(f64(np.float32(pos[0])), f64(np.float32(pos[1])), f64(s32), f64(c32))
    out, k = [], 0
    for poly in range_obs_ref.hull_polygons():
        out.append(np.stack([ax[k:k + len(poly)], ay[k:k + len(poly)]], axis=1)); k += len(poly)
    return out


def grid(L, bodies, positions, rows, tile_flags, H, W, cell, origin=None, polys=None):
    """bodies [N, 5, 6] f32, positions [N, 2] f32, rows [T, 4] f64 (alpha, beta, x, y), tile_flags [>= T] ints (bit c: car c visited the
    tile) -> [N, H, W] u8.  polys: flags_ref.road_polys(rows) if the caller has it"""
    N = bodies.shape[0]
    origin = default_origin(H, W) if origin is None else origin
    poly, tile, _ = flags_ref.road_polys(rows) if polys is None else polys
    flags = np.asarray(tile_flags).astype(np.int64)
    is_tile = tile >= 0
    tf = np.where(is_tile, flags[np.maximum(tile, 0)], 0)
    hulls = [hull_world_polygons(L, bodies[j], positions[j]) for j in range(N)]
    out = np.zeros((N, H, W), np.uint8)
    for a in range(N):
        qx, qy = centres(L, bodies[a], positions[a], H, W, cell, origin)
        others = ((1 << N) - 1) & ~(1 << a)
        w = within_matrix(poly, qx, qy)
        g = GRID_ROAD * w.any(axis=1).astype(np.uint8)
        g |= GRID_FRESH * w[:, is_tile & (((tf >> a) & 1) == 0)].any(axis=1).astype(np.uint8)
        g |= GRID_TAKEN * w[:, is_tile & ((tf & others) != 0)].any(axis=1).astype(np.uint8)
        for j in range(N):
            if j != a:
                for hp in hulls[j]:
                    g |= GRID_CAR * within_matrix(hp[None], qx, qy)[:, 0].astype(np.uint8)
        g = g.reshape(H, W)
        out[a] = g
    return out


def of_oracle(L, o, ep, H, W, cell, origin=None):
    """the tensor [N, H, W] of oracle env `o` playing episode `ep`"""
    return grid(L, o.state()["bodies"], o.positions(), ep["track"], o.env_state()["visited"], H, W, cell, origin)
