"""Shapes, tracks, poses and visit bits for the grid-observation kernel (a helper, not a test): csrc/k_gridobs.h driven through its own
launch (mcr_set_grid_obs / mcr_grid_obs_now) on inputs no rollout reaches — tests/test_gpu_grid_obs_kernel.py.  The handle is
obs_cases.Rig(lib, tracks, N, None), pointed at a guarded BYTE buffer of this file at a chosen misalignment; tracks and poses come from
obs_cases / flag_cases plus a circle of 512 tiles 0.25 apart (a fan of 512 slivers: hundreds of polygons under one grid).

The host-side conditions on the inputs (centres exactly on an edge, a view that meets all 768 entries, one that meets none, ...) are
functions of the restatement (tests/grid_obs_ref.py) alone; tests/test_grid_cases.py holds them without a GPU."""
import numpy as np

from tests import flag_cases as F
from tests import flags_ref, grid_obs_ref as G
from tests import obs_cases as C
from tests.util import hull_positions

f32, f64 = np.float32, np.float64
TILE_CAP = 512

# name -> (H, W, cell, origin (row, col))
CONFIGS = {
    "default": (32, 32, 1.5, (24.0, 16.0)),          # VecMultiCarRacing's defaults
    "pow2": (32, 32, 1.0, (24.0, 16.0)),             # with a pose at (k + 0.5, .) and heading 0 the centres have integer coordinates
    "fine": (32, 32, 0.25, (24.0, 16.0)),
    "one": (1, 1, 1.0, (0.5, 0.5)),                  # the one centre is the hull's origin
    "big": (64, 64, 6.0, (32.0, 32.0)),              # 384 x 384 world units: a whole track
    "wide": (7, 64, 0.25, (3.5, 10.25)),
    "tall": (64, 3, 1.0, (70.0, -2.0)),              # the origin lies outside the grid: the car looks at cells behind and beside it
    "odd": (33, 17, 1.5, (20.3, 8.7)),               # odd H * W: a view's base is odd in every second view
}
# (config, pose set, visit bits, byte offset of the buffer from a 16-byte boundary); "big" runs at N <= 2 on BIG_TRACKS only: 64 x 64 x 768
# decisions per view are the restatement's slow side
CASES = [
    ("default", "scatter", "random", 0), ("default", "close", "all", 1), ("default", "border", "clear", 2), ("default", "far", "random", 3),
    ("default", "nonfinite", "high", 0), ("default", "dense", "random", 1), ("default", "overlap", "bit8", 2),
    ("pow2", "edge", "random", 3), ("pow2", "scatter2", "all", 0),
    ("fine", "scatter", "random", 0), ("fine", "overlap", "clear", 1),
    ("one", "scatter", "random", 1), ("one", "centre", "all", 0), ("one", "close", "clear", 3),
    ("big", "dense", "random", 3), ("big", "scatter", "clear", 0),
    ("wide", "scatter", "random", 2), ("wide", "overlap", "high", 1),
    ("tall", "scatter", "random", 3), ("tall", "border", "all", 0),
    ("odd", "close", "random", 1), ("odd", "edge", "clear", 2), ("odd", "overlap", "random", 3),
]
BIG_TRACKS = ("wiggle", "c512q", "border", "truncated", "circle128")
EDGE_POSE = (0.5, 40.0)              # on border_loop: 0.5 to the right of the border x = 0


def tracks_for(lib, N):
    """[(name, rows, cw)]: N == 2 — obs_cases' tracks in both directions and four more; any other N — nine of them"""
    more = [("wiggle", F.wiggle(), False), ("scs", F.scs(), True), ("columns", F.columns(), False), ("c512q", C.circle(512, 0.25), False)]
    base = C.all_tracks(lib)
    if N != 2:
        keep = {("circle20", True), ("circle512", False), ("circle128", True), ("lattice", False), ("border", True), ("border", False), ("truncated", False)}
        base = [t for t in base if (t[0], t[2]) in keep]
    return base + more


# ------------------------------------------------------------------------------------------------------------------------------ poses
def _ulp_x(px, k):
    """px moved k float32 steps"""
    px = f32(px)
    for _ in range(abs(k)):
        px = np.nextafter(px, f32(np.inf if k > 0 else -np.inf))
    return float(px)


def edge_variant(e, a):
    """which of the three neighbouring float32 p.x car a of env e takes in the pose set "edge": 0 exact, +1, -1"""
    return (0, 1, -1)[(a + e) % 3]


def pose_sets(L, tracks, N, base):
    """obs_cases.pose_sets plus: "edge" (border_loop: EDGE_POSE at heading 0, p.x exact or one float32 up or down — with a power-of-two cell
    32 centres lie exactly on the border x = 0, or 1e-8 beside it; elsewhere: on a track point, looking down the track), "dense" (every
    car at the track's centroid, turned by 0.7 a — on c512q a fan of slivers under the grid, on wiggle with "big" the whole track) and
    "overlap" (the cars 0.4 apart on a track point: every hull lies across every viewer's origin)"""
    sets = C.pose_sets(L, tracks, N, base)
    B = len(tracks)

    def build(fn):
        out = np.zeros((B, N, 5, 6), f32)
        for e, (name, rows, cw) in enumerate(tracks):
            for a in range(N):
                px, py, ang = fn(e, a, name, rows)
                out[e, a] = C.place(L, base[e, a], px, py, ang, 1.0, 2.0)
        return out

    def edge(e, a, name, rows):
        if name == "border":
            return _ulp_x(EDGE_POSE[0], edge_variant(e, a)), EDGE_POSE[1] + 4.0 * (a // 3), 0.0
        i = (7 + 5 * a + e) % len(rows)
        return rows[i, 2], rows[i, 3], rows[i, 1]
    sets["edge"] = build(edge)

    def dense(e, a, name, rows):
        cx, cy = (0.0, 0.0) if name.startswith(("circle", "c512q")) else (float(rows[:, 2].mean()), float(rows[:, 3].mean()))
        return cx + 0.01 * a, cy - 0.02 * a, 0.7 * a
    sets["dense"] = build(dense)

    def overlap(e, a, name, rows):
        i = (3 + e) % len(rows)
        return rows[i, 2] + 0.4 * a, rows[i, 3] - 0.3 * a, rows[i, 1] + 0.5 * a
    sets["overlap"] = build(overlap)
    return sets


# ------------------------------------------------------------------------------------------------------------------------------ visit bits
def flag_sets(tracks, N):
    """{name: tile_flags [B, TILE_CAP] u16}: clear; random bits of the N cars; every bit of the N cars; "high": random bits >= N and bit 8
    (the recolour bit) — no car's, the grid must equal "clear"'s; "bit8": random bits of the cars and bit 8 everywhere"""
    B = len(tracks)
    rng = np.random.RandomState(20 + N)
    low = (rng.randint(0, 1 << N, (B, TILE_CAP)) & rng.randint(0, 1 << N, (B, TILE_CAP))).astype(np.uint16)       # (about a quarter of the bits)
    high = ((rng.randint(0, 256, (B, TILE_CAP)) & ~((1 << N) - 1) & 0xff) | 0x100).astype(np.uint16)
    return {"clear": np.zeros((B, TILE_CAP), np.uint16), "random": low, "all": np.full((B, TILE_CAP), (1 << N) - 1, np.uint16), "high": high,
            "bit8": (low | 0x100).astype(np.uint16)}


# ------------------------------------------------------------------------------------------------------------------------------ restatement
_polys = {}


def road_polys(name, rows):
    key = (name, len(rows), float(rows[0, 2]), float(rows[-1, 3]))
    if key not in _polys:
        _polys[key] = flags_ref.road_polys(rows)
    return _polys[key]


def reference(L, tracks, bodies, flags, config, envs=None):
    """{env: [N, H, W] u8} of grid_obs_ref.grid on get_state()'s bodies, hull_positions and the track rows"""
    H, W, cell, origin = CONFIGS[config]
    pos = hull_positions(L, bodies)
    envs = range(len(tracks)) if envs is None else envs
    with np.errstate(all="ignore"):
        return {e: G.grid(L, bodies[e], pos[e], tracks[e][1], flags[e], H, W, cell, origin, polys=road_polys(tracks[e][0], tracks[e][1])) for e in envs}


def view_box_meets(L, body, pos, rows, name, config):
    """[P] bool: the box of the view's cell centres meets the box of road_poly entry p (closed boxes, float64)"""
    H, W, cell, origin = CONFIGS[config]
    qx, qy = G.centres(L, body, pos, H, W, cell, origin)
    poly = road_polys(name, rows)[0]
    with np.errstate(all="ignore"):
        return ((poly[:, :, 0].min(1) <= qx.max()) & (poly[:, :, 0].max(1) >= qx.min()) & (poly[:, :, 1].min(1) <= qy.max()) & (poly[:, :, 1].max(1) >= qy.min()))


def on_edge(poly, qx, qy):
    """[H, W] bool: the centre lies on an edge of some polygon — one cross product is exactly 0 and the polygon's others share a sign"""
    out = np.zeros(qx.size, bool)
    fx, fy = qx.reshape(-1), qy.reshape(-1)
    for lo in range(0, len(fx), G.CHUNK):
        cr = G.crosses(poly, fx[lo:lo + G.CHUNK], fy[lo:lo + G.CHUNK])
        zero = cr == 0
        rest_pos = ((cr > 0) | zero).all(axis=2); rest_neg = ((cr < 0) | zero).all(axis=2)
        out[lo:lo + G.CHUNK] = (zero.any(axis=2) & (rest_pos | rest_neg) & (zero.sum(axis=2) == 1)).any(axis=1)
    return out.reshape(qx.shape)


# ------------------------------------------------------------------------------------------------------------------------------ the handle
GUARD = 256                          # sentinel bytes in front of and behind a tensor under test
SENTINEL, STALE = 0xA5, 0x5A


class GridRig(C.Rig):
    """obs_cases.Rig without a derived observation of its own: the grid is set through the C ABI on a guarded byte buffer"""

    def __init__(self, lib, tracks, N, **kw):
        super().__init__(lib, tracks, N, None, **kw)

    def guarded_bytes(self, n, offset):
        """(whole u8 tensor of SENTINEL, the n-byte view that starts `offset` bytes behind a 16-byte boundary, filled with STALE)"""
        whole = self.torch.full((n + 2 * GUARD + 32,), SENTINEL, dtype=self.torch.uint8, device=self.env.device)
        start = GUARD + (-(whole.data_ptr() + GUARD)) % 16 + offset
        view = whole[start:start + n]
        assert view.data_ptr() % 16 == offset
        view.fill_(STALE)
        self.held = whole
        return whole, view, start

    def launch(self, config, offset=0):
        """the kernel's tensor [B, N, H, W] for the handle's current state; the bytes around it must stay SENTINEL"""
        import ctypes
        H, W, cell, origin = CONFIGS[config]
        n = self.B * self.N * H * W
        whole, view, start = self.guarded_bytes(n, offset)
        st = self.torch.cuda.current_stream(self.env.device)
        assert self.L.mcr_set_grid_obs(self.env.h, ctypes.c_void_p(view.data_ptr()), H, W, ctypes.c_float(cell), ctypes.c_float(origin[0]), ctypes.c_float(origin[1])) == 0
        assert self.L.mcr_grid_obs_now(self.env.h, ctypes.c_void_p(st.cuda_stream)) == 0
        st.synchronize()
        h = whole.cpu().numpy()
        assert (h[:start] == SENTINEL).all() and (h[start + n:] == SENTINEL).all(), "the bytes around the tensor were written"
        return h[start:start + n].reshape(self.B, self.N, H, W).copy()

    def close(self):
        self.L.mcr_set_grid_obs(self.env.h, None, 0, 0, 0.0, 0.0, 0.0)      # (the handle never holds a pointer to freed memory)
        super().close()
