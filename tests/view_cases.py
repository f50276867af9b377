"""Synthetic scenes for the main raster (a helper, not a test): csrc/k_view.h, with the record it draws from (csrc/k_carview.h), through a
launch of its own (mcr_obs_now) on states no rollout reaches — tests/test_gpu_view_kernel.py.  tests/test_view_cases.py holds the cases to
what they are meant to be without a device: the oracle's frames stay inside the ambiguity cap, every branch of the candidate layout is
reached with a margin, the oracle's setters round-trip.

A case is the whole drawn state of an env: the five bodies of every car, the wheels' spin and stripe phase, the rewards (the score label),
the episode clock (the zoom), the tiles' touched bits.  Everything is generated in float64 from fixed seeds and rounded once; the same
arrays go to the device (set_bodies / set_wheels / set_env_state) and to each env's oracle (set_body / set_render_state / set_time /
set_reward / set_touched), whose episode is the device's own blob unpacked — both sides draw the same road_poly.

A car is placed by its hull's body origin (what the camera follows) and heading; `ego_frame` places it in another car's view by pixel."""
import math

import numpy as np

from tests import flag_cases as F
from tests.util import rigid_teleport

f32, f64 = np.float32, np.float64
SETS = ("zoom", "crowd", "field", "hud", "tiles", "generic")
NS = (1, 2, 3, 5, 8)
EGO_COLOR_NS = (3, 8)                  # the rigs created with use_ego_color
AMB_CAP = 256                          # ambiguous pixels per view a case may have
BUDGET = 40                            # the project's budget of differing edge pixels per view
PLAYFIELD = 2000 / 6.0
ZOOM_IN = 2.7 * 6.0                    # window units per world unit once the camera has zoomed in
PX, PY = ZOOM_IN * 96 / 1000, ZOOM_IN * 96 / 800      # pixels per world unit, zoomed in: 1.555 across, 1.944 along
CAR_RADIUS = 4.5                       # csrc/k_view.h
MID = (0.05, -0.7)                     # the middle of vertices 0 and 4 of the hull's 8-gon in the hull's frame: (25, 20) and (-20, -90) x 0.02 / 2
OFF = (0.137, 0.071)                   # a fixed offset for scenes that would otherwise be axis-aligned
TILT = 0.0313                          # ... and a heading offset

# (name, cw) of tests/flag_cases.all_tracks: a small circle, the loop that fills road_poly (48 blocks, 64 kerbs in both colours), the lattice,
# kerbs in both colours, the truncated lap, a generated lap, three columns of tiles close together, a loop whose seam lies in a kerbed bend;
# and one walk of flag_cases' builder that none of its tracks has: a ring tight enough for a kerb on every tile (KERBRING_T)
TRACKS = (("circle20", False), ("wiggle", False), ("wiggle", True), ("lattice", False), ("scs", True), ("truncated", False), ("lap", False),
          ("columns", False), ("seam", True), ("kerbring", False))
KERBRING_T = 90                        # tiles 1.0 apart on a circle of radius 14.3: every tile kerbed, 180 road_poly entries (12 blocks) inside ONE zoomed-in view
T_VALUES = (0.0, 0.02, 0.5, 0.98, 1.0, 1.02, 37.4)
SPEEDS = (0.0, 0.49, 0.51, 50.0, 199.0, 201.0, 400.0, 5000.0)
REWARDS = (-0.5, 0.999, -1.0, 9.0, 999.0, 1000.0, 9999.0, 10000.0, -1000.0, 99999.0, -99999.0, 999999.0, 1000000.0, -100000.0, 1999999999.0, 2.5e9)
OMEGAS = (-400.0, -99.0, 0.0, 550.0, 101.0, 399.0, 401.0, 1000.0)      # (550: a gauge 3.6 px taller than the bar; 401: 0.02 px)
HULL_W = (1.0, -1.0, 50.0, -50.0, 0.0, 12.5)
STEER = (0.42, -0.42, 0.0, 0.21)
# quad_meta's colour id -> the colour the reference gives the road_poly entry (multi_car_racing.py:300-337)
COLOURS = np.array([[0.4 + 0.01 * k] * 3 for k in range(3)] + [[1.0, 1.0, 1.0], [1.0, 0.0, 0.0]])


def tracks(lib):
    every = {(name, cw): (name, rows, cw) for name, rows, cw in F.all_tracks(lib)}
    every[("kerbring", False)] = ("kerbring", F.walk([2 * math.pi / KERBRING_T] * KERBRING_T, step=1.0), False)
    return [every[k] for k in TRACKS]


def label_text(reward):
    """"%04i" % reward as the build defines it (csrc/mcr_kernels.h: mcr_label_value): truncation towards zero, 0 beyond +-2e9"""
    r = float(reward)
    return "%04i" % (int(r) if -2.0e9 < r < 2.0e9 else 0)


def episode_of(lib, O, blob, N):
    """the oracle's episode dict of a device blob: the blob's own quads, colours and tiles"""
    ep = lib.unpack_episode(np.ascontiguousarray(blob))
    m = ep["quad_meta"]
    rows = np.stack([ep["alpha"], ep["track"][:, 2], ep["track"][:, 0], ep["track"][:, 1]], axis=1)
    return dict(track=rows, poly=ep["quads"].astype(f64), color=COLOURS[m & 0xff], tile_of_quad=(((m >> 8) & 0x3ff).astype(np.int32) - 1),
                direction="CW" if ep["cw"] else "CCW", car_order=list(range(N)), poses=O.spawn_poses(rows, list(range(N)), ep["cw"]),
                quads32=ep["quads"])


# ------------------------------------------------------------------------------------------------------------------------------ cases
class Car:
    """one car of a case: hull body origin (x, y), heading, hull velocity, what the HUD shows"""

    def __init__(self, x, y, ang, vx=0.0, vy=0.0, hw=0.0, steer=0.0, omega=(0.0, 0.0, 0.0, 0.0), phase=(0.0, 0.0, 0.0, 0.0), reward=0.0, tag=""):
        self.x, self.y, self.ang, self.vx, self.vy, self.hw, self.steer = x, y, ang, vx, vy, hw, steer
        self.omega, self.phase, self.reward, self.tag = tuple(omega), tuple(phase), reward, tag


def ego_frame(ego, px, py, ang_rel, **kw):
    """a car whose hull MIDDLE (what the raster's visibility test looks at) lies at pixel (px, py) — GL rows, the scene is y 12 .. 96 — of
    the zoomed-in view of `ego` (at rest: the camera looks along its heading), its heading ang_rel away from the ego's"""
    a = ego.ang
    r, f = (px - 48.0) / PX, (py - 24.0) / PY
    mx = ego.x + r * math.cos(a) - f * math.sin(a); my = ego.y + r * math.sin(a) + f * math.cos(a)
    b = a + ang_rel
    return Car(mx - (MID[0] * math.cos(b) - MID[1] * math.sin(b)), my - (MID[0] * math.sin(b) + MID[1] * math.cos(b)), b, **kw)


def cull_reach(ang):
    """the raster's reach round the scene rectangle for a car's middle, in pixels across / along, for a camera at angle `ang`"""
    k = abs(math.cos(ang)) + abs(math.sin(ang))
    return CAR_RADIUS * PX * k + 1.0, CAR_RADIUS * PY * k + 1.0


def _along(rows, cw, i):
    """the heading of a car that follows the track at point i"""
    return float(rows[i % len(rows), 1]) - (math.pi if cw else 0.0)


def _on_track(rows, cw, i, lateral=0.0, dang=0.0, **kw):
    i %= len(rows)
    b = float(rows[i, 1])
    return Car(float(rows[i, 2]) + lateral * math.cos(b) + OFF[0], float(rows[i, 3]) + lateral * math.sin(b) + OFF[1], _along(rows, cw, i) + TILT + dang, **kw)


def _spin(rng):
    return dict(omega=tuple(rng.uniform(-60, 90, 4)), phase=tuple(rng.uniform(-40, 40, 4)), hw=float(rng.uniform(-2, 2)), steer=float(rng.uniform(-0.4, 0.4)))


def _dense_tile(name, rows):
    """a tile on a dense stretch: in a kerbed bend where the track has one, between the columns of `columns`, on the lattice's short side"""
    return {"wiggle": 70, "scs": 16, "lap": 0, "seam": 2, "columns": 40, "lattice": 41, "circle20": 3, "truncated": 50, "kerbring": 0}[name]


# what the cars behind the ego of the crowd set are: (pixel of the hull's middle in the ego's view, heading relative to the ego's)
def _crowd_roles(ang):
    rx, ry = cull_reach(ang)
    m = 0.8                                        # world units either side of the raster's reach: 1.2 px and more
    inside = [
        ("stacked", 48.0, 24.0 - 0.7 * PY, 0.3), ("stacked across", 49.0, 25.0, 1.4),
        ("left quarter", -1.5, 50.0, math.pi / 2), ("right quarter", 97.5, 60.0, math.pi / 2),
        ("top quarter", 30.0, 97.9, 0.0), ("bottom quarter", 70.0, 10.5, math.pi),
        ("under the bar", 20.0, 5.0, 0.4),
        # the front wing's corners are the farthest a car reaches from its middle, 3.46: the middle 2.9 outside, heading for the frame, a strip
        # 0.4 wide (0.6 px and more) inside it — drawn only if the raster's reach is no shorter than the car
        ("left wing", -2.9 * PX, 40.0, -math.pi / 2), ("top wing", 20.0, 96.0 + 2.9 * PY, math.pi),
        ("right wing", 96.0 + 2.9 * PX, 30.0, math.pi / 2), ("bottom wing", 85.0, 12.0 - 2.9 * PY, 0.0),
        ("within right", 96.0 + rx - m * PX, 70.0, 0.7), ("within left", -rx + m * PX, 30.0, 2.0), ("within top", 80.0, 96.0 + ry - m * PY, 2.5),
    ]
    beyond = [("beyond right", 96.0 + rx + m * PX, 40.0, 0.7), ("beyond top", 60.0, 96.0 + ry + m * PY, 0.2), ("beyond below", 40.0, 12.0 - ry - m * PY, 1.0),
              ("beyond left", -rx - m * PX, 80.0, 1.9)]
    return inside, beyond


def _field_spots():
    P = PLAYFIELD
    out = []
    for sx, sy in ((1, 1), (-1, 1), (-1, -1), (1, -1), (1, 0), (0, 1), (-1, 0), (0, -1)):
        for d, what in ((-5.0, "inside"), (4.0, "outside")):
            out.append((sx * (P + d) + (0 if sx else 17.3), sy * (P + d) + (0 if sy else -41.9), f"{what} {sx} {sy}"))
    out += [(400.0, 12.0, "400"), (-5000.0, 5000.0, "5000"), (30.0, -400.0, "400"), (5000.0, 77.0, "5000")]
    return out


def env_case(set_name, rnd, e, name, rows, cw, N):
    """(cars [N], t, touched [T] uint8) of env e in round `rnd` of a set"""
    T = len(rows)
    rng = np.random.RandomState(1000 * (SETS.index(set_name) + 1) + 100 * rnd + e)
    touched = np.zeros(T, np.uint8)
    t = 1.02
    if set_name == "zoom":
        t = T_VALUES[(e - 1 + 3 * rnd) % len(T_VALUES)]         # (env 1, the largest track, at t = 0 in round 0)
        lat = (0.0, 3.0, -7.5, 10.0, -12.0, 5.0, 20.0, -4.0)
        cars = [_on_track(rows, cw, int(rng.randint(T)), lat[a], float(rng.uniform(-0.5, 0.5)), reward=float(rng.uniform(-50, 900)), tag=f"lateral {lat[a]}", **_spin(rng))
                for a in range(N)]
    elif set_name == "crowd":
        ego = _on_track(rows, cw, _dense_tile(name, rows), 0.0, 0.0, tag="ego", **_spin(rng))
        inside, beyond = _crowd_roles(-ego.ang)
        cars = [ego]
        for a in range(1, N):                      # round 0: every car inside the ego's view; round 1: every other one beyond the raster's reach
            what, px, py, rel = beyond[(a // 2 + e) % len(beyond)] if rnd == 1 and a % 2 == 1 else inside[(a - 1 + 3 * e) % len(inside)]
            cars.append(ego_frame(ego, px, py, rel, tag=what, reward=float(a), **_spin(rng)))
        touched[::3] = 1
    elif set_name == "field":
        spots = _field_spots()
        cars = []
        for a in range(N):
            x, y, what = spots[(a + 3 * e + 11 * rnd) % len(spots)]
            cars.append(Car(x, y, float(rng.uniform(-3, 3)), tag=what, reward=float(rng.uniform(0, 500)), **_spin(rng)))
    elif set_name == "hud":
        cars = []
        for a in range(N):
            k = rnd * len(TRACKS) * N + e * N + a
            against = (k // 2) % 2 == 1                            # the backwards flag: looking and moving against the track
            speed = SPEEDS[(k + k // len(REWARDS)) % len(SPEEDS)]
            c = _on_track(rows, cw, 10 + 7 * a, 0.0, math.pi if against else 0.0, reward=REWARDS[k % len(REWARDS)], hw=HULL_W[k % len(HULL_W)], steer=STEER[k % len(STEER)],
                          omega=tuple(OMEGAS[(k + 3 * w) % len(OMEGAS)] for w in range(4)), phase=tuple(rng.uniform(-40, 40, 4)),
                          tag=f"reward {REWARDS[k % len(REWARDS)]} speed {speed} {'against' if against else 'along'}")
            d = c.ang + 0.3                                        # the velocity's direction is not the hull's: above speed 0.5 the camera follows it
            c.vx, c.vy = -math.sin(d) * speed, math.cos(d) * speed
            cars.append(c)
    elif set_name == "tiles":
        pat = (e + rnd) % 5
        if pat == 1: touched[:] = 1
        elif pat == 2: touched[::2] = 1
        elif pat == 3: touched[0] = 1
        elif pat == 4: touched[T - 1] = 1
        at = (0, T - 1, 1, T - 2, T // 2, T // 3, 2, T // 2 + 1)
        cars = [_on_track(rows, cw, at[a], (0.0, 2.0, -3.0)[a % 3], 0.0, tag=f"tile {at[a] % T} pattern {pat}", **_spin(rng)) for a in range(N)]
    elif set_name == "generic":
        t = T_VALUES[int(rng.randint(len(T_VALUES)))]
        cars = []
        for a in range(N):
            i = int(rng.randint(T))
            cars.append(Car(float(rows[i, 2] + rng.uniform(-8, 8)), float(rows[i, 3] + rng.uniform(-8, 8)), float(rng.uniform(-7, 7)), float(rng.normal(0, 10)), float(rng.normal(0, 10)),
                            reward=float(rng.uniform(-200, 1200)), tag="random", **_spin(rng)))
    else:
        raise KeyError(set_name)
    return cars, float(t), touched


def rounds(set_name, N):
    if set_name == "hud":
        return -(-len(REWARDS) // (len(TRACKS) * N))           # every reward on some car
    return 2 if set_name in ("zoom", "crowd", "field") else 1


def realise(L, base_bodies, cars):
    """(bodies [N, 5, 6] f32, wheels [N, 4, 5] f64) of one env's cars: the base car moved rigidly (f64, one rounding), then the hull's
    velocities and the front wheels' angles set"""
    mp = np.zeros(6, f32)
    import ctypes
    L.mcr_mass_props(mp.ctypes.data_as(ctypes.c_void_p))
    lx, ly = float(mp[2]), float(mp[3])
    N = len(cars)
    bodies = np.zeros((N, 5, 6), f32); wheels = np.zeros((N, 4, 5), f64)
    for a, c in enumerate(cars):
        cx = c.x + (math.cos(c.ang) * lx - math.sin(c.ang) * ly); cy = c.y + (math.sin(c.ang) * lx + math.cos(c.ang) * ly)
        b = rigid_teleport(base_bodies[a], cx, cy, c.ang)
        b[0, 3], b[0, 4], b[0, 5] = f32(c.vx), f32(c.vy), f32(c.hw)
        b[1, 2] = f32(b[0, 2] + f32(c.steer)); b[2, 2] = f32(b[0, 2] + f32(c.steer))
        bodies[a] = b
        wheels[a, :, 3] = c.phase; wheels[a, :, 4] = c.omega
    return bodies, wheels


def build(L, trks, N, base_bodies, set_name, rnd):
    """the whole batch of a round: dict(bodies [B, N, 5, 6] f32, wheels [B, N, 4, 5] f64, reward [B, N] f64, t [B] f64, touched [B][T] u8,
    tags [B][N])"""
    B = len(trks)
    out = dict(bodies=np.zeros((B, N, 5, 6), f32), wheels=np.zeros((B, N, 4, 5), f64), reward=np.zeros((B, N), f64), t=np.zeros(B, f64), touched=[], tags=[])
    for e, (name, rows, cw) in enumerate(trks):
        cars, t, touched = env_case(set_name, rnd, e, name, rows, cw, N)
        out["bodies"][e], out["wheels"][e] = realise(L, base_bodies[e], cars)
        out["reward"][e] = [c.reward for c in cars]
        out["t"][e] = t
        out["touched"].append(touched); out["tags"].append([c.tag for c in cars])
    return out


def tile_flags(base_flags, touched):
    """tile_flags [B, TILE_CAP] u16 with bit 8 of every tile as `touched` says, the visited bits as they were"""
    f = np.array(base_flags, np.uint16, copy=True)
    for e, tt in enumerate(touched):
        f[e, :len(tt)] = (f[e, :len(tt)] & np.uint16(0xfeff)) | (tt.astype(np.uint16) << 8)
    return f


def apply_to_oracle(o, case, e, backward=None):
    """one env's state of a built round into its oracle"""
    N = o.N
    for a in range(N):
        for k in range(5):
            o.set_body(a, k, case["bodies"][e, a, k])
        o.set_render_state(a, float(case["bodies"][e, a, 0, 5]), case["bodies"][e, a, 1:, 2], case["wheels"][e, a, :, 4], case["wheels"][e, a, :, 3])
    o.set_time(float(case["t"][e]))
    o.set_reward(case["reward"][e])
    o.set_touched(case["touched"][e])
    if backward is not None:
        o.set_backward(backward)


# ------------------------------------------------------------------------------------------------------------------------------ restatement
RC, QBLK = 168, 16


class Layout:
    """what csrc/k_view.h makes of a view: the visible blocks and cars (lb_finish) and the candidate layout (layout_of), restated in float32
    from the oracle's camera, the cars' hull middles and the block boxes — `slack` pixels added to (> 0) or taken from (< 0) every
    visibility threshold"""

    def __init__(self, cam, h_ratio, boxes, mids, gauge_vals, slack=0.0):
        zoom, angle = cam["zoom"], cam["angle"]
        ftx, fty, fz = f32(cam["tx"]), f32(cam["ty"]), f32(zoom)
        rad = f64(f32(57.29577951308232 * angle)) * (math.pi / 180.0)
        fcs, fsn = f32(math.cos(rad)), f32(math.sin(rad))
        kx, ky = f32(96.0) / f32(1000.0), f32(96.0) / f32(800.0)
        c = [fcs * fz * kx, -fsn * fz * kx, fsn * fz * ky, fcs * fz * ky, ftx * kx, fty * ky]
        inv_z = f32(1.0) / fz
        a, b = f32(1000.0) / f32(96.0), f32(800.0) / f32(96.0)
        v = [fcs * a * inv_z, fsn * b * inv_z, -(fcs * ftx + fsn * fty) * inv_z, -fsn * a * inv_z, fcs * b * inv_z, (fsn * ftx - fcs * fty) * inv_z]
        s = f32(slack)
        self.blocks = []
        mx = abs(v[0]) + abs(v[1]) + f32(0.05) + s * (abs(v[0]) + abs(v[1])); my = abs(v[3]) + abs(v[4]) + f32(0.05) + s * (abs(v[3]) + abs(v[4]))
        corners = [(f32(U), f32(V)) for V in (12.0, 96.0) for U in (0.0, 96.0)]
        wx = [v[0] * U + v[1] * V + v[2] for U, V in corners]; wy = [v[3] * U + v[4] * V + v[5] for U, V in corners]
        for k, bb in enumerate(boxes):
            if not bb[0] <= bb[2]:
                continue
            px = [c[0] * X + c[1] * Y + c[4] for X in (bb[0], bb[2]) for Y in (bb[1], bb[3])]; py = [c[2] * X + c[3] * Y + c[5] for X in (bb[0], bb[2]) for Y in (bb[1], bb[3])]
            if (max(px) >= -1.0 - s and min(px) <= 97.0 + s and max(py) >= 11.0 - s and min(py) <= 97.0 + s and
                    bb[2] >= min(wx) - mx and bb[0] <= max(wx) + mx and bb[3] >= min(wy) - my and bb[1] <= max(wy) + my):
                self.blocks.append(k)
        rx = f32(CAR_RADIUS) * (abs(c[0]) + abs(c[1])) + f32(1.0) + s; ry = f32(CAR_RADIUS) * (abs(c[2]) + abs(c[3])) + f32(1.0) + s
        self.cars = []
        for k, (ax, ay) in enumerate(mids):
            cpx = c[0] * f32(ax) + c[1] * f32(ay) + c[4]; cpy = c[2] * f32(ax) + c[3] * f32(ay) + c[5]
            if -rx <= cpx <= 96.0 + rx and 12.0 - ry <= cpy <= 96.0 + ry:
                self.cars.append(k)
        # the gauges taller than the bar, the grass range, the playfield quad (csrc/k_carview.h)
        hH = 800 / 40.0
        top = max([12.0] + [max(float(f32(f32(hH + hH * val) * ky)), float(f32(f32(hH) * ky))) + 1.0 for val in gauge_vals])
        self.tg = 5 if top > 13.0 else 0
        hk = f32(0.5) / f32(PLAYFIELD / 20.0)
        u = [float((v[0] * hk) * U + (v[1] * hk) * V + v[2] * hk) for U, V in corners]; w = [float((v[3] * hk) * U + (v[4] * hk) * V + v[5] * hk) for U, V in corners]
        mu = float(abs(v[0] * hk) + abs(v[1] * hk)) + 1e-3; mv = float(abs(v[3] * hk) + abs(v[4] * hk)) + 1e-3
        self.inside = min(u) - mu >= -10 and max(u) + mu <= 10 and min(w) - mv >= -10 and max(w) + mv <= 10
        a0, a1 = max(math.ceil(min(u) - mu - 0.5), -10), min(math.floor(max(u) + mu), 9)
        b0, b1 = max(math.ceil(min(w) - mv - 0.5), -10), min(math.floor(max(w) + mv), 9)
        self.G = max(a1 - a0 + 1, 0) * max(b1 - b0 + 1, 0)
        self.pv, self.cs = len(self.blocks) * QBLK, len(self.cars) * 14
        self.f = self.cs + self.tg + (0 if self.inside else 1)
        nspec = (self.f + self.G + 1) & ~1
        self.nround = (self.pv + nspec + RC - 1) // RC
        self.spread = self.pv + self.cs <= 128 and self.f - self.cs + self.G <= RC - 128
        if self.spread:
            self.nround = 1

    def key(self):
        return (tuple(self.blocks), tuple(self.cars))


def block_boxes(quads32):
    """the float32 boxes of the runs of QBLK road_poly entries, as the episode blob holds them"""
    P = len(quads32)
    return [(quads32[b:b + QBLK, :, 0].min(), quads32[b:b + QBLK, :, 1].min(), quads32[b:b + QBLK, :, 0].max(), quads32[b:b + QBLK, :, 1].max()) for b in range(0, P, QBLK)]


def layouts_of(o, quads32, case, e):
    """per view of oracle env `o` (the case applied): (Layout, clear) — clear: the visible blocks and cars are the same with every threshold
    half a pixel further out and half a pixel further in"""
    boxes = block_boxes(quads32)
    out = []
    mids = None
    for a in range(o.N):
        cam, prims = o.render_stream(a)
        if mids is None:
            mids = []
            for c in range(o.N):
                hull = [xy for space, tag, xy, _ in prims if tag == 1 + c and len(xy) == 8]
                assert len(hull) == 1, f"car {c}: {len(hull)} 8-gons in the render stream"
                mids.append((0.5 * (hull[0][0, 0] + hull[0][4, 0]), 0.5 * (hull[0][0, 1] + hull[0][4, 1])))
        b = case["bodies"][e, a, 0]
        speed = math.sqrt(float(b[3]) ** 2 + float(b[4]) ** 2)
        vals = [0.02 * speed] + [0.01 * w for w in case["wheels"][e, a, :, 4]]
        L0, Lo, Li = (Layout(cam, 0.25, boxes, mids, vals, s) for s in (0.0, 0.5, -0.5))
        out.append((L0, Lo.key() == Li.key() == L0.key()))
    return out


# ------------------------------------------------------------------------------------------------------------------------------ oracles
def blobs_of(trks, N):
    from multi_car_racing_amd import levels
    return np.concatenate([levels.from_tracks([rows], N, "CW" if cw else "CCW") for _, rows, cw in trks])


def make_oracles(lib, O, trks, N, blobs=None):
    """(oracles, episodes, base bodies [B, N, 5, 6]): env e's oracle on the device's own blob of track e, its cars created and never stepped
    — their bodies are the base car every case moves about, on the device too"""
    blobs = blobs_of(trks, N) if blobs is None else blobs
    orcs, eps = [], []
    for e in range(len(trks)):
        ep = episode_of(lib, O, blobs[e], N)
        o = O.OracleEnv(N, use_ego_color=N in EGO_COLOR_NS)
        o.reset_nostep(ep)
        orcs.append(o); eps.append(ep)
    return orcs, eps, np.stack([o.state()["bodies"] for o in orcs])
