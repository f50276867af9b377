"""Synthetic tracks and scripted scenes for the wheel<->tile sensor pass (a helper, not a test): csrc/k_collide.h's block culling, candidate list,
overlap items, per-tile begin / end state, begin-event queue and its replay in Box2D's order, driven on what no rollout on a generated track
reaches.  tests/test_tile_cases.py holds every scene to the counts it is named for on the oracle alone; tests/test_gpu_tile_kernel.py runs
the scenes on the device in lockstep with the oracle.

Tracks (tests/obs_cases.circle; a generated track's tiles are 3.5 apart, a car's box then meets about 3 tiles and a pass holds at most ~35 begin
events): circles of 512 and 256 tiles 0.5 apart (a car's wheels rest on ~13 tiles), 512 tiles 0.25 apart (~23 tiles; the reset pass of 8 cars
alone holds 185 begin events), 512 tiles 0.44 apart (STEP_USED: why), 65 and 449 tiles 3.5 apart (a last block of one tile), 512 tiles 3.5 apart (block 31), one generated lap; the
steps are the issue's — mcr_episode_from_track took every one of them as it stands, none had to be widened (STEP_USED).

A scene is one env's script.  All scenes of a group (one N, car<->car contacts on or off: one handle) run side by side on one schedule of
STEPS steps:
  step 0        every car is moved rigidly onto the grass (park_pose) — the pass sees the spawn tiles through touch_blocks alone, end events only
  step 1        the scene's placement: car c at scene["place"][c] = (x, y, heading, speed) — the pass whose counts the scene is named for
  steps 2 ..    the scene's actions
  step LEAVE    onto the grass again (the blocks the cars stood on are visited through touch_blocks alone), one idle step behind it
A teleport is handle-wide (mcr_set_bodies re-creates every car proxy of every env; the oracle's set_body does the same per env), so the
schedule is the group's, not the scene's.  The group is played three times on one handle — reset, schedule, reset, schedule, reset, schedule —
with level_order="cycle": env e plays scene (e + k) % B in its k-th episode, on the world its earlier episodes left behind (proxy ids off the
tree's free list; the car fixture may hold the lower id and b2TestOverlap's arguments flip).

The poses of the scenes named `exact128` / `over129` were found by search_counts below (seeded; python -m tests.tile_cases prints them)."""
import math

import numpy as np

from tests import obs_cases as C
from tests import range_obs_ref
from tests.util import hull_positions

f64 = np.float64
TBLK, TILE_CAP = 16, 512             # csrc/mcr_common.h: MCR_TBLK, MCR_TILE_CAP
CAND_CAP, EVQ_CAP = 128, 128         # csrc/k_collide.h
MCR_CC_MAX = 24                      # csrc/mcr_kernels.h: manifold records per env
STEPS, PLACE, LEAVE = 24, 1, 22      # the group schedule
EPISODES = 3
NS = (1, 2, 3, 5, 8)
WHEEL_HALF = (14 * 0.02, 27 * 0.02)  # gym car_dynamics: WHEEL_W, WHEEL_R times SIZE
# (tiles, spacing) the issue names, and the spacing used (mcr_episode_from_track refused none)
STEP_USED = {"d512": (512, 0.5), "d256": (256, 0.5), "q512": (512, 0.25), "c65": (65, 3.5), "c449": (449, 3.5), "c512": (512, 3.5),
             # one more than the issue lists: two mid-loop flushes (280 box hits) BELOW the event cap need eight cars — 51 hits a car is the most a
             # circle of 512 tiles gives, on q512 — and q512's reset pass at N = 8 is itself beyond the cap (185); at 0.5 eight cars reach 264 hits.
             # 0.44 (scanned 0.34 .. 0.44 in steps of 0.02): 296 hits, 116 begin events in the placement pass and in the reset pass
             "e512": (512, 0.44)}


def generated_lap(lib, seed=91):
    from multi_car_racing_amd import levels
    blobs, _ = levels.make_levels(1, 1, seed, direction_mode=0, threads=1)
    ep = lib.unpack_episode(np.ascontiguousarray(blobs[0]))
    return np.ascontiguousarray(np.stack([ep["alpha"], ep["track"][:, 2], ep["track"][:, 0], ep["track"][:, 1]], axis=1), f64)


_tracks = {}


def track(lib, name):
    if name not in _tracks:
        _tracks[name] = generated_lap(lib) if name == "lap" else C.circle(*STEP_USED[name])
    return _tracks[name]


# ------------------------------------------------------------------------------------------------------------------------------ poses
def on_tile(rows, cw, i, lat=0.0, lon=0.0, dh=0.0, speed=0.0):
    """(x, y, heading, speed): `lon` ahead of track point i along the direction of travel, `lat` to the right of it, heading turned by dh"""
    i %= len(rows)
    h = rows[i, 1] - (math.pi if cw else 0.0)
    fx, fy, rx, ry = -math.sin(h), math.cos(h), math.cos(h), math.sin(h)
    return (rows[i, 2] + fx * lon + rx * lat, rows[i, 3] + fy * lon + ry * lat, h + dh, speed)


def park_pose(rows, name, c):
    """car c's place on the grass: inside a circle round its centre (two rows of four, 4 apart: the hulls 2.4 wide do not touch), beside a
    generated lap 30 beyond its easternmost point"""
    if name == "lap":
        return (float(rows[:, 2].max()) + 30.0 + 4.0 * c, float(rows[:, 3].mean()), 0.0, 0.0)
    return (4.0 * (c % 4 - 1.5), 7.0 * (c // 4) - 3.5, 0.0, 0.0)


WHEELPOS = ((-55, 80), (55, 80), (-55, -82), (55, -82))          # gym car_dynamics, times SIZE = 0.02: the wheels' body origins in the hull's frame
_lc = None


def car_at(lib, x, y, h, v):
    """[5, 6] f32: a car as Car.__init__ builds it — the hull's centre of mass at (x, y), heading h, the wheels on their anchors at the hull's
    angle — every body at the velocity v * (the forward axis), no spin.  Not a function of the bodies it replaces: what the reset pass of an
    earlier episode did to the cars (on the dense tracks the grid's cars overlap at spawn) does not reach the scene."""
    global _lc
    if _lc is None:
        import ctypes
        mp = np.zeros(6, np.float32)
        lib.load().mcr_mass_props(mp.ctypes.data_as(ctypes.c_void_p))
        _lc = (float(mp[2]), float(mp[3]))
    s, c = math.sin(h), math.cos(h)
    px, py = x - (c * _lc[0] - s * _lc[1]), y - (s * _lc[0] + c * _lc[1])          # the hull's body origin
    out = np.zeros((5, 6), f64)
    out[0, :3] = (x, y, h)
    for k, (wx, wy) in enumerate(WHEELPOS, start=1):
        wx, wy = wx * 0.02, wy * 0.02
        out[k, :3] = (px + c * wx - s * wy, py + s * wx + c * wy, h)
    out[:, 3] = -s * v; out[:, 4] = c * v
    return out.astype(np.float32)


def teleport(lib, bodies, poses):
    """bodies [N, 5, 6] f32, poses {car: (x, y, heading, speed)} -> the bodies with those cars replaced by car_at(pose)"""
    out = np.array(bodies, np.float32, copy=True)
    for c, pose in poses.items():
        out[c] = car_at(lib, *pose)
    return out


# ------------------------------------------------------------------------------------------------------------------------------ restatements
def tile_boxes(lib, blob):
    """[T, 4] f64 lo.xy hi.xy: the boxes of the tiles' float32 vertices as the episode blob holds them (what MCR_OFF_TAABB is made of)"""
    ep = lib.unpack_episode(np.ascontiguousarray(blob))
    q = ep["quads"][((ep["quad_meta"] >> 8) & 0x3ff) != 0].astype(f64)
    assert len(q) == ep["T"]
    return np.concatenate([q.min(axis=1), q.max(axis=1)], axis=1)


def block_boxes(tb):
    """[ceil(T / 16), 4] f64: the boxes of the runs of MCR_TBLK tile boxes (MCR_OFF_TBLK)"""
    nb = (len(tb) + TBLK - 1) // TBLK
    return np.array([np.concatenate([tb[b * TBLK:(b + 1) * TBLK, :2].min(axis=0), tb[b * TBLK:(b + 1) * TBLK, 2:].max(axis=0)]) for b in range(nb)])


_hull = None


def fixture_vertices(L, bodies):
    """world vertices of one env's car fixtures in f64: (hull [N, 20, 2] — the four hull polygons —, wheels [N, 16, 2])"""
    global _hull
    if _hull is None:
        _hull = np.concatenate(range_obs_ref.hull_polygons()).astype(f64)
    b = np.asarray(bodies, np.float32)
    p = hull_positions(L, b).astype(f64)
    hull, wheels = [], []
    hw, hr = WHEEL_HALF
    box = np.array([(-hw, -hr), (hw, -hr), (hw, hr), (-hw, hr)], f64)
    for c in range(len(b)):
        a = f64(b[c, 0, 2]); s, co = math.sin(a), math.cos(a)
        hull.append(np.stack([p[c, 0] + co * _hull[:, 0] - s * _hull[:, 1], p[c, 1] + s * _hull[:, 0] + co * _hull[:, 1]], axis=1))
        ws = []
        for k in range(1, 5):
            a = f64(b[c, k, 2]); s, co = math.sin(a), math.cos(a)
            ws.append(np.stack([f64(b[c, k, 0]) + co * box[:, 0] - s * box[:, 1], f64(b[c, k, 1]) + s * box[:, 0] + co * box[:, 1]], axis=1))
        wheels.append(np.concatenate(ws))
    return np.stack(hull), np.stack(wheels)


def _meets(a, b):
    """boxes a [n, 4] against boxes b [m, 4] -> [n, m] bool: the test of k_collide.h's `hit` / `near`"""
    return ~((a[:, None, 0] > b[None, :, 2]) | (a[:, None, 2] < b[None, :, 0]) | (a[:, None, 1] > b[None, :, 3]) | (a[:, None, 3] < b[None, :, 1]))


def pass_counts(L, tb, bb, bodies, touch_before, fresh):
    """What a pass at `bodies` has to go through, restated in f64: dict(candidates = (tile, car) pairs whose boxes meet — the car's box being
    that of all its fixtures' vertices -+ 0.05 —, blocks = the visited blocks (a car's box meets the block's, or a tile of it held a wheel after
    the pass before: touch_before [T] u32; `fresh` — every proxy was re-created — also: the box of the wheels' vertices -+ 0.11, their new fat
    AABBs, comes within 0.12 of the block's), near = those a car's box meets, margin_only = those visited through that last clause alone)"""
    hull, wheels = fixture_vertices(L, bodies)
    allv = np.concatenate([hull, wheels], axis=1)
    cbox = np.concatenate([allv.min(axis=1) - 0.05, allv.max(axis=1) + 0.05], axis=1)
    near = _meets(bb, cbox).any(axis=1)
    touched = np.zeros(len(bb), bool)
    for b in range(len(bb)):
        touched[b] = bool(np.any(touch_before[b * TBLK:(b + 1) * TBLK]))
    margin = np.zeros(len(bb), bool)
    if fresh:
        cfat = np.concatenate([wheels.min(axis=1) - 0.11, wheels.max(axis=1) + 0.11], axis=1)
        wide = bb + np.array([-0.12, -0.12, 0.12, 0.12])
        margin = _meets(wide, cfat).any(axis=1)
    return dict(candidates=int(_meets(tb, cbox).sum()), blocks=np.nonzero(near | touched | margin)[0].tolist(), near=np.nonzero(near)[0].tolist(),
                margin_only=np.nonzero(margin & ~near & ~touched)[0].tolist())


# ------------------------------------------------------------------------------------------------------------------------------ scenes
def scene(name, N, track_name, cw, contacts, place, gas=0.0, steer=0.0, streams2=False, **want):
    """place: [(x, y, heading, speed)] per car — or a function (rows, cw) -> that list; gas / steer: a number or one per car, held from step 2
    to LEAVE - 1.  want: the conditions tests/test_tile_cases.py holds the scene to —
      events=(lo, hi)     begin events of the placement pass
      candidates=lo       (tile, car) box hits of the placement pass, at least
      blocks=lo           visited blocks of the placement pass, at least
      has_blocks=(..)     blocks that some pass of the scene visits
      past=True           the largest `past` of the scene is N - 1
      order=n             steps whose rewards differ between Box2D's event order and the (tile, car, wheel) order, at least
      stamp=n             ... and between Box2D's order and its order with every contact in one batch, at least
      margin=True         the placement pass visits a block through the moved-proxy margin alone
      max_events=hi       no pass of the scene holds more begin events (default EVQ_CAP: the scene stays below the cap)"""
    return dict(name=name, N=N, track=track_name, cw=cw, contacts=contacts, place=place, gas=gas, steer=steer, streams2=streams2, want=want)


def stacked(N, track_name, cw, i, speed, gas=0.5, **kw):
    return scene(f"stacked-{track_name}{'-cw' if cw else ''}", N, track_name, cw, False, lambda rows, cw_: [on_tile(rows, cw_, i, speed=speed)] * N,
                 gas=gas, past=True, **kw)


def spread(rows, cw, tiles, speed=0.0, lat=0.0, dh=0.0):
    pick = lambda v, c: v[c] if isinstance(v, (list, tuple)) else v
    return [on_tile(rows, cw, t, lat=pick(lat, c), dh=pick(dh, c), speed=pick(speed, c)) for c, t in enumerate(tiles)]


# search_counts' results: (lat, lon, dh) per car of an N = 5 scene on q512, the cars on track points 40, 110, 180, 250, 320
EXACT128 = [(-2.096, 0.047, 0.053), (-1.81, 0.052, -0.224), (-1.57, 0.005, -0.292), (-1.667, 0.19, -0.482), (-1.316, -0.057, -0.317)]
OVER129 = [(-2.765, -0.109, -0.532), (-1.223, -0.191, -0.255), (-0.514, -0.218, 0.269), (0.4, -0.117, 0.033), (-2.436, 0.038, 0.601)]
SEARCH_TILES = [40 + 70 * c for c in range(5)]
# two cars side by side at each of a 512-tile circle's four diagonals, where a tile's box is 9.4 wide and meets a car's box from 18 tiles away
DIAGONALS = (64, 64, 192, 192, 320, 320, 448, 448)

FIVE_BLOCKS = (8, 100, 200, 300, 400, 505, 250, 350)
# beside c512's track point 0 the road's edge x = r + W is the east side of block 0's box (block 31's lies 0.02 inside it); a car parallel to it
# whose wheels' outer vertices (1.1 + 0.28 from its axis) are 0.15 from that side: beyond the car box's 0.05, within the fat AABBs' 0.11 + 0.12
MARGIN_LAT = float(C.W) + 1.1 + WHEEL_HALF[0] + 0.15


def scenes_for(N):
    """the scenes of one N, contact-free ones first"""
    out = [stacked(N, "d512", False, 100, 10.0, streams2=True, events=(13 * N - 2 * N, 13 * N + 3 * N)),
           stacked(N, "d256", True, 3, 15.0, has_blocks=(0, 15)),                                       # across the seam against the indices
           stacked(N, "lap", False, 30, 20.0, streams2=True),
           stacked(N, "c65", False, 63, 30.0, has_blocks=(3, 4, 0)),                                    # tile 64: a last block of one tile, then the seam
           stacked(N, "c65", True, 2, 30.0, has_blocks=(0, 4)),
           stacked(N, "c449", False, 446, 30.0, has_blocks=(27, 28, 0)),
           stacked(N, "c512", False, 508, 30.0, has_blocks=(31, 0)),                                    # block 31 and bit 31 of the masks
           stacked(N, "d512", True, 510, 12.0, has_blocks=(31, 0))]
    if N >= 2:
        # side by side across the road (13.3 wide), front axles level, different speeds: the wheels' fat AABBs reach a tile in different passes
        lats = [(-4.5, 4.5), (-4.5, 0.0, 4.5), None, (-5.2, -2.6, 0.0, 2.6, 5.2)][min(N, 5) - 2] if N <= 5 else tuple(-5.25 + 1.5 * c for c in range(8))
        speeds = [10.0 + (0.6 if N == 2 else 3.0) * ((5 * c) % N) for c in range(N)]
        out.append(scene("staggered", N, "d512", False, N <= 3, lambda rows, cw_: [on_tile(rows, cw_, 60, lat=lats[c], speed=speeds[c]) for c in range(N)],
                         gas=[0.2 + 0.1 * c for c in range(N)], streams2=True, order=3, stamp=1 if N >= 3 else 0))
        out.append(scene("side-approach", N, "c512", False, True,
                         lambda rows, cw_: [on_tile(rows, cw_, 0, lat=MARGIN_LAT, lon=6.0 * c) for c in range(N)],
                         gas=0.6, steer=-0.5, margin=True))
    if N >= 3:
        out.append(scene("on-road-q512", N, "q512", False, True, lambda rows, cw_: spread(rows, cw_, [40 + 70 * c for c in range(N)][:N]),
                         streams2=True, events=(65, 127) if 3 <= N <= 5 else (180, 400), candidates=150,
                         max_events=EVQ_CAP if N <= 5 else 400))
    if N >= 5:
        out.append(scene("five-blocks", N, "c512", False, True, lambda rows, cw_: spread(rows, cw_, FIVE_BLOCKS[:N], speed=15.0), gas=0.4, blocks=5,
                         has_blocks=(31,)))
    if N == 8:
        # cars spread over a quarter of d512, the tiles' boxes growing towards the diagonal: more than CAND_CAP box hits, fewer than twice as many
        out.append(scene("one-flush", N, "d512", False, True, lambda rows, cw_: spread(rows, cw_, [44 + 22 * c for c in range(N)]), streams2=True,
                         candidates=150, events=(65, 127)))
    if N == 5:
        for name, sh, ev in (("exact128", EXACT128, (128, 128)), ("over129", OVER129, (129, 129))):
            out.append(scene(name, N, "q512", False, True,
                             lambda rows, cw_, sh=sh: [on_tile(rows, cw_, SEARCH_TILES[c], lat=sh[c][0], lon=sh[c][1], dh=sh[c][2]) for c in range(5)],
                             streams2=True, events=ev, candidates=150, max_events=ev[1]))
    if N == 8:
        out.append(scene("two-flushes", N, "e512", False, True, lambda rows, cw_: spread(rows, cw_, DIAGONALS, lat=[-3.0, 3.0] * 4), streams2=True, candidates=280, events=(65, 127)))
    return out


def groups():
    """{(N, contacts): [scene]} — one handle each, at most 16 envs"""
    out = {}
    for N in NS:
        for sc in scenes_for(N):
            out.setdefault((N, sc["contacts"] and N > 1), []).append(sc)
    assert all(len(v) <= 16 for v in out.values())
    return out


def placements(lib, sc):
    rows = track(lib, sc["track"])
    p = sc["place"](rows, sc["cw"]) if callable(sc["place"]) else sc["place"]
    assert len(p) == sc["N"]
    return list(p)


def actions(sc, k):
    """[N, 3] f32 of step k of the schedule"""
    a = np.zeros((sc["N"], 3), np.float32)
    if 2 <= k < LEAVE:
        a[:, 0] = np.asarray(sc["steer"], np.float32); a[:, 1] = np.asarray(sc["gas"], np.float32)
    return a


def teleports(lib, sc, k):
    """{car: pose} of step k of the schedule, or None"""
    rows = track(lib, sc["track"])
    if k in (0, LEAVE):
        return {c: park_pose(rows, sc["track"], c) for c in range(sc["N"])}
    if k == PLACE:
        return dict(enumerate(placements(lib, sc)))
    return None


# ------------------------------------------------------------------------------------------------------------------------------ the oracle's side
def episode_of(O, lib, sc):
    """the oracle's episode of the scene's track: the tiles and spawn poses levels.from_tracks gives the device (tests/obs_cases.py: oracle_warmup)"""
    rows = track(lib, sc["track"]); cw = sc["cw"]; N = sc["N"]; T = len(rows); W = C.W
    c, s = np.array([math.cos(b) for b in rows[:, 1]]), np.array([math.sin(b) for b in rows[:, 1]])
    x, y = rows[:, 2], rows[:, 3]
    j = (np.arange(T) - 1) % T
    poly = np.stack([np.stack([x - W * c, y - W * s], 1), np.stack([x + W * c, y + W * s], 1),
                     np.stack([x[j] + W * c[j], y[j] + W * s[j]], 1), np.stack([x[j] - W * c[j], y[j] - W * s[j]], 1)], 1)
    return dict(track=rows, poly=poly, color=np.full((T, 3), 0.4), tile_of_quad=np.arange(T, dtype=np.int32), direction="CW" if cw else "CCW",
                car_order=list(range(N)), poses=O.spawn_poses(rows, list(range(N)), cw))


def blobs_of(lib, group):
    from multi_car_racing_amd import levels
    return np.concatenate([levels.from_tracks([track(lib, sc["track"])], sc["N"], "CW" if sc["cw"] else "CCW") for sc in group])


def set_oracle_bodies(o, bodies):
    for c in range(len(bodies)):
        for k in range(5):
            o.set_body(c, k, bodies[c, k])


class Twin:
    """One env's oracle through the episodes of a group: ONE world; `order`: OracleEnv.set_event_order"""

    def __init__(self, O, lib, group, e, order=0):
        self.O, self.lib, self.group, self.e = O, lib, group, e
        N = group[0]["N"]
        self.o = O.OracleEnv(N, car_contacts=group[0]["contacts"] and N > 1)
        self.o.set_contact_cap(MCR_CC_MAX)       # (on the dense tracks the grid's cars overlap at spawn: the product's manifold store and its drop rule)
        self.o.set_event_order(order)
        self.k = -1

    def reset(self):
        """the env's next episode -> its scene"""
        self.k += 1
        self.sc = self.group[(self.e + self.k) % len(self.group)]
        self.o.reset(episode_of(self.O, self.lib, self.sc), render=False)
        return self.sc

    def close(self):
        self.o.close()


def run_oracle(O, lib, group, e, episodes=EPISODES, order=0, each_pass=None):
    """env e of the group on the oracle alone: [per episode dict(scene, reset_events, fixture_first = (wheel, tile) pairs in which the wheel's proxy
    holds the lower id, reset_manifolds = touching car<->car pairs the reset pass stored (the grid's cars overlap on the dense tracks), steps=[dict(events, past, reward [N], done, touch [T],
    bodies [N, 5, 6] the step was entered with, fresh)])]"""
    tw = Twin(O, lib, group, e, order)
    out = []
    try:
        for _ in range(episodes):
            sc = tw.reset()
            tid, fid = tw.o.proxy_ids()
            ep = dict(scene=sc, reset_events=tw.o.begin_events()[0], steps=[], fixture_first=int((fid[:, 4:, None] < tid[None, None, :]).sum()),
                      reset_manifolds=tw.o.num_car_contacts() if sc["contacts"] and sc["N"] > 1 else 0)
            for k in range(STEPS):
                tp = teleports(lib, sc, k)
                fresh = k in (0, PLACE, LEAVE)
                touch_before = tw.o.wheel_touch()
                if fresh:                    # (the group's schedule: every env's cars are set again, moved or not)
                    b = tw.o.state()["bodies"] if tp is None else teleport(lib, tw.o.state()["bodies"], tp)
                    set_oracle_bodies(tw.o, b)
                entered = tw.o.state()["bodies"]
                _, r, d, _ = tw.o.step(actions(sc, k), render=False)
                ev, past = tw.o.begin_events()
                ep["steps"].append(dict(events=ev, past=past, reward=r.copy(), done=d, touch=tw.o.wheel_touch(), touch_before=touch_before,
                                        bodies=entered, fresh=fresh))
            out.append(ep)
    finally:
        tw.close()
    return out


# ------------------------------------------------------------------------------------------------------------------------------ the search
def search_counts(O, lib, wanted=(128, 129), trials=400):
    """{count: [(lat, lon, dh)] * 5}: five cars on q512's track points 40, 110, .., each shifted and turned a little (RandomState(0)), whose
    placement pass from the grass holds exactly `count` begin events"""
    rng = np.random.RandomState(0); found = {}
    for _ in range(trials):
        sh = [(round(rng.uniform(-3, 3), 3), round(rng.uniform(-0.25, 0.25), 3), round(rng.uniform(-0.7, 0.7), 3)) for _ in range(5)]
        sc = scene("probe", 5, "q512", False, True, lambda rows, cw_, sh=sh: [on_tile(rows, cw_, SEARCH_TILES[c], lat=sh[c][0], lon=sh[c][1], dh=sh[c][2]) for c in range(5)])
        tw = Twin(O, lib, [sc], 0); tw.reset()
        try:
            for k in (0, PLACE):
                set_oracle_bodies(tw.o, teleport(lib, tw.o.state()["bodies"], teleports(lib, sc, k)))
                tw.o.step(actions(sc, k), render=False)
            n = tw.o.begin_events()[0]
        finally:
            tw.close()
        if n in wanted and n not in found:
            found[n] = sh
        if len(found) == len(wanted):
            break
    return found


if __name__ == "__main__":
    from multi_car_racing_amd import _lib as _L
    from oracle import oracle as _O
    print(search_counts(_O, _L))
