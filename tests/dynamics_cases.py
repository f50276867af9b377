"""Scenes for the per-car dynamics (csrc/k_dynamics.h): synthetic states on ordinary episodes — env e of a batch plays the episode of SEED + e,
cars as spawned (tests/util.py: oracles / make_env) — made by three means that exist alike on the device and on the oracle: teleports of single
bodies (set_bodies <-> orc_set_body), wheel state (set_wheels <-> orc_set_wheels) and scripted actions.  A scene is a dict

    name, N, edits {step: [edit, ...]}, script [(first step, [car][steer, gas, brake])], steps, pins {(step, car): (sweeps, solved, fixed_at)}

and `Run` plays a list of scenes, env e playing scenes[e], on per-env oracles and, when given, on a VecMultiCarRacing in lockstep.  What a
scene reaches is read from the oracle (OracleEnv.dynamics_coverage); tests/test_dynamics_cases.py holds every scene to what it is pinned to,
without a device, and tests/test_gpu_dynamics_kernel.py compares the kernel with the oracle on them, bit for bit.

Three families:
  * POSITION: the position loop beyond one sweep — every count the main launch's grant (MCR_DEFER_AFTER = 3 sweeps), its probing sweeps
    ((it & 3) == 2: sweeps 3, 7, 11, ...) and the resume launch (it0 = 3 or 60) tell apart.  Found by `search_counts` / `find_pins`, pinned below.
  * wavefront compositions (`composition`): which lanes of which wavefront enter the velocity sweeps with a joint at its limit — the three
    wave-uniform forms of the sweeps are chosen by a ballot over those.
  * TYRE and SLEEP: the branches of the f64 tyre model, the clamps of the integration and the sleep rule.
"""
import numpy as np

from tests.util import oracle_episode

F = np.float32
SEED = 700
DEFER_AFTER = 3                                     # csrc/mcr_common.h: MCR_DEFER_AFTER, the sweeps the main launch grants before it parks an env
CONFIGS = {1: (1, 130), 2: (2, 65), 3: (4, 33), 5: (8, 17), 8: (8, 17)}      # N -> (G lanes per env, B): two full wavefronts and a partial one
LIMIT = F(0.4)                                      # the wheel joints' limits are +-0.4 rad
TRACK_WIDTH = 40 / 6.0


def lanes(N):
    """(envs per wavefront, number of wavefronts): the main launch's work slot is the env index, wavefront w holds envs [w * E, (w + 1) * E)"""
    G, B = CONFIGS[N]
    E = 64 // G
    return E, (B + E - 1) // E


# ----------------------------------------------------------------------------------------------------------------- edits
# An edit is a tuple (kind, car, ...) applied to one env's bodies [N, 5, 6] f32 (hull, four wheels; cx cy a vx vy w) and wheels [N, 4, 5] f64
# (gas brake steer phase omega).  Wheels are numbered 1..4 like the bodies (1, 2 front, steered; 3, 4 rear).
def wheel_angle_for(ah, which):
    """the wheel body angle next to a joint limit, for hull angle ah (f32).  The joint angle the solver sees is f32(aw - ah):
    "at+": the smallest aw with f32(aw - ah) >= 0.4f (the upper limit holds), "in+": its f32 neighbour below (the largest aw that is inside);
    "at-" / "in-": the same at the lower limit"""
    ah = F(ah); sgn = F(1 if which[-1] == "+" else -1)
    outward = F(sgn * np.inf)
    inside = lambda x: abs(F(F(x) - ah)) < LIMIT
    aw = F(ah + sgn * LIMIT)
    while inside(aw):
        aw = np.nextafter(aw, outward)
    while not inside(np.nextafter(aw, -outward)):
        aw = np.nextafter(aw, -outward)
    return F(aw) if which.startswith("at") else F(np.nextafter(aw, -outward))


def nearest_point(ep, x, y):
    tr = ep["track"]
    return int(np.argmin((tr[:, 2] - x) ** 2 + (tr[:, 3] - y) ** 2))


def apply_edits(b, w, ep, edits):
    """-> (bodies, wheels) of one env after `edits`:
    ("angle", car, wheel, offset, spin)    wheel angle = f32(hull angle + f32(offset)), the wheel body's angular velocity = spin
    ("joint", car, wheel, which, spin)     wheel angle = wheel_angle_for(hull angle, which)
    ("shift", car, wheel, dx, dy)          the wheel body displaced from its anchor
    ("hullspin", car, w)                   the hull's angular velocity
    ("omega", car, [4])                    the tyres' omega (phase 0)
    ("behind", car, front, gap)            the car rigidly `gap` metres behind car `front`, same heading, at rest (4.9: the hulls overlap a little)
    ("rest", car)                          all five bodies at rest
    ("hullvel", car, forward)              the hull alone at that speed along its forward axis
    ("vel", car, forward, sideways)        all five bodies at that velocity along the hull's axes (m/s)
    ("lateral", car, d)                    the car moved rigidly by d metres AWAY from the centre line, across its heading
    ("split", car)                         ... so that its hull sits on the road's edge: the wheels of one side on the road, the others on the grass"""
    b = b.copy(); w = w.copy()
    for ed in edits:
        kind, c = ed[0], ed[1]
        if kind == "angle":
            b[c, ed[2], 2] = F(b[c, 0, 2] + F(ed[3])); b[c, ed[2], 5] = F(ed[4])
        elif kind == "joint":
            b[c, ed[2], 2] = wheel_angle_for(b[c, 0, 2], ed[3]); b[c, ed[2], 5] = F(ed[4])
        elif kind == "shift":
            b[c, ed[2], 0] = F(b[c, ed[2], 0] + F(ed[3])); b[c, ed[2], 1] = F(b[c, ed[2], 1] + F(ed[4]))
        elif kind == "hullspin":
            b[c, 0, 5] = F(ed[2])
        elif kind == "omega":
            w[c, :, 4] = np.asarray(ed[2], np.float64); w[c, :, 3] = 0.0
        elif kind == "behind":
            from tests.util import rigid_teleport
            a = float(b[ed[2], 0, 2])
            b[c] = rigid_teleport(b[c], float(b[ed[2], 0, 0]) + np.sin(a) * ed[3], float(b[ed[2], 0, 1]) - np.cos(a) * ed[3], a)
        elif kind == "rest":
            b[c, :, 3:] = F(0.0)
        elif kind == "hullvel":
            a = float(b[c, 0, 2]); b[c, 0, 3] = F(-np.sin(a) * ed[2]); b[c, 0, 4] = F(np.cos(a) * ed[2])
        elif kind == "vel":
            a = float(b[c, 0, 2])
            b[c, :, 3] = F(-np.sin(a) * ed[2] + np.cos(a) * ed[3]); b[c, :, 4] = F(np.cos(a) * ed[2] + np.sin(a) * ed[3])
        elif kind in ("lateral", "split"):
            a = float(b[c, 0, 2]); side = np.array([np.cos(a), np.sin(a)])
            j = nearest_point(ep, float(b[c, 0, 0]), float(b[c, 0, 1]))
            lat = float(np.dot(np.array([b[c, 0, 0], b[c, 0, 1]], np.float64) - ep["track"][j, 2:4], side))
            out = 1.0 if lat >= 0 else -1.0
            d = ed[2] if kind == "lateral" else TRACK_WIDTH - abs(lat)
            b[c, :, 0] = b[c, :, 0] + F(out * d * side[0]); b[c, :, 1] = b[c, :, 1] + F(out * d * side[1])
        else:
            raise ValueError(kind)
    return b, w


def scene(name, N, edits=None, script=None, steps=4, pins=None, **want):
    """script: [(first step, rows)] — rows [steer, gas, brake] for every car, or one row per car; the last entry at or before a step holds"""
    return dict(name=name, N=N, edits=edits or {}, script=script or [(0, [0.0, 0.0, 0.0])], steps=steps, pins=pins or {}, want=want)


def action_of(sc, k):
    rows = [r for k0, r in sc["script"] if k0 <= k][-1]
    a = np.zeros((sc["N"], 3), np.float32)
    a[:] = np.asarray(rows, np.float32)
    return a


class Run:
    """env e plays scenes[e] on its own oracle (and on env e of `env`, in lockstep).  An edit step is a teleport of the whole batch: every
    body of every env is set (each env's proxies are re-created, as the handle-wide mcr_set_bodies does) and every wheel's omega and phase."""

    def __init__(self, O, scenes, contacts=False, env=None, seed=SEED):
        self.N = scenes[0]["N"]; self.scenes = scenes; self.env = env
        self.eps = [oracle_episode(O, self.N, seed, e) for e in range(len(scenes))]
        self.orcs = []
        for ep in self.eps:
            o = O.OracleEnv(self.N, car_contacts=contacts); o.reset(ep, render=False); self.orcs.append(o)
            o.dynamics_coverage(reset=True)                                  # (the totals count from here: not reset()'s own step)
        self.k = 0
        self.steps = max(sc["steps"] for sc in scenes)

    def close(self):
        for o in self.orcs:
            o.close()

    def teleport(self, edits):
        """edits[e]: env e's list of edits (may be empty)"""
        bodies, wheels = [], []
        for e, o in enumerate(self.orcs):
            st = o.state()
            b, w = apply_edits(st["bodies"], st["wheels"], self.eps[e], edits[e])
            for c in range(self.N):
                for k in range(5):
                    o.set_body(c, k, b[c, k])
                o.set_wheels(c, w[c, :, 4], w[c, :, 3])
            bodies.append(b); wheels.append(w)
        if self.env is not None:
            self.env.set_bodies(np.stack(bodies)); self.env.set_wheels(np.stack(wheels))

    def step(self, actions=None, render=False):
        """the scenes' edits of this step, then one step.  -> (oracle rewards [B, N], oracle dones [B], env.step's result or None, actions)"""
        k = self.k
        edits = [sc["edits"].get(k, []) for sc in self.scenes]
        if any(edits):
            self.teleport(edits)
        a = np.stack([action_of(sc, k) for sc in self.scenes]) if actions is None else np.ascontiguousarray(actions, np.float32)
        if actions is None:
            for e, sc in enumerate(self.scenes):                             # steer exactly onto a joint's angle: Car.steer stores -action
                if "steer_to_joint" in sc["want"]:
                    c, wheel = sc["want"]["steer_to_joint"]; b = self.orcs[e].state()["bodies"]
                    a[e, c, 0] = -F(b[c, wheel, 2] - b[c, 0, 2])
        got = None
        if self.env is not None:
            import torch
            got = self.env.step(torch.from_numpy(a).to(self.env.device))
        rew = np.zeros((len(self.orcs), self.N)); done = np.zeros(len(self.orcs), bool)
        for e, o in enumerate(self.orcs):
            _, rew[e], done[e], _ = o.step(a[e], render=render)
        self.k += 1
        return rew, done, got, a

    def coverage(self):
        """[B] of the oracles' last-step coverage dicts (row -> [N])"""
        return [o.dynamics_coverage()[0] for o in self.orcs]

    def totals(self):
        return [o.dynamics_coverage()[1] for o in self.orcs]


def outcome(cov, car):
    """(sweeps, solved, fixed_at) of a car from a last-step coverage dict"""
    return int(cov["sweeps"][car]), int(cov["solved"][car]), int(cov["fixed_at"][car])


# ----------------------------------------------------------------------------------------------------------------- the search
def search_counts(O, N=1, e=0, car=0, trials=3000, seed=0, stop=None):
    """A uniform scan of one wheel's angle offset over +-3.2 rad in env e's episode, half of the trials with the wheel body spinning at up to
    +-60 rad/s: [(sweeps, solved, fixed_at, wheel, offset, spin)] of the first step after the teleport, one entry per trial (offset and spin
    are rounded to f32: the values are the pin).  stop(sweeps, solved, fixed_at): end the scan at the first trial for which it holds."""
    rng = np.random.RandomState(seed)
    ep = oracle_episode(O, N, SEED, e)
    o = O.OracleEnv(N, car_contacts=False)
    out = []
    try:
        for _ in range(trials):
            wheel = int(rng.randint(1, 5)); off = float(F(rng.uniform(-3.2, 3.2)))
            spin = float(F(rng.uniform(-60, 60))) if rng.rand() < 0.5 else 0.0
            o.reset(ep, render=False)
            st = o.state()
            b, _ = apply_edits(st["bodies"], st["wheels"], ep, [("angle", car, wheel, off, spin)])
            o.set_body(car, wheel, b[car, wheel])
            o.step(np.zeros((N, 3), np.float32), render=False)
            r = outcome(o.dynamics_coverage()[0], car)
            out.append(r + (wheel, off, spin))
            if stop is not None and stop(*r):
                break
    finally:
        o.close()
    return out


# ----------------------------------------------------------------------------------------------------------------- the position loop
# (name, wheel, offset, spin) -> (sweeps, solved, fixed_at) on the first step after the teleport, in env i = the entry's index of an N = 1
# batch (car 0).  Found by find_pins() below; every value is an f32.  The counts sit either side of what the kernel tells apart: the main
# launch's 3 sweeps, the probing sweeps 3, 7 and 11, the last sweep, and fixed points (a failing sweep that moves nothing: the oracle runs on
# to 60, the kernel stops at its next probing sweep) first seen at sweep 2 (the main launch stops, nothing is parked), 4 (the resume launch
# stops at 7), 10 (at 11) and 52 (at 55).
POSITION_PINS = [
    ("s1", 4, 0.28725236654281616, 17.507293701171875, (1, 1, 0)),
    ("s3", 1, -0.5292492508888245, 0.0, (3, 1, 0)),
    ("s4", 1, 0.7752565145492554, 0.0, (4, 1, 0)),
    ("s5", 1, -0.780838131904602, 18.4093074798584, (5, 1, 0)),
    ("s6", 2, -0.7259438037872314, 54.79835510253906, (6, 1, 0)),
    ("s7", 4, 1.1834598779678345, 0.0, (7, 1, 0)),
    ("s10", 2, -1.5767418146133423, 29.58128547668457, (10, 1, 0)),
    ("s11", 4, -1.7450299263000488, 57.386749267578125, (11, 1, 0)),
    ("s12_30", 4, -3.1288676261901855, -14.697962760925293, (26, 1, 0)),
    ("s31_58", 3, -2.3128750324249268, -0.6414581537246704, (53, 1, 0)),
    ("s59", 2, -2.3107826709747314, -46.40095901489258, (59, 1, 0)),
    ("s60_solved", 4, -2.2833750247955322, 0.0, (60, 1, 0)),
    ("s60_unsolved", 2, 3.1139912605285645, -45.40754318237305, (60, 0, 0)),
    ("fixed_by_3", 4, -0.5012130737304688, 0.0, (60, 0, 2)),
    ("fixed_4_7", 3, -0.723933756351471, -51.724449157714844, (60, 0, 4)),
    ("fixed_8_11", 1, 1.4914578199386597, 0.0, (60, 0, 10)),
    ("fixed_late", 2, 1.4524234533309937, 25.318931579589844, (60, 0, 52)),
]
# what find_pins() looks for, entry by entry: (sweeps, solved, fixed_at) -> bool
POSITION_TARGETS = [
    lambda s, ok, f: s == 1 and ok, lambda s, ok, f: s == 3 and ok, lambda s, ok, f: s == 4 and ok, lambda s, ok, f: s == 5 and ok,
    lambda s, ok, f: s == 6 and ok, lambda s, ok, f: s == 7 and ok, lambda s, ok, f: s == 10 and ok, lambda s, ok, f: s == 11 and ok,
    lambda s, ok, f: 12 <= s <= 30 and ok, lambda s, ok, f: 31 <= s <= 58 and ok, lambda s, ok, f: s == 59 and ok, lambda s, ok, f: s == 60 and ok,
    lambda s, ok, f: s == 60 and not ok and f == 0, lambda s, ok, f: 1 <= f <= 3, lambda s, ok, f: 4 <= f <= 7, lambda s, ok, f: 8 <= f <= 11,
    lambda s, ok, f: f > 40,
]
# wheels displaced from their anchors and a spinning hull, envs 17.. of the same batch: {(step, car): (sweeps, solved, fixed_at)}
POSITION_MORE = [
    ("shift_1cm", [("shift", 0, 2, 0.01, 0.0)], {(0, 0): (2, 1, 0)}),
    ("shift_10cm", [("shift", 0, 3, 0.06, 0.08)], {(0, 0): (2, 1, 0)}),
    ("shift_50cm", [("shift", 0, 1, 0.3, -0.4)], {(0, 0): (3, 1, 0)}),
    ("hullspin_100", [("hullspin", 0, 100.0)], {(0, 0): (3, 1, 0), (1, 0): (3, 1, 0), (2, 0): (3, 1, 0)}),
]
# the parked state with more than one car in the env: (N, env, [(car, wheel, offset, spin, (sweeps, solved, fixed_at))]); the cars not named need 1
POSITION_MULTI = [
    ("one_late", 2, 0, [(0, 4, -0.8604831695556641, 0.0, (30, 1, 0))]),
    ("two_late", 2, 1, [(0, 4, 0.7105504870414734, 0.0, (4, 1, 0)), (1, 3, 1.2657785415649414, 0.0, (8, 1, 0))]),
    ("late_beside_stuck", 2, 2, [(0, 3, 2.9701333045959473, -43.883506774902344, (22, 1, 0)), (1, 3, 0.5578461289405823, 3.4091012477874756, (60, 0, 3))]),
    ("states_0_1_2", 3, 0, [(0, 2, 2.7616562843322754, 46.28142547607422, (19, 1, 0)), (1, 3, -0.5917911529541016, 0.0, (60, 0, 3))]),
    ("late_fixed_beside_4", 3, 1, [(0, 4, -0.6937355399131775, 0.0, (4, 1, 0)), (2, 4, 1.0786651372909546, -9.743783950805664, (60, 0, 7))]),
]
POSITION_STEPS = 4


def position_scenes(N):
    """the position-loop scenes of an N-car batch, env e playing entry e"""
    out = []
    if N == 1:
        for name, wheel, off, spin, want in POSITION_PINS:
            out.append(scene(name, 1, {0: [("angle", 0, wheel, off, spin)]}, steps=POSITION_STEPS, pins={(0, 0): want}))
        for name, edits, pins in POSITION_MORE:
            out.append(scene(name, 1, {0: edits}, steps=POSITION_STEPS, pins=pins))
        return out
    rows = sorted((e, name, cars) for name, n, e, cars in POSITION_MULTI if n == N)
    assert [e for e, _, _ in rows] == list(range(len(rows)))
    for e, name, cars in rows:
        pins = {(0, c): (1, 1, 0) for c in range(N)}
        pins.update({(0, c): want for c, _, _, _, want in cars})
        out.append(scene(name, N, {0: [("angle", c, wheel, off, spin) for c, wheel, off, spin, _ in cars]}, steps=POSITION_STEPS, pins=pins))
    return out


def find_pins(O):
    """the search behind POSITION_PINS: entry i in env i's episode, scan seed i"""
    out = []
    for e, (pin, pred) in enumerate(zip(POSITION_PINS, POSITION_TARGETS)):
        r = search_counts(O, 1, e, 0, trials=6000, seed=e, stop=pred)[-1]
        assert pred(*r[:3]), f"{pin[0]}: not found in env {e}"
        out.append((pin[0],) + r[3:] + (r[:3],))
    return out


# ----------------------------------------------------------------------------------------------------------------- wavefront compositions
# What a car's wheels are teleported to.  INSIDE: no limit holds at the step's entry (the f32 neighbours inside +-0.4 included, with spin into
# the limit: the state is decided by the angle at entry alone).  LIMITED: a limit holds — the smallest angle at or beyond either limit, f32(+-0.4)
# added to the hull angle as tests/test_gpu_parity.py does, and +0.45 / -0.47; spinning into the limit (the 3x3 solve, the limit impulse
# accumulates) and away from it (the impulse would change sign: the 2x2 re-solve).
INSIDE = [("angle", 0.0, 0.0), ("angle", 0.2, 2.0), ("joint", "in+", 4.0), ("angle", -0.2, -3.0), ("joint", "in-", -4.0), ("joint", "in+", -1.0),
          ("joint", "in-", 0.0)]
LIMITED = [("joint", "at+", 3.0), ("joint", "at-", 5.0), ("angle", 0.45, -5.0), ("angle", -0.47, -2.0), ("joint", "at+", -5.0),
           ("joint", "at-", -3.0), ("angle", 0.45, 3.0), ("angle", -0.47, 5.0)]
EITHER = [("angle", 0.4, 0.0), ("angle", -0.4, 0.0)]       # (whether f32(f32(hull + 0.4f) - hull) reaches 0.4f depends on the hull angle: "mixed" only)
FULL_ROLES = ("none", "front_first", "front_last", "rear_first", "rear_last", "mixed")
PARTIAL_ROLES = ("none", "front_first", "none", "rear_last", "none", "mixed")
ROUNDS = 6                      # every full wavefront plays every role once; the partial one alternates
ROUND_STEPS = 4


def roles(k):
    """round k: the roles of wavefronts 0, 1 and of the partial one.  "none": no limit anywhere; "front_first" / "front_last" / "rear_first" /
    "rear_last": the ONLY limit of the wavefront is on a front (rear) joint of the car in its first lane / its last real lane (at N = 3 and 5
    that lane sits beside a padding lane); "mixed": every wheel of every car drawn from INSIDE and LIMITED alike"""
    return FULL_ROLES[k % 6], FULL_ROLES[(k + 3) % 6], PARTIAL_ROLES[k % 6]


def touching_envs(N):
    """the env of each wavefront whose cars 0 and 1 touch in composition(N, k, touching=True): the second one, the first where there is one only"""
    G, B = CONFIGS[N]; E, W = lanes(N)
    return [min(w * E + 1, B - 1) for w in range(W)]


def composition(N, k, touching=False):
    """-> (edits [B] per env, role per wavefront [3], limited {wavefront: (env, car, wheel)}) of round k.  Which limit state an edit gives
    follows from the teleported angles (expected_limits); the roles say which lanes hold one.  touching: one env of every wavefront
    (touching_envs) gets its car 1 placed against car 0 — with car<->car contacts enabled the wavefront that holds it runs the contact form
    of the sweeps, which chooses between its limit-free and its limited form by the same ballot."""
    G, B = CONFIGS[N]; E, W = lanes(N)
    rl = roles(k)
    rng = np.random.RandomState(1000 * N + k)
    edits = [[] for _ in range(B)]; limited = {}
    for w in range(W):
        envs = list(range(w * E, min((w + 1) * E, B)))
        role = rl[w]
        if role.endswith("first"):
            limited[w] = (envs[0], 0, (1 + k % 2) if role.startswith("front") else (3 + k % 2))
        elif role.endswith("last"):
            limited[w] = (envs[-1], N - 1, (2 - k % 2) if role.startswith("front") else (4 - k % 2))
        for e in envs:
            for c in range(N):
                edits[e].append(("rest", c))        # (every round starts from rest, where the last one left the car: the cars stay apart)
                for wheel in range(1, 5):
                    lane = (e - w * E) * G + c
                    if role == "mixed":          # (the first lane holds both limits on a front and on a rear joint, whatever the draws give)
                        pool = INSIDE + LIMITED + EITHER; kind, x, spin = pool[int(rng.randint(len(pool)))] if lane else LIMITED[wheel - 1]
                    elif limited.get(w) == (e, c, wheel):
                        kind, x, spin = LIMITED[(k * 3 + w * 5 + N) % len(LIMITED)]
                    else:
                        kind, x, spin = INSIDE[(lane * 4 + wheel + k) % len(INSIDE)]
                    edits[e].append((kind, c, wheel, x, spin))
    if touching:
        for e in touching_envs(N):
            edits[e].insert(0, ("behind", 1, 0, 4.9))
    return edits, rl, limited


def expected_limits(bodies):
    """[..., N, 4] int: the limit state b2RevoluteJoint::InitVelocityConstraints gives each joint of bodies [..., N, 5, 6] f32 at the step's
    entry — 1 where f32(wheel angle - hull angle) <= -0.4f, 2 where >= 0.4f, else 0"""
    b = np.asarray(bodies, np.float32)
    ja = (b[..., 1:, 2] - b[..., :1, 2]).astype(np.float32)
    return np.where(ja <= -LIMIT, 1, np.where(ja >= LIMIT, 2, 0)).astype(np.int64)


def wavefront_form(lim, N):
    """per wavefront, from limit states [B, N, 4]: "free" (no limit on any lane: the limit-free form of all four joints), "rear_free" (limits
    on front joints only: the limit-free form of the rear joints) or "limited" — what the ballot of k_dynamics.h chooses from"""
    E, W = lanes(N)
    out = []
    for w in range(W):
        x = lim[w * E:(w + 1) * E]
        out.append("limited" if (x[..., 2:] != 0).any() else "rear_free" if (x != 0).any() else "free")
    return out


def composition_actions(N, k):
    """[ROUND_STEPS, B, N, 3]: random steering, gas and a little brake, drawn once per round"""
    G, B = CONFIGS[N]
    rng = np.random.RandomState(77 * N + k)
    a = np.empty((ROUND_STEPS, B, N, 3), np.float32)
    a[..., 0] = rng.uniform(-1, 1, a.shape[:3]); a[..., 1] = rng.uniform(0, 1, a.shape[:3]); a[..., 2] = rng.uniform(0, 0.2, a.shape[:3])
    return a


# ----------------------------------------------------------------------------------------------------------------- tyres, clamps, sleep
def tyre_scenes():
    """N = 1 scenes, env e playing entry e: the branches of the f64 tyre model and the clamps of the integration"""
    S = []
    for om in (0.0, 5.0, -5.0, 300.0, -300.0, 1e4):
        S.append(scene(f"omega_{om:g}", 1, {0: [("omega", 0, [om] * 4)]}, [(0, [1.0, 1.0, 0.5])], steps=3))
    S.append(scene("roll_no_brake", 1, {0: [("vel", 0, 30.0, 0.0), ("omega", 0, [55.0] * 4)]}, [(0, [0.1, 0.5, 0.0])], steps=4))
    S.append(scene("brake_005_slow_wheel", 1, {0: [("omega", 0, [0.5, -0.5, 0.3, 20.0])]}, [(0, [0.0, 0.0, 0.05])], steps=4))
    S.append(scene("brake_09", 1, {0: [("vel", 0, 30.0, 0.0), ("omega", 0, [55.0] * 4)]}, [(0, [0.0, 0.0, 0.9])], steps=4))
    S.append(scene("brake_1", 1, {0: [("vel", 0, 30.0, 0.0), ("omega", 0, [55.0] * 4)]}, [(0, [-0.3, 0.2, 1.0])], steps=4))
    S.append(scene("gas_up_and_down", 1, {}, [(0, [0.0, 1.0, 0.0]), (6, [0.0, 0.0, 0.0])], steps=10))
    S.append(scene("steer_to_joint", 1, {0: [("angle", 0, 1, 0.25, 0.0)]}, [(0, [0.0, 0.3, 0.0])], steps=3, steer_to_joint=(0, 1)))
    S.append(scene("steer_small", 1, {}, [(0, [0.01, 0.2, 0.0])], steps=4))
    S.append(scene("steer_held_right", 1, {}, [(0, [1.0, 0.3, 0.0])], steps=10, front_limit=2 - 1))
    S.append(scene("steer_held_left", 1, {}, [(0, [-1.0, 0.3, 0.0])], steps=10, front_limit=2))
    S.append(scene("forward_30", 1, {0: [("vel", 0, 30.0, 0.0)]}, [(0, [0.2, 1.0, 0.0])], steps=4))
    S.append(scene("sideways_15", 1, {0: [("vel", 0, 0.0, 15.0)]}, [(0, [0.0, 0.0, 0.0])], steps=4))
    S.append(scene("reverse_10", 1, {0: [("vel", 0, -10.0, 0.0)]}, [(0, [0.5, 1.0, 0.0])], steps=4))
    S.append(scene("forward_110", 1, {0: [("hullvel", 0, 110.0)]}, [(0, [0.0, 0.0, 0.0])], steps=3, pins={(0, 0): (1, 1, 0)}, translation_clamp=True))   # (all five bodies are clamped alike: one sweep)
    S.append(scene("car_spin_100", 1, {0: [("hullspin", 0, 100.0)] + [("angle", 0, k, 0.0, 100.0) for k in (1, 2, 3, 4)]}, [(0, [0.0, 0.0, 0.0])], steps=3, rotation_clamp=True))
    S.append(scene("grass_drive_brake", 1, {0: [("lateral", 0, 12.0), ("vel", 0, 30.0, 0.0), ("omega", 0, [55.0] * 4)]},
                   [(0, [1.0, 1.0, 0.5]), (4, [0.0, 0.0, 1.0])], steps=7, surface="grass"))
    S.append(scene("grass_rest_light_brake", 1, {0: [("lateral", 0, 12.0), ("rest", 0)]}, [(0, [0.0, 0.0, 0.0]), (3, [0.0, 0.0, 0.05])], steps=6, surface="grass"))
    S[-1]["edits"][1] = [("rest", 0)]                  # (the tyres see the grass from the second step on: at rest again, the force is exactly 0)
    S[-1]["edits"][3] = [("omega", 0, [0.0] * 4)]
    S.append(scene("grass_gas_up_and_down", 1, {0: [("lateral", 0, 12.0)]}, [(0, [0.01, 1.0, 0.0]), (6, [0.01, 0.0, 0.0])], steps=10, surface="grass"))
    S.append(scene("grass_sideways", 1, {0: [("lateral", 0, 12.0), ("vel", 0, 0.0, 15.0)]}, [(0, [0.0, 0.0, 0.0])], steps=4, surface="grass"))
    S.append(scene("split_drive", 1, {0: [("split", 0), ("vel", 0, 20.0, 0.0), ("omega", 0, [36.0] * 4)]}, [(0, [0.0, 1.0, 0.0]), (4, [0.0, 0.0, 0.5])], steps=7, surface="split"))
    return S


# sleep: (scene, the steps on which the sleep rule zeroes a car, per car) — the steps are counted from the first step() after reset()
def sleep_scenes(N):
    if N == 1:
        return [scene("idle", 1, {}, [(0, [0.0, 0.0, 0.0])], steps=52, slept={0: SLEEP_STEPS["idle"]}),
                scene("braked_to_rest", 1, {}, [(0, [0.0, 1.0, 0.0]), (12, [0.0, 0.0, 1.0])], steps=SLEEP_STEPS["braked_to_rest"][-1] + 2,
                      slept={0: SLEEP_STEPS["braked_to_rest"]})]
    return [scene("one_awake", 2, {}, [(0, [[0.0, 1.0, 0.0], [0.0, 0.0, 0.0]])], steps=30, slept={0: [], 1: SLEEP_STEPS["one_awake"]})]


SLEEP_STEPS = {"idle": [25, 50], "braked_to_rest": [40], "one_awake": [25]}


def play(O, scenes, contacts=False):
    """the scenes on the oracle alone -> (run, log): log[k][e] = env e's coverage of step k (row -> [N]); every state finite, every hull
    inside the playfield, no episode over — unless the scene's want says `leaves`"""
    from tests.util import playfield_ok
    run = Run(O, scenes, contacts=contacts); log = []
    for k in range(run.steps):
        _, done, _, _ = run.step()
        log.append(run.coverage())
        for e, (o, sc) in enumerate(zip(run.orcs, scenes)):
            st = o.state()
            assert all(np.isfinite(st[x]).all() for x in ("bodies", "joints", "wheels", "sleep")), f"{sc['name']} step {k}: not finite"
            assert sc["want"].get("leaves") or (playfield_ok(o) and not done[e]), f"{sc['name']} step {k}: left the playfield"
    return run, log


if __name__ == "__main__":
    from oracle import oracle as _O
    for row in find_pins(_O):
        print(f"    {row!r},")
