"""Synthetic car<->car contact scenes (a helper, not a test): whole cars placed rigidly around car 0 of an ordinary episode, with velocities and
a short action script, so that the contact pass (csrc/k_collide.h, k_carcontacts.h, k_touch.h) and the contact part of the dynamics
(csrc/k_dynamics.h) run on what no drive along a track reaches.  tests/test_contact_cases.py holds every case to the conditions below on the
oracle alone; tests/test_gpu_contact_kernel.py runs them on the device in lockstep with the oracle.

A case is a dict:
  N, seed        the episodes: env e of the case plays the episode of global env e of `seed` (tests/util.py: oracles / make_env)
  envs           one scene per env.  A scene is a list of N - 1 placements (lat, lon, dh, vlat, vlon, w) of cars 1 .. N - 1 in the frame of car
                 0's hull at spawn: `lat` to its right, `lon` ahead of it, heading turned by dh; the car's rigid velocity (vlat, vlon) in the
                 same frame and its spin w.  Every body of a placed car gets the rigid velocity field of its hull.  A scene may also be
                 a dict {"cars": that list, "car0": (vlat, vlon, w) of car 0 itself, which keeps its spawn pose}.
  steps          6 .. 10
  gas            None (zero actions) or {car: gas}: constant gas on those cars, everything else zero
  cap            True: the scene has more touching pairs than the product's store holds; the oracle runs with set_contact_cap(MCR_CC_MAX)
  reach          {coverage row: [envs]}: the rows of OracleEnv.contact_coverage() the case is named for, and the envs that reach them
  counts         {env: (step, manifolds)}: the exact number of touching pairs (before any cap) the env finds in that step
  episodes       1, or 3: the scenes are set up again in the second and third episode of the same world (reset() again)
Loose cars stand FAR_LAT apart to the right of car 0, clear of everything.

The numbers below were found by seeded random search against the oracle (the searches are described where their results stand); the CPU
test pins what they give."""
import math

import numpy as np

from tests.util import rigid_teleport

MCR_CC_MAX = 24          # csrc/mcr_kernels.h: manifold records per env
FAR_LAT = 40.0           # a loose car k stands k * FAR_LAT to the right of car 0


def far(k):
    return (k * FAR_LAT, 0.0, 0.0, 0.0, 0.0, 0.0)


def place(bodies, scene):
    """bodies [N, 5, 6] f32 of one env after reset() -> the scene's bodies [N, 5, 6] f32.  f64 arithmetic, one rounding to f32."""
    b = np.asarray(bodies, np.float32)
    out = b.copy(); out[:, :, 3:] = 0.0
    cars = scene["cars"] if isinstance(scene, dict) else scene
    a0 = float(b[0, 0, 2]); x0, y0 = float(b[0, 0, 0]), float(b[0, 0, 1])
    right = np.array([math.cos(a0), math.sin(a0)]); fwd = np.array([-math.sin(a0), math.cos(a0)])

    def velocities(car, vlat, vlon, w):
        v = right * vlat + fwd * vlon
        r = out[car, :, :2].astype(np.float64) - out[car, 0, :2].astype(np.float64)
        out[car, :, 3] = (v[0] - w * r[:, 1]).astype(np.float32)
        out[car, :, 4] = (v[1] + w * r[:, 0]).astype(np.float32)
        out[car, :, 5] = np.float32(w)

    assert len(cars) == len(b) - 1
    for c, (lat, lon, dh, vlat, vlon, w) in enumerate(cars, start=1):
        p = np.array([x0, y0]) + right * lat + fwd * lon
        out[c] = rigid_teleport(b[c], p[0], p[1], a0 + dh)
        velocities(c, vlat, vlon, w)
    if isinstance(scene, dict) and "car0" in scene:
        velocities(0, *scene["car0"])
    return out


def decode_keys(words):
    """store words (k_carcontacts.h; OracleEnv.car_contacts / mcr_debug_read_contacts of one env) -> [(carA, fixA, carB, fixB)] in stored order"""
    n = int(words[0])
    return [(int(k & 15), int(k >> 4) & 15, int(k >> 8) & 15, int(k >> 12) & 15) for k in words[4:4 + 16 * n:16]]


def case_oracles(O, case, cap=None):
    """the case's oracles after reset(), one tests/util.py Follower per env (f.o is the OracleEnv; f.new_episode() is the env's next episode in
    the same world); cap: override the case's own"""
    from tests.util import Follower
    fs = [Follower(O, case["N"], case["seed"], e, 0, use_random_direction=False, contacts=True, render=False) for e in range(len(case["envs"]))]
    for f in fs:
        f.o.set_contact_cap(MCR_CC_MAX if (case["cap"] if cap is None else cap) else 0)
    return fs


def scene_bodies(case, spawn):
    """spawn [B, N, 5, 6] (the bodies after reset()) -> the case's scenes [B, N, 5, 6] f32"""
    return np.stack([place(spawn[e], sc) for e, sc in enumerate(case["envs"])])


def set_oracle_bodies(o, bodies):
    for c in range(len(bodies)):
        for k in range(5):
            o.set_body(c, k, bodies[c, k])


def add_coverage(total, cov):
    """accumulate OracleEnv.contact_coverage() dicts: the max_* rows by maximum, the others by sum"""
    for k, v in cov.items():
        total[k] = max(total.get(k, 0), v) if k.startswith("max_") else total.get(k, 0) + v
    return total


def actions(case, k):
    """[B, N, 3] f32 of step k"""
    a = np.zeros((len(case["envs"]), case["N"], 3), np.float32)
    for car, g in (case.get("gas") or {}).items():
        a[:, car, 1] = g
    return a


PI = math.pi
Z = (0.0, 0.0, 0.0)

# ---- N = 2: geometry.  One scene per env; `reach` names what the CPU test holds each env to (besides the rows: WHEEL_ONLY_ENV, DEEP_ENVS)
GEOMETRY = [
    [(0.0, -4.9, 0.0, *Z)],                        # 0 rear-end at gap 4.9 (tests/util.py: lap_touching_pair), the anchor
    [(3.6, 0.5, PI / 2, -5.0, 0.0, 0.0)],          # 1 T-bone from the right at 5 m/s
    [(-3.6, -0.5, -PI / 2, 5.0, 0.0, 0.0)],        # 2 ... from the left
    [(0.2, 5.0, PI, 0.0, -10.0, 0.0)],             # 3 head-on, 10 m/s, 0.2 off the axis
    [(2.6, 2.0, 0.3, -3.0, 0.0, 0.0)],             # 4 .. 8 oblique, a corner on a face, five angles
    [(2.6, 2.0, 0.8, -3.0, 0.0, 0.0)],
    [(2.6, 2.0, 1.2, -3.0, 0.0, 0.0)],
    [(2.6, 2.0, 2.0, -3.0, 0.0, 0.0)],
    [(2.6, 2.0, 2.6, -3.0, 0.0, 0.0)],
    [(2.229, 2.754, 0.107, -2.0, 0.0, 0.0)],       # 9 wheel on hull only (search_wheel_only: lat 1.9 .. 2.5 either side, lon -4 .. 4, |dh| < 0.15, RandomState(0))
    [(0.5, 1.0, 0.4, *Z)],                         # 10, 11 deep overlap: several hull polygons of each car inside the other
    [(0.0, 0.3, 1.5, *Z)],
]
WHEEL_ONLY_ENV = 9
DEEP_ENVS = (10, 11)

# ---- N = 2: hulls whose distance straddles the touch threshold (total polygon radius 0.02).  Per env the two float64 `lon` values between
# which 70 bisection steps (search_straddle) put the verdict of the first step's contact pass (car 1 behind car 0, closing at 0.5 m/s): one double apart,
# so the placed float32 bodies are neighbours too.  Even envs touch in step 0, odd envs from step 1 on.
STRADDLE_LON = ((-5.0199995290293185, -5.019999529029319), (-5.020000104092838, -5.020000104092839),
                (-5.019998821802191, -5.019998821802192), (-5.019997410679429, -5.01999741067943))
STRADDLE = [[(0.0, STRADDLE_LON[e][e & 1], 0.0, 0.0, 0.5, 0.0)] for e in range(4)]

# ---- N = 2: kinematics
KINEMATICS = [
    {"cars": [(0.0, -5.0, 0.0, 0.0, 250.0, 0.0)], "car0": (0.0, 100.0, 0.0)},     # 0 closing at 150 m/s, both above the 2 m per step clamp, touching throughout
    [(0.0, 9.0, PI, 0.0, -150.0, 0.0)],            # 1 head-on at 150 m/s from 9 ahead: clamped in flight, contact from step 2
    [(2.9, 0.5, 0.3, 0.0, 0.0, 8.5)],              # 2, 3 spinning at +-8.5 rad/s against car 0's side
    [(2.9, 0.5, 0.3, 0.0, 0.0, -8.5)],
    [(2.9, 0.5, 0.3, 0.0, 0.0, -90.0)],            # 4 at -90 rad/s: above the quarter turn per step (78.5 rad/s) the rotation is clamped
    [(0.204, 4.442, -0.65, -11.8, -2.74, -3.06)],  # 5 a contact that ends and begins again: manifolds 4, 1, 0, 2, 1, .. (search_solver)
    [(2.768, 2.066, 2.219, 0.0, 0.0, 100.0)],      # 6 at +100 rad/s, in and out of contact over five steps: six rotation clamps (search_spin)
]
FAST_ENVS, SPIN_CLAMP_ENVS, END_BEGIN_ENV = (0, 1), (4, 6), 5

# ---- solver branches (search_solver: random placements and velocities, first scene that reaches the row)
SOLVER2 = [
    [(1.352, 0.013, 2.866, *Z)],                   # 0 the block solver's no-solution exit
    [(-0.13, 0.531, 1.962, *Z)],                   # 1 an ill-conditioned two-point manifold solved as one point, the same pair well-conditioned next step
]
SOLVER3 = [
    [(-2.66, -2.273, -0.14, 9.37, -0.6, -1.61), (-2.574, -4.129, -3.015, 2.0, 1.67, 1.11)],          # 0 no-solution exit
    [(-0.091, 1.832, 2.018, -10.5, 7.62, 3.29), (0.508, -4.087, 0.631, -3.55, 11.03, -2.8)],         # 1 ill-conditioned, then well
    [(-2.323, 4.905, 2.17, 0.21, -0.45, -0.64), (1.298, -2.125, -0.003, *Z)],                        # 2 ends and begins again
]
STACK3 = [(0.0, -4.88, 0.0, *Z), (0.0, 4.88, PI, *Z)]      # cars 1 and 2 push car 0 from both ends under full gas: every step uses all 60 position sweeps

# ---- N = 3: exact manifold counts in step 0 (search_counts: two cars at lat +-2.5, lon +-3, any heading, every third trial at 0.4 of that;
# RandomState(0), 1500 trials, first scene per count whose later steps stay within the store)
COUNT_SCENES = {
    1: [(0.0, -4.9, 0.0, *Z), far(2)],
    2: [(0.0, -4.9, 0.0, *Z), (0.0, -9.8, 0.0, *Z)],
    3: [(-2.31, -2.23, -2.791, *Z), (2.025, -2.191, 2.197, *Z)],
    4: [(-2.424, 0.422, 0.744, *Z), (2.439, 2.312, 0.11, *Z)],
    5: [(2.312, -2.337, 0.822, *Z), (2.49, 2.927, 0.649, *Z)],
    23: [(-0.554, 1.086, -0.332, *Z), (0.693, 0.479, -1.273, *Z)],
    24: [(-1.132, 1.788, -1.975, *Z), (2.264, 1.125, -1.788, *Z)],
    25: [(0.954, 0.252, 1.503, *Z), (-0.922, -0.521, -2.386, *Z)],
    40: [(-0.875, -0.62, -0.425, *Z), (0.044, 0.656, 2.882, *Z)],
}
NONE3 = [far(1), far(2)]

# ---- N = 8: islands
CHAIN8 = [(0.0, -4.88 * k, 0.0, *Z) for k in range(1, 8)]
STAR7 = [(1.099, 5.42, 2.942, *Z), (4.287, 1.438, 1.894, *Z), (3.81, -3.366, 0.847, *Z), (-1.02, -5.03, -0.2, *Z), (-4.288, -1.438, -1.247, *Z),
         (-3.995, 3.53, -2.294, *Z), far(1)]      # six cars nose-on to car 0, 0.04 inside the distance at which each touches it (search_star); one loose
TWO_ISLANDS = [(0.0, -4.88, 0.0, *Z), (0.3, -9.7, 0.1, *Z), (15.0, 0.0, 0.0, *Z), (15.5, 4.6, PI, *Z), far(1), far(2), far(3)]
def cluster8():
    """all eight cars within 1.5 of car 0, any heading (RandomState(1)): 276 touching pairs"""
    rng = np.random.RandomState(1)
    return [(round(rng.uniform(-1.5, 1.5), 3), round(rng.uniform(-1.5, 1.5), 3), round(rng.uniform(-PI, PI), 3), *Z) for _ in range(7)]


CLUSTER8 = cluster8()

# ---- reused worlds: the same scenes in the second and third episode of one world (proxy ids off the tree's free list: `flipped` manifolds)
REUSE4 = [(0.0, -4.9, 0.0, *Z), (2.6, 2.0, 1.2, -3.0, 0.0, 0.0), (-3.6, -0.5, -PI / 2, 5.0, 0.0, 0.0)]


def case(N, seed, envs, steps=6, gas=None, cap=False, reach=None, counts=None, episodes=1):
    assert 6 <= steps <= 10 and len(envs) <= 16
    for sc in envs:
        assert len(sc["cars"] if isinstance(sc, dict) else sc) == N - 1
    return dict(N=N, seed=seed, envs=envs, steps=steps, gas=gas, cap=cap, reach=reach or {}, counts=counts or {}, episodes=episodes)


CASES = {
    "geometry": case(2, 300, GEOMETRY, steps=8, reach={"face_a": list(range(12)), "face_b": [1, 5, 6, 7, 8, 10, 11], "id_miss": [1, 5, 6, 7, 10, 11]}),
    "straddle": case(2, 330, STRADDLE, steps=6, reach={"id_match": [0, 1, 2, 3]}),
    "kinematics": case(2, 300, KINEMATICS, steps=8, reach={"translation_clamp": [0, 1, 4, 6], "rotation_clamp": [4, 6]}),
    "solver2": case(2, 300, SOLVER2, steps=8, reach={"block_none": [0], "ill_conditioned": [1], "ill_then_well": [1], "block_both": [0, 1], "block_x1": [0, 1],
                                                     "block_x2": [0, 1], "block_neither": [0, 1]}),
    "solver3": case(3, 310, SOLVER3, steps=8, reach={"block_none": [0], "ill_conditioned": [1], "ill_then_well": [1]}),
    "stack": case(3, 310, [STACK3, STACK3], steps=8, gas={1: 1.0, 2: 1.0}, reach={"pos_sweeps_all": [0, 1]}),
    # (single-stream handles pack 64 / G envs into a wavefront, all sharing its LDS pool of 2 * MCR_CC_MAX constraint records: `counts_full`
    # stays below it, `full2` fills it exactly, `full4` is beyond it and makes the packed dynamics step the wavefront's envs two at a time)
    "counts": case(3, 310, [COUNT_SCENES[c] for c in (1, 2, 3, 4, 5)], steps=6, counts={e: (0, c) for e, c in enumerate((1, 2, 3, 4, 5))},
                   reach={"max_island_cars": [0, 1]}),
    "counts_full": case(3, 310, [COUNT_SCENES[23], COUNT_SCENES[24]], steps=6, counts={0: (0, 23), 1: (0, 24)}),      # 47 of the pool's 48
    "full2": case(3, 310, [COUNT_SCENES[24]] * 2, steps=6, counts={0: (0, 24), 1: (0, 24)}),                            # the pool exactly full
    "full4": case(3, 310, [COUNT_SCENES[24]] * 4, steps=6, counts={e: (0, 24) for e in range(4)}),
    "over_cap25": case(3, 310, [COUNT_SCENES[25], COUNT_SCENES[1]], steps=6, cap=True, counts={0: (0, 25), 1: (0, 1)}, reach={"dropped": [0]}),
    "over_cap40": case(3, 310, [COUNT_SCENES[40], COUNT_SCENES[5]], steps=6, cap=True, counts={0: (0, 40), 1: (0, 5)}, reach={"dropped": [0]}),
    "islands": case(8, 320, [CHAIN8, STAR7, TWO_ISLANDS], steps=6, gas={7: 1.0}, reach={"max_island_cars": [0, 1, 2]}),
    "cluster": case(8, 320, [CLUSTER8, CHAIN8], steps=6, cap=True, counts={0: (0, 276), 1: (0, 7)}, reach={"dropped": [0]}),
    "reuse2": case(2, 0, [GEOMETRY[10]] * 3, steps=6, episodes=3, reach={"flipped": [0, 2]}),
    "reuse4": case(4, 7, [REUSE4] * 3, steps=6, episodes=3, reach={"flipped": [0, 1, 2]}),
}
# the largest island of each `islands` env, in cars
ISLAND_CARS = (8, 7, 3)


# ------------------------------------------------------------------------------------------------------------------------------ the searches
# How the literals above were found — not run by any test (python -m tests.contact_cases runs them all and prints what they find, a few
# minutes on a CPU): if a hull vertex, a spawn pose or a solver constant changes and tests/test_contact_cases.py fails, these find the
# replacements.  O is the oracle module (oracle/oracle.py); every search is seeded and deterministic.
def evaluate(O, N, seed, e, scene, steps, cap=False, gas=None):
    """the scene in env e of `seed` on the oracle alone -> (manifolds per step, keys per step, coverage, state finite and no episode ended)"""
    from tests.util import oracle_episode
    o = O.OracleEnv(N); o.reset(oracle_episode(O, N, seed, e), render=False)
    o.set_contact_cap(MCR_CC_MAX if cap else 0)
    set_oracle_bodies(o, place(o.state()["bodies"], scene))
    o.contact_coverage(reset=True)
    a = np.zeros((N, 3), np.float32)
    for car, g in (gas or {}).items():
        a[car, 1] = g
    counts, keys, ok = [], [], True
    for _ in range(steps):
        _, _, done, _ = o.step(a, render=False)
        w = o.car_contacts(); counts.append(int(w[0])); keys.append(decode_keys(w)); ok = ok and not done
    cov = o.contact_coverage(); ok = ok and bool(np.isfinite(o.state()["bodies"]).all()); o.close()
    return counts, keys, cov, ok


def search_counts(O, wanted=(3, 4, 5, 23, 24, 25, 40), trials=1500, N=3, seed=310, e=0):
    """{count: scene}: the first scene per count with that many touching pairs in step 0, contacts in three steps at least and — below the
    cap — no later step beyond the store (counts 1 and 2 are placed by hand: a rear-end pair, a chain of three)"""
    rng = np.random.RandomState(0); found = {}
    for t in range(trials):
        sc = [(round(rng.uniform(-2.5, 2.5), 3), round(rng.uniform(-3, 3), 3), round(rng.uniform(-PI, PI), 3), *Z) for _ in range(N - 1)]
        if t % 3 == 0:
            sc = [(round(v[0] * 0.4, 3), round(v[1] * 0.4, 3), v[2], *Z) for v in sc]
        n, _, _, ok = evaluate(O, N, seed, e, sc, 6)
        if ok and n[0] in wanted and n[0] not in found and sum(c > 0 for c in n) >= 3 and (n[0] > MCR_CC_MAX or max(n) <= MCR_CC_MAX):
            found[n[0]] = sc
        if len(found) == len(wanted):
            break
    return found


def search_solver(O, trials=4000):
    """{"block_none2", "ill_then_well2", "end_begin2", and the same with 3}: first scene (N = 2 and N = 3 in turn, one RNG) that reaches the
    block solver's no-solution exit / an ill-conditioned manifold whose pair is well-conditioned in the next step / a contact that ends and
    begins again, within the store and with contacts in three steps"""
    rng = np.random.RandomState(0); found = {}
    for t in range(trials):
        N = 2 if t % 2 == 0 else 3
        sc = []
        for _ in range(N - 1):
            sp = rng.choice([0.0, 3.0, 15.0])
            sc.append((round(rng.uniform(-3, 3), 3), round(rng.uniform(-5, 5), 3), round(rng.uniform(-PI, PI), 3),
                       round(rng.uniform(-sp, sp), 2), round(rng.uniform(-sp, sp), 2), round(rng.uniform(-sp, sp) * 0.5, 2)))
        n, _, cov, ok = evaluate(O, N, 300 if N == 2 else 310, 0, sc, 8)
        if not ok or max(n) > MCR_CC_MAX or sum(c > 0 for c in n) < 3:
            continue
        s = "".join("1" if c else "0" for c in n)
        for tag, hit in (("block_none", cov["block_none"] > 0), ("ill_then_well", cov["ill_then_well"] > 0),
                         ("end_begin", "10" in s and "01" in s[s.index("10"):] if "10" in s else False)):
            if hit:
                found.setdefault(f"{tag}{N}", sc)
        if len(found) == 6:
            break
    return found


def search_wheel_only(O, trials=3000):
    """a car beside car 0, pressed against it at 2 m/s, whose every manifold over 8 steps joins a wheel and a hull"""
    rng = np.random.RandomState(0)
    for _ in range(trials):
        lat = float(round(rng.uniform(1.9, 2.5) * rng.choice([-1, 1]), 3))
        sc = [(lat, round(rng.uniform(-4, 4), 3), round(rng.uniform(-0.15, 0.15), 3), -2.0 if lat > 0 else 2.0, 0.0, 0.0)]
        n, keys, _, ok = evaluate(O, 2, 300, 0, sc, 8)
        if ok and sum(c > 0 for c in n) >= 4 and all((k[1] >= 4) != (k[3] >= 4) for s in keys for k in s):
            return sc
    return None


def search_straddle(O, envs=4, seed=330):
    """per env (lon that touches, lon that does not), one double apart: bisection on the first step's verdict"""
    out = []
    for e in range(envs):
        lo, hi = -4.80, -5.60
        for _ in range(70):
            mid = 0.5 * (lo + hi)
            if evaluate(O, 2, seed, e, [(0.0, mid, 0.0, 0.0, 0.5, 0.0)], 1)[0][0]:
                lo = mid
            else:
                hi = mid
        out.append((lo, hi))
    return out


def search_star(O, spokes=6, seed=320):
    """`spokes` cars nose-on to car 0 at equal angles (from 0.2), each 0.04 inside the distance at which it alone touches car 0"""
    star = []
    for i in range(spokes):
        th = 2 * PI * i / spokes + 0.2
        lo, hi = 0.5, 9.0
        for _ in range(30):
            r = 0.5 * (lo + hi)
            sc = [far(k) for k in range(1, 8)]; sc[0] = (r * math.sin(th), r * math.cos(th), PI - th, *Z)
            if evaluate(O, 8, seed, 0, sc, 1)[0][0]:
                lo = r
            else:
                hi = r
        r = round(lo - 0.04, 3)
        star.append((round(r * math.sin(th), 3), round(r * math.cos(th), 3), round(PI - th, 3), *Z))
    return star + [far(k) for k in range(1, 8 - spokes)]


def search_spin(O, trials=400, e=6):
    """a car spinning at 90 .. 120 rad/s beside car 0 (env e of the kinematics case): contacts in three steps, two rotation clamps at least"""
    rng = np.random.RandomState(0)
    for _ in range(trials):
        sc = [(float(round(rng.uniform(2.0, 3.4) * rng.choice([-1, 1]), 3)), round(rng.uniform(-3, 3), 3), round(rng.uniform(-3.1, 3.1), 3), 0.0, 0.0,
               float(rng.choice([90.0, 100.0, 120.0])))]
        n, _, cov, ok = evaluate(O, 2, 300, e, sc, 8)
        if ok and sum(c > 0 for c in n) >= 3 and any(n[1:]) and cov["rotation_clamp"] >= 2 and max(n) <= MCR_CC_MAX:
            return sc
    return None


if __name__ == "__main__":
    from oracle import oracle as _O
    for _name, _f in (("straddle", search_straddle), ("wheel_only", search_wheel_only), ("spin", search_spin), ("star", search_star),
                      ("solver", search_solver), ("counts", search_counts)):
        print(_name, _f(_O), flush=True)
