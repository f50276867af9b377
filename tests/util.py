"""The parity suite's shared tools: the oracle's episodes on the seeds the product uses, envs and oracles built alike, the follower of an
auto-resetting env, and the comparators (tests/test_compare_tools.py holds them to what they must catch).  torch and the package are imported
inside the functions that need them, so the CPU tests can import this module."""
import os
import socket

import numpy as np

STATE_ARRAYS = ("bodies", "joints", "wheels", "limit", "on_road", "sleep")      # get_state() / OracleEnv.state()


def env_streams(seed, g):
    """THE seeding rule (vec_env.py docstring): the RNG streams of global env g — (track stream, global stream: car order and direction)"""
    s = (seed + g) % 2 ** 32
    return np.random.RandomState(s), np.random.RandomState((s + 2 ** 31) % 2 ** 32)


def oracle_episode(O, N, seed, g, direction="CCW", use_random_direction=False):
    """Episode of global env index g exactly as VecMultiCarRacing seeds it."""
    return O.new_episode(N, *env_streams(seed, g), direction=direction, use_random_direction=use_random_direction)


def random_actions(rng, B, N, brake_scale=1.0):
    a = np.empty((B, N, 3), np.float32)
    a[..., 0] = rng.uniform(-1, 1, (B, N))
    a[..., 1] = rng.uniform(0, 1, (B, N))
    a[..., 2] = rng.uniform(0, 1, (B, N)) * brake_scale
    return a


def drive_actions(torch, gen, B, N, k, L=84):
    """a policy that drives INTO its neighbours (bench.py --actions drive plus a bias): gas 1, steering noise +-0.05; in the first 40 steps of
    an episode of L steps the even cars steer one way and the odd cars the other (the grid's pairs converge in half of the envs), then the
    even cars brake for 35 steps (whoever is behind runs into them)"""
    a = torch.zeros((B, N, 3), device="cuda")
    a[..., 0] = torch.rand((B, N), device="cuda", generator=gen) * 0.1 - 0.05
    a[..., 1] = 1.0
    ke = k % L
    if ke < 40: a[:, ::2, 0] += 0.12; a[:, 1::2, 0] -= 0.12
    if 40 <= ke < 75: a[:, ::2, 1] = 0.0; a[:, ::2, 2] = 0.9
    return a


def luma_np(rgb):
    """OpenCV's COLOR_RGB2GRAY on 8-bit data (the formula of include/mcr.h)"""
    x = rgb.astype(np.int64)
    return ((4899 * x[..., 0] + 9617 * x[..., 1] + 1868 * x[..., 2] + 8192) >> 14).astype(np.uint8)


def free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def device_proxy_ids(env, lib, g):
    """the broadphase proxy ids of global env g's current episode: tiles, then the cars' fixtures"""
    out = np.zeros(512 + 64, np.int32)
    n = lib.load().mcr_debug_read_proxy_ids(env.h, int(g), lib.ptr(out), len(out))
    assert n > 0
    return out[:n]


# ----------------------------------------------------------------------------------------------------------------- envs and their oracles
def make_env(B, N, seed, contacts=True, **kw):
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    kw.setdefault("use_random_direction", False); kw.setdefault("auto_reset", False); kw.setdefault("max_episode_steps", 0)
    kw.setdefault("streams", int(os.environ.get("MCR_TEST_STREAMS", "1")))     # 2: whole suite with the contact side stream
    return VecMultiCarRacing(B, N, seed=seed, car_contacts=contacts, async_refill=False, **kw)


def oracles(O, B, N, seed, contacts=True, **kw):
    out = []
    for e in range(B):
        o = O.OracleEnv(N, car_contacts=contacts, h_ratio=kw.get("h_ratio", 0.25), backwards_flag=kw.get("backwards_flag", True),
                        use_ego_color=kw.get("use_ego_color", False))
        o.reset(oracle_episode(O, N, seed, e, direction=kw.get("direction", "CCW"), use_random_direction=kw.get("use_random_direction", False)))
        out.append(o)
    return out


def rear_end_setup(env, orcs, gap=5.2):
    """Put car 1 of every env `gap` behind car 0 (same heading) so that full gas on car 1 + brake on car 0 collide."""
    st = env.get_state()["bodies"].copy()
    for e in range(env.B):
        a = st[e, 0, 0, 2]
        fwd = np.array([-np.sin(a), np.cos(a)], np.float32)          # hull forward axis
        delta = (st[e, 0, 0, :2] - fwd * np.float32(gap)) - st[e, 1, 0, :2]
        st[e, 1, :, 0] += delta[0]; st[e, 1, :, 1] += delta[1]
        st[e, 1, :, 2] = a
    env.set_bodies(st)
    for e, o in enumerate(orcs):
        for k in range(5):
            o.set_body(1, k, st[e, 1, k])


class Follower:
    """Per-env oracle that follows global env g of a VecMultiCarRacing through its episodes: the env's RNG streams, ONE world for the env's
    life, TimeLimit counted here (the oracle is the bare env), next episode = next draw.  `ep` is the episode being played; with render,
    `first_obs` / `first_amb` are its first frame and that frame's ambiguous mask."""

    def __init__(self, O, N, seed, g, max_steps, use_random_direction=True, contacts=True, render=True):
        self.O, self.N, self.g, self.max_steps, self.urd, self.render = O, N, g, max_steps, use_random_direction, render
        self.tr, self.gr = env_streams(seed, g)
        self.o = O.OracleEnv(N, car_contacts=contacts)
        self.new_episode()

    def new_episode(self):
        self.ep = self.O.new_episode(self.N, self.tr, self.gr, use_random_direction=self.urd)
        obs = self.o.reset(self.ep, render=self.render)
        self.first_obs, self.first_amb = (obs, self.o.last_amb) if self.render else (None, None)
        self.steps = 0

    def after_step(self, done):
        """bookkeeping after the batched oracle step: returns (done incl. TimeLimit, truncated)"""
        self.steps += 1
        trunc = False
        if self.max_steps > 0 and self.steps >= self.max_steps:
            trunc = not done
            done = True
        return done, trunc


# ----------------------------------------------------------------------------------------------------------------- comparators
def assert_frame(got, want, amb, what, budget):
    """frames [views, 96, 96, C] against the oracle's: exact outside its "ambiguous" mask (pixel centres within 0.02 px of a drawn edge, where
    real GL is implementation-defined too), at most `budget` differing pixels per view in all"""
    assert want is not None, f"{what}: the oracle step was not rendered"
    d = (got != want).any(-1)
    bad = int((d & (amb == 0)).sum())
    if bad:
        where = np.argwhere(d & (amb == 0))[:6]
        detail = "; ".join(f"view {a} row {r} col {c}: got {got[a, r, c].tolist()} want {want[a, r, c].tolist()}" for a, r, c in where)
        raise AssertionError(f"{what}: {bad} unambiguous pixels differ: {detail}")
    assert int(d.sum()) <= budget * len(want), f"{what}: {int(d.sum())} edge pixels differ"


def assert_pixels(obs, orcs, budget=12):
    """GPU obs vs the frame each oracle rendered INSIDE its last step/reset (call step(..., render=True))."""
    for e, o in enumerate(orcs):
        assert_frame(obs[e], o.last_obs, o.last_amb, f"env {e}", budget)


def assert_state(env, pairs, what=""):
    """the whole state of env index e against oracle o for every (e, o) of `pairs`, BIT-EXACT: the rigid bodies, joints and wheels, the
    rewards and visit counts, every tile's visited and touched bits, the tile count and the episode clock"""
    st = env.get_state(); es = env.get_env_state()
    for e, o in pairs:
        so = o.state(); eo = o.env_state(); T = o.T
        for k in STATE_ARRAYS:
            assert np.array_equal(st[k][e], so[k]), f"{what} env {e}: {k} differs (max abs {np.abs(st[k][e].astype(np.float64) - so[k]).max()})"
        for k in ("reward", "tile_visited_count"):
            assert np.array_equal(es[k][e], eo[k]), f"{what} env {e}: {k} {es[k][e].tolist()} vs the oracle's {eo[k].tolist()}"
        flags = es["tile_flags"][e, :T]
        assert np.array_equal(flags & 0xff, eo["visited"]), f"{what} env {e}: visited bits of tiles {np.nonzero((flags & 0xff) != eo['visited'])[0][:6].tolist()}"
        assert np.array_equal((flags >> 8) & 1, eo["touched"]), f"{what} env {e}: touched bit of tiles {np.nonzero(((flags >> 8) & 1) != eo['touched'])[0][:6].tolist()}"
        assert es["num_tiles"][e] == T, f"{what} env {e}: num_tiles {es['num_tiles'][e]} vs {T}"
        assert es["t"][e] == eo["t"], f"{what} env {e}: t {es['t'][e]!r} vs the oracle's {eo['t']!r}"


# ----------------------------------------------------------------------------------------------------------------- lap scenario
# How the suite gets a car to `tile_visited_count == T` in a few hundred steps instead of ~1800: a TELEPORT phase — each step the lapping car
# is moved rigidly onto track point j = T-1, T-2, ..., LAP_K with zero velocities and zero actions (a teleport is DEFINED on both sides as "every
# car proxy is re-created at its current transform": csrc/mcr_state.hip mcr_set_bodies, oracle orc_set_body), which visits all but a handful of
# tiles — then a DRIVE phase: back on the spawn pose, ordinary steps under a pure-pursuit controller until the last tile is reached.
# tests/test_lap_scenario.py holds every case below to the conditions the GPU tests rest on.
LAP_K = 8                # the teleport script stops at this track point
LAP_TRAIL = 4            # a trailing car sits this many track points behind the leader
LAP_GAS = 0.5
LAP_LOOKAHEAD = 3
LAP_DRIVE_MAX = 120      # the drive phase must complete the lap within this many steps (measured: 44-51)

# (N, lapping car, direction, seed, B): the configurations of tests/test_gpu_lap_completion.py; env e of a case plays the episode of seed + e
LAP_CASES = {
    "n1": (1, 0, "CCW", 101, 2),
    "n2": (2, 1, "CCW", 102, 2),
    "n2cw": (2, 1, "CW", 103, 2),
    "n3": (3, 0, "CCW", 206, 2),       # (N >= 3: seeds whose lapping car spawns on the front row, so that it drives off without meeting the grid;
    "n8": (8, 7, "CCW", 184, 2),       # at N = 8 the teleports along the centre line brush the cars standing on the grid: a few manifolds, on both sides alike)
}
# car<->car manifolds summed over the steps of the teleport phase, per env (cases not listed: none) — pinned, so that a drift in what the
# N = 8 teleports brush does not go unnoticed
LAP_TELEPORT_CONTACTS = {"n8": (2, 27)}


def rigid_teleport(bodies, x, y, heading):
    """bodies [5, 6] f32 of one car (hull, four wheels; cx cy a vx vy w) -> the same car moved rigidly: hull centre at (x, y), hull angle
    `heading`, the five bodies keeping their relative poses, velocities zero.  f64 arithmetic, one rounding to f32."""
    b = np.asarray(bodies, np.float64)
    da = float(heading) - b[0, 2]
    c, s = np.cos(da), np.sin(da)
    out = np.zeros((5, 6), np.float64)
    rx, ry = b[:, 0] - b[0, 0], b[:, 1] - b[0, 1]
    out[:, 0] = x + c * rx - s * ry
    out[:, 1] = y + s * rx + c * ry
    out[:, 2] = b[:, 2] + da
    return out.astype(np.float32)


class LapRun:
    """A list of oracles — env e playing episode eps[e] — and, when given, a VecMultiCarRacing whose env e is the same episode, driven in
    lockstep through the lap scenario.  `step` returns (oracle rewards [n, N], oracle dones [n], what env.step returned or None)."""

    def __init__(self, orcs, eps, lap_car, trail_car=None, env=None, streams=None, direction="CCW"):
        """streams[e]: env e's RNG streams (vec_env.py docstring) behind eps[e] — O.new_episode(N, *streams[e], direction=direction, ...) is
        its next episode"""
        self.orcs, self.eps, self.lap_car, self.trail_car, self.env = orcs, eps, lap_car, trail_car, env
        self.streams, self.direction = streams, direction
        self.N = orcs[0].N
        self.spawn = [o.state()["bodies"].copy() for o in orcs]       # the poses after reset(): the drive phase starts from the lapping car's
        self.steps = 0                                                # env steps taken (all with actions)
        self.last_teleport = -1

    # ---- teleports
    def set_bodies(self, bodies):
        """bodies [n, N, 5, 6] f32 into every oracle (every body: each env's proxies are re-created, as the handle-wide mcr_set_bodies does)"""
        bodies = np.ascontiguousarray(bodies, np.float32)
        for e, o in enumerate(self.orcs):
            for c in range(self.N):
                for k in range(5):
                    o.set_body(c, k, bodies[e, c, k])
        if self.env is not None:
            self.env.set_bodies(bodies)
        self.last_teleport = self.steps

    def bodies(self):
        return np.stack([o.state()["bodies"] for o in self.orcs])

    def heading(self, e, j):
        """the heading of a car that follows env e's track at point j in the episode's direction (spawn_poses' angle)"""
        return self.eps[e]["track"][j, 1] - (np.pi if self.eps[e]["direction"] == "CW" else 0.0)

    def teleport_to_point(self, i):
        """teleport number i of the script: the lapping car of env e onto track point j = max(T_e - 1 - i, LAP_K) (envs with shorter tracks
        wait on their last point), the trailing car LAP_TRAIL points behind it; an i beyond the script (script_len() teleports) goes on below
        LAP_K in every env alike, LAP_K - 1, LAP_K - 2, ... (a negative j wraps).  A CW episode runs the mirrored script, j -> (T_e - j) % T_e:
        its cars spawn at track[0] facing the END of the track, so the stretch left for the drive phase has to be T_e - 1, T_e - 2, ..."""
        st = self.bodies()
        for e, ep in enumerate(self.eps):
            tr = ep["track"]; T = len(tr)
            j = max(T - 1 - i, LAP_K) - max(i - (self.script_len() - 1), 0); jt = j + LAP_TRAIL
            if ep["direction"] == "CW":
                j, jt = T - j, T - jt
            j %= T; jt %= T
            st[e, self.lap_car] = rigid_teleport(st[e, self.lap_car], tr[j, 2], tr[j, 3], self.heading(e, j))
            if self.trail_car is not None:
                st[e, self.trail_car] = rigid_teleport(st[e, self.trail_car], tr[jt, 2], tr[jt, 3], self.heading(e, jt))
        self.set_bodies(st)

    def script_len(self):
        return max(len(ep["track"]) for ep in self.eps) - LAP_K

    def to_spawn(self):
        """the lapping car (and the trailing car, which idles from here on) back onto their spawn poses, at rest"""
        st = self.bodies()
        for e in range(len(self.orcs)):
            for c in (self.lap_car, self.trail_car):
                if c is not None:
                    st[e, c] = self.spawn[e][c]; st[e, c, :, 3:] = 0.0
        self.set_bodies(st)

    # ---- steps
    def step(self, a, render=False):
        a = np.ascontiguousarray(a, np.float32)
        got = None
        if self.env is not None:
            import torch
            got = self.env.step(torch.from_numpy(a).to(self.env.device))
        rew = np.zeros((len(self.orcs), self.N)); done = np.zeros(len(self.orcs), bool)
        for e, o in enumerate(self.orcs):
            _, rew[e], done[e], _ = o.step(a[e], render=render)
        self.steps += 1
        return rew, done, got

    def idle(self):
        return np.zeros((len(self.orcs), self.N, 3), np.float32)

    def drive_actions(self, cars=None):
        """gas LAP_GAS and pure pursuit of the track point LAP_LOOKAHEAD ahead of the nearest one, from the ORACLE's state (so both sides get
        identical actions), for the lapping car; the other cars idle"""
        a = self.idle()
        cars = [self.lap_car] if cars is None else cars
        for e, (o, ep) in enumerate(zip(self.orcs, self.eps)):
            tr = ep["track"]; T = len(tr); d = -1 if ep["direction"] == "CW" else 1
            b = o.state()["bodies"]
            for c in cars:
                x, y, ang = float(b[c, 0, 0]), float(b[c, 0, 1]), float(b[c, 0, 2])
                i = int(np.argmin((tr[:, 2] - x) ** 2 + (tr[:, 3] - y) ** 2))
                t = (i + d * LAP_LOOKAHEAD) % T
                want = np.arctan2(-(tr[t, 2] - x), tr[t, 3] - y)          # heading whose forward axis (-sin, cos) points at the target
                err = (want - ang + np.pi) % (2 * np.pi) - np.pi
                a[e, c, 0] = np.float32(np.clip(-2.0 * err, -1.0, 1.0))    # (positive steer turns the car clockwise)
                a[e, c, 1] = LAP_GAS
        return a

    def tvc(self):
        return np.stack([o.env_state()["tile_visited_count"] for o in self.orcs])

    def lapped(self):
        """per env: has the lapping car visited every tile?"""
        return np.array([int(o.env_state()["tile_visited_count"][self.lap_car]) == o.T for o in self.orcs])


def lap_run(O, case, trail_car=None, env=None, envs=None):
    """LapRun of a LAP_CASES entry after reset() (envs: which of the case's envs, default all).  run.streams[e] are the env's RNG streams
    (vec_env.py docstring) behind its first episode: O.new_episode(N, *run.streams[e], ...) is its second."""
    N, lap_car, direction, seed, B = LAP_CASES[case]
    orcs, eps, streams = [], [], []
    for e in (range(B) if envs is None else envs):
        tr, gr = env_streams(seed, e)
        ep = O.new_episode(N, tr, gr, direction=direction, use_random_direction=False)
        o = O.OracleEnv(N, car_contacts=True); o.reset(ep, render=False)
        orcs.append(o); eps.append(ep); streams.append((tr, gr))
    return LapRun(orcs, eps, lap_car, trail_car=trail_car, env=env, streams=streams, direction=direction)


def lap_teleport_phase(run, each_step=None):
    """the whole teleport script with idle actions; each_step(i, oracle rewards, oracle dones, env.step's result) after every step"""
    for i in range(run.script_len()):
        run.teleport_to_point(i)
        rew, done, got = run.step(run.idle())
        if each_step is not None:
            each_step(i, rew, done, got)


def lap_drive_phase(run, each_step=None, before=None, render=False):
    """back to the spawn poses (plus `before()`: further teleports of the same set_bodies round), then drive steps until every env's lapping
    car has visited every tile (at most LAP_DRIVE_MAX); each_step(k, oracle rewards, oracle dones, env.step's result).  Returns the steps taken."""
    run.to_spawn()
    if before is not None:
        before()
    for k in range(LAP_DRIVE_MAX):
        rew, done, got = run.step(run.drive_actions(), render=render)
        if each_step is not None:
            each_step(k, rew, done, got)
        if run.lapped().all():
            return k + 1
    return LAP_DRIVE_MAX


def lap_touching_pair(run, front, back, gap=4.9):
    """car `back` of every env rigidly behind car `front`, same heading, the hulls overlapping a little (they touch from the next step on)"""
    st = run.bodies()
    for e in range(len(run.orcs)):
        ang = float(st[e, front, 0, 2])
        x = float(st[e, front, 0, 0]) + np.sin(ang) * gap; y = float(st[e, front, 0, 1]) - np.cos(ang) * gap
        st[e, back] = rigid_teleport(st[e, back], x, y, ang)
    run.set_bodies(st)


def playfield_ok(o, playfield=2000 / 6.0):
    """no hull of oracle env `o` outside the playfield (multi_car_racing.py:503-507)"""
    return bool((np.abs(o.positions()) <= playfield).all())


# ----------------------------------------------------------------------------------------------------------------- derived observations
def hull_positions(L, bodies):
    """The hull's body origin of every car, xf_of (csrc/mcr_common.h) restated in numpy float32: p = c - R(a) lc, with (s, c) =
    mcr_sincos_host(a), lc the hull's local centre (mcr_mass_props), every product, sum and difference rounded to float32 on its own (no
    contraction).  bodies [..., 5, 6] f32 (cx cy a vx vy w; body 0 is the hull) -> [..., 2] f32: what mcr_get_positions / the oracle's
    positions() return, from get_state() alone.  L: the loaded libmcr_hip.so."""
    import ctypes
    f32 = np.float32
    mp = np.zeros(6, f32)
    L.mcr_mass_props(mp.ctypes.data_as(ctypes.c_void_p))
    lx, ly = f32(mp[2]), f32(mp[3])
    b = np.asarray(bodies, f32)
    hull = b[..., 0, :].reshape(-1, 6)
    out = np.zeros((len(hull), 2), f32)
    s, c = ctypes.c_float(), ctypes.c_float()
    with np.errstate(all="ignore"):
        for i, h in enumerate(hull):
            L.mcr_sincos_host(ctypes.c_float(float(h[2])), ctypes.byref(s), ctypes.byref(c))
            qs, qc = f32(s.value), f32(c.value)
            out[i, 0] = f32(h[0]) - f32(f32(qc * lx) - f32(qs * ly))
            out[i, 1] = f32(h[1]) - f32(f32(qs * lx) + f32(qc * ly))
    return out.reshape(b.shape[:-2] + (2,))


def assert_f32_bits(got, want, what=""):
    """float32 tensors [envs, cars, ...] compared BY BITS: +0.0 and -0.0 differ, one ulp differs.  NaN is a class: the NaN positions must
    coincide, their payloads and signs are ignored.  Names the first differing (env, car, index within the car's row) with both values."""
    got = np.asarray(got); want = np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32, f"{what}: dtypes {got.dtype} / {want.dtype}, float32 expected"
    assert got.shape == want.shape and got.ndim >= 2, f"{what}: shapes {got.shape} / {want.shape}"
    gn, wn = np.isnan(got), np.isnan(want)
    bad = (gn != wn) | (~gn & ~wn & (np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)))
    if bad.any():
        flat = bad.reshape(bad.shape[0], bad.shape[1], -1)
        e, a, i = (int(v) for v in np.argwhere(flat)[0])
        g = got.reshape(flat.shape)[e, a, i]; w = want.reshape(flat.shape)[e, a, i]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} values differ; first at env {e} car {a} index {i}: got {g!r} "
                             f"(0x{int(np.float32(g).view(np.uint32)):08x}) want {w!r} (0x{int(np.float32(w).view(np.uint32)):08x})")
