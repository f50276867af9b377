"""MI355X: k_flags (csrc/k_flags.h) on the synthetic tracks and poses of tests/flag_cases.py, through a launch of its own (mcr_flags_now) —
driving_backward and driving_on_grass of every car, bit for bit, against tests/flags_ref.py on get_state() arrays, tests/util.py's
hull_positions and the track rows.  tests/test_flag_cases.py ties that restatement to the oracle and holds the cases to what they are meant
to be, without a device.

What the oracle rollouts cannot reach and this file does: cars far from every block of road_poly, cars whose nearest track point lies in
another block than the car, a kerb-only last block, 48 blocks in use; exact f64 ties and one-ulp gaps between lanes, 16-lane groups and trips
of the block loop; poses exactly on a border, a seam, a vertex, a kerb's edges; cars on a kerb and on no tile, the kerb of tile 0; hull angles
beyond a turn, a quarter turn to the last float32 bit, the speed threshold to the last bit, the wrap of the angle difference; poses 1e3 ..
3.4e38 away, inf and NaN; N = 3, 5, 8 with every car of an env on a case of its own.

The last test steps: every path a step can take to the scans (the single-stream launch, k_flags_viewprep, the list rasters' bookkeeping
workgroups, the deferred launch) on tracks with kerbs, N up to 8, cars in contact — the flags being a function of the post-step hull state
alone, they are compared with the restatement on get_state()."""
import ctypes

import numpy as np
import pytest

from tests import flag_cases as F
from tests import obs_cases as C
from tests.util import make_env, rigid_teleport

pytestmark = pytest.mark.gpu

NS = (1, 2, 3, 5, 8)


@pytest.fixture(scope="module")
def tracks(lib):
    return F.all_tracks(lib)


@pytest.fixture(scope="module", params=NS, ids=lambda n: f"N{n}")
def rig(request, lib, tracks):
    """reset once, stepped ONCE (just_reset is clear), never stepped again"""
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    r = C.Rig(lib, tracks, request.param, None, steps=1)
    r.geos = F.geometry(tracks)
    r.status0 = r.env.status_words().tolist()        # (N = 8 on a 20-tile circle: the grid's cars overlap at reset; what that raised is not the scans')
    yield r
    r.close()


def _flags_now(rig_or_env):
    """mcr_flags_now on the current stream, waited for; the flags mcr_get_env_state then shows"""
    import torch
    env = getattr(rig_or_env, "env", rig_or_env)
    st = torch.cuda.current_stream(env.device)
    assert env.L.mcr_flags_now(env.h, ctypes.c_void_p(st.cuda_stream)) == 0
    st.synchronize()
    es = env.get_env_state()
    return es["driving_backward"], es["driving_on_grass"]


def _compare(got, want, tracks, tags, what):
    bad = [(e, a) for e in range(got[0].shape[0]) for a in range(got[0].shape[1]) if (got[0][e, a], got[1][e, a]) != (want[0][e, a], want[1][e, a])]
    if bad:
        e, a = bad[0]
        raise AssertionError(f"{what}: {len(bad)} cars differ; first: track {tracks[e][0]} cw {tracks[e][2]} (env {e}) car {a}, pose {tags[e][a]}: "
                             f"backward / on grass {int(got[0][e, a])} / {int(got[1][e, a])}, the restatement's {int(want[0][e, a])} / {int(want[1][e, a])} "
                             f"(nearest tile {int(want[2][e, a])})")


def test_the_rig_is_live_and_past_its_first_step(rig):
    rec = np.zeros((rig.B, 12), np.int32)
    assert rig.L.mcr_debug_read_env_records(rig.env.h, rec.ctypes.data_as(ctypes.c_void_p), rec.nbytes) >= 0
    assert (rec[:, 6] == 1).all() and (rec[:, 8] == 0).all(), "every env active, none just reset"
    assert rig.status0[:2] == [0, 0]


@pytest.mark.parametrize("set_name", F.SETS)
def test_flags_equal_the_restatement(rig, set_name):
    seen = set()
    for rnd in range(F.rounds(set_name, rig.tracks, rig.geos, rig.N)):
        with np.errstate(all="ignore"):
            bodies, tags = F.assign(rig.L, rig.tracks, rig.geos, rig.N, rig.base["bodies"], set_name, rnd)
        st = rig.set_bodies(bodies)
        got = _flags_now(rig)
        want = F.reference(rig.L, rig.tracks, rig.geos, st["bodies"])
        _compare(got, want, rig.tracks, tags, f"N {rig.N} set {set_name} round {rnd}")
        seen |= set(zip(want[0].ravel().tolist(), want[1].ravel().tolist()))
    assert len(seen) >= 2, "one class of flags only"
    assert rig.env.status_words().tolist() == rig.status0, "a status word was raised"


def test_nonfinite_poses_are_defined(rig):
    """NaN / inf in x, y or the angle: MCR_OK, no status word, nearest tile 0 (argmin of a row of NaN or inf), on the grass — and the finite
    cars beside them are not disturbed"""
    n = 0
    for rnd in range(F.rounds("far", rig.tracks, rig.geos, rig.N)):
        with np.errstate(all="ignore"):
            bodies, tags = F.assign(rig.L, rig.tracks, rig.geos, rig.N, rig.base["bodies"], "far", rnd)
        st = rig.set_bodies(bodies)
        got = _flags_now(rig)
        want = F.reference(rig.L, rig.tracks, rig.geos, st["bodies"])
        _compare(got, want, rig.tracks, tags, f"N {rig.N} far round {rnd}")
        for e in range(rig.B):
            for a in range(rig.N):
                if tags[e][a].startswith("nonfinite") and not np.isfinite(st["bodies"][e, a, 0, :2]).all():
                    assert want[2][e, a] == 0 and got[1][e, a] == 1, f"env {e} car {a}: {tags[e][a]}"
                    n += 1
    assert n >= rig.B and rig.env.status_words().tolist() == rig.status0, "a status word was raised"


def test_after_reset_alone_the_flags_stay_zero(lib, tracks):
    """just_reset: the reference's reset() steps without an action and skips the bookkeeping (:435) — whatever the poses are"""
    geos = F.geometry(tracks)
    for N in (2, 5):
        r = C.Rig(lib, tracks, N, None, steps=0)
        try:
            for set_name in ("scatter", "heading_slow"):
                bodies, _ = F.assign(r.L, tracks, geos, N, r.base["bodies"], set_name, 0)
                st = r.set_bodies(bodies)
                want = F.reference(r.L, tracks, geos, st["bodies"])
                assert want[0].any() and want[1].any(), "the poses would set both flags"
                bw, og = _flags_now(r)
                assert not bw.any() and not og.any()
        finally:
            r.close()


def _spread_poses(tracks, geos, e, N, rng, K):
    """N poses of track e's scatter, kerb-only and culling cases that lie near the road, at least 8 apart"""
    pool = [c for s in ("kerb_only", "culling", "scatter") for c in F.cases(s, e, tracks, geos)
            if c[5].split()[0] not in ("centroid", "outside", "spur")]
    rows = tracks[e][1]
    while len(pool) < 40:
        pool += [p + ("random",) for p in C._scatter(rng, rows, 8)]
    k = (e // K) * 5 % len(pool)         # (the second env of a track starts elsewhere in the pool)
    pool = pool[k:] + pool[:k]
    for _ in range(50):                   # greedy; more candidates while it comes up short (a 20-tile circle is small for 8 cars)
        out = []
        for c in pool:
            if all((c[0] - o[0]) ** 2 + (c[1] - o[1]) ** 2 >= 64.0 for o in out):
                out.append(c)
            if len(out) == N:
                return out
        pool = [p + ("random",) for p in C._scatter(rng, rows, 16)] + pool
    raise AssertionError(f"track {tracks[e][0]}: no {N} poses 8 apart")


@pytest.mark.parametrize("streams", [1, None], ids=["one-stream", "default-streams"])
@pytest.mark.parametrize("N", [2, 4, 8])
def test_every_path_of_a_step_equals_the_restatement(lib, tracks, N, streams):
    """streams None: what VecMultiCarRacing picks by itself — two, and the three-chain step, from 64 envs on: every track twice"""
    import torch
    from multi_car_racing_amd import levels
    blobs = np.concatenate([levels.from_tracks([rows], N, "CW" if cw else "CCW") for _, rows, cw in tracks])
    K = len(tracks)
    tracks = tracks * (1 if streams == 1 else 2)              # (level_order "cycle": env e plays level e mod K)
    geos = F.geometry(tracks)
    B = len(tracks)
    env = make_env(B, N, 0, levels=blobs, level_order="cycle", obs=True, streams=streams) if streams is not None else _default_streams_env(B, N, blobs)
    try:
        if streams is None and not (env.L.mcr_step_ordering(env.h) & 1):
            pytest.skip("kernels of different streams do not overlap here: the step orders its streams with events")
        env.reset()
        L = env.L
        st = env.get_state()["bodies"].copy()
        rng = np.random.RandomState(5)
        contact_envs = [e for e, t in enumerate(tracks) if t[0] in ("circle128", "circle321")]      # (tracks long enough for a grid of 8 cars)
        assert len(contact_envs) == 4 * (B // K)
        for e in range(B):
            if e in contact_envs:          # car 1 behind car 0, the hulls overlapping a little (tests/util.py: rear_end_setup, closer)
                a0 = float(st[e, 0, 0, 2])
                x = float(st[e, 0, 0, 0]) + np.sin(a0) * 4.9; y = float(st[e, 0, 0, 1]) - np.cos(a0) * 4.9
                st[e, 1] = rigid_teleport(st[e, 1], x, y, a0)
                continue
            for a, (px, py, ang, _, _, _) in enumerate(_spread_poses(tracks, geos, e, N, rng, K)):
                st[e, a] = C.place(L, st[e, a], px, py, ang)
                speed = rng.uniform(3, 10)
                st[e, a, :, 3] = np.float32(-np.sin(ang) * speed); st[e, a, :, 4] = np.float32(np.cos(ang) * speed)
        env.set_bodies(st)
        act = torch.zeros((B, N, 3), device=env.device); act[..., 1] = 0.3
        act[contact_envs, 1, 1] = 1.0; act[contact_envs, 0, 2] = 0.8
        listed, marked = [], []
        seen = set()
        routed0 = np.zeros(4, np.uint64)
        assert L.mcr_debug_read_counters(env.h, lib.ptr(routed0)) == 0            # (cumulative since the handle was made: the compared steps' share is a difference)
        for k in range(3):
            _, _, done, _ = env.step(act)
            assert not done.any().item(), f"step {k}: an env ended its episode"
            if streams is None:
                part = np.zeros(B, np.uint8); clist = np.zeros(1 + B, np.int32)
                assert L.mcr_debug_read_partition(env.h, lib.ptr(part), lib.ptr(clist)) == 0
                listed.append(int(clist[0])); marked.append(np.nonzero(part)[0].tolist())
            es = env.get_env_state()
            bodies = env.get_state()["bodies"]
            want = F.reference(L, tracks, geos, bodies)
            tags = [[f"hull {bodies[e, a, 0].tolist()}" for a in range(N)] for e in range(B)]
            _compare((es["driving_backward"], es["driving_on_grass"]), want, tracks, tags, f"N {N} streams {streams} step {k}")
            seen |= set(zip(want[0].ravel().tolist(), want[1].ravel().tolist()))
        counts = np.zeros(B, np.int32)
        assert L.mcr_debug_read_contact_counts(env.h, lib.ptr(counts)) == 0
        assert (counts[contact_envs] > 0).all() and counts.sum() == counts[contact_envs].sum(), f"car<->car contacts per env: {counts.tolist()}"
        if streams is None:
            # (mcr_debug_read_partition's list length reads 0 behind a fused step: the contact chain empties the count of its list when it
            # is through with it, k_list_chain.h.  The verdicts the step went by — the same call's part_out — name the list's envs, and
            # counter 2, over the compared steps alone, counts the envs the contact pass routed to the chain.)
            routed = np.zeros(4, np.uint64)
            assert L.mcr_debug_read_counters(env.h, lib.ptr(routed)) == 0
            in_steps = int(routed[2] - routed0[2])
            assert contact_envs in marked and (max(listed) > 0 or in_steps >= len(contact_envs)), \
                (f"the touching envs were the contact chain's in no compared step: list lengths {listed}, envs whose touch verdict was set {marked}, "
                 f"envs routed to the chain in the compared steps {in_steps}, contact pass beside the dynamics {L.mcr_concurrent_collide(env.h)}")
        assert len(seen) == 4, f"classes of (backward, on grass) seen: {seen}"
        assert env.status_words()[:2].tolist() == [0, 0] and env.verdict_mismatches() == 0
    finally:
        env.close()


def _default_streams_env(B, N, blobs):
    """the handle VecMultiCarRacing makes when nobody says `streams`"""
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    return VecMultiCarRacing(B, N, seed=0, car_contacts=True, async_refill=False, use_random_direction=False, auto_reset=False,
                             max_episode_steps=0, levels=blobs, level_order="cycle", obs=True)
