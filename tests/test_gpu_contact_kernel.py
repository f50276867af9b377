"""MI355X: the car<->car contact pass (csrc/k_collide.h, k_carcontacts.h), the touch verdict (k_touch.h) and the contact part of the dynamics
(k_dynamics.h: dynamics_block<CC>) on the synthetic scenes of tests/contact_cases.py, in lockstep with the oracle.  Every step: rewards bit for
bit, and the device's manifold store — count, overflow mark, joint orders, every record's key, type, local geometry, feature ids and post-solve
impulses, in solve order — equal to the oracle's (OracleEnv.car_contacts); the last step: the whole state.  streams = 1 runs the packed
dynamics with 64 / G envs per wavefront, streams = 2 the contact chain with one; no verdict mismatch, no status word but the
documented overflow, raised in exactly the steps where the oracle (with the same cap, oracle/mcr_oracle_contacts.inc: THE DROP RULE) dropped
pairs.  tests/test_contact_cases.py holds the scenes to what they are named for."""
import warnings

import numpy as np
import pytest

from tests import contact_cases as C
from tests import contact_obs_ref as R
from tests.util import assert_state, make_env

pytestmark = pytest.mark.gpu
ST_CC_OVERFLOW = 2


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _make(B, N, seed, streams, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                              # (a second handle of a process orders its streams with events: the same results)
        return make_env(B, N, seed, contacts=True, streams=streams, obs=False, **kw)


def _stores(env, lib):
    """the device's manifold stores in the oracle's layout: [B, 4 + 16 MCR_CC_MAX] u32 — the four header words, then words 0 .. 15 of each of
    the `count` records (the device keeps MCR_CC_WORDS = 20 per record: k_carcontacts.h); and the raw stores [B, STORE_WORDS].  Synchronises."""
    raw = np.zeros((env.B, R.STORE_WORDS), np.uint32)
    assert lib.load().mcr_debug_read_contacts(env.h, lib.ptr(raw)) == 0
    out = np.zeros((env.B, 4 + 16 * R.CC_MAX), np.uint32)
    out[:, :4] = raw[:, :4]
    recs = raw[:, 4:].reshape(env.B, R.CC_MAX, R.CC_WORDS)[:, :, :16]
    for e in range(env.B):
        n = min(int(raw[e, 0]), R.CC_MAX)
        out[e, 4:4 + 16 * n] = recs[e, :n].reshape(-1)
    return out, raw


def _assert_store(got, want, what):
    """one env's device store against OracleEnv.car_contacts()"""
    n = int(want[0])
    assert int(got[0]) == n, f"{what}: {int(got[0])} manifolds stored, the oracle holds {n}; keys {C.decode_keys(got)} vs {C.decode_keys(want)}"
    assert int(got[1]) == int(want[1]), f"{what}: overflow mark {int(got[1])} vs the oracle's {int(want[1])}"
    if n == 0:
        return                                                       # (an env without a touching pair: the joint-order words are not rewritten)
    assert got[2:4].tolist() == want[2:4].tolist(), f"{what}: joint orders {got[2]:#x} {got[3]:#x} vs the oracle's {want[2]:#x} {want[3]:#x}"
    assert C.decode_keys(got) == C.decode_keys(want), f"{what}: keys in solve order {C.decode_keys(got)} vs the oracle's {C.decode_keys(want)}"
    g = got[4:4 + 16 * n].reshape(n, 16); w = want[4:4 + 16 * n].reshape(n, 16)
    if not np.array_equal(g, w):
        i, j = (int(v) for v in np.argwhere(g != w)[0])
        names = ("key", "type|n", "localNormal.x", "localNormal.y", "localPoint.x", "localPoint.y", "p0.x", "p0.y", "p0.nImp", "p0.tImp", "p0.id",
                 "p1.x", "p1.y", "p1.nImp", "p1.tImp", "p1.id")
        raise AssertionError(f"{what}: record {i} (key {C.decode_keys(got)[i]}, type|n {int(g[i, 1]):#x}) word {names[j]}: {int(g[i, j]):#010x} "
                             f"({g[i, j:j + 1].view(np.float32)[0]!r}) vs the oracle's {int(w[i, j]):#010x} ({w[i, j:j + 1].view(np.float32)[0]!r}); "
                             f"{int((g != w).sum())} words differ")


def run_case(torch, O, lib, cs, streams, each_step=None):
    """the case on the device and on its oracles in lockstep, everything compared; returns per step [B] manifold counts and the stores, and
    dict(rewards = per step [B, N], state = get_state() behind the last step).
    each_step(env, k, counts): extra checks behind step k."""
    B, N = len(cs["envs"]), cs["N"]
    env = _make(B, N, cs["seed"], streams); L = env.L
    fs = C.case_oracles(O, cs)
    counts_all, stores_all, rewards_all = [], [], []
    try:
        two = streams == 2 and bool(L.mcr_concurrent_collide(env.h))
        beside = 0
        for epi in range(cs["episodes"]):
            env.reset()
            if epi:
                for f in fs:
                    f.new_episode()
            spawn = env.get_state()["bodies"]
            for e, f in enumerate(fs):
                assert np.array_equal(spawn[e], f.o.state()["bodies"]), f"episode {epi} env {e}: the spawn poses differ"
            st = C.scene_bodies(cs, spawn)
            env.set_bodies(st)
            for e, f in enumerate(fs):
                C.set_oracle_bodies(f.o, st[e])
            status0 = env.status_words().copy()
            for k in range(cs["steps"]):
                a = C.actions(cs, k)
                _, rew, done, _ = env.step(torch.from_numpy(a).to(env.device))
                stores, _ = _stores(env, lib)
                rw = rew.cpu().numpy(); dn = done.cpu().numpy().astype(bool)
                want = []
                for e, f in enumerate(fs):
                    _, r, d, _ = f.o.step(a[e], render=False)
                    what = f"streams {streams} episode {epi} step {k} env {e}"
                    assert not d and not dn[e], f"{what}: the episode ended"
                    w = f.o.car_contacts(); want.append(w)
                    _assert_store(stores[e], w, what)
                    assert np.array_equal(r, rw[e]), f"{what}: rewards {rw[e].tolist()} vs the oracle's {r.tolist()}"
                n = np.array([int(w[0]) for w in want]); over = np.array([int(w[1]) for w in want])
                cnt = np.zeros(B, np.int32)
                assert L.mcr_debug_read_contact_counts(env.h, lib.ptr(cnt)) == 0
                assert cnt.tolist() == n.tolist(), f"streams {streams} episode {epi} step {k}: counts {cnt.tolist()} vs num_car_contacts {n.tolist()}"
                status = env.status_words().copy()
                assert (status[ST_CC_OVERFLOW] != status0[ST_CC_OVERFLOW]) == bool(over.any()), \
                    f"streams {streams} episode {epi} step {k}: ST_CC_OVERFLOW {status0[ST_CC_OVERFLOW]} -> {status[ST_CC_OVERFLOW]}, the oracle dropped pairs in envs {np.nonzero(over)[0].tolist()}"
                assert not cs["cap"] or k > 0 or over.any(), "a cap case that does not overflow in its first step"
                assert [int(v) for i, v in enumerate(status) if i != ST_CC_OVERFLOW] == [0] * 7, f"streams {streams} episode {epi} step {k}: status words {status.tolist()}"
                status0 = status
                assert env.verdict_mismatches() == 0
                if streams == 2:
                    part = np.zeros(B, np.uint8); clist = np.zeros(1 + B, np.int32)
                    assert L.mcr_debug_read_partition(env.h, lib.ptr(part), lib.ptr(clist)) == 0
                    assert (part != 0).tolist() == (n > 0).tolist(), f"streams 2 episode {epi} step {k}: partition {part.tolist()}, manifolds {n.tolist()}"
                    # the contact list names the same envs, in any order (verdict writers append to it); its COUNT reads 0 behind a fused step,
                    # whose contact chain empties it when it is through with the list (k_list_chain.h), the entries stay
                    nc = int((n > 0).sum())
                    assert int(clist[0]) in (0, nc) and sorted(clist[1:1 + nc].tolist()) == np.nonzero(n > 0)[0].tolist(), \
                        f"streams 2 episode {epi} step {k}: contact list {clist.tolist()}, envs with manifolds {np.nonzero(n > 0)[0].tolist()}"
                    beside += int(two and k > 0 and n.any())
                counts_all.append(n); stores_all.append(stores); rewards_all.append(rw)
                if each_step is not None:
                    each_step(env, k, n)
            assert_state(env, [(e, f.o) for e, f in enumerate(fs)], f"streams {streams} episode {epi}")
            final = env.get_state()
        if two:
            assert beside >= 2, "the contact pass never ran beside the dynamics on a step with contacts"
        print(f"(streams {streams}: contact pass beside the dynamics {two}, step ordering {int(L.mcr_step_ordering(env.h))})")
    finally:
        env.close()
        for f in fs:
            f.o.close()
    return counts_all, stores_all, dict(rewards=rewards_all, state=final)


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("name", list(C.CASES))
def test_contact_case_matches_the_oracle(torch_cuda, oracle, lib, name, streams):
    """Every case at both stream settings.  full2 fills a single-stream wavefront's LDS pool of 2 * MCR_CC_MAX constraint records exactly;
    full4 (N = 3: its four envs share one wavefront, 96 manifolds) is beyond it: the packed dynamics then steps the wavefront's envs two at a
    time (k_dynamics.h: k_dynamics_passes).  Before that it left envs 2 and 3 unsolved and wrote the overflow mark 2 into env 0's store."""
    cs = C.CASES[name]
    counts, _, _ = run_case(torch_cuda, oracle, lib, cs, streams)
    per_env = np.stack(counts).T
    print(f"{name} streams {streams}: manifolds per env and step {per_env.tolist()}")
    assert ((per_env[:, :cs['steps']] > 0).sum(1) >= 3).all()
    if name in ("full2", "full4"):
        assert counts[0].tolist() == [C.MCR_CC_MAX] * len(cs["envs"]), "full stores: a wavefront's LDS pool of 2 * MCR_CC_MAX records exactly full"


@pytest.mark.parametrize("streams", [1, 2])
def test_results_do_not_depend_on_who_shares_the_wavefront(torch_cuda, oracle, lib, streams):
    """The env with a full store (24 manifolds) alone, B = 1, and as env 1 of a batch beside envs with 24, 1 and 0 manifolds (the batch's seed
    is one lower, so that its env 1 plays the same episode): stores and rewards bit-identical step by step, the whole state at the end.
    At streams = 1 the batch's 49 manifolds are one more than the wavefront's LDS pool holds."""
    s24, s1 = C.COUNT_SCENES[24], C.COUNT_SCENES[1]
    alone = C.case(3, 310, [s24], steps=6)
    batch = C.case(3, 309, [s24, s24, s1, C.NONE3], steps=6)
    ca, sa, xa = run_case(torch_cuda, oracle, lib, alone, streams)
    cb, sb, xb = run_case(torch_cuda, oracle, lib, batch, streams)
    assert cb[0].tolist() == [24, 24, 1, 0] and ca[0].tolist() == [24]
    for k in range(6):
        n = int(ca[k][0])
        assert np.array_equal(sa[k][0][:4 + 16 * n], sb[k][1][:4 + 16 * n]), f"step {k}: the env's store depends on its neighbours"
        assert xa["rewards"][k][0].tobytes() == xb["rewards"][k][1].tobytes(), f"step {k}: the env's rewards depend on its neighbours"
    for name, a in xa["state"].items():
        assert a[0].tobytes() == xb["state"][name][1].tobytes(), f"the env's final {name} depend on its neighbours"


def test_next_verdicts_agree_with_the_next_contact_pass(torch_cuda, oracle, lib):
    """the straddling case at streams = 2: what this step's bookkeeping says about the next step's entry poses (mcr_debug_next_verdicts) is what
    the next step's contact pass finds, env by env, on both sides of the threshold"""
    cs = C.CASES["straddle"]
    seen = []

    def each_step(env, k, n):
        if seen:
            assert (seen[-1] != 0).tolist() == (n > 0).tolist(), f"step {k}: verdicts {seen[-1].tolist()}, the contact pass found {n.tolist()}"
        v = np.zeros(env.B, np.uint8)
        assert env.L.mcr_debug_next_verdicts(env.h, 0, lib.ptr(v)) == 0
        seen.append(v)

    counts, _, _ = run_case(torch_cuda, oracle, lib, cs, 2, each_step=each_step)
    assert (counts[0] > 0).tolist() == [True, False, True, False] and (counts[1] > 0).all()
    assert len(seen) == cs["steps"]


def test_contact_observation_equals_the_reference_on_the_store(torch_cuda, oracle, lib):
    """contact_obs on the N = 3 counts case: mask and impulse sums equal tests/contact_obs_ref.py applied to the store the oracle confirmed"""
    torch = torch_cuda
    cs = C.CASES["counts"]; B, N = len(cs["envs"]), cs["N"]
    env = _make(B, N, cs["seed"], 1, contact_obs=True)
    try:
        env.reset()
        env.set_bodies(C.scene_bodies(cs, env.get_state()["bodies"]))
        for k in range(3):
            env.step(torch.from_numpy(C.actions(cs, k)).to(env.device))
            _, raw = _stores(env, lib)
            mask, imp = R.contact_obs(raw, N)
            assert np.array_equal(env.contact_mask.cpu().numpy(), mask), f"step {k}: contact_mask"
            assert R.same_bits(env.contact_impulse.cpu().numpy(), imp), f"step {k}: contact_impulse"
            assert imp.max() > 0.0 and mask.any(1).all()
    finally:
        env.close()
