"""MI355X: the wheel<->tile sensor pass of csrc/k_collide.h — block culling, the candidate list and its mid-loop flushes, the overlap items, the
per-tile begin / end state, the begin-event queue and its replay in Box2D's order — on the scenes of tests/tile_cases.py, in lockstep with the
oracle: three episodes on one handle, env e playing scene (e + k) % B in its k-th episode.  tests/test_tile_cases.py holds the scenes to the
counts they are named for (65 .. 128 begin events in one pass, 128 exactly, 129, 185 and more; 150 and 280 candidates; five and more blocks,
block 31, a one-tile last block, blocks visited through touch_blocks or the moved-proxy margin alone; past = N - 1; orders the batch stamps
decide), without a device.

While an env's episode has stayed at or below EVQ_CAP = 128 begin events per pass, its reset pass included, every step is compared bit for bit
(tests/util.py: assert_state — bodies, joints, wheels, limit states, on-road bits, sleep, rewards, visit counts, every tile's visited and
touched bits, T, t), the step's reward and `done` as well, and the device's per-tile wheel bits (mcr_debug_read_tile_touch) with the oracle's.
From the first pass beyond the cap to the episode's end the kept events are whichever won the queue's atomicAdd: only what does not pass
through the queue is compared (bodies .. sleep, the wheel bits, T, t), and what holds whichever events were kept — visited bits a subset of the
oracle's, tile_visited_count the popcount of the device's own bits, the env's rewards summed over its cars not above the oracle's (a car alone may
get MORE than the oracle gives it: a dropped event of another car lowers its `past`).  Status word 3 (ST_EVENT_OVERFLOW) moves in exactly the
resets and steps in which some env's pass held more than 128 events on the oracle.  The env that overflowed plays another scene in its next
episode, bit-exact again."""
import warnings

import numpy as np
import pytest

from tests import tile_cases as T
from tests.util import STATE_ARRAYS, assert_state, make_env

pytestmark = pytest.mark.gpu
ST_CC_OVERFLOW, ST_EVENT_OVERFLOW = 2, 3
GROUPS = T.groups()
CASES = [(key, 1) for key in GROUPS] + [(key, 2) for key, g in GROUPS.items() if any(s["streams2"] for s in g)]


def _touch(env, lib):
    out = np.zeros((env.B, T.TILE_CAP), np.uint32)
    assert lib.load().mcr_debug_read_tile_touch(env.h, lib.ptr(out)) == 0
    return out


def _compare(env, lib, e, o, exact, what):
    """env e against its oracle after a reset or a step; returns the device's per-tile wheel bits of the env"""
    touch = _touch(env, lib)[e, :o.T]
    want = o.wheel_touch()
    assert np.array_equal(touch, want), f"{what}: wheel bits of tiles {np.nonzero(touch != want)[0][:8].tolist()} differ"
    counts = np.array([[int(((touch >> (c * 4 + w)) & 1).sum()) for w in range(4)] for c in range(o.N)])
    assert np.array_equal(counts, o.wheel_tile_counts()), f"{what}: tiles under each wheel {counts.tolist()} vs {o.wheel_tile_counts().tolist()}"
    if exact:
        assert_state(env, [(e, o)], what)
        return
    st = env.get_state(); es = env.get_env_state(); so = o.state(); eo = o.env_state()
    for k in STATE_ARRAYS:
        assert np.array_equal(st[k][e], so[k]), f"{what} (beyond the cap): {k} differs"
    assert es["num_tiles"][e] == o.T and es["t"][e] == eo["t"]
    visited = (es["tile_flags"][e, :o.T] & 0xff).astype(np.uint8)
    assert not (visited & ~eo["visited"]).any(), f"{what}: visited bits the oracle does not hold"
    own = [int(((visited >> c) & 1).sum()) for c in range(o.N)]
    assert es["tile_visited_count"][e].tolist() == own, f"{what}: visit counts {es['tile_visited_count'][e].tolist()}, the device's own bits give {own}"
    assert es["reward"][e].sum() <= eo["reward"].sum() + 1e-9, f"{what}: rewards {es['reward'][e].tolist()} vs the oracle's {eo['reward'].tolist()}"


@pytest.mark.parametrize("key,streams", CASES, ids=[f"N{k[0]}-{'contacts' if k[1] else 'free'}-streams{s}" for k, s in CASES])
def test_scenes_match_the_oracle(oracle, lib, key, streams):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    N, contacts = key
    group = [s for s in GROUPS[key] if streams == 1 or s["streams2"]]
    B = len(group)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                    # (the overflow words are this test's subject: it reads them itself)
        env = make_env(B, N, 0, contacts=contacts, levels=T.blobs_of(lib, group), level_order="cycle", obs=False, streams=streams)
    twins = [T.Twin(oracle, lib, group, e) for e in range(B)]
    overflowed = []
    try:
        status = env.status_words().copy()

        def check_status(over, cc_over, what):
            nonlocal status
            now = env.status_words().copy()
            assert (now[ST_EVENT_OVERFLOW] != status[ST_EVENT_OVERFLOW]) == bool(over), \
                f"{what}: ST_EVENT_OVERFLOW {status[ST_EVENT_OVERFLOW]} -> {now[ST_EVENT_OVERFLOW]}, envs beyond the cap on the oracle {over}"
            assert now[ST_CC_OVERFLOW] == status[ST_CC_OVERFLOW] or cc_over, f"{what}: ST_CC_OVERFLOW moved, the oracle dropped no pair"
            rest = [i for i in range(8) if i not in (ST_CC_OVERFLOW, ST_EVENT_OVERFLOW)]
            assert now[rest].tolist() == status[rest].tolist(), f"{what}: status words {status.tolist()} -> {now.tolist()}"
            status = now

        for epi in range(T.EPISODES):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                env.reset()
            scenes = [tw.reset() for tw in twins]
            assert env.level.cpu().tolist() == [(e + epi) % B for e in range(B)]
            exact = [tw.o.begin_events()[0] <= T.EVQ_CAP for tw in twins]
            check_status([e for e in range(B) if not exact[e]], [e for e, tw in enumerate(twins) if contacts and tw.o.car_contacts()[1]], f"episode {epi} reset")
            for e, tw in enumerate(twins):
                _compare(env, lib, e, tw.o, exact[e], f"streams {streams} episode {epi} env {e} ({scenes[e]['name']}) after reset")
            for k in range(T.STEPS):
                if k in (0, T.PLACE, T.LEAVE):
                    bodies = []
                    for e, tw in enumerate(twins):
                        tp = T.teleports(lib, scenes[e], k)
                        b = tw.o.state()["bodies"] if tp is None else T.teleport(lib, tw.o.state()["bodies"], tp)
                        T.set_oracle_bodies(tw.o, b); bodies.append(b)
                    env.set_bodies(np.stack(bodies))
                a = np.stack([T.actions(sc, k) for sc in scenes])
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    _, rew, done, _ = env.step(torch.from_numpy(a).to(env.device))
                rw = rew.cpu().numpy(); dn = done.cpu().numpy().astype(bool)
                over, cc_over = [], []
                for e, tw in enumerate(twins):
                    what = f"streams {streams} episode {epi} step {k} env {e} ({scenes[e]['name']})"
                    _, r, d, _ = tw.o.step(a[e], render=False)
                    assert not d and not dn[e], f"{what}: the episode ended"
                    n = tw.o.begin_events()[0]
                    if n > T.EVQ_CAP:
                        over.append(e); overflowed.append((epi, k, e, n))
                        if exact[e]:                # the state was the oracle's until this pass: this step's rewards cannot exceed the oracle's
                            assert rw[e].sum() <= r.sum() + 1e-9, f"{what}: step rewards {rw[e].tolist()} vs the oracle's {r.tolist()}"
                        exact[e] = False
                    elif exact[e]:
                        assert np.array_equal(r, rw[e]), f"{what}: rewards {rw[e].tolist()} vs the oracle's {r.tolist()}"
                    if contacts and tw.o.car_contacts()[1]:
                        cc_over.append(e)
                    _compare(env, lib, e, tw.o, exact[e], what)
                check_status(over, cc_over, f"streams {streams} episode {epi} step {k}")
            assert env.verdict_mismatches() == 0
        want_over = any(s["want"].get("max_events", 0) > T.EVQ_CAP for s in group)
        assert bool(overflowed) == want_over, f"passes beyond the cap (episode, step, env, events): {overflowed}"
        print(f"N {N} contacts {contacts} streams {streams}: passes beyond the cap (episode, step, env, events) {overflowed}; "
              f"contact pass beside the dynamics {bool(env.L.mcr_concurrent_collide(env.h))}")
    finally:
        env.close()
        for tw in twins:
            tw.close()
