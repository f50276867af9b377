"""MI355X: the backward / on-grass bookkeeping of a phase-word step's main envs runs at the NEXT step's begin (csrc/k_flags.h, mcr_hip.hip:
step_phase_words) or, for anybody else who needs it, when that caller flushes it.  `driving_backward` / `driving_on_grass` and the HUD flag
pixels (step t + 1 shows step t's value) against the CPU oracle, on the three-chain handle, with and without reads in between, and across
everything that interrupts the chain of steps: an auto-reset, a masked reset, envs that move main -> contact list -> main, a switch to
graph replay and back, plain event-path steps on a stream that was never bound and back, a state blob round trip taken while a launch is
pending.  Every test asserts that its steps are on the path that defers the scans (phase words, contact pass beside the dynamics), and one
drops a pending launch (debug bit 20) to show that the values come through it."""
import ctypes

import numpy as np
import pytest

from tests.util import assert_pixels, env_streams, make_env, oracles, random_actions, rear_end_setup

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _assert_deferring(env, torch, stream=None):
    """the steps launched on `stream` (default: the current one) take the path that leaves the main envs' scans to their successor"""
    st = stream if stream is not None else torch.cuda.current_stream()
    assert env.L.mcr_step_ordering_for(env.h, ctypes.c_void_p(st.cuda_stream)) & 1, "the step orders its streams with events here: nothing is deferred"
    assert env.L.mcr_concurrent_collide(env.h), "the contact pass runs in front of the dynamics here: nothing is deferred"


def _assert_flags(env, orcs, what):
    es = env.get_env_state()                                        # (goes through the flush)
    for e, o in enumerate(orcs):
        eo = o.env_state()
        assert np.array_equal(es["driving_backward"][e], eo["driving_backward"]), f"{what} env {e}: driving_backward"
        assert np.array_equal(es["driving_on_grass"][e], eo["driving_on_grass"]), f"{what} env {e}: driving_on_grass"


def _seen(orcs):
    eo = [o.env_state() for o in orcs]
    return any(bool(x["driving_backward"].any()) for x in eo), any(bool(x["driving_on_grass"].any()) for x in eo)


@pytest.mark.parametrize("read_every_step", [True, False])
def test_flags_and_hud_pixels_with_and_without_reads_in_between(torch_cuda, oracle, read_every_step):
    """A rollout that turns round and leaves the road.  read_every_step: the flags of EVERY step through mcr_get_env_state (each read flushes
    the pending launch); otherwise nothing is read between the steps (the launch runs beside the next step's dynamics) and the HUD flag
    pixels of every frame must still show the previous step's flags."""
    torch = torch_cuda
    B, N, seed = 3, 2, 21
    env = make_env(B, N, seed, contacts=False, direction="CW", streams=2); env.reset()
    orcs = oracles(oracle, B, N, seed, contacts=False, direction="CW")
    rng = np.random.RandomState(2)
    back = grass = False
    for k in range(120):
        a = random_actions(rng, B, N, 0.0); a[..., 0] = 1.0 if k > 40 else a[..., 0]
        obs, _, _, _ = env.step(torch.from_numpy(a).cuda())
        for e, o in enumerate(orcs):
            o.step(a[e], render=True)
        _assert_deferring(env, torch)
        if read_every_step:
            _assert_flags(env, orcs, f"step {k}")
        assert_pixels(obs.cpu().numpy(), orcs, budget=40)
        b, g = _seen(orcs); back |= b; grass |= g
    assert back and grass, "scenario never set driving_backward / driving_on_grass"
    _assert_flags(env, orcs, "end")
    env.close()


def test_a_dropped_pending_launch_leaves_stale_flags(torch_cuda, oracle, lib):
    """The control: the same rollout, nothing read between the steps; at the first step that changes a flag, debug bit 20 makes the flush DROP
    the pending launch.  The flags then read are the previous step's — the step did leave its scans pending and the flush is what delivers
    them.  (With debug bit 19, scans in their step, the same read is right: the second half.)"""
    torch = torch_cuda
    B, N, seed = 3, 2, 21
    for in_step in (False, True):
        env = make_env(B, N, seed, contacts=False, direction="CW", streams=2); env.reset()
        orcs = oracles(oracle, B, N, seed, contacts=False, direction="CW")
        if in_step:
            lib.check(env.L.mcr_debug_set(env.h, lib.DEBUG_FLAGS_IN_STEP))
        rng = np.random.RandomState(2)
        prev = None
        for k in range(120):
            a = random_actions(rng, B, N, 0.0); a[..., 0] = 1.0 if k > 40 else a[..., 0]
            env.step(torch.from_numpy(a).cuda())
            for e, o in enumerate(orcs):
                o.step(a[e], render=False)
            _assert_deferring(env, torch)
            now = np.stack([np.stack([o.env_state()["driving_backward"], o.env_state()["driving_on_grass"]]) for o in orcs]).astype(np.uint8)
            if prev is not None and k > 3 and (now != prev).any():
                break
            prev = now
        else:
            raise AssertionError("scenario never changed a flag")
        torch.cuda.synchronize()
        lib.check(env.L.mcr_debug_set(env.h, lib.DEBUG_DROP_PENDING_FLAGS | (lib.DEBUG_FLAGS_IN_STEP if in_step else 0)))
        es = env.get_env_state()
        got = np.stack([np.stack([es["driving_backward"][e], es["driving_on_grass"][e]]) for e in range(B)]).astype(np.uint8)
        if in_step:
            assert np.array_equal(got, now), "scans in their step: nothing was pending, the flags are this step's"
        else:
            assert np.array_equal(got, prev) and not np.array_equal(got, now), "the dropped launch should have left the previous step's flags"
        env.close()


def test_flags_across_resets_path_switches_and_a_blob_round_trip(torch_cuda, oracle):
    """Auto-reset (TimeLimit), a masked reset, graph replay on and off, plain event-path steps (a caller stream that was never bound) and back
    to phase words, a get / set state blob round trip with a launch pending: the HUD flag pixels of every frame and the flags around every
    interruption equal the oracle's."""
    torch = torch_cuda
    B, N, seed, L = 4, 2, 77, 120
    env = make_env(B, N, seed, contacts=False, auto_reset=True, max_episode_steps=L, use_random_direction=True, streams=2)
    env.reset()
    torch.cuda.synchronize()
    bound, unbound = torch.cuda.Stream(), torch.cuda.Stream()     # (bound: not the null stream, which cannot be captured for graph replay)
    env._bound_streams.add(unbound.cuda_stream)                        # VecMultiCarRacing.step will not hand this one to mcr_bind_stream: events
    modes = set()
    streams, orcs = [], []
    for e in range(B):
        tr, gr = env_streams(seed, e)
        o = oracle.OracleEnv(N, car_contacts=False); o.reset(oracle.new_episode(N, tr, gr, use_random_direction=True))
        streams.append((tr, gr)); orcs.append(o)
    steps = np.zeros(B, np.int64)
    rng = np.random.RandomState(3)
    back = grass = False
    for k in range(270):
        a = random_actions(rng, B, N, 0.0); a[steps > 30, :, 0] = 1.0        # every episode turns round and leaves the road
        if k == 110:
            env.L.mcr_set_step_graph(env.h, 1)                         # graph replay: the step takes the event path from here ...
        if k == 140:
            env.L.mcr_set_step_graph(env.h, 0)                         # ... and the phase-word path again
        plain_events = 200 <= k < 212 or 250 <= k < 256                # un-captured step_events steps between phase-word steps
        st = unbound if plain_events else bound
        if k in (200, 212, 250, 256):
            torch.cuda.synchronize()                                   # (the caller orders its streams)
        with torch.cuda.stream(st):
            obs, _, done, _ = env.step(torch.from_numpy(a).cuda())
            dn = done.cpu().numpy()
            env.wait_refills()
            frames = obs.cpu().numpy()
            words = int(env.L.mcr_step_ordering_for(env.h, ctypes.c_void_p(st.cuda_stream))) & 1
            modes.add(("events" if plain_events else "graph" if 110 <= k < 140 else "words", words))
            if not plain_events and not 110 <= k < 140:
                _assert_deferring(env, torch, st)
            for e, o in enumerate(orcs):
                o.step(a[e], render=True); steps[e] += 1
                assert bool(dn[e]) == (steps[e] == L), f"step {k} env {e}: done"
                if steps[e] == L:                                          # TimeLimit: the env's next episode, first observation in this step's frame
                    o.reset(oracle.new_episode(N, *streams[e], use_random_direction=True)); steps[e] = 0
            assert_pixels(frames, orcs, budget=40)
            b, g = _seen(orcs); back |= b; grass |= g
            if k == 20:                                                    # a snapshot taken and restored while the step's launch is pending
                blob = env.get_state_blob(1); env.set_state_blob(1, blob)
                _assert_flags(env, orcs, "after the blob round trip")
            if k == 180:
                mask = np.array([1, 0, 1, 0], np.uint8)
                frames = env.reset_envs(torch.from_numpy(mask).cuda()).cpu().numpy()
                env.wait_refills()
                for e in (0, 2):
                    o2 = orcs[e].reset(oracle.new_episode(N, *streams[e], use_random_direction=True)); steps[e] = 0
                    d = (o2 != frames[e]).any(-1)
                    assert (d & (orcs[e].last_amb == 0)).sum() == 0
                _assert_flags(env, orcs, "after the masked reset")
            if k in (L - 1, L, 111, 141, 199, 200, 201, 211, 212, 213, 239, 240, 250, 256):
                _assert_flags(env, orcs, f"step {k}")
    assert back and grass, "scenario never set driving_backward / driving_on_grass"
    assert ("words", 1) in modes and ("events", 0) in modes and ("graph", 0) in modes and len(modes) == 3, f"the rollout did not see the three paths: {modes}"
    assert env.verdict_mismatches() == 0 and env.status_words()[:2].tolist() == [0, 0]
    env.close()


def test_flags_of_envs_that_move_between_the_main_launch_and_the_contact_list(torch_cuda, oracle):
    """Rear-end collisions: every env is the main launch's, then the contact chain's, then the main launch's again; flags and HUD pixels of
    every frame against the oracle (no reads in between but the last)."""
    torch = torch_cuda
    B, N, seed = 5, 2, 62
    env = make_env(B, N, seed, contacts=True, streams=2); env.reset()
    orcs = oracles(oracle, B, N, seed, contacts=True)
    rear_end_setup(env, orcs)
    rng = np.random.RandomState(4)
    touched = free_after = 0
    for k in range(160):
        a = random_actions(rng, B, N, 0.0)
        a[:, 0, 1] = 0.0; a[:, 0, 2] = 0.8 if k < 60 else 0.0          # car 0 brakes, then coasts
        a[:, 1, 0] *= 0.2; a[:, 1, 1] = 1.0                              # car 1 floors it
        if k > 100:
            a[:, 1, 0] = 1.0                                             # ... and turns away: onto the grass, facing backwards
        obs, rew, _, _ = env.step(torch.from_numpy(a).cuda())
        rw = rew.cpu().numpy()
        for e, o in enumerate(orcs):
            _, r, _, _ = o.step(a[e], render=True)
            n = o.num_car_contacts(); touched += n; free_after += 1 if (touched and not n) else 0
            assert np.array_equal(r, rw[e]), f"step {k} env {e}"
        _assert_deferring(env, torch)
        assert_pixels(obs.cpu().numpy(), orcs, budget=40)
        if k % 40 == 39:
            _assert_flags(env, orcs, f"step {k}")
    assert touched > 50 and free_after > 50, "scenario produced no car<->car contacts, or never left them"
    _assert_flags(env, orcs, "end")
    env.close()
