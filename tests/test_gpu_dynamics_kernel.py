"""MI355X: the per-car dynamics (csrc/k_dynamics.h) on the scenes of tests/dynamics_cases.py, in lockstep with the oracle and bit for bit
(tests/util.py: assert_state after EVERY step, the step's rewards and dones as well).  tests/test_dynamics_cases.py holds the scenes to
what they are named for, without a device.

  * wavefront compositions: two full wavefronts and a partial one at every N, each playing every role over six rounds — no limit anywhere,
    the only limit on a front (rear) joint of the first lane / the last real lane (beside a padding lane at N = 3 and 5), everything mixed —
    with car<->car contacts off and on, one stream and two; and with a touching pair in every wavefront (the contact form of the sweeps,
    which chooses its limited form by the same ballot).
  * the position loop at every pinned sweep count, two streams: the main launch parks exactly the envs the oracle's coverage says it must,
    the resume launch takes every one of them, nothing else moves in the status words; the frames of the parked envs are the oracle's.
  * tyre model, integration clamps and the sleep rule.
  * the controls: with the ablation bit DEBUG_POS_ITERS_2 the comparison fails in exactly the env-steps that need a third position sweep,
    with DEBUG_VEL_ITERS_2 in the wavefronts that run the contact form.  (Both bits only shorten loops.)"""
import ctypes

import numpy as np
import pytest

from tests import dynamics_cases as D
from tests.util import STATE_ARRAYS, assert_pixels, assert_state, make_env

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _path(env, torch):
    """how the env's steps are ordered here (recorded in failure messages, never asserted)"""
    st = torch.cuda.current_stream()
    words = int(env.L.mcr_step_ordering_for(env.h, ctypes.c_void_p(st.cuda_stream))) & 1
    return f"ordering {'phase words' if words else 'events'}, contact pass {'beside' if env.L.mcr_concurrent_collide(env.h) else 'in front of'} the dynamics"


def _compare(env, torch, run, rew, done, got, what):
    _, r, d, _ = got
    what = f"{what} [{_path(env, torch)}]"
    assert np.array_equal(r.cpu().numpy(), rew), f"{what}: rewards differ in envs {np.nonzero((r.cpu().numpy() != rew).any(1))[0].tolist()}"
    assert np.array_equal(d.cpu().numpy().astype(bool), done), f"{what}: dones differ"
    assert_state(env, enumerate(run.orcs), what)


def _differing(env, run):
    """[B] bool: the env's state differs from its oracle's somewhere"""
    st = env.get_state()
    return np.array([any(not np.array_equal(st[k][e], so[k]) for k in STATE_ARRAYS) for e, so in enumerate(o.state() for o in run.orcs)])


def _healthy(env, what):
    assert env.status_words().tolist() == [0] * 8, f"{what}: status words {env.status_words().tolist()}"
    assert env.verdict_mismatches() == 0, what


def _play_compositions(env, torch, run, N, rounds, what, touching=False, compare=True):
    """-> per (round, step): the oracles' coverage"""
    log = {}
    for k in rounds:
        edits, rl, _ = D.composition(N, k, touching=touching)
        run.teleport(edits)
        acts = D.composition_actions(N, k)
        for s in range(D.ROUND_STEPS):
            rew, done, got, _ = run.step(acts[s])
            log[(k, s)] = run.coverage()
            if touching and s == 0:
                assert all(run.orcs[e].num_car_contacts() > 0 for e in D.touching_envs(N)), f"{what} round {k}: the pairs do not touch"
            if compare:
                _compare(env, torch, run, rew, done, got, f"{what} round {k} {rl} step {s}")
    return log


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("contacts", [False, True], ids=["free", "contacts"])
@pytest.mark.parametrize("N", sorted(D.CONFIGS))
def test_wavefront_compositions_match_the_oracle(torch_cuda, oracle, N, contacts, streams):
    B = D.CONFIGS[N][1]
    env = make_env(B, N, D.SEED, contacts=contacts, obs=False, streams=streams); env.reset()
    run = D.Run(oracle, [D.scene("composition", N)] * B, contacts=contacts, env=env)
    try:
        _play_compositions(env, torch_cuda, run, N, range(D.ROUNDS), f"N {N} contacts {contacts} streams {streams}")
        _healthy(env, f"N {N} contacts {contacts} streams {streams}")
    finally:
        env.close(); run.close()


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("N", [2, 5])
def test_compositions_with_a_touching_pair_in_every_wavefront(torch_cuda, oracle, N, streams):
    B = D.CONFIGS[N][1]
    env = make_env(B, N, D.SEED, contacts=True, obs=False, streams=streams); env.reset()
    run = D.Run(oracle, [D.scene("composition", N)] * B, contacts=True, env=env)
    try:
        _play_compositions(env, torch_cuda, run, N, range(D.ROUNDS), f"N {N} touching streams {streams}", touching=True)
        _healthy(env, f"N {N} touching streams {streams}")
    finally:
        env.close(); run.close()


def _must_defer(cov, N):
    """an env-step the main launch has to park: some car neither solved nor stuck by its last granted sweep (a fixed point first seen on or
    before that sweep stops it there: the probe runs on it)"""
    return any(int(cov["sweeps"][c]) > D.DEFER_AFTER and not 0 < int(cov["fixed_at"][c]) <= D.DEFER_AFTER for c in range(N))


@pytest.mark.parametrize("N", [1, 2, 3])
def test_position_loop_scenes_park_and_resume(torch_cuda, oracle, N):
    """streams = 2: every step bit-exact; deferred == resumed; deferred >= the env-steps in which the oracle solved a car after more than
    MCR_DEFER_AFTER sweeps (such a car moved on every sweep: the main launch cannot have stopped it) and, where the step defers at all,
    == the env-steps that are neither solved nor at a fixed point by then — the fixed point inside the grant is NOT parked."""
    torch = torch_cuda
    scenes = D.position_scenes(N)
    env = make_env(len(scenes), N, D.SEED, contacts=False, obs=False, streams=2); env.reset()
    run = D.Run(oracle, scenes, env=env)
    try:
        before = env.debug_counters().copy()
        late = must = 0
        for k in range(run.steps):
            rew, done, got, _ = run.step()
            _compare(env, torch, run, rew, done, got, f"N {N} step {k}")
            for e, cov in enumerate(run.coverage()):
                for (kk, c), want in scenes[e]["pins"].items():
                    assert kk != k or D.outcome(cov, c) == want
                late += any(cov["solved"][c] and cov["sweeps"][c] > D.DEFER_AFTER for c in range(N))
                must += _must_defer(cov, N)
        deferred, resumed = (int(v) for v in (env.debug_counters() - before)[:2])
        what = f"N {N}: deferred {deferred} resumed {resumed}, oracle: solved late {late}, not through after {D.DEFER_AFTER} sweeps {must} [{_path(env, torch)}]"
        assert late > 0 and must >= late
        assert deferred == resumed, what
        print(what)
        if deferred == 0 and "phase words" not in _path(env, torch):
            print("this path does not defer; only the states were compared")
        else:
            assert late <= deferred == must, what
        _healthy(env, what)
    finally:
        env.close(); run.close()


def test_frames_of_parked_envs_are_the_resumed_state(torch_cuda, oracle):
    """N = 2, two streams, observations on: on the parking step the list raster draws the parked envs from the state the resume launch
    left, the main raster the others (two plain envs ride along)"""
    torch = torch_cuda
    scenes = D.position_scenes(2) + [D.scene("plain", 2, script=[(0, [0.3, 0.6, 0.0])]), D.scene("plain", 2, script=[(0, [-0.5, 1.0, 0.1])])]
    env = make_env(len(scenes), 2, D.SEED, contacts=False, streams=2); env.reset()
    run = D.Run(oracle, scenes, env=env)
    try:
        for k in range(2):
            rew, done, got, _ = run.step(render=True)
            _compare(env, torch, run, rew, done, got, f"frames step {k}")
            assert_pixels(got[0].cpu().numpy(), run.orcs)
            if k == 0:
                assert [_must_defer(c, 2) for c in run.coverage()] == [True] * 3 + [False] * 2
        _healthy(env, "frames")
    finally:
        env.close(); run.close()


@pytest.mark.parametrize("streams", [1, 2])
def test_tyre_clamp_and_sleep_scenes_match_the_oracle(torch_cuda, oracle, streams):
    for name, scenes in (("tyre", D.tyre_scenes()), ("sleep", D.sleep_scenes(1)), ("sleep N 2", D.sleep_scenes(2))):
        N = scenes[0]["N"]
        env = make_env(len(scenes), N, D.SEED, contacts=False, obs=False, streams=streams); env.reset()
        run = D.Run(oracle, scenes, env=env)
        try:
            slept = 0
            for k in range(run.steps):
                rew, done, got, _ = run.step()
                _compare(env, torch_cuda, run, rew, done, got, f"{name} streams {streams} step {k}")
                slept += sum(int(c["slept"].sum()) for c in run.coverage())
            assert name == "tyre" or slept == sum(len(v) for sc in scenes for v in sc["want"]["slept"].values())
            _healthy(env, f"{name} streams {streams}")
        finally:
            env.close(); run.close()


def test_two_position_sweeps_fail_exactly_where_a_third_is_needed(torch_cuda, oracle, lib):
    """The control for the position loop: with DEBUG_POS_ITERS_2 (the loop stops after two sweeps) an env's state leaves the oracle's in the
    first step in which one of its cars needs a third sweep that moves something — three or more sweeps on the oracle, unless it sat at a
    fixed point by the second (then two sweeps give the very same poses, and `unsolved` either way) — and in no step before."""
    torch = torch_cuda
    scenes = D.position_scenes(1)
    env = make_env(len(scenes), 1, D.SEED, contacts=False, obs=False); env.reset()
    lib.check(env.L.mcr_debug_set(env.h, lib.DEBUG_POS_ITERS_2))
    run = D.Run(oracle, scenes, env=env)
    try:
        off = np.zeros(len(scenes), bool); hit = 0
        for k in range(run.steps):
            run.step()
            needs = np.array([int(c["sweeps"][0]) >= 3 and not 0 < int(c["fixed_at"][0]) <= 2 for c in run.coverage()])
            diff = _differing(env, run)
            fresh = ~off
            assert np.array_equal(diff[fresh], needs[fresh]), \
                f"step {k}: envs that differ {np.nonzero(diff & fresh)[0].tolist()}, envs that need a third sweep {np.nonzero(needs & fresh)[0].tolist()} [{_path(env, torch)}]"
            hit += int((needs & fresh).sum()); off |= needs
        assert hit >= 17 and (~off).sum() >= 4, (hit, off.tolist())
    finally:
        env.close(); run.close()


def test_two_velocity_sweeps_fail_in_the_wavefronts_of_the_contact_form(torch_cuda, oracle, lib):
    """The control for the velocity sweeps: DEBUG_VEL_ITERS_2 shortens the sweeps of the contact form (a wavefront that holds a touching
    pair; the contact-free form has no such switch).  One stream, N = 2, a touching pair in every wavefront: after the first step of the
    round whose wavefronts hold a limit, cars with a joint at its limit differ from the oracle — and without the bit nothing does
    (test_compositions_with_a_touching_pair_in_every_wavefront)."""
    torch = torch_cuda
    N = 2; B = D.CONFIGS[N][1]
    env = make_env(B, N, D.SEED, contacts=True, obs=False, streams=1); env.reset()
    lib.check(env.L.mcr_debug_set(env.h, lib.DEBUG_VEL_ITERS_2))
    run = D.Run(oracle, [D.scene("composition", N)] * B, contacts=True, env=env)
    try:
        k = 1                                                   # front_first | rear_last | front_first: a limit in every wavefront
        edits, rl, limited = D.composition(N, k, touching=True)
        assert len(limited) == 3
        run.teleport(edits); run.step(D.composition_actions(N, k)[0])
        diff = _differing(env, run)
        assert all(diff[e] for e, _, _ in limited.values()), f"{rl}: envs that differ {np.nonzero(diff)[0].tolist()}, limited {limited} [{_path(env, torch)}]"
        assert all(diff[e] for e in D.touching_envs(N))
    finally:
        env.close(); run.close()
