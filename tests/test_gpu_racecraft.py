"""MI355X: VecMultiCarRacing(scripted_agents=all, racecraft=True) in lockstep with the CPU oracle driven by the float64 restatement
(tests/racecraft_ref.py) — actions, rewards and the final state BIT-EXACT.  The episodes are those of tests/test_racecraft_scenario.py
(seed 500, random direction) with its parameter split — car 0 at half the default v_max, the others at the defaults — so that within
150 steps a fast car comes up behind the slow one, side-steps and is held by the follow rule; the oracle side asserts through
racecraft_ref's branches that both happened."""
import numpy as np
import pytest

from tests import driver_ref as D
from tests import racecraft_ref as R
from tests.util import STATE_ARRAYS, assert_f32_bits, assert_state, make_env, oracle_episode

pytestmark = pytest.mark.gpu

SEED, B, STEPS = D.SCENARIO_SEED, 6, 150


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def split_rows(N):
    q = D.default_params(N)
    q[0, D.V_MAX] = np.float32(D.DEFAULTS[D.V_MAX] / 2)
    return q


def oracles(oracle, N):
    eps = [oracle_episode(oracle, N, SEED, e, use_random_direction=True) for e in range(B)]
    orcs = [oracle.OracleEnv(N) for _ in range(B)]
    for o, ep in zip(orcs, eps):
        o.reset(ep, render=False)
    return orcs, eps


def want_actions(L, orcs, eps, prm, rc, mask, fired=None):
    out = []
    for o, ep in zip(orcs, eps):
        reps = []
        out.append(R.of_oracle(L, o, ep, prm, rc, mask, reps))
        if fired is not None:
            for rep in reps:
                if rep is not None:
                    fired |= {k for k, v in rep.items() if (v is not None if k == "leader" else bool(v))}
    return np.stack(out)


@pytest.mark.parametrize("N,frame_skip", [(2, 1), (3, 1), (2, 2)])
def test_closed_loop_bit_exact_vs_oracle(torch_cuda, oracle, lib, N, frame_skip):
    torch = torch_cuda
    L = lib.load()
    prm, rc, mask = split_rows(N), R.default_params(N), (1 << N) - 1
    env = make_env(B, N, SEED, streams=1, obs=False, use_random_direction=True, scripted_agents=range(N), driver_params=prm, racecraft=True,
                   frame_skip=frame_skip)
    assert np.array_equal(env.racecraft_params, rc) and env.racecraft_agents == tuple(range(N))
    env.reset()
    orcs, eps = oracles(oracle, N)
    zeros = torch.zeros((B, N, 3), device="cuda")
    fired = set()
    for k in range(STEPS // frame_skip):
        want = want_actions(L, orcs, eps, prm, rc, mask, fired)
        _, rew, done, info = env.step(zeros)
        assert_f32_bits(info["actions"].cpu().numpy(), want, f"step {k}")
        total = None
        for _ in range(frame_skip):
            _, _, r, d = oracle.step_batch(orcs, want, None, threads=4)
            assert not d.any(), "an episode ended: the stretch is meant to stay inside one"
            total = r.copy() if total is None else total + r
        assert np.array_equal(rew.cpu().numpy(), total), f"step {k}: rewards"
        assert not bool(done.any())
    print("branches fired:", sorted(fired))
    assert "follow" in fired and ({"step_left", "step_right"} & fired), f"the stretch was meant to hold a side-step and a follow phase: {sorted(fired)}"
    assert_state(env, enumerate(orcs), f"after {STEPS} env steps")
    assert_f32_bits(env.expert_actions().cpu().numpy(), want_actions(L, orcs, eps, prm, rc, mask), "expert_actions() at the end")
    assert env.status_words()[:5].tolist() == [0] * 5
    env.close()
    for o in orcs:
        o.close()


def test_expert_actions_with_a_learner_in_front(torch_cuda, oracle, lib):
    """N = 2, only car 1 scripted and racing, car 0 the caller's (slow, straight): info["actions"] row 0 is the caller's, row 1 the
    restatement's with car 0 seen as a leader; expert_actions() is the restatement for EVERY car — racecraft for car 1, the plain
    controller for car 0"""
    torch = torch_cuda
    L = lib.load()
    N = 2
    prm, rc = D.default_params(N), R.default_params(N)
    env = make_env(B, N, SEED, streams=1, obs=False, use_random_direction=True, scripted_agents=(1,), racecraft=True)
    assert env.racecraft_agents == (1,)
    env.reset()
    orcs, eps = oracles(oracle, N)
    mine = np.zeros((B, N, 3), np.float32); mine[:, 0, 1] = 0.1
    fired = set()
    for k in range(STEPS):
        want = want_actions(L, orcs, eps, prm, rc, 0b10, fired); want[:, 0] = mine[:, 0]
        if k % 25 == 0:
            assert_f32_bits(env.expert_actions().cpu().numpy(), want_actions(L, orcs, eps, prm, rc, 0b10), f"step {k}: expert_actions()")
        _, _, _, info = env.step(torch.from_numpy(mine).cuda())
        assert_f32_bits(info["actions"].cpu().numpy(), want, f"step {k}")
        oracle.step_batch(orcs, want, None, threads=4)
    assert "leader" in fired and ({"step_left", "step_right"} & fired), f"car 1 was meant to see the caller's car and side-step: {sorted(fired)}"
    assert_state(env, enumerate(orcs), f"after {STEPS} steps")
    env.close()
    for o in orcs:
        o.close()


def test_snapshot_reproduces_the_actions(torch_cuda):
    """save_states(), 40 steps, load_states(), the same 40 steps again: the same actions and states — nothing but the env's state feeds the
    controller"""
    torch = torch_cuda
    N = 2
    env = make_env(B, N, SEED, streams=1, obs=False, use_random_direction=True, scripted_agents=(0, 1), driver_params=split_rows(N), racecraft=True)
    env.reset()
    zeros = torch.zeros((B, N, 3), device="cuda")
    for _ in range(40):
        env.step(zeros)
    snap = env.save_states()

    def run():
        acts = []
        for _ in range(40):
            env.step(zeros); acts.append(env.actions.clone())
        return torch.stack(acts), env.get_state()
    a1, s1 = run()
    env.load_states(snap)
    a2, s2 = run()
    assert torch.equal(a1.view(torch.int32), a2.view(torch.int32)) and bool((a1[:, :, 0] != a1[:, :, 1]).any())
    for key in STATE_ARRAYS:
        assert np.array_equal(s1[key], s2[key]), key
    env.close()
