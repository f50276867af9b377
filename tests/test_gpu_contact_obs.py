"""MI355X: the car-contact observation through VecMultiCarRacing(contact_obs=True): `contact_mask` / `contact_impulse` against the host
definition (tests/contact_obs_ref.py) applied to the device's own manifold stores (mcr_debug_read_contacts), bit for bit, and — independently
of those stores — against the oracle's count of touching manifolds; frame_skip's chain of adds against a frame_skip = 1 twin; snapshots; and
the feature switched off.  Every scenario asserts that it is not trivial: the observed counts stand in the comments."""
import warnings

import numpy as np
import pytest

from tests import contact_obs_ref as R
from tests.util import drive_actions, make_env, oracles, random_actions, rear_end_setup

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _stores(env, lib):
    """the raw manifold stores [B, STORE_WORDS] u32 (synchronises)"""
    out = np.zeros((env.B, R.STORE_WORDS), np.uint32)
    assert lib.load().mcr_debug_read_contacts(env.h, lib.ptr(out)) == 0
    return out


def _tensors(env):
    return env.contact_mask.cpu().numpy(), env.contact_impulse.cpu().numpy()


def _assert_rows(got, want, what):
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64
    assert np.array_equal(got[0], want[0]), f"{what}: contact_mask {got[0].tolist()} vs the reference on the store {want[0].tolist()}"
    assert R.same_bits(got[1], want[1]), f"{what}: contact_impulse differs from the reference on the store in envs {np.nonzero((got[1].view(np.uint64) != want[1].view(np.uint64)).any((1, 2)))[0][:8].tolist()}"


def _rear_end_actions(rng, B, k):
    a = random_actions(rng, B, 2, 0.0)
    a[:, 0, 1] = 0.0; a[:, 0, 2] = 0.8                               # car 0 brakes
    a[:, 1, 0] *= 0.2; a[:, 1, 1] = 1.0                              # car 1 floors it
    return a


def _make(B, N, seed, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                              # (a second handle of a process orders its streams with events: the same results)
        return make_env(B, N, seed, **kw)


# ---------------------------------------------------------------------------------------------------------------- 1. rear-end collisions, N = 2
@pytest.mark.parametrize("B,streams", [(5, 1), (67, None)])
def test_rear_end_matches_the_store_and_the_oracle(torch_cuda, oracle, lib, B, streams):
    """Car 1 runs into the braking car 0, in lockstep with the oracle.  B = 5 on one stream; B = 67 with the default two, where the envs
    with a touching pair run in the contact chain of the three-chain step.  Oracle alone, 40 steps at gap 5.2: every env touches from step
    3 on (37 env-steps each), one manifold at a time, no episode ends.  Observed on the device: 37 env-steps with contact per env, every one
    of them with a two-point manifold (185 at B = 5, 2479 at B = 67), largest impulse sum 19.178."""
    torch = torch_cuda
    N, seed, steps = 2, 62, 40
    env = _make(B, N, seed, contacts=True, streams=streams, obs=False, contact_obs=True); env.reset()
    assert env.contact_mask.shape == (B, N) and env.contact_impulse.shape == (B, N, N)
    if streams is None:
        assert int(env.L.mcr_step_ordering(env.h)) != 0, "B = 67 is meant to run the three-chain step"
    _assert_rows(_tensors(env), (np.zeros((B, N), np.int32), np.zeros((B, N, N))), "after reset")
    orcs = oracles(oracle, B, N, seed, contacts=True)
    rear_end_setup(env, orcs)
    rng = np.random.RandomState(4)
    contact_steps = np.zeros(B, int); two_points = 0; hardest = 0.0
    for k in range(steps):
        a = _rear_end_actions(rng, B, k)
        _, rew, done, info = env.step(torch.from_numpy(a).cuda())
        assert info["contact_mask"] is env.contact_mask and info["contact_impulse"] is env.contact_impulse
        got = _tensors(env); dn = done.cpu().numpy().astype(bool); rw = rew.cpu().numpy()
        stores = _stores(env, lib)
        _assert_rows(got, R.contact_obs(stores, N), f"step {k}")
        for e, o in enumerate(orcs):
            _, r, d, _ = o.step(a[e], render=False)
            assert np.array_equal(r, rw[e]) and bool(d) == dn[e], f"step {k} env {e}: the env left the oracle"
            if dn[e]:
                continue
            touching = o.num_car_contacts() > 0                      # touching car<->car manifolds of the step the oracle just took: what the store counts
            assert ((got[0][e, 0] & 0xff) != 0) == touching, f"step {k} env {e}: mask {got[0][e].tolist()}, the oracle's manifolds {o.num_car_contacts()}"
            if touching:
                assert got[0][e, 0] & 0xff == 0b10 and got[0][e, 1] & 0xff == 0b01, f"step {k} env {e}: {got[0][e].tolist()}"
                assert got[0][e, 0] >> 8 and got[0][e, 1] >> 8, "a touching car names its own fixture's kind"
                contact_steps[e] += 1
                two_points += any(len(r[4]) == 2 for r in R.decode(stores[e]))
            else:
                assert not got[0][e].any() and not got[1][e].any()
        hardest = max(hardest, float(got[1].max()))
    print(f"B {B}: env-steps with contact per env {contact_steps.min()}..{contact_steps.max()}, with a two-point manifold {two_points}, largest impulse sum {hardest:.3f}")
    assert contact_steps.min() >= 1, f"an env never touched: {contact_steps.tolist()}"
    assert two_points >= 1, "no env-step with a two-point manifold"
    assert hardest > 0.0, "no normal impulse was ever applied"
    assert env.status_words()[:5].tolist() == [0] * 5 and env.verdict_mismatches() == 0
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 2. N = 3 and N = 8
@pytest.mark.parametrize("N,seed", [(3, 71), (8, 72)])
def test_pile_up_matches_the_store(torch_cuda, lib, N, seed):
    """All cars leave the grid at full throttle, the even ones steering into the odd ones (util.drive_actions).  Oracle alone with the same
    policy, 60 steps: N = 3 first manifold at step 30 in two of the three envs, up to 4 at a time; N = 8 at steps 25-51 in all three, up to 6.
    Observed on the device (its own steering noise): N = 3 31 steps with a contact, cars (1, 2) in env 0 and (0, 1) in env 2; N = 8 35 steps,
    cars (3, 7) in env 0, (4, 5) in env 1, (1, 4) and (3, 6) in env 2: four distinct pairs."""
    torch = torch_cuda
    B, steps = 3, 60
    env = _make(B, N, seed, contacts=True, obs=False, contact_obs=True); env.reset()
    gen = torch.Generator(device="cuda"); gen.manual_seed(seed)
    pairs = set(); touched_steps = 0
    for k in range(steps):
        _, _, done, _ = env.step(drive_actions(torch, gen, B, N, k))
        mask, imp = _tensors(env)
        stores = _stores(env, lib)
        _assert_rows((mask, imp), R.contact_obs(stores, N), f"step {k}")
        assert not done.any().item()
        for e in range(B):
            for a in range(N):
                assert imp[e, a, a] == 0.0 and not (mask[e, a] >> a) & 1, f"step {k} env {e} car {a}: the diagonal"
                for j in range(N):
                    assert ((mask[e, a] >> j) & 1) == ((mask[e, j] >> a) & 1), f"step {k} env {e}: bit {j} of car {a} without bit {a} of car {j}"
                    if (mask[e, a] >> j) & 1:
                        pairs.add((e, min(a, j), max(a, j)))
            assert R.same_bits(imp[e], imp[e].T.copy())
        touched_steps += int(mask.any())
    assert touched_steps >= 1, "the pile-up produced no car<->car contact"
    if N == 8:
        assert len({p[1:] for p in pairs}) >= 2, f"fewer than two distinct pairs of cars touched: {sorted(pairs)}"
    print(f"N {N}: steps with a contact {touched_steps}, (env, car, car) that touched {sorted(pairs)}")
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 3. frame_skip
def test_frame_skip_sums_the_sub_steps_in_one_chain(torch_cuda, lib):
    """frame_skip = 4 against a frame_skip = 1 twin (same seed, same actions, stepped four times): the macro-step's rows are the reference's
    ONE chain of adds over the twin's four stores, in step order.  The rear-end run: touching from step 3 on, so macro-step 0 reports one
    sub-step and every later one sums four; no episode ends in the 10 macro-steps.  Observed: 9 macro-steps sum four sub-steps."""
    torch = torch_cuda
    B, N, seed, K, macros = 5, 2, 62, 4, 10
    skip = _make(B, N, seed, contacts=True, streams=1, obs=False, contact_obs=True, frame_skip=K); skip.reset()
    twin = _make(B, N, seed, contacts=True, streams=1, obs=False, contact_obs=True); twin.reset()
    rear_end_setup(skip, []); rear_end_setup(twin, [])
    rng = np.random.RandomState(4)
    summed = 0; chain_differs = 0
    for m in range(macros):
        a = torch.from_numpy(_rear_end_actions(rng, B, m)).cuda()
        _, rew, done, _ = skip.step(a)
        rows = []; total = torch.zeros_like(rew); per_step_sum = np.zeros((B, N, N))
        for s in range(K):
            _, r1, d1, _ = twin.step(a)
            assert not d1.any().item(), "the comparison ends at the first done: this run has none"
            stores = _stores(twin, lib)
            _assert_rows(_tensors(twin), R.contact_obs(stores, N), f"twin macro-step {m} sub-step {s}")
            rows.append((stores, N, None)); total += r1
            per_step_sum = per_step_sum + twin.contact_impulse.cpu().numpy()
        assert torch.equal(rew, total) and not done.any().item()
        want = R.accumulate_steps(rows)
        _assert_rows(_tensors(skip), want, f"macro-step {m}")
        touching = sum(int(R.contact_obs(st, N)[0].any()) for st, _, _ in rows)
        summed += touching >= 2
        chain_differs += not R.same_bits(want[1], per_step_sum)      # (the sum of the per-step sums is another association of the same adds)
    assert summed >= 1, "no macro-step summed contact from two or more sub-steps"
    print(f"macro-steps summing two or more sub-steps {summed}, of which the chain differs from the sum of the steps' sums in {chain_differs}")
    skip.close(); twin.close()


def test_frame_skip_never_reports_the_ending_sub_step(torch_cuda, lib):
    """max_episode_steps = 6, auto-reset, hulls overlapping from the start (gap 4.9: a manifold in every step).  The first macro-step sums
    steps 1-4.  In the second every env is truncated in sub-step 1 (step 6), is parked, and re-spawns in sub-step 3: that call's rows are the
    twin's step-5 rows alone — step 6, the ending one, is not reported, and the new episode adds nothing.  The twin's own step 6 (done, re-spawned
    in the step) shows the first state of the new episode: no contact."""
    torch = torch_cuda
    B, N, seed, K = 5, 2, 62, 4
    kw = dict(contacts=True, streams=1, obs=False, contact_obs=True, auto_reset=True, max_episode_steps=6)
    skip = _make(B, N, seed, frame_skip=K, **kw); skip.reset()
    twin = _make(B, N, seed, **kw); twin.reset()
    rear_end_setup(skip, [], gap=4.9); rear_end_setup(twin, [], gap=4.9)
    rng = np.random.RandomState(4)
    a = torch.from_numpy(_rear_end_actions(rng, B, 0)).cuda()
    # ---- macro-step 1 = steps 1 .. 4
    _, _, done, _ = skip.step(a)
    rows = []
    for s in range(K):
        _, _, d1, _ = twin.step(a)
        assert not d1.any().item()
        rows.append((_stores(twin, lib), N, None))
        assert R.contact_obs(rows[-1][0], N)[0].all(), f"step {s + 1}: every env touches"
    assert not done.any().item()
    _assert_rows(_tensors(skip), R.accumulate_steps(rows), "macro-step 1")
    # ---- macro-step 2 = step 5, step 6 (truncated), parked, re-spawn
    _, _, done, info = skip.step(a)
    assert done.all().item() and info["TimeLimit.truncated"].all().item()
    _, _, d1, _ = twin.step(a)
    assert not d1.any().item()
    step5 = _tensors(twin)
    assert step5[0].all() and (step5[1][:, 0, 1] > 0).all(), "step 5 holds a contact with an impulse in every env"
    _assert_rows(_tensors(skip), step5, "macro-step 2: the twin's step-5 rows alone")
    _, _, d1, _ = twin.step(a)
    assert d1.all().item()
    _assert_rows(_tensors(twin), (np.zeros((B, N), np.int32), np.zeros((B, N, N))), "the twin's step 6: the new episode's first state")
    skip.close(); twin.close()


# ---------------------------------------------------------------------------------------------------------------- 4. snapshots
def test_restore_and_clone_recompute_the_rows(torch_cuda, lib):
    """save_states with live contacts, step on, load_states: the rows are the reference on the RESTORED store (what the saved state's last step
    produced), not the later step's; clone_envs: the clone's rows equal its source's.  Then both go on bit for bit like the original."""
    torch = torch_cuda
    B, N, seed = 5, 2, 62
    env = _make(B, N, seed, contacts=True, streams=1, obs=False, contact_obs=True); env.reset()
    rear_end_setup(env, [], gap=4.9)
    rng = np.random.RandomState(4)
    acts = [torch.from_numpy(_rear_end_actions(rng, B, k)).cuda() for k in range(12)]
    for k in range(4):
        env.step(acts[k])
    saved_rows, saved_stores = _tensors(env), _stores(env, lib)
    assert saved_rows[0].all() and (saved_rows[1][:, 0, 1] > 0).all(), "the snapshot is taken with live contacts"
    blobs = env.save_states()
    later = []
    for k in range(4, 8):
        env.step(acts[k]); later.append(_tensors(env))
    assert not R.same_bits(later[-1][1], saved_rows[1]), "the impulses moved on"
    # ---- restore: every row recomputed, without accumulation, from the restored store
    env.load_states(blobs)
    assert np.array_equal(_stores(env, lib)[:, 0], saved_stores[:, 0])
    _assert_rows(_tensors(env), R.contact_obs(_stores(env, lib), N), "after load_states")
    _assert_rows(_tensors(env), saved_rows, "after load_states: the saved state's rows")
    for k in range(4, 8):
        env.step(acts[k])
        _assert_rows(_tensors(env), later[k - 4], f"step {k} again after the restore")
    # ---- clone: env 3 and 4 become copies of env 0 (contact) — and of env 1 after it has been reset (no contact)
    mask = torch.zeros(B, dtype=torch.uint8, device="cuda"); mask[1] = 1
    env.reset_envs(mask)
    rows = _tensors(env)
    _assert_rows(rows, R.contact_obs(_stores(env, lib), N), "after reset_envs")
    assert not rows[0][1].any() and not rows[1][1].any() and rows[0][0].all(), "reset_envs empties the reset env's rows and keeps the others"
    env.clone_envs([0, 1], [3, 4])
    rows = _tensors(env)
    _assert_rows(rows, R.contact_obs(_stores(env, lib), N), "after clone_envs")
    assert np.array_equal(rows[0][3], rows[0][0]) and R.same_bits(rows[1][3], rows[1][0]) and rows[0][3].all()
    assert not rows[0][4].any() and not rows[1][4].any()
    # ---- refresh_contacts: the same rows again, into buffers that held something else
    env.contact_mask.fill_(-1); env.contact_impulse.fill_(float("nan"))
    m, x = env.refresh_contacts()
    assert m is env.contact_mask and x is env.contact_impulse
    _assert_rows(_tensors(env), rows, "refresh_contacts")
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 5. off
def test_off_by_default_and_without_effect_on_the_step(torch_cuda):
    """Without the keyword: no tensors, no info keys, refresh_contacts refuses.  A twin with the feature on produces bit-identical obs, reward
    and done over the rear-end run (B = 67, two streams: the contact chain is on the path)."""
    torch = torch_cuda
    B, N, seed = 67, 2, 62
    off = _make(B, N, seed, contacts=True, streams=None); o0 = off.reset().clone()
    on = _make(B, N, seed, contacts=True, streams=None, contact_obs=True); o1 = on.reset()
    assert off.contact_mask is None and off.contact_impulse is None
    from multi_car_racing_amd._lib import McrError
    with pytest.raises(McrError, match="contact_obs"):
        off.refresh_contacts()
    assert torch.equal(o0, o1)
    rear_end_setup(off, []); rear_end_setup(on, [])
    rng = np.random.RandomState(4)
    touched = 0
    for k in range(30):
        a = torch.from_numpy(_rear_end_actions(rng, B, k)).cuda()
        ob0, r0, d0, i0 = off.step(a)
        ob1, r1, d1, i1 = on.step(a)
        assert "contact_mask" not in i0 and "contact_impulse" not in i0 and "contact_mask" in i1
        assert torch.equal(ob0, ob1) and torch.equal(r0, r1) and torch.equal(d0, d1), f"step {k}"
        touched += int(on.contact_mask.any().item())
    assert touched >= 20, "the run was meant to collide"
    off.close(); on.close()


# ---------------------------------------------------------------------------------------------------------------- 6. the ABI's checks on a handle
def test_set_contact_obs_refuses_handles_without_a_store(torch_cuda):
    import ctypes
    torch = torch_cuda
    ERR_ARG, ERR_STATE = -1, -3
    m = torch.zeros((4, 2), dtype=torch.int32, device="cuda"); x = torch.zeros((4, 2, 2), dtype=torch.float64, device="cuda")
    mp, xp = ctypes.c_void_p(m.data_ptr()), ctypes.c_void_p(x.data_ptr())
    for N, contacts in ((1, True), (2, False)):
        env = _make(4, N, 5, contacts=contacts, obs=False)
        assert env.L.mcr_set_contact_obs(env.h, mp, xp) == ERR_ARG, f"N {N}, car_contacts {contacts}"
        assert env.L.mcr_contact_obs_now(env.h, None) == ERR_STATE
        env.close()
    env = _make(4, 2, 5, contacts=True, obs=False)
    assert env.L.mcr_set_contact_obs(env.h, mp, None) == ERR_ARG and env.L.mcr_set_contact_obs(env.h, None, xp) == ERR_ARG
    assert env.L.mcr_contact_obs_now(env.h, None) == ERR_STATE          # nothing was set by the refused calls
    assert env.L.mcr_set_contact_obs(env.h, mp, xp) == 0
    env.reset()
    m.fill_(-1); x.fill_(7.0)
    assert env.L.mcr_contact_obs_now(env.h, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    assert not m.any().item() and not x.any().item(), "cars on the grid do not touch"
    assert env.L.mcr_set_contact_obs(env.h, None, None) == 0 and env.L.mcr_contact_obs_now(env.h, None) == ERR_STATE      # off again
    env.step(torch.zeros((4, 2, 3), device="cuda")); m.fill_(-1); torch.cuda.synchronize()
    env.step(torch.zeros((4, 2, 3), device="cuda")); torch.cuda.synchronize()
    assert (m == -1).all().item(), "switched off: the step no longer writes the buffers"
    env.close()
