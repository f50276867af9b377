"""MI355X: batched device-side snapshot / restore / clone of env states (VecMultiCarRacing.save_states / load_states / clone_envs over
csrc/k_envcopy.h) against the per-env host path it batches (get_state_blob / set_state_blob), the oracle, and itself."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from tests.util import make_env, oracles, random_actions, rear_end_setup

pytestmark = pytest.mark.gpu

MCR_OK, MCR_ERR_ARG, MCR_ERR_STATE = 0, -1, -3


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _crash_actions(rng, B, N, k):
    """car 0 brakes, then coasts; car 1 floors it (the rear-end scenario of tests/test_gpu_parity.py)"""
    a = random_actions(rng, B, N, 0.0)
    if N > 1:
        a[:, 0, 1] = 0.0; a[:, 0, 2] = 0.8 if k < 60 else 0.0; a[:, 1, 0] *= 0.2; a[:, 1, 1] = 1.0
    return a


def _contact_counts(env):
    out = np.zeros(env.B, np.int32)
    assert env.L.mcr_debug_read_contact_counts(env.h, out.ctypes.data_as(ctypes.c_void_p)) == 0
    return out


def _host_blobs(env):
    return [env.get_state_blob(e) for e in range(env.B)]


CASES = {
    "N1": dict(N=1, B=5, steps=15, kw=dict(streams=1)),
    "N2-contacts-2streams": dict(N=2, B=6, steps=70, rear=True, kw=dict(streams=2)),
    "N8": dict(N=8, B=3, steps=10, kw=dict()),
    "particles": dict(N=2, B=4, steps=25, kw=dict(skid_particles=True)),
    "fresh-world": dict(N=2, B=4, steps=15, kw=dict(fresh_world=True)),
}


def scripted_rollout(torch, case):
    """the env of CASES[case] after its scripted steps, nothing synchronous behind the last one (tools/make_state_blob_golden.py runs the same)"""
    c = CASES[case]; N, B = c["N"], c["B"]
    env = make_env(B, N, 70 + N, contacts=True, **c["kw"]); env.reset()
    if c.get("rear"):
        rear_end_setup(env, [])
    rng = np.random.RandomState(5)
    for k in range(c["steps"]):
        env.step(torch.from_numpy(_crash_actions(rng, B, N, k) if c.get("rear") else random_actions(rng, B, N, 0.2)).cuda())
    return env

@pytest.mark.parametrize("case", list(CASES))
def test_save_states_is_byte_identical_with_the_host_snapshot(torch_cuda, case):
    """Row e of save_states() — taken FIRST after the steps, so a pending flag scan has to be flushed by the call itself — holds exactly
    get_state_blob(e), header included, zeros up to the pitch; also for a permuted id list that holds env B-1, for one id, and into `out`."""
    torch = torch_cuda
    c = CASES[case]; N, B = c["N"], c["B"]
    env = scripted_rollout(torch, case)
    dev = env.save_states()
    some = [B - 1, 0, 2]
    dev_some = env.save_states(some)
    out1 = torch.full((1, env.state_blob_pitch), 0xAB, dtype=torch.uint8, device=env.device)
    assert env.save_states(torch.tensor([B - 2], dtype=torch.int32, device=env.device), out=out1) is out1
    nbytes, pitch = int(env.L.mcr_state_blob_bytes(env.h)), env.state_blob_pitch
    assert pitch == (nbytes + 15) // 16 * 16 and tuple(dev.shape) == (B, pitch) and dev.dtype == torch.uint8
    got, got_some, got1 = dev.cpu().numpy(), dev_some.cpu().numpy(), out1.cpu().numpy()
    host = _host_blobs(env)
    if c.get("rear"):
        assert _contact_counts(env).sum() > 0, "the snapshot should be taken with live car<->car contacts"
    hdr = host[0][:16].view(np.uint32)
    assert hdr[1] == N and hdr[2] == (1 if c["kw"].get("skid_particles") else 0) | (0 if c["kw"].get("fresh_world") else 2) and hdr[3] == nbytes
    for e in range(B):
        d = np.nonzero(got[e, :nbytes] != host[e])[0]
        assert len(d) == 0, f"env {e}: {len(d)} bytes differ, first at {d[:4]}"
        assert not got[e, nbytes:].any()
    for i, e in enumerate(some):
        assert np.array_equal(got_some[i, :nbytes], host[e]), f"id list row {i} (env {e})"
    assert np.array_equal(got1[0, :nbytes], host[B - 2]) and not got1[0, nbytes:].any()
    env.close()


@pytest.mark.parametrize("case", list(CASES))
def test_blobs_reproduce_the_recorded_format(torch_cuda, case):
    """tests/golden/state_blob_format.json (tools/make_state_blob_golden.py, recorded before the section table replaced the four hand-written
    layouts): after the case's scripted rollout the blob size, the header words and the SHA-256 of every env's blob are the recorded ones,
    from get_state_blob (the host walk over the table) and from the first blob_bytes of each save_states() row (the kernel's segment table)."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "state_blob_format.json")) as f:
        want = json.load(f)[case]
    env = scripted_rollout(torch_cuda, case)
    rows = env.save_states().cpu().numpy()
    nbytes = int(env.L.mcr_state_blob_bytes(env.h))
    hdr = np.zeros(4, np.uint32)
    assert env.L.mcr_state_blob_header(env.h, hdr.ctypes.data) == MCR_OK
    assert nbytes == want["blob_bytes"] and hdr.tolist() == want["header"] and len(want["sha256"]) == env.B
    for e in range(env.B):
        host = env.get_state_blob(e)
        assert host[:16].view(np.uint32).tolist() == want["header"]
        assert hashlib.sha256(host.tobytes()).hexdigest() == want["sha256"][e], f"env {e}: get_state_blob"
        assert hashlib.sha256(rows[e, :nbytes].tobytes()).hexdigest() == want["sha256"][e], f"env {e}: save_states"
    env.close()


@pytest.mark.parametrize("streams", [1, 2])
def test_batched_restore_into_another_handle_continues_bit_identically(torch_cuda, oracle, streams):
    """tests/test_gpu_parity.py::test_state_blob_round_trip_mid_episode in ONE call each way: all envs of src, mid-collision, into a
    permutation of the slots of a handle with another seed and B + 2 envs; both continue bit-identically, and like the oracle."""
    torch = torch_cuda
    B, N, seed = 5, 2, 61
    src = make_env(B, N, seed, contacts=True, max_episode_steps=0, streams=streams); src.reset()
    orcs = oracles(oracle, B, N, seed, contacts=True)
    rear_end_setup(src, orcs)
    rng = np.random.RandomState(4)
    for k in range(70):
        a = _crash_actions(rng, B, N, k); src.step(torch.from_numpy(a).cuda())
        for e, o in enumerate(orcs):
            o.step(a[e], render=False)
    assert sum(o.num_car_contacts() for o in orcs) > 0, "snapshot should be taken with live car<->car contacts"
    dst = make_env(B + 2, N, 999, contacts=True, max_episode_steps=0, streams=streams); dst.reset()
    slots = [4, 1, 5, 2, 3]                                            # src env e -> dst env slots[e]
    refused = dst.load_states(src.save_states(), env_ids=slots)
    assert int(refused.item()) == 0
    s1, s2 = src.get_state(), dst.get_state()
    for key in s1:
        assert np.array_equal(s1[key], s2[key][slots]), key
    for k in range(70, 130):
        a = _crash_actions(rng, B, N, k)
        a2 = np.zeros((B + 2, N, 3), np.float32); a2[slots] = a
        o1, r1, d1, _ = src.step(torch.from_numpy(a).cuda()); o2, r2, d2, _ = dst.step(torch.from_numpy(a2).cuda())
        o1 = o1.cpu().numpy(); o2 = o2.cpu().numpy(); r1 = r1.cpu().numpy(); r2 = r2.cpu().numpy(); d1 = d1.cpu().numpy(); d2 = d2.cpu().numpy()
        assert np.array_equal(r1, r2[slots]) and np.array_equal(d1, d2[slots]) and np.array_equal(o1, o2[slots]), f"step {k}"
        for e, o in enumerate(orcs):
            _, r, d, _ = o.step(a[e], render=False)
            assert np.array_equal(r, r1[e]) and bool(d1[e]) == d, (k, e)
    s1, s2 = src.get_state(), dst.get_state()
    for key in s1:
        assert np.array_equal(s1[key], s2[key][slots]), key
    for env in (src, dst):
        assert env.verdict_mismatches() == 0 and not env.status_words()[:5].any()
    src.close(); dst.close()


def test_rewind_reproduces_the_rollout(torch_cuda):
    """save, 40 steps, load, the same 40 actions again: every reward, done flag and frame comes out bit for bit, and so does the state."""
    torch = torch_cuda
    B, N = 8, 2
    env = make_env(B, N, 61, contacts=True, max_episode_steps=0, streams=2); env.reset()
    rear_end_setup(env, [])
    rng = np.random.RandomState(4)
    for k in range(45):
        env.step(torch.from_numpy(_crash_actions(rng, B, N, k)).cuda())
    snap = env.save_states()
    acts = [torch.from_numpy(_crash_actions(rng, B, N, 45 + k)).cuda() for k in range(40)]

    def rollout():
        rec = []
        for a in acts:
            obs, rew, done, _ = env.step(a)
            rec.append((obs.clone(), rew.clone(), done.clone()))
        return rec, env.get_state()
    rec1, end1 = rollout()
    assert _contact_counts(env).sum() > 0, "the rewound stretch should hold car<->car contacts"
    env.load_states(snap)
    rec2, end2 = rollout()
    for k, (x, y) in enumerate(zip(rec1, rec2)):
        assert torch.equal(x[1], y[1]) and torch.equal(x[2], y[2]), f"step {k}: reward / done"
        assert torch.equal(x[0], y[0]), f"step {k}: obs"
    for key in end1:
        assert np.array_equal(end1[key], end2[key]), key
    assert env.verdict_mismatches() == 0 and not env.status_words()[:5].any()
    env.close()


@pytest.mark.parametrize("fmt", ["rgb", "gray-stack4"])
def test_fan_out_clone(torch_cuda, fmt):
    """clone_envs([0] * 7 + [1] * 7, 2 .. 15) mid-collision: state vector and observations of a clone equal its source's at once (no
    refresh_state), and under group-wise identical actions at every one of 40 steps; a clone driven differently leaves its source."""
    torch = torch_cuda
    B, N = 16, 2
    kw = dict(obs_format="gray", frame_stack=4) if fmt != "rgb" else {}
    env = make_env(B, N, 61, contacts=True, streams=2, state_obs=True, **kw); env.reset()
    assert not env.auto_reset
    rear_end_setup(env, [])
    rng = np.random.RandomState(4)
    k0 = 0
    while k0 < 50 or (k0 < 120 and _contact_counts(env)[:2].min() == 0):    # ~50 steps, and on until both sources' cars touch
        env.step(torch.from_numpy(_crash_actions(rng, B, N, k0)).cuda()); k0 += 1
    assert _contact_counts(env)[:2].min() > 0, "the sources should hold car<->car contacts"
    env.step(torch.from_numpy(_crash_actions(rng, B, N, k0)).cuda()); k0 += 1      # (the clone is taken right behind a step, nothing synchronous in between)
    src = [0] * 7 + [1] * 7; dst = list(range(2, 16))
    env.clone_envs(src, range(2, 16))
    assert torch.equal(env.state[dst], env.state[src]) and torch.equal(env.obs[dst], env.obs[src])
    group = np.array([0, 1] + src)                                      # env -> the source whose actions it gets
    odd, differed = 15, False                                           # one clone of env 1 is driven differently
    same = [e for e in dst if e != odd]; same_src = [int(group[e]) for e in same]
    for k in range(40):
        a = _crash_actions(rng, B, N, k0 + k)[group]
        a[odd, :, 0] = 1.0; a[odd, :, 1] = 0.0
        obs, rew, done, info = env.step(torch.from_numpy(a).cuda())
        for name, t in (("obs", obs), ("reward", rew), ("done", done), ("state", info["state"])):
            assert torch.equal(t[same], t[same_src]), f"step {k}: {name} of a clone differs from its source's"
        differed = differed or not torch.equal(info["state"][odd], info["state"][1])
    assert differed, "the clone with its own actions never left its source: are the clones stepping?"
    assert env.verdict_mismatches() == 0 and not env.status_words()[:5].any()
    env.close()


def test_refused_rows_leave_their_envs_untouched(torch_cuda):
    torch = torch_cuda
    B, N = 6, 2
    env = make_env(B, N, 33, contacts=True); env.reset()
    rng = np.random.RandomState(1)
    for k in range(8):
        env.step(torch.from_numpy(random_actions(rng, B, N, 0.2)).cuda())
    snap = env.save_states()
    saved = snap.cpu().numpy().copy()
    for k in range(8):
        env.step(torch.from_numpy(random_actions(rng, B, N, 0.2)).cuda())
    before = _host_blobs(env)
    bad = snap.clone()
    bad[1, 0] ^= 0x5A                                                   # the magic of row 1
    bad[4, 4] = N + 1                                                   # the N word of row 4
    with pytest.raises(ValueError):
        env.load_states(bad, check=True)
    for e, b in enumerate(_host_blobs(env)):
        assert np.array_equal(b, before[e]), f"check=True changed env {e}"
    counter = env.load_states(bad, check=False)
    assert counter.dtype == torch.int32 and int(counter.item()) == 2
    nbytes = int(env.L.mcr_state_blob_bytes(env.h))
    for e, b in enumerate(_host_blobs(env)):
        want = before[e] if e in (1, 4) else saved[e, :nbytes]
        assert np.array_equal(b, want), f"env {e}: " + ("a refused row was written" if e in (1, 4) else "not restored")
    # ids out of range are refused too (device ids: nothing validates them on the host)
    ids = torch.tensor([0, B, -1], dtype=torch.int32, device=env.device)
    assert int(env.load_states(snap[:3].clone(), env_ids=ids, check=False).item()) == 2
    env.close()


def test_arguments(torch_cuda, lib):
    torch = torch_cuda
    B, N = 4, 2
    env = make_env(B, N, 33)
    L, vp = env.L, ctypes.c_void_p
    buf = torch.zeros((B, env.state_blob_pitch), dtype=torch.uint8, device=env.device)
    ids = torch.arange(B, dtype=torch.int32, device=env.device)
    assert L.mcr_save_states(env.h, None, 1, vp(buf.data_ptr()), None) == MCR_ERR_STATE          # before the first reset
    assert L.mcr_copy_states(env.h, vp(ids.data_ptr()), vp(ids.data_ptr()), 1, None) == MCR_ERR_STATE
    with pytest.raises(lib.McrError):
        env.save_states()
    env.reset()
    assert L.mcr_save_states(env.h, None, -1, vp(buf.data_ptr()), None) == MCR_ERR_ARG
    assert L.mcr_save_states(env.h, None, B + 1, vp(buf.data_ptr()), None) == MCR_ERR_ARG
    assert L.mcr_load_states(env.h, None, -1, vp(buf.data_ptr()), None, None) == MCR_ERR_ARG
    assert L.mcr_copy_states(env.h, vp(ids.data_ptr()), vp(ids.data_ptr()), -1, None) == MCR_ERR_ARG
    assert L.mcr_save_states(env.h, None, 1, None, None) == MCR_ERR_ARG
    assert L.mcr_save_states(env.h, None, 1, vp(buf.data_ptr() + 4), None) == MCR_ERR_ARG        # misaligned rows
    assert L.mcr_copy_states(env.h, None, vp(ids.data_ptr()), 1, None) == MCR_ERR_ARG
    assert L.mcr_save_states(env.h, None, 0, vp(buf.data_ptr()), None) == MCR_OK
    assert L.mcr_load_states(env.h, None, 0, vp(buf.data_ptr()), None, None) == MCR_OK
    assert L.mcr_copy_states(env.h, vp(ids.data_ptr()), vp(ids.data_ptr()), 0, None) == MCR_OK
    snap = env.save_states()
    with pytest.raises(ValueError):
        env.load_states(snap[:, :-16])                                  # wrong row size
    with pytest.raises(ValueError):
        env.load_states(snap.to(torch.int8))                            # wrong dtype
    with pytest.raises(ValueError):
        env.load_states(snap[:3], env_ids=[0, 2, 2])                    # duplicate destinations
    with pytest.raises(ValueError):
        env.load_states(snap[:2], env_ids=[0, B])                       # out of range
    with pytest.raises(ValueError):
        env.load_states(snap[:2], env_ids=[0, 1, 2])                    # rows and ids disagree
    with pytest.raises(ValueError):
        env.clone_envs([0, 1], [1, 2])                                  # a destination that is a source
    with pytest.raises(ValueError):
        env.clone_envs([0, 0], [2, 2])
    with pytest.raises(ValueError):
        env.save_states(out=torch.zeros((B, 16), dtype=torch.uint8, device=env.device))
    env.close()
    stacked = make_env(2, 1, 33, obs_format="gray", frame_stack=4); stacked.reset()
    with pytest.raises(ValueError):
        stacked.load_states(stacked.save_states())
    stacked.close()
