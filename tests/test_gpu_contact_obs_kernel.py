"""MI355X: k_contactobs (csrc/k_contactobs.h) on synthetic manifold stores, through mcr_debug_contact_obs — the step's own launch function on
caller-made buffers — against the host definition of tests/contact_obs_ref.py: the masks equal, the impulses equal as bit patterns.

What a rollout does not reach and this file does: 24 records in an env, every pair of eight cars, both point counts side by side, NaN bit
patterns behind the count and in the unused second point (a read of either shows in the sum), f32 denormals and the largest f32 values, impulses sixteen decades apart
with both signs — a reordered or re-associated sum shows: asserted on the host first —, an accumulating launch that continues from
arbitrary bits (f64 denormals among them), more envs than one workgroup holds and a last workgroup that is not full, and output buffers
that start one element behind their allocation."""
import ctypes
import itertools

import numpy as np
import pytest

from tests import contact_obs_ref as R

pytestmark = pytest.mark.gpu

NAN32 = 0x7fc0dead
GUARD = 8
MASK_SENTINEL = -1515870811                          # 0xa5a5a5a5
IMP_SENTINEL = 0xfff85a5a5a5a5a5a - (1 << 64)        # as int64: a NaN pattern no sum produces
COUNTS = (R.CC_MAX, 1, 0, R.CC_MAX, R.CC_MAX)        # env e holds COUNTS[e % 5] records


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _impulses(rng, n):
    """f32: magnitudes 10^U(-8, 8) with random signs (sixteen decades: two f32 values less than nine decades apart add exactly in f64,
    and more than sixteen apart the smaller one vanishes — in between an addition rounds, and the order of a sum shows); one in eight a denormal or a zero"""
    x = (10.0 ** rng.uniform(-8, 8, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    special = np.array([1e-45, -1e-45, 3e-40, -1.1e-38, 0.0, -0.0], np.float32)
    pick = rng.rand(n) < 0.125
    x[pick] = rng.choice(special, int(pick.sum()))
    return x


def _stores(rng, B, N, counts):
    """[B, STORE_WORDS] u32: env e holds counts[e] records, the pairs of cars taken in turn, two records each, from the list of all pairs (over
    the batch every pair appears once there are that many records), either car first, any fixtures, one or two points; every other word — the records
    behind the count keep well-formed keys — is a NaN bit pattern"""
    pairs = list(itertools.combinations(range(N), 2))
    s = np.full((B, R.STORE_WORDS), NAN32, np.uint32)
    t = rng.randint(len(pairs))
    for e in range(B):
        s[e, 0] = counts[e]
        s[e, 1:4] = rng.randint(0, 2 ** 32, 3, dtype=np.uint64).astype(np.uint32)
        for i in range(R.CC_MAX):
            a, b = pairs[(t // 2) % len(pairs)]                  # (two records in a row per pair: a sum has an order)
            if i < counts[e]:
                t += 1
            if rng.rand() < 0.5:
                a, b = b, a
            rec = s[e, 4 + i * R.CC_WORDS: 4 + (i + 1) * R.CC_WORDS]
            n = 1 + (i + e) % 2 if counts[e] > 1 else 1 + e % 2
            rec[0] = R.make_key(a, rng.randint(8), b, rng.randint(8))
            rec[1] = rng.randint(1, 3) | n << 8
            if i < counts[e]:
                rec[8:8 + 5 * n:5] = _impulses(rng, n).view(np.uint32)
        if counts[e] == R.CC_MAX and e % 2 == 0:
            # the first two neighbouring records of one pair of cars: (+3e38 - 3e38) + 1 = 1 in store order, (1 + 3e38) - 3e38 = 0 in any other
            recs = s[e, 4:].reshape(R.CC_MAX, R.CC_WORDS)
            cars = [frozenset((int(k) & 15, (int(k) >> 8) & 15)) for k in recs[:, 0]]
            i = next(i for i in range(R.CC_MAX - 1) if cars[i] == cars[i + 1])
            recs[i, 1] = 1 | 2 << 8; recs[i, 8], recs[i, 13] = np.array([3.0e38, -3.0e38], np.float32).view(np.uint32)
            recs[i + 1, 1] = 2 | 1 << 8; recs[i + 1, 8] = np.array([1.0], np.float32).view(np.uint32)[0]; recs[i + 1, 13] = NAN32
    return s


def _reversed_records(stores):
    """the same stores with every env's records in the opposite order (host-side check that the order of the additions shows)"""
    out = stores.copy()
    for e in range(len(stores)):
        c = min(int(stores[e, 0]), R.CC_MAX)
        recs = stores[e, 4:4 + c * R.CC_WORDS].reshape(c, R.CC_WORDS)
        out[e, 4:4 + c * R.CC_WORDS] = recs[::-1].reshape(-1)
    return out


def _arbitrary_f64(rng, shape):
    """random bit patterns of finite f64 values, one in eight a denormal"""
    bits = rng.randint(0, 2 ** 63, shape, dtype=np.int64).astype(np.uint64) | (rng.randint(0, 2, shape).astype(np.uint64) << np.uint64(63))
    expo = (bits >> np.uint64(52)) & np.uint64(0x7ff)
    bits[expo == 0x7ff] &= np.uint64(0xbfffffffffffffff)                  # no inf / NaN: x86 and gfx950 propagate NaN payloads differently
    den = rng.rand(*shape) < 0.125
    bits[den] &= np.uint64(0x800fffffffffffff)
    return bits.view(np.float64)


class _Device:
    """the two output buffers, `offset` elements behind their allocations and GUARD sentinels on either side"""

    def __init__(self, torch, lib, B, N, offset):
        self.torch, self.L, self.B, self.N = torch, lib.load(), B, N
        self.mask_all = torch.full((GUARD + offset + B * N + GUARD,), MASK_SENTINEL, dtype=torch.int32, device="cuda")
        self.imp_all = torch.full((GUARD + offset + B * N * N + GUARD,), IMP_SENTINEL, dtype=torch.int64, device="cuda").view(torch.float64)
        self.mask = self.mask_all[GUARD + offset: GUARD + offset + B * N]
        self.imp = self.imp_all[GUARD + offset: GUARD + offset + B * N * N]
        assert self.mask.data_ptr() == self.mask_all.data_ptr() + 4 * (GUARD + offset) and self.imp.data_ptr() == self.imp_all.data_ptr() + 8 * (GUARD + offset)

    def put(self, mask, imp):
        self.mask.copy_(self.torch.from_numpy(np.ascontiguousarray(mask).reshape(-1)).cuda())
        self.imp.view(self.torch.int64).copy_(self.torch.from_numpy(np.ascontiguousarray(imp).reshape(-1).view(np.int64)).cuda())

    def launch(self, stores, accumulate):
        d = self.torch.from_numpy(stores.view(np.int32)).cuda()
        st = self.torch.cuda.current_stream()
        rc = self.L.mcr_debug_contact_obs(ctypes.c_void_p(d.data_ptr()), self.B, self.N, int(accumulate), ctypes.c_void_p(self.mask.data_ptr()),
                                          ctypes.c_void_p(self.imp.data_ptr()), ctypes.c_void_p(st.cuda_stream))
        assert rc == 0, self.L.mcr_last_error()
        self.torch.cuda.synchronize()
        m = self.mask_all.cpu().numpy(); x = self.imp_all.view(self.torch.int64).cpu().numpy()
        for g in (m[:GUARD], m[-GUARD:]):
            assert (g == MASK_SENTINEL).all(), "the kernel wrote outside the mask buffer"
        for g in (x[:GUARD], x[-GUARD:]):
            assert (g == IMP_SENTINEL).all(), "the kernel wrote outside the impulse buffer"
        if self.mask.data_ptr() != self.mask_all.data_ptr() + 4 * GUARD:
            assert m[GUARD] == MASK_SENTINEL and x[GUARD] == IMP_SENTINEL, "the kernel wrote in front of an offset buffer"
        return self.mask.cpu().numpy().reshape(self.B, self.N), self.imp.cpu().numpy().reshape(self.B, self.N, self.N)


def _check(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: masks differ in envs {np.nonzero((got[0] != want[0]).any(1))[0][:8].tolist()}"
    gb, wb = got[1].view(np.uint64), want[1].view(np.uint64)
    assert np.array_equal(gb, wb), f"{what}: impulse bits differ in envs {np.nonzero((gb != wb).any((1, 2)))[0][:8].tolist()}"


@pytest.mark.parametrize("N", [2, 3, 8])
@pytest.mark.parametrize("B", [1, 3, 5, 67])
def test_kernel_matches_the_host_definition(torch_cuda, lib, B, N):
    rng = np.random.RandomState(9000 + 16 * B + N)
    dev = _Device(torch_cuda, lib, B, N, offset=1)
    all_counts = [[COUNTS[e % 5] for e in range(B)]]
    if B == 1:
        all_counts += [[1], [0]]                                   # the one env with every count
    for ci, counts in enumerate(all_counts):
        first, second = _stores(rng, B, N, counts), _stores(rng, B, N, counts[::-1] if B > 1 else counts)
        # ---- the inputs are what they are meant to be (host only)
        if max(counts) == R.CC_MAX:
            assert not np.array_equal(R.contact_obs(first, N)[1].view(np.uint64), R.contact_obs(_reversed_records(first), N)[1].view(np.uint64)), \
                "the order of the additions does not show in these inputs"
            ns = {len(r[4]) for e in range(B) for r in R.decode(first[e])}
            assert ns == {1, 2}, "both point counts"
        if N == 8 and B >= 5:
            seen = {frozenset(r[:3:2]) for e in range(B) for r in R.decode(first[e])}
            assert len(seen) == 28, "every pair of cars"
        # ---- a launch that does not accumulate overwrites whatever the buffers held
        want = R.contact_obs(first, N)
        _check(dev.launch(first, False), want, f"B {B} N {N} counts {ci}, from zero")
        assert R.same_bits(want[1], want[1].transpose(0, 2, 1)) and not np.diagonal(want[1], axis1=1, axis2=2).any()
        # ---- an accumulating launch goes on from arbitrary bits: NaN patterns where no addition can happen (the diagonal), finite ones elsewhere
        prev_mask = rng.randint(-2 ** 31, 2 ** 31, (B, N)).astype(np.int32)
        prev_imp = _arbitrary_f64(rng, (B, N, N))
        for a in range(N):
            prev_imp[:, a, a] = np.array([0x7ff8dead0000beef], np.uint64).view(np.float64)[0]
        dev.put(prev_mask, prev_imp)
        want = R.contact_obs(second, N, prev=(prev_mask, prev_imp))
        _check(dev.launch(second, True), want, f"B {B} N {N} counts {ci}, accumulating")
        for e in range(B):
            if second[e, 0] == 0:                                  # nothing stored for such an env: its rows are the bits they were
                assert R.same_bits(want[1][e], prev_imp[e]) and R.same_bits(want[0][e], prev_mask[e])
        # ---- and the chain of two accumulating launches behind one from zero is the macro-step's
        want = R.accumulate_steps([(first, N, None), (second, N, None), (first, N, None)])
        dev.launch(first, False); dev.launch(second, True)
        _check(dev.launch(first, True), want, f"B {B} N {N} counts {ci}, three sub-steps")
