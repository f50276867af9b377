"""MI355X: k_levelstats (csrc/k_levelstats.h) on synthetic rows, through mcr_debug_level_stats — the step tail's own launch function on
caller-supplied buffers — against the host accumulator of tests/level_stats_ref.py: `finished` equal, `stats` equal as uint64 bit patterns,
after every launch.

What the rollouts of tests/test_gpu_level_curriculum.py cannot reach and this file does: the row pass's fast path (16-byte `done` loads,
the ballot, the `continue` on a round without endings, the chunk selection — B >= 1024 only), rounds beyond the first and a tail round behind
full ones, the finished pass striding past waves * 256, more wavefronts than rounds or than envs, sparse endings at those sizes, N up to 8,
misaligned caller buffers (the env-by-env fallbacks), every non-zero `done` / `truncated` byte, out-of-range level rows, and sums that go
on from arbitrary bits.

The returns are spread over 24 decades with random signs, so that a reordered addition shows: every test that says `order=True` first
asserts ON THE HOST that adding each launch's envs in descending index order changes the bits of a return column and of a square column.
Returns whose square overflows go to stats row 1 only (`_case`): a column that holds an inf no longer tells orders apart."""
import ctypes

import numpy as np
import pytest

from tests import level_stats_ref as ref

pytestmark = pytest.mark.gpu

MCR_OK = 0
GUARD = 64                                           # words in front of and behind `finished` and `stats`
FIN_SENTINEL = -1515870811                           # 0xa5a5a5a5
STATS_SENTINEL = 0xfff85a5a5a5a5a5a - (1 << 64)      # as int64: a NaN pattern no sum produces
DONE_BYTES = np.array([1, 2, 0x80, 0xff], np.uint8)
TRUNC_BYTES = np.array([0, 0, 0, 1, 2, 7, 0x80, 0xff], np.uint8)
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
SEEDED_NAN = 0x7ff8dead0000beef                      # a quiet NaN with a payload of its own
BATCHES = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1089, 2048, 2118, 3073]
LEVELS = [1, 3, 4, 6, 255, 256, 300]
CARS = [1, 2, 3, 5, 8]
# seeds: (test's base, parameters) -> how often the default seed was stepped on until the host-side conditions on the INPUTS held (the order
# of the additions shows in a return and in a square column; the sparsest random pattern holds an ending).  Never chosen by a device result.
RESEED = {(2000, 64, 4): 1, (2000, 64, 6): 2, (2000, 64, 255): 2, (2000, 64, 256): 5, (3000, 70, 1): 1, (4000, 2118): 1, (6200, 70): 1, (6300, 70): 1}


def _rng(base, *key):
    return np.random.RandomState(base + sum(int(k) * 7 ** i for i, k in enumerate(key)) + 100003 * RESEED.get((base,) + key, 0))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


# ------------------------------------------------------------------ inputs (host only)
class _Case:
    """one launch's rows on the host"""

    def __init__(self, done, trunc, ret, length, level):
        self.done, self.trunc, self.ret, self.length, self.level = done, trunc, ret, length, level

    def reversed(self):
        """the same rows with the env order turned round: adding them in ascending order is adding the original in DESCENDING order"""
        return _Case(self.done[::-1], None if self.trunc is None else self.trunc[::-1], self.ret[::-1], self.length[::-1], self.level[::-1])


def _row(level, K):
    return np.where((level >= 0) & (level < K), level, K)


def _levels(rng, B, K):
    """in range, one in eight outside: -1, K, K + 5, INT32_MIN, INT32_MAX — all row K"""
    lv = rng.randint(0, K, B).astype(np.int64)
    out = rng.rand(B) < 0.125
    lv[out] = rng.choice([-1, K, K + 5, I32_MIN, I32_MAX], int(out.sum()))
    return lv.astype(np.int32)


def _returns(rng, B, N, level, K):
    """random sign, magnitudes 10^U(-12, 12); one in eight a special value: 0.0, -0.0, subnormals, and — for envs of stats row 1 only —
    values whose square overflows to inf (their sum stays finite)"""
    x = 10.0 ** rng.uniform(-12, 12, (B, N)) * rng.choice([-1.0, 1.0], (B, N))
    special = rng.rand(B, N) < 0.125
    small = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, -2.5e-308])
    big = np.array([1e200, -1e200, 3e180, -7e160, 1.5e154])
    pick_small = small[rng.randint(0, len(small), (B, N))]
    pick_big = big[rng.randint(0, len(big), (B, N))]
    in_row1 = (_row(level.astype(np.int64), K) == 1)[:, None] & (rng.rand(B, N) < 0.5)
    x = np.where(special, np.where(in_row1, pick_big, pick_small), x)
    return np.ascontiguousarray(x, np.float64)


def _case(rng, B, N, K, mask, trunc=True, level=None, ret=None):
    """the rows of one launch: `mask` says which envs end; their `done` bytes are any of 1, 2, 0x80, 0xff, `truncated` any byte value"""
    mask = np.asarray(mask, bool)
    assert mask.shape == (B,)
    done = np.where(mask, DONE_BYTES[rng.randint(0, 4, B)], 0).astype(np.uint8)
    tr = TRUNC_BYTES[rng.randint(0, len(TRUNC_BYTES), B)].astype(np.uint8) if trunc else None
    level = _levels(rng, B, K) if level is None else np.asarray(level, np.int32)
    ret = _returns(rng, B, N, level, K) if ret is None else ret
    length = rng.randint(0, 2 ** 31, B).astype(np.int64)
    length[rng.rand(B) < 0.05] = I32_MAX
    return _Case(done, tr, ret, length.astype(np.int32), level)


def _start(rng, K, N):
    """arbitrary non-zero sums to go on from (counts and lengths integral, as a running rollout would hold them; the rest spread)"""
    C = 3 + 2 * N
    s = 10.0 ** rng.uniform(-6, 6, (K + 1, C)) * rng.choice([-1.0, 1.0], (K + 1, C))
    s[:, 0] = rng.randint(1, 10 ** 6, K + 1); s[:, 1] = rng.randint(0, 10 ** 3, K + 1); s[:, 2] = rng.randint(1, 10 ** 9, K + 1)
    s[:, 3 + N:] = np.abs(s[:, 3 + N:])
    return s


def _reference(cases, K, N, start):
    """[(finished, stats bits)] after each launch, adding in ascending env index"""
    acc = ref.LevelStats(K, N, start=start)
    out = []
    for c in cases:
        fin = acc.step(c.level, c.done, c.trunc, c.ret, c.length)
        out.append((fin, acc.array().view(np.uint64).copy()))
    return out


def _assert_order_shows(cases, K, N, start, want):
    """a condition on the INPUTS: taking each launch's envs in descending order changes bits in a return and in a square column"""
    down = _reference([c.reversed() for c in cases], K, N, start)[-1][1]
    diff = (want[-1][1] != down).any(axis=0)
    assert diff[3:3 + N].any() and diff[3 + N:].any(), f"these rows would not expose a reordered addition: columns that differ {np.flatnonzero(diff).tolist()}"
    assert not diff[:3].any()                      # (integers far below 2^53: exact in any order)


# ------------------------------------------------------------------ the device side
class _Rig:
    """device buffers for one (B, N, K): `finished` and `stats` inside larger tensors filled with a sentinel, `done` / `level` / `finished`
    optionally off their natural 16-byte alignment by `done_off` bytes / `level_off`, `fin_off` int32 words"""

    def __init__(self, torch, lib, B, N, K, start=None, done_off=0, level_off=0, fin_off=0):
        self.torch, self.L, self.B, self.N, self.K = torch, lib.load(), B, N, K
        dev = "cuda:0"
        C = 3 + 2 * N
        self.done_buf = torch.zeros(GUARD + done_off + B + GUARD, dtype=torch.uint8, device=dev)
        self.done = self.done_buf[GUARD + done_off: GUARD + done_off + B]
        self.trunc = torch.zeros(B, dtype=torch.uint8, device=dev)
        self.ret = torch.zeros((B, N), dtype=torch.float64, device=dev)
        self.length = torch.zeros(B, dtype=torch.int32, device=dev)
        self.level_buf = torch.zeros(GUARD + level_off + B, dtype=torch.int32, device=dev)
        self.level = self.level_buf[GUARD + level_off:]
        self.fin_buf = torch.full((GUARD + fin_off + B + GUARD,), FIN_SENTINEL, dtype=torch.int32, device=dev)
        self.fin = self.fin_buf[GUARD + fin_off: GUARD + fin_off + B]
        self.stats_buf = torch.full((GUARD + (K + 1) * C + GUARD,), STATS_SENTINEL, dtype=torch.int64, device=dev)
        self.stats = self.stats_buf[GUARD: GUARD + (K + 1) * C]
        s = np.zeros((K + 1, C)) if start is None else np.asarray(start, np.float64)
        self.stats.copy_(torch.from_numpy(np.ascontiguousarray(s).view(np.int64).reshape(-1)))
        for t, off in ((self.done, done_off), (self.level, 4 * level_off), (self.fin, 4 * fin_off)):
            assert t.data_ptr() % 16 == off % 16, "the allocator's alignment is not what the offsets assume"
        assert self.stats.data_ptr() % 8 == 0 and self.ret.data_ptr() % 8 == 0

    def launch(self, c):
        """upload, ONE launch through the step tail's launch function, read back: (finished int32 [B], stats uint64 [K + 1][C]); guards checked"""
        torch, B = self.torch, self.B
        self.done.copy_(torch.from_numpy(np.ascontiguousarray(c.done)))
        if c.trunc is not None:
            self.trunc.copy_(torch.from_numpy(np.ascontiguousarray(c.trunc)))
        self.ret.copy_(torch.from_numpy(np.ascontiguousarray(c.ret)))
        self.length.copy_(torch.from_numpy(np.ascontiguousarray(c.length)))
        self.level.copy_(torch.from_numpy(np.ascontiguousarray(c.level)))
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        rc = self.L.mcr_debug_level_stats(p(self.done), None if c.trunc is None else p(self.trunc), p(self.ret), p(self.length),
                                          p(self.level), B, self.N, self.K, p(self.fin), p(self.stats),
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == MCR_OK, self.L.mcr_last_error()
        torch.cuda.synchronize()
        fin_all, stats_all = self.fin_buf.cpu().numpy(), self.stats_buf.cpu().numpy()
        n_fin = len(fin_all) - 2 * GUARD - B
        assert (fin_all[:GUARD + n_fin] == FIN_SENTINEL).all() and (fin_all[GUARD + n_fin + B:] == FIN_SENTINEL).all(), "a word beside `finished` was written"
        assert (stats_all[:GUARD] == STATS_SENTINEL).all() and (stats_all[-GUARD:] == STATS_SENTINEL).all(), "a word beside `stats` was written"
        return fin_all[GUARD + n_fin: GUARD + n_fin + B].copy(), stats_all[GUARD:-GUARD].view(np.uint64).reshape(self.K + 1, -1).copy()


def _run(torch, lib, B, N, K, cases, start=None, order=False, by_class=False, **offsets):
    """the launches of `cases` on one `stats`, compared with the host accumulator after each; returns the reference's [(finished, bits)]"""
    want = _reference(cases, K, N, start)
    if order:
        _assert_order_shows(cases, K, N, start, want)
    rig = _Rig(torch, lib, B, N, K, start=start, **offsets)
    for i, (c, (fin, bits)) in enumerate(zip(cases, want)):
        got_fin, got = rig.launch(c)
        assert np.array_equal(got_fin, fin), f"launch {i}: finished differs at envs {np.flatnonzero(got_fin != fin)[:16].tolist()}"
        if by_class:                               # NaN payloads and signs are not part of the contract: the same positions, all else bit-equal
            g_nan, w_nan = np.isnan(got.view(np.float64)), np.isnan(bits.view(np.float64))
            assert np.array_equal(g_nan, w_nan), f"launch {i}: NaN at other positions"
            assert np.array_equal(got[~w_nan], bits[~w_nan]), f"launch {i}: stats differ beside the NaNs"
        else:
            bad = np.argwhere(got != bits)
            assert len(bad) == 0, (f"launch {i} (B = {B}, N = {N}, K = {K}): stats differ in {len(bad)} of {got.size} values, first (row, col) "
                                   f"{bad[:8].tolist()}: {got.view(np.float64)[tuple(bad[0])]!r} != {bits.view(np.float64)[tuple(bad[0])]!r}")
    return want


def _three_patterns(rng, B):
    return [rng.rand(B) < 1 / 16, np.ones(B, bool), rng.rand(B) < 0.5]


# ------------------------------------------------------------------ sizes
@pytest.mark.parametrize("B", BATCHES)
def test_batch_sizes(torch_cuda, lib, B):
    """whole rounds only (1024, 2048), a one-env tail (1025), a round + a chunk + one env (1089), two rounds + a tail of 70 (2118), three
    rounds + one env (3073), and the small sizes on the slow path under the same harness.  Three launches on one `stats` that starts from
    arbitrary sums: one env in 16, every env, half of them.  (K = 3 is four wavefronts: from B = 1025 on the finished pass strides past
    its first sweep of waves * 256 envs.)"""
    N, K = 2, 3
    rng = _rng(1000, B)
    cases = [_case(rng, B, N, K, m) for m in _three_patterns(rng, B)]
    _run(torch_cuda, lib, B, N, K, cases, start=_start(rng, K, N), order=B >= 63)


@pytest.mark.parametrize("B", [64, 1089, 2118])
@pytest.mark.parametrize("K", LEVELS)
def test_level_counts(torch_cuda, lib, B, K):
    """K + 1 rows, one wavefront each, four per workgroup: K = 3 exactly one workgroup, K = 4 an idle tail in the second, K = 256 the bench
    value (257 wavefronts: more than rounds of the finished pass, wavefronts r > K leave behind it), K = 300 at B = 64 more wavefronts than envs"""
    N = 1
    rng = _rng(2000, B, K)
    cases = [_case(rng, B, N, K, m) for m in _three_patterns(rng, B)]
    _run(torch_cuda, lib, B, N, K, cases, start=_start(rng, K, N), order=True)


@pytest.mark.parametrize("B", [70, 2118])
@pytest.mark.parametrize("N", CARS)
def test_car_counts(torch_cuda, lib, B, N):
    """C = 3 + 2N columns, 5 .. 19: the unrolled column loops with their `a < N` guards, every column stored"""
    K = 4
    rng = _rng(3000, B, N)
    cases = [_case(rng, B, N, K, m) for m in _three_patterns(rng, B)]
    want = _run(torch_cuda, lib, B, N, K, cases, start=_start(rng, K, N), order=True)
    assert want[-1][1].shape == (K + 1, 3 + 2 * N)


# ------------------------------------------------------------------ which envs end
def _patterns(B, rng):
    """name -> mask, for B >= 2118 (two or three full rounds and a tail)"""
    e = np.arange(B)
    full = (B // 1024) * 1024
    p = {"none": e < 0, "all": e >= 0}
    for i in (0, 15, 16, 63, 64, 1023, 1024, B - 1):
        p[f"single_{'last' if i == B - 1 else i}"] = e == i
    p["pair_1023_1024"] = (e == 1023) | (e == 1024)
    p["last_of_every_16"] = e % 16 == 15
    p["first_of_every_16"] = e % 16 == 0
    p["tail_round_only"] = e >= full
    p["first_round_only"] = (e < 1024) & (rng.rand(B) < 0.25)
    p["last_full_round_only"] = (e >= full - 1024) & (e < full) & (rng.rand(B) < 0.25)
    p["chunk_15_only"] = (e % 1024 >= 960) & (e < full)
    p["chunk_15_of_round_1_only"] = (e >= 1024 + 960) & (e < 2048)
    p["one_env_per_chunk"] = e % 64 == 37
    for name, d in (("random_1_1000", 1 / 1000), ("random_1_16", 1 / 16), ("random_1_2", 1 / 2)):
        p[name] = rng.rand(B) < d
    return p


PATTERN_NAMES = list(_patterns(2118, np.random.RandomState(0)))


@pytest.mark.parametrize("B", [2118, 3073])
def test_done_patterns(torch_cuda, lib, B):
    """every pattern one launch, all on the same `stats`, compared after each: no ending (every full round takes the `continue`), all, single
    endings at the edges of a lane's 16 bytes, of a chunk and of a round, the first / last env of every 16 only, the tail round only, one
    full round only (the others take the `continue`), chunk 15 only (the top four ballot bits), and random endings at three densities —
    1 / 1000 is the steady state the ballots were written for"""
    N, K = 2, 6
    rng = _rng(4000, B)
    pats = _patterns(B, rng)
    assert list(pats) == PATTERN_NAMES and pats["random_1_1000"].any() and not pats["none"].any()
    assert pats["tail_round_only"].sum() == B % 1024 and pats["chunk_15_only"].sum() == 64 * (B // 1024)
    cases = [_case(rng, B, N, K, m) for m in pats.values()]
    _run(torch_cuda, lib, B, N, K, cases, start=_start(rng, K, N), order=True)


@pytest.mark.parametrize("name", PATTERN_NAMES)
def test_done_patterns_from_zero(torch_cuda, lib, name):
    """each pattern alone on a zeroed `stats`, B = 2118: a row without an ending stays all-zero bits, and nothing rides on an earlier launch"""
    B, N, K = 2118, 3, 4
    rng = _rng(4500)
    mask = _patterns(B, rng)[name]
    assert mask.any() == (name != "none")
    want = _run(torch_cuda, lib, B, N, K, [_case(rng, B, N, K, mask)])
    assert want[0][1][:, 0].view(np.float64).sum() == mask.sum()


@pytest.mark.parametrize("value", [1, 2, 0x80, 0xff])
def test_done_byte_values(torch_cuda, lib, value):
    """"non-zero" is the definition: one byte value for every ending, at every position of a lane's 4-byte and 16-byte loads"""
    B, N, K = 2118, 1, 3
    rng = _rng(5000, value)
    cases = []
    for m in (rng.rand(B) < 0.3, np.arange(B) % 4 == 2, np.arange(B) % 16 == 9):
        c = _case(rng, B, N, K, m)
        c.done = np.where(m, value, 0).astype(np.uint8)
        cases.append(c)
    _run(torch_cuda, lib, B, N, K, cases, order=True)


# ------------------------------------------------------------------ level rows, truncation, values
def test_out_of_range_levels_go_to_row_K(torch_cuda, lib):
    """-1, K, K + 5, INT32_MIN, INT32_MAX, each for a fifth of the envs and nothing in range: row K is the only one hit, the others keep
    their starting bits"""
    B, N, K = 2118, 2, 6
    rng = _rng(6000)
    level = np.array([-1, K, K + 5, I32_MIN, I32_MAX], np.int64)[np.arange(B) % 5].astype(np.int32)
    start = _start(rng, K, N)
    cases = [_case(rng, B, N, K, m, level=level) for m in (rng.rand(B) < 0.1, np.ones(B, bool))]
    want = _run(torch_cuda, lib, B, N, K, cases, start=start, order=True)
    assert (want[-1][0] == K).all() and np.array_equal(want[-1][1][:K], start.view(np.uint64)[:K])
    assert want[-1][1][K, 0].view(np.float64) == start[K, 0] + (cases[0].done != 0).sum() + B


@pytest.mark.parametrize("row", [0, 2])
def test_every_ending_in_one_row(torch_cuda, lib, row):
    """one long chain — 2118 additions per column in one wavefront — and every other row untouched"""
    B, N, K = 2118, 2, 3
    rng = _rng(6100, row)
    start = _start(rng, K, N)
    cases = [_case(rng, B, N, K, m, level=np.full(B, row)) for m in (np.ones(B, bool), rng.rand(B) < 0.5)]
    want = _run(torch_cuda, lib, B, N, K, cases, start=start, order=True)
    others = [r for r in range(K + 1) if r != row]
    assert np.array_equal(want[-1][1][others], start.view(np.uint64)[others])


@pytest.mark.parametrize("B", [70, 2118])
def test_without_a_truncated_row(torch_cuda, lib, B):
    """d_trunc NULL: column 1 takes +0.0 per ending (so a -0.0 there becomes +0.0, and only in a row that took one)"""
    N, K = 2, 3
    rng = _rng(6200, B)
    start = _start(rng, K, N)
    start[:, 1] = [-0.0, 5.0, -0.0, 0.0]
    level = rng.randint(0, 2, B)                   # rows 0 and 1 only
    cases = [_case(rng, B, N, K, m, trunc=False, level=level) for m in _three_patterns(rng, B)]
    want = _run(torch_cuda, lib, B, N, K, cases, start=start, order=True)
    col1 = want[-1][1][:, 1]
    assert col1.tolist() == np.array([0.0, 5.0, -0.0, 0.0]).view(np.uint64).tolist()


@pytest.mark.parametrize("B", [70, 2118])
def test_truncated_bytes_other_than_one(torch_cuda, lib, B):
    """every non-zero `truncated` byte counts 1.0"""
    N, K = 1, 3
    rng = _rng(6300, B)
    cases = []
    for v in (2, 7, 0x80, 0xff):
        c = _case(rng, B, N, K, rng.rand(B) < 0.5)
        c.trunc = np.where(rng.rand(B) < 0.5, v, 0).astype(np.uint8)
        cases.append(c)
    want = _run(torch_cuda, lib, B, N, K, cases, order=True)
    n_trunc = sum(int(((c.done != 0) & (c.trunc != 0)).sum()) for c in cases)
    assert want[-1][1][:, 1].view(np.float64).sum() == n_trunc > 0


def test_episode_lengths_up_to_int32_max(torch_cuda, lib):
    B, N, K = 1089, 1, 3
    rng = _rng(6400)
    c = _case(rng, B, N, K, np.ones(B, bool))
    c.length = np.full(B, I32_MAX, np.int32)
    want = _run(torch_cuda, lib, B, N, K, [c], order=True)
    assert want[0][1][:, 2].view(np.float64).sum() == float(B) * I32_MAX


@pytest.mark.parametrize("B", [70, 2118])
def test_nan_and_inf_returns(torch_cuda, lib, B):
    """NaN, +inf and -inf among the returns of four ending envs per launch: the sums go NaN (inf - inf, NaN + x) where the host's do and
    nowhere else; everything that is no NaN — infinities included — is bit-equal.  NaN payloads are not part of the contract."""
    N, K = 2, 6
    rng = _rng(6500, B)
    cases = []
    for m in _three_patterns(rng, B):
        c = _case(rng, B, N, K, m)
        for e in rng.choice(np.flatnonzero(m), 4, replace=False):
            c.ret[e, rng.randint(N)] = [np.nan, np.inf, -np.inf][rng.randint(3)]
        cases.append(c)
    want = _run(torch_cuda, lib, B, N, K, cases, start=_start(rng, K, N), by_class=True)
    last = want[-1][1].view(np.float64)
    assert np.isnan(last).any() and np.isinf(last[:, 3:3 + N]).any() and np.isfinite(last[:, 3:3 + N]).any()


# ------------------------------------------------------------------ accumulation
@pytest.mark.parametrize("B", [70, 1089, 2118])
def test_accumulation_keeps_untouched_rows(torch_cuda, lib, B):
    """three launches with three patterns on one `stats` that starts from arbitrary sums; row 1 starts as -0.0 throughout and takes its first
    ending in the third launch only, row 4 holds a NaN pattern of its own and never takes one: a row without an ending in a launch keeps its
    bits exactly — it is not stored at all"""
    N, K = 2, 6
    rng = _rng(7000, B)
    start = _start(rng, K, N)
    start[1] = -0.0
    start.view(np.uint64)[4] = SEEDED_NAN
    lv = rng.choice([0, 2, 3, 5, -1], B)           # rows 0, 2, 3, 5 and K
    lv3 = rng.choice([0, 1, 2, 3, 5, K + 5], B)    # row 1 joins
    cases = [_case(rng, B, N, K, rng.rand(B) < 1 / 16, level=lv), _case(rng, B, N, K, np.arange(B) % 16 == 15, level=lv),
             _case(rng, B, N, K, rng.rand(B) < 0.5, level=lv3)]
    want = _run(torch_cuda, lib, B, N, K, cases, start=start, order=True)
    neg0 = np.array(-0.0).view(np.uint64)
    for fin, bits in want[:2]:
        assert (bits[1] == neg0).all() and (bits[4] == SEEDED_NAN).all() and not (fin == 1).any()
    assert (want[2][0] == 1).any() and (want[2][1][1] != neg0).any() and (want[2][1][4] == SEEDED_NAN).all()


def test_guard_words_with_B_no_multiple_of_four(torch_cuda, lib):
    """`finished` of 1, 2, 3 envs past a multiple of four (the finished pass's scalar tail) and past a round of 256 between sentinel words:
    _Rig.launch asserts the words in front and behind after every launch"""
    N, K = 1, 3
    for B in (1, 2, 3, 5, 6, 7, 257, 258, 259, 1027):
        rng = _rng(7100, B)
        _run(torch_cuda, lib, B, N, K, [_case(rng, B, N, K, np.ones(B, bool)), _case(rng, B, N, K, np.zeros(B, bool))])


# ------------------------------------------------------------------ misaligned caller buffers
OFFSETS = {"aligned": {}, "done+1": dict(done_off=1), "done+4": dict(done_off=4), "level+1": dict(level_off=1), "finished+1": dict(fin_off=1),
           "all": dict(done_off=1, level_off=1, fin_off=1)}


@pytest.mark.parametrize("B", [70, 2118])
@pytest.mark.parametrize("which", list(OFFSETS))
def test_misaligned_buffers_give_the_same_bits(torch_cuda, lib, B, which):
    """`done` off by 1 byte (neither 4-byte nor 16-byte loads) and by 4 (no 16-byte loads: the row pass visits every chunk), `level` and
    `finished` off by one int32 (the finished pass goes env by env): the same cases — same seed for every offset — the same bits"""
    N, K = 2, 6
    rng = _rng(8000, B)
    cases = [_case(rng, B, N, K, m) for m in (rng.rand(B) < 1 / 1000 if B > 1000 else np.arange(B) == 33, rng.rand(B) < 1 / 16, np.ones(B, bool),
                                              np.arange(B) % 16 == 15, np.zeros(B, bool))]
    _run(torch_cuda, lib, B, N, K, cases, start=_start(rng, K, N), order=True, **OFFSETS[which])
