"""CPU: the comparators of tests/util.py that the GPU suite's "bit-exact against the oracle" rests on must BITE — assert_state on a stand-in
env stacked from oracles with exactly one element changed, assert_frame around its edge budget, Follower against the seeding rule, hull_positions against the oracle's positions(), assert_f32_bits on single bits and on NaNs."""
import numpy as np
import pytest

from tests.util import Follower, STATE_ARRAYS, assert_f32_bits, assert_frame, assert_state, hull_positions, oracle_episode, random_actions

TILE_CAP = 512


class _StandIn:
    """what assert_state reads of a VecMultiCarRacing, stacked from oracles"""

    def __init__(self, orcs):
        so = [o.state() for o in orcs]; eo = [o.env_state() for o in orcs]
        self.state = {k: np.stack([s[k] for s in so]) for k in STATE_ARRAYS}
        flags = np.zeros((len(orcs), TILE_CAP), np.uint16)
        for e, x in enumerate(eo):
            flags[e, :len(x["visited"])] = x["visited"] | (x["touched"].astype(np.uint16) << 8)
        self.env_state = dict(reward=np.stack([x["reward"] for x in eo]), tile_visited_count=np.stack([x["tile_visited_count"] for x in eo]),
                              t=np.array([x["t"] for x in eo]), tile_flags=flags, num_tiles=np.array([o.T for o in orcs], np.int32))

    def get_state(self):
        return self.state

    def get_env_state(self):
        return self.env_state


@pytest.fixture(scope="module")
def stand_in(oracle):
    B, N, seed = 2, 2, 5
    orcs = [oracle.OracleEnv(N) for _ in range(B)]
    for e, o in enumerate(orcs):
        o.reset(oracle_episode(oracle, N, seed, e), render=False)
    rng = np.random.RandomState(1)
    for _ in range(5):
        a = random_actions(rng, B, N)
        for e, o in enumerate(orcs):
            o.step(a[e], render=False)
    return _StandIn(orcs), orcs


def _one_off(x):
    """the neighbouring value: one ulp up for a float, the lowest bit flipped for an integer"""
    return np.nextafter(x, np.inf, dtype=x.dtype) if x.dtype.kind == "f" else x ^ 1


def test_assert_state_passes_on_equal_state(stand_in):
    env, orcs = stand_in
    assert_state(env, enumerate(orcs), "untouched")


@pytest.mark.parametrize("key", list(STATE_ARRAYS) + ["reward", "tile_visited_count", "visited bit", "touched bit", "num_tiles", "t"])
def test_assert_state_sees_one_changed_element(stand_in, key):
    """the last element of env 1's array (a flag bit: of its last tile) changed by the smallest step its type has"""
    env, orcs = stand_in
    whole = env.state if key in STATE_ARRAYS else env.env_state
    name, idx = {"visited bit": ("tile_flags", (1, orcs[1].T - 1)), "touched bit": ("tile_flags", (1, orcs[1].T - 1))}.get(key, (key, None))
    arr = whole[name]
    if idx is None:
        idx = tuple(n - 1 for n in arr.shape)
    kept = arr[idx].copy()
    arr[idx] = kept ^ 0x100 if key == "touched bit" else _one_off(kept)
    assert arr[idx] != kept
    try:
        with pytest.raises(AssertionError):
            assert_state(env, enumerate(orcs), key)
    finally:
        arr[idx] = kept
    assert_state(env, enumerate(orcs), "restored")


@pytest.mark.parametrize("budget", [12, 14, 40])
def test_assert_frame_holds_its_edge_budget(budget):
    """two views; the ambiguous mask holds 2 * budget + 1 pixels, all in view 0 (the budget is per view, the count over the frame)"""
    rng = np.random.RandomState(budget)
    want = rng.randint(0, 256, (2, 96, 96, 3)).astype(np.uint8)
    amb = np.zeros((2, 96, 96), np.uint8)
    cols = np.arange(2 * budget + 1)
    amb[0, 50, cols] = 1

    def changed(n_amb, clear=False):
        got = want.copy()
        got[0, 50, cols[:n_amb], 1] ^= 0x80
        if clear:
            got[1, 3, 4, 2] ^= 1
        return got
    assert_frame(want.copy(), want, amb, "identical", budget)
    with pytest.raises(AssertionError, match="1 unambiguous pixels differ: view 1 row 3 col 4"):
        assert_frame(changed(0, clear=True), want, amb, "one clear pixel", budget)
    assert_frame(changed(2 * budget), want, amb, "budget * views edge pixels", budget)
    with pytest.raises(AssertionError, match=f"{2 * budget + 1} edge pixels differ"):
        assert_frame(changed(2 * budget + 1), want, amb, "one more", budget)
    with pytest.raises(AssertionError, match="not rendered"):
        assert_frame(want, None, None, "no oracle frame", budget)


def test_follower_plays_the_episodes_of_the_seeding_rule(oracle):
    N, seed, g = 2, 7, 3
    f = Follower(oracle, N, seed, g, 0, render=False)
    want = oracle_episode(oracle, N, seed, g, use_random_direction=True)
    first = f.ep
    assert f.o.T == len(want["track"]) and f.steps == 0 and f.first_obs is None
    assert first["direction"] == want["direction"] and first["car_order"] == want["car_order"]
    for k, v in want.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(first[k], v), k
    f.new_episode()
    assert f.ep is not first and not np.array_equal(f.ep["track"][:50], first["track"][:50]), "the second episode is the streams' next draw"
    f.o.close()


def test_hull_positions_equals_the_oracles_positions(lib, oracle):
    """bit for bit along a short N = 3 rollout (cars turning and moving: the rotation of the local centre matters)"""
    L = lib.load()
    N = 3
    o = oracle.OracleEnv(N)
    o.reset(oracle_episode(oracle, N, 11, 0), render=False)
    rng = np.random.RandomState(2)
    for k in range(25):
        got = hull_positions(L, o.state()["bodies"]); want = o.positions()
        assert got.dtype == np.float32 and got.shape == (N, 2)
        assert np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32)), f"step {k}: {got.tolist()} vs {want.tolist()}"
        o.step(random_actions(rng, 1, N)[0], render=False)
    assert np.abs(o.state()["bodies"][:, 0, 2] - o.state()["bodies"][0, 0, 2]).max() > 0, "the cars never turned differently"
    stacked = np.stack([o.state()["bodies"]] * 2)
    assert np.array_equal(hull_positions(L, stacked)[1], o.positions().astype(np.float32)), "batched input"
    o.close()


def test_assert_f32_bits_bites():
    rng = np.random.RandomState(4)
    want = rng.randn(3, 2, 2, 5).astype(np.float32)
    want[1, 0, 1, 2] = np.nan; want[2, 1, 0, 0] = 0.0
    assert_f32_bits(want.copy(), want, "identical")
    other_nan = want.copy(); other_nan.view(np.uint32)[1, 0, 1, 2] = 0xffc01234          # another payload, the sign set: the same class
    assert np.isnan(other_nan[1, 0, 1, 2])
    assert_f32_bits(other_nan, want, "NaN payloads")
    for idx, value, flat in (((2, 1, 1, 4), None, 9), ((2, 1, 0, 0), np.float32(-0.0), 0), ((1, 0, 1, 2), np.float32(1.0), 7), ((0, 1, 0, 3), np.float32(np.nan), 3)):
        got = want.copy()
        got[idx] = np.nextafter(want[idx], np.float32(np.inf)) if value is None else value
        with pytest.raises(AssertionError, match=f"first at env {idx[0]} car {idx[1]} index {flat}: got "):
            assert_f32_bits(got, want, "one value")
    with pytest.raises(AssertionError, match="float32 expected"):
        assert_f32_bits(want.astype(np.float64), want, "dtype")
    with pytest.raises(AssertionError, match="shapes"):
        assert_f32_bits(want[:2], want, "shape")
