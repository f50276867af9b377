"""The scenes of tests/dynamics_cases.py held to what they are named for, on the oracle alone (no device): every pinned sweep count, solved
flag and fixed-point index at its env, car and step; every wavefront composition with exactly the limit states it states, lane by lane;
every row of OracleEnv.dynamics_coverage reached, the tyre rows on the road and on the grass; the sleep rule on its steps.  A scene that
misses what it is pinned to fails here — before tests/test_gpu_dynamics_kernel.py compares the kernel with the oracle on it."""
import numpy as np
import pytest

from tests import dynamics_cases as D

_cache = {}


def played(O, key, make, contacts=False):
    if key not in _cache:
        _cache[key] = D.play(O, make(), contacts=contacts)
    return _cache[key]


def total(run):
    """row -> the totals summed over the run's envs and cars"""
    out = {}
    for t in run.totals():
        for k, v in t.items():
            out[k] = out.get(k, 0) + int(v.sum())
    return out


@pytest.mark.parametrize("N", [1, 2, 3])
def test_position_scenes_reach_their_pinned_counts(oracle, N):
    scenes = D.position_scenes(N)
    run, log = played(oracle, ("pos", N), lambda: scenes)
    for e, sc in enumerate(scenes):
        assert sc["pins"], sc["name"]
        for (k, c), want in sc["pins"].items():
            assert D.outcome(log[k][e], c) == want, f"N {N} env {e} ({sc['name']}) step {k} car {c}: (sweeps, solved, fixed_at) {D.outcome(log[k][e], c)}, pinned {want}"


def test_the_pinned_set_holds_every_count_the_kernel_tells_apart(oracle):
    first = [sc["pins"][(0, 0)] for sc in D.position_scenes(1)]
    solved = {s for s, ok, f in first if ok}
    assert {1, 2, 3, 4, 5, 6, 7, 10, 11, 59, 60} <= solved, sorted(solved)
    assert any(12 <= s <= 30 for s in solved) and any(31 <= s <= 58 for s in solved)
    assert (60, 0, 0) in first, "60 sweeps, unsolved, no fixed point"
    fixed = sorted(f for s, ok, f in first if f)
    assert all(s == 60 and not ok for s, ok, f in first if f), "a fixed point is a failing sweep: the oracle runs on to 60"
    assert fixed[0] <= D.DEFER_AFTER, "a fixed point inside the main launch's sweeps: it must stop, not defer"
    assert any(D.DEFER_AFTER < f <= 7 for f in fixed) and any(7 < f <= 11 for f in fixed) and any(f > 11 for f in fixed), fixed
    hull = next(sc for sc in D.position_scenes(1) if sc["name"] == "hullspin_100")
    assert [hull["pins"][(k, 0)][0] for k in range(3)] == [D.DEFER_AFTER] * 3, "exactly the main launch's grant, three steps running"
    # the parked state with more than one car in the env
    multi = {sc["name"]: sc["pins"] for N in (2, 3) for sc in D.position_scenes(N)}
    p = multi["one_late"]; assert p[(0, 0)][0] >= 7 and p[(0, 0)][1] and p[(0, 1)] == (1, 1, 0)
    p = multi["two_late"]; assert p[(0, 0)][0] > 3 and p[(0, 1)][0] > 3 and p[(0, 0)][0] != p[(0, 1)][0] and p[(0, 0)][1] and p[(0, 1)][1]
    p = multi["late_beside_stuck"]; assert p[(0, 0)][0] > 3 and p[(0, 0)][1] and 0 < p[(0, 1)][2] <= 3
    p = multi["states_0_1_2"]                         # defer_state 0 (keeps iterating), 2 (stuck within the grant) and 1 (solved) in one env
    assert p[(0, 0)][0] > 3 and p[(0, 0)][1] and 0 < p[(0, 1)][2] <= 3 and p[(0, 2)] == (1, 1, 0)
    p = multi["late_fixed_beside_4"]; assert p[(0, 0)] == (4, 1, 0) and 3 < p[(0, 2)][2] <= 7


def test_the_search_finds_the_pins_again(oracle):
    assert D.find_pins(oracle) == D.POSITION_PINS


def test_wheel_angle_for_is_the_f32_neighbour_of_the_limit():
    for ah in (0.0, 0.3, -1.7, 3.1, -6.5, 12.0):
        ah = np.float32(ah)
        for sign in "+-":
            at, inn = D.wheel_angle_for(ah, "at" + sign), D.wheel_angle_for(ah, "in" + sign)
            assert abs(np.float32(at - ah)) >= D.LIMIT and abs(np.float32(inn - ah)) < D.LIMIT
            assert inn == np.nextafter(at, np.float32(-np.inf if sign == "+" else np.inf)) and np.sign(at - ah) == (1 if sign == "+" else -1)


@pytest.mark.parametrize("N", sorted(D.CONFIGS))
def test_compositions_hold_exactly_the_stated_limit_states(oracle, N):
    """round by round: the limit states of the first step after the teleport are those the teleported angles give (every joint of every
    lane), each wavefront's limits sit where its role says and nowhere else, and over the rounds every full wavefront plays every role.
    With car<->car contacts enabled (N >= 2) no pair ever touches: the contact build runs these scenes with no manifold in the wavefront."""
    G, B = D.CONFIGS[N]; E, W = D.lanes(N)
    assert W == 3 and B > 2 * E and B - 2 * E < E, "two full wavefronts and a partial one"
    run = D.Run(oracle, [D.scene("composition", N)] * B, contacts=N > 1)
    seen = {w: set() for w in range(W)}
    reduce_where, solve_where, states = set(), set(), set()
    try:
        for k in range(D.ROUNDS):
            edits, rl, limited = D.composition(N, k)
            run.teleport(edits)
            want = D.expected_limits(np.stack([o.state()["bodies"] for o in run.orcs]))
            acts = D.composition_actions(N, k)
            for s in range(D.ROUND_STEPS):
                _, done, _, _ = run.step(acts[s])
                assert not done.any()
                cov = run.coverage()
                for e, o in enumerate(run.orcs):
                    assert np.isfinite(o.state()["bodies"]).all() and o.num_car_contacts() == 0, f"N {N} round {k} step {s} env {e}"
                if s:
                    continue
                got = np.stack([np.stack([c[f"lim_j{q}"] for q in range(4)], -1) for c in cov])
                assert np.array_equal(got, want), f"N {N} round {k}: limit states differ from what the teleported angles give in envs {np.nonzero((got != want).any((1, 2)))[0].tolist()}"
                form = D.wavefront_form(got, N)
                for w in range(W):
                    x = got[w * E:(w + 1) * E]
                    where = [(w * E + int(e), int(c), int(q) + 1) for e, c, q in np.argwhere(x != 0)]
                    role = rl[w]; seen[w].add(role)
                    if role == "none":
                        assert not where and form[w] == "free", f"N {N} round {k} wavefront {w}: limits at (env, car, wheel) {where}"
                    elif role == "mixed":
                        assert form[w] == "limited" and {1, 2} <= set(x[..., :2].ravel().tolist()) and {1, 2} <= set(x[..., 2:].ravel().tolist())
                    else:
                        assert where == [limited[w]], f"N {N} round {k} wavefront {w} ({role}): limits at {where}, stated {limited[w]}"
                        e, c, wheel = limited[w]
                        assert (wheel <= 2) == role.startswith("front") and form[w] == ("rear_free" if wheel <= 2 else "limited")
                        lane = (e - w * E) * G + c
                        assert lane == (0 if role.endswith("first") else (min((w + 1) * E, B) - w * E - 1) * G + N - 1)
                        if role.endswith("last") and w < 2:
                            assert lane == 63 - (G - N), "the last real lane of a full wavefront"
                        kind = ("front" if wheel <= 2 else "rear", int(x[e - w * E, c, wheel - 1]))
                        states.add(kind)
                        if cov[e]["reduce22"][c]: reduce_where.add(kind[0])
                        if cov[e]["solve33"][c] > cov[e]["reduce22"][c]: solve_where.add(kind[0])
    finally:
        run.close()
    assert seen[0] == seen[1] == set(D.FULL_ROLES) and seen[2] == set(D.PARTIAL_ROLES), seen
    _cache[("composition", N)] = (states, reduce_where, solve_where)


@pytest.mark.parametrize("N", [2, 5])
def test_compositions_with_a_touching_pair(oracle, N):
    """touching=True: in every round one env of every wavefront holds a touching pair on the first step, nobody else touches, and the limit
    states are still those the teleported angles give"""
    B = D.CONFIGS[N][1]
    run = D.Run(oracle, [D.scene("composition", N)] * B, contacts=True)
    try:
        for k in range(D.ROUNDS):
            edits, _, _ = D.composition(N, k, touching=True)
            run.teleport(edits)
            want = D.expected_limits(np.stack([o.state()["bodies"] for o in run.orcs]))
            acts = D.composition_actions(N, k)
            for s in range(D.ROUND_STEPS):
                _, done, _, _ = run.step(acts[s])
                assert not done.any() and all(np.isfinite(o.state()["bodies"]).all() for o in run.orcs)
                if s == 0:
                    got = np.stack([np.stack([c[f"lim_j{q}"] for q in range(4)], -1) for c in run.coverage()])
                    assert np.array_equal(got, want), f"N {N} round {k}"
                    assert [e for e, o in enumerate(run.orcs) if o.num_car_contacts()] == sorted(set(D.touching_envs(N))), f"N {N} round {k}"
    finally:
        run.close()


def test_compositions_reach_both_limits_and_both_branches_on_front_and_rear_joints(oracle):
    states, red, sol = set(), set(), set()
    for N in sorted(D.CONFIGS):
        if ("composition", N) not in _cache:
            test_compositions_hold_exactly_the_stated_limit_states(oracle, N)
        a, b, c = _cache[("composition", N)]; states |= a; red |= b; sol |= c
    assert states == {("front", 1), ("front", 2), ("rear", 1), ("rear", 2)}, states
    # (a rear joint's motor always turns the wheel back towards 0, away from the limit it sits at: on rear joints every limited sweep re-solves)
    assert red == {"front", "rear"} and "front" in sol, (red, sol)


def test_tyre_scenes_reach_every_branch_on_the_road_and_on_the_grass(oracle):
    scenes = D.tyre_scenes()
    run, log = played(oracle, "tyre", lambda: scenes)
    tot = total(run)
    for r in oracle.TYRE_ROWS:
        for s in ("road", "grass"):
            assert tot[f"{r}_{s}"] > 0, f"{r} on the {s}: never reached"
    assert tot["translation_clamp"] > 0 and tot["rotation_clamp"] > 0
    for e, sc in enumerate(scenes):
        w = sc["want"]; name = sc["name"]
        for (k, c), want in sc["pins"].items():
            assert D.outcome(log[k][e], c) == want, f"{name} step {k}: {D.outcome(log[k][e], c)}, pinned {want}"
        if w.get("translation_clamp"): assert log[0][e]["translation_clamp"][0] > 0, name
        if w.get("rotation_clamp"): assert log[0][e]["rotation_clamp"][0] > 0, name
        road = run.orcs[e].state()["on_road"][0].tolist()
        if w.get("surface") == "grass":
            assert road == [0, 0, 0, 0], f"{name}: on_road {road}"
        elif w.get("surface") == "split":                  # the left wheels (1, 3) on one surface, the right wheels (2, 4) on the other
            assert road in ([1, 0, 1, 0], [0, 1, 0, 1]), f"{name}: on_road {road}"
        else:
            assert road == [1, 1, 1, 1], f"{name}: on_road {road}"
        if "front_limit" in w:                             # the steered joints reach their stops by themselves, and stay there
            lim = [(int(log[k][e]["lim_j0"][0]), int(log[k][e]["lim_j1"][0])) for k in range(sc["steps"])]
            assert lim[0] == (0, 0) and lim[-1] == (w["front_limit"],) * 2, f"{name}: front limit states {lim}"
        if "steer_to_joint" in w:
            assert log[0][e]["steer_equal_road"][0] >= 1 and log[0][e]["lim_j0"][0] == 0, name
        if name.startswith("omega_"):
            assert all(log[k][e]["brake_unclamped_road"][0] + log[k][e]["brake_clamped_road"][0] == 4 for k in range(3)), name
    assert tot["brake_lock_road"] and tot["gas_falling_road"] and tot["brake_omega0_road"]


@pytest.mark.parametrize("N", [1, 2])
def test_the_sleep_rule_zeroes_on_the_stated_steps(oracle, N):
    scenes = D.sleep_scenes(N)
    run, log = played(oracle, ("sleep", N), lambda: scenes)
    for e, sc in enumerate(scenes):
        for c, want in sc["want"]["slept"].items():
            got = [k for k in range(sc["steps"]) if log[k][e]["slept"][c]]
            assert got == want, f"{sc['name']} car {c}: zeroed on steps {got}, stated {want}"
    if N == 1:                                             # the timers just below the rule: 0.48 s the step before it fires
        o = oracle.OracleEnv(1, car_contacts=False); o.reset(run.eps[0], render=False)
        for k in range(D.SLEEP_STEPS["idle"][0]):
            o.step(np.zeros((1, 3), np.float32), render=False)
        assert 0.47 < float(o.state()["sleep"].min()) < 0.5
        o.step(np.zeros((1, 3), np.float32), render=False)
        assert not o.state()["sleep"].any() and not o.state()["bodies"][..., 3:].any()
        o.close()


def test_every_coverage_row_is_reached(oracle):
    """over the whole scene set; `lim_equal` is the one row nothing can reach: the joints' limits are -0.4 and +0.4, and b2RevoluteJoint
    enters e_equalLimits only where lower == upper"""
    tot = {}
    for key, make in [(("pos", 1), lambda: D.position_scenes(1)), (("pos", 2), lambda: D.position_scenes(2)), ("tyre", D.tyre_scenes),
                      (("sleep", 1), lambda: D.sleep_scenes(1))]:
        for k, v in total(played(oracle, key, make)[0]).items():
            tot[k] = tot.get(k, 0) + v
    run = D.Run(oracle, [D.scene("composition", 2)] * D.CONFIGS[2][1])
    edits, _, _ = D.composition(2, 5)
    run.teleport(edits); run.step(D.composition_actions(2, 5)[0])
    for k, v in total(run).items():
        tot[k] = tot.get(k, 0) + v
    run.close()
    assert tot.pop("lim_equal") == 0
    assert set(tot) == set(oracle.DYNAMICS_ROWS) - {"lim_equal"}
    assert not [k for k, v in tot.items() if v == 0], [k for k, v in tot.items() if v == 0]
