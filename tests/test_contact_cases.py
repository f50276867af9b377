"""CPU, oracle only: every case of tests/contact_cases.py does what it is named for — the conditions tests/test_gpu_contact_kernel.py rests on.
Per case and env the oracle is stepped through the case once (module-scoped, shared by the tests below), with the coverage counters
(OracleEnv.contact_coverage) read after every step."""
import numpy as np
import pytest

from tests import contact_cases as C


@pytest.fixture(scope="module")
def runs(oracle):
    """{case: [per env: dict(steps=[per step dict(n, keys, cov, words)], cov=total, finite, final)]}; episodes > 1: the steps of all episodes in a
    row, `episode_cov` = per-episode totals"""
    out = {}
    for name, cs in C.CASES.items():
        out[name] = run_case(oracle, cs)
    return out


def run_case(O, cs, cap=None):
    fs = C.case_oracles(O, cs, cap=cap)
    res = [dict(steps=[], cov={}, episode_cov=[], finite=True, placed=[]) for _ in fs]
    for epi in range(cs["episodes"]):
        if epi:
            for f in fs:
                f.new_episode()
        st = C.scene_bodies(cs, np.stack([f.o.state()["bodies"] for f in fs]))
        for e, f in enumerate(fs):
            C.set_oracle_bodies(f.o, st[e]); f.o.contact_coverage(reset=True)
            res[e]["placed"].append(st[e]); ecov = {}
            for k in range(cs["steps"]):
                _, _, done, _ = f.o.step(C.actions(cs, k)[e], render=False)
                res[e]["finite"] &= not done                                  # (an episode that ends — a car off the playfield — is no use either)
                w = f.o.car_contacts(); cov = f.o.contact_coverage(reset=True)
                res[e]["steps"].append(dict(n=int(w[0]), keys=C.decode_keys(w), cov=cov, words=w))
                C.add_coverage(ecov, cov)
                res[e]["finite"] &= bool(all(np.isfinite(v).all() for v in f.o.state().values()))
            res[e]["episode_cov"].append(ecov); C.add_coverage(res[e]["cov"], ecov)
            res[e]["final"] = f.o.state()["bodies"]
    for f in fs:
        f.o.close()
    return res


@pytest.mark.parametrize("name", list(C.CASES))
def test_case_reaches_what_it_is_named_for(runs, name):
    cs = C.CASES[name]; res = runs[name]
    for row, envs in cs["reach"].items():
        for e in envs:
            assert res[e]["cov"][row] > 0, f"{name} env {e}: never reached {row}: {res[e]['cov']}"
    for e, (step, count) in cs["counts"].items():
        assert res[e]["steps"][step]["cov"]["max_candidates"] == count, f"{name} env {e} step {step}: {res[e]['steps'][step]['cov']['max_candidates']} touching pairs, {count} claimed"
    for e, r in enumerate(res):
        assert r["finite"], f"{name} env {e}: the state did not stay finite"
        per_episode = [r["steps"][i:i + cs["steps"]] for i in range(0, len(r["steps"]), cs["steps"])]
        for epi, steps in enumerate(per_episode):
            # the device runs the contact pass in front of the first step after set_bodies and beside the dynamics afterwards: both with contacts
            assert sum(s["n"] > 0 for s in steps) >= 3 and any(s["n"] > 0 for s in steps[1:]), f"{name} env {e} episode {epi}: manifolds per step {[s['n'] for s in steps]}"
        if not cs["cap"]:
            assert max(s["cov"]["max_candidates"] for s in r["steps"]) <= C.MCR_CC_MAX, f"{name} env {e}: an uncapped case beyond the store"
            assert all(s["words"][1] == 0 for s in r["steps"])
        else:
            assert all(s["n"] <= C.MCR_CC_MAX and int(s["words"][1]) == int(s["cov"]["max_candidates"] > C.MCR_CC_MAX) for s in r["steps"])


def test_geometry_scenes(runs):
    res = runs["geometry"]
    wheel = res[C.WHEEL_ONLY_ENV]["steps"]
    assert all((k[1] >= 4) != (k[3] >= 4) for s in wheel for k in s["keys"]) and sum(s["n"] for s in wheel) >= 4, "wheel-on-hull: a hull<->hull pair touched"
    for e in C.DEEP_ENVS:
        hull_pairs = {(k[1], k[3]) for k in res[e]["steps"][0]["keys"] if k[1] < 4 and k[3] < 4}
        assert len(hull_pairs) >= 3, f"deep overlap env {e}: hull polygon pairs {sorted(hull_pairs)}"
    assert all(s["keys"] == [(0, 3, 1, 0)] for s in res[0]["steps"]), "the anchor: one manifold, car 0's tail polygon on car 1's nose polygon"


def test_straddle_sits_on_both_sides_of_the_threshold(oracle, runs):
    res = runs["straddle"]; cs = C.CASES["straddle"]
    for e, r in enumerate(res):
        n = [s["n"] for s in r["steps"]]
        assert (n[0] > 0) == (e % 2 == 0) and n[1] > 0, f"env {e}: manifolds per step {n}"
    # the other side of each env's threshold is at most 2 ulps of a coordinate away
    for side in (0, 1):
        other = dict(cs, envs=[[(0.0, C.STRADDLE_LON[e][side], 0.0, 0.0, 0.5, 0.0)] for e in range(4)])
        r2 = run_case(oracle, other)
        for e in range(4):
            assert (r2[e]["steps"][0]["n"] > 0) == (side == 0), f"env {e} side {side}"
            a, b = res[e]["placed"][0][1, :, :2], r2[e]["placed"][0][1, :, :2]
            ulps = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max()
            assert ulps <= 2 and (ulps > 0) == (side != e % 2), f"env {e}: the two sides are {ulps} ulps apart"


def test_kinematics_scenes(runs):
    res = runs["kinematics"]
    assert any(s["n"] > 0 and s["cov"]["translation_clamp"] > 0 for s in res[C.FAST_ENVS[0]]["steps"]), "no translation clamp in a step with a live contact"
    for e in C.SPIN_CLAMP_ENVS:
        assert any(s["n"] > 0 and s["cov"]["rotation_clamp"] > 0 for s in res[e]["steps"]), f"env {e}: no rotation clamp in a step with a live contact"
    assert res[C.SPIN_CLAMP_ENVS[1]]["cov"]["rotation_clamp"] >= 2, "the +100 rad/s env clamps in more than one body-step"
    for e, name in ((C.END_BEGIN_ENV, "kinematics"),):
        n = "".join("1" if s["n"] else "0" for s in res[e]["steps"])
        assert "10" in n and "01" in n[n.index("10"):], f"{name} env {e}: no contact ended and began again: {n}"
    n = "".join("1" if s["n"] else "0" for s in runs["solver3"][2]["steps"])
    assert "10" in n and "01" in n[n.index("10"):], f"solver3 env 2: {n}"


def test_island_scenes(runs):
    res = runs["islands"]
    for e, cars in enumerate(C.ISLAND_CARS):
        assert res[e]["cov"]["max_island_cars"] == cars, f"islands env {e}: largest island {res[e]['cov']['max_island_cars']} cars"
    assert all(0 in (k[0], k[2]) for s in res[1]["steps"] for k in s["keys"]), "the star: two spokes touch each other"
    assert {c for k in res[1]["steps"][0]["keys"] for c in (k[0], k[2])} == set(range(7))
    touching = {c for k in res[2]["steps"][0]["keys"] for c in (k[0], k[2])}
    assert touching == {0, 1, 2, 3, 4}, f"two islands and three loose cars: cars with a contact {sorted(touching)}"
    assert not any({k[0], k[2]} & {0, 1, 2} and {k[0], k[2]} & {3, 4} for s in res[2]["steps"] for k in s["keys"])
    assert runs["cluster"][0]["cov"]["max_candidates"] >= 200 and runs["cluster"][0]["cov"]["max_island_cars"] == 8


def test_reused_worlds_flip_fixture_pairs(runs):
    """first episode: car a's fixture is fixtureA of every pair (a < b); later episodes of the same world hand out proxy ids off the tree's free
    list, and some pairs come the other way round"""
    for name in ("reuse2", "reuse4"):
        for e, r in enumerate(runs[name]):
            assert r["episode_cov"][0]["flipped"] == 0
        flipped = [[c["flipped"] for c in r["episode_cov"]] for r in runs[name]]
        assert sum(f[1] + f[2] for f in flipped) > 0, f"{name}: {flipped}"
        print(name, "flipped manifolds per env and episode", flipped)


@pytest.mark.parametrize("name", [n for n, c in C.CASES.items() if c["cap"]])
def test_cap_changes_the_result(oracle, runs, name):
    """with the cap the oracle drops pairs and leaves the uncapped oracle in the envs that overflow — and only there"""
    free = run_case(oracle, C.CASES[name], cap=False)
    for e, (a, b) in enumerate(zip(runs[name], free)):
        over = any(s["cov"]["max_candidates"] > C.MCR_CC_MAX for s in b["steps"])
        assert over == (a["cov"]["dropped"] > 0)
        assert np.array_equal(a["final"], b["final"]) == (not over), f"{name} env {e}: overflow {over}, same final bodies {np.array_equal(a['final'], b['final'])}"
        if over:
            s0 = a["steps"][0]; f0 = b["steps"][0]
            # THE DROP RULE: the first MCR_CC_MAX pairs by (car pair, fixture of the lower car * 8 + fixture of the higher car)
            order = sorted(f0["keys"], key=lambda k: ((k[0], k[2], k[1], k[3]) if k[0] < k[2] else (k[2], k[0], k[3], k[1])))
            assert sorted(s0["keys"]) == sorted(order[:C.MCR_CC_MAX]), f"{name} env {e}: kept {sorted(s0['keys'])}"


def test_coverage_table_has_no_zero_row(runs):
    total = {}
    for name, res in runs.items():
        for r in res:
            C.add_coverage(total, r["cov"])
    print("\ncoverage of the contact code by tests/contact_cases.py (oracle):")
    for k, v in total.items():
        print(f"  {k:20s} {v}")
    assert all(v > 0 for v in total.values()), f"rows never reached: {[k for k, v in total.items() if v == 0]}"
