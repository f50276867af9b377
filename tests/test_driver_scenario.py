"""The scripted driver (csrc/k_driver.h) in closed loop on the CPU oracle alone, through its float64 restatement (tests/driver_ref.py): the
conditions tests/test_gpu_driver.py rests on, as tests/test_lap_scenario.py holds them for the lap script.  A change of the controller's
definition or defaults after which it leaves the road, stalls or no longer completes a lap fails HERE instead of silently testing nothing on
the GPU.

Cases: N = 1, global envs 0..5 of seed 500 (the episodes of seeds 500..505), random direction, default parameters, TimeLimit 1000.
Measured with the exact restatement (mcr_sincos_host for the hull, libm for beta):

    env  direction   T   tiles visited   lap completed at step
    0    CW         269  269             832
    1    CCW        302  302             965
    2    CCW        287  287             922
    3    CCW        325  300             -   (TimeLimit)
    4    CW         278  278             908
    5    CW         302  302             964

and no step of any run with all four wheels of the car off the road.  The conditions below are these outcomes with some slack."""
import numpy as np
import pytest

from tests import driver_ref as D
from tests.util import oracle_episode

SCENARIO_SEED, SCENARIO_ENVS, TIME_LIMIT, DRIVER_LAP = D.SCENARIO_SEED, D.SCENARIO_ENVS, D.SCENARIO_TIME_LIMIT, D.DRIVER_LAP


def closed_loop(O, L, seed, g, params, limit=TIME_LIMIT):
    """N = 1: global env g of `seed` driven by the restatement until done or `limit` steps -> dict(T, tiles, lap_step or None, off_road_steps, direction)"""
    ep = oracle_episode(O, 1, seed, g, use_random_direction=True)
    o = O.OracleEnv(1)
    o.reset(ep, render=False)
    off = 0; lap = None
    for k in range(limit):
        a = D.of_oracle(L, o, ep, params)
        assert np.isfinite(a).all() and -1.0 <= a[0, 0] <= 1.0 and 0.0 <= a[0, 1] <= 1.0 and 0.0 <= a[0, 2] <= 1.0, f"env {g} step {k}: action {a[0]} outside the action space"
        _, _, done, _ = o.step(a, render=False)
        if not o.state()["on_road"][0].any():
            off += 1
        if done:
            lap = k + 1
            break
    out = dict(T=o.T, tiles=int(o.env_state()["tile_visited_count"][0]), lap_step=lap, off_road_steps=off, direction=ep["direction"])
    o.close()
    return out


@pytest.fixture(scope="module")
def runs(oracle, lib):
    L = lib.load()
    return {g: closed_loop(oracle, L, SCENARIO_SEED, g, D.default_params(1)) for g in SCENARIO_ENVS}


def test_driver_stays_on_the_road(runs):
    for g, r in runs.items():
        assert r["off_road_steps"] == 0, f"env {g}: {r['off_road_steps']} steps with all four wheels off the road"


def test_driver_visits_the_track(runs):
    for g, r in runs.items():
        assert r["tiles"] >= 0.85 * r["T"], f"env {g}: {r['tiles']} of {r['T']} tiles visited"


def test_driver_completes_laps(runs):
    laps = {g: r["lap_step"] for g, r in runs.items() if r["lap_step"] is not None and r["tiles"] == r["T"]}
    print("lap steps:", laps, "tiles:", {g: (r["tiles"], r["T"]) for g, r in runs.items()})
    assert len(laps) >= 4, f"only {len(laps)} of {len(runs)} runs completed the lap before step {TIME_LIMIT}: {laps}"
    assert all(s < TIME_LIMIT for s in laps.values())


def test_recorded_lap(runs):
    """the run the GPU lap test repeats: it completes its lap, at exactly the recorded step, in a run of the scenario"""
    seed, g, step = DRIVER_LAP
    assert seed == SCENARIO_SEED and g in runs
    assert runs[g]["lap_step"] == step and runs[g]["tiles"] == runs[g]["T"], runs[g]


def test_both_directions_are_covered(runs):
    assert {r["direction"] for r in runs.values()} == {"CW", "CCW"}
