"""Batched MultiCarRacing-v0 on one MI355X: B independent envs advanced by the HIP kernels behind
include/mcr.h.  torch is plumbing only (device memory, streams); every step is the C-ABI `mcr_step`.

Semantics per env follow the reference's `reset()`/`step()` (multi_car_racing.py:340-509) with the
TimeLimit(1000) of gym_multi_car_racing/__init__.py:8.  With `auto_reset=True` a finished env is re-spawned
on the device inside the same `step` call (its `obs` row is the first observation of the next episode,
its `done` row is 1) — the convention of baselines-style VecEnvs; with `terminal_obs=True` the LAST frame of the finished
episode (what the reference returns with done = True, multi_car_racing.py:431, :509) is handed out as well, as
info["terminal_observation"][i] for env info["terminal_env_ids"][i], i < info["terminal_count"].

Like the reference, every env keeps ONE b2World for its life (multi_car_racing.py:138; _destroy :173-181, reset :341): from an env's second
episode on the fixtures' broadphase proxy ids come off the world's free list — they order same-step tile events, i.e. which of two cars that
reach a tile in the same step is its first visitor (`1000/T` vs `(1 - 1/N)·1000/T`, :113-120), and name fixtureA of a car<->car contact (the
manifold's reference face: poses once cars touch).  The ids need no tree on the device: leaf ids never depend on the tree's shape, a per-env
stack of free leaf ids reproduces them (csrc/k_world.h), advanced by the env's reset pass inside `step`.  `fresh_world=True` is rounds 1-5's
definition instead — every episode the first episode of a fresh world —; measured against the reference's semantics on the oracle
(profiles/r06_world_reuse_effect.txt, 5 episodes back to back): 50-64 % of the (env, car) pairs of an even episode see a different reward in
some step, and with a policy that drives the tile-visit counts of 4-17 % of the envs differ at the end of episodes 2-5.

Determinism: env with global index g uses two numpy-compatible MT19937 streams,
  track stream  RandomState(seed + g)                (the reference's `env.np_random`)
  draw stream   RandomState((seed + g + 2**31) % 2**32)   (stands in for the reference's *global* np.random:
                direction choice then car order, multi_car_racing.py:351-357)
so results do not depend on B, on the GPU count, or on scheduling.

Observation format: `obs_format="rgb"` (default) hands out [B, N, 96, 96, 3] frames.  `obs_format="gray"` is gym's GrayScaleObservation
(OpenCV's fixed-point COLOR_RGB2GRAY, (4899 R + 9617 G + 1868 B + 8192) >> 14, of the bytes the RGB frame would hold), drawn by the raster
itself: [B, N, 96, 96].  With `frame_stack=k > 1` it is also gym's FrameStack(k): [B, N, k, 96, 96], oldest frame first, and after a reset or
an auto-reset the env's first frame k times (gym's rule; SB3's VecFrameStack zero-fills instead).  The stack is a strided VIEW of a ring of
2k frames per agent that the raster writes in place (include/mcr.h: mcr_set_obs_format): nothing is shifted or copied, and the view
changes with every step — keep the tensor step() returns, not an older one.  reset() and step() draw; the state setters (set_bodies(),
set_wheels(), set_env_state(), set_state_blob()) do not: refresh_obs() draws the state as it stands (frame_stack 1).

State-vector observation: `state_obs=True` adds what a non-pixel policy trains on, with `obs=True` or `obs=False`: `self.state`, a persistent
float32 device tensor [B, N, F] that a kernel of its own (csrc/k_stateobs.h: the feature table) rewrites after every reset() / reset_envs() /
step() on the stepping stream, also handed out as info["state"].  F = 18 + 2 * state_waypoints + 4 * (N - 1) raw, un-normalised features
per car: own velocity in the hull's frame, yaw rate, wheel speeds, steering angle, on-road bits, progress, offset and heading against the
nearest track point, the episode's direction, `state_waypoints` track points `state_stride` tiles apart ahead of the car, and the other
cars' relative positions and velocities.  The row of an env that auto-reset in the step describes the first state of its new episode, like
its `obs` row.  After set_bodies() / set_state_blob() call refresh_state().

Range-finder observation: `range_obs=True` adds what racing policies are usually trained on (TORCS's 19-ray `track` and `opponents`
sensors, F1TENTH's lidar), with `obs=True` or `obs=False`, with or without `state_obs`: `self.ranges`, a persistent float32 device tensor
[B, N, 2, R], also info["ranges"], that a kernel of its own (csrc/k_rangeobs.h: the definition) rewrites wherever `self.state` is rewritten.
Per car R rays leave the hull's body origin; channel 0 is the distance along a ray to the track's border (the road's edge; kerbs do not
count), channel 1 the distance to the nearest other car's HULL (its four polygons, so extent and orientation count), both clamped to
`range_max` world units (TRACK_WIDTH is 6.67).  The rays are `range_rays` angles np.linspace(-range_fov / 2, range_fov / 2, range_rays) — 0 is
straight ahead, positive angles lie towards the car's right, a single ray points ahead — or the explicit `range_angles`; `self.range_angles`
holds them (f64), `self.range_dirs` the float32 (cos, sin) table the kernel is given, `self.range_shape` = (N, 2, R).  With one car channel
1 is `range_max`.  At a folded inner hairpin the inner border can lie inside the road: channel 0 is the first border segment a ray meets.
After set_bodies() / set_state_blob() call refresh_ranges().

Grid observation: `grid_obs=True` adds the ego-centred bird's-eye-view tensor driving policies are usually trained on, with `obs=True` or
`obs=False` and beside every other observation: `self.grid`, a persistent uint8 device tensor [B, N, H, W], also info["grid"], that a kernel
of its own (csrc/k_gridobs.h: the definition) rewrites wherever `self.state` is rewritten.  `grid_shape=(H, W)` (1..64 each) cells of
`grid_cell` world units are fixed to the hull: row 0 is farthest ahead, column 0 leftmost, and the hull's body origin sits at
`grid_origin=(row, col)` in cell units (None: (0.75 H, 0.5 W), a quarter from the bottom; fractional or outside the grid if you wish).  A
byte says what lies under the cell's CENTRE: GRID_ROAD (1: road or kerb — a car there would not be driving_on_grass), GRID_FRESH (2: a tile
this car has not visited yet, so it still pays), GRID_TAKEN (4: a tile another car has visited, so the pay is dampened), GRID_CAR (8: another
car's hull).  "Under" is the reference's own strict-interior test in float64: a centre exactly on a tile's edge is in nothing.
`self.grid_shape` = (N, H, W); grid_planes() gives the four bits as [B, N, 4, H, W] planes of 0/1.  With one car GRID_TAKEN and GRID_CAR are
never set.  After set_bodies() / set_env_state() / set_state_blob() call refresh_grid().

Car-contact observation: `contact_obs=True` (needs `num_agents >= 2` and `car_contacts=True`) reports the one thing that makes the simulator
multi-car — who touched whom in the step, and how hard — with `obs=True` or `obs=False`: `self.contact_mask`, a persistent int32 device
tensor [B, N], also info["contact_mask"], and `self.contact_impulse`, float64 [B, N, N], also info["contact_impulse"], that a kernel of its
own (csrc/k_contactobs.h: the definition) rewrites wherever `self.state` is rewritten, from the car<->car manifolds the env keeps for warm
starting — what Box2D's PostSolve would report.  Bit j of `contact_mask[e, a]` (j < 8): a fixture of car a touched one of car j in the
step; bit 8: with its hull; bit 9: with a wheel.  `contact_impulse[e, a, j]` is the sum of the normal impulses of all manifold points
between the two cars, one f64 add per point in a fixed order (bit for bit reproducible: tests/contact_obs_ref.py); the matrix is symmetric to
the bit and its diagonal is 0.  With `frame_skip=k` the kernel runs behind every env step: impulses are summed in step order, masks OR-ed.
The env step in which an episode ends is never reported: the row of an env that auto-reset in the step describes the first state of its new
episode (no contacts), like its `state` row, and with `frame_skip > 1` an env that ended early keeps what the env steps before the ending
one summed.  After reset() / reset_envs() / load_states() / clone_envs() a row shows what the state's last env step produced (a clone: its
source's).  Where an env's store overflowed (status word 2: more than 24 touching fixture pairs) the outputs describe the 24 kept records.
refresh_contacts() recomputes both tensors from the stores as they stand.

Early episode ending: `end_patience=P` ends an episode when the counted cars (`end_agents`, default all; for a learner racing scripted cars
pass the learners) have visited no new tile for P env steps, `end_offroad=G` when every counted car (`end_offroad_mode="all"`) or some counted
car ("any") has had no wheel on a tile for G env steps in a row; 0 turns a rule off, both 0 (the default) the feature.  A kernel of its own
(csrc/k_endrules.h: the definition; tests/end_rules_ref.py: the same as a wrapper round the oracle) counts behind every env step taken with
actions — step(None) counts nothing and ends nothing — in `self.end_counters`, int32 [B, 4] = idle, offroad, tvc_sum, 0, which the CALLER owns
(load_states() leaves them alone: save and restore the rows beside the states).  The episode ends in the env step AFTER the one in which a rule
was first met — one step of lag, the price of leaving the step's kernels as they are — exactly as under the TimeLimit: `truncated = !done`,
`done = 1`, then auto-reset, episode statistics, terminal observations, level statistics as ever; `end_reward` (default 0.0) is added to every
car's reward of that step, one f64 add.  `self.end_reason` = info["end_reason"], uint8 [B]: 0, or why the step ended the episode by these
rules (bit 0 idle, bit 1 off-road; OR-ed over a macro-step's env steps); `truncated = 0` beside it says that the reference's own rules or the
TimeLimit ended the episode in the same env step; after step(None) it is 0.  With `auto_reset=False` an env stepped past such an ending reports `done` in every step
while its rule holds, until reset_envs().  refresh_end_rules() after writing the counters yourself.

Action repeat: `frame_skip=k` (1..16) makes step() one MACRO-step, gym's FrameSkip_k(TimeLimit(env)) per env with the auto-reset outside it
(include/mcr.h: mcr_step_repeat): the same actions drive up to k env steps of every env, an env stops at the step that ends its episode,
`reward` is the f64 sum of the env steps' rewards in order, `done` their OR, `truncated` the ending step's; `max_episode_steps`,
`episode_length` and `refill_lag` keep counting env steps.  Observations are drawn once, from the state after the last env step, so a
`frame_stack` holds policy-step frames (FrameStack(FrameSkip(env))) and `self.state` is written once.  With `auto_reset` an env whose episode
ended inside the macro-step shows the first observation of its next episode, which that macro-step has not advanced.  `frame_skip=1` is
the plain step.  Not with `terminal_obs=True`, and step(None) — reset()'s action-less step — needs `frame_skip=1`.

Batched snapshots: `save_states()`, `load_states()` and `clone_envs()` are get_state_blob / set_state_blob for many envs at once, as one
kernel each (csrc/k_envcopy.h; include/mcr.h: mcr_save_states) — for planning with the simulator as the model (fork a state into K
candidates, roll them out, rewind), restore-to-state exploration and checkpoints of the envs.  They are STREAM-ORDERED and ASYNCHRONOUS:
enqueued on the current stream, which must be the stepping stream, with ids that may live on the device; nothing synchronises unless
load_states(check=True) is asked to validate on the host.  The blob rows are byte for byte what get_state_blob returns.  The staging
protocol stays the target's: an env restored or cloned on an `auto_reset=True` handle continues with that handle's own next staged episode
when its episode ends (set_state_blob's rule) — planning handles are normally created with `auto_reset=False`.  Observations are not part
of the state: clone_envs copies the rows of `obs`, load_states leaves them to the next step (and refuses `frame_stack > 1`).

Level pools: by default every episode of every env is a brand-new random track, generated by host threads and copied over PCIe while the
rollout runs.  `levels=K` plays a FINITE set of K tracks instead (procgen's `num_levels`: train on K levels, evaluate on held-out ones;
fixed-track evaluation; per-track return statistics): the K episodes are generated once, by the same bit-exact generator
(multi_car_racing_amd/levels.py: level j is the first episode of global env j under `level_seed`, default `seed`), uploaded once, and from
then on a kernel re-stages every env that re-spawned from the resident pool (csrc/k_pool.h; include/mcr.h: mcr_set_episode_pool) — no
refill service, no worker thread, no host work per step, and an env can never freeze waiting for a track (`gen_threads`, `async_refill`
and `refill_lag` are ignored).  `levels` may also be a uint8 array [K, episode_bytes] of the caller's own blobs.  Env with global index g
plays level levels.pool_level(seed, g, k, K, level_order) in its k-th episode — `level_order="random"` a counter-based hash, `"cycle"`
(g + k) % K — so rollouts do not depend on B, sharding or scheduling.  `self.level` (int32 device tensor [B], also info["level"]) is the
pool row of each env's CURRENT episode; `self.level_info` the [K, 12] info rows (T, P, retries, cw, car order) of a generated pool, None
for caller blobs.  Snapshots: clone_envs copies the `level` rows; load_states sets them to -1 (a state blob does not say which level it
came from); either way the env goes on with its OWN next level when the restored episode ends (the staging words stay the target's).

Level curricula: the two halves of a loop that stays on the device — `w = f(vec.level_stats); vec.set_level_weights(w)` — with no
synchronisation and no host work per step (include/mcr.h: mcr_set_level_stats, mcr_set_level_sampler).
`level_stats=True` (needs `levels`): behind every step() a kernel (csrc/k_levelstats.h) rewrites `self.finished_level` (int32 [B], also
info["finished_level"]): -1 where `done` is 0, else the level of the episode that just ENDED — `self.level` already names the new one —
or K, the "unattributed" row, when that level is unknown (a `level` row of -1 after load_states; after clone_envs a clone's episode counts
for the source's level, whose row was copied).  The same kernel adds the episode to row `finished_level[e]` of `self.level_stats`
(float64 [K + 1, 3 + 2N], also level_stats_now()): column 0 episodes, 1 those with `truncated` set, 2 the sum of `episode_length`,
3..3+N the sum of `episode_return` per car, 3+N..3+2N the sum of its squares; row K collects the unattributed episodes, so nothing is
dropped silently.  Counting rule, rollout_stats()'s: a `done` row counts once per step() call that reports it — once per macro-step with
`frame_skip`; with `auto_reset=False` an env that keeps being stepped past its end reports `done`, and counts, again in every call until
reset_envs().  Per row and column the additions happen in step order and within a step in ascending env index, one f64 add each: a host
reproduces every bit (tests/level_stats_ref.py); no floating-point atomics.  reset_level_stats() zeroes the tensor in stream order.  The
statistics are per handle, hence per rank (sharded.py): a job may all_reduce `level_stats`; the sums then depend on the world size in
their last bits.
`level_order="weighted"`: env g plays in its k-th episode level levels.weighted_level(seed, g, k, cdf) — "random"'s hash as an f64 uniform
in [0, 1), mapped through the CDF of the weights (levels.level_cdf: running f64 sum in index order over the total; a weight that is not
finite or is negative counts as 0; a zero-weight level is never drawn).  A new handle draws uniformly; set_level_weights(w) rebuilds the CDF
(`self.level_cdf`, float64 [K]) with one small kernel on the stepping stream.  An env's NEXT episode is staged — and its level drawn, from
the CDF in force at that point of the stream — behind the reset or step in which it installed its current one: new weights act with a
LAG OF ONE EPISODE per env (Prioritized Level Replay tolerates that).  Rollouts stay a pure function of (seed, g, k, the sequence of
set_level_weights calls in stream order): independent of B and of sharding, provided every rank sets the same weights at the same steps.
The drawn level is staging state, like the staged episode: load_states and clone_envs leave it the target's.

Scripted drivers: `scripted_agents=(1,)` lets the DEVICE drive the listed cars — opponents for a learner, or (all cars) a baseline policy —
with a stateless track-following controller (csrc/k_driver.h holds the definition; `drivers.DRIVER_DEFAULTS` the default parameters;
`driver_params` overrides them: a dict {name: scalar or per-car sequence} or a float array [N, 10]).  step(actions) then runs one kernel in
front of the step that writes `self.actions`, a persistent float32 device tensor [B, N, 3]: the controller's action for every scripted car
(computed from the state BEFORE the step; the caller's rows for those cars are ignored), a copy of the caller's row for every other car.
The step is driven by that tensor, which is also info["actions"] — the actions the step applied; the caller's tensor is never written.
With `frame_skip=k` the controller is evaluated once per step() call, like the learner's policy (a scripted car sits under the same
FrameSkip wrapper).  A caller who scripts ALL N cars still passes a [B, N, 3] tensor (its contents are ignored): step(None) stays the
reference's action-less step for every car, with no driver.  `expert_actions()` returns the controller's action for EVERY car from the
current state ([B, N, 3], no step, no synchronisation: labels for imitation learning / DAgger); it needs `scripted_agents` or
`driver_params` (`driver_params={}` = the defaults, no car scripted).  An action is a pure function of the env's state, its episode and
`self.driver_params` ([N, 10]): snapshots, clones, level pools, sharding and every step path need nothing new.  The controller follows
the track on a free road; on its own it does not avoid collisions, overtake, or recover from a spin or from the grass.
`racecraft=True` (or a dict of overrides {name: scalar or per-car sequence}, optionally with "agents": the cars it applies to, or a float
array [N, 8]; `drivers.RACECRAFT_DEFAULTS`) gives the scripted cars racecraft, still stateless (csrc/k_driver.h): a car looks at every other
car of its env, moves its line to the free side of the car ahead when that car sits on it, holds the leader's speed while it is still
behind it, and slows down when it is off the road.  It needs `scripted_agents` or `driver_params`; `self.racecraft_params` ([N, 8]) and
`self.racecraft_agents` report what is set (None and () when off), and `expert_actions()` uses it for the same cars.
"""
import atexit
import collections
import ctypes
import math
import weakref
import os
import queue
import threading
import time

import numpy as np
import torch

from . import _lib
from . import drivers as _drivers

_DIRECTION_MODE = {"CCW": 0, "CW": 1}


_LIVE = weakref.WeakSet()


def _close_all():
    """Interpreter exit with envs still open (e.g. after an exception): stop the refill threads before the runtime is
    torn down — a worker inside the native generator at that moment would abort the process."""
    for env in list(_LIVE):
        try:
            env.close()
        except Exception:
            pass


atexit.register(_close_all)


def range_obs_table(range_rays=19, range_fov=math.pi, range_angles=None, range_max=100.0):
    """The rays of the range-finder observation (module docstring), validated on the host: (angles f64 [R], dirs f32 [R, 2] = np.cos / np.sin
    of the angles cast to float32, max range as a float).  ValueError for a ray count outside 1..32, angles that are not finite or not a
    1-D sequence, a field of view that is not finite, or a range_max that is not finite or <= 0."""
    if range_angles is not None:
        angles = np.array(range_angles, dtype=np.float64)
        if angles.ndim != 1:
            raise ValueError("range_angles must be a 1-D sequence of angles")
    else:
        if isinstance(range_rays, bool) or not isinstance(range_rays, (int, np.integer)) or not 1 <= int(range_rays) <= _lib.RANGE_RAYS_MAX:
            raise ValueError(f"range_rays must be an int 1..{_lib.RANGE_RAYS_MAX}, got {range_rays!r}")
        fov = float(range_fov)
        if not math.isfinite(fov):
            raise ValueError(f"range_fov must be finite, got {range_fov!r}")
        angles = np.linspace(-fov / 2, fov / 2, int(range_rays)) if int(range_rays) > 1 else np.zeros(1, np.float64)
    if not 1 <= len(angles) <= _lib.RANGE_RAYS_MAX:
        raise ValueError(f"the range-finder takes 1..{_lib.RANGE_RAYS_MAX} rays, got {len(angles)}")
    if not np.isfinite(angles).all():
        raise ValueError("range_angles must be finite")
    rmax = float(range_max)
    if not math.isfinite(rmax) or not 0 < rmax <= float(np.finfo(np.float32).max):
        raise ValueError(f"range_max must be finite and > 0, got {range_max!r}")
    dirs = np.ascontiguousarray(np.stack([np.cos(angles), np.sin(angles)], axis=1).astype(np.float32))
    return angles, dirs, rmax


def grid_obs_geometry(grid_shape=(32, 32), grid_cell=1.5, grid_origin=None):
    """The geometry of the grid observation (module docstring), validated on the host: (H, W, cell, origin_row, origin_col), the last three as
    the float32 values the kernel is given.  ValueError for a shape that is not two ints 1..64, a cell that is not finite or <= 0 (as
    float32), or an origin that is not two finite numbers."""
    try:
        H, W = grid_shape
    except (TypeError, ValueError):
        raise ValueError(f"grid_shape must be (rows, cols), got {grid_shape!r}") from None
    for v in (H, W):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= _lib.GRID_MAX:
            raise ValueError(f"grid_shape must be two ints 1..{_lib.GRID_MAX}, got {grid_shape!r}")
    H, W = int(H), int(W)
    try:
        with np.errstate(all="ignore"):
            cell = np.float32(grid_cell)
    except (TypeError, ValueError):
        raise ValueError(f"grid_cell must be a number, got {grid_cell!r}") from None
    if not np.isfinite(cell) or not cell > 0:
        raise ValueError(f"grid_cell must be finite and > 0 as float32, got {grid_cell!r}")
    if grid_origin is None:
        grid_origin = (0.75 * H, 0.5 * W)
    try:
        orow, ocol = grid_origin
        with np.errstate(all="ignore"):
            orow, ocol = np.float32(orow), np.float32(ocol)
    except (TypeError, ValueError):
        raise ValueError(f"grid_origin must be (row, col) or None, got {grid_origin!r}") from None
    if not (np.isfinite(orow) and np.isfinite(ocol)):
        raise ValueError(f"grid_origin must be finite as float32, got {grid_origin!r}")
    return H, W, float(cell), float(orow), float(ocol)


END_OFFROAD_MODE = {"all": 0, "any": 1}


def end_rules_config(num_agents, end_patience, end_offroad, end_offroad_mode, end_agents, end_reward):
    """The end-rule keywords of VecMultiCarRacing, validated on the host: None when both patiences are 0 (the feature is off, whatever the
    other keywords say), else (patience, offroad patience, mode, counted cars as a sorted tuple, end_reward)."""
    N = int(num_agents)
    for name, v in (("end_patience", end_patience), ("end_offroad", end_offroad)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= 2 ** 31 - 1:
            raise ValueError(f"{name} must be an int in 0 .. 2^31 - 1 (0: off), got {v!r}")
    if end_offroad_mode not in END_OFFROAD_MODE:
        raise ValueError(f"end_offroad_mode must be one of {sorted(END_OFFROAD_MODE)}, got {end_offroad_mode!r}")
    try:
        reward = float(end_reward)
    except (TypeError, ValueError):
        raise ValueError(f"end_reward must be a finite float, got {end_reward!r}") from None
    if not np.isfinite(reward):
        raise ValueError(f"end_reward must be a finite float, got {end_reward!r}")
    if end_agents is None:
        cars = tuple(range(N))
    else:
        try:
            cars = tuple(sorted(set(int(a) for a in end_agents)))
            ok = all(isinstance(a, (int, np.integer)) and not isinstance(a, bool) for a in end_agents)
        except (TypeError, ValueError):
            raise ValueError(f"end_agents must be None or a sequence of car indices, got {end_agents!r}") from None
        if not ok or not cars or cars[0] < 0 or cars[-1] >= N:
            raise ValueError(f"end_agents must name at least one car in 0 .. {N - 1}, got {end_agents!r}")
    if int(end_patience) == 0 and int(end_offroad) == 0:
        return None
    return int(end_patience), int(end_offroad), end_offroad_mode, cars, reward


class VecMultiCarRacing:
    def __init__(self, num_envs, num_agents=2, device=None, seed=0, env_offset=0, direction="CCW",
                 use_random_direction=True, backwards_flag=True, h_ratio=0.25, use_ego_color=False,
                 obs=True, auto_reset=True, max_episode_steps=1000, car_contacts=True,
                 gen_threads=None, async_refill=True, streams=None, refill_lag=64, world_size=1, graph=None,
                 skid_particles=False, terminal_obs=False, terminal_cap=None, fresh_world=False, obs_format="rgb", frame_stack=1,
                 state_obs=False, state_waypoints=6, state_stride=5, frame_skip=1, levels=None, level_seed=None, level_order="random",
                 level_stats=False,
                 scripted_agents=None, driver_params=None, racecraft=None, range_obs=False, range_rays=19, range_fov=math.pi, range_angles=None,
                 range_max=100.0, contact_obs=False, grid_obs=False, grid_shape=(32, 32), grid_cell=1.5, grid_origin=None,
                 end_patience=0, end_offroad=0, end_offroad_mode="all", end_agents=None, end_reward=0.0):
        # scripted drivers (module docstring): validated on the host before anything is created
        drv_mask = _drivers.driver_mask(num_agents, scripted_agents)
        drv_rows = _drivers.driver_params_array(num_agents, driver_params) if (drv_mask or driver_params is not None) else None
        rc_rows, rc_mask = _drivers.racecraft_params_array(num_agents, racecraft, drv_mask)
        if rc_rows is not None and drv_rows is None:
            raise ValueError("racecraft needs scripted_agents or driver_params (there is no scripted driver to apply it to)")
        range_table = range_obs_table(range_rays, range_fov, range_angles, range_max) if range_obs else None
        grid_geom = grid_obs_geometry(grid_shape, grid_cell, grid_origin) if grid_obs else None
        if contact_obs and (int(num_agents) < 2 or not car_contacts):
            raise ValueError("contact_obs=True needs num_agents >= 2 and car_contacts=True (there is no car<->car manifold store otherwise)")
        end_rules = end_rules_config(num_agents, end_patience, end_offroad, end_offroad_mode, end_agents, end_reward)
        frame_skip = int(frame_skip)
        if not 1 <= frame_skip <= _lib.REPEAT_MAX:
            raise ValueError(f"frame_skip must be 1..{_lib.REPEAT_MAX}, got {frame_skip}")
        if frame_skip > 1 and terminal_obs:
            raise ValueError("frame_skip > 1 cannot be combined with terminal_obs=True (the terminal frame would belong to an env step that draws nothing)")
        if levels is not None:            # (checked before anything is created)
            if level_order not in _lib.LEVEL_ORDER and level_order != "weighted":
                raise ValueError(f"level_order must be one of {sorted(_lib.LEVEL_ORDER) + ['weighted']}, got {level_order!r}")
            if isinstance(levels, (int, np.integer)) and not isinstance(levels, bool):
                if int(levels) < 1:
                    raise ValueError(f"levels must be at least 1, got {levels}")
            elif (not isinstance(levels, np.ndarray) or levels.dtype != np.uint8 or levels.ndim != 2 or levels.shape[0] < 1
                  or levels.shape[1] != _lib.episode_bytes()):
                raise ValueError(f"levels must be an int K >= 1 or a uint8 array [K, {_lib.episode_bytes()}] of episode blobs")
        elif level_stats:
            raise ValueError("level_stats=True needs a level pool (levels=...)")
        if not torch.cuda.is_available():
            raise _lib.McrError("VecMultiCarRacing needs a HIP device: the step path has no CPU fallback")
        self.L = _lib.load()
        self.B, self.N = int(num_envs), int(num_agents)
        self.env_offset = int(env_offset)
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        torch.cuda.set_device(self.device)
        self.obs_enabled = bool(obs)
        if obs_format not in ("rgb", "gray"):
            raise ValueError(f"obs_format must be 'rgb' or 'gray', got {obs_format!r}")
        frame_stack = int(frame_stack)
        if obs_format == "rgb" and frame_stack != 1:
            raise ValueError("frame_stack > 1 needs obs_format='gray'")
        if not 1 <= frame_stack <= _lib.OBS_STACK_MAX:
            raise ValueError(f"frame_stack must be 1..{_lib.OBS_STACK_MAX}, got {frame_stack}")
        if (obs_format != "rgb" or frame_stack != 1) and not self.obs_enabled:
            raise ValueError("obs_format / frame_stack need obs=True")
        if 0 < int(max_episode_steps) < frame_stack:
            raise ValueError("max_episode_steps must be 0 or at least frame_stack: a terminal stack reads the ring copies of the episode's last "
                             "frame_stack - 1 frames")
        self.obs_format, self.frame_stack = obs_format, frame_stack
        self.frame_skip = frame_skip      # env steps per step() call (include/mcr.h: mcr_step_repeat)
        if streams is None:           # contact side stream (include/mcr.h: num_streams) pays as soon as there is a batch
            streams = 2 if int(num_envs) >= 64 and int(num_agents) > 1 and car_contacts else 1
        self.auto_reset = bool(auto_reset)
        self.direction_mode = 2 if use_random_direction else _DIRECTION_MODE[direction]
        # host threads of the track generator: the ranks of one node share the cores the cgroup allows.  (No core is set aside for
        # the stepping thread: it sleeps at its fences — blocking events — and one generator thread per rank runs at ~85 % duty at
        # 12 M env-steps/s, too close to the edge: bench.py --emulate-world 8 measured 10.9 M with one thread on a 2-core share)
        self.gen_threads = gen_threads or max(1, _lib.effective_cpus() // max(1, int(world_size)))
        # A re-spawned env consumes its staged episode; the refill thread generates + stages the next one.  An env could
        # only FREEZE (k_dynamics: inactive, zero outputs until the episode arrives) if it finished a whole episode before
        # that refill landed, so step() waits for any refill batch queued more than `refill_lag` steps ago — fewer steps
        # than any episode can last (a car needs a few hundred steps to leave the playfield from the track; a TimeLimit
        # shorter than the lag shortens it) — and the freeze path stays a safety net (debug_counters()[3] counts its
        # env-steps).  (8 steps until round 3: at 0.28 ms per step that is 2 ms for generate + stage + a blocking event
        # on a 2-core host share, and step() sat in wait_refills() 80 % of the time with the cores 2/3 busy.)
        self.refill_lag = max(1, min(int(refill_lag), int(max_episode_steps) - 1)) if int(max_episode_steps) > 0 else max(1, int(refill_lag))
        self._step_idx = 0
        self.blocked_s = 0.0          # wall time step() spent waiting for the refill thread (host behind the device)
        self._pending = collections.deque()      # step index at which each queued refill batch was queued
        self._pending_lock = threading.Lock()
        self._worker_exc = None
        self._hold_refills = False    # tests: withhold staging to exercise the freeze/thaw path
        cfg = _lib.Config(self.B, self.N, self.device.index or 0, int(self.obs_enabled), int(self.auto_reset),
                          int(backwards_flag), int(use_ego_color), int(car_contacts), int(max_episode_steps), int(streams),
                          float(h_ratio), int(bool(skid_particles)), int(bool(fresh_world)))
        self.fresh_world = bool(fresh_world)
        self.h = ctypes.c_void_p()
        _lib.check(self.L.mcr_create(ctypes.byref(cfg), ctypes.byref(self.h)), "mcr_create")
        self._status_now = np.zeros(8, np.uint32); self._status_seen = np.zeros(8, np.uint32)
        self._bound_streams = set()   # caller streams already handed to mcr_bind_stream (the check synchronises the device: once per stream)
        if int(self.L.mcr_step_ordering(self.h)) & 4:
            import warnings
            warnings.warn("another VecMultiCarRacing of this process holds this device's phase-word ordering: this one orders the streams "
                          "of its step with events (same results, about 0.02 ms more per step)", _lib.McrWarning, stacklevel=2)
        if graph is None:             # hipGraph replay of the step: measured r02 at B=4096 — 0.433 vs 0.435 ms per step, i.e. the gaps
            graph = False             # between the step's dependent kernels are drain/start-up on the GPU, not host launch cost: off
        _lib.check(self.L.mcr_set_step_graph(self.h, int(bool(graph))), "mcr_set_step_graph")
        if obs_format == "gray":
            _lib.check(self.L.mcr_set_obs_format(self.h, _lib.OBS_GRAY, frame_stack), "mcr_set_obs_format")
        # the shape of one env's observation as step() hands it out (learners size their buffers from it)
        self.obs_shape = ((self.N, 96, 96, 3) if obs_format == "rgb" else (self.N, 96, 96) if frame_stack == 1
                          else (self.N, frame_stack, 96, 96)) if self.obs_enabled else None
        # persistent outputs (overwritten by every step).  Stacked gray: self._ring [B, N, 2k, 96, 96] is what the raster writes; self.obs
        # is the window of the last drawing step (_window)
        self._ring = None
        if self.obs_enabled and frame_stack > 1:
            self._ring = torch.zeros((self.B, self.N, 2 * frame_stack, 96, 96), dtype=torch.uint8, device=self.device)
            assert self._ring[0, 0].numel() == int(self.L.mcr_obs_bytes_per_view(self.h))
            self.obs = self._window()
        elif self.obs_enabled:
            self.obs = torch.zeros((self.B,) + self.obs_shape, dtype=torch.uint8, device=self.device)
            assert self.obs[0, 0].numel() == int(self.L.mcr_obs_bytes_per_view(self.h))
        else:
            self.obs = None
        self.reward = torch.zeros((self.B, self.N), dtype=torch.float64, device=self.device)
        self.done = torch.zeros((self.B,), dtype=torch.uint8, device=self.device)
        self.truncated = torch.zeros((self.B,), dtype=torch.uint8, device=self.device)
        # episode statistics, valid in the rows where `done` is set (overwritten when that env's next episode ends)
        self.episode_return = torch.zeros((self.B, self.N), dtype=torch.float64, device=self.device)
        self.episode_length = torch.zeros((self.B,), dtype=torch.int32, device=self.device)
        _lib.check(self.L.mcr_set_episode_stats(self.h, ctypes.c_void_p(self.episode_return.data_ptr()), ctypes.c_void_p(self.episode_length.data_ptr())), "mcr_set_episode_stats")
        # terminal observations (include/mcr.h: mcr_set_terminal_obs): the last frame of every episode that ends in a step, next to the first
        # frame of the next episode that the env's row of `obs` shows.  Compact: entry i belongs to env terminal_env_ids[i], i < terminal_count.
        self.terminal_obs = self.terminal_env_ids = self.terminal_count = None
        if terminal_obs:
            if not (self.obs_enabled and self.auto_reset):
                raise ValueError("terminal_obs needs obs=True and auto_reset=True")
            cap = self.B if terminal_cap is None else max(1, min(int(terminal_cap), self.B))
            self.terminal_obs = torch.zeros((cap,) + self.obs_shape, dtype=torch.uint8, device=self.device)
            self.terminal_env_ids = torch.zeros((cap,), dtype=torch.int32, device=self.device)
            self.terminal_count = torch.zeros((1,), dtype=torch.int32, device=self.device)
            _lib.check(self.L.mcr_set_terminal_obs(self.h, ctypes.c_void_p(self.terminal_obs.data_ptr()), ctypes.c_void_p(self.terminal_env_ids.data_ptr()),
                                                   ctypes.c_void_p(self.terminal_count.data_ptr()), cap), "mcr_set_terminal_obs")
        # state-vector observation (include/mcr.h: mcr_set_state_obs): [B, N, F] f32, rewritten by every reset / step on the stepping stream
        self.state = None
        self.state_shape = None
        if state_obs:
            F = _lib.state_obs_dim(self.N, int(state_waypoints))
            self.state = torch.zeros((self.B, self.N, F), dtype=torch.float32, device=self.device)
            self.state_shape = (self.N, F)
            _lib.check(self.L.mcr_set_state_obs(self.h, ctypes.c_void_p(self.state.data_ptr()), int(state_waypoints), int(state_stride)), "mcr_set_state_obs")
        # range-finder observation (include/mcr.h: mcr_set_range_obs): [B, N, 2, R] f32, rewritten where self.state is
        self.ranges = self.range_shape = self.range_angles = self.range_dirs = self.range_max = None
        if range_table is not None:
            self.range_angles, self.range_dirs, self.range_max = range_table
            R = len(self.range_angles)
            self.ranges = torch.zeros((self.B, self.N, 2, R), dtype=torch.float32, device=self.device)
            self.range_shape = (self.N, 2, R)
            _lib.check(self.L.mcr_set_range_obs(self.h, ctypes.c_void_p(self.ranges.data_ptr()), _lib.ptr(self.range_dirs), R,
                                                ctypes.c_float(self.range_max)), "mcr_set_range_obs")
        # grid observation (include/mcr.h: mcr_set_grid_obs): [B, N, H, W] u8, rewritten where self.state is
        self.grid = self.grid_shape = self.grid_cell = self.grid_origin = None
        if grid_geom is not None:
            gh, gw, self.grid_cell, orow, ocol = grid_geom
            self.grid_origin = (orow, ocol)
            self.grid = torch.zeros((self.B, self.N, gh, gw), dtype=torch.uint8, device=self.device)
            self.grid_shape = (self.N, gh, gw)
            _lib.check(self.L.mcr_set_grid_obs(self.h, ctypes.c_void_p(self.grid.data_ptr()), gh, gw, ctypes.c_float(self.grid_cell),
                                               ctypes.c_float(orow), ctypes.c_float(ocol)), "mcr_set_grid_obs")
        # car-contact observation (include/mcr.h: mcr_set_contact_obs): [B, N] int32 and [B, N, N] f64, rewritten where self.state is and behind
        # every env step of a macro-step
        self.contact_mask = self.contact_impulse = None
        if contact_obs:
            self.contact_mask = torch.zeros((self.B, self.N), dtype=torch.int32, device=self.device)
            self.contact_impulse = torch.zeros((self.B, self.N, self.N), dtype=torch.float64, device=self.device)
            _lib.check(self.L.mcr_set_contact_obs(self.h, ctypes.c_void_p(self.contact_mask.data_ptr()),
                                                  ctypes.c_void_p(self.contact_impulse.data_ptr())), "mcr_set_contact_obs")
        # early episode ending (include/mcr.h: mcr_set_end_rules): [B, 4] int32 counters the caller owns (idle, offroad, tvc_sum, 0), the armed
        # bytes beside them and [B] u8 end_reason, all advanced by a kernel of its own behind every env step taken with actions
        self.end_counters = self.end_armed = self.end_reason = None
        self.end_patience, self.end_offroad, self.end_offroad_mode, self.end_agents, self.end_reward = end_rules[:5] if end_rules else (0, 0, "all", (), 0.0)
        if end_rules:
            self.end_counters = torch.zeros((self.B, 4), dtype=torch.int32, device=self.device)
            self.end_armed = torch.zeros((self.B,), dtype=torch.uint8, device=self.device)
            self.end_reason = torch.zeros((self.B,), dtype=torch.uint8, device=self.device)
            self._set_end_rules()
            torch.cuda.synchronize(self.device)                    # the zeros are in place whichever stream the first reset() runs on
        # scripted drivers (include/mcr.h: mcr_set_drivers): self.actions [B, N, 3] f32 is what step() is driven by when cars are scripted
        self.driver_params, self.scripted_agents = drv_rows, tuple(a for a in range(self.N) if drv_mask >> a & 1)
        self._drv_mask = drv_mask
        self.actions = self._drv_buf = None
        if drv_rows is not None:
            self._drv_buf = torch.zeros((self.B, self.N, 3), dtype=torch.float32, device=self.device)
            if drv_mask:
                self.actions = self._drv_buf
            _lib.check(self.L.mcr_set_drivers(self.h, _lib.ptr(drv_rows), ctypes.c_uint32(drv_mask), ctypes.c_void_p(self._drv_buf.data_ptr())), "mcr_set_drivers")
        self.racecraft_params, self.racecraft_agents = rc_rows, tuple(a for a in range(self.N) if rc_mask >> a & 1)
        if rc_rows is not None:
            _lib.check(self.L.mcr_set_racecraft(self.h, _lib.ptr(rc_rows), ctypes.c_uint32(rc_mask)), "mcr_set_racecraft")
        # RNG streams
        self.mt_track = np.zeros((self.B, _lib.MT_WORDS), np.uint32)
        self.mt_draw = np.zeros((self.B, _lib.MT_WORDS), np.uint32)
        for e in range(self.B):
            g = (int(seed) + int(env_offset) + e) % 2 ** 32
            self.L.mcr_mt_seed(_lib.ptr(self.mt_track[e]), ctypes.c_uint32(g))
            self.L.mcr_mt_seed(_lib.ptr(self.mt_draw[e]), ctypes.c_uint32((g + 2 ** 31) % 2 ** 32))
        self.slot_bytes = _lib.episode_bytes()
        # the staging source of the host path, [B, 96 KB] page-locked — not with a level pool, which stages from device memory
        self._blobs = torch.empty((self.B, self.slot_bytes), dtype=torch.uint8, pin_memory=True) if levels is None else None
        self._blobs_np = self._blobs.numpy() if levels is None else None
        self._refill_pin = None       # pinned bounce buffer of the refill thread (grown on demand)
        self.episode_info = np.zeros((self.B, 12), np.int32)      # T, P, retries, cw, car_order[8] of the newest generated episode
        self._ids = np.zeros(self.B, np.int32)
        self._episodes_generated = 0
        self._copy_stream = torch.cuda.Stream(device=self.device)
        self._copy_done = torch.cuda.Event(blocking=True)
        # async_refill: True (default) — the handle's own native thread polls, generates and stages (include/mcr.h: mcr_refill_start; no
        # interpreter in the loop: 2.1 -> 1.x host cores per rank, bench.py --emulate-world); "python" — rounds 2-5's worker thread in this
        # module (kept for comparison); False — synchronously inside step() (tests that need the staging at a known point)
        self._async = bool(async_refill)
        self._native = async_refill is True or async_refill == "native"
        self._svc = False             # the native service is running
        self._q = None
        self._worker = None
        self._closed = False
        self._has_reset = False
        # level pool (module docstring): K resident episodes the device re-stages from; the host generates nothing after this
        self.level = self.level_info = self._pool = self._pool_np = None
        self.level_cdf = self._staged_level = self.finished_level = self.level_stats = None
        self.num_levels = 0
        if levels is not None:
            self._init_levels(levels, seed if level_seed is None else level_seed, level_order, seed)
            if level_stats:
                self._init_level_stats()
        _LIVE.add(self)

    def _set_end_rules(self):
        """hand the (possibly re-pointed: tests use row views) end-rule tensors to the handle"""
        mask = sum(1 << a for a in self.end_agents)
        _lib.check(self.L.mcr_set_end_rules(self.h, self.end_patience, self.end_offroad, END_OFFROAD_MODE[self.end_offroad_mode], ctypes.c_uint32(mask),
                                            ctypes.c_double(self.end_reward), ctypes.c_void_p(self.end_counters.data_ptr()),
                                            ctypes.c_void_p(self.end_armed.data_ptr()), ctypes.c_void_p(self.end_reason.data_ptr())), "mcr_set_end_rules")

    def _init_levels(self, levels, level_seed, level_order, seed):
        if isinstance(levels, np.ndarray):
            blobs = np.array(levels, dtype=np.uint8, order="C", copy=True)      # (the handle's own copy: the caller may reuse the array)
        else:
            from .levels import make_levels
            blobs, self.level_info = make_levels(int(levels), self.N, int(level_seed), self.direction_mode, threads=self.gen_threads)
        self.num_levels = int(blobs.shape[0])
        self.level_order = level_order
        self._pool_np = blobs                                  # host copy: current_episode()
        self._pool = torch.from_numpy(blobs).to(self.device)   # resident for the life of the handle
        # [B] + one spare row that load_states points ids out of range at
        self._level_buf = torch.full((self.B + 1,), -1, dtype=torch.int32, device=self.device)
        self.level = self._level_buf[:self.B]
        _lib.check(self.L.mcr_set_episode_pool(self.h, ctypes.c_void_p(self._pool.data_ptr()), self.num_levels, ctypes.c_uint64(int(seed) % 2 ** 64),
                                               ctypes.c_uint32(self.env_offset), _lib.LEVEL_ORDER["random" if level_order == "weighted" else level_order],
                                               ctypes.c_void_p(self.level.data_ptr())), "mcr_set_episode_pool")
        if level_order == "weighted":     # a sampler on the mode-0 pool (include/mcr.h: mcr_set_level_sampler); starts uniform
            self.level_cdf = torch.zeros((self.num_levels,), dtype=torch.float64, device=self.device)
            self._staged_level = torch.full((self.B,), -1, dtype=torch.int32, device=self.device)
            _lib.check(self.L.mcr_set_level_sampler(self.h, ctypes.c_void_p(self.level_cdf.data_ptr()), ctypes.c_void_p(self._staged_level.data_ptr())),
                       "mcr_set_level_sampler")
        torch.cuda.synchronize(self.device)                    # the upload is complete whichever stream the first reset() runs on
        self._episodes_generated = self.num_levels
        self._async = self._native = False                     # nobody polls, generates or stages: the kernel owns the staged slots

    def _init_level_stats(self):
        """per-level episode statistics (module docstring; include/mcr.h: mcr_set_level_stats)"""
        cols = _lib.check(self.L.mcr_level_stats_dim(self.N), "mcr_level_stats_dim")
        self.finished_level = torch.full((self.B,), -1, dtype=torch.int32, device=self.device)
        self.level_stats = torch.zeros((self.num_levels + 1, cols), dtype=torch.float64, device=self.device)
        _lib.check(self.L.mcr_set_level_stats(self.h, ctypes.c_void_p(self.finished_level.data_ptr()), ctypes.c_void_p(self.level_stats.data_ptr())),
                   "mcr_set_level_stats")
        torch.cuda.synchronize(self.device)                    # the zeros are in place whichever stream the first step() runs on

    def level_stats_now(self):
        """`self.level_stats`, float64 [K + 1, 3 + 2N] on the device (module docstring): a plain accessor — no copy, no synchronisation; the
        values are those of the last step() once that step is complete on its stream."""
        if self.level_stats is None:
            raise _lib.McrError("level_stats_now() needs level_stats=True")
        return self.level_stats

    def reset_level_stats(self):
        """Zero `self.level_stats` on the current stream (the stepping stream): steps enqueued later start from zero.  No synchronisation."""
        if self.level_stats is None:
            raise _lib.McrError("reset_level_stats() needs level_stats=True")
        self.level_stats.zero_()

    def set_level_weights(self, weights, check=True):
        """New level weights for `level_order="weighted"` (module docstring): a sequence, a numpy array or a float64 / float32 device tensor
        [K].  One small kernel rebuilds the CDF (`self.level_cdf`) on the current stream — the stepping stream; episodes STAGED from then on
        are drawn from it, so every env plays one more episode drawn from the old weights first.  May be called before the first reset().
        check=True validates on the host — shape, finite, >= 0, sum > 0: ValueError, nothing changed — which synchronises when `weights`
        is a device tensor.  check=False never synchronises, treats a weight that is not finite or is negative as 0, falls back to the
        uniform CDF if the sum is 0 or not finite, and returns the int32 device flag [1] "fell back to uniform"."""
        if self.level_cdf is None:
            raise _lib.McrError('set_level_weights() needs levels=... with level_order="weighted"')
        K = self.num_levels
        if torch.is_tensor(weights):
            if weights.dtype not in (torch.float64, torch.float32) or weights.dim() != 1 or weights.shape[0] != K:
                raise ValueError(f"level weights must be a float64 / float32 tensor [{K}], got {weights.dtype} {list(weights.shape)}")
            if check:
                from .levels import check_weights
                check_weights(weights.detach().to(torch.float64).cpu().numpy(), K)
            w = weights.detach().to(device=self.device, dtype=torch.float64).contiguous()
        else:
            from .levels import check_weights
            if check:
                host = check_weights(weights, K)
            else:
                host = np.ascontiguousarray(weights, dtype=np.float64)
                if host.ndim != 1 or len(host) != K:
                    raise ValueError(f"level weights must have shape [{K}], got {list(host.shape)}")
            w = torch.from_numpy(host).to(self.device)
        fell_back = torch.zeros(1, dtype=torch.int32, device=self.device)
        st = torch.cuda.current_stream(self.device)
        _lib.check(self.L.mcr_level_weights(self.h, ctypes.c_void_p(w.data_ptr()), ctypes.c_void_p(fell_back.data_ptr()),
                                            ctypes.c_void_p(st.cuda_stream)), "mcr_level_weights")
        w.record_stream(st)
        return fell_back

    # ------------------------------------------------------------------ episode generation / staging
    def _generate(self, ids):
        """Generate each listed env's next episode (advances its RNG streams).  Returns the pinned, contiguous array
        [len(ids), slot_bytes] holding the blobs in the order of `ids` — what `_stage` uploads; it stays valid until the
        next `_generate` call of the same thread."""
        ids = np.ascontiguousarray(ids, np.int32)
        n = len(ids)
        if n == 0:
            return None
        mt_t = np.ascontiguousarray(self.mt_track[ids]); mt_d = np.ascontiguousarray(self.mt_draw[ids])
        if n != self.B:               # subset: generate into a contiguous pinned buffer so that staging is ONE call
            if self._refill_pin is None or self._refill_pin.shape[0] < n:
                self._refill_pin = torch.empty((max(n, 64), self.slot_bytes), dtype=torch.uint8, pin_memory=True)
            blobs = self._refill_pin.numpy()[:n]
        else:
            blobs = self._blobs_np
        info = np.zeros((n, 12), np.int32)
        _lib.check(self.L.mcr_episodes_generate(_lib.ptr(mt_t), _lib.ptr(mt_d), n, self.N, self.direction_mode,
                                                _lib.ptr(blobs), _lib.ptr(info), min(self.gen_threads, n)), "mcr_episodes_generate")
        self.mt_track[ids] = mt_t; self.mt_draw[ids] = mt_d
        self.episode_info[ids] = info
        if n != self.B:
            self._blobs_np[ids] = blobs              # per-env copy for introspection (current_episode / facade env.track)
        self._episodes_generated += n
        return blobs

    def _stage(self, ids, rows, stream):
        """Upload `rows` (from `_generate(ids)`) into the staged device slots of envs `ids` (async on `stream`)."""
        ids = np.ascontiguousarray(ids, np.int32)
        if len(ids) == 0:
            return
        _lib.check(self.L.mcr_stage_episodes(self.h, _lib.ptr(ids), len(ids), _lib.ptr(rows), ctypes.c_void_p(stream.cuda_stream)), "mcr_stage_episodes")

    def _refill(self, ids):
        rows = self._generate(ids)
        self._stage(ids, rows, self._copy_stream)
        # the bounce buffer may be overwritten as soon as the copies are done.  Polled with a sleep in between: hipStreamSynchronize
        # spins, and so does hipEventSynchronize on a "blocking" event (measured: 0.8 of a core in bench.py's look-ahead fence); a
        # thread that spins takes a core from the track generator — with the ranks of a node sharing few cores
        # (bench.py --emulate-world) that is what the host side runs out of first
        self._copy_done.record(self._copy_stream)
        while not self._copy_done.query():          # (not .synchronize(): see above — it spins on this runtime, blocking event or not)
            time.sleep(5e-5)

    def _worker_main(self):
        try:                                                   # name the thread for top / bench.py's per-thread CPU report (PR_SET_NAME)
            ctypes.CDLL(None).prctl(15, b"mcr-refill", 0, 0, 0)
        except Exception:
            pass
        torch.cuda.set_device(self.device)
        while True:
            ids = self._q.get()
            if ids is None:
                self._q.task_done()
                return
            batch, taken, stop = [ids], 1, False
            while True:               # drain: everything queued meanwhile goes into the same generate + stage batch
                try:
                    more = self._q.get_nowait()
                except queue.Empty:
                    break
                taken += 1
                if more is None:
                    stop = True
                    break
                batch.append(more)
            try:
                if self._worker_exc is None:
                    self._refill(np.concatenate(batch))
            except BaseException as exc:   # surfaced by wait_refills()/step(); the queue must still drain or join() hangs
                self._worker_exc = exc
            finally:
                with self._pending_lock:
                    for _ in range(len(batch)):
                        if self._pending:
                            self._pending.popleft()
                for _ in range(taken):
                    self._q.task_done()
            if stop:
                return

    def _raise_worker_error(self):
        if self._worker_exc is not None:
            exc, self._worker_exc = self._worker_exc, None
            raise _lib.McrError(f"episode refill thread failed: {exc!r}") from exc

    @property
    def episodes_generated(self):
        return self._episodes_generated + (int(self.L.mcr_refill_generated(self.h)) if self._svc else 0)

    @property
    def hold_refills(self):
        return self._hold_refills

    @hold_refills.setter
    def hold_refills(self, v):
        self._hold_refills = bool(v)
        if self._svc:
            _lib.check(self.L.mcr_refill_hold(self.h, int(self._hold_refills)), "mcr_refill_hold")

    def _poll_and_refill(self):
        if self._pool is not None:    # level pool: the device re-staged the env behind the step that consumed its episode
            return 0
        if self._native:
            if not self._svc:         # (started after the first reset()'s own staging: from here on the RNG states and the blob rows are the service's)
                _lib.check(self.L.mcr_refill_start(self.h, _lib.ptr(self.mt_track), _lib.ptr(self.mt_draw), self.direction_mode, self.gen_threads,
                                                   ctypes.c_void_p(self._blobs.data_ptr()), _lib.ptr(self.episode_info)), "mcr_refill_start")
                self._svc = True
                if self._hold_refills:
                    _lib.check(self.L.mcr_refill_hold(self.h, 1), "mcr_refill_hold")
            return 0
        if self.hold_refills:
            return 0
        n = self.L.mcr_poll_consumed(self.h, _lib.ptr(self._ids), self.B, None)
        if n <= 0:
            return 0
        ids = self._ids[:n].copy()
        if self._async:
            if self._worker is None:
                self._q = queue.Queue()
                self._worker = threading.Thread(target=self._worker_main, daemon=True)
                self._worker.start()
            with self._pending_lock:
                self._pending.append(self._step_idx)
            self._q.put(ids)
        else:
            self._refill(ids)
        return n

    def wait_refills(self):
        if self._svc:
            _lib.check(self.L.mcr_refill_wait(self.h), "mcr_refill_wait")
            return
        if self._q is not None:
            self._q.join()
        self._raise_worker_error()

    def _settle_staging(self, st):
        """Every env that consumed its staged episode gets the next one staged NOW (stream drained, consumption polled,
        refills finished): afterwards k_install finds `staged_ready` set for every env it is asked to reset."""
        if self._pool is not None:    # level pool: every env was re-staged behind the reset / step that consumed its episode
            return
        st.synchronize()
        self._poll_and_refill()
        self.wait_refills()

    # ------------------------------------------------------------------ API
    def reset(self):
        """Reset every env; returns obs [B, *obs_shape] uint8 (device tensor, overwritten by later steps)."""
        st = torch.cuda.current_stream(self.device)
        self.wait_refills()
        if self._pool is not None:
            pass                      # level pool: mcr_reset stages every env from the pool itself
        elif not self._has_reset:
            every = np.arange(self.B, dtype=np.int32)
            self._stage(every, self._generate(every), st)
        else:
            # envs re-spawned by steps whose consumption has not been polled yet would find their staged slot empty
            # (k_install skips those): drain, poll and refill first, then every env installs a fresh episode
            self._settle_staging(st)
        _lib.check(self.L.mcr_reset(self.h, None, self._obs_ptr(), ctypes.c_void_p(st.cuda_stream)), "mcr_reset")
        if self.end_reason is not None:
            self.end_reason.zero_()   # (no step has ended anything yet; the counters and armed bytes are mcr_reset's settle pass)
        st.synchronize()
        self._has_reset = True
        self._poll_and_refill()
        return self.obs

    def reset_envs(self, mask):
        """Reset the envs whose byte in `mask` (uint8 device tensor [B]) is non-zero: each installs its staged
        episode (reference reset(), :340-408) and gets its first observation written into `self.obs`."""
        if not self._has_reset:
            raise AttributeError("reset_envs() before reset()")
        st = torch.cuda.current_stream(self.device)
        if mask.dtype != torch.uint8 or mask.device != self.device or mask.numel() != self.B or not mask.is_contiguous():
            mask = mask.to(device=self.device, dtype=torch.uint8).contiguous()
            if mask.numel() != self.B:
                raise ValueError(f"mask must have {self.B} elements")
        self._settle_staging(st)              # a masked env must find its staged slot filled
        _lib.check(self.L.mcr_reset(self.h, ctypes.c_void_p(mask.data_ptr()), self._obs_ptr(), ctypes.c_void_p(st.cuda_stream)), "mcr_reset")
        st.synchronize()
        self._poll_and_refill()
        return self.obs

    def step(self, actions):
        """actions: float32 device tensor [B,N,3] (steer, gas, brake) or None. Returns (obs, reward, done, info).
        With frame_skip=k > 1 one call is a macro-step of up to k env steps per env (module docstring); actions must not be None then.
        With scripted_agents the rows of the scripted cars are replaced by the controller's (info["actions"] = self.actions is what the step
        applied; `actions` itself is not written); step(None) is the action-less step for every car, scripted or not."""
        if actions is None and self.frame_skip > 1:
            raise ValueError("step(None) needs frame_skip=1: the action-less step belongs to reset()")
        st = torch.cuda.current_stream(self.device)
        self._raise_worker_error()
        if self._pool is not None:
            behind = False            # level pool: no host refills to fall behind
        elif self._svc:
            lag = int(self.L.mcr_refill_lag(self.h))
            if lag < 0:
                _lib.check(lag, "mcr_refill_lag")
            # (the service notices a consumption up to a few steps after it happened; the lag counts env steps, and this call adds frame_skip of them)
            behind = lag + self.frame_skip - 1 >= max(1, self.refill_lag - 4)
        else:
            with self._pending_lock:          # (the refill worker pops entries under the same lock)
                behind = bool(self._pending) and self._step_idx + self.frame_skip - 1 - self._pending[0] >= self.refill_lag
        if behind:
            t0 = time.perf_counter()
            self.wait_refills()               # the host fell behind: block instead of letting an env freeze
            self.blocked_s += time.perf_counter() - t0
        if st.cuda_stream not in self._bound_streams:      # first step on this stream: may it use the phase-word ordering? (synchronises, once)
            _lib.check(self.L.mcr_bind_stream(self.h, ctypes.c_void_p(st.cuda_stream)), "mcr_bind_stream")
            self._bound_streams.add(st.cuda_stream)
        a_ptr = None
        if actions is not None:
            if actions.dtype != torch.float32 or not actions.is_contiguous() or actions.device != self.device:
                actions = actions.to(device=self.device, dtype=torch.float32).contiguous()
            if actions.numel() != self.B * self.N * 3:
                raise ValueError(f"actions must have {self.B * self.N * 3} elements, got {actions.numel()}")
            a_ptr = ctypes.c_void_p(actions.data_ptr())
            if self._drv_mask:        # one kernel in front of the step: the scripted cars' rows from the current state, the others copied
                _lib.check(self.L.mcr_driver_actions(self.h, a_ptr, ctypes.c_uint32(0), None, ctypes.c_void_p(st.cuda_stream)), "mcr_driver_actions")
                a_ptr = ctypes.c_void_p(self.actions.data_ptr())
        _lib.check(self.L.mcr_step_repeat(self.h, a_ptr, self.frame_skip, self._obs_ptr(),
                                          ctypes.c_void_p(self.reward.data_ptr()), ctypes.c_void_p(self.done.data_ptr()),
                                          ctypes.c_void_p(self.truncated.data_ptr()), ctypes.c_void_p(st.cuda_stream)), "mcr_step_repeat")
        if actions is None and self.end_reason is not None:
            self.end_reason.zero_()   # the action-less step ends nothing (and no k_endrules pass runs behind it: the word would be the last step's)
        self._step_idx += self.frame_skip     # env steps (only a step that was launched counts: a reported McrError leaves the accounting alone)
        if self._ring is not None:
            self.obs = self._window()
        self._warn_degraded()
        if self.auto_reset:
            self._poll_and_refill()
        info = {"TimeLimit.truncated": self.truncated, "episode_return": self.episode_return, "episode_length": self.episode_length}
        if self.terminal_obs is not None:     # (device tensors, like everything else here: entry i < terminal_count is env terminal_env_ids[i])
            info["terminal_observation"] = self.terminal_obs
            info["terminal_env_ids"] = self.terminal_env_ids
            info["terminal_count"] = self.terminal_count
        if self.state is not None:
            info["state"] = self.state
        if self.ranges is not None:
            info["ranges"] = self.ranges
        if self.grid is not None:
            info["grid"] = self.grid
        if self.contact_mask is not None:
            info["contact_mask"] = self.contact_mask
            info["contact_impulse"] = self.contact_impulse
        if self.end_reason is not None:
            info["end_reason"] = self.end_reason
        if self.level is not None:
            info["level"] = self.level
        if self.level_stats is not None:
            info["finished_level"] = self.finished_level
        if self._drv_mask and actions is not None:
            info["actions"] = self.actions
        return self.obs, self.reward, self.done, info

    def expert_actions(self, out=None):
        """The controller's action for EVERY car from the CURRENT state (include/mcr.h: mcr_driver_actions), float32 [B, N, 3] on the current
        stream — a new tensor, or `out`.  Does not step, does not synchronise, and leaves `self.actions` alone.  Rows of envs that are not
        active (before reset(), frozen) are zeros.  Needs scripted_agents or driver_params (McrError otherwise)."""
        if self._drv_buf is None:
            raise _lib.McrError("created without scripted_agents / driver_params")
        shape = (self.B, self.N, 3)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        elif (not torch.is_tensor(out) or out.dtype != torch.float32 or out.device != self.device or tuple(out.shape) != shape or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous float32 tensor {list(shape)} on {self.device}")
        st = torch.cuda.current_stream(self.device)
        _lib.check(self.L.mcr_driver_actions(self.h, None, ctypes.c_uint32(0xffffffff), ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(st.cuda_stream)), "mcr_driver_actions")
        return out

    def refresh_state(self):
        """Recompute `self.state` from the CURRENT state on the current stream (include/mcr.h: mcr_state_obs_now) — after set_bodies() /
        set_state_blob(), which do not; reset() and step() keep it current by themselves.  Returns the tensor; does not synchronise."""
        if self.state is None:
            raise _lib.McrError("created without state_obs=True")
        st = torch.cuda.current_stream(self.device)
        _lib.check(self.L.mcr_state_obs_now(self.h, ctypes.c_void_p(st.cuda_stream)), "mcr_state_obs_now")
        return self.state

    def refresh_grid(self):
        """Recompute `self.grid` from the CURRENT state on the current stream (include/mcr.h: mcr_grid_obs_now) — after set_bodies() /
        set_env_state() / set_state_blob(), which leave it alone.  Returns the tensor."""
        if self.grid is None:
            raise _lib.McrError("created without grid_obs=True")
        st = torch.cuda.current_stream(self.device)
        _lib.check(self.L.mcr_grid_obs_now(self.h, ctypes.c_void_p(st.cuda_stream)), "mcr_grid_obs_now")
        return self.grid

    def grid_planes(self, dtype=torch.float32):
        """`self.grid` as four planes of 0 / 1 — GRID_ROAD, GRID_FRESH, GRID_TAKEN, GRID_CAR — [B, N, 4, H, W] of `dtype`: a torch expression on
        the current stream, a new tensor every call."""
        if self.grid is None:
            raise _lib.McrError("created without grid_obs=True")
        shifts = torch.arange(4, dtype=torch.uint8, device=self.grid.device).view(1, 1, 4, 1, 1)
        return ((self.grid.unsqueeze(2) >> shifts) & 1).to(dtype)

    def refresh_ranges(self):
        """Recompute `self.ranges` from the CURRENT state on the current stream (include/mcr.h: mcr_range_obs_now) — after set_bodies() /
        set_state_blob(), which do not; reset() and step() keep it current by themselves.  Returns the tensor; does not synchronise."""
        if self.ranges is None:
            raise _lib.McrError("created without range_obs=True")
        st = torch.cuda.current_stream(self.device)
        _lib.check(self.L.mcr_range_obs_now(self.h, ctypes.c_void_p(st.cuda_stream)), "mcr_range_obs_now")
        return self.ranges

    def refresh_contacts(self):
        """Recompute `self.contact_mask` and `self.contact_impulse`, without accumulation, from the envs' manifold stores as they stand, on the
        current stream (include/mcr.h: mcr_contact_obs_now); reset(), step() and the snapshot calls keep them current by themselves.  Returns
        the two tensors; does not synchronise."""
        if self.contact_mask is None:
            raise _lib.McrError("created without contact_obs=True")
        st = torch.cuda.current_stream(self.device)
        _lib.check(self.L.mcr_contact_obs_now(self.h, ctypes.c_void_p(st.cuda_stream)), "mcr_contact_obs_now")
        return self.contact_mask, self.contact_impulse

    def refresh_end_rules(self):
        """Settle the end rules on the current stream (include/mcr.h: mcr_end_rules_now) after writing `self.end_counters` yourself — a restore
        beside load_states() — or after set_state_blob() / set_env_state(): rows of envs in the first state of an episode start over, every other
        row keeps its counters and has its armed byte recomputed from them.  reset(), reset_envs(), load_states() and clone_envs() do this by
        themselves.  Returns (end_counters, end_reason); does not synchronise."""
        if self.end_counters is None:
            raise _lib.McrError("created without end_patience / end_offroad")
        st = torch.cuda.current_stream(self.device)
        _lib.check(self.L.mcr_end_rules_now(self.h, ctypes.c_void_p(st.cuda_stream)), "mcr_end_rules_now")
        return self.end_counters, self.end_reason

    def refresh_flags(self):
        """Run the backward / on-grass scans on the CURRENT state on the current stream (include/mcr.h: mcr_flags_now) — after set_bodies() /
        set_state_blob(), which do not; step() keeps the flags current by itself.  get_env_state() shows the result; does not synchronise."""
        st = torch.cuda.current_stream(self.device)
        _lib.check(self.L.mcr_flags_now(self.h, ctypes.c_void_p(st.cuda_stream)), "mcr_flags_now")

    def refresh_obs(self, out=None):
        """Draw every env's observation from the CURRENT state on the current stream (include/mcr.h: mcr_obs_now) — after set_bodies() /
        set_wheels() / set_env_state() / set_state_blob(), which draw nothing; reset() and step() draw by themselves.  The score label shows
        the current reward, the backwards flag the current driving_backward.  Writes into `out` (a contiguous uint8 tensor of `self.obs`'s
        shape on the device) or, by default, into `self.obs`; returns that tensor; does not synchronise.  Not with frame_stack > 1."""
        if not self.obs_enabled:
            raise _lib.McrError("created with obs=False")
        if self._ring is not None:
            raise _lib.McrError("refresh_obs() with a stacked observation format: the ring's slots belong to step()")
        if out is None:
            out = self.obs
        elif (not torch.is_tensor(out) or out.dtype != torch.uint8 or out.device != self.device or tuple(out.shape) != tuple(self.obs.shape)
              or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous uint8 tensor {list(self.obs.shape)} on {self.device}")
        st = torch.cuda.current_stream(self.device)
        _lib.check(self.L.mcr_obs_now(self.h, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(st.cuda_stream)), "mcr_obs_now")
        return out

    def _obs_ptr(self):
        """the observation buffer the raster writes: the frames, or the ring of a stacked format"""
        if not self.obs_enabled:
            return None
        return ctypes.c_void_p((self._ring if self._ring is not None else self.obs).data_ptr())

    def _window(self):
        """stacked gray: the ring's slots j + 1 .. j + k of the last enqueued drawing step (include/mcr.h: mcr_obs_window), a view"""
        w = int(self.L.mcr_obs_window(self.h))
        return self._ring[:, :, w:w + self.frame_stack]

    def terminal_observations(self):
        """(env ids [k], frames [k, *obs_shape]) of the episodes that ended in the last step — what the reference returns as its observation
        with done = True (multi_car_racing.py:431, :509) — as device tensors; synchronises (reads the count)."""
        if self.terminal_obs is None:
            raise _lib.McrError("created without terminal_obs=True")
        k = int(self.terminal_count.item())
        return self.terminal_env_ids[:k], self.terminal_obs[:k]

    _DEGRADED = {2: "more touching car<->car fixture pairs in an env than the manifold store holds (MCR_CC_MAX): the excess contacts were dropped — that env's "
                    "physics deviates from the reference from here on",
                 3: "more tile begin events in one env-step than the replay buffer holds: the excess events (tile visits, rewards) were dropped",
                 4: "an env ended its episode before the host had staged its next one and froze (zero reward, done = 0, stale frame) until the episode "
                    "arrived: the track generator is behind the device (more gen_threads, async_refill=True, a longer TimeLimit, or fence the stepping loop)"}

    def _warn_degraded(self):
        """The capacity / starvation conditions the kernels count without failing (include/mcr.h: mcr_status words 2..4): say so, once per change.
        Reads mapped host memory — no synchronisation; a condition raised by a step still in flight surfaces a call later."""
        _lib.check(self.L.mcr_status(self.h, _lib.ptr(self._status_now), 8), "mcr_status")
        for w, what in self._DEGRADED.items():
            if self._status_now[w] != self._status_seen[w]:
                import warnings
                warnings.warn(f"{what} ({int(self._status_now[w])} so far)", _lib.McrWarning, stacklevel=3)
                self._status_seen[w] = self._status_now[w]

    def debug_counters(self):
        """cumulative [envs deferred, envs resumed, contact envs routed to the side stream, env-steps spent frozen
        waiting for a staged episode] (synchronises)"""
        out = np.zeros(4, np.uint64)
        _lib.check(self.L.mcr_debug_read_counters(self.h, _lib.ptr(out)), "mcr_debug_read_counters")
        return out


    def verdict_mismatches(self):
        """envs in which the contact pass disagreed with the touch verdict the main launches went by (must be 0; synchronises)"""
        out = np.zeros(1, np.uint64)
        _lib.check(self.L.mcr_debug_read_verdict_mismatches(self.h, _lib.ptr(out)), "mcr_debug_read_verdict_mismatches")
        return int(out[0])

    def status_words(self):
        """cumulative status words of include/mcr.h `mcr_status`: [0] in-kernel waits given up, [1] touch-verdict mismatches,
        [2] car<->car manifold overflows, [3] begin-event queue overflows, [4] envs that froze waiting for a staged episode (all 0 in a healthy
        rollout; does not synchronise)"""
        out = np.zeros(8, np.uint32)
        _lib.check(self.L.mcr_status(self.h, _lib.ptr(out), 8), "mcr_status")
        return out

    def rollout_stats(self, reset=False):
        """(episodes finished, sum of their returns over all agents) accumulated on the device; synchronises."""
        out = np.zeros(2)
        _lib.check(self.L.mcr_read_rollout_stats(self.h, _lib.ptr(out), int(bool(reset))), "mcr_read_rollout_stats")
        return float(out[0]), float(out[1])

    def render_rgb(self, e=0, width=600, height=400):
        """render('rgb_array') of env e: uint8 device tensor [N, height, width, 3] of its CURRENT state (reference
        :511-604 with the VIDEO_W x VIDEO_H viewport), score label included; skid particles (Car.draw(viewer, True), :564) are
        drawn when the env was created with skid_particles=True (the facade does; batched envs leave them off)."""
        if not self._has_reset:
            raise AttributeError("render before reset()")
        out = torch.empty((self.N, int(height), int(width), 3), dtype=torch.uint8, device=self.device)
        st = torch.cuda.current_stream(self.device)
        _lib.check(self.L.mcr_render(self.h, int(e), int(width), int(height), ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(st.cuda_stream)), "mcr_render")
        return out

    # ------------------------------------------------------------------ introspection (synchronous; tests / debugging)
    def get_state(self):
        B, N = self.B, self.N
        bodies = np.zeros((B, N, 5, 6), np.float32); joints = np.zeros((B, N, 4, 4), np.float32)
        wheels = np.zeros((B, N, 4, 5), np.float64); limit = np.zeros((B, N, 4), np.int32)
        on_road = np.zeros((B, N, 4), np.uint8); sleep = np.zeros((B, N, 5), np.float32)
        _lib.check(self.L.mcr_get_state(self.h, _lib.ptr(bodies), _lib.ptr(joints), _lib.ptr(wheels), _lib.ptr(limit),
                                        _lib.ptr(on_road), _lib.ptr(sleep)), "mcr_get_state")
        return dict(bodies=bodies, joints=joints, wheels=wheels, limit=limit, on_road=on_road, sleep=sleep)

    def set_bodies(self, bodies):
        b = np.ascontiguousarray(bodies, np.float32)
        assert b.shape == (self.B, self.N, 5, 6)
        _lib.check(self.L.mcr_set_bodies(self.h, _lib.ptr(b)), "mcr_set_bodies")

    def set_wheels(self, wheels):
        """get_state()["wheels"] back: phase and omega (columns 3, 4) of every wheel; the controls (columns 0..2) are ignored.  Synchronous."""
        w = np.ascontiguousarray(wheels, np.float64)
        assert w.shape == (self.B, self.N, 4, 5)
        _lib.check(self.L.mcr_set_wheels(self.h, _lib.ptr(w)), "mcr_set_wheels")

    def set_env_state(self, reward=None, t=None, tile_flags=None):
        """get_env_state()'s reward [B, N] f64, t [B] f64 and tile_flags [B, TILE_CAP] u16 back (None: left alone) — those fields only.  Synchronous."""
        r = None if reward is None else np.ascontiguousarray(reward, np.float64)
        tt = None if t is None else np.ascontiguousarray(t, np.float64)
        f = None if tile_flags is None else np.ascontiguousarray(tile_flags, np.uint16)
        assert (r is None or r.shape == (self.B, self.N)) and (tt is None or tt.shape == (self.B,)) and (f is None or f.shape == (self.B, _lib.TILE_CAP))
        _lib.check(self.L.mcr_set_env_state(self.h, _lib.ptr(r), _lib.ptr(tt), _lib.ptr(f)), "mcr_set_env_state")

    def get_env_state(self):
        B, N = self.B, self.N
        reward = np.zeros((B, N)); tvc = np.zeros((B, N), np.int32)
        bw = np.zeros((B, N), np.uint8); og = np.zeros((B, N), np.uint8); t = np.zeros(B)
        flags = np.zeros((B, _lib.TILE_CAP), np.uint16); nt = np.zeros(B, np.int32)
        _lib.check(self.L.mcr_get_env_state(self.h, _lib.ptr(reward), _lib.ptr(tvc), _lib.ptr(bw), _lib.ptr(og), _lib.ptr(t),
                                            _lib.ptr(flags), _lib.ptr(nt)), "mcr_get_env_state")
        return dict(reward=reward, tile_visited_count=tvc, driving_backward=bw, driving_on_grass=og, t=t,
                    tile_flags=flags, num_tiles=nt)

    def get_state_blob(self, e):
        """Full snapshot of env e (uint8 host array): everything `step` reads — see include/mcr.h mcr_get_state_blob."""
        blob = np.zeros(int(self.L.mcr_state_blob_bytes(self.h)), np.uint8)
        _lib.check(self.L.mcr_get_state_blob(self.h, int(e), _lib.ptr(blob)), "mcr_get_state_blob")
        return blob

    def set_state_blob(self, e, blob):
        """Restore a snapshot into env e (any env index, any handle with the same num_agents); stepping continues
        bit-identically from it."""
        blob = np.ascontiguousarray(blob, np.uint8)
        _lib.check(self.L.mcr_set_state_blob(self.h, int(e), _lib.ptr(blob)), "mcr_set_state_blob")
        self._has_reset = self._has_reset or True

    # ------------------------------------------------------------------ batched snapshots on the device (stream-ordered; module docstring)
    @property
    def state_blob_pitch(self):
        """bytes per row of a save_states() tensor: mcr_state_blob_bytes rounded up to 16"""
        return int(self.L.mcr_state_blob_pitch(self.h))

    def _env_ids(self, ids, what, distinct=False):
        """env ids -> (int32 device tensor or None, count, host array or None).  A sequence is validated here (range, and
        distinctness where asked: ValueError); a device tensor is taken as it is — the kernel skips ids out of range."""
        if ids is None:
            return None, self.B, None
        if torch.is_tensor(ids):
            if ids.dim() != 1:
                raise ValueError(f"{what} must be one-dimensional")
            if ids.numel() > self.B:
                raise ValueError(f"{what}: at most num_envs = {self.B} ids, got {ids.numel()}")
            return ids.to(device=self.device, dtype=torch.int32).contiguous(), int(ids.numel()), None
        host = np.asarray(list(ids), dtype=np.int64).reshape(-1)
        if len(host) > self.B:
            raise ValueError(f"{what}: at most num_envs = {self.B} ids, got {len(host)}")
        if len(host) and (host.min() < 0 or host.max() >= self.B):
            raise ValueError(f"{what} must be in 0..{self.B - 1}")
        if distinct and len(np.unique(host)) != len(host):
            raise ValueError(f"{what} must be distinct")
        return torch.from_numpy(host.astype(np.int32)).to(self.device), len(host), host

    def save_states(self, env_ids=None, out=None):
        """Snapshot envs `env_ids` (None: all; a sequence; an int32 device tensor) into a uint8 device tensor [n, state_blob_pitch]: row i
        starts with exactly the bytes of get_state_blob(env_ids[i]).  One kernel on the current stream; does not synchronise."""
        ids, n, _ = self._env_ids(env_ids, "env_ids")
        pitch = self.state_blob_pitch
        if out is None:
            out = torch.empty((n, pitch), dtype=torch.uint8, device=self.device)
        elif (not torch.is_tensor(out) or out.dtype != torch.uint8 or out.device != self.device or tuple(out.shape) != (n, pitch)
              or not out.is_contiguous() or out.data_ptr() % 16):
            raise ValueError(f"out must be a contiguous, 16-byte aligned uint8 tensor [{n}, {pitch}] on {self.device}")
        st = torch.cuda.current_stream(self.device)
        _lib.check(self.L.mcr_save_states(self.h, None if ids is None else ctypes.c_void_p(ids.data_ptr()), n, ctypes.c_void_p(out.data_ptr()),
                                          ctypes.c_void_p(st.cuda_stream)), "mcr_save_states")
        return out

    def load_states(self, blobs, env_ids=None, check=True):
        """Restore rows of a save_states() tensor into envs `env_ids` (None: row i into env i) of this handle — any handle with the same
        num_agents, skid_particles and fresh_world; stepping continues bit-identically (set_state_blob's rule: an env restored on an
        auto_reset handle continues with THIS handle's next staged episode when its episode ends).  `self.state` is rewritten; the
        observation buffers are not redrawn (the next step draws them).  check=True validates on the host first — shape, ids given as a
        sequence, the header words of every row: ValueError, nothing changed — which synchronises, and raises McrError if the kernel
        refused a row.  check=False never synchronises and returns the int32 device counter [1] of refused rows (rows whose header is not
        this handle's, ids out of range: those envs stay untouched).
        End rules (end_patience / end_offroad): the blob does not hold `self.end_counters` — they are the caller's.  Save the rows with the
        states and write them back IN FRONT of this call, whose settle pass recomputes the armed bytes from them (or afterwards, followed by
        refresh_end_rules()): the continuation is then bit-identical.  Left alone, a restored env goes on from whatever its row held."""
        if self.frame_stack > 1:
            raise ValueError("load_states with frame_stack > 1: a restored env has no frame history to fill its stack with")
        pitch = self.state_blob_pitch
        if not torch.is_tensor(blobs) or blobs.dtype != torch.uint8 or blobs.dim() != 2 or blobs.shape[1] != pitch:
            raise ValueError(f"blobs must be a uint8 tensor [n, {pitch}] (save_states)")
        ids, n, _ = self._env_ids(env_ids, "env_ids", distinct=check)
        if env_ids is None:
            n = int(blobs.shape[0])
            if n > self.B:
                raise ValueError(f"blobs has {n} rows, the handle {self.B} envs")
        elif blobs.shape[0] != n:
            raise ValueError(f"blobs has {blobs.shape[0]} rows for {n} env ids")
        if blobs.device != self.device or not blobs.is_contiguous() or blobs.data_ptr() % 16:
            blobs = blobs.to(self.device).contiguous().clone()
        if check and n:
            want = np.zeros(4, np.uint32)
            _lib.check(self.L.mcr_state_blob_header(self.h, _lib.ptr(want)), "mcr_state_blob_header")
            got = blobs[:, :16].cpu().numpy().view(np.uint32)
            bad = np.nonzero((got != want[None]).any(1))[0]
            if len(bad):
                raise ValueError(f"rows {bad[:8].tolist()} are not state blobs of this handle (header {got[bad[0]].tolist()}, expected {want.tolist()}: "
                                 "magic, num_agents, skid_particles | one-world tables << 1, bytes)")
        refused = torch.zeros(1, dtype=torch.int32, device=self.device)
        st = torch.cuda.current_stream(self.device)
        _lib.check(self.L.mcr_load_states(self.h, None if ids is None else ctypes.c_void_p(ids.data_ptr()), n, ctypes.c_void_p(blobs.data_ptr()),
                                          ctypes.c_void_p(refused.data_ptr()), ctypes.c_void_p(st.cuda_stream)), "mcr_load_states")
        self._has_reset = True
        if self.level is not None:            # the blob does not say which level it came from (rows the kernel refuses — check=False — read -1 too)
            if ids is None:
                self.level[:n] = -1
            else:                             # (no synchronisation: an id out of range, which the kernel skips, lands on the spare row)
                i64 = ids.long()
                self._level_buf.index_fill_(0, torch.where((i64 >= 0) & (i64 < self.B), i64, torch.full_like(i64, self.B)), -1)
        if not check:
            return refused
        k = int(refused.item())
        if k:
            raise _lib.McrError(f"load_states: the kernel refused {k} rows (their envs are untouched)")
        return refused

    def clone_envs(self, src_ids, dst_ids, check=True):
        """Env dst_ids[i] becomes a copy of env src_ids[i] (a source may be listed many times): the state by one kernel (mcr_copy_states),
        then the rows of obs (the ring of a stacked format), reward, done and truncated, so that the clone is observationally equal at once;
        `self.state`, `self.ranges` and `self.grid` are rewritten, with a level pool the `level` rows are copied, and with end rules the `end_counters` / `end_reason` rows (the clone arms when its source does).  Destinations must be distinct and disjoint from the sources — validated (ValueError) with check=True when
        the ids are sequences, the caller's obligation otherwise.  On the current stream; does not synchronise."""
        src, n, src_h = self._env_ids(src_ids, "src_ids")
        dst, m, dst_h = self._env_ids(dst_ids, "dst_ids", distinct=check)
        if src is None or dst is None:
            raise ValueError("clone_envs needs src_ids and dst_ids")
        if n != m:
            raise ValueError(f"{n} src_ids for {m} dst_ids")
        if check and src_h is not None and dst_h is not None and len(np.intersect1d(src_h, dst_h)):
            raise ValueError("dst_ids must be disjoint from src_ids")
        st = torch.cuda.current_stream(self.device)
        s64, d64 = src.long(), dst.long()
        if self.end_counters is not None and n:      # in front of mcr_copy_states, whose settle pass makes the clones' armed bytes from the copied rows
            for t in (self.end_counters, self.end_reason):
                t.index_copy_(0, d64, t.index_select(0, s64))
        _lib.check(self.L.mcr_copy_states(self.h, ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()), n,
                                          ctypes.c_void_p(st.cuda_stream)), "mcr_copy_states")
        frames = self._ring if self._ring is not None else self.obs
        for t in (frames, self.reward, self.done, self.truncated, self.level):
            if t is not None and n:
                t.index_copy_(0, d64, t.index_select(0, s64))

    def synth_actions(self, t, seed=0, out=None, steps=None):
        """Counter-based synthetic actions (bench/tests): a pure function of (seed, global env index, agent, t).  Step t as a
        device tensor [B,N,3] f32, or — with `steps` — the steps t .. t+steps-1 in one launch as [steps,B,N,3]."""
        n = 1 if steps is None else int(steps)
        if out is None:
            out = torch.empty(((self.B, self.N, 3) if steps is None else (n, self.B, self.N, 3)), dtype=torch.float32, device=self.device)
        st = torch.cuda.current_stream(self.device)
        _lib.check(self.L.mcr_synth_actions_block(self.h, ctypes.c_void_p(out.data_ptr()), ctypes.c_uint64(int(seed)), ctypes.c_uint32(int(t) & 0xffffffff),
                                                  n, ctypes.c_uint32(self.env_offset), ctypes.c_void_p(st.cuda_stream)), "mcr_synth_actions_block")
        return out

    def positions(self):
        pos = np.zeros((self.B, self.N, 2), np.float32)
        _lib.check(self.L.mcr_get_positions(self.h, _lib.ptr(pos)), "mcr_get_positions")
        return pos

    def current_episode(self, e):
        """Host copy of the NEWEST generated episode of env e (the staged one once the env has reset).  With a level pool: of the level env e
        is playing NOW, pool row `self.level[e]` (synchronises)."""
        if self._pool is not None:
            lv = int(self.level[int(e)].item())
            if lv < 0:
                raise _lib.McrError(f"env {e} has no known level (before reset(), or restored by load_states)")
            return _lib.unpack_episode(np.ascontiguousarray(self._pool_np[lv]))
        return _lib.unpack_episode(np.ascontiguousarray(self._blobs_np[e]))

    def timing(self, mask):
        """HIP-event kernel timing; mask bit 0 collide, 1 dynamics, 2 view, 3/4 reset-pass collide/dynamics,
        5/6 dynamics/view of the contact side stream, 7 its reset pass."""
        _lib.check(self.L.mcr_timing_enable(self.h, int(mask)))

    def timing_read(self):
        ms = np.zeros(8); n = np.zeros(8, np.int64)
        _lib.check(self.L.mcr_timing_read(self.h, _lib.ptr(ms), _lib.ptr(n)))
        return ms, n

    def close(self):
        if self._closed:
            return
        self._closed = True
        if self._worker is not None:
            self._q.put(None)
            self._worker.join()
        if self._svc and self.h:
            self.L.mcr_refill_stop(self.h)
            self._svc = False
        if self.h:
            self.L.mcr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
