/* include/mcr.h — C ABI of the MI355X-native MultiCarRacing-v0 batched step.
 *
 * The reference has no FFI of its own for this path: its native boundary is SWIG'd Box2D
 * (`Box2D.b2World.Step`, multi_car_racing.py:428) plus ctypes OpenGL (`gl.glVertex3f`, :613-674).
 * This header is the boundary a maintainer would bind instead (INTEGRATION.md shows the ctypes stub);
 * each entry point names the reference interface it replaces.
 *
 * Conventions: plain pointers and sizes only, `int` status returns (0 = MCR_OK, <0 = error enum),
 * nothing throws across the boundary, no exit().  `d_*` pointers are DEVICE pointers on the handle's
 * HIP device; `stream` is a `hipStream_t` passed as `void*` (NULL = the null stream).  Kernels are only
 * enqueued — no hidden device synchronisation in mcr_step / mcr_reset (the one check that needs one is mcr_bind_stream).
 * One handle = one device = one env slice; handles are independent (thread-compatible).
 */
#ifndef MCR_H
#define MCR_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MCR_OK 0
#define MCR_ERR_ARG (-1)      /* bad argument (NULL, range) */
#define MCR_ERR_HIP (-2)      /* a HIP runtime call failed; see mcr_last_error() */
#define MCR_ERR_STATE (-3)    /* call order violated (e.g. step before reset: AttributeError in the reference) */
#define MCR_ERR_CAPACITY (-4) /* track larger than MCR_TILE_CAP / MCR_QUAD_CAP */

#define MCR_MAX_AGENTS 8      /* CAR_COLORS has 8 entries (multi_car_racing.py:67-70) */
#define MCR_TILE_CAP 512      /* tiles per track: observed 239..379 */
#define MCR_QUAD_CAP 768      /* road_poly entries: observed 279..460 */
#define MCR_OBS_H 96
#define MCR_OBS_W 96
#define MCR_MT_WORDS 625      /* MT19937 key[624] + pos — numpy RandomState layout */
#define MCR_OBS_RGB 0         /* mcr_set_obs_format: 96x96x3 RGB frames (default) */
#define MCR_OBS_GRAY 1        /* ... 96x96 luma frames, optionally stacked */
#define MCR_OBS_STACK_MAX 8

typedef struct mcr_env mcr_env; /* opaque */

/* ctor kwargs of MultiCarRacing.__init__ (multi_car_racing.py:131-133) + batch/device knobs */
typedef struct mcr_config {
  int32_t num_envs;          /* B: environments in this slice */
  int32_t num_agents;        /* N: 1..8 */
  int32_t device;            /* HIP device ordinal */
  int32_t obs_enabled;       /* 0: physics only ("obs=none"); 1: 96x96x3 state_pixels per agent */
  int32_t auto_reset;        /* 1: finished envs are re-spawned inside mcr_step from their staged episode */
  int32_t backwards_flag;    /* :158 */
  int32_t use_ego_color;     /* :160 */
  int32_t car_contacts;      /* 1: car<->car rigid contacts (Box2D default); 0: ghost cars (debug) */
  int32_t max_episode_steps; /* gym TimeLimit from __init__.py:8 (1000); 0 disables */
  int32_t num_streams;       /* 0/1: every kernel on the caller's stream; 2: envs whose dynamics chain is long (a touching car<->car pair,
                              * or a position loop still iterating after 2 sweeps) run it + their raster on internal streams, concurrently
                              * with the others; results are bit-identical in both modes */
  double h_ratio;            /* :159 */
  int32_t skid_particles;    /* 1: keep the skid particles of gym car_dynamics.Car (step(): "Skid trace", _create_particle) so that
                              * mcr_render can draw them (Car.draw(viewer, True), :564); 0: not tracked (observations never show them) */
  int32_t fresh_world;       /* 0 (default): ONE b2World per env for the env's life, as the reference keeps it (:138; _destroy :173-181, reset :341): from an
                              * env's second episode on the fixtures' proxy ids come off the world's free list, which orders same-step tile events
                              * (:113-120: who is a tile's first visitor) and names fixtureA of a car<->car contact.  The ids' rule needs no tree
                              * (csrc/k_world.h): a per-env stack of free leaf ids, advanced by the env's reset pass on the device.
                              * 1: every episode is the first episode of a fresh world (rounds 1-5; the oracle's world mode 0) */
} mcr_config;

const char* mcr_last_error(void);
const char* mcr_version(void);

/* ---- lifetime.  Replaces MultiCarRacing.__init__ (:131-166) / close (:606-611). */
int mcr_create(const mcr_config* cfg, mcr_env** out);
int mcr_destroy(mcr_env* h);

/* ---- host-side episode setup (NO GPU needed).  Replaces reset()'s RNG draws + _create_track + spawn
 * maths (:349-406, :183-338).  An "episode blob" is the host image of one env's device track slot. */
size_t mcr_episode_bytes(void);
/* numpy-compatible MT19937 helpers (RandomState.seed(int) / .seed(array), legacy stream). */
void mcr_mt_seed(uint32_t* mt, uint32_t seed);
void mcr_mt_seed_by_array(uint32_t* mt, const uint32_t* key, int key_len);
double mcr_mt_random_sample(uint32_t* mt);
/* np.random.choice(['CW','CCW']) (:352) -> 1 if 'CW';  np.random.choice(ids,size=N,replace=False) (:356) */
int mcr_mt_choice_cw(uint32_t* mt);
void mcr_mt_car_order(uint32_t* mt, int n, int32_t* order_out);
/* One episode: retries _create_track until success (:359-364), builds tiles/quads/spawn poses.
 * info_out[0..3] = T, P, retries, cw.  `mt_track` advances exactly as env.np_random does. */
int mcr_episode_generate(uint32_t* mt_track, int num_agents, int cw, const int32_t* car_order,
                         void* blob_out, int32_t* info_out);
/* Batched + threaded: per env i draws direction (direction_mode 2) and car order from mt_global[i],
 * then the track from mt_track[i].  direction_mode: 0 'CCW', 1 'CW', 2 random per episode. */
int mcr_episodes_generate(uint32_t* mt_track, uint32_t* mt_global, int n, int num_agents,
                          int direction_mode, void* blobs_out, int32_t* info_out, int num_threads);
/* ... for rows ids[0 .. n) of PER-ENV arrays (mt_track_all / mt_global_all [num_envs][MCR_MT_WORDS], blobs_all [num_envs][mcr_episode_bytes()],
 * info_all [num_envs][12] or NULL), in place. */
int mcr_episodes_generate_rows(uint32_t* mt_track_all, uint32_t* mt_global_all, const int32_t* ids, int n, int num_agents,
                               int direction_mode, void* blobs_all, int32_t* info_all, int num_threads);
/* The blob of a CALLER's track: rows (alpha, beta, x, y) as mcr_episode_unpack hands them out, through everything mcr_episode_generate does
 * behind its track walk (kerb flags, arrays, quads, tile hulls, block boxes, spawn poses) — a generated track fed back gives the generated blob
 * byte for byte.  info_out[0..3] = T, P, 0, cw, or NULL.  MCR_ERR_ARG: a null argument, num_agents outside 1..8, T outside 20..MCR_TILE_CAP (the
 * generator's own rule), an entry that is not finite, more than MCR_QUAD_CAP quads (road tiles + kerbs). */
int mcr_episode_from_track(const double* track /*[T][4]*/, int T, int num_agents, int cw, const int32_t* car_order,
                           void* blob_out, int32_t* info_out);
/* Read-only views into a blob (tests / facade attributes such as env.track). */
int mcr_episode_unpack(const void* blob, int32_t* T, int32_t* P, int32_t* cw, double* track_xyb /*[T*3]*/,
                       float* quads /*[P*8]*/, uint32_t* quad_meta /*[P]*/, double* spawn /*[8*3]*/,
                       double* track_alpha /*[T]*/);

/* ---- the env's b2World across reset() as a LITERAL host-side tree (NO GPU needed).  The reference keeps ONE world for the life of an env
 * (multi_car_racing.py:138; _destroy :173-181 and reset :341 destroy and re-create its bodies): from the second episode on, the fixtures'
 * broadphase proxy ids come off the dynamic tree's free list, and the ids order the contact callbacks of a step — which of two cars that reach a
 * tile in the same step is its first visitor (:113-120) — and name fixtureA of a car<->car contact.  Since round 6 every handle carries that world
 * itself (mcr_config::fresh_world = 0: a per-env stack of free leaf ids on the device, csrc/k_world.h — a proxy's leaf id never depends on the
 * tree's shape); this host-side dynamic AABB tree with Box2D's insertion / balance / free-list rules (rounds 4-5's facade used it) stays as the
 * independent twin the tests hold the stack rule against (tests/test_world_ids.py), and for callers of a fresh_world = 1 handle who want to supply
 * the ids themselves: mcr_world_reset(w, blob) before staging an episode blob (destroys the old episode's proxies and creates the new one's in the
 * reference's order; writes the ids into the blob, header word pad0 = 1, where the contact pass of a fresh_world = 1 handle finds them),
 * mcr_world_step(w, bodies) after EVERY step and after the reset's own step, with the bodies of mcr_get_state (b2Body::SynchronizeFixtures ->
 * b2DynamicTree::MoveProxy in b2World::Solve's order). */
typedef struct mcr_world mcr_world;
mcr_world* mcr_world_create(int num_agents);
void mcr_world_destroy(mcr_world* w);
int mcr_world_reset(mcr_world* w, void* blob_io);
int mcr_world_step(mcr_world* w, const float* bodies /*[N,5,6]*/);
int mcr_world_proxy_ids(const mcr_world* w, int32_t* out, int cap);

/* ---- device side */
/* Copy n host blobs into the STAGED slot of envs env_ids[0..n) (async on stream; blobs must stay valid
 * until the stream reaches this point — use pinned memory for real overlap). */
int mcr_stage_episodes(mcr_env* h, const int32_t* env_ids, int n, const void* blobs, void* stream);
/* Level pools: a finite set of K tracks that the DEVICE re-stages by itself (procgen's num_levels: train on K tracks, evaluate on others;
 * fixed-track evaluation; per-track statistics) — and no host work per step.  d_pool is the caller's device memory [K][mcr_episode_bytes()],
 * 16-byte aligned, holding K episode blobs exactly as mcr_episodes_generate writes them; it must outlive the handle's use of it.  From then on
 * a kernel of the handle (csrc/k_pool.h) does what mcr_stage_episodes does for the host: in front of and behind every mcr_reset and behind
 * every mcr_step / mcr_step_repeat, on the caller's stream, every env that installed its staged episode gets its next one copied from the
 * pool into its staged slot.  Env e plays pool row mcr_pool_level(seed, env_offset + e, k, K, mode) in its k-th episode (k = 0: the first;
 * k counts the episodes the env has installed, by reset or auto-reset):
 *   mode 0 "random"  mcr_mix64(mcr_mix64(seed + 0x9e3779b97f4a7c15 * ((k << 32) | global env))) % K   (splitmix64's finaliser, csrc/mcr_common.h)
 *   mode 1 "cycle"   (global env + k) % K
 * — a pure function: results do not depend on the batch size, on the sharding (env_offset) or on scheduling.  mcr_pool_level is that
 * function on the host (no handle, no GPU; MCR_ERR_ARG for K < 1 or a bad mode).  d_level, [num_envs] int32 on the device or NULL, receives
 * the pool row of each env's CURRENT episode (written when the env installs it; valid once that reset / step is complete on its stream).
 * With a pool an env never finds its staged slot empty at a step's begin: mcr_status word 4 and mcr_debug_read_counters [3] stay 0.
 * MCR_ERR_ARG: NULL handle or pool, K < 1, a misaligned pool, a bad mode.  MCR_ERR_STATE: after the first mcr_reset (the pool is chosen for
 * the life of the handle: the staged slots have ONE owner), or with the refill service running.  While a pool is set mcr_stage_episodes,
 * mcr_refill_start and mcr_poll_consumed return MCR_ERR_STATE.  mcr_load_states / mcr_copy_states / mcr_set_state_blob keep their rule: the
 * staging words of the target's record and its staged slot are not touched, so a restored env goes on with the TARGET's next level. */
int32_t mcr_pool_level(uint64_t seed, uint32_t global_env, uint32_t episode, int32_t K, int mode);
int mcr_set_episode_pool(mcr_env* h, const void* d_pool, int K, uint64_t seed, uint32_t env_offset, int mode, int32_t* d_level);
/* Level curricula, part 1 — weighted level sampling (Prioritized Level Replay and its kin: the learner scores the levels, the env draws the
 * next level in proportion to the score).  A switch on a pool created with mode 0; mcr_set_episode_pool and mcr_pool_level keep their two modes.
 *   uniform   u = (mcr_mix64(mcr_mix64(seed + 0x9e3779b97f4a7c15 * ((k << 32) | global env))) >> 11) * 2^-53: mode 0's hash with mode 0's key,
 *             an exact f64 in [0, 1)
 *   CDF       from weights w[0 .. K) (f64): a weight that is not finite or is negative counts as 0; S_j is the running f64 sum in index order;
 *             cdf[j] = S_j / S_{K-1}.  If S_{K-1} is 0 or not finite the CDF is the uniform one, cdf[j] = (double)(j + 1) / (double)K, and the
 *             "fell back" flag is raised.  A new sampler starts with the uniform CDF — bit for bit the CDF of all-ones weights.
 *   level     the smallest j with u < cdf[j] (K - 1 if there is none).  A level of weight 0 is never drawn.
 * mcr_level_cdf (returns 1 if it fell back, 0 otherwise; MCR_ERR_ARG for NULL or K < 1) and mcr_pool_level_weighted (MCR_ERR_ARG for a NULL
 * cdf or K < 1) are these definitions on the host: no handle, no GPU.  The kernels evaluate the same code (csrc/mcr_common.h).
 * WHEN a level is drawn: an env's NEXT episode is staged behind the reset or step in which it installed its current one (mcr_set_episode_pool),
 * and the level is drawn there, from the CDF in force at that point of the stream; it is kept per env in d_staged_level and becomes the
 * env's d_level row when the env installs that episode.  New weights therefore act with a lag of ONE EPISODE per env.  Rollouts remain a
 * pure function of (seed, global env, episode ordinal, the sequence of mcr_level_weights calls in stream order): independent of the batch
 * size and of the sharding, provided every rank sets the same weights at the same points.  d_staged_level is staging state like the staged
 * slot: mcr_load_states / mcr_copy_states / mcr_set_state_blob leave it the target's, and the state blob does not change.
 * mcr_set_level_sampler: d_cdf [K] f64 and d_staged_level [num_envs] int32 are the caller's device memory for the life of the handle; writes
 * the uniform CDF into d_cdf (a blocking copy).  MCR_ERR_ARG: a NULL argument.  MCR_ERR_STATE: no pool, a mode-1 pool, after the first mcr_reset.
 * mcr_level_weights: one small kernel on `stream` — the stepping stream — rebuilds d_cdf from d_weights [K] f64 (device) in the order above
 * and stores the fell-back flag into *d_fell_back (int32 on the device; may be NULL).  Only enqueues.  MCR_ERR_STATE without a sampler. */
int mcr_level_cdf(const double* w, int K, double* cdf_out);
int32_t mcr_pool_level_weighted(uint64_t seed, uint32_t global_env, uint32_t episode, const double* cdf, int32_t K);
int mcr_set_level_sampler(mcr_env* h, double* d_cdf /*[K]*/, int32_t* d_staged_level /*[B]*/);
int mcr_level_weights(mcr_env* h, const double* d_weights, int32_t* d_fell_back, void* stream);
/* Level curricula, part 2 — per-level episode statistics, what the weights are computed from.  Behind every mcr_step / mcr_step_repeat, on
 * the caller's stream, a kernel (csrc/k_levelstats.h: definition and arithmetic contract) rewrites d_finished_level [num_envs] int32 — -1 for
 * an env whose d_done row is 0, else the pool row of the episode that ENDED (d_level as it stood before the re-stage) if that is in 0 .. K-1,
 * else K: the "unattributed" row, e.g. a level row of -1 after mcr_load_states — and adds the episode to row d_finished_level[e] of d_stats
 * [K + 1][mcr_level_stats_dim(num_agents) = 3 + 2N] f64: col 0 episodes, 1 those with d_trunc set, 2 sum of d_ep_len, 3 .. 3+N sum of
 * d_ep_return per car, 3+N .. 3+2N sum of its squares.  Per row and column the additions happen in step order and within a step in
 * ascending env index, one f64 add each (the square: one f64 multiply first): a host reproduces every bit; no floating-point atomics.
 * Counting rule (mcr_read_rollout_stats'): a done row counts once per step CALL that reports it — once per macro-step; an env of an
 * auto_reset = 0 handle that is stepped past its end reports done, and counts, again in every call until it is reset.
 * The caller zeroes d_stats (and may zero it again at any point of the stream).  Needs a pool with a d_level buffer and the
 * mcr_set_episode_stats buffers (MCR_ERR_STATE otherwise); NULL pointers switch it off; takes effect with the next step.  No HIP call.
 * Per handle, hence per rank: a job may all-reduce d_stats, after which the sums depend on the world size in their last bits. */
int mcr_level_stats_dim(int num_agents);
int mcr_set_level_stats(mcr_env* h, int32_t* d_finished_level, double* d_stats /*[K+1][3+2N]*/);
/* reset() (:340-408): installs the staged episode for every env whose d_env_mask byte != 0 (NULL = all),
 * spawns the cars, runs the no-action step of :408 and writes the first observation.
 * d_obs: [B,N,96,96,3] u8 or NULL; with mcr_set_obs_format the layout that call describes. */
int mcr_reset(mcr_env* h, const uint8_t* d_env_mask, uint8_t* d_obs, void* stream);
/* step() (:410-509) for all B envs.
 *   d_actions  [B,N,3] f32 (steer,gas,brake), NULL = the action-less step of :408
 *   d_obs      [B,N,96,96,3] u8 or NULL (ignored when obs_enabled == 0); gray: [B,N,96,96] (k = 1) or the ring [B,N,2k,96,96] (k > 1,
 *              mcr_set_obs_format), which must not be NULL
 *   d_reward   [B,N] f64 step_reward (:443,:507)
 *   d_done     [B] u8   (:498-499, :503-506, TimeLimit)
 *   d_trunc    [B] u8 or NULL: info['TimeLimit.truncated']
 * With auto_reset, a finished env's obs row is the first observation of its next episode (its last frame: mcr_set_terminal_obs). */
int mcr_step(mcr_env* h, const float* d_actions, uint8_t* d_obs, double* d_reward, uint8_t* d_done,
             uint8_t* d_trunc, void* stream);
/* Action repeat (frame skip): ONE macro-step = FrameSkip_repeat(TimeLimit(env)) per env, auto-reset outside it.  The same d_actions drive up to
 * `repeat` consecutive env steps (sub-steps) of every env; an env stops at the sub-step in which its episode ends (all tiles visited, out of
 * the playfield, TimeLimit — which keeps counting env steps, as do d_ep_len and mcr_refill_lag's epochs).  Per env:
 *   d_reward   the f64 sum of its sub-step rewards, added in sub-step order starting from the first one's value (gym's `total += r`)
 *   d_done     the OR of the sub-steps' flags (with auto_reset at most one episode ends per env and macro-step); d_trunc: the ending sub-step's
 *   d_obs      drawn ONCE, from the state after the last sub-step; a stacked ring advances once (one drawing step: mcr_obs_window moves by one),
 *              so the stack holds macro-step frames; the state-vector observation (mcr_set_state_obs) is written once, too
 * With auto_reset an env whose episode ended in the macro-step is re-spawned in its LAST sub-step and shows the first observation (first state) of
 * the next episode, which this macro-step has not advanced; episode, proxy ids and RNG streams are those of a re-spawn in the ending sub-step.
 * In between the env is parked (inactive, zero outputs) — not starved: neither mcr_debug_read_counters [3] nor mcr_status word 4 count it, unless
 * the host has staged no episode by the last sub-step (then it is an ordinary frozen env from there on).  A frozen env thaws in a last sub-step only.
 * Without auto_reset a finished env goes through the later sub-steps as it goes through later mcr_step calls.
 * repeat == 1 is mcr_step (which forwards here): the same launches, the same bits.  repeat > 1: the sub-steps are ordinary steps of the same
 * topology, enqueued without synchronising, the first repeat - 1 without a draw; MCR_ERR_ARG for NULL d_actions or a repeat outside
 * 1 .. MCR_REPEAT_MAX.  With mcr_set_step_graph(1) a macro-step of repeat > 1 runs as plain launches (no macro-step graph is captured).
 * With terminal observations set (mcr_set_terminal_obs) repeat > 1 returns MCR_ERR_STATE: the terminal frame would have to be drawn in a
 * sub-step that draws nothing — the follow-up to this entry. */
#define MCR_REPEAT_MAX 16
int mcr_step_repeat(mcr_env* h, const float* d_actions, int repeat, uint8_t* d_obs, double* d_reward, uint8_t* d_done,
                    uint8_t* d_trunc, void* stream);
/* render(mode) at another viewport (multi_car_racing.py:511-604 with VP_W x VP_H of :573-586; 'rgb_array' = 600 x 400):
 * the CURRENT state of env `env` as seen by each of its agents, d_out [N, height, width, 3] u8 (device), rows top-down.
 * Needs obs_enabled. */
int mcr_render(mcr_env* h, int env, int width, int height, uint8_t* d_out, void* stream);
/* Episode statistics (what gym's RecordEpisodeStatistics would add): in the step that ends an env's
 * episode (done), mcr_step writes the sum of the step rewards of that episode per agent into d_ep_return[B,N] and
 * its length in steps into d_ep_len[B]; other rows are left untouched.  NULL disables either. */
int mcr_set_episode_stats(mcr_env* h, double* d_ep_return, int32_t* d_ep_len);
/* Terminal observations (what a baselines / SB3-style VecEnv hands out as info["terminal_observation"]).  The reference renders
 * the state AFTER the last solve of an episode and returns it with done = True (multi_car_racing.py:431, :509; TimeLimit: __init__.py:8); with
 * auto_reset the env's row of d_obs already shows the first observation of the next episode.  With this set, every step that ends an env's
 * episode and re-spawns it also draws that last frame: entry i = env d_term_ids[i], frames d_term_obs[i] [N,96,96,3] (gray: [N,96,96], or with
 * k > 1 [N,k,96,96] — the previous k - 1 frames of the episode, then its last one, what a stacked VecEnv hands out); *d_term_count = the
 * number of entries of the last completed step (0 when no episode ended), at most `cap` — episodes that end beyond `cap` in one step get no
 * entry (cap = num_envs never drops one).  The three buffers are the caller's device memory, overwritten by every mcr_step with actions and
 * valid once that step is complete on its stream.  An env that ends while the host has not staged its next episode FREEZES instead of being
 * re-spawned (mcr_debug_read_counters [3]) and gets no entry.  All NULL: off.  Synchronises the device (allocates the entries' state). */
int mcr_set_terminal_obs(mcr_env* h, uint8_t* d_term_obs, int32_t* d_term_ids, int32_t* d_term_count, int cap);
/* Observation format (gym's GrayScaleObservation + FrameStack(k), drawn by the raster itself).  format MCR_OBS_RGB (stack 1) or MCR_OBS_GRAY
 * with stack k = 1 .. MCR_OBS_STACK_MAX.  A gray pixel is (4899 R + 9617 G + 1868 B + 8192) >> 14 of the RGB bytes the RGB format would
 * store (OpenCV's COLOR_RGB2GRAY on 8-bit data), HUD included.  Per view d_obs then holds one 96x96 frame (k = 1) or a RING of 2k frames
 * (k > 1): drawing step d (an mcr_step with d_obs, counted from the handle's creation) writes its frame into slots j = d mod k and j + k;
 * after it the observation is slots j + 1 .. j + k, oldest first, contiguous per view (mcr_obs_window) — no frame is ever shifted.  A reset
 * or re-spawn writes the env's first frame into slots j .. j + k (j: the head of the last drawing step); the observation is then that
 * frame k times, as gym's FrameStack does (SB3's VecFrameStack zero-fills instead).  The format shapes the terminal entries, so it is set
 * before mcr_set_terminal_obs, and before the first mcr_reset (MCR_ERR_STATE otherwise, and with obs_enabled == 0);
 * MCR_ERR_ARG for a NULL handle, a bad format or stack, or RGB with stack > 1.  With k > 1 every mcr_step must pass d_obs (MCR_ERR_ARG
 * otherwise: a step that skipped its draw would leave a hole in the ring), and episodes must last at least k steps (max_episode_steps). */
int mcr_set_obs_format(mcr_env* h, int format, int stack);
/* bytes of d_obs per view: 27,648 (RGB), 9,216 (gray, k = 1), 2k x 9,216 (gray, k > 1) */
size_t mcr_obs_bytes_per_view(const mcr_env* h);
/* the first ring slot of the observation after the last ENQUEUED drawing step (k > 1: 1 .. k; k = 1 and RGB: 0) */
int mcr_obs_window(const mcr_env* h);
/* State-vector observations: the low-dimensional observation a non-pixel policy trains on, written on the device by a kernel of its own
 * (csrc/k_stateobs.h, which holds the feature table and the arithmetic contract) after every mcr_reset and every mcr_step, on the caller's
 * stream behind the step — valid once that call is complete on its stream, with obs_enabled 0 or 1.  Per car F = 18 + 2 K + 4 (N - 1) f32
 * features in raw SI / model units (no normalisation): the hull's velocity in its own frame, yaw rate, wheel speeds, steering angle, on-road
 * bits, progress, offset and heading against the nearest track point, the episode's direction, K waypoints `stride` tiles apart ahead of the
 * car in its frame, and every other car's relative position and velocity.  Every value is defined in IEEE f64 operations in a fixed order
 * and rounded to f32 once: a host reproduces it bit for bit (tests/state_obs_ref.py).  Rows of envs that are not active (never reset,
 * frozen) are zeros; an env that re-spawned in the step (auto_reset) shows the first state of its new episode, like its d_obs row.
 * mcr_state_obs_dim: F for num_agents 1..8 and waypoints 0..16 (MCR_ERR_ARG otherwise); no handle, no GPU needed. */
int mcr_state_obs_dim(int num_agents, int waypoints);
/* d_state: the caller's device buffer [B, N, F] f32, F = mcr_state_obs_dim(num_agents, waypoints); NULL turns the feature off (the step path
 * then does nothing new).  MCR_ERR_ARG for a NULL handle, waypoints outside 0..16 or stride outside 1..64.  Allowed at any time; takes effect
 * with the next mcr_reset / mcr_step / mcr_state_obs_now.  No synchronisation. */
int mcr_set_state_obs(mcr_env* h, float* d_state, int waypoints, int stride);
/* Recompute the tensor from the CURRENT state on `stream` (after mcr_set_bodies / mcr_set_state_blob, which do not; tests).  MCR_ERR_STATE
 * when no buffer is set.  Only enqueues: the features read no backward / on-grass flags, so the pending flag scans (mcr_get_env_state's
 * note) are neither launched nor waited for. */
int mcr_state_obs_now(mcr_env* h, void* stream);
/* Range-finder observations: what racing policies are usually trained on (TORCS's 19-ray `track` and `opponents` sensors, a lidar) — per car
 * a fan of R rays from the hull's body origin, and per ray two ranges: channel 0 to the track's borders (the two polylines through the road
 * quads' outer vertices; kerbs are no borders), channel 1 to the hull polygons of the env's other cars.  [B, N, 2, R] f32 in world units,
 * clamped to max_range, written on the device by a kernel of its own (csrc/k_rangeobs.h, which holds the definition and the arithmetic
 * contract) wherever the state vector is: after every mcr_reset, mcr_step (once per macro-step) and state restore / copy, on the caller's
 * stream behind the step, with obs_enabled 0 or 1.  Ray k points along dirs[k][0] forward + dirs[k][1] right in the hull's frame — (cos, sin)
 * of an angle measured from straight ahead towards the car's right; a direction is not renormalised, a range is the ray parameter.  Every
 * value is defined in IEEE f64 operations in a fixed order and rounded to f32 once: a host reproduces it bit for bit
 * (tests/range_obs_ref.py).  Rows of envs that are not active (never reset, frozen) are zeros; an env that re-spawned in the step shows the
 * first state of its new episode.  With one car channel 1 is max_range.  At a folded inner hairpin the inner border can lie inside the road:
 * channel 0 is the first border SEGMENT a ray meets. */
#define MCR_RANGE_RAYS_MAX 32
/* mcr_set_range_obs' validation of the table, the ray count and the range without a handle (no GPU needed): MCR_OK or MCR_ERR_ARG */
int mcr_check_range_obs(const float* dirs, int rays, float max_range);
/* d_ranges: the caller's device buffer [B, N, 2, rays] f32; NULL turns the feature off (the step path then does nothing new; the other
 * arguments are ignored).  dirs: host [rays][2] f32, copied (it travels with every launch).  MCR_ERR_ARG for a NULL handle, rays outside
 * 1..MCR_RANGE_RAYS_MAX, NULL dirs, a dirs entry that is not finite, or a max_range that is not finite or <= 0.  Allowed at any time; takes
 * effect with the next mcr_reset / mcr_step / mcr_range_obs_now.  No HIP call, no synchronisation. */
int mcr_set_range_obs(mcr_env* h, float* d_ranges, const float* dirs /* [rays][2] host */, int rays, float max_range);
/* Recompute the tensor from the CURRENT state on `stream` (after mcr_set_bodies / mcr_set_state_blob, which do not; tests).  MCR_ERR_STATE
 * when no buffer is set.  Only enqueues: the ranges read no backward / on-grass flags. */
int mcr_range_obs_now(mcr_env* h, void* stream);
/* Grid observations: the ego-centred bird's-eye-view tensor driving policies are usually trained on — per car rows x cols bytes fixed to the
 * hull, row 0 farthest ahead, column 0 leftmost, [B, N, rows, cols] u8.  A cell's byte says what lies under its CENTRE: MCR_GRID_ROAD (a
 * road or kerb quad: a car standing there would not be driving_on_grass), MCR_GRID_FRESH (a tile this car has not visited: it still gets
 * paid there), MCR_GRID_TAKEN (a tile another car has visited: the pay is dampened), MCR_GRID_CAR (a hull polygon of another car); bits 4..7
 * are 0.  `cell` is the cell size in world units; (origin_row, origin_col) is where the hull's body origin sits, in cell units from the
 * grid's top left corner — fractional or outside the grid if the caller wishes.  csrc/k_gridobs.h holds the definition and the arithmetic
 * contract: "under" is the reference's own strict-interior predicate in IEEE f64 (a centre exactly on an edge is in nothing), and a host
 * reproduces every bit (tests/grid_obs_ref.py).  Written on the device by a kernel of its own wherever the range finder is: after every
 * mcr_reset, mcr_step (once per macro-step) and state restore / copy, on the caller's stream behind the step, with obs_enabled 0 or 1.  Rows
 * of envs that are not active (never reset, frozen) are zeros; an env that re-spawned in the step shows the first state of its new episode
 * (the tiles the cars spawned on are visited, as the reference's reset leaves them; every other tile cell is FRESH).  With one car MCR_GRID_TAKEN and MCR_GRID_CAR are never set. */
#define MCR_GRID_MAX 64
#define MCR_GRID_ROAD 1
#define MCR_GRID_FRESH 2
#define MCR_GRID_TAKEN 4
#define MCR_GRID_CAR 8
/* mcr_set_grid_obs' validation of the geometry without a handle (no GPU needed): MCR_OK, or MCR_ERR_ARG for rows or cols outside
 * 1..MCR_GRID_MAX, a cell that is not finite or <= 0, or an origin that is not finite */
int mcr_check_grid_obs(int rows, int cols, float cell, float origin_row, float origin_col);
/* d_grid: the caller's device buffer [B, N, rows, cols] u8 at ANY byte alignment (a view is rows * cols bytes; odd products happen); NULL
 * turns the feature off (the step path then does nothing new; the other arguments are ignored).  MCR_ERR_ARG for a NULL handle or what
 * mcr_check_grid_obs refuses.  Allowed at any time; takes effect with the next mcr_reset / mcr_step / mcr_grid_obs_now.  No HIP call, no
 * synchronisation. */
int mcr_set_grid_obs(mcr_env* h, uint8_t* d_grid, int rows, int cols, float cell, float origin_row, float origin_col);
/* Recompute the tensor from the CURRENT state on `stream` (after mcr_set_bodies / mcr_set_state_blob / mcr_set_env_state, which do not;
 * tests).  MCR_ERR_STATE when no buffer is set.  Only enqueues: the grid reads the tiles' visit bits, which the step itself writes, and no
 * backward / on-grass flags. */
int mcr_grid_obs_now(mcr_env* h, void* stream);
/* Car-contact observations: who touched whom in the step, and how hard — what Box2D's PostSolve would report, reduced on the device from the
 * car<->car manifold store every env keeps for warm starting (csrc/k_contactobs.h holds the definition and the arithmetic contract;
 * csrc/k_carcontacts.h the record layout).  Two tensors, written by a kernel of its own on the caller's stream behind every mcr_reset, every env
 * step of mcr_step / mcr_step_repeat and every state restore / copy, with obs_enabled 0 or 1:
 *   d_mask    [B, N] int32: bit j (0..7) car j shared a stored touching manifold with this car; bit 8 this car's fixture in such a record is a
 *             hull polygon (fixture index < 4), bit 9 it is a wheel (index >= 4)
 *   d_impulse [B, N, N] f64: entry [a][j] the sum of the normal impulses of every manifold point between cars a and j, one f64 add per point
 *             in store order — a host reproduces every bit (tests/contact_obs_ref.py); [a][j] and [j][a] are the same bits, the diagonal is 0.
 * mcr_step_repeat: the kernel runs behind every sub-step; sub-step 0 starts from zero, the later ones continue the chain of adds from the
 * value in the buffer and OR the masks.  An env that is not live at that point (never reset, frozen, parked behind the end of its episode)
 * contributes nothing, so the env step in which an episode ends is never reported: with repeat = 1 and auto_reset a `done` row shows the
 * first state of the new episode (no contacts).  After mcr_reset / mcr_load_states / mcr_copy_states every row is recomputed, without
 * accumulation, from the env's store: what that state's last env step produced (a clone shows its source's).  Where the store overflowed
 * (mcr_status word 2) the outputs describe the MCR_CC_MAX records that were kept: the store's documented deviation.
 * Both pointers NULL turn the feature off (nothing is launched).  MCR_ERR_ARG: exactly one pointer NULL, a NULL handle, num_agents < 2, a
 * handle created with car_contacts = 0.  Allowed at any time; takes effect with the next mcr_reset / mcr_step.  No HIP call. */
int mcr_set_contact_obs(mcr_env* h, int32_t* d_mask /* [B][N] */, double* d_impulse /* [B][N][N] */);
/* Recompute both tensors, without accumulation, from the stores as they stand, on `stream`.  MCR_ERR_STATE when no buffers are set.  Only enqueues. */
int mcr_contact_obs_now(mcr_env* h, void* stream);
/* Early episode ending on the device: "no new tile for `patience` env steps" and "off the road for `offroad_patience` env steps" (csrc/k_endrules.h
 * holds the definition; tests/end_rules_ref.py restates it as a wrapper round the oracle).  Three buffers the CALLER owns:
 *   d_counters [B, 4] int32, 16-byte aligned: idle (env steps since the counted cars' sum of tile_visited_count last changed), offroad (env
 *              steps in a row in which every — offroad_mode 0 — or some — offroad_mode 1 — counted car had no wheel on a tile), tvc_sum
 *              (that sum), a reserved 0; both counts saturate at INT32_MAX and start at 0 with every episode
 *   d_armed    [B] u8: bit 0 idle >= patience > 0, bit 1 offroad >= offroad_patience > 0, as of the last env step
 *   d_reason   [B] u8: the armed word the env entered its last env step with — non-zero: that step ended the episode by these rules;
 *              mcr_step_repeat ORs the sub-steps' words, like `done`.  An action-less mcr_step runs no pass and leaves the word of the last
 *              env step taken with actions in place (VecMultiCarRacing.step(None) zeroes its tensor itself)
 * A kernel of its own counts behind every env step taken WITH actions (the action-less step counts nothing and ends nothing), for the cars
 * of agent_mask (bit a: car a), on the caller's stream.  An env that is armed ends its episode in the NEXT env step taken with actions, one
 * step after its rule was first met, exactly as under the TimeLimit: truncated = !done, then done = 1 — so truncated = 0 says that the
 * reference's own rules (or the TimeLimit) ended the episode in that very step —, end_reward added to every car's step reward (one f64 add
 * behind the reference's arithmetic: reward and episode return stay reproducible bit for bit), and everything behind `done` as ever:
 * auto-reset and re-spawn, parking inside a macro-step, episode statistics, terminal entries, level statistics.  With auto_reset 0 an env
 * stepped past such an ending stays armed while its rule holds and reports done in every step until it is reset.  Envs that are not live
 * (never reset, frozen, parked) keep their counters and are not armed.  mcr_reset / mcr_load_states / mcr_copy_states run the kernel's
 * SETTLE pass: rows of envs in the first state of an episode start over, every other row keeps its counters and has its armed byte
 * recomputed from them — restore the counter rows you saved with the states, in front of mcr_load_states, and the continuation is bit-identical.
 * All three pointers NULL turn the feature off (nothing is launched, the step's kernels test one null pointer).  MCR_ERR_ARG: some but not
 * all pointers NULL, a patience < 0, both patiences 0 with buffers given, offroad_mode outside {0, 1}, an end_reward that is not finite,
 * counters not 16-byte aligned — all checked in front of the handle —, a NULL handle, an agent_mask without a car below num_agents.
 * Allowed at any time; takes effect with the next mcr_reset / mcr_step.  No HIP call. */
int mcr_set_end_rules(mcr_env* h, int patience, int offroad_patience, int offroad_mode, uint32_t agent_mask, double end_reward,
                      int32_t* d_counters /* [B][4] */, uint8_t* d_armed /* [B] */, uint8_t* d_reason /* [B] */);
/* the value checks of mcr_set_end_rules for a given num_agents; no handle, no GPU needed */
int mcr_check_end_rules(int num_agents, int patience, int offroad_patience, int offroad_mode, uint32_t agent_mask, double end_reward);
/* The SETTLE pass on `stream`: after writing d_counters yourself (a restore), or after mcr_set_state_blob / mcr_set_env_state, which leave
 * the buffers alone.  MCR_ERR_STATE when no buffers are set.  Only enqueues. */
int mcr_end_rules_now(mcr_env* h, void* stream);
/* the manifold store's sizes in u32 words, per env and per record (either pointer may be NULL); returns the records kept per env (MCR_CC_MAX).
 * An env's store: word 0 the record count, 1 the overflow mark, 2-3 the joint order, then the records.  No handle, no GPU needed. */
int mcr_contact_store_words(int32_t* words_per_env, int32_t* words_per_record);
/* the four hull fixture polygons as the kernels hold them (b2PolygonShape::Set's vertex order): out [4][8][2] f32 body-frame vertices,
 * counts [4]; no handle, no GPU needed (tests pin the host restatement of the range-finder's channel 1 with it) */
int mcr_hull_polygons(float* out, int32_t* counts);
/* Scripted drivers: cars the DEVICE drives — opponents for a learner, or an expert that labels states (imitation learning, DAgger, a baseline
 * return).  A stateless track-following controller (csrc/k_driver.h holds the definition and the arithmetic contract): pure pursuit of the
 * track point L1 tiles ahead of the nearest one for the steering, a target speed that falls with the curvature towards the point L2 tiles
 * ahead for gas and brake.  An action is a pure function of the env's current state, its episode and the car's parameter row, defined in
 * IEEE f64 operations in a fixed order and rounded to f32 once: a host reproduces it bit for bit (tests/driver_ref.py), and snapshots,
 * clones, level pools and sharding need nothing new.  On its own it follows the track on a free road; it does NOT avoid collisions, overtake,
 * or recover from a spin or from the grass — mcr_set_racecraft (below) adds a side-step, a follow rule and a speed cap on the grass.
 * A parameter row is MCR_DRV_PARAMS floats: L1, L2 (integers 1..64), v_max (> 0, the speed on a straight), K_s, K_c, K_g, K_b (gains >= 0),
 * offset (lateral offset of the line, positive = to the right of the episode's driving direction), gas_max, brake_max (in [0, 1]). */
#define MCR_DRV_PARAMS 10
#define MCR_DRV_DEFAULTS { 4.0f, 12.0f, 70.0f, 8.0f, 20.0f, 0.2f, 0.1f, 0.0f, 1.0f, 0.8f }
/* the default row (host [MCR_DRV_PARAMS]); no handle, no GPU needed */
int mcr_driver_defaults(float* out);
/* mcr_set_drivers' validation of rows and mask without a handle (no GPU needed): MCR_OK or MCR_ERR_ARG */
int mcr_check_drivers(int num_agents, const float* params, uint32_t agent_mask);
/* params: host [num_agents][MCR_DRV_PARAMS], copied; agent_mask: bit a = car a is scripted (0 is legal: expert labels only); d_actions: the
 * caller's device buffer [B, N, 3] f32 that mcr_driver_actions fills by default.  MCR_ERR_ARG: a NULL handle, rows or buffer, a value out
 * of range or not finite, mask bits >= num_agents.  May be called again: launches enqueued later use the new rows (they travel with the
 * launch).  No HIP call, no synchronisation.  The step entry points are unchanged: the filled buffer is simply the d_actions they are given. */
int mcr_set_drivers(mcr_env* h, const float* params, uint32_t agent_mask, float* d_actions);
/* One kernel on `stream`, from the CURRENT state: for every car whose bit is set in the mask the controller's action, for every other car a
 * copy of its row of d_actions_in (zeros if that is NULL; it is only read, and may be the output buffer itself); rows of envs that are not
 * active (never reset, frozen) are zeros.  agent_mask_override: 0xffffffff = every car, anything else = the registered mask.  d_out: the
 * buffer to fill, NULL = the registered one.  So "merge the scripted cars into the step's buffer" is (actions, 0, NULL) and "every car's
 * expert action into a buffer of the caller's" is (NULL, 0xffffffff, buf).  MCR_ERR_STATE without mcr_set_drivers.  Only enqueues. */
int mcr_driver_actions(mcr_env* h, const float* d_actions_in, uint32_t agent_mask_override, float* d_out, void* stream);
/* Racecraft: an optional second parameter row per scripted car (csrc/k_driver.h holds the definition, tests/racecraft_ref.py restates it).
 * A car with its bit in the racecraft mask looks at EVERY car of its env (scripted or not): the nearest car ahead within `look` track points
 * is its leader; if the leader sits within w_block of the car's line, the line is moved w_pass to the leader's free side (never beyond
 * +-off_max); while the leader is within w_block laterally in the car's own frame the target speed is capped at the leader's speed plus
 * K_f (gap - d_safe); and a car more than w_off from the centre line drives at v_off at most.  Still stateless, still reproducible bit for
 * bit.  Every other scripted car keeps the plain controller, bit for bit, and a handle without racecraft launches the plain kernel.
 * A row is MCR_RC_PARAMS floats: look (an integer 1..64), w_block, w_pass, off_max, d_safe, K_f, w_off, v_off (finite, >= 0). */
#define MCR_RC_PARAMS 8
#define MCR_RC_DEFAULTS { 24.0f, 3.5f, 4.25f, 4.5f, 16.0f, 2.0f, 7.5f, 15.0f }
/* the default row (host [MCR_RC_PARAMS]); no handle, no GPU needed */
int mcr_racecraft_defaults(float* out);
/* mcr_set_racecraft's validation of rows and mask without a handle (no GPU needed): MCR_OK or MCR_ERR_ARG */
int mcr_check_racecraft(int num_agents, const float* params, uint32_t agent_mask);
/* params: host [num_agents][MCR_RC_PARAMS], copied; agent_mask: bit a = car a races.  NULL params or mask 0 turn racecraft off.
 * mcr_driver_actions then uses the extended controller for the cars that are both in the mask it drives (the registered one, or every car
 * under its override) and in this one, and the plain controller for the rest.  MCR_ERR_STATE before mcr_set_drivers; MCR_ERR_ARG as
 * mcr_set_drivers.  May be called again; no HIP call, no synchronisation. */
int mcr_set_racecraft(mcr_env* h, const float* params, uint32_t agent_mask);
/* Rollout statistics accumulated on the device since creation / the last reset of the counters (synchronises):
 * out2[0] = episodes finished, out2[1] = sum of their returns over all agents.  These are the per-rank inputs of the
 * job-wide metric all-reduce. */
int mcr_read_rollout_stats(mcr_env* h, double* out2, int reset);
/* Replay mcr_step as a hipGraph (1) or as plain launches (0, default).  A step is a fixed sequence of launches whose
 * arguments change only with an internal parity; the graph is (re)captured whenever an argument of mcr_step differs from
 * the captured call (buffers, stream) and bypassed while kernel timing is enabled.  Results are identical; the measured
 * gain at B=4096 is 0.4 % (the gaps between dependent kernels are not host launch cost), so it is off by default. */
int mcr_set_step_graph(mcr_env* h, int enable);
/* Envs whose staged episode was consumed (installed by a reset or an auto-reset) since the last poll: the host must
 * stage a fresh one for each.  Reads per-env install counters the kernels write to mapped host memory — no device
 * synchronisation, `stream` is unused; an install whose kernel has not finished yet shows up in a later poll.
 * Writes up to `cap` env ids; returns the count (>=0) or an error. */
int mcr_poll_consumed(mcr_env* h, int32_t* env_ids_out, int cap, void* stream);
/* The refill service: host threads owned by the handle (one service thread + up to min(gen_threads, 6) generator threads that stay awake while
 * there is work) do what a stepping loop would do with the three calls above after every step —
 * poll the consumed-episode counters, generate the next episode of every env that re-spawned from ITS rows of the caller's RNG-state arrays
 * (mt_track / mt_draw [num_envs][MCR_MT_WORDS], advanced in place), write the blob into ITS row of blobs_pinned [num_envs][mcr_episode_bytes()]
 * (page-locked host memory: the staging source) and episode_info [num_envs][12] (T, P, retries, cw, car_order[8]; may be NULL), stage it.
 * The reference generates a track inside reset() on the stepping thread (:359-364); here that work is off the stepping loop, in native
 * code (no interpreter: bench.py --emulate-world).  The arrays belong to the caller and must outlive the service; while it runs,
 * mcr_poll_consumed is refused and the caller must not call mcr_stage_episodes.  mcr_destroy stops it.
 * mcr_refill_wait: every consumption visible now is staged on return (synchronise the stepping stream first to mean "all").
 * mcr_refill_lag: steps launched since the oldest not-yet-staged consumption was noticed (0: none) — a stepping loop that finds it near
 * the shortest possible episode should wait instead of letting an env freeze.  mcr_refill_hold(1): the service ignores consumptions (tests). */
int mcr_refill_start(mcr_env* h, uint32_t* mt_track, uint32_t* mt_draw, int direction_mode, int gen_threads, void* blobs_pinned, int32_t* episode_info);
int mcr_refill_stop(mcr_env* h);
int mcr_refill_wait(mcr_env* h);
int mcr_refill_lag(mcr_env* h);
int mcr_refill_hold(mcr_env* h, int hold);
long long mcr_refill_generated(mcr_env* h);
/* diagnostics of the last mcr_refill_wait: tracks queued / being generated / finished-but-unstaged at entry, service cycles run, tracks the waiting
 * thread generated itself, microseconds inside the cycles (polling + staging), microseconds in total, generator threads */
int mcr_refill_debug(mcr_env* h, long long* out8);

/* ---- state access for differential tests / facade attributes (synchronous) */
/* bodies [B,N,5,6] f32 (c.x c.y angle v.x v.y w; body 0 hull, 1..4 wheels FL FR RL RR)
 * joints [B,N,4,4] f32 (impulse x y z, motorImpulse); wheels [B,N,4,5] f64 (gas brake steer phase omega)
 * limit [B,N,4] i32; on_road [B,N,4] u8; sleep [B,N,5] f32.  Any pointer may be NULL. */
int mcr_get_state(mcr_env* h, float* bodies, float* joints, double* wheels, int32_t* limit, uint8_t* on_road,
                  float* sleep);
int mcr_set_bodies(mcr_env* h, const float* bodies /*[B,N,5,6]*/);
/* reward [B,N] f64 (self.reward), tile_visited_count [B,N] i32, backward/on_grass [B,N] u8,
 * t [B] f64, tile_flags [B,MCR_TILE_CAP] u16 (bits 0..7 road_visited per agent, bit 8 recoloured).
 * backward / on_grass: a completed mcr_step guarantees its observations, rewards, done flags, episode statistics and
 * terminal frames — not that these two flags of its main envs are already in device memory: on the phase-word path
 * (N <= 3) their scans run beside the NEXT step's dynamics.  Every call that reads or writes them (this one,
 * mcr_get_state, mcr_set_bodies, the state blobs, mcr_reset, mcr_render, mcr_destroy, a step that
 * takes another path) launches the pending scans first: the values returned here are always those of the last step. */
int mcr_get_env_state(mcr_env* h, double* reward, int32_t* tile_visited_count, uint8_t* backward,
                      uint8_t* on_grass, double* t, uint16_t* tile_flags, int32_t* num_tiles);
/* Run the backward / on-grass scans (csrc/k_flags.h) NOW, on the state as it stands, on `stream`: the pending scans of the last step first,
 * then one scan per car of every env — after mcr_set_bodies / a state restore, which leave the flags of the last step in place (tests).
 * An env that is not active, or that no step has followed since its reset(), keeps its flags.  No touch verdicts, no other state is
 * written.  MCR_ERR_ARG for a NULL handle (checked before any HIP call).  Only enqueues: no synchronisation. */
int mcr_flags_now(mcr_env* h, void* stream);
/* Test / facade plumbing, the counterparts of mcr_get_state's `wheels` and of mcr_get_env_state; synchronous like mcr_set_bodies, the
 * pending flag scans launched and waited for first.
 * mcr_set_wheels: phase and omega (columns 3 and 4) of every wheel; columns 0..2, the controls, are ignored.
 * mcr_set_env_state: self.reward, self.t and the tile flags — any pointer may be NULL; those three fields only: visit counts, the
 * backward / on-grass flags and every other field of the env record stay as they are. */
int mcr_set_wheels(mcr_env* h, const double* wheels /*[B,N,4,5]*/);
int mcr_set_env_state(mcr_env* h, const double* reward /*[B,N]*/, const double* t /*[B]*/, const uint16_t* tile_flags /*[B,MCR_TILE_CAP]*/);
/* Draw every env's observation NOW, from the state as it stands, into d_obs on `stream` (after the state setters, which draw nothing;
 * tests): the pending flag scans, one pass that rewrites every active env's view records and car polygons from the state arrays — the
 * score label's value is the current reward, the backwards flag the current driving_backward: the frame render("state_pixels") of the
 * reference would return now — and ONE main raster launch (csrc/k_view.h) over all envs, in the handle's observation format (RGB, or
 * GRAY with stack 1; d_obs [B,N] frames of mcr_obs_bytes_per_view).  An env that is not active keeps its frame.  Changes no state a step
 * reads (the next step rewrites the records) and is not part of a step: outside the step's streams, lists and graphs.
 * MCR_ERR_ARG for a NULL handle or buffer (checked before any HIP call).  MCR_ERR_STATE before the first mcr_reset, on a handle without
 * obs_enabled, with a stacked format (the ring's slots are the step's), inside a caller's stream capture.  Only enqueues: no synchronisation. */
int mcr_obs_now(mcr_env* h, uint8_t* d_obs, void* stream);
/* hull.position per car [B,N,2] f32 */
int mcr_get_positions(mcr_env* h, float* pos);
/* mass KATs: hull invMass, invI, localCenter.x, .y, wheel invMass, invI (host computation) */
void mcr_mass_props(float* out6);
/* the build's sinf/cosf spec evaluated on the host (tests compare with the device kernel's) */
void mcr_sincos_host(float a, float* s, float* c);
int mcr_sincos_device(mcr_env* h, const float* d_in, float* d_sin, float* d_cos, int n, void* stream);

/* ---- full state snapshot / restore of one env (differential tests, checkpoint/resume; SURVEY 8b "mcr_get_state /
 * mcr_set_state").  The blob holds everything the step path reads for env `env`: per-car f32/f64/u32 state (bodies, joint
 * impulses, sleep timers, wheel omega/phase, controls, rewards, episode return, limit states, on-road bits, tile-visit
 * counts, flags), the env record (t, TimeLimit counter, flags), per-tile touch/visit state, the car<->car manifold store
 * (warm-start impulses) and the CURRENT episode slot (track, quads, tile hulls, spawn poses).  Restoring a blob into any
 * env index of any handle with the same num_agents continues bit-identically.  Both calls synchronise the device. */
size_t mcr_state_blob_bytes(const mcr_env* h);
int mcr_get_state_blob(mcr_env* h, int env, void* blob_out);
int mcr_set_state_blob(mcr_env* h, int env, const void* blob);

/* ---- the same snapshots as BATCHED, stream-ordered device operations (planning with the simulator as the model: fork a
 * state into K candidates, roll them out, rewind; restore-to-state exploration; checkpoints of the envs).  One kernel
 * (csrc/k_envcopy.h), one workgroup per listed env.  The calls only enqueue on `stream` — the stepping stream — and never
 * synchronise; the pending flag scans of a phase-word step are launched in front, like for every reader / writer of env state.
 *   d_blobs     [n][mcr_state_blob_pitch] bytes of device memory, 16-byte aligned.  The first mcr_state_blob_bytes bytes of a
 *               row are exactly what mcr_get_state_blob writes, header (magic, N, flags word, total bytes) included; the
 *               bytes up to the pitch are zero.
 *   d_env_ids   [n] int32 on the device: the env of row i; NULL: envs 0 .. n-1.
 *   n           0 .. num_envs (0: MCR_OK, nothing is launched).
 * mcr_load_states / mcr_copy_states follow mcr_set_state_blob's rule: slot, staged_ready and consumed of the env record
 * stay the TARGET's, the episode image goes into the target's current slot, the staged slot and the install counters are
 * not touched (an env restored on an auto_reset handle continues with that handle's own next staged episode).  The next
 * step re-evaluates the touch verdicts and the contact list; if a state-vector buffer is set (mcr_set_state_obs) it is
 * rewritten behind the copy.  Observation buffers are not part of the state and are not redrawn: the next step draws them.
 * mcr_load_states SKIPS a row, leaving its env untouched, when the row's header is not this handle's (another build,
 * num_agents, skid_particles or fresh_world setting) or its id is outside 0 .. num_envs-1, and counts it with one atomic
 * add into *d_refused (int32 on the device, zeroed by the caller; may be NULL).  mcr_save_states writes a zero header —
 * a row mcr_load_states refuses — for an id out of range; mcr_copy_states skips a pair with such an id.
 * The caller's obligations, NOT checked: destination ids are distinct, and in mcr_copy_states (env d_dst_ids[i] becomes a
 * copy of env d_src_ids[i]; a source may be listed many times) disjoint from the sources — a violation is a data race
 * between workgroups with an unspecified result.
 * MCR_ERR_ARG: NULL handle or buffer, misaligned d_blobs, n out of range.  MCR_ERR_STATE: save / copy before the first
 * reset; any of the three inside a caller's stream capture. */
size_t mcr_state_blob_pitch(const mcr_env* h);   /* mcr_state_blob_bytes rounded up to 16; 0 for NULL */
/* the four header words a blob of this handle starts with (what mcr_load_states compares) */
int mcr_state_blob_header(const mcr_env* h, uint32_t* out4);
int mcr_save_states(mcr_env* h, const int32_t* d_env_ids, int n, void* d_blobs, void* stream);
int mcr_load_states(mcr_env* h, const int32_t* d_env_ids, int n, const void* d_blobs, int32_t* d_refused, void* stream);
int mcr_copy_states(mcr_env* h, const int32_t* d_src_ids, const int32_t* d_dst_ids, int n, void* stream);

/* ---- synthetic workload (bench.py, tests): counter-based action stream, action of (global env, agent) at step t is a
 * pure function of (seed, env_offset + env, agent, t): steer ~ U(-1,1), gas ~ U(0,1), brake ~ U(0,1) (the action_space
 * bounds, multi_car_racing.py:162-165).  Device version writes d_actions [B,N,3] f32 on `stream`; the host twin produces
 * the same values for the CPU baseline. */
int mcr_synth_actions(mcr_env* h, float* d_actions, uint64_t seed, uint32_t t, uint32_t env_offset, void* stream);
/* the same stream for steps t0 .. t0 + nsteps - 1 in one launch: d_actions [nsteps][num_envs][num_agents][3] */
int mcr_synth_actions_block(mcr_env* h, float* d_actions, uint64_t seed, uint32_t t0, int nsteps, uint32_t env_offset, void* stream);
void mcr_synth_actions_host(float* out, int num_envs, int num_agents, uint64_t seed, uint32_t t, uint32_t env_offset);

/* ---- instrumentation for bench.py: HIP-event timing of the kernels enqueued by mcr_step, recorded on the
 * launch stream.  `mask` bit k enables timing slot k: 0 collide, 1 dynamics, 2 view, 3/4 = collide/dynamics of
 * the auto-reset pass, 5/6 = dynamics/view of the contact side stream, 7 = its reset pass (255 = all, 0 = off).
 * mcr_timing_read synchronises the device and drains accumulated milliseconds + launch counts. */
int mcr_timing_enable(mcr_env* h, int mask);
/* Debug switches, 0 in production; some make the results WRONG on purpose.  Bits 5-20: enum McrDebugBit in
 * multi_car_racing_amd/csrc/mcr_kernels.h is the one table (what each bit does, who reads it, whether results change).
 * Bits 0-4 are ablations of the raster (results WRONG): 0 skip flags block, 1 skip road shading, 2 skip cars, 3 skip write-out, 4 skip binning/cull. */
int mcr_debug_set(mcr_env* h, int value);
/* debug bit 5 (32): the raster kernel stamps s_memtime per phase; read the 64-float tail of a view's scratch */
int mcr_debug_read_view_scratch(mcr_env* h, int view, void* out, int nbytes);
/* debug bit 8 (256): k_dynamics stamps the clock per phase, [2 roles][blocks][8]; read n_u64 words of it */
int mcr_debug_read_dynamics_stamps(mcr_env* h, uint64_t* out, int n_u64);
/* cumulative diagnostics of the multi-stream step: [0] envs deferred by the main dynamics launch, [1] envs resumed,
 * [2] contact envs routed to the side stream, [3] env-steps frozen because the host had not staged the next episode yet
 * (a healthy rollout keeps this at 0) */
int mcr_debug_read_counters(mcr_env* h, uint64_t* out4);
/* all eight: [4] touch-verdict mismatches, [5] waits given up, [6] the last mismatch (env | manifolds << 20 | verdict << 28 | role << 32 | episode step << 36), [7] its step counter */
int mcr_debug_read_counters8(mcr_env* h, uint64_t* out8);
/* the three-chain step decides one step ahead which envs hold a touching car<->car pair (the main dynamics launch runs
 * beside the contact pass); the contact pass counts the envs where it disagrees: must stay 0 */
int mcr_debug_read_verdict_mismatches(mcr_env* h, uint64_t* out1);
/* 1: the three-chain step runs the contact pass beside the main dynamics (mcr_create found that kernels of different streams
 * overlap in this process); 0: it runs first (single stream, profilers that serialise kernels, MCR_SEQUENTIAL_COLLIDE=1) */
int mcr_concurrent_collide(const mcr_env* h);
/* How the streams of the three-chain step are ordered (bit mask; 0 for a single-stream handle):
 *   1  phase words in device memory, posted and awaited by kernels (no marker / barrier packets; needs overlapping kernels, like
 *      the concurrent contact pass; MCR_SOFT_SYNC=0 turns it off) — for steps launched on a caller stream that mcr_bind_stream
 *      accepted; on any other stream, and without this bit: events;
 *   2  on the event path, events are completed by the launches they mark (hipExtLaunchKernelGGL) rather than recorded behind them;
 *      always set for a three-chain handle (inside a graph capture the events are recorded behind the kernels);
 *   4  kernels do overlap here, but the internal streams of this handle share a hardware queue with those of another live phase-word
 *      handle of this process (probed pairwise at mcr_create; HIP spreads the streams of a priority class over GPU_MAX_HW_QUEUES queues,
 *      4 by default): this handle runs on events (same results, ~0.02 ms more per step).  Handles whose streams have queues of their own
 *      all keep bit 1.
 * A wait that gave up (status word 0) puts the handle on the event path for the rest of its life.
 * gfx950-specific: a phase word is posted with a RELAXED agent-scope store behind the end-of-kernel write-back of the kernels it
 * follows and polled with RELAXED agent-scope loads (sc1 accesses, served by the memory side — the device's coherence point); the
 * release / acquire pair the HIP memory model asks for between kernels of different streams costs +12 us per step (measured) and
 * is not used.  The event path makes no such assumption. */
int mcr_step_ordering(const mcr_env* h);
/* The same mask for steps launched on caller stream `stream`: bit 0 only if mcr_bind_stream accepted that stream (a stream that was never
 * bound, or that the check rejected, steps on events whatever the handle could do). */
int mcr_step_ordering_for(const mcr_env* h, void* stream);
/* Check ONCE whether steps launched on caller stream `stream` may use the phase-word ordering: two probe kernels and device
 * synchronisations (~1 ms).  Call it when a stream is first used with the handle (VecMultiCarRacing.step does); mcr_step itself never
 * synchronises: a step on a stream that was not bound, or that the check rejected, orders the internal streams with events. */
int mcr_bind_stream(mcr_env* h, void* stream);
/* the per-env records (mcr_common.h: McrEnvState, 48 bytes each: t f64, then steps, slot, staged_ready, consumed, active, resetting, just_reset,
 * frozen as i32, touch_blocks, bp_step as u32) of the first n_bytes / 48 envs; synchronises.  Diagnostics of the auto-reset's staging protocol. */
int mcr_debug_read_env_records(mcr_env* h, void* out, int n_bytes);
/* the last step's contact partition (three-chain step): part_out[B] = the touch verdicts it went by, clist_out[1 + B] = its contact list (count, env ids); synchronises */
int mcr_debug_read_partition(mcr_env* h, uint8_t* part_out, int32_t* clist_out);
/* out NULL: fill the verdict buffer the next step WRITES with fill_value; out != NULL (after that step): read it back [B].  Synchronises. */
int mcr_debug_next_verdicts(mcr_env* h, int fill_value, uint8_t* out_or_null);
/* number of touching car<->car fixture pairs (stored manifolds) per env after the last collide pass */
int mcr_debug_read_contact_counts(mcr_env* h, int32_t* out /*[num_envs]*/);
/* the raw manifold stores of all envs after the last step (mcr_contact_store_words: the sizes; csrc/k_carcontacts.h: the record layout);
 * synchronises.  The input of the car-contact observation's host reference. */
int mcr_debug_read_contacts(mcr_env* h, uint32_t* out /*[num_envs][words per env]*/);
/* the wheel<->tile sensor pass's per-tile state after the last step (csrc/k_collide.h): out[env][tile] bit car * 4 + wheel = that wheel rests on
 * the tile (the reference's `tile in wheel.tiles`); tiles at and beyond the episode's count are not meaningful.  Read-only; synchronises. */
int mcr_debug_read_tile_touch(mcr_env* h, uint32_t* out /*[num_envs][MCR_TILE_CAP]*/);
/* fresh_world = 0: the broadphase proxy ids of env `env`'s live episode on its one world (csrc/k_world.h) — out[0 .. T) tiles in track order,
 * then num_agents * 8 car fixtures (car * 8 + fixture; 0..3 hull polygons, 4..7 wheels); returns the count written; synchronises.  Tests
 * hold it against the oracle's literal b2DynamicTree (what mcr_world_proxy_ids is for the host-side twin). */
int mcr_debug_read_proxy_ids(mcr_env* h, int env, int32_t* out, int cap);
/* Conditions reported by the kernels in mapped host memory (counted on the device, stored with system scope: no PCIe atomics needed),
 * read by mcr_step without synchronising (a condition raised by a step still in flight surfaces one call later).  Words:
 * [0] a bounded in-kernel wait gave up (the main dynamics for the contact pass of an env, any kernel for a phase word),
 * [1] contact pass vs one-step-ahead touch verdict mismatches — FATAL: the next mcr_step returns MCR_ERR_STATE once per change (the
 *     handle then runs the contact pass in front of the dynamics and orders its streams with events);
 * [2] car<->car manifold store / LDS pool overflows, [3] tile begin-event queue overflows — DEGRADED: a documented capacity was
 *     exceeded and the excess dropped (that env's contacts / tile events of that step are incomplete); [4] envs that FROZE: their episode
 *     ended before the host had staged the next one (zero outputs until it arrives; stage earlier).  The rollout goes on, the counts are
 *     visible here; VecMultiCarRacing.step turns every change of [2..4] into an McrWarning.
 * mcr_status copies the cumulative counts (n_words <= 8). */
int mcr_status(mcr_env* h, uint32_t* out, int n_words);
/* The sensor predicate of the contact pass (Box2D's b2TestOverlap: GJK b2Distance behind mcr.py:428 -> b2Contact::Update) on
 * caller-supplied cases, for differential tests: case i = a tile given by its 4 points quads[i][8] (host, f32; the hull is
 * built as the episode generator builds it) against car fixture `fixture` (0..3 hull polygons, 4 the wheel box) of a body
 * whose origin and angle are poses[i][3]; out[i] = touching (host).  fixture + 8: the car fixture is fixtureA (b2TestOverlap(fixture, tile):
 * what a world that lives across reset() can ask for, mcr_world above).  Synchronous. */
int mcr_debug_overlap(mcr_env* h, int n, const float* quads, const float* poses, int fixture, uint8_t* out);
/* The step tail's launch of the per-level statistics kernel (mcr_set_level_stats above: definition and arithmetic contract) on
 * caller-supplied rows, for differential tests: the same launch function, hence the same grid, block size and argument order, fed with the
 * caller's device buffers instead of a handle's — d_done [num_envs] u8 (non-zero: the env ended), d_trunc [num_envs] u8 (may be NULL:
 * nothing truncated), d_ep_return [num_envs][num_agents] f64, d_ep_len and d_level [num_envs] int32, K levels.  Rewrites d_finished
 * [num_envs] and adds to d_stats [K + 1][3 + 2 num_agents]; every buffer naturally aligned, nothing more (16-byte aligned ones take the
 * vector loads).  Takes no handle.  MCR_ERR_ARG, before any HIP call: a NULL required pointer, num_envs < 1, num_agents outside 1..8,
 * K < 1.  Otherwise one launch on `stream`, no synchronisation. */
int mcr_debug_level_stats(const uint8_t* d_done, const uint8_t* d_trunc /* may be NULL */,
                          const double* d_ep_return /* [num_envs][num_agents] */, const int32_t* d_ep_len,
                          const int32_t* d_level, int num_envs, int num_agents, int K,
                          int32_t* d_finished /* [num_envs] */, double* d_stats /* [K+1][3+2N] */, void* stream);
/* The step's launch of the car-contact observation kernel (mcr_set_contact_obs above) on caller-made stores, for differential tests: the same
 * launch function, hence the same grid and block size, fed with the caller's device buffers — d_store [num_envs][words per env] u32 — and
 * no env records (every env is live).  accumulate != 0: continue from the contents of d_mask / d_impulse.  Buffers naturally aligned,
 * nothing more.  Takes no handle.  MCR_ERR_ARG, before any HIP call: a NULL pointer, num_envs < 1, num_agents outside 2..8.  Otherwise one
 * launch on `stream`, no synchronisation. */
int mcr_debug_contact_obs(const uint32_t* d_store, int num_envs, int num_agents, int accumulate,
                          int32_t* d_mask /* [num_envs][N] */, double* d_impulse /* [num_envs][N][N] */, void* stream);
#define MCR_TIMING_SLOTS 8
int mcr_timing_read(mcr_env* h, double* ms_out /*[MCR_TIMING_SLOTS]*/, int64_t* launches_out /*[MCR_TIMING_SLOTS]*/);

#ifdef __cplusplus
}
#endif
#endif /* MCR_H */
