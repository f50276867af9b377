// mcr_derived.hip — what the C ABI (include/mcr.h) DERIVES from the state a reset / a restore / a step ended with: the state vector (k_stateobs.h),
// the range finder (k_rangeobs.h), the grid (k_gridobs.h), scripted drivers (k_driver.h), level pools (k_pool.h), car contacts (k_contactobs.h),
// early episode ending (k_endrules.h).  Launched from mcr_hip.hip / mcr_state.hip: mcr_env.h.
#include "mcr_env.h"
#include "k_stateobs.h"
#include "k_rangeobs.h"
#include "k_gridobs.h"
#include "k_driver.h"
#include "k_pool.h"
#include "k_levelstats.h"
#include "k_contactobs.h"
#include "k_endrules.h"
#include <cmath>

// The low-dimensional observation of the state a reset / a step ended with (k_stateobs.h), a wavefront per env on the caller's stream: behind
// launch_reset / launch_step (whose tail makes `st` wait for the whole step), outside the step's streams and outside a replayed step graph.
// It reads no flags: nothing is flushed.  Off (no buffer): one test.  The range-finder observation (k_rangeobs.h) goes wherever it goes, for
// the same reasons, behind it: launch_derived is what mcr_reset, the step's tail and a restore / clone (mcr_state.hip) call.
static void launch_state_obs(mcr_env* h, hipStream_t st) {
  if (!h->so.out) return;
  hipLaunchKernelGGL(k_stateobs, dim3(h->P.B), dim3(64), 0, st, h->P, h->so);
}
static void launch_range_obs(mcr_env* h, hipStream_t st) {
  if (!h->ro.out) return;
  hipLaunchKernelGGL(k_rangeobs, dim3(h->P.B), dim3(64), 0, st, h->P, h->ro);
}
// The car-contact observation (k_contactobs.h): a wavefront per env over the manifold store as the last step left it.  run_contact_obs is THE
// launch — grid, block size, argument order — on plain device pointers: launch_contact_obs hands it the handle's, mcr_debug_contact_obs the
// caller's (what tests/test_gpu_contact_obs_kernel.py runs is this geometry, not a copy of it).  On the caller's stream behind launch_step, like
// k_stateobs, outside the step's streams and outside a replayed step graph; it reads neither CU_FLAGS nor anything k_flags writes: no flush.
// Nobody rewrites the store before it has run: the next step's contact pass starts behind something that step enqueues on the caller's
// stream (its own launch there, W_BEGIN's post by its main dynamics, the fork event), hence behind this kernel (k_contactobs.h: Ordering).
static void run_contact_obs(hipStream_t st, const uint32_t* d_store, const McrEnvState* d_env, int B, int N, bool accumulate, int32_t* d_mask, double* d_impulse) {
  const int per_group = MCR_CO_LANES / 64;
  hipLaunchKernelGGL(k_contactobs, dim3((B + per_group - 1) / per_group), dim3(MCR_CO_LANES), 0, st, d_store, d_env, B, N, accumulate ? 1 : 0,
                     McrContactObs{d_mask, d_impulse});
}
void launch_contact_obs(mcr_env* h, hipStream_t st, bool accumulate) {
  if (!h->co.mask) return;
  run_contact_obs(st, h->P.cc_store, h->P.env, h->P.B, h->P.N, accumulate, h->co.mask, h->co.impulse);
}
// The grid observation (k_gridobs.h) goes wherever the range finder goes, behind it: a wavefront per view on the caller's stream.  It reads
// tile_flags, which k_collide alone writes — inside the step, behind whose tail `st` waits; the k_flags launch a phase-word step leaves
// pending writes CU_FLAGS only: no flush_flags.  Off (no buffer): one test.
static void launch_grid_obs(mcr_env* h, hipStream_t st) {
  if (!h->go.out) return;
  hipLaunchKernelGGL(k_gridobs, dim3(h->P.B * h->P.N), dim3(64), 0, st, h->P, h->go);
}
// (the step's tail takes the first three only: step_one has launched the contact observation behind every sub-step, mcr_env.h)
static void launch_state_range(mcr_env* h, hipStream_t st) { launch_state_obs(h, st); launch_range_obs(h, st); launch_grid_obs(h, st); }
// Early episode ending (k_endrules.h): a lane per env on the caller's stream, where launch_contact_obs goes and for its reasons — behind
// launch_step, outside the step's streams and outside a replayed step graph; it reads the env record, CU_TVC and CU_ONROAD, none of which
// k_flags writes: no flush.  The next step's dynamics, whichever chain, loads armed[] behind this kernel (k_endrules.h: Ordering).  Off: one test.
static void run_end_rules(mcr_env* h, hipStream_t st, int pass) {
  if (!h->er.counters) return;
  hipLaunchKernelGGL(k_endrules, dim3((h->P.B + MCR_ER_LANES - 1) / MCR_ER_LANES), dim3(MCR_ER_LANES), 0, st, (const McrEnvState*)h->P.env, (const uint32_t*)h->P.caru,
                     h->P.B, h->P.N, pass, h->er);
}
void launch_end_rules(mcr_env* h, hipStream_t st, bool accumulate) { run_end_rules(h, st, accumulate ? MCR_ER_ADVANCE_ACCUMULATE : MCR_ER_ADVANCE); }
void launch_derived(mcr_env* h, hipStream_t st) { launch_state_range(h, st); launch_contact_obs(h, st, false); run_end_rules(h, st, MCR_ER_SETTLE); }

// Level pools (k_pool.h): every env that installed its staged episode gets its next one from the pool.  Launched where launch_state_obs goes — on
// the caller's stream in front of and behind launch_reset and behind the LAST sub-step of a macro-step (a parked env re-spawns only there), whose
// tail makes `st` wait for the whole step, outside the step's streams and outside a replayed step graph.  Behind the step's tail the terminal
// frames (mcr_set_terminal_obs), which read the slot an env just left — the slot this kernel overwrites —, are drawn.  No flush_flags: the
// scans a phase-word step left pending (k_flags.h) read an env's record and its CURRENT slot, and return at once for an env that just
// re-spawned; the kernel writes staged slots and `staged_ready`, which the scans load with the record and never look at — and they are
// launched by the NEXT step, behind this kernel in stream order (W_BEGIN is posted by that step's dynamics on `st`).
void launch_pool_restage(mcr_env* h, hipStream_t st, int envs_per_group) {
  if (!h->pool.blobs) return;
  const int B = h->P.B;
  hipLaunchKernelGGL(k_pool_restage, dim3((B + envs_per_group - 1) / envs_per_group), dim3(MCR_POOL_LANES), 0, st, h->P.env, h->P.slots, B, h->pool, envs_per_group);
}
// Per-level episode statistics (k_levelstats.h): one launch, a wavefront per stats row, from the done / truncated rows the step just wrote.  It
// reads level[] and must see the rows of the episodes that ENDED: in front of the re-stage, which hands an env that installed its next
// episode that episode's row.  Behind the last sub-step of a macro-step only, like everything here: once per step call.
// launch_level_stats is THE launch — grid, block size, argument order — on plain device pointers: the step tail hands it the handle's, and
// mcr_debug_level_stats the caller's (what tests/test_gpu_level_stats_kernel.py runs is this geometry, not a copy of it).
static void launch_level_stats(hipStream_t st, const uint8_t* d_done, const uint8_t* d_trunc, const double* d_ep_return, const int32_t* d_ep_len,
                               const int32_t* d_level, int B, int N, int K, int32_t* d_finished, double* d_stats) {
  const int waves = K + 1, per_group = MCR_LS_LANES / 64;
  hipLaunchKernelGGL(k_levelstats, dim3((waves + per_group - 1) / per_group), dim3(MCR_LS_LANES), 0, st, McrLevelStats{d_finished, d_stats}, d_done, d_trunc,
                     d_ep_return, d_ep_len, d_level, B, N, K);
}
void launch_step_tail(mcr_env* h, hipStream_t st, const uint8_t* d_done, const uint8_t* d_trunc) {
  launch_state_range(h, st);
  if (h->ls.stats)
    launch_level_stats(st, d_done, d_trunc, (const double*)h->P.ep_return_out, (const int32_t*)h->P.ep_len_out, (const int32_t*)h->pool.level,
                       h->P.B, h->P.N, h->pool.K, h->ls.finished, h->ls.stats);
  launch_pool_restage(h, st, MCR_POOL_GROUP);
}

extern "C" int mcr_state_obs_dim(int num_agents, int waypoints) {
  if (num_agents < 1 || num_agents > MCR_MAX_AGENTS || waypoints < 0 || waypoints > MCR_SO_WAYPOINTS_MAX) { g_err = "mcr_state_obs_dim: num_agents 1..8, waypoints 0..16"; return MCR_ERR_ARG; }
  return mcr_so_dim(num_agents, waypoints);
}
extern "C" int mcr_set_state_obs(mcr_env* h, float* d_state, int waypoints, int stride) {
  if (!h) { g_err = "null handle"; return MCR_ERR_ARG; }
  if (waypoints < 0 || waypoints > MCR_SO_WAYPOINTS_MAX || stride < 1 || stride > MCR_SO_STRIDE_MAX) { g_err = "mcr_set_state_obs: waypoints 0..16, stride 1..64"; return MCR_ERR_ARG; }
  h->so.out = d_state; h->so.K = waypoints; h->so.stride = stride; h->so.F = mcr_so_dim(h->P.N, waypoints);
  return MCR_OK;
}
extern "C" int mcr_state_obs_now(mcr_env* h, void* stream) {
  if (!h) { g_err = "null handle"; return MCR_ERR_ARG; }
  if (!h->so.out) { g_err = "mcr_state_obs_now: no buffer set (mcr_set_state_obs)"; return MCR_ERR_STATE; }
  launch_state_obs(h, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MCR_OK;
}

// The range-finder observation (k_rangeobs.h).  mcr_set_range_obs only validates and stores: no HIP call, no device needed for its argument checks.
extern "C" int mcr_check_range_obs(const float* dirs, int rays, float max_range) {
  if (rays < 1 || rays > MCR_RANGE_RAYS_MAX) { g_err = "range_obs: rays 1..32"; return MCR_ERR_ARG; }
  if (!dirs) { g_err = "range_obs: null direction table"; return MCR_ERR_ARG; }
  for (int i = 0; i < 2 * rays; ++i) if (!std::isfinite(dirs[i])) { g_err = "range_obs: a direction is not finite"; return MCR_ERR_ARG; }
  if (!std::isfinite(max_range) || !(max_range > 0.0f)) { g_err = "range_obs: max_range must be finite and > 0"; return MCR_ERR_ARG; }
  return MCR_OK;
}
extern "C" int mcr_set_range_obs(mcr_env* h, float* d_ranges, const float* dirs, int rays, float max_range) {
  if (!h) { g_err = "null handle"; return MCR_ERR_ARG; }
  if (!d_ranges) { h->ro.out = nullptr; return MCR_OK; }
  if (int rc = mcr_check_range_obs(dirs, rays, max_range)) return rc;
  McrRangeObs ro{};
  double umax = 0.0;
  for (int k = 0; k < rays; ++k) {
    ro.dir[k][0] = dirs[2 * k]; ro.dir[k][1] = dirs[2 * k + 1];
    umax = fmax(umax, sqrt((double)dirs[2 * k] * (double)dirs[2 * k] + (double)dirs[2 * k + 1] * (double)dirs[2 * k + 1]));
  }
  ro.out = d_ranges; ro.R = rays; ro.max_range = max_range;
  ro.cull = (double)max_range * umax * (1.0 + 1e-6) + 1e-2;
  h->ro = ro;
  return MCR_OK;
}
extern "C" int mcr_range_obs_now(mcr_env* h, void* stream) {
  if (!h) { g_err = "null handle"; return MCR_ERR_ARG; }
  if (!h->ro.out) { g_err = "mcr_range_obs_now: no buffer set (mcr_set_range_obs)"; return MCR_ERR_STATE; }
  launch_range_obs(h, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MCR_OK;
}
// The grid observation (k_gridobs.h).  mcr_set_grid_obs only validates and stores: no HIP call, no device needed for its argument checks.
extern "C" int mcr_check_grid_obs(int rows, int cols, float cell, float origin_row, float origin_col) {
  if (rows < 1 || rows > MCR_GRID_MAX || cols < 1 || cols > MCR_GRID_MAX) { g_err = "grid_obs: rows, cols 1..64"; return MCR_ERR_ARG; }
  if (!std::isfinite(cell) || !(cell > 0.0f)) { g_err = "grid_obs: cell must be finite and > 0"; return MCR_ERR_ARG; }
  if (!std::isfinite(origin_row) || !std::isfinite(origin_col)) { g_err = "grid_obs: the origin is not finite"; return MCR_ERR_ARG; }
  return MCR_OK;
}
extern "C" int mcr_set_grid_obs(mcr_env* h, uint8_t* d_grid, int rows, int cols, float cell, float origin_row, float origin_col) {
  if (!h) { g_err = "null handle"; return MCR_ERR_ARG; }
  if (!d_grid) { h->go.out = nullptr; return MCR_OK; }
  if (int rc = mcr_check_grid_obs(rows, cols, cell, origin_row, origin_col)) return rc;
  h->go = McrGridObs{d_grid, rows, cols, cell, origin_row, origin_col};
  return MCR_OK;
}
extern "C" int mcr_grid_obs_now(mcr_env* h, void* stream) {
  if (!h) { g_err = "null handle"; return MCR_ERR_ARG; }
  if (!h->go.out) { g_err = "mcr_grid_obs_now: no buffer set (mcr_set_grid_obs)"; return MCR_ERR_STATE; }
  launch_grid_obs(h, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MCR_OK;
}
// the four hull fixture polygons as the kernels hold them (McrShapes::hull): out [4][8][2] f32 body-frame vertices, counts [4]; no handle, no GPU needed
extern "C" int mcr_hull_polygons(float* out, int32_t* counts) {
  if (!out || !counts) { g_err = "null argument"; return MCR_ERR_ARG; }
  McrShapes S; mcr_build_shapes(&S);
  for (int k = 0; k < 4; ++k) {
    counts[k] = S.hull[k].n;
    for (int i = 0; i < 8; ++i) { out[(k * 8 + i) * 2] = S.hull[k].vx[i]; out[(k * 8 + i) * 2 + 1] = S.hull[k].vy[i]; }
  }
  return MCR_OK;
}

// The car-contact observation (k_contactobs.h).  mcr_set_contact_obs only validates and stores: no HIP call; the pairing of the two pointers is
// checked in front of the handle, so that it can be tested without a device.
extern "C" int mcr_set_contact_obs(mcr_env* h, int32_t* d_mask, double* d_impulse) {
  if ((d_mask == nullptr) != (d_impulse == nullptr)) { g_err = "mcr_set_contact_obs: the mask and the impulse buffer are set together or not at all (exactly one is null)"; return MCR_ERR_ARG; }
  if (!h) { g_err = "null handle"; return MCR_ERR_ARG; }
  if (!d_mask) { h->co = McrContactObs{nullptr, nullptr}; return MCR_OK; }
  if (h->P.N < 2) { g_err = "mcr_set_contact_obs: needs num_agents >= 2"; return MCR_ERR_ARG; }
  if (!h->P.car_contacts) { g_err = "mcr_set_contact_obs: the handle was created with car_contacts = 0 (no manifold store is kept)"; return MCR_ERR_ARG; }
  h->co = McrContactObs{d_mask, d_impulse};
  return MCR_OK;
}
extern "C" int mcr_contact_obs_now(mcr_env* h, void* stream) {
  if (!h) { g_err = "null handle"; return MCR_ERR_ARG; }
  if (!h->co.mask) { g_err = "mcr_contact_obs_now: no buffers set (mcr_set_contact_obs)"; return MCR_ERR_STATE; }
  launch_contact_obs(h, (hipStream_t)stream, false);
  HIPCHK(hipGetLastError());
  return MCR_OK;
}
// Early episode ending (k_endrules.h).  mcr_set_end_rules only validates and stores: no HIP call; everything that does not need the handle's
// num_agents is checked in front of the handle, so that it can be tested without a device (mcr_check_end_rules: all of it, for a given N).
static int end_rules_values(int patience, int offroad_patience, int offroad_mode, double end_reward) {
  if (patience < 0 || offroad_patience < 0) { g_err = "end_rules: patience and offroad_patience must be >= 0 (0: the rule is off)"; return MCR_ERR_ARG; }
  if (patience == 0 && offroad_patience == 0) { g_err = "end_rules: both patiences are 0 (no rule to count for; pass null buffers to turn the feature off)"; return MCR_ERR_ARG; }
  if (offroad_mode != 0 && offroad_mode != 1) { g_err = "end_rules: offroad_mode 0 (all counted cars off the road) or 1 (any)"; return MCR_ERR_ARG; }
  if (!std::isfinite(end_reward)) { g_err = "end_rules: end_reward is not finite"; return MCR_ERR_ARG; }
  return MCR_OK;
}
extern "C" int mcr_check_end_rules(int num_agents, int patience, int offroad_patience, int offroad_mode, uint32_t agent_mask, double end_reward) {
  if (num_agents < 1 || num_agents > MCR_MAX_AGENTS) { g_err = "end_rules: num_agents 1..8"; return MCR_ERR_ARG; }
  if (int rc = end_rules_values(patience, offroad_patience, offroad_mode, end_reward)) return rc;
  if (!(agent_mask & ((1u << num_agents) - 1u))) { g_err = "end_rules: agent_mask names no car below num_agents"; return MCR_ERR_ARG; }
  return MCR_OK;
}
extern "C" int mcr_set_end_rules(mcr_env* h, int patience, int offroad_patience, int offroad_mode, uint32_t agent_mask, double end_reward,
                                 int32_t* d_counters, uint8_t* d_armed, uint8_t* d_reason) {
  const int given = (d_counters != nullptr) + (d_armed != nullptr) + (d_reason != nullptr);
  if (given != 0 && given != 3) { g_err = "mcr_set_end_rules: the counters, the armed and the reason buffer are set together or not at all"; return MCR_ERR_ARG; }
  if (given) {
    if (int rc = end_rules_values(patience, offroad_patience, offroad_mode, end_reward)) return rc;
    if ((uintptr_t)d_counters & 15u) { g_err = "mcr_set_end_rules: the counters buffer must be 16-byte aligned (one row is one 16-byte access)"; return MCR_ERR_ARG; }
  }
  if (!h) { g_err = "null handle"; return MCR_ERR_ARG; }
  if (!given) { h->er = McrEndRules{}; h->P.end_armed = nullptr; h->P.end_reward = 0.0; return MCR_OK; }
  if (int rc = mcr_check_end_rules(h->P.N, patience, offroad_patience, offroad_mode, agent_mask, end_reward)) return rc;
  h->er = McrEndRules{d_counters, d_armed, d_reason, patience, offroad_patience, offroad_mode, agent_mask & ((1u << h->P.N) - 1u)};
  h->P.end_armed = d_armed; h->P.end_reward = end_reward;
  return MCR_OK;
}
extern "C" int mcr_end_rules_now(mcr_env* h, void* stream) {
  if (!h) { g_err = "null handle"; return MCR_ERR_ARG; }
  if (!h->er.counters) { g_err = "mcr_end_rules_now: no buffers set (mcr_set_end_rules)"; return MCR_ERR_STATE; }
  run_end_rules(h, (hipStream_t)stream, MCR_ER_SETTLE);
  HIPCHK(hipGetLastError());
  return MCR_OK;
}
extern "C" int mcr_contact_store_words(int32_t* words_per_env, int32_t* words_per_record) {
  if (words_per_env) *words_per_env = MCR_CC_STORE_WORDS;
  if (words_per_record) *words_per_record = MCR_CC_WORDS;
  return MCR_CC_MAX;
}
// the step's launch on caller-made stores: no handle (every env is live), the argument checks in front of any HIP call, one launch, no synchronisation
extern "C" int mcr_debug_contact_obs(const uint32_t* d_store, int num_envs, int num_agents, int accumulate, int32_t* d_mask, double* d_impulse, void* stream) {
  if (!d_store || !d_mask || !d_impulse) { g_err = "mcr_debug_contact_obs: null argument"; return MCR_ERR_ARG; }
  if (num_envs < 1 || num_agents < 2 || num_agents > MCR_MAX_AGENTS) { g_err = "mcr_debug_contact_obs: num_envs >= 1, num_agents 2..8"; return MCR_ERR_ARG; }
  run_contact_obs((hipStream_t)stream, d_store, nullptr, num_envs, num_agents, accumulate != 0, d_mask, d_impulse);
  HIPCHK(hipGetLastError());
  return MCR_OK;
}

// The scripted driver (k_driver.h).  mcr_set_drivers only validates and stores: no HIP call, no device needed for its argument checks.
static const float MCR_DRV_DEFAULT_ROW[MCR_DRV_PARAMS] = MCR_DRV_DEFAULTS;
static const char* drv_check_row(const float* q) {
  for (int j = 0; j < MCR_DRV_PARAMS; ++j) if (!std::isfinite(q[j])) return "a parameter is not finite";
  for (int j = 0; j < 2; ++j) if (q[j] < 1.0f || q[j] > (float)MCR_DRV_LOOKAHEAD_MAX || q[j] != (float)(int)q[j]) return "L1, L2 must be integers 1..64";
  if (!(q[2] > 0.0f)) return "v_max must be > 0";
  for (int j = 3; j <= 6; ++j) if (q[j] < 0.0f) return "K_s, K_c, K_g, K_b must be >= 0";
  for (int j = 8; j <= 9; ++j) if (q[j] < 0.0f || q[j] > 1.0f) return "gas_max, brake_max must be in [0, 1]";
  return nullptr;
}
extern "C" int mcr_driver_defaults(float* out) {
  if (!out) { g_err = "null argument"; return MCR_ERR_ARG; }
  for (int j = 0; j < MCR_DRV_PARAMS; ++j) out[j] = MCR_DRV_DEFAULT_ROW[j];
  return MCR_OK;
}
extern "C" int mcr_check_drivers(int num_agents, const float* params, uint32_t agent_mask) {
  if (num_agents < 1 || num_agents > MCR_MAX_AGENTS) { g_err = "drivers: num_agents 1..8"; return MCR_ERR_ARG; }
  if (!params) { g_err = "drivers: null parameter rows"; return MCR_ERR_ARG; }
  if (agent_mask >> num_agents) { g_err = "drivers: agent_mask has bits of cars >= num_agents"; return MCR_ERR_ARG; }
  for (int a = 0; a < num_agents; ++a)
    if (const char* why = drv_check_row(params + (size_t)a * MCR_DRV_PARAMS)) { g_err = "drivers: car " + std::to_string(a) + ": " + why; return MCR_ERR_ARG; }
  return MCR_OK;
}
extern "C" int mcr_set_drivers(mcr_env* h, const float* params, uint32_t agent_mask, float* d_actions) {
  if (!h) { g_err = "null handle"; return MCR_ERR_ARG; }
  if (!d_actions) { g_err = "mcr_set_drivers: null action buffer"; return MCR_ERR_ARG; }
  if (int rc = mcr_check_drivers(h->P.N, params, agent_mask)) return rc;
  for (int a = 0; a < MCR_MAX_AGENTS; ++a)
    for (int j = 0; j < MCR_DRV_PARAMS; ++j) h->drv.prm[a][j] = a < h->P.N ? params[a * MCR_DRV_PARAMS + j] : MCR_DRV_DEFAULT_ROW[j];
  h->drv_out = d_actions; h->drv_mask = agent_mask;
  return MCR_OK;
}
// Racecraft (k_driver.h): rows and mask beside the driver's, validated and stored alike
static const float MCR_RC_DEFAULT_ROW[MCR_RC_PARAMS] = MCR_RC_DEFAULTS;
static const char* rc_check_row(const float* w) {
  for (int j = 0; j < MCR_RC_PARAMS; ++j) if (!std::isfinite(w[j])) return "a parameter is not finite";
  if (w[0] < 1.0f || w[0] > (float)MCR_DRV_LOOKAHEAD_MAX || w[0] != (float)(int)w[0]) return "look must be an integer 1..64";
  for (int j = 1; j < MCR_RC_PARAMS; ++j) if (w[j] < 0.0f) return "w_block, w_pass, off_max, d_safe, K_f, w_off, v_off must be >= 0";
  return nullptr;
}
extern "C" int mcr_racecraft_defaults(float* out) {
  if (!out) { g_err = "null argument"; return MCR_ERR_ARG; }
  for (int j = 0; j < MCR_RC_PARAMS; ++j) out[j] = MCR_RC_DEFAULT_ROW[j];
  return MCR_OK;
}
extern "C" int mcr_check_racecraft(int num_agents, const float* params, uint32_t agent_mask) {
  if (num_agents < 1 || num_agents > MCR_MAX_AGENTS) { g_err = "racecraft: num_agents 1..8"; return MCR_ERR_ARG; }
  if (!params) { g_err = "racecraft: null parameter rows"; return MCR_ERR_ARG; }
  if (agent_mask >> num_agents) { g_err = "racecraft: agent_mask has bits of cars >= num_agents"; return MCR_ERR_ARG; }
  for (int a = 0; a < num_agents; ++a)
    if (const char* why = rc_check_row(params + (size_t)a * MCR_RC_PARAMS)) { g_err = "racecraft: car " + std::to_string(a) + ": " + why; return MCR_ERR_ARG; }
  return MCR_OK;
}
extern "C" int mcr_set_racecraft(mcr_env* h, const float* params, uint32_t agent_mask) {
  if (!h) { g_err = "null handle"; return MCR_ERR_ARG; }
  if (!h->drv_out) { g_err = "mcr_set_racecraft: no drivers set (mcr_set_drivers)"; return MCR_ERR_STATE; }
  if (!params || !agent_mask) { h->drv.rc_mask = 0; return MCR_OK; }
  if (int rc = mcr_check_racecraft(h->P.N, params, agent_mask)) return rc;
  for (int a = 0; a < MCR_MAX_AGENTS; ++a)
    for (int j = 0; j < MCR_RC_PARAMS; ++j) h->drv.rc[a][j] = a < h->P.N ? params[a * MCR_RC_PARAMS + j] : MCR_RC_DEFAULT_ROW[j];
  h->drv.rc_mask = agent_mask;
  return MCR_OK;
}
extern "C" int mcr_driver_actions(mcr_env* h, const float* d_actions_in, uint32_t agent_mask_override, float* d_out, void* stream) {
  if (!h) { g_err = "null handle"; return MCR_ERR_ARG; }
  if (!h->drv_out) { g_err = "mcr_driver_actions: no drivers set (mcr_set_drivers)"; return MCR_ERR_STATE; }
  const uint32_t mask = agent_mask_override == 0xffffffffu ? (1u << h->P.N) - 1u : h->drv_mask;
  // (the extended kernel only where a car it drives races: a handle without racecraft launches the plain instantiation)
  if (mask & h->drv.rc_mask) hipLaunchKernelGGL(k_driver<true>, dim3(h->P.B), dim3(64), 0, (hipStream_t)stream, h->P, h->drv, d_actions_in, mask, d_out ? d_out : h->drv_out);
  else hipLaunchKernelGGL(k_driver<false>, dim3(h->P.B), dim3(64), 0, (hipStream_t)stream, h->P, h->drv, d_actions_in, mask, d_out ? d_out : h->drv_out);
  HIPCHK(hipGetLastError());
  return MCR_OK;
}

extern "C" int mcr_set_episode_pool(mcr_env* h, const void* d_pool, int K, uint64_t seed, uint32_t env_offset, int mode, int32_t* d_level) {
  if (!h || !d_pool) { g_err = "mcr_set_episode_pool: null argument"; return MCR_ERR_ARG; }
  if (K < 1 || ((uintptr_t)d_pool & 15u) || (mode != 0 && mode != 1)) { g_err = "mcr_set_episode_pool: K >= 1 rows, a 16-byte aligned pool, mode 0 (random) or 1 (cycle)"; return MCR_ERR_ARG; }
  // (the staged slots have ONE owner for the life of the handle: a pool set later would meet episodes the host staged and counters it polls)
  if (h->any_reset) { g_err = "mcr_set_episode_pool after the first mcr_reset"; return MCR_ERR_STATE; }
  if (h->svc) { g_err = "mcr_set_episode_pool: the refill service is running"; return MCR_ERR_STATE; }
  h->pool.blobs = (const uint8_t*)d_pool; h->pool.K = K; h->pool.mode = mode; h->pool.seed = seed; h->pool.env_offset = env_offset; h->pool.level = d_level;
  return MCR_OK;
}

// Weighted level sampling on a mode-0 pool (k_pool.h).  The uniform CDF goes into the caller's buffer with a blocking copy: set-up time, before the first reset.
extern "C" int mcr_set_level_sampler(mcr_env* h, double* d_cdf, int32_t* d_staged_level) {
  if (!h || !d_cdf || !d_staged_level) { g_err = "mcr_set_level_sampler: null argument"; return MCR_ERR_ARG; }
  if (!h->pool.blobs) { g_err = "mcr_set_level_sampler: no level pool (mcr_set_episode_pool)"; return MCR_ERR_STATE; }
  if (h->pool.mode != 0) { g_err = "mcr_set_level_sampler: the pool was created with mode 1 (cycle); weighted sampling replaces mode 0's hash"; return MCR_ERR_STATE; }
  if (h->any_reset) { g_err = "mcr_set_level_sampler after the first mcr_reset"; return MCR_ERR_STATE; }
  std::vector<double> uniform((size_t)h->pool.K);
  for (int j = 0; j < h->pool.K; ++j) uniform[j] = mcr_level_cdf_uniform(j, h->pool.K);
  HIPCHK(hipMemcpy(d_cdf, uniform.data(), uniform.size() * sizeof(double), hipMemcpyHostToDevice));
  h->pool.cdf = d_cdf; h->pool.staged_level = d_staged_level;
  return MCR_OK;
}
extern "C" int mcr_level_weights(mcr_env* h, const double* d_weights, int32_t* d_fell_back, void* stream) {
  if (!h || !d_weights) { g_err = "mcr_level_weights: null argument"; return MCR_ERR_ARG; }
  if (!h->pool.cdf) { g_err = "mcr_level_weights: no sampler set (mcr_set_level_sampler)"; return MCR_ERR_STATE; }
  hipLaunchKernelGGL(k_level_cdf, dim3(1), dim3(64), 0, (hipStream_t)stream, d_weights, const_cast<double*>(h->pool.cdf), h->pool.K, d_fell_back);
  HIPCHK(hipGetLastError());
  return MCR_OK;
}
extern "C" int mcr_level_stats_dim(int num_agents) {
  if (num_agents < 1 || num_agents > MCR_MAX_AGENTS) { g_err = "mcr_level_stats_dim: num_agents 1..8"; return MCR_ERR_ARG; }
  return MCR_LS_COLS(num_agents);
}
extern "C" int mcr_set_level_stats(mcr_env* h, int32_t* d_finished_level, double* d_stats) {
  if (!h) { g_err = "null handle"; return MCR_ERR_ARG; }
  if (!d_finished_level || !d_stats) { h->ls.finished = nullptr; h->ls.stats = nullptr; return MCR_OK; }
  if (!h->pool.blobs || !h->pool.level) { g_err = "mcr_set_level_stats: needs a level pool with a level buffer (mcr_set_episode_pool)"; return MCR_ERR_STATE; }
  if (!h->P.ep_return_out || !h->P.ep_len_out) { g_err = "mcr_set_level_stats: needs the episode statistics buffers (mcr_set_episode_stats)"; return MCR_ERR_STATE; }
  h->ls.finished = d_finished_level; h->ls.stats = d_stats;
  return MCR_OK;
}
// the step tail's launch on caller-supplied rows: no handle, the argument checks in front of any HIP call, one launch, no synchronisation
extern "C" int mcr_debug_level_stats(const uint8_t* d_done, const uint8_t* d_trunc, const double* d_ep_return, const int32_t* d_ep_len,
                                     const int32_t* d_level, int num_envs, int num_agents, int K, int32_t* d_finished, double* d_stats, void* stream) {
  if (!d_done || !d_ep_return || !d_ep_len || !d_level || !d_finished || !d_stats) { g_err = "mcr_debug_level_stats: null argument (only d_trunc may be NULL)"; return MCR_ERR_ARG; }
  if (num_envs < 1 || num_agents < 1 || num_agents > MCR_MAX_AGENTS || K < 1) { g_err = "mcr_debug_level_stats: num_envs >= 1, num_agents 1..8, K >= 1"; return MCR_ERR_ARG; }
  launch_level_stats((hipStream_t)stream, d_done, d_trunc, d_ep_return, d_ep_len, d_level, num_envs, num_agents, K, d_finished, d_stats);
  HIPCHK(hipGetLastError());
  return MCR_OK;
}
