// mcr_env.h — the handle behind include/mcr.h's mcr_env and what the library's translation units share: mcr_hip.hip (creation, reset, the
// step, staging, observation format), mcr_derived.hip (what is derived from the state a reset / step ended with: state vector, range finder,
// scripted drivers, level pools and their statistics, car contacts), mcr_refill.hip (the refill service), mcr_debug.hip (debug readers, bench helpers) and mcr_state.hip (state
// access and snapshots).  The shared surface is listed ONCE, at the end, under the unit that defines it.  Internal: nothing outside csrc/ includes it.
#pragma once
#include "../../include/mcr.h"
#include "mcr_kernels.h"
#include <hip/hip_runtime.h>
#include <atomic>
#include <string>
#include <vector>

extern thread_local std::string g_err;      // what mcr_last_error returns (mcr_hip.hip)
#define HIPCHK(x)                                                                                         \
  do {                                                                                                    \
    hipError_t e_ = (x);                                                                                  \
    if (e_ != hipSuccess) {                                                                               \
      g_err = std::string(#x) + ": " + hipGetErrorString(e_);                                             \
      return MCR_ERR_HIP;                                                                                 \
    }                                                                                                     \
  } while (0)

struct TimedLaunch { int id; hipEvent_t a, b; };

struct mcr_env {
  mcr_config cfg{};           // every field starts null / 0 / false: mcr_create assigns what differs, release_env (mcr_hip.hip) tolerates the rest
  McrParams P{};
  void* slab = nullptr;
  size_t slab_bytes = 0;
  int32_t* consumed_host = nullptr;     // mapped host memory
  int32_t* consumed_seen = nullptr;     // host copy of the last polled counters
  int timing = 0;                 // bit mask of kernel ids to time with HIP events
  std::vector<TimedLaunch> pending;
  std::vector<hipEvent_t> free_events;
  double t_ms[MCR_TIMING_SLOTS] = {}; int64_t t_n[MCR_TIMING_SLOTS] = {};
  bool any_reset = false;
  bool split = false;                 // contact side stream enabled (cfg.num_streams == 2)
  int step_parity = 0;            // which contact-list buffer the next step fills
  int32_t* stage_ids = nullptr;   // [B] device scratch of stage_rows
  hipStream_t s_side = nullptr, s_defer = nullptr;   // internal streams: the contact envs' chain, the deferred envs' chain
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_fork2 = nullptr, ev_join2 = nullptr, ev_col = nullptr;
  unsigned long long* view_stamps = nullptr;   // [BN][16] phase clocks of the rasteriser (DEBUG_VIEW_CLOCKS)
  // hipGraph of one step (mcr_set_step_graph): one per contact-list parity, re-captured when any argument changes
  struct StepGraph { bool valid = false; McrParams P{}; hipStream_t st = nullptr; int view_flags = 0; hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; };
  StepGraph sg[2 * MCR_OBS_STACK_MAX];   // [ring head j][parity] (mcr_set_obs_format: the raster's launches carry j)
  int use_graph = 0;              // 0 off, 1 on, -1 capture failed once: stay off
  bool concurrent_collide = false;    // the contact pass may run beside the main dynamics (kernels of different streams do overlap here: probed at create)
  bool verdict_fresh = false;         // the touch verdicts (k_touch.h) of the next step's entry poses are in place (last step's bookkeeping wrote them)
  bool last_fused = false;    // ... and so is the next step's contact list (the last step ran with McrParams::fuse_collide)
  uint32_t* status_host = nullptr;      // [MCR_STATUS_WORDS] mapped host memory the kernels report trouble in (mcr_kernels.h: ST_*)
  uint32_t status_seen[MCR_STATUS_WORDS] = {};   // what mcr_step has already reported
  std::atomic<int32_t> step_count{0};   // steps launched: the epoch of the three-chain step's per-env "contact pass done" words.  Written by the stepping thread only; the refill service reads it for its lag figure (relaxed both ways)
  bool bp_fresh = false;              // mcr_set_bodies teleported cars: the next contact pass re-creates their broadphase proxies
  int simd_count = 0;             // SIMDs of the device (4 per CU)
  int32_t* dev_step_ctr = nullptr;      // device-side step counter (the epoch of a replayed step graph)
  bool viewprep_in_flags = false;     // three-chain step: k_viewprep (side stream, beside the bookkeeping) produces the main envs' view records / car polygons
  int list_view_grid = 0;         // workgroups of a list raster launch
  std::vector<std::pair<hipStream_t, bool>> bound;   // caller streams checked by mcr_bind_stream: may the step order its streams with phase words when launched on this one?
  bool soft_denied = false;   // kernels overlap here, but another handle of this process holds the device's one phase-word token (mcr_create)
  bool soft_token = false;    // this handle is its device's one phase-word handle (mcr_create)
  bool soft_sync = false;     // the step's streams meet through phase words in device memory (mcr_kernels.h: mcr_post / mcr_await) instead of events
  int chain_grid = 0;             // workgroups of a list chain launch (each walks the list, 2 envs at a time)
  bool vorder_dirty[2] = {};       // the raster order list of that step parity was filled by a step that did not draw
  void* term_slab = nullptr;  // terminal observations (mcr_set_terminal_obs): entry state, view records, per-parity counters and lists
  int32_t* term_cnt2 = nullptr;   // [2][4] counters by step parity
  int32_t* term_list2 = nullptr;  // [2][2][cap] entry lists by step parity and chain
  struct RefillSvc* svc = nullptr;  // mcr_refill_start: the handle's own host thread that generates and stages consumed episodes
  bool obs_gray = false;      // mcr_set_obs_format: the raster's GRAY instantiations ...
  McrObsRing ring{nullptr, 1, 0};   // ... and where their frames go (ring.j: set per launch)
  uint64_t obs_draws = 0;     // drawing steps enqueued (mcr_step with an observation buffer): the ring head is obs_draws mod k
  bool flags_pending = false; // the last step left the bookkeeping of its main envs (k_flags.h) to its successor (step_phase_words): flags_P launches it
  McrParams flags_P{};          // ... the launch's parameters: ROLE_MAIN with that step's partition marks (its parity's part / dpart buffers), no touch verdicts
  McrStateObs so{nullptr, 0, 0, 0};   // mcr_set_state_obs: the low-dimensional observation (k_stateobs.h); out == nullptr: off
  McrRangeObs ro{};           // mcr_set_range_obs: the range-finder observation (k_rangeobs.h); out == nullptr: off
  McrGridObs go{};            // mcr_set_grid_obs: the grid observation (k_gridobs.h); out == nullptr: off
  McrDriver drv{};            // mcr_set_drivers / mcr_set_racecraft: the scripted driver's parameter rows, racecraft rows and mask (k_driver.h) ...
  float* drv_out = nullptr;   // ... the registered [B][N][3] buffer (nullptr: no drivers, nothing is launched) ...
  uint32_t drv_mask = 0;      // ... and the cars it drives
  McrPool pool{nullptr, 0, 0, 0, 0, nullptr, nullptr, nullptr};   // mcr_set_episode_pool: the device stages the episodes itself (k_pool.h); blobs == nullptr: the host does
  McrLevelStats ls{nullptr, nullptr};   // mcr_set_level_stats: per-level episode statistics (k_levelstats.h); stats == nullptr: off
  McrContactObs co{nullptr, nullptr};   // mcr_set_contact_obs: the car-contact observation (k_contactobs.h); mask == nullptr: off
  McrEndRules er{};           // mcr_set_end_rules: early episode ending (k_endrules.h); counters == nullptr: off (P.end_armed is null then, too)
};

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
void mcr_build_shapes(McrShapes* S);                   // mcr_host.cpp
// mcr_hip.hip: what every reader / writer of env state outside the step calls ...
void flush_flags(mcr_env* h, hipStream_t st);          // launch the bookkeeping a phase-word step left to its successor
hipError_t sync_state(mcr_env* h);                     // the device's work complete, that bookkeeping included
bool capturing(hipStream_t st);
bool stream_bound(const mcr_env* h, hipStream_t st);   // may a step launched on caller stream `st` order its streams with phase words?
// ... and the one staging path (mcr_stage_episodes, the refill service): n rows of `src` into the free slots of envs ids[0..n) (null: 0..n-1)
hipError_t stage_rows(mcr_env* h, const int32_t* ids, int n, const uint8_t* src, bool row_by_id, hipStream_t st, const char** what);
// mcr_derived.hip: the launches behind a reset, a restore and a step, on the caller's stream; each returns at once where its feature is off
void launch_derived(mcr_env* h, hipStream_t st);       // the outputs derived from the current state: state vector (k_stateobs.h), range finder (k_rangeobs.h), grid (k_gridobs.h), car contacts (k_contactobs.h, not accumulating), the end rules' settle pass (k_endrules.h)
// the car-contact observation (k_contactobs.h) from the store as it stands.  ONE place launches it for a step: step_one (mcr_hip.hip), behind
// launch_step of EVERY sub-step with accumulate = sub > 0 — launch_step_tail, which runs behind the last sub-step only, leaves it alone
// (a second, non-accumulating pass there would wipe the earlier sub-steps' sums).  Reset, restore and clone get it through launch_derived
void launch_contact_obs(mcr_env* h, hipStream_t st, bool accumulate);
// early episode ending (k_endrules.h), the ADVANCE pass: the same ONE place, step_one, behind launch_step of every sub-step that has actions
// (an action-less step counts nothing), accumulate = sub > 0 for the reason word.  The SETTLE pass goes with launch_derived.  Off: one test
void launch_end_rules(mcr_env* h, hipStream_t st, bool accumulate);
void launch_pool_restage(mcr_env* h, hipStream_t st, int envs_per_group);   // level pools (k_pool.h): the next episode of every env that installed its staged one
// behind the last sub-step of a macro-step: the state vector, the range finder and the grid (launch_derived's, less the car contacts), the per-level statistics (k_levelstats.h) from the step's done / truncated rows while
// `level` still names the episodes that ended, then the pool re-stage with MCR_POOL_GROUP
void launch_step_tail(mcr_env* h, hipStream_t st, const uint8_t* d_done, const uint8_t* d_trunc);
// mcr_refill.hip, mcr_debug.hip: ABI entry points only (mcr_destroy calls mcr_refill_stop first).
