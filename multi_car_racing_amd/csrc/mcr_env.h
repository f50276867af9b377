// mcr_env.h — the handle behind include/mcr.h's mcr_env and what the library's translation units share: mcr_hip.hip (creation, the step, the
// refill service, debug readers) and mcr_state.hip (state access and snapshots).  Internal: nothing outside csrc/ includes it.
#pragma once
#include "../../include/mcr.h"
#include "mcr_kernels.h"
#include <hip/hip_runtime.h>
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
  mcr_config cfg;
  McrParams P;
  void* slab;
  size_t slab_bytes;
  int32_t* consumed_host;     // mapped host memory
  int32_t* consumed_seen;     // host copy of the last polled counters
  int timing;                 // bit mask of kernel ids to time with HIP events
  std::vector<TimedLaunch> pending;
  std::vector<hipEvent_t> free_events;
  double t_ms[MCR_TIMING_SLOTS]; int64_t t_n[MCR_TIMING_SLOTS];
  bool any_reset;
  bool split;                 // contact side stream enabled (cfg.num_streams == 2)
  int step_parity;            // which contact-list buffer the next step fills
  int32_t* stage_ids;         // [B] device scratch of mcr_stage_episodes
  hipStream_t s_side, s_defer; // internal streams: the contact envs' chain, the deferred envs' chain
  hipEvent_t ev_fork, ev_join, ev_fork2, ev_join2, ev_col;
  unsigned long long* view_stamps;   // [BN][16] phase clocks of the rasteriser (DEBUG_VIEW_CLOCKS)
  // hipGraph of one step (mcr_set_step_graph): one per contact-list parity, re-captured when any argument changes
  struct StepGraph { bool valid; McrParams P; hipStream_t st; int view_flags; hipGraph_t graph; hipGraphExec_t exec; };
  StepGraph sg[2 * MCR_OBS_STACK_MAX];   // [ring head j][parity] (mcr_set_obs_format: the raster's launches carry j)
  int use_graph;              // 0 off, 1 on, -1 capture failed once: stay off
  bool concurrent_collide;    // the contact pass may run beside the main dynamics (kernels of different streams do overlap here: probed at create)
  bool verdict_fresh;         // the touch verdicts (k_touch.h) of the next step's entry poses are in place (last step's bookkeeping wrote them)
  bool last_fused = false;    // ... and so is the next step's contact list (the last step ran with McrParams::fuse_collide)
  uint32_t* status_host;      // [MCR_STATUS_WORDS] mapped host memory the kernels report trouble in (mcr_kernels.h: ST_*)
  uint32_t status_seen[MCR_STATUS_WORDS];   // what mcr_step has already reported
  int32_t step_count;         // steps launched: the epoch of the three-chain step's per-env "contact pass done" words
  bool bp_fresh;              // mcr_set_bodies teleported cars: the next contact pass re-creates their broadphase proxies
  int simd_count;             // SIMDs of the device (4 per CU)
  int32_t* dev_step_ctr;      // device-side step counter (the epoch of a replayed step graph)
  bool viewprep_in_flags;     // three-chain step: k_viewprep (side stream, beside the bookkeeping) produces the main envs' view records / car polygons
  int list_view_grid;         // workgroups of a list raster launch
  std::vector<std::pair<hipStream_t, bool>> bound;   // caller streams checked by mcr_bind_stream: may the step order its streams with phase words when launched on this one?
  bool soft_denied = false;   // kernels overlap here, but another handle of this process holds the device's one phase-word token (mcr_create)
  bool soft_token = false;    // this handle is its device's one phase-word handle (mcr_create)
  bool soft_sync = false;     // the step's streams meet through phase words in device memory (mcr_kernels.h: mcr_post / mcr_await) instead of events
  int chain_grid;             // workgroups of a list chain launch (each walks the list, 2 envs at a time)
  bool vorder_dirty[2];       // the raster order list of that step parity was filled by a step that did not draw
  void* term_slab = nullptr;  // terminal observations (mcr_set_terminal_obs): entry state, view records, per-parity counters and lists
  int32_t* term_cnt2 = nullptr;   // [2][4] counters by step parity
  int32_t* term_list2 = nullptr;  // [2][2][cap] entry lists by step parity and chain
  struct RefillSvc* svc = nullptr;  // mcr_refill_start: the handle's own host thread that generates and stages consumed episodes
  bool obs_gray = false;      // mcr_set_obs_format: the raster's GRAY instantiations ...
  McrObsRing ring{nullptr, 1, 0};   // ... and where their frames go (ring.j: set per launch)
  uint64_t obs_draws = 0;     // drawing steps enqueued (mcr_step with an observation buffer): the ring head is obs_draws mod k
  bool flags_pending = false; // the last step left the bookkeeping of its main envs (k_flags.h) to its successor (step_phase_words): flags_P launches it
  McrParams flags_P;          // ... the launch's parameters: ROLE_MAIN with that step's partition marks (its parity's part / dpart buffers), no touch verdicts
  McrStateObs so{nullptr, 0, 0, 0};   // mcr_set_state_obs: the low-dimensional observation (k_stateobs.h); out == nullptr: off
  McrRangeObs ro{};           // mcr_set_range_obs: the range-finder observation (k_rangeobs.h); out == nullptr: off
  McrDriver drv{};            // mcr_set_drivers: the scripted driver's parameter rows (k_driver.h) ...
  float* drv_out = nullptr;   // ... the registered [B][N][3] buffer (nullptr: no drivers, nothing is launched) ...
  uint32_t drv_mask = 0;      // ... and the cars it drives
  McrPool pool{nullptr, 0, 0, 0, 0, nullptr};   // mcr_set_episode_pool: the device stages the episodes itself (k_pool.h); blobs == nullptr: the host does
};

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
// mcr_hip.hip: what every reader / writer of env state outside the step calls
void flush_flags(mcr_env* h, hipStream_t st);          // launch the bookkeeping a phase-word step left to its successor
hipError_t sync_state(mcr_env* h);                     // the device's work complete, that bookkeeping included
bool capturing(hipStream_t st);
void launch_state_obs(mcr_env* h, hipStream_t st);     // the state vector of the current state (k_stateobs.h), where the feature is on
void launch_range_obs(mcr_env* h, hipStream_t st);     // the range-finder tensor of the current state (k_rangeobs.h), where the feature is on
