// mcr_hip.hip — the core of the C ABI (include/mcr.h) over the gfx950 kernels: handle creation and the stream-ordering probe, reset, the three
// step paths, episode staging, the observation-format / terminal-obs / graph setters, render.  One handle owns one env slice on one device:
// SoA car state, per-env state, two episode slots per env.  The other units of the ABI and what they share with this one: mcr_env.h.
#include "mcr_env.h"
#include "k_dynamics.h"
#include "k_collide.h"
#include "k_raster_common.h"
#include "k_flags.h"
#include "k_viewprep.h"
#include "k_list_chain.h"
#include "k_render.h"
#include <hip/hip_ext.h>
#include <cstring>
#include <cstdlib>

thread_local std::string g_err;
extern "C" const char* mcr_last_error(void) { return g_err.c_str(); }
extern "C" const char* mcr_version(void) { return "mcr-hip 0.1 (gfx950)"; }

#define MCR_LIST_GRID 128        // workgroups of a list launch (they walk the device-side list)
// Does the three-chain step run the contact pass BESIDE the main dynamics?  Only where kernels of different streams overlap
// (probed at create), up to 7 cars per env (measured), and only for batches whose main dynamics launch puts at most one of its
// 256-VGPR wavefronts on a SIMD: that launch waits INSIDE the kernel for words of the contact pass, which must be able to get onto
// the machine beside it (one such wavefront per SIMD leaves half the register file and nearly all LDS free; two on every SIMD
// could starve a contact pass dispatched second).  After a reported give-up the handle stays with the contact pass in front.
static bool cc_active(const mcr_env* h) { return h->split && h->concurrent_collide; }

#include <mutex>
#include <algorithm>
// live handles of this process that order their streams with phase words.  Several per device are fine AS LONG AS their internal streams sit
// on hardware queues of their own (probed pairwise in mcr_create): an await at the head of a queue that two handles share could hold back the
// very kernel another handle's await waits for (host threads stepping two handles interleave their enqueues freely) — a cycle that only the
// wait bound would break.  HIP multiplexes the streams of a priority class over a few hardware queues (GPU_MAX_HW_QUEUES, 4 by default):
// where the probe finds two handles' streams on one queue, the later handle orders its streams with events.
static std::mutex g_soft_mu;
static std::vector<mcr_env*> g_soft_list;

// Do kernels of two streams really run side by side in this process?  Under a counter-collecting profiler, a debugger or
// AMD_SERIALIZE_KERNEL they do not — and the cc_mode step (the main dynamics waits inside the kernel for words the
// contact pass, launched on another stream, writes) must not be used then.  Probe: kernel A spins (bounded, ~2 ms) until
// kernel B, launched AFTER it on another stream, has set a flag.
__global__ void k_probe_wait(int* flag, int* result) {
  int seen = 0;
  for (int i = 0; i < 20000 && !seen; ++i) { seen = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); __builtin_amdgcn_s_sleep(32); }
  *result = seen;
}
__global__ void k_step_begin(int32_t* step_ctr) { *step_ctr = (int32_t)((uint32_t)*step_ctr + 1u); }      // (wraps: epochs are compared as 32-bit distances)
__global__ void k_probe_set(int* flag) { __hip_atomic_store(flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
static bool kernels_overlap(hipStream_t sa, hipStream_t sb) {
  int* d = nullptr; int r = 0;
  if (hipMalloc(&d, 2 * sizeof(int)) != hipSuccess) return false;
  bool ok = hipMemset(d, 0, 2 * sizeof(int)) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL(k_probe_wait, dim3(1), dim3(1), 0, sa, d, d + 1);
    hipLaunchKernelGGL(k_probe_set, dim3(1), dim3(1), 0, sb, d);
    ok = hipDeviceSynchronize() == hipSuccess && hipMemcpy(&r, d + 1, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess && r == 1;
  }
  (void)hipFree(d);
  return ok;
}

// The three-chain step's internal streams and how it orders its streams (mcr_config.num_streams == 2, launch_step): sets the handle's split
// (false where a stream cannot be created), soft_sync, soft_token, soft_denied and concurrent_collide.  MCR_SOFT_SYNC=0 forces events and
// MCR_SEQUENTIAL_COLLIDE=1 the contact pass in front of the dynamics: what serialising profilers, graph capture and a give-up get (the parity
// suite covers each).
static void select_step_ordering(mcr_env* h) {
  const int B = h->cfg.num_envs, N = h->cfg.num_agents, G = h->P.G;
  // highest priority: their few workgroups must not queue behind the main stream's saturating raster launch.
  // (Tried: giving the chains CUs of their own with hipExtStreamCreateWithCUMask — tools/ubench/cumask_probe.hip shows
  // the mask layout — restores their stand-alone kernel times beside the raster, but every launch and event hop on a
  // masked stream costs ~10 us more: 0.81 ms per step.)
  int prio_lo = 0, prio_hi = 0; (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
  if (hipStreamCreateWithPriority(&h->s_side, hipStreamNonBlocking, prio_hi) != hipSuccess) { (void)hipGetLastError(); return; }
  // (the priority of the third stream — it carries the main raster, whose backlog of workgroups competes with the list raster at the
  // tail of the caller's stream for every LDS slot that frees up — makes no difference: high / normal / low 14.73 / 14.72 / 14.72 M)
  if (hipStreamCreateWithPriority(&h->s_defer, hipStreamNonBlocking, prio_hi) != hipSuccess) { (void)hipStreamDestroy(h->s_side); h->s_side = nullptr; (void)hipGetLastError(); return; }
  const unsigned evf = hipEventDisableTiming;     // (hipEventReleaseToDevice changes nothing measurable: tools/ubench/event_gap.hip)
  for (hipEvent_t* e : {&h->ev_fork, &h->ev_join, &h->ev_fork2, &h->ev_join2, &h->ev_col}) (void)hipEventCreateWithFlags(e, evf);
  h->soft_sync = kernels_overlap(h->s_defer, h->s_side);     // (a waiting kernel needs the kernels it waits for to run beside it)
  if (const char* g = getenv("MCR_SOFT_SYNC")) h->soft_sync = h->soft_sync && atoi(g) != 0;
  // A further phase-word handle on the device needs internal streams on hardware queues of its own.  The main dynamics, which posts
  // "begin", goes out before every wait of its step, but host threads stepping two handles interleave their enqueues freely: with the
  // streams of both multiplexed over the same hardware queues, handle A's waiting kernel can sit in front of a kernel handle B's step
  // waits for, and B's in front of one of A's — a cycle that only the wait bound would break.  A handle whose streams share a queue
  // with another phase-word handle's orders its streams with events (every wait there is for work enqueued earlier).
  if (h->soft_sync) {
    std::lock_guard<std::mutex> lk(g_soft_mu);
    bool own_queues = true;
    for (mcr_env* o : g_soft_list)
      if (own_queues && o->cfg.device == h->cfg.device)
        own_queues = kernels_overlap(h->s_side, o->s_side) && kernels_overlap(h->s_side, o->s_defer) && kernels_overlap(h->s_defer, o->s_side) && kernels_overlap(h->s_defer, o->s_defer) &&
                     kernels_overlap(o->s_side, h->s_side) && kernels_overlap(o->s_defer, h->s_defer);
    if (own_queues) { h->soft_token = true; g_soft_list.push_back(h); }
    else { h->soft_sync = false; h->soft_denied = true; }
  }
  // (at 8 cars per env the one-step-ahead touch verdict — a second pass over up to 28 car pairs — costs more than the
  // contact pass gains by running beside the dynamics: measured at N = 8, round 2: 3.66 vs 4.28 M env-steps/s.  Round 3 tried a
  // CONSERVATIVE verdict there instead — bounding discs + car boxes, no narrowphase, the contact chain taking every env it
  // marks: with ~340 of 4096 envs in contact and as many near misses per step the side stream's chain, bookkeeping and raster
  // grow faster than the 110 us of k_collide that leave the critical path: 1.40 vs 0.975 ms per step.  What bounds N = 8 is the
  // contact chain itself — 585 us for its slowest wavefront, a sequential Gauss-Seidel over the contacts between the joint sweeps)
  // (round 3, phase-word path, contact pass beside / in front of the dynamics: N = 5 8.99 / 8.50 M env-steps/s, N = 6 7.87 / 7.49,
  // N = 7 7.16 / 6.80, N = 8 4.90 / 5.47 — up to seven cars per env it runs beside)
  h->concurrent_collide = N <= 8 && !getenv("MCR_SEQUENTIAL_COLLIDE") && mcr_dyn_blocks(B, G) <= h->simd_count && kernels_overlap(h->s_defer, h->s_side);
  h->split = true;
  (void)hipGetLastError();
}

// What a handle owns, given back in mcr_destroy's order — graphs, events, streams, memory — and the handle itself.  Tolerates a partly built
// one (mcr_create's error paths): whatever is still null was never made.
static void release_env(mcr_env* h) {
  for (auto& g : h->sg) if (g.valid) { (void)hipGraphExecDestroy(g.exec); (void)hipGraphDestroy(g.graph); g.valid = false; }
  for (auto& t : h->pending) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }
  for (auto e : h->free_events) (void)hipEventDestroy(e);
  for (hipStream_t st : {h->s_side, h->s_defer}) if (st) (void)hipStreamDestroy(st);
  for (hipEvent_t e : {h->ev_fork, h->ev_join, h->ev_fork2, h->ev_join2, h->ev_col}) if (e) (void)hipEventDestroy(e);
  for (void* d : {h->slab, h->term_slab, (void*)h->ring.fresh}) if (d) (void)hipFree(d);
  for (void* m : {(void*)h->consumed_host, (void*)h->status_host}) if (m) (void)hipHostFree(m);
  delete[] h->consumed_seen;
  delete h;
}

extern "C" int mcr_create(const mcr_config* cfg, mcr_env** out) {
  if (!cfg || !out) { g_err = "null argument"; return MCR_ERR_ARG; }
  if (cfg->num_envs < 1 || cfg->num_envs > MCR_VORDER_ENV_MASK || cfg->num_agents < 1 || cfg->num_agents > MCR_MAX_AGENTS) { g_err = "num_envs/num_agents out of range"; return MCR_ERR_ARG; }
  HIPCHK(hipSetDevice(cfg->device));
  mcr_env* h = new mcr_env();
  h->cfg = *cfg;
  // A list chain is a serial solver chain per wavefront (2 envs each).  With i.i.d. random actions and two cars per env the
  // contact list holds ~15 envs of 4096, but a policy that actually drives (or N = 8: ~340 envs) fills it with hundreds, and
  // every further round of the walk adds a whole chain (~300 us) to the side stream: the grid covers 1024 envs in one round;
  // surplus workgroups exit on their first load.
  h->chain_grid = 4 * MCR_LIST_GRID;
  h->viewprep_in_flags = cfg->num_agents <= 3;     // beyond three cars per env the bookkeeping + raster chain is the step's critical path: the epilogue stays in the dynamics (round 3, phase-word path: N = 3 13.4 -> 13.7 M with it, N = 4 10.8 -> 10.6, N = 8 no difference)
  h->list_view_grid = cfg->num_agents <= 2 ? MCR_LIST_GRID : 8 * MCR_LIST_GRID;
  { hipDeviceProp_t prop; h->simd_count = (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess ? prop.multiProcessorCount : 256) * 4; }
  const int B = cfg->num_envs, N = cfg->num_agents;
  int G = 1; while (G < N) G <<= 1;
  const size_t BN = (size_t)B * N;
  size_t off = 0;
  auto carve = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
  const size_t o_carf = carve(sizeof(float) * CF_COUNT * BN);
  const size_t o_card = carve(sizeof(double) * CD_COUNT * BN);
  const size_t o_caru = carve(sizeof(uint32_t) * CU_COUNT * BN);
  const size_t o_env = carve(sizeof(McrEnvState) * B);
  const size_t o_touch = carve(sizeof(uint32_t) * MCR_TILE_CAP * (size_t)B);
  const size_t o_tflags = carve(sizeof(uint16_t) * MCR_TILE_CAP * (size_t)B);
  const size_t o_cc = carve(sizeof(uint32_t) * (size_t)B * (MCR_CC_MAX * MCR_CC_WORDS + 4));
  const size_t o_bpf = carve(sizeof(float4) * BP_COUNT * MCR_BP_FIX * BN);
  const size_t o_ccstamp = carve(sizeof(uint32_t) * (size_t)B * mcr_cc_stamp_words(N));
  const size_t o_bpstamp = carve(sizeof(uint32_t) * (size_t)B * MCR_TILE_CAP * 4 * N);
  const size_t o_part = carve(2 * (size_t)B);                 // x2: the touch verdicts of a step live in the buffer of its parity
  const size_t o_dpart = carve(2 * (size_t)B);                // x2, like part: the next step's deferred bookkeeping launch reads this step's
  const size_t o_epoch = carve(sizeof(int32_t) * ((size_t)B + 1));
  const size_t o_sync = carve(sizeof(int32_t) * 16 * MCR_SYNC_WORDS);
  const size_t o_dlist = carve(sizeof(int32_t) * 2 * ((size_t)B + 1));      // x2: the lists of a step live in the buffers of its parity
  const size_t o_rlist = carve(sizeof(int32_t) * 2 * ((size_t)B + 1));
  const size_t o_dstate = carve(BN);
  const size_t o_counters = carve(sizeof(unsigned long long) * 8);
  const size_t o_statusdev = carve(sizeof(uint32_t) * MCR_STATUS_WORDS);
  const size_t o_stage_ids = carve(sizeof(int32_t) * (size_t)B);
  const size_t o_stats = carve(sizeof(double) * 2);
  const size_t o_vorder = carve(sizeof(int32_t) * 2 * ((size_t)B + 2));
  const size_t o_stamps = carve(sizeof(unsigned long long) * 8 * ((size_t)mcr_dyn_blocks(B, G) + 2 * (size_t)B));
  const size_t o_clist = carve(sizeof(int32_t) * 2 * ((size_t)B + 1));
  const size_t o_shapes = carve(sizeof(McrShapes));
  const size_t o_viewp = carve(sizeof(float) * MCR_VIEWP_FLOATS * BN);
  const size_t o_carpoly = carve(sizeof(float) * MCR_CARPOLY_FLOATS * BN);
  const size_t o_vscratch = carve(sizeof(unsigned long long) * 16 * BN);
  const size_t o_particles = carve(cfg->skid_particles ? sizeof(uint32_t) * MCR_PART_WORDS * BN : 0);
  const bool one_world = cfg->fresh_world == 0;      // (k_world.h: the env's b2World across its episodes, the reference's semantics; zero-initialised = an empty world)
  const size_t o_pidtab = carve(one_world ? sizeof(uint16_t) * MCR_PID_TAB * (size_t)B : 0);
  const size_t o_pidstk = carve(one_world ? sizeof(uint16_t) * MCR_PID_STACK * (size_t)B : 0);
  const size_t o_pidmeta = carve(one_world ? sizeof(int32_t) * 4 * (size_t)B : 0);
  const size_t o_slots = carve((size_t)B * 2 * MCR_SLOT_BYTES);
  h->slab_bytes = off;
  if (hipMalloc(&h->slab, off) != hipSuccess) { h->slab = nullptr; g_err = "hipMalloc failed"; release_env(h); return MCR_ERR_HIP; }
  (void)hipMemset(h->slab, 0, o_slots);
  for (int par = 0; par < 2; ++par)      // raster order lists (per step parity: 2 counts, then B entries): -1 = unused entry
    (void)hipMemset((uint8_t*)h->slab + o_vorder + sizeof(int32_t) * ((size_t)par * (B + 2) + 2), 0xff, sizeof(int32_t) * (size_t)B);
  uint8_t* base = (uint8_t*)h->slab;
  McrParams& P = h->P;
  memset(&P, 0, sizeof(P));      // (padding included: step_one compares whole blocks)
  P.B = B; P.N = N; P.G = G; P.BN = (int)BN;
  P.carf = (float*)(base + o_carf); P.card = (double*)(base + o_card); P.caru = (uint32_t*)(base + o_caru);
  P.env = (McrEnvState*)(base + o_env); P.tile_touch = (uint32_t*)(base + o_touch); P.tile_flags = (uint16_t*)(base + o_tflags);
  P.cc_store = (uint32_t*)(base + o_cc); P.bpf = (float4*)(base + o_bpf); P.cc_stamp = (uint32_t*)(base + o_ccstamp); P.bp_stamp = (uint32_t*)(base + o_bpstamp); P.shapes = (const McrShapes*)(base + o_shapes); P.slots = base + o_slots;
  P.pid_tab = one_world ? (uint16_t*)(base + o_pidtab) : nullptr; P.pid_stack = one_world ? (uint16_t*)(base + o_pidstk) : nullptr; P.pid_meta = one_world ? (int32_t*)(base + o_pidmeta) : nullptr;
  h->view_stamps = (unsigned long long*)(base + o_vscratch);
  P.viewp = (float*)(base + o_viewp);
  P.part = base + o_part; P.dpart = base + o_dpart; P.collide_epoch = (int32_t*)(base + o_epoch); h->dev_step_ctr = P.collide_epoch + B; P.sync_words = (int32_t*)(base + o_sync); P.dlist = (int32_t*)(base + o_dlist); P.rlist = (int32_t*)(base + o_rlist); P.defer_state = base + o_dstate; P.counters = (unsigned long long*)(base + o_counters); P.status_dev = (uint32_t*)(base + o_statusdev); P.stats = (double*)(base + o_stats);
  h->stage_ids = (int32_t*)(base + o_stage_ids); P.vcount = (int32_t*)(base + o_vorder); P.vorder = P.vcount + 2; P.dbg_stamps = (unsigned long long*)(base + o_stamps); P.clist = (int32_t*)(base + o_clist);
  P.carpoly = (float*)(base + o_carpoly);
  P.particles = cfg->skid_particles ? (uint32_t*)(base + o_particles) : nullptr;
  P.auto_reset = cfg->auto_reset; P.max_steps = cfg->max_episode_steps; P.car_contacts = cfg->car_contacts;
  P.backwards_flag = cfg->backwards_flag; P.use_ego_color = cfg->use_ego_color; P.h_ratio = cfg->h_ratio;
  McrShapes S; mcr_build_shapes(&S);
  // the raster gives two record slots to hull polygon 2 (HULL_POLY3, 8 vertices) and one to every other car polygon
  if (S.hull[0].n > 4 || S.hull[1].n > 4 || S.hull[2].n > 8 || S.hull[3].n > 4 || S.wheel.n > 4) { g_err = "unexpected car fixture vertex counts"; release_env(h); return MCR_ERR_STATE; }
  (void)hipMemcpy((void*)P.shapes, &S, sizeof(S), hipMemcpyHostToDevice);
  if (hipHostMalloc((void**)&h->consumed_host, sizeof(int32_t) * B, hipHostMallocMapped) != hipSuccess) { h->consumed_host = nullptr; g_err = "hipHostMalloc failed"; release_env(h); return MCR_ERR_HIP; }
  memset(h->consumed_host, 0, sizeof(int32_t) * B);
  void* dptr = nullptr;
  (void)hipHostGetDevicePointer(&dptr, h->consumed_host, 0);
  P.consumed_host = (int32_t*)dptr;
  h->consumed_seen = new int32_t[B]();
  if (hipHostMalloc((void**)&h->status_host, sizeof(uint32_t) * (MCR_STATUS_WORDS + MCR_HOST_COUNTS), hipHostMallocMapped) != hipSuccess) { h->status_host = nullptr; g_err = "hipHostMalloc failed"; release_env(h); return MCR_ERR_HIP; }
  memset(h->status_host, 0, sizeof(uint32_t) * (MCR_STATUS_WORDS + MCR_HOST_COUNTS));
  (void)hipHostGetDevicePointer(&dptr, h->status_host, 0);
  P.status = (uint32_t*)dptr; P.host_counts = P.status + MCR_STATUS_WORDS;
  P.nenv = B; P.role = ROLE_ALL;
  if (cfg->num_streams == 2) select_step_ordering(h);
  (void)hipDeviceSynchronize();
  *out = h;
  return MCR_OK;
}

extern "C" int mcr_destroy(mcr_env* h) {
  if (!h) return MCR_ERR_ARG;
  (void)mcr_refill_stop(h);
  if (h->soft_token) { std::lock_guard<std::mutex> lk(g_soft_mu); g_soft_list.erase(std::remove(g_soft_list.begin(), g_soft_list.end(), h), g_soft_list.end()); }
  (void)hipSetDevice(h->cfg.device);
  (void)sync_state(h);
  release_env(h);
  return MCR_OK;
}

// The one staging path (mcr_stage_episodes; the refill service, mcr_refill.hip): row i (row_by_id: row ids[i]) of `src` goes into the staged slot
// of env ids[i] (ids null: env i), then one id upload + one tiny kernel flip the n staged_ready flags (a 4-byte copy per env from pageable
// memory made staging a whole batch take longer than generating it).  The ids are in range (the callers' business).  On failure *what names the
// call.  The staged slot of env e is ((installs & 1) ^ 1): slot 0 is "current" before the first install and every install flips it.  `installs`
// is read from the mapped-host counter the install wrote; the device cannot install again before this copy lands (staged_ready is 0 until then).
hipError_t stage_rows(mcr_env* h, const int32_t* ids, int n, const uint8_t* src, bool row_by_id, hipStream_t st, const char** what) {
  if (n <= 0) return hipSuccess;
  hipError_t er = hipSuccess;
  *what = "hipMemcpyAsync (episode)";
  for (int i = 0; i < n; ++i) {
    const int e = ids ? ids[i] : i;
    const int32_t installs = ((volatile int32_t*)h->consumed_host)[e];
    uint8_t* dst = h->P.slots + ((size_t)e * 2 + ((installs & 1) ^ 1)) * MCR_SLOT_BYTES;
    if ((er = hipMemcpyAsync(dst, src + (size_t)(row_by_id ? e : i) * MCR_SLOT_BYTES, MCR_SLOT_BYTES, hipMemcpyHostToDevice, st)) != hipSuccess) return er;
  }
  *what = "hipMemcpyAsync (ids)";
  if (ids && (er = hipMemcpyAsync(h->stage_ids, ids, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st)) != hipSuccess) return er;
  *what = "k_mark_staged";
  hipLaunchKernelGGL(k_mark_staged, dim3((n + 255) / 256), dim3(256), 0, st, h->P, ids ? (const int32_t*)h->stage_ids : nullptr, n);
  return hipGetLastError();
}
// TODO(ADVICE r06-2): not refused while the refill service runs (both would stage into the same slots)
extern "C" int mcr_stage_episodes(mcr_env* h, const int32_t* env_ids, int n, const void* blobs, void* stream) {
  if (!h || !blobs || n < 0) { g_err = "bad argument"; return MCR_ERR_ARG; }
  if (h->pool.blobs) { g_err = "mcr_stage_episodes: the handle stages its episodes from a level pool (mcr_set_episode_pool)"; return MCR_ERR_STATE; }
  for (int i = 0; i < n; ++i) { const int e = env_ids ? env_ids[i] : i; if (e < 0 || e >= h->cfg.num_envs) { g_err = "env id out of range"; return MCR_ERR_ARG; } }
  const char* what = "";
  const hipError_t er = stage_rows(h, env_ids, n, (const uint8_t*)blobs, false, (hipStream_t)stream, &what);
  if (er != hipSuccess) { g_err = std::string("mcr_stage_episodes: ") + what + ": " + hipGetErrorString(er); return MCR_ERR_HIP; }
  return MCR_OK;
}

static hipEvent_t get_event(mcr_env* h) {
  if (!h->free_events.empty()) { hipEvent_t e = h->free_events.back(); h->free_events.pop_back(); return e; }
  hipEvent_t e; (void)hipEventCreate(&e); return e;
}
#define LAUNCH(kid_, kernel, grid, block, st, ...) LAUNCH_LDS(kid_, kernel, grid, block, 0, st, __VA_ARGS__)
// `launch_` between two event records where mcr_timing asks for kernel kid_'s time
#define TIMED(kid_, st, launch_)                                                         \
  do {                                                                                   \
    TimedLaunch tl_; bool tm_ = (h->timing >> (kid_)) & 1;                                              \
    if (tm_) { tl_.id = (kid_); tl_.a = get_event(h); tl_.b = get_event(h); (void)hipEventRecord(tl_.a, st); } \
    launch_;                                                                             \
    if (tm_) { (void)hipEventRecord(tl_.b, st); h->pending.push_back(tl_); }                   \
  } while (0)
// a launch that completes the event `stop_` itself (nullptr: none): see mcr_view_launch
#define LAUNCH_LDS_STOP(kid_, kernel, grid, block, lds_, st, stop_, ...) TIMED(kid_, st, hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds_, st, nullptr, stop_, 0, __VA_ARGS__))
#define LAUNCH_LDS(kid_, kernel, grid, block, lds_, st, ...) TIMED(kid_, st, hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds_, st, __VA_ARGS__))

// a launch of the dynamics over all envs: with or without the contact code (k_dynamics.h)
// (with the contact code: k_dynamics_passes behind it, for the wavefronts whose envs hold more manifolds than their LDS pool — k_dynamics.h)
static void launch_dyn_cc(int grid, hipStream_t st, const McrParams& P, int mode) {
  hipLaunchKernelGGL(k_dynamics<true>, dim3(grid), dim3(64), 0, st, P, mode);
  hipLaunchKernelGGL(k_dynamics_passes, dim3(grid), dim3(64), 0, st, P, mode);
}
#define LAUNCH_DYN(kid_, cc_, grid, st, ...) do { if (cc_) TIMED(kid_, st, launch_dyn_cc(grid, st, __VA_ARGS__)); else LAUNCH(kid_, k_dynamics<false>, grid, 64, st, __VA_ARGS__); } while (0)

void mcr_view_launch(int variant, int grid, hipStream_t st, const McrParams& P, unsigned long long* stamps, int only_just_reset, hipEvent_t stop, hipEvent_t start,
                     bool gray, const McrObsRing& ring);   // mcr_view.hip
// raster launch (k_view.h).  Main launches: one workgroup per work slot.  List launches (mcr_is_list_role): MCR_LIST_GRID
// persistent workgroups that walk the list (lane k of a wavefront holds a workgroup's k-th env, so never fewer than
// slots / 64 workgroups).
static int list_grid(int slots, int want) { return std::min(slots, std::max(want, (slots + 63) / 64)); }
static void launch_view(mcr_env* h, int kid, int slots, hipStream_t st, const McrParams& P, int only_just_reset, hipEvent_t stop = nullptr, int want_grid = 0) {
  TimedLaunch tl; const bool tm = (h->timing >> kid) & 1;
  // mcr_timing: where the launch has no stop event of the step's own, the two timing events ARE the dispatch's begin / end timestamps
  // (hipExtLaunchKernelGGL's start and stop events: the kernel's duration as a kernel trace reports it, no marker packets around the launch —
  // records in front of and behind the launch add the gap to the kernel before it: 85.2 against the trace's 82.6 us, round 6)
  const bool own_ts = tm && stop == nullptr;
  hipEvent_t start = nullptr;
  if (tm) { tl.id = kid; tl.a = get_event(h); tl.b = get_event(h); if (own_ts) { start = tl.a; stop = tl.b; } else (void)hipEventRecord(tl.a, st); }
  // (list launches: with more than two cars per env the contact list is long — N = 8: ~340 envs x 8 views per step — and 128
  // workgroups would draw ~20 views each, one after the other, at the end of the side stream's chain)
  if (mcr_is_list_role(P.role)) { McrParams Q = P; Q.split_views = 1; mcr_view_launch(2, list_grid(slots * (Q.split_views ? P.N : 1), std::max(h->list_view_grid, want_grid)) + Q.flags_blocks, st, Q, h->view_stamps, only_just_reset, stop, start, h->obs_gray, h->ring); }
  else mcr_view_launch((P.debug & DEBUG_VIEW_CLOCKS) ? 1 : 0, slots, st, P, h->view_stamps, only_just_reset, stop, start, h->obs_gray, h->ring);
  if (tm) { if (!own_ts) (void)hipEventRecord(tl.b, st); h->pending.push_back(tl); }
}

// The bookkeeping a phase-word step left to its successor (step_phase_words), for everybody who is not that successor: whoever reads or writes what
// the scans read or write (CU_FLAGS, poses, env records, episode slots) launches them first, on the stream its own work goes to — every state
// getter / setter, reset, render, and a step that takes another path than the last one.  The scans depend on nothing a later call changes:
// the poses, env records and episode slots are the ones the step ended with until the next step's dynamics writes back.
// k_flags' geometry: one wavefront per car of the batch, whatever the launch's role (a wavefront whose env is not the role's returns)
static void launch_flags(hipStream_t st, const McrParams& P) { hipLaunchKernelGGL(k_flags, dim3(P.B * P.N), dim3(64), 0, st, P); }
void flush_flags(mcr_env* h, hipStream_t st) {
  if (!h->flags_pending) return;
  h->flags_pending = false;
  if (h->P.debug & DEBUG_DROP_PENDING_FLAGS) return;     // (tests): the pending launch is DROPPED — stale flags show that the results came through it
  launch_flags(st, h->flags_P);
}
// The scan NOW, on the state as it stands (after mcr_set_bodies / a state restore, which launch nothing; tests): the pending launch first, then
// every env's cars — ROLE_ALL, so that no partition mark skips an env —, no touch verdicts (they are the step's business).  Only enqueues.
extern "C" int mcr_flags_now(mcr_env* h, void* stream) {
  if (!h) { g_err = "null handle"; return MCR_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  flush_flags(h, st);
  McrParams P = h->P;
  P.role = ROLE_ALL; P.part_next = nullptr; P.flags_deferred = 0;
  launch_flags(st, P);
  HIPCHK(hipGetLastError());
  return MCR_OK;
}
// The frame NOW, of the state as it stands (after the state setters, which launch nothing; tests): the pending scans first (the flag word is
// drawn), one pass over every active env's cars for the view records, car polygons, label value and flag word (k_viewprep_now), then ONE main
// raster launch over all B envs — ROLE_ALL, work slot = env index, no raster order list, the plain RGB / GRAY instantiation — into the
// caller's buffer.  Outside the step's streams, lists and graphs; the records it writes are rewritten by the next step.  Only enqueues.
extern "C" int mcr_obs_now(mcr_env* h, uint8_t* d_obs, void* stream) {
  if (!h || !d_obs) { g_err = "mcr_obs_now: null argument"; return MCR_ERR_ARG; }
  if (!h->cfg.obs_enabled) { g_err = "mcr_obs_now needs obs_enabled"; return MCR_ERR_STATE; }
  if (!h->any_reset) { g_err = "mcr_obs_now before reset()"; return MCR_ERR_STATE; }
  if (h->obs_gray && h->ring.k > 1) { g_err = "mcr_obs_now with a stacked observation format (the ring's slots belong to the step)"; return MCR_ERR_STATE; }
  hipStream_t st = (hipStream_t)stream;
  if (capturing(st)) { g_err = "mcr_obs_now inside a stream capture"; return MCR_ERR_STATE; }
  flush_flags(h, st);
  McrParams P = h->P;
  P.role = ROLE_ALL; P.split = 0; P.use_vorder = 0; P.actions = nullptr; P.obs = d_obs;
  hipLaunchKernelGGL(k_viewprep_now, dim3((P.BN + 63) / 64), dim3(64), 0, st, P);
  mcr_view_launch(0, P.B, st, P, h->view_stamps, 0, nullptr, nullptr, h->obs_gray, h->ring);
  HIPCHK(hipGetLastError());
  return MCR_OK;
}
// the synchronous calls (state getters / setters): the device's work is complete and so is the pending bookkeeping (null stream, waited for)
hipError_t sync_state(mcr_env* h) {
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess && h->flags_pending) { flush_flags(h, nullptr); e = hipDeviceSynchronize(); }
  return e;
}

// reset(): install -> collide(1) -> dynamics(1) -> view, in order on one stream
static void launch_reset(mcr_env* h, McrParams P, hipStream_t st) {
  const int B = P.B, N = P.N;
  const int dyn_blocks = mcr_dyn_blocks(B, P.G);
  P.split = 0; P.role = ROLE_ALL; P.use_vorder = 0;
  hipLaunchKernelGGL(k_install, dim3(dyn_blocks), dim3(64), 0, st, P);
  LAUNCH_LDS(3, k_collide, B, 64, col::lds_bytes(N), st, P, 1);
  LAUNCH_DYN(4, P.car_contacts && N > 1, dyn_blocks, st, P, 1);
  if (P.obs) launch_view(h, 2, B, st, P, 1);
}

// may a step launched on caller stream `st` order its streams with phase words?  (mcr_bind_stream checked it; an unbound stream: events)
bool stream_bound(const mcr_env* h, hipStream_t st) {
  for (const auto& b : h->bound) if (b.first == st) return b.second;
  return false;
}
bool capturing(hipStream_t st) { hipStreamCaptureStatus c = hipStreamCaptureStatusNone; (void)hipStreamIsCapturing(st, &c); return c != hipStreamCaptureStatusNone; }
// Does a three-chain step launched on `st` order its streams with phase words (step_phase_words)?  Otherwise with events (step_events).
static bool phase_words(const mcr_env* h, hipStream_t st) {
  return h->soft_sync && h->use_graph <= 0 && !capturing(st) && stream_bound(h, st);
}
// Do the contact chain's workgroups run their envs' contact pass themselves (McrParams::fuse_collide)?  Whenever the contact pass runs beside the
// dynamics (the list then comes from the one-step-ahead verdicts) on the phase-word path (the side stream's last kernel empties the list) — measured
// +0.9 % (N = 2 default), +1.8 % (N = 4) against a chain that waits for the all-env pass.  (Round 5's first attempt diverged in 7 of 10 rollouts
// with ~1000 contact envs: the chain's wavefronts, filling the machine at the step's begin, held the contact pass of the OTHER envs up long enough
// for a latent race of the contact-pass-beside-the-dynamics mode to show — k_dynamics.h "Parking overwrites", NOTES 11.)
static bool fused_collide(const mcr_env* h, hipStream_t st) { return cc_active(h) && phase_words(h, st); }

// The host side of every step: the raster order list of the step's parity, the parity's device-side lists, the terminal counts; flips step_parity
static void step_prologue(mcr_env* h, McrParams& P, hipStream_t st) {
  const int B = P.B;
  // (the raster workgroups reset the raster order entries they consume; a step that filled the list of its parity without
  // drawing — mcr_step without an observation buffer on a handle that has one — left it unconsumed: wipe it before its next use)
  if (h->vorder_dirty[h->step_parity]) { (void)hipMemsetAsync(h->P.vcount + (size_t)h->step_parity * (B + 2) + 2, 0xff, sizeof(int32_t) * (size_t)B, st); h->vorder_dirty[h->step_parity] = false; }
  if (!P.obs && h->cfg.obs_enabled) h->vorder_dirty[h->step_parity] = true;
  P.role = ROLE_ALL; P.split = h->split ? 1 : 0; P.defer_after = 0; P.respawn_list = 0;
  // the device-side lists of a step are double-buffered by step parity: no memset, and nobody zeroes a list somebody reads
  const size_t par = (size_t)h->step_parity, oth = par ^ 1;
  P.clist = h->P.clist + par * (B + 1); P.clist_next = h->P.clist + oth * (B + 1);
  P.dlist = h->P.dlist + par * (B + 1); P.rlist = h->P.rlist + par * (B + 1);
  P.vcount = h->P.vcount + par * (B + 2); P.vorder = P.vcount + 2;
  P.part = h->P.part + par * B; P.part_next = cc_active(h) ? h->P.part + oth * B : nullptr; P.dpart = h->P.dpart + par * B;
  P.next_counts[0] = h->P.dlist + oth * (B + 1); P.next_counts[1] = h->P.rlist + oth * (B + 1);
  P.next_counts[2] = h->P.vcount + oth * (B + 2); P.next_counts[3] = P.next_counts[2] + 1;
  if (h->term_slab && P.obs && P.actions) { P.term_cnt = h->term_cnt2 + par * 4; P.term_cnt_next = h->term_cnt2 + oth * 4; P.term_list = h->term_list2 + par * 2 * (size_t)P.term_cap; }
  else {
    // a step that draws no terminal frames (no actions: frame skip, step(None); no observation buffer) still flips the parity: it zeroes
    // the counters the NEXT step starts from in the drawing step's stead, and reports "no entries" (the next terminal step of
    // that parity started from the counts of two steps back)
    if (h->term_slab) {
      (void)hipMemsetAsync(h->term_cnt2 + oth * 4, 0, sizeof(int32_t) * 4, st);
      if (P.term_count_out) (void)hipMemsetAsync(P.term_count_out, 0, sizeof(int32_t), st);
    }
    P.term_cnt = P.term_cnt_next = nullptr; P.term_idx = nullptr;
  }
  h->step_parity ^= 1;
}

// The argument block of ONE launch: the path's block `p` with the launch's role and the fields its line names — nothing else differs
static McrParams with(McrParams p, McrRole role) { p.role = role; return p; }
template <class F> static McrParams with(McrParams p, McrRole role, F&& edit) { p.role = role; edit(p); return p; }

// single stream: collide -> dynamics -> reset pass of the re-spawned envs (:408) -> raster -> bookkeeping, all envs
//   launch (all on st)                      grid         block: P (the prologue's: ROLE_ALL, split 0) with
//   k_collide pass 0, k_dynamics            B, dyn       -
//   auto_reset: k_term_prep, k_collide pass 1, k_dynamics mode 1     B, B, dyn    -
//   raster 2                                B            use_vorder 1
//   terminal entries: raster 7 (list), k_term_finish     B (slots), 1   ROLE_TERMINAL; -
//   k_flags                                 B * N        -
static void step_single_stream(mcr_env* h, const McrParams& P, hipStream_t st, int view_flags) {
  const int B = P.B, N = P.N, dyn_blocks = mcr_dyn_blocks(B, P.G);
  const bool draw = P.obs != nullptr;
  LAUNCH_LDS(0, k_collide, B, 64, col::lds_bytes(N), st, P, 0);
  LAUNCH_DYN(1, P.car_contacts && N > 1, dyn_blocks, st, P, 0);
  if (P.auto_reset) {
    if (P.term_cnt) hipLaunchKernelGGL(k_term_prep, dim3(B), dim3(64), 0, st, P);     // (the terminal entries of the envs that end here, before the pass clears their tile flags)
    LAUNCH_LDS(3, k_collide, B, 64, col::lds_bytes(N), st, P, 1);
    LAUNCH_DYN(4, P.car_contacts && N > 1, dyn_blocks, st, P, 1);
  }
  if (draw) launch_view(h, 2, B, st, with(P, ROLE_ALL, [](McrParams& q) { q.use_vorder = 1; }), 0);
  if (P.term_cnt) { launch_view(h, 7, B, st, with(P, ROLE_TERMINAL), 0); hipLaunchKernelGGL(k_term_finish, dim3(1), dim3(256), 0, st, P); }
  if (view_flags) launch_flags(st, P);
}

// Grid sizes of the three-chain step, whichever way its streams are ordered (launch_step computes them once)
struct StepGrids {
  int dyn_blocks;      // the main dynamics
  int lg_con;          // the contact chain (a list launch): one env per wavefront
  int prev_contacts;   // the length of the LAST step's contact list (mapped host word: no synchronisation)
  int lg_flags;        // the bookkeeping of a chain's cars as a list launch of its own
  int ga, gb;          // the caller's chain: workgroups that resume the deferred envs, workgroups for the reset pass of the re-spawned ones
  int vg_con;          // the contact raster's grid wish: sized by the LAST step's list — the lists change slowly — so that a long list, a policy that
                       // drives: ~90 envs of 4096, takes one round of workgroups instead of two or three behind the chain, the step's critical path
};
static StepGrids step_grids(const mcr_env* h, const McrParams& P) {
  const int B = P.B, N = P.N;
  StepGrids g;
  g.dyn_blocks = mcr_dyn_blocks(B, P.G);
  g.lg_con = std::min(B, 2 * h->chain_grid);
  g.prev_contacts = std::min(B, (int)((volatile uint32_t*)h->status_host)[MCR_STATUS_WORDS + HC_CONTACT_ENVS]);
  g.lg_flags = std::min(B * N, (N <= 2 ? 4 : 32) * MCR_LIST_GRID);
  g.ga = std::min({(B + MCR_SIDE_ENVS_PER_WAVE - 1) / MCR_SIDE_ENVS_PER_WAVE, h->chain_grid, MCR_LIST_GRID / 2});
  g.gb = P.auto_reset ? std::min(B, MCR_LIST_GRID) : 0;
  g.vg_con = std::min(2048, g.prev_contacts * N + g.prev_contacts * N / 4 + 8);
  return g;
}

// The three chains ordered by phase words (mcr_kernels.h: soft_sync) — no marker / barrier packets on any stream ([...]: with the contact pass
// beside the dynamics, cc_active; (...): without it):
//   s_side  : await(BEGIN) -> chain(contact envs [, each with its own contact pass in front]) -> raster -> post(SIDE)
//   st      : (collide(all) ->) dynamics(main envs: posts BEGIN, then DYN) -> [await(COL)] chain(resume + re-spawned envs) -> raster -> await(SIDE, MAIN)
//   s_defer : [await(BEGIN) -> {bookkeeping(the LAST step's main envs)} -> collide(main envs) -> post(COL) ->] await(DYN) -> view records, bookkeeping(main envs) -> raster(main envs) -> post(MAIN)
// {...}: N <= 3, drawn steps with actions and the contact pass beside the dynamics.  Nothing mcr_step hands its caller depends on the step's own
// backward / on-grass flags (k_flags.h), so the main envs' scans — 8192 wavefronts, the longest part of the launch in front of the main raster —
// are left to the NEXT step's begin, where the main dynamics keeps one wavefront per SIMD busy and the rest of the machine idles; in front of the
// main raster stay the view records and the touch verdicts of the marked envs (k_viewprep_verdict).  In-stream in front of k_collide: the
// per-env "contact pass done" word that holds back the end of the dynamics (write-back, auto-reset install, parking) then also covers the scans'
// reads, and W_COL also means "the last step's flags are written" (k_dynamics.h: flags_deferred).  Anybody else who needs them: flush_flags.
// (kernel trace, round 3: the resume chain starts 3 us after the dynamics instead of 11-21, the next step's dynamics 0-1 us after
// the step's last kernel instead of 20-32; the chains' bookkeeping: list launches behind the chains; N > 3: the main envs'
// bookkeeping on the caller's stream)
// The launches in enqueue order.  P: launch_step's block with soft_sync 1, flags_deferred (the last step's scans run in this one), split 0,
// viewprep_in_flags vif.  Pbegin (what opens the step): P with ROLE_ALL, split 1, viewprep_in_flags 0.  Pside (the side stream): P with
// ROLE_CONTACT, viewprep_in_flags 0.
//   launch                               stream    grid                     block
//   (k_collide pass 0)                   st        B                        Pbegin
//   (the pending k_flags, flush_flags)   st        B * N                    h->flags_P
//   k_dynamics<false>                    st        dyn_blocks               P, ROLE_MAIN
//   k_await(BEGIN)                       s_side    1                        Pbegin
//   [k_await(BEGIN)]                     s_defer   1                        Pbegin
//   [{the pending k_flags}]              s_defer   B * N                    h->flags_P
//   [k_collide pass 0, k_post(COL)]      s_defer   B, 1                     Pbegin
//   k_list_chain<true>                   s_side    lg_con                   Pside, list_envs_per_block 1 (both lists)
//   k_flags_list (no fiv)                s_side    lg_flags                 Pside
//   raster 6 (list)                      s_side    B or 2B slots, vg_con    Pside, flags_blocks fiv_c
//   k_post(SIDE)                         s_side    1                        Pside
//   k_list_chain<false>                  st        ga + gb                  P, ROLE_DEFERRED; P, ROLE_RESPAWN, list_envs_per_block 1
//   k_flags_list (no fiv)                st        lg_flags                 P, ROLE_DEFERRED
//   k_flags (flags_on_caller)            st        B * N                    P, ROLE_MAIN
//   raster 7 (list)                      st        B or 2B slots            P, ROLE_DEFERRED_RESPAWN (no auto_reset: ROLE_DEFERRED), await_tail 1, flags_blocks fiv
//   k_await(DYN)                         s_defer   1                        P, ROLE_MAIN
//   k_viewprep_verdict (defer_flags) | k_flags_viewprep (vif) | k_flags     s_defer   dyn_blocks + B | dyn_blocks + B * N | B * N     P, ROLE_MAIN
//   raster 2                             s_defer   B                        P, ROLE_MAIN, use_vorder 1
//   k_post(MAIN)                         s_defer   1                        P, ROLE_MAIN
//   not drawn: k_await(SIDE, MAIN)       st        1                        P, ROLE_MAIN
//   h->flags_P (defer_flags: launched by the next step or flush_flags): P, ROLE_MAIN, part_next null, flags_deferred 0
static void step_phase_words(mcr_env* h, const McrParams& Pin, const StepGrids& g, hipStream_t st, int view_flags) {
  const int B = Pin.B, N = Pin.N, dyn_blocks = g.dyn_blocks;
  const bool draw = Pin.obs != nullptr, cc = Pin.cc_mode != 0;
  const int vif = (view_flags && draw && h->viewprep_in_flags) ? 1 : 0;
  // (not with a long contact list — a policy that drives: the contact chain, which fills the machine from the step's begin, is the step's critical
  // path then, the raster's chain has slack, and 8192 wavefronts beside the chain's first sweeps cost `--actions drive` 1.3 %, measured.  The
  // bound is an ABSOLUTE count found at B = 4096, N = 2 (random actions: ~15 contact envs, drive: ~1000) and not verified at other batch sizes;
  // it comes from a mapped host word read without synchronisation, so WHICH steps defer can differ between runs — results do not depend on it)
  const bool defer_flags = vif && cc && g.prev_contacts <= 64 && !(Pin.debug & DEBUG_FLAGS_IN_STEP);     // (DEBUG_FLAGS_IN_STEP: the scans stay in their step — A/B runs)
  const bool take_flags = cc && h->flags_pending;                      // (without cc: flushed below — mcr_step flushes for every step that cannot take the scans in: not reached)
  const McrParams P = with(Pin, ROLE_MAIN, [&](McrParams& q) { q.soft_sync = 1; q.flags_deferred = take_flags ? 1 : 0; q.split = 0; q.viewprep_in_flags = vif; });
  const McrParams Pbegin = with(P, ROLE_ALL, [](McrParams& q) { q.split = 1; q.viewprep_in_flags = 0; });     // (split: k_collide pass 0 fills part / clist)
  const McrParams Pside = with(P, ROLE_CONTACT, [](McrParams& q) { q.viewprep_in_flags = 0; });
  if (!cc) LAUNCH_LDS(0, k_collide, B, 64, col::lds_bytes(N), st, Pbegin, 0);
  // The step's critical kernel goes out FIRST (round 6): everything the other two streams run in this step waits for a word the dynamics posts
  // (BEGIN from its first thread), so the order of enqueueing across the streams is free — and behind a host synchronisation (an RL loop
  // reads its observations every step) the seven launches that used to precede it cost the step their enqueue time, ~45 us.
  if (h->flags_pending && !cc) flush_flags(h, st);
  LAUNCH(1, k_dynamics<false>, dyn_blocks, 64, st, with(P, ROLE_MAIN), 0);          // (the main envs: no touching car<->car pair)
  hipLaunchKernelGGL(k_await, dim3(1), dim3(64), 0, h->s_side, Pbegin, (int)W_BEGIN, -1);
  if (cc) {
    // the contact pass of the main envs on the THIRD stream (idle until the dynamics is through), the contact chain — each workgroup with its
    // env's own contact pass in front (fuse_collide) — on the side stream from the step's begin: the chain, the step's critical path when cars
    // pile up, does not wait for the 4096-env launch
    hipLaunchKernelGGL(k_await, dim3(1), dim3(64), 0, h->s_defer, Pbegin, (int)W_BEGIN, -1);
    if (take_flags) flush_flags(h, h->s_defer);                      // the last step's main envs' bookkeeping: beside this step's main dynamics
    LAUNCH_LDS(0, k_collide, B, 64, col::lds_bytes(N), h->s_defer, Pbegin, 0);
    hipLaunchKernelGGL(k_post, dim3(1), dim3(64), 0, h->s_defer, Pbegin, (int)W_COL);
  }
  { const McrParams Pc = with(Pside, ROLE_CONTACT, [](McrParams& q) { q.list_envs_per_block = 1; }); LAUNCH_LDS(5, k_list_chain<true>, g.lg_con, 64, col::lds_bytes(N), h->s_side, Pc, Pc, 0, g.lg_con); }   // ONE contact env per wavefront: the uniform contact sweeps (k_dynamics.h)
  // (the chains' bookkeeping: workgroups of its own inside the chain's raster launch when there is one, a list launch otherwise)
  // (beyond four cars per env the lists hold thousands of cars — ~315 contact envs x 8 at N = 8 — and a few 256-thread workgroups
  // would take them in many rounds at the end of the contact chain, the critical path there; measured N = 2 15.37 -> 15.65 M
  // env-steps/s, N = 4 11.00 -> 11.07, N = 8 5.47 -> 5.44)
  const int fiv = (view_flags && draw && N <= 8) ? (N <= 2 ? 8 : 64) : 0;
  // (the contact list's bookkeeping workgroups: sized by the LAST step's list, like the raster's — StepGrids::vg_con)
  const int fiv_c = fiv ? std::min(512, std::max(fiv, (g.prev_contacts * (N + 1) + 3) / 4 + 2)) : 0;
  if (view_flags && !fiv) hipLaunchKernelGGL(k_flags_list, dim3(g.lg_flags), dim3(64), 0, h->s_side, Pside);
  if (draw) launch_view(h, 6, P.term_cnt ? 2 * B : B, h->s_side, with(Pside, ROLE_CONTACT, [&](McrParams& q) { q.flags_blocks = fiv_c; }), 0, nullptr, g.vg_con);
  hipLaunchKernelGGL(k_post, dim3(1), dim3(64), 0, h->s_side, Pside, (int)W_SIDE);
  const bool flags_on_caller = view_flags && draw && !vif && N <= 7;   // (N = 8: the raster would share the machine with the bookkeeping: 6.70 -> 6.49 M env-steps/s, round 5)
  LAUNCH_LDS(7, k_list_chain<false>, g.ga + g.gb, 64, col::lds_bytes(N), st, with(P, ROLE_DEFERRED), with(P, ROLE_RESPAWN, [](McrParams& q) { q.list_envs_per_block = 1; }), 0, g.ga);
  if (view_flags && !fiv) hipLaunchKernelGGL(k_flags_list, dim3(g.lg_flags), dim3(64), 0, st, with(P, ROLE_DEFERRED));
  // Beyond three cars per env the third stream's chain (bookkeeping of B*N cars, then B*N views) is the longer one and the caller's
  // has slack: the main envs' bookkeeping — which the raster does not depend on — moves here, between the resume chain and its raster
  if (flags_on_caller) launch_flags(st, with(P, ROLE_MAIN));
  // ... and the step's join (+ the terminal entries' frames and count)
  if (draw) launch_view(h, 7, P.term_cnt ? 2 * B : B, st, with(P, P.auto_reset ? ROLE_DEFERRED_RESPAWN : ROLE_DEFERRED, [&](McrParams& q) { q.await_tail = 1; q.flags_blocks = fiv; }), 0);
  hipLaunchKernelGGL(k_await, dim3(1), dim3(64), 0, h->s_defer, with(P, ROLE_MAIN), (int)W_DYN, -1);
  if (defer_flags) {
    // view records + the marked envs' touch verdicts; the flag scans: the next step's begin (or flush_flags)
    hipLaunchKernelGGL(k_viewprep_verdict, dim3(dyn_blocks + B), dim3(64), 0, h->s_defer, with(P, ROLE_MAIN), dyn_blocks);
    h->flags_P = with(P, ROLE_MAIN, [](McrParams& q) { q.part_next = nullptr; q.flags_deferred = 0; }); h->flags_pending = true;
  }
  else if (vif) hipLaunchKernelGGL(k_flags_viewprep, dim3(dyn_blocks + B * N), dim3(64), 0, h->s_defer, with(P, ROLE_MAIN), dyn_blocks);      // view records + bookkeeping: one launch
  else if (view_flags && !flags_on_caller) launch_flags(h->s_defer, with(P, ROLE_MAIN));
  if (draw) launch_view(h, 2, B, h->s_defer, with(P, ROLE_MAIN, [](McrParams& q) { q.use_vorder = 1; }), 0);
  hipLaunchKernelGGL(k_post, dim3(1), dim3(64), 0, h->s_defer, with(P, ROLE_MAIN), (int)W_MAIN);
  if (!draw) hipLaunchKernelGGL(k_await, dim3(1), dim3(64), 0, st, with(P, ROLE_MAIN), (int)W_SIDE, (int)W_MAIN);
}

// The three chains ordered by events:
//   st      : -+-> dynamics(main envs, 3 position sweeps) -+-> chain(resume the deferred envs || reset pass of the re-spawned envs) -> their raster -+
//   s_side  :  +-> collide(all) -> chain(contact envs) -> their raster ---------------------------------------------------------------------------+
//   s_defer :                                              +-> view records, bookkeeping(main envs) -> raster(main envs) -------------------------+
// Where the kernel an event marks is known, the launch completes the event itself (hipExtLaunchKernelGGL's stop event:
// the dispatch packet's own completion signal).  A hipEventRecord is a marker packet BEHIND the kernel: +3 us before the next
// kernel of the same stream, 11 instead of 7.5 us for a dependent kernel on another stream (tools/ubench/event_gap.hip), and the
// step has four of them on its critical path.  Not inside a graph capture (plain records there).
// The launches in enqueue order.  P: launch_step's block with split 0 and viewprep_in_flags vif.  Pbegin, Pside: as in step_phase_words.
//   launch                               stream              grid                     block
//   k_collide pass 0                     st (cc: s_side)     B                        Pbegin
//   k_list_chain<true>                   s_side              lg_con                   Pside, list_envs_per_block 1 (both lists)
//   k_flags_list (flags_list)            s_side              lg_flags                 Pside
//   raster 6 (list)                      s_side              B or 2B slots, vg_con    Pside
//   k_dynamics<false>                    st                  dyn_blocks               P, ROLE_MAIN
//   k_list_chain<false>                  st                  ga + gb                  P, ROLE_DEFERRED; P, ROLE_RESPAWN, list_envs_per_block 1
//   k_flags_list (flags_list)            st                  lg_flags                 P, ROLE_DEFERRED
//   raster 7 (list)                      st                  B or 2B slots            P, ROLE_DEFERRED_RESPAWN (no auto_reset: ROLE_DEFERRED)
//   k_viewprep (vif), k_flags            s_defer             dyn_blocks, B * N        P, ROLE_MAIN
//   raster 2                             s_defer             B                        P, ROLE_MAIN, use_vorder 1
//   terminal entries: k_term_finish      st                  1                        P, ROLE_MAIN
static void step_events(mcr_env* h, const McrParams& Pin, const StepGrids& g, hipStream_t st, int view_flags) {
  const int B = Pin.B, N = Pin.N, dyn_blocks = g.dyn_blocks;
  const bool draw = Pin.obs != nullptr, cc = Pin.cc_mode != 0;
  const bool sev = h->use_graph <= 0 && !capturing(st);
  // the main envs' view records and car polygons: by k_viewprep on the third stream, in front of the bookkeeping kernel, in a drawn step
  // with actions; otherwise by the dynamics' own epilogue
  const int vif = (view_flags && draw && h->viewprep_in_flags) ? 1 : 0;
  const McrParams P = with(Pin, ROLE_MAIN, [&](McrParams& q) { q.split = 0; q.viewprep_in_flags = vif; });
  const McrParams Pbegin = with(P, ROLE_ALL, [](McrParams& q) { q.split = 1; q.viewprep_in_flags = 0; });     // (split: k_collide pass 0 fills part / clist)
  const McrParams Pside = with(P, ROLE_CONTACT, [](McrParams& q) { q.viewprep_in_flags = 0; });
#define STOP(ev) (sev ? (ev) : (hipEvent_t) nullptr)
#define RECORD_UNLESS_STOP(ev, stream) do { if (!sev) (void)hipEventRecord(ev, stream); } while (0)
  if (!cc) LAUNCH_LDS_STOP(0, k_collide, B, 64, col::lds_bytes(N), st, STOP(h->ev_col), Pbegin, 0);
  (void)hipEventRecord(h->ev_fork, st);
  (void)hipStreamWaitEvent(h->s_side, h->ev_fork, 0);
  if (cc) LAUNCH_LDS_STOP(0, k_collide, B, 64, col::lds_bytes(N), h->s_side, STOP(h->ev_col), Pbegin, 0);
  RECORD_UNLESS_STOP(h->ev_col, cc ? h->s_side : st);
  // bookkeeping of a chain's cars: fused into the chain for N <= 2 (2 envs x N cars take their turns on one wavefront),
  // a list launch of its own beyond that
  const int fuse_flags = (view_flags && N <= 2) ? 1 : 0;
  const bool flags_list = view_flags && !fuse_flags;
  // (the side stream's last kernel completes ev_join; which one that is depends on the step's shape)
  { const McrParams Pc = with(Pside, ROLE_CONTACT, [](McrParams& q) { q.list_envs_per_block = 1; }); LAUNCH_LDS_STOP(5, k_list_chain<true>, g.lg_con, 64, col::lds_bytes(N), h->s_side, STOP((!draw && !flags_list) ? h->ev_join : nullptr), Pc, Pc, fuse_flags, g.lg_con); }
  if (flags_list) hipExtLaunchKernelGGL(k_flags_list, dim3(g.lg_flags), dim3(64), 0, h->s_side, nullptr, STOP(!draw ? h->ev_join : nullptr), 0, Pside);
  if (draw) launch_view(h, 6, P.term_cnt ? 2 * B : B, h->s_side, Pside, 0, STOP(h->ev_join), g.vg_con);
  LAUNCH_LDS_STOP(1, k_dynamics<false>, dyn_blocks, 64, 0, st, STOP(h->ev_fork2), with(P, ROLE_MAIN), 0);
  RECORD_UNLESS_STOP(h->ev_fork2, st);
  // The chain that follows the dynamics IN-STREAM starts ~2 us after it, one that has to hop to another stream ~8 us (kernel trace,
  // round 3).  The longer chain is the resume chain (85-150 us beside the raster + its own raster, 25-70 us) — not bookkeeping + main
  // raster (40 + 100 us): it keeps the caller's stream and gets its wavefronts placed before the raster starts (a chain that starts
  // beside a raster that fills every CU runs 2-3x slower); the main envs' bookkeeping + raster take the hop to the third stream.
  (void)hipStreamWaitEvent(h->s_defer, h->ev_fork2, 0);
  (void)hipStreamWaitEvent(st, h->ev_col, 0);              // the resume chain reads the contact pass's results of its envs (a deferred env never got to the main dynamics' in-kernel wait)
  if (!draw) (void)hipStreamWaitEvent(h->s_side, h->ev_fork2, 0);
  // the resume chain and — same launch, workgroups of their own — the reset pass (:408, ~50 us of serial solver work) of the
  // envs the main dynamics re-spawned (one per workgroup: they run side by side); then, in one list launch, the deferred envs' frames and
  // the re-spawned envs' first observations (the caller's stream needs no event for its own chain)
  LAUNCH_LDS(7, k_list_chain<false>, g.ga + g.gb, 64, col::lds_bytes(N), st, with(P, ROLE_DEFERRED), with(P, ROLE_RESPAWN, [](McrParams& q) { q.list_envs_per_block = 1; }), fuse_flags, g.ga);
  if (flags_list) hipLaunchKernelGGL(k_flags_list, dim3(g.lg_flags), dim3(64), 0, st, with(P, ROLE_DEFERRED));
  if (draw) launch_view(h, 7, P.term_cnt ? 2 * B : B, st, with(P, P.auto_reset ? ROLE_DEFERRED_RESPAWN : ROLE_DEFERRED), 0);
  RECORD_UNLESS_STOP(h->ev_join, h->s_side);
  // The bookkeeping of the main envs (:446-495; k_flags.h, one wavefront per car) needs the poses only.  It runs right
  // before the raster, and those ~16 us are what the list chains — forked off at the same moment — need to get their
  // wavefronts placed: a chain that starts beside a raster that already fills every CU runs 2-3x slower (measured).
  // (k_viewprep in front of it, in-stream: the side stream may be held by a long contact chain, and a further stream slows every queue)
  const hipEvent_t main_done = h->ev_join2;
  if (vif) hipLaunchKernelGGL(k_viewprep, dim3(dyn_blocks), dim3(64), 0, h->s_defer, with(P, ROLE_MAIN));
  if (view_flags) hipExtLaunchKernelGGL(k_flags, dim3(B * N), dim3(64), 0, h->s_defer, nullptr, STOP(!draw ? main_done : nullptr), 0, with(P, ROLE_MAIN));
  (void)hipStreamWaitEvent(h->s_defer, h->ev_col, 0);              // the raster reads the tiles' recolour flags (long done)
  if (draw) launch_view(h, 2, B, h->s_defer, with(P, ROLE_MAIN, [](McrParams& q) { q.use_vorder = 1; }), 0, STOP(main_done));
  // the join: the caller's stream waits for the other two (waiting for them one behind the other — one wait on the caller's
  // stream — costs a second hop: 23 vs 18.5 us after the later of the two, tools/ubench/event_gap.hip)
  if (!sev || (!draw && !view_flags)) (void)hipEventRecord(h->ev_join2, h->s_defer);
  (void)hipStreamWaitEvent(st, h->ev_join, 0);
  (void)hipStreamWaitEvent(st, h->ev_join2, 0);
  if (P.term_cnt) hipLaunchKernelGGL(k_term_finish, dim3(1), dim3(256), 0, st, with(P, ROLE_MAIN));     // (the phase-word path: the join's workgroup does it)
#undef STOP
#undef RECORD_UNLESS_STOP
}

// step(): collide -> dynamics [-> auto-reset pass] -> view on the caller's stream `st`; with num_streams == 2 the step forks into three
// chains that meet again at the end, ordered by phase words (step_phase_words) or by events (step_events); grids are sized for the worst
// case, surplus workgroups exit on their first load.  Contact envs: a wavefront holding a touching car<->car pair takes 2-4x as long as
// the others.  Deferred envs: the few whose position loop is still iterating after 3 sweeps (a slow marginal crawl that would hold the
// whole main launch for up to 60).  Re-spawned envs (auto-reset, ~B/1000 per step): their reset pass would hold the raster of everybody
// else (they are not in the main raster's list, see k_dynamics).  An env of the contact or deferred list that ended its episode in this
// step (rare) takes its reset pass inside its own chain.
static void launch_step(mcr_env* h, McrParams P, hipStream_t st, int view_flags) {
  step_prologue(h, P, st);
  if (!h->split) { step_single_stream(h, P, st, view_flags); return; }
  P.defer_after = MCR_DEFER_AFTER; P.respawn_list = P.auto_reset ? 1 : 0; P.list_envs_per_block = MCR_SIDE_ENVS_PER_WAVE;
  // The contact pass runs on another stream BESIDE the main dynamics (cc_mode, mcr_kernels.h): nothing the solver needs
  // comes from it (Car.step reads the wheels' tile bits of the PREVIOUS pass; which envs are the contact chain's follows
  // from the entry poses), only the step's bookkeeping at the end of the dynamics kernel does, and that waits for
  // k_collide's per-env "done" word.  24 us + a kernel boundary off the critical path.
  // Where kernels of different streams do not overlap (mcr_create probes it: counter-collecting profilers, debuggers) the
  // contact pass simply runs first, on the caller's stream.
  P.cc_mode = cc_active(h) ? 1 : 0; P.epoch = h->step_count.load(std::memory_order_relaxed); P.epoch_ptr = nullptr;
  P.fuse_collide = fused_collide(h, st) ? 1 : 0; P.flags_deferred = 0;
  if (h->use_graph > 0) {
    // a replayed graph has constant arguments: the epoch lives in a device-side counter that the first node of the step advances
    // (before the fork: the contact pass and the dynamics read the same value)
    hipLaunchKernelGGL(k_step_begin, dim3(1), dim3(1), 0, st, h->dev_step_ctr);
    P.epoch = 0; P.epoch_ptr = h->dev_step_ctr;
  }
  const StepGrids g = step_grids(h, P);
  if (phase_words(h, st)) step_phase_words(h, P, g, st, view_flags);
  else step_events(h, P, g, st, view_flags);
}

// The kernels report conditions that make results wrong in mapped host memory (mcr_kernels.h: ST_*); read here without
// synchronising, like the install counters — a condition raised by a step that is still running shows up in a later call.
static int check_status(mcr_env* h) {
  static const char* what[MCR_STATUS_WORDS] = {
      "a kernel gave up waiting for the kernels of another stream (three-chain step: the contact pass of an env, a phase word); the handle now runs the contact pass in front and orders its streams with events",
      "the contact pass disagreed with the one-step-ahead touch verdict; the handle now runs the contact pass in front of the dynamics", "", "", "", "", "", ""};
  // FATAL: a wait that gave up, a verdict mismatch — results of that step are wrong.  The overflow words (ST_CC_OVERFLOW, ST_EVENT_OVERFLOW) are
  // documented capacity deviations (the excess was dropped and flagged): the rollout goes on, mcr_status / VecMultiCarRacing.status_words show them.
  for (int i : {(int)ST_SPIN_GIVEUP, (int)ST_VERDICT}) {
    const uint32_t v = ((volatile uint32_t*)h->status_host)[i];
    if (v != h->status_seen[i]) {
      h->status_seen[i] = v;
      if (i == ST_SPIN_GIVEUP) { h->concurrent_collide = false; h->soft_sync = false; h->verdict_fresh = false; }
      if (i == ST_VERDICT) { h->concurrent_collide = false; h->verdict_fresh = false; }     // (the contact pass in front from now on: it marks the contact chain's envs itself)
      g_err = std::string("results of an earlier step are wrong: ") + what[i] + " (" + std::to_string(v) + " so far)";
      return MCR_ERR_STATE;
    }
  }
  return MCR_OK;
}
extern "C" int mcr_status(mcr_env* h, uint32_t* out, int n_words) {
  if (!h || !out || n_words < 0) return MCR_ERR_ARG;
  for (int i = 0; i < n_words && i < MCR_STATUS_WORDS; ++i) out[i] = ((volatile uint32_t*)h->status_host)[i];
  return MCR_OK;
}

extern "C" int mcr_reset(mcr_env* h, const uint8_t* d_env_mask, uint8_t* d_obs, void* stream) {
  if (!h) { g_err = "null handle"; return MCR_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  McrParams P = h->P;
  P.reset_mask = d_env_mask; P.obs = h->cfg.obs_enabled ? d_obs : nullptr; P.actions = nullptr;
  h->ring.j = (int)((h->obs_draws + (uint64_t)h->ring.k - 1u) % (uint64_t)h->ring.k);     // the head of the last drawing step: the window stays put
  flush_flags(h, st);
  launch_pool_restage(h, st, 1);          // the first reset finds every env staged (a later one: nothing to do) ...
  launch_reset(h, P, st);
  launch_pool_restage(h, st, 1);          // ... and every env that installed gets its next episode: up to B copies, one workgroup per env
  launch_derived(h, st);
  HIPCHK(hipGetLastError());
  h->any_reset = true; h->verdict_fresh = false;
  return MCR_OK;
}

// One env step of a checked call: mcr_step's only one, or sub-step `sub` of the `repeat` of a macro-step (mcr_step_repeat; mcr_kernels.h has the
// table of what each sub-step carries).  The handle's bookkeeping — step counter, list parity, verdicts, fused list, pending scans — advances
// here, per env step.  Sub-steps in front of the last one draw nothing, write no state observation and are not replayed from the step graph.
static int step_one(mcr_env* h, const float* d_actions, uint8_t* d_obs, double* d_reward, uint8_t* d_done, uint8_t* d_trunc, hipStream_t st, int sub, int repeat) {
  const bool last = sub == repeat - 1;
  McrParams P = h->P;
  P.actions = d_actions; P.obs = (h->cfg.obs_enabled && last) ? d_obs : nullptr;
  P.reward_out = d_reward; P.done_out = d_done; P.trunc_out = d_trunc;
  P.defer_respawn = last ? 0 : 1; P.accumulate = sub > 0 ? 1 : 0;
  P.bp_fresh = h->bp_fresh ? 1 : 0; h->bp_fresh = false;
  if (P.obs) { h->ring.j = (int)(h->obs_draws % (uint64_t)h->ring.k); ++h->obs_draws; }
  h->step_count.store((int32_t)((uint32_t)h->step_count.load(std::memory_order_relaxed) + 1u), std::memory_order_relaxed);      // (wraps: epochs are compared as 32-bit distances, mcr_kernels.h)
  // with auto_reset, finished envs are re-spawned on the device and take the action-less first step of their
  // new episode inside this call; the view kernel always runs (it also owns the backward/on-grass flags)
  const int vf = d_actions ? 1 : 0;
  // the bookkeeping the last step left to this one (step_phase_words) runs beside this step's main dynamics if this is a phase-word step with
  // actions and the contact pass beside the dynamics; for any other step — single stream, events, graph capture or replay, no actions — first
  if (h->flags_pending && !(vf && h->split && cc_active(h) && phase_words(h, st))) flush_flags(h, st);
  // (the contact list of a fused step is made by the step before it, if that one was fused too: a change of mode — another caller stream, a
  // give-up — is treated like stale verdicts one way, and empties the half-made list the other way)
  const bool fz = fused_collide(h, st);
  if (h->last_fused && !fz) (void)hipMemsetAsync(h->P.clist + (size_t)h->step_parity * (P.B + 1), 0, sizeof(int32_t), st);
  // ... and into fused mode: this step's verdict writers APPEND to the other parity's list, which a fused dynamics no longer zeroes and
  // which an unfused step's contact pass filled two steps ago and nobody emptied (the next step's chain re-stepped stale envs)
  if (cc_active(h) && fz && !h->last_fused) (void)hipMemsetAsync(h->P.clist + (size_t)(h->step_parity ^ 1) * (P.B + 1), 0, sizeof(int32_t), st);
  if (cc_active(h) && (!h->verdict_fresh || (fz && !h->last_fused))) {   // after reset() / reset_envs() / a state restore / a step without actions: which envs hold a touching car<->car pair?
    McrParams Pt = P; Pt.role = ROLE_ALL; Pt.part = h->P.part + (size_t)h->step_parity * P.B;
    Pt.fuse_collide = fused_collide(h, st) ? 1 : 0; Pt.clist = h->P.clist + (size_t)h->step_parity * (P.B + 1);
    if (Pt.fuse_collide) (void)hipMemsetAsync(Pt.clist, 0, sizeof(int32_t), st);
    hipLaunchKernelGGL(k_touch, dim3(P.B), dim3(64), 0, st, Pt);
  }
  h->verdict_fresh = vf != 0;             // this step's bookkeeping evaluates the next step's
  h->last_fused = fz && vf != 0;
  bool replay = false;
  if (h->use_graph > 0 && !h->timing && repeat == 1) {
    // The step is a fixed sequence of ~13 launches on up to three streams whose arguments only change with the
    // contact-list parity: it can be replayed as a hipGraph (measured r02: 0.4 % faster — the gaps between the step's
    // dependent kernels are GPU-side drain/start-up, not host launch cost — so VecMultiCarRacing leaves it off).  Any change of an argument
    // (other buffers, another stream, debug switches) re-captures.  This branch only decides whether the step is replayed or launched.
    const int parity_before = h->step_parity;
    mcr_env::StepGraph& G = h->sg[parity_before + 2 * (P.obs ? h->ring.j : 0)];
    replay = G.valid && G.st == st && G.view_flags == vf && memcmp(&G.P, &P, sizeof(P)) == 0;
    if (replay) h->step_parity ^= 1;                    // what launch_step does on the host side
    else {
      if (G.valid) { (void)hipGraphExecDestroy(G.exec); (void)hipGraphDestroy(G.graph); G.valid = false; }
      if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess) {
        launch_step(h, P, st, vf);
        hipGraph_t graph = nullptr;
        if (hipStreamEndCapture(st, &graph) == hipSuccess && graph && hipGraphInstantiate(&G.exec, graph, nullptr, nullptr, 0) == hipSuccess) {
          G.graph = graph; G.P = P; G.st = st; G.view_flags = vf; G.valid = replay = true;
        }
        else if (graph) (void)hipGraphDestroy(graph);
      }
      if (!replay) {
        (void)hipGetLastError();
        h->use_graph = -1;                               // capture is not available here: plain launches from now on
        h->step_parity = parity_before;
      }
    }
    if (replay) HIPCHK(hipGraphLaunch(G.exec, st));
  }
  if (!replay) launch_step(h, P, st, vf);
  launch_contact_obs(h, st, sub > 0);                                    // behind EVERY sub-step, the only place a step launches it (mcr_env.h); off: one test
  if (d_actions) launch_end_rules(h, st, sub > 0);                       // early ending (k_endrules.h): counted behind every sub-step that has actions; off: one test
  if (last) launch_step_tail(h, st, d_done, d_trunc);                    // (a replayed step is a whole call: repeat == 1)
  HIPCHK(hipGetLastError());
  return MCR_OK;
}

extern "C" int mcr_step_repeat(mcr_env* h, const float* d_actions, int repeat, uint8_t* d_obs, double* d_reward, uint8_t* d_done, uint8_t* d_trunc, void* stream) {
  if (!h || !d_reward || !d_done) { g_err = "null argument"; return MCR_ERR_ARG; }
  if (repeat < 1 || repeat > MCR_REPEAT_MAX) { g_err = "mcr_step_repeat: repeat 1 .. MCR_REPEAT_MAX"; return MCR_ERR_ARG; }
  if (repeat > 1 && !d_actions) { g_err = "mcr_step_repeat: repeat > 1 needs actions (the action-less step belongs to reset)"; return MCR_ERR_ARG; }
  if (!h->any_reset) { g_err = "step() before reset()"; return MCR_ERR_STATE; }
  if (h->ring.k > 1 && !d_obs) { g_err = "mcr_step: a stacked observation format needs d_obs every step (a skipped draw leaves a hole in the ring)"; return MCR_ERR_ARG; }
  if (repeat > 1 && h->term_slab) { g_err = "mcr_step_repeat: repeat > 1 with terminal observations is not supported (the terminal frame would be drawn in a sub-step that draws nothing)"; return MCR_ERR_STATE; }
  if (int rc = check_status(h)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (h->use_graph <= 0) {
    // a step captured by the CALLER cannot be replayed: its launches carry this step's epoch and list parity as constants.  The supported
    // way to replay a step is mcr_set_step_graph (the handle captures both parities itself and keeps the epoch in device memory).
    if (capturing(st)) { g_err = "mcr_step inside a stream capture: use mcr_set_step_graph for graph replay"; return MCR_ERR_STATE; }
  }
  for (int sub = 0; sub < repeat; ++sub)
    if (int rc = step_one(h, d_actions, d_obs, d_reward, d_done, d_trunc, st, sub, repeat)) return rc;
  return MCR_OK;
}
extern "C" int mcr_step(mcr_env* h, const float* d_actions, uint8_t* d_obs, double* d_reward, uint8_t* d_done, uint8_t* d_trunc, void* stream) {
  return mcr_step_repeat(h, d_actions, 1, d_obs, d_reward, d_done, d_trunc, stream);
}

// Phase words need the caller's stream and the two internal ones on hardware queues of their own: a waiting kernel at the head of a shared
// queue would hold back the very kernel it waits for (HIP multiplexes streams of one priority over a few queues; the internal streams are
// high-priority ones, so an ordinary caller's stream never shares theirs).  Checked HERE, once per stream, with two probe kernels and
// device synchronisations (~1 ms) — never inside mcr_step, which launches and returns.
extern "C" int mcr_bind_stream(mcr_env* h, void* stream) {
  if (!h) { g_err = "null handle"; return MCR_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  for (const auto& b : h->bound) if (b.first == st) return MCR_OK;
  // (a pending bookkeeping launch stays pending: nothing orders `st` behind the stream the last step ran on yet, and the next mcr_step takes
  // the scans in or flushes them on its own stream, ordered like the step itself)
  bool ok = false;
  if (h->split && h->soft_sync) {
    if (capturing(st)) { g_err = "mcr_bind_stream on a capturing stream"; return MCR_ERR_STATE; }
    HIPCHK(hipSetDevice(h->cfg.device));
    ok = kernels_overlap(h->s_side, st) && kernels_overlap(h->s_defer, st);
    // ... and of every other phase-word handle of the device: their awaits must not sit in front of this stream's posts either
    std::lock_guard<std::mutex> lk(g_soft_mu);
    for (mcr_env* o : g_soft_list) if (ok && o != h && o->cfg.device == h->cfg.device) ok = kernels_overlap(o->s_side, st) && kernels_overlap(o->s_defer, st);
  }
  if (h->bound.size() >= 64) h->bound.erase(h->bound.begin());
  h->bound.emplace_back(st, ok);
  return MCR_OK;
}

extern "C" int mcr_set_terminal_obs(mcr_env* h, uint8_t* d_term_obs, int32_t* d_term_ids, int32_t* d_term_count, int cap) {
  if (!h) { g_err = "null handle"; return MCR_ERR_ARG; }
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipDeviceSynchronize());
  for (auto& g : h->sg) if (g.valid) { (void)hipGraphExecDestroy(g.exec); (void)hipGraphDestroy(g.graph); g.valid = false; }
  if (h->term_slab) { (void)hipFree(h->term_slab); h->term_slab = nullptr; }
  McrParams& P = h->P;
  P.term_obs = nullptr; P.term_ids = nullptr; P.term_count_out = nullptr; P.term_cap = 0; P.term_idx = nullptr;
  if (!d_term_obs && !d_term_ids && !d_term_count) return MCR_OK;                      // off
  if (!d_term_obs || !d_term_ids || !d_term_count || cap < 1) { g_err = "mcr_set_terminal_obs: all three buffers and cap >= 1, or all null"; return MCR_ERR_ARG; }
  if (!h->cfg.obs_enabled || !h->cfg.auto_reset) { g_err = "terminal observations need obs_enabled and auto_reset"; return MCR_ERR_STATE; }
  cap = std::min(cap, h->cfg.num_envs);
  const size_t N = h->cfg.num_agents, CN = (size_t)cap * N, B = h->cfg.num_envs;
  size_t off = 0;
  auto carve = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
  const size_t o_cnt = carve(sizeof(int32_t) * 8), o_list = carve(sizeof(int32_t) * 4 * cap), o_idx = carve(sizeof(int32_t) * B);
  const size_t o_carf = carve(sizeof(float) * CF_COUNT * CN), o_card = carve(sizeof(double) * CD_COUNT * CN);
  const size_t o_vp = carve(sizeof(float) * MCR_VIEWP_FLOATS * CN), o_cp = carve(sizeof(float) * MCR_CARPOLY_FLOATS * CN);
  const size_t o_tf = carve(sizeof(uint16_t) * MCR_TILE_CAP * (size_t)cap), o_te = carve(sizeof(McrTermEnv) * cap);
  if (hipMalloc(&h->term_slab, off) != hipSuccess) { h->term_slab = nullptr; g_err = "hipMalloc failed"; return MCR_ERR_HIP; }
  uint8_t* base = (uint8_t*)h->term_slab;
  HIPCHK(hipMemset(base, 0, off));
  HIPCHK(hipMemset(base + o_idx, 0xff, sizeof(int32_t) * B));
  HIPCHK(hipMemset(d_term_count, 0, sizeof(int32_t)));
  h->term_cnt2 = (int32_t*)(base + o_cnt); h->term_list2 = (int32_t*)(base + o_list);
  P.term_obs = d_term_obs; P.term_ids = d_term_ids; P.term_count_out = d_term_count; P.term_cap = cap;
  P.term_idx = (int32_t*)(base + o_idx); P.term_carf = (float*)(base + o_carf); P.term_card = (double*)(base + o_card);
  P.term_viewp = (float*)(base + o_vp); P.term_carpoly = (float*)(base + o_cp); P.term_tflags = (uint16_t*)(base + o_tf); P.term_env = (McrTermEnv*)(base + o_te);
  return MCR_OK;
}

extern "C" int mcr_set_obs_format(mcr_env* h, int format, int stack) {
  if (!h) { g_err = "null handle"; return MCR_ERR_ARG; }
  if ((format != MCR_OBS_RGB && format != MCR_OBS_GRAY) || stack < 1 || stack > MCR_OBS_STACK_MAX || (format == MCR_OBS_RGB && stack != 1)) {
    g_err = "mcr_set_obs_format: format MCR_OBS_RGB with stack 1, or MCR_OBS_GRAY with stack 1 .. MCR_OBS_STACK_MAX"; return MCR_ERR_ARG;
  }
  if (!h->cfg.obs_enabled) { g_err = "mcr_set_obs_format needs obs_enabled"; return MCR_ERR_STATE; }
  if (h->any_reset) { g_err = "mcr_set_obs_format after the first mcr_reset"; return MCR_ERR_STATE; }
  if (h->term_slab) { g_err = "mcr_set_obs_format after mcr_set_terminal_obs: set the format first (it shapes the terminal entries)"; return MCR_ERR_STATE; }
  HIPCHK(hipSetDevice(h->cfg.device));
  if (h->ring.fresh) { (void)hipFree(h->ring.fresh); h->ring.fresh = nullptr; }
  const size_t bn = (size_t)h->cfg.num_envs * h->cfg.num_agents;
  if (stack > 1) {
    if (hipMalloc(&h->ring.fresh, bn) != hipSuccess) { h->ring.fresh = nullptr; g_err = "hipMalloc failed"; return MCR_ERR_HIP; }
    HIPCHK(hipMemset(h->ring.fresh, 0, bn));
  }
  h->obs_gray = format == MCR_OBS_GRAY; h->ring.k = stack; h->ring.j = 0;
  return MCR_OK;
}
extern "C" size_t mcr_obs_bytes_per_view(const mcr_env* h) {
  if (!h) return 0;
  return !h->obs_gray ? (size_t)96 * 96 * 3 : (size_t)96 * 96 * (h->ring.k > 1 ? 2 * h->ring.k : 1);
}
extern "C" int mcr_obs_window(const mcr_env* h) {
  if (!h) { g_err = "null handle"; return MCR_ERR_ARG; }
  return h->ring.k > 1 ? (int)((h->obs_draws + (uint64_t)h->ring.k - 1u) % (uint64_t)h->ring.k) + 1 : 0;
}

extern "C" int mcr_set_step_graph(mcr_env* h, int enable) {
  if (!h) { g_err = "null handle"; return MCR_ERR_ARG; }
  if (enable && h->use_graph <= 0) {     // the device-side epoch counter continues the host's (both advance once per step from here on)
    HIPCHK(hipDeviceSynchronize());
    const int32_t steps = h->step_count.load(std::memory_order_relaxed);
    HIPCHK(hipMemcpy(h->dev_step_ctr, &steps, sizeof(int32_t), hipMemcpyHostToDevice));
  }
  h->use_graph = enable ? 1 : 0;
  return MCR_OK;
}

extern "C" int mcr_render(mcr_env* h, int env, int width, int height, uint8_t* d_out, void* stream) {
  if (!h || !d_out) { g_err = "null argument"; return MCR_ERR_ARG; }
  if (env < 0 || env >= h->cfg.num_envs || width < 1 || height < 1 || width > 4096 || height > 4096) { g_err = "env / viewport out of range"; return MCR_ERR_ARG; }
  if (!h->any_reset) { g_err = "render() before reset()"; return MCR_ERR_STATE; }
  if (!h->cfg.obs_enabled) { g_err = "render() needs obs_enabled (the camera and car polygons are produced for the observation path)"; return MCR_ERR_STATE; }
  McrParams P = h->P;
  flush_flags(h, (hipStream_t)stream);                    // (k_render.h reads CU_FLAGS itself: the frame shows the CURRENT flags)
  const dim3 grid((width + RENDER_TILE - 1) / RENDER_TILE, (height + RENDER_TILE - 1) / RENDER_TILE, P.N);
  hipLaunchKernelGGL(k_render_frame, grid, dim3(256), 0, (hipStream_t)stream, P, env, width, height, d_out);
  HIPCHK(hipGetLastError());
  return MCR_OK;
}

extern "C" int mcr_read_rollout_stats(mcr_env* h, double* out2, int reset) {
  if (!h || !out2) { g_err = "null argument"; return MCR_ERR_ARG; }
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out2, h->P.stats, sizeof(double) * 2, hipMemcpyDeviceToHost));
  if (reset) HIPCHK(hipMemset(h->P.stats, 0, sizeof(double) * 2));
  return MCR_OK;
}

extern "C" int mcr_set_episode_stats(mcr_env* h, double* d_ep_return, int32_t* d_ep_len) {
  if (!h) { g_err = "null handle"; return MCR_ERR_ARG; }
  h->P.ep_return_out = d_ep_return; h->P.ep_len_out = d_ep_len;
  return MCR_OK;
}
