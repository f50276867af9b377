// mcr_refill.hip — who tells the host that an env consumed its staged episode (mcr_poll_consumed) and the native refill service built on it
// (mcr_refill_*, include/mcr.h).  Host code only: it launches no kernel of its own and stages through stage_rows (mcr_hip.hip).
#include "mcr_env.h"
#include <algorithm>
#include <atomic>
#include <deque>
#include <mutex>
#include <thread>
#include <unistd.h>
#include <sys/prctl.h>

extern "C" int mcr_poll_consumed(mcr_env* h, int32_t* env_ids_out, int cap, void* stream) {
  if (!h) return MCR_ERR_ARG;
  if (h->pool.blobs) { g_err = "mcr_poll_consumed: the handle stages its episodes from a level pool (mcr_set_episode_pool)"; return MCR_ERR_STATE; }
  if (h->svc) { g_err = "mcr_poll_consumed: the handle's refill service owns the counters (mcr_refill_start)"; return MCR_ERR_STATE; }
  (void)stream;   // counters live in mapped host memory: no device synchronisation needed
  int n = 0;
  const int B = h->cfg.num_envs;
  for (int e = 0; e < B; ++e) {
    int32_t c = ((volatile int32_t*)h->consumed_host)[e];
    if (c != h->consumed_seen[e]) {
      if (n < cap && env_ids_out) { env_ids_out[n] = e; h->consumed_seen[e] = c; ++n; }
      else if (!env_ids_out) ++n;
    }
  }
  return n;
}

// ---------------------------------------------------------------------------- the refill service
// What VecMultiCarRacing's Python worker did every step — poll the consumed-episode counters, generate the next episode of every env that
// re-spawned (its own RNG streams), stage it — as native threads of the handle: a service thread (polls, queues env ids, stages finished
// tracks) and up to six generator threads (one track at a time off the queue).  No interpreter, no GIL hand-offs, no gather / scatter of RNG
// states, no bounce buffer (the env's row of the caller's pinned blob array is the staging source), no condition variable or per-batch barrier
// on the path.  Host share of a rank: bench.py --emulate-world 8.  The arrays belong to the caller and must outlive the service.
// INVARIANT: the service and generator threads touch only atomics (theirs and the handle's step_count), members guarded by `qm` / `m`, the
// mapped consumed_host words (volatile reads) and the handle's consumed_seen / their own `ids` under `m`.  They only READ what is fixed before
// they start: their own mt_* / blobs / info / st / ev, and of the handle cfg, stage_ids and the P block stage_rows hands k_mark_staged (the
// kernel uses P.env alone; against that block's setters — debug bits, episode stats, terminal obs — the copy is still formally a race).
struct RefillSvc {
  std::thread th;                      // polls the counters, hands env ids to the generators, stages what they finished
  std::vector<std::thread> gens;       // generator threads: one track at a time each, off a queue — AWAKE while there is work (they poll with
                                       // short sleeps and back off when idle): a batch handed to sleeping helpers through a condition variable
                                       // cost the wake-up latency of the slowest helper per batch, and when the helpers woke late the calling
                                       // thread generated every track itself, 0.1 ms each against 4 consumptions per 0.22 ms step — a 20-step
                                       // bench run then ended with 8 ms of host backlog (round 6, profiles/r06_driver_style_runs.txt)
  std::mutex m;                        // one service cycle at a time (the thread's, or a caller's inside mcr_refill_wait)
  std::mutex qm;                       // todo / done / inflight / err_msg
  std::deque<int32_t> todo; std::vector<int32_t> done; int inflight = 0;
  std::atomic<bool> stop{false}, hold{false};
  uint32_t* mt_track; uint32_t* mt_draw; int direction_mode, gen_threads;
  uint8_t* blobs; int32_t* info;
  hipStream_t st = nullptr; hipEvent_t ev = nullptr;
  std::vector<int32_t> ids;
  std::atomic<long long> generated{0};
  // the age of the oldest consumption that is not staged yet (mcr_refill_lag): consumptions are served first in, first out — near enough —, so the
  // oldest unserved one is the `staged`-th to arrive; seen_step[k % size] = the step count when the k-th was noticed
  std::vector<std::atomic<int32_t>> seen_step; std::atomic<long long> arrived{0}, staged{0};
  std::atomic<int> err{0}; std::string err_msg;      // err_msg: written under qm BEFORE err is stored, read under qm (refill_failed)
  long long dbg[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // (under m) last mcr_refill_wait: queued / in flight / done at entry, cycles, tracks the waiter generated, us staging, us total, generator threads
};
static int refill_fail(RefillSvc* s, int rc, const std::string& msg) { std::lock_guard<std::mutex> lk(s->qm); s->err_msg = msg; s->err.store(rc); return rc; }
static int refill_failed(RefillSvc* s) {       // the ABI calls' report of a failed service (0: it has not failed)
  const int rc = s->err.load();
  if (rc) { std::lock_guard<std::mutex> lk(s->qm); g_err = "the refill service failed: " + s->err_msg; }
  return rc;
}
// take one env off the queue and generate its track — its next episode from ITS rows of the caller's arrays (mcr_host.cpp; num_threads 1: on
// this thread); false: nothing to do
static bool refill_work_one(mcr_env* h, RefillSvc* s) {
  int32_t e = -1;
  { std::lock_guard<std::mutex> lk(s->qm); if (!s->todo.empty()) { e = s->todo.front(); s->todo.pop_front(); ++s->inflight; } }
  if (e < 0) return false;
  const int rc = mcr_episodes_generate_rows(s->mt_track, s->mt_draw, &e, 1, h->cfg.num_agents, s->direction_mode, s->blobs, s->info, 1);
  if (rc != MCR_OK) refill_fail(s, rc, "track generation failed (capacity: MCR_TILE_CAP / MCR_QUAD_CAP)");
  { std::lock_guard<std::mutex> lk(s->qm); --s->inflight; if (rc == MCR_OK) s->done.push_back(e); }
  return true;
}
static void refill_gen_main(mcr_env* h, RefillSvc* s) {
  (void)prctl(PR_SET_NAME, "mcr-gen", 0, 0, 0);
  int idle = 0;
  while (!s->stop.load()) {
    if (refill_work_one(h, s)) { idle = 0; continue; }
    ++idle;
    usleep(idle < 400 ? 50 : 500);     // (20 ms without work: an idle env costs its generators next to nothing)
  }
}
// one cycle of the service: new consumptions -> the generators' queue; finished tracks -> their envs' staged slots.  Returns what is still
// pending afterwards (queued + being generated + consumptions not yet seen: 0 = all caught up), < 0: error.  Caller holds s->m.
static int refill_cycle(mcr_env* h, RefillSvc* s, bool urgent = false) {
  const int B = h->cfg.num_envs;
  int n = 0;
  for (int e = 0; e < B; ++e) {
    const int32_t c = ((volatile int32_t*)h->consumed_host)[e];
    if (c != h->consumed_seen[e]) { h->consumed_seen[e] = c; s->ids[n++] = e; }
  }
  int m = 0, left = 0;
  {
    std::lock_guard<std::mutex> lk(s->qm);
    for (int i = 0; i < n; ++i) s->todo.push_back(s->ids[i]);
    m = (int)s->done.size();
    for (int i = 0; i < m; ++i) s->ids[i] = s->done[i];
    s->done.clear();
    left = (int)s->todo.size() + s->inflight;
  }
  { const long long a0 = s->arrived.load(); for (int i = 0; i < n; ++i) s->seen_step[(size_t)((a0 + i) % (long long)s->seen_step.size())].store(h->step_count.load(std::memory_order_relaxed), std::memory_order_relaxed); s->arrived.store(a0 + n); }
  if (s->err.load()) return s->err.load();
  if (m > 0) {
    auto fail = [&](const char* what, hipError_t e) { return refill_fail(s, MCR_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); };
    const char* what = "";
    hipError_t er = stage_rows(h, s->ids.data(), m, s->blobs, true, s->st, &what);      // the env's own row of the caller's array
    if (er != hipSuccess) return fail(what, er);
    if ((er = hipEventRecord(s->ev, s->st)) != hipSuccess) return fail("hipEventRecord", er);
    // (polled with a sleep in between: hipEventSynchronize / hipStreamSynchronize spin on this runtime — 0.8 of a core, measured in round 3 —
    // and a spinning thread takes a core from the track generators where the ranks of a node share few)
    // (urgent — a caller waits in mcr_refill_wait: poll without sleeping for the first 100 us; the copies are 0.1 MB each)
    for (int spins = 0;; ++spins) { er = hipEventQuery(s->ev); if (er == hipSuccess) break; if (er != hipErrorNotReady) return fail("hipEventQuery", er); if (!urgent || spins > 2000) usleep(30); }
    s->generated.fetch_add(m);
    s->staged.fetch_add(m);
  }
  if (left == 0) {                     // nothing queued, nothing in flight — unless a track finished meanwhile (it shows up in `done` next cycle)
    std::lock_guard<std::mutex> lk(s->qm);
    if (!(s->todo.empty() && s->inflight == 0 && s->done.empty())) left = 1;
  }
  return left;
}
static void refill_main(mcr_env* h, RefillSvc* s) {
  (void)prctl(PR_SET_NAME, "mcr-refill", 0, 0, 0);
  (void)hipSetDevice(h->cfg.device);
  while (!s->stop.load()) {
    if (!s->hold.load() && s->err.load() == 0) { std::lock_guard<std::mutex> lk(s->m); (void)refill_cycle(h, s); }
    usleep(100);                       // (a step takes 0.2 ms and an env needs hundreds of steps to end its next episode: nothing is urgent here)
  }
}
extern "C" int mcr_refill_start(mcr_env* h, uint32_t* mt_track, uint32_t* mt_draw, int direction_mode, int gen_threads, void* blobs_pinned, int32_t* episode_info) {
  if (!h || !mt_track || !mt_draw || !blobs_pinned) { g_err = "mcr_refill_start: null argument"; return MCR_ERR_ARG; }
  if (h->svc) { g_err = "mcr_refill_start: already running"; return MCR_ERR_STATE; }
  if (h->pool.blobs) { g_err = "mcr_refill_start: the handle stages its episodes from a level pool (mcr_set_episode_pool)"; return MCR_ERR_STATE; }
  HIPCHK(hipSetDevice(h->cfg.device));
  RefillSvc* s = new RefillSvc();
  s->mt_track = mt_track; s->mt_draw = mt_draw; s->direction_mode = direction_mode; s->gen_threads = std::max(1, gen_threads);
  s->blobs = (uint8_t*)blobs_pinned; s->info = episode_info; s->ids.resize(h->cfg.num_envs); s->seen_step = std::vector<std::atomic<int32_t>>((size_t)h->cfg.num_envs * 2);
  if (hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&s->ev, hipEventDisableTiming) != hipSuccess) { delete s; g_err = "mcr_refill_start: stream / event"; return MCR_ERR_HIP; }
  h->svc = s;
  s->th = std::thread(refill_main, h, s);
  const int ngen = std::max(1, std::min(s->gen_threads, 6));       // (19 k tracks/s at B = 4096, N = 2 are two of them busy; 30 k at B = 32768 three)
  for (int i = 0; i < ngen; ++i) s->gens.emplace_back(refill_gen_main, h, s);
  return MCR_OK;
}
// TODO(ADVICE r06-2): envs still queued or being generated are dropped here, their consumptions already marked seen
extern "C" int mcr_refill_stop(mcr_env* h) {
  if (!h) return MCR_ERR_ARG;
  RefillSvc* s = h->svc;
  if (!s) return MCR_OK;
  s->stop.store(true);
  if (s->th.joinable()) s->th.join();
  for (auto& g : s->gens) if (g.joinable()) g.join();
  (void)hipSetDevice(h->cfg.device);
  (void)hipStreamSynchronize(s->st);
  (void)hipStreamDestroy(s->st); (void)hipEventDestroy(s->ev);
  h->svc = nullptr;
  delete s;
  return MCR_OK;
}
// every consumption visible NOW is staged when this returns (the caller synchronised the stepping stream first if it needs "all of them");
// honours the hold switch (tests: an env that finds no staged episode freezes)
extern "C" int mcr_refill_wait(mcr_env* h) {
  if (!h) return MCR_ERR_ARG;
  RefillSvc* s = h->svc;
  if (!s) return MCR_OK;
  if (int rc = refill_failed(s)) return rc;
  if (s->hold.load()) return MCR_OK;
  HIPCHK(hipSetDevice(h->cfg.device));
  timespec t0; clock_gettime(CLOCK_MONOTONIC, &t0);
  auto us_since = [&](const timespec& a) { timespec b; clock_gettime(CLOCK_MONOTONIC, &b); return (long long)((b.tv_sec - a.tv_sec) * 1000000ll + (b.tv_nsec - a.tv_nsec) / 1000); };
  std::lock_guard<std::mutex> lk(s->m);
  { std::lock_guard<std::mutex> q(s->qm); s->dbg[0] = (long long)s->todo.size(); s->dbg[1] = s->inflight; s->dbg[2] = (long long)s->done.size(); }
  s->dbg[3] = s->dbg[4] = s->dbg[5] = 0; s->dbg[7] = (long long)s->gens.size();
  for (;;) {
    timespec tc; clock_gettime(CLOCK_MONOTONIC, &tc);
    const int left = refill_cycle(h, s, true);
    s->dbg[5] += us_since(tc); ++s->dbg[3];
    if (left < 0) { (void)refill_failed(s); return left; }
    if (left == 0) break;
    if (refill_work_one(h, s)) ++s->dbg[4]; else usleep(10);       // the waiting thread generates too: progress does not depend on how fast a sleeping generator wakes
  }
  s->dbg[6] = us_since(t0);
  return MCR_OK;
}
// steps launched since the oldest consumption that is not staged yet was noticed (0: nothing pending); < 0: the service failed
extern "C" int mcr_refill_lag(mcr_env* h) {
  if (!h || !h->svc) return 0;
  RefillSvc* s = h->svc;
  if (int rc = refill_failed(s)) return rc;
  const long long st = s->staged.load(), ar = s->arrived.load();
  if (st >= ar) return 0;
  return std::max(0, (int32_t)((uint32_t)h->step_count.load(std::memory_order_relaxed) - (uint32_t)s->seen_step[(size_t)(st % (long long)s->seen_step.size())].load(std::memory_order_relaxed)));
}
extern "C" int mcr_refill_debug(mcr_env* h, long long* out8) { if (!h || !h->svc || !out8) return MCR_ERR_STATE; std::lock_guard<std::mutex> lk(h->svc->m); for (int i = 0; i < 8; ++i) out8[i] = h->svc->dbg[i]; return MCR_OK; }
extern "C" int mcr_refill_hold(mcr_env* h, int hold) { if (!h || !h->svc) return MCR_ERR_STATE; h->svc->hold.store(hold != 0); return MCR_OK; }
extern "C" long long mcr_refill_generated(mcr_env* h) { return (h && h->svc) ? h->svc->generated.load() : 0; }
