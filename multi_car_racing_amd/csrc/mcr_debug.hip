// mcr_debug.hip — the debug readers and bench helpers of the C ABI (include/mcr.h): mcr_debug_*, mcr_timing_*, the step-ordering queries,
// and three kernels no step launches (k_synth_actions, k_sincos, k_debug_overlap).  Entry points only: no other unit calls into this one.
#define MCR_DEVICE_FUNCTIONS_ONLY          // k_collide.h: col::overlap for k_debug_overlap, not the kernel (it lives in mcr_hip.hip)
#include "mcr_env.h"
#include "k_collide.h"
#include "k_contactobs.h"
#include <algorithm>

// blockIdx.y = step offset: out[nsteps][n_cars][3]
__global__ void k_synth_actions(float* __restrict__ out, int n_cars, int N, unsigned long long seed, unsigned t, unsigned env_offset) {
  const int ci = blockIdx.x * blockDim.x + threadIdx.x;
  if (ci >= n_cars) return;
  float a[3];
  mcr_synth_action(seed, env_offset + (unsigned)(ci / N), (unsigned)(ci % N), t + blockIdx.y, a);
  float* o = out + ((size_t)blockIdx.y * n_cars + ci) * 3;
  o[0] = a[0]; o[1] = a[1]; o[2] = a[2];
}
extern "C" int mcr_synth_actions_block(mcr_env* h, float* d_actions, uint64_t seed, uint32_t t0, int nsteps, uint32_t env_offset, void* stream) {
  if (!h || !d_actions || nsteps < 1 || nsteps > 65535) { g_err = "bad argument"; return MCR_ERR_ARG; }
  hipLaunchKernelGGL(k_synth_actions, dim3((h->P.BN + 255) / 256, nsteps), dim3(256), 0, (hipStream_t)stream, d_actions, h->P.BN, h->P.N,
                     (unsigned long long)seed, t0, env_offset);
  HIPCHK(hipGetLastError());
  return MCR_OK;
}
extern "C" int mcr_synth_actions(mcr_env* h, float* d_actions, uint64_t seed, uint32_t t, uint32_t env_offset, void* stream) {
  return mcr_synth_actions_block(h, d_actions, seed, t, 1, env_offset, stream);
}

__global__ void k_sincos(const float* in, float* s, float* c, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) mcr_sincosf(in[i], &s[i], &c[i]);
}
extern "C" int mcr_sincos_device(mcr_env* h, const float* d_in, float* d_sin, float* d_cos, int n, void* stream) {
  if (!h || !d_in || !d_sin || !d_cos) return MCR_ERR_ARG;
  hipLaunchKernelGGL(k_sincos, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_in, d_sin, d_cos, n);
  HIPCHK(hipGetLastError());
  return MCR_OK;
}

// the readers: everything enqueued so far is complete, then `bytes` of device memory come back
static int read_back(void* out, const void* d_src, size_t bytes) {
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out, d_src, bytes, hipMemcpyDeviceToHost));
  return MCR_OK;
}
extern "C" int mcr_debug_read_view_scratch(mcr_env* h, int view, void* out, int nbytes) {
  if (!h || !out || view < 0 || view >= h->P.BN || nbytes < 0 || nbytes > 128) return MCR_ERR_ARG;
  return read_back(out, h->view_stamps + (size_t)view * 16, nbytes);
}
extern "C" int mcr_debug_read_counters(mcr_env* h, uint64_t* out4) {
  if (!h || !out4) return MCR_ERR_ARG;
  return read_back(out4, h->P.counters, sizeof(uint64_t) * 4);
}
extern "C" int mcr_debug_read_counters8(mcr_env* h, uint64_t* out8) {
  if (!h || !out8) return MCR_ERR_ARG;
  return read_back(out8, h->P.counters, sizeof(uint64_t) * 8);
}
extern "C" int mcr_concurrent_collide(const mcr_env* h) { return (h && h->split && h->concurrent_collide) ? 1 : 0; }
extern "C" int mcr_step_ordering(const mcr_env* h) {
  if (!h || !h->split) return 0;
  return ((h->soft_sync && h->use_graph <= 0) ? 1 : 0) | 2 | (h->soft_denied ? 4 : 0);     // (bit 1: the event path always lets the launches complete the events, outside a capture)
}
extern "C" int mcr_step_ordering_for(const mcr_env* h, void* stream) {
  if (!h || !h->split) return 0;
  const int all = mcr_step_ordering(h);
  return stream_bound(h, (hipStream_t)stream) ? all : (all & ~1);
}
extern "C" int mcr_debug_read_verdict_mismatches(mcr_env* h, uint64_t* out) {
  if (!h || !out) return MCR_ERR_ARG;
  return read_back(out, h->P.counters + 4, sizeof(uint64_t));
}
// the last step's contact partition: part_out[B] (touch verdicts it went by), clist_out[1 + B] (its contact list: count, env ids); synchronises
extern "C" int mcr_debug_read_partition(mcr_env* h, uint8_t* part_out, int32_t* clist_out) {
  if (!h || !part_out || !clist_out) return MCR_ERR_ARG;
  HIPCHK(hipDeviceSynchronize());
  const size_t B = h->cfg.num_envs, par = (size_t)(h->step_parity ^ 1);
  HIPCHK(hipMemcpy(part_out, h->P.part + par * B, B, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(clist_out, h->P.clist + par * (B + 1), sizeof(int32_t) * (B + 1), hipMemcpyDeviceToHost));
  return MCR_OK;
}
// diagnostics of the verdict protocol: fill the buffer the NEXT step's verdict writers write (its part_next) with `value` / read it back after that step
extern "C" int mcr_debug_next_verdicts(mcr_env* h, int fill_value, uint8_t* out_or_null) {
  if (!h) return MCR_ERR_ARG;
  if (!out_or_null && (fill_value & 0x100)) {     // (no synchronisation: the fill is enqueued on the null stream, in front of a step launched there)
    flush_flags(h, nullptr);                      // (the pending bookkeeping reads that buffer as the last step's partition)
    HIPCHK(hipMemsetAsync(h->P.part + (size_t)(h->step_parity ^ 1) * h->cfg.num_envs, fill_value & 0xff, h->cfg.num_envs, 0));
    return MCR_OK;
  }
  HIPCHK(sync_state(h));
  const size_t B = h->cfg.num_envs;
  if (out_or_null) { HIPCHK(hipMemcpy(out_or_null, h->P.part + (size_t)h->step_parity * B, B, hipMemcpyDeviceToHost)); }       // (after a step: the parity has flipped)
  else { HIPCHK(hipMemset(h->P.part + (size_t)(h->step_parity ^ 1) * B, fill_value, B)); }
  return MCR_OK;
}
extern "C" int mcr_debug_read_env_records(mcr_env* h, void* out, int n_bytes) {
  if (!h || !out || n_bytes < 0) return MCR_ERR_ARG;
  return read_back(out, h->P.env, std::min((size_t)n_bytes, sizeof(McrEnvState) * (size_t)h->cfg.num_envs));
}
extern "C" int mcr_debug_read_contact_counts(mcr_env* h, int32_t* out) {
  if (!h || !out) return MCR_ERR_ARG;
  HIPCHK(hipDeviceSynchronize());
  const size_t stride = MCR_CC_MAX * MCR_CC_WORDS + 4;
  HIPCHK(hipMemcpy2D(out, sizeof(int32_t), h->P.cc_store, stride * sizeof(uint32_t), sizeof(int32_t), h->cfg.num_envs, hipMemcpyDeviceToHost));
  return MCR_OK;
}
// the raw manifold stores (k_carcontacts.h: the record layout; mcr_contact_store_words: the sizes), the input of the car-contact observation's host reference
extern "C" int mcr_debug_read_contacts(mcr_env* h, uint32_t* out) {
  if (!h || !out) return MCR_ERR_ARG;
  return read_back(out, h->P.cc_store, sizeof(uint32_t) * MCR_CC_STORE_WORDS * (size_t)h->cfg.num_envs);
}
// the per-tile wheel bits the sensor pass keeps between steps (k_collide.h: touch[]); read-only
extern "C" int mcr_debug_read_tile_touch(mcr_env* h, uint32_t* out) {
  if (!h || !out) { g_err = "mcr_debug_read_tile_touch: null argument"; return MCR_ERR_ARG; }
  HIPCHK(sync_state(h));
  HIPCHK(hipMemcpy(out, h->P.tile_touch, sizeof(uint32_t) * MCR_TILE_CAP * (size_t)h->cfg.num_envs, hipMemcpyDeviceToHost));
  return MCR_OK;
}
extern "C" int mcr_debug_read_proxy_ids(mcr_env* h, int env, int32_t* out, int cap) {
  if (!h || !out || env < 0 || env >= h->cfg.num_envs) return MCR_ERR_ARG;
  if (!h->P.pid_tab) { g_err = "mcr_debug_read_proxy_ids: the handle was created with fresh_world = 1 (ids ascend in creation order)"; return MCR_ERR_STATE; }
  HIPCHK(hipDeviceSynchronize());
  std::vector<uint16_t> tab(MCR_PID_TAB); int32_t meta[4];
  HIPCHK(hipMemcpy(tab.data(), h->P.pid_tab + (size_t)env * MCR_PID_TAB, sizeof(uint16_t) * MCR_PID_TAB, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(meta, h->P.pid_meta + (size_t)env * 4, sizeof(meta), hipMemcpyDeviceToHost));
  const int T = meta[2], F = 8 * h->cfg.num_agents;
  int n = 0;
  for (int t = 0; t < T && n < cap; ++t) out[n++] = tab[t];
  for (int f = 0; f < F && n < cap; ++f) out[n++] = tab[MCR_TILE_CAP + f];
  return n;
}
extern "C" int mcr_debug_read_dynamics_stamps(mcr_env* h, uint64_t* out, int n_u64) {
  if (!h || !out) return MCR_ERR_ARG;
  return read_back(out, h->P.dbg_stamps, sizeof(uint64_t) * (size_t)n_u64);
}
// the sensor predicate of k_collide (col::overlap: SAT far-field filter + Box2D's GJK) on caller-supplied cases
__global__ void k_debug_overlap(const McrShapes* shapes, int fixture_arg, int n, const float4* __restrict__ va, const float4* __restrict__ vb,
                                const float4* __restrict__ na, const float4* __restrict__ nb, const int* __restrict__ cnt,
                                const float* __restrict__ poses, uint8_t* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const McrShapes& S = *shapes;
  const bool fixture_first = fixture_arg >= 8;                     // b2TestOverlap(fixture, tile): the car fixture holds the lower proxy id
  const int fixture = fixture_arg & 7;
  const McrPoly& P = fixture < 4 ? S.hull[fixture] : S.wheel;
  const V2 lc = fixture < 4 ? v2(S.hull_lcx, S.hull_lcy) : v2(0.0f, 0.0f);
  // the body origin is given (b2BodyDef.position); sweep.c = xf * localCenter, then the transform k_collide derives from (c, a)
  Xf x0; x0.q = rot_of(poses[i * 3 + 2]); x0.p = v2(poses[i * 3], poses[i * 3 + 1]);
  const Xf xf = xf_of(xmul(x0, lc), poses[i * 3 + 2], lc);
  float wx[8], wy[8], nx[8], ny[8];
  for (int k = 0; k < 8; ++k) { wx[k] = wy[k] = nx[k] = ny[k] = 0.0f; }
  for (int k = 0; k < P.n; ++k) { const V2 w = xmul(xf, v2(P.vx[k], P.vy[k])); const V2 nn = rmul(xf.q, v2(P.nx[k], P.ny[k])); wx[k] = w.x; wy[k] = w.y; nx[k] = nn.x; ny[k] = nn.y; }
  col::TilePoly TP; const float4 a = va[i], b = vb[i], c = na[i], d = nb[i];
  TP.n = cnt[i];
  TP.vx[0] = a.x; TP.vy[0] = a.y; TP.vx[1] = a.z; TP.vy[1] = a.w; TP.vx[2] = b.x; TP.vy[2] = b.y; TP.vx[3] = b.z; TP.vy[3] = b.w;
  TP.nx[0] = c.x; TP.ny[0] = c.y; TP.nx[1] = c.z; TP.ny[1] = c.w; TP.nx[2] = d.x; TP.ny[2] = d.y; TP.nx[3] = d.z; TP.ny[3] = d.w;
  out[i] = col::overlap(wx, wy, nx, ny, P.n, TP, a, b, &P, make_float4(xf.p.x, xf.p.y, xf.q.s, xf.q.c), fixture_first) ? 1 : 0;
}
void mcr_tile_hull(const float* fx, const float* fy, float* aabb4, float* va4, float* vb4, float* na4, float* nb4, int* count);   // mcr_host.cpp
extern "C" int mcr_debug_overlap(mcr_env* h, int n, const float* quads, const float* poses, int fixture, uint8_t* out) {
  if (!h || !quads || !poses || !out || n < 0 || fixture < 0 || (fixture & 7) > 4 || fixture > 12) { g_err = "bad argument"; return MCR_ERR_ARG; }
  if (n == 0) return MCR_OK;
  std::vector<float> hull((size_t)n * 16); std::vector<int> cnt(n);
  float* VA = hull.data(); float* VB = VA + (size_t)n * 4; float* NA = VB + (size_t)n * 4; float* NB = NA + (size_t)n * 4;
  for (int i = 0; i < n; ++i) {
    float fx[4], fy[4], box[4];
    for (int k = 0; k < 4; ++k) { fx[k] = quads[(size_t)i * 8 + 2 * k]; fy[k] = quads[(size_t)i * 8 + 2 * k + 1]; }
    mcr_tile_hull(fx, fy, box, VA + (size_t)i * 4, VB + (size_t)i * 4, NA + (size_t)i * 4, NB + (size_t)i * 4, &cnt[i]);
  }
  uint8_t* d = nullptr;
  const size_t b_hull = sizeof(float) * 16 * (size_t)n, b_cnt = sizeof(int) * (size_t)n, b_pose = sizeof(float) * 3 * (size_t)n;
  HIPCHK(hipMalloc(&d, b_hull + b_cnt + b_pose + (size_t)n));
  float* d_hull = (float*)d; int* d_cnt = (int*)(d + b_hull); float* d_pose = (float*)(d + b_hull + b_cnt); uint8_t* d_out = d + b_hull + b_cnt + b_pose;
  hipError_t e = hipMemcpy(d_hull, hull.data(), b_hull, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_cnt, cnt.data(), b_cnt, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_pose, poses, b_pose, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_debug_overlap, dim3((n + 255) / 256), dim3(256), 0, 0, h->P.shapes, fixture, n, (const float4*)d_hull, (const float4*)(d_hull + (size_t)n * 4),
                       (const float4*)(d_hull + (size_t)n * 8), (const float4*)(d_hull + (size_t)n * 12), d_cnt, d_pose, d_out);
    e = hipMemcpy(out, d_out, (size_t)n, hipMemcpyDeviceToHost);
  }
  (void)hipFree(d);
  if (e != hipSuccess) { g_err = std::string("mcr_debug_overlap: ") + hipGetErrorString(e); return MCR_ERR_HIP; }
  return MCR_OK;
}
extern "C" int mcr_debug_set(mcr_env* h, int value) { if (!h) return MCR_ERR_ARG; h->P.debug = value; return MCR_OK; }
extern "C" int mcr_timing_enable(mcr_env* h, int enable) { if (!h) return MCR_ERR_ARG; h->timing = enable; return MCR_OK; }
extern "C" int mcr_timing_read(mcr_env* h, double* ms_out, int64_t* launches_out) {
  if (!h) return MCR_ERR_ARG;
  HIPCHK(hipDeviceSynchronize());
  for (auto& t : h->pending) {
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess) { h->t_ms[t.id] += ms; h->t_n[t.id] += 1; }
    h->free_events.push_back(t.a); h->free_events.push_back(t.b);
  }
  h->pending.clear();
  for (int i = 0; i < MCR_TIMING_SLOTS; ++i) { if (ms_out) ms_out[i] = h->t_ms[i]; if (launches_out) launches_out[i] = h->t_n[i]; h->t_ms[i] = 0; h->t_n[i] = 0; }
  return MCR_OK;
}
