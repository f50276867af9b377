// k_viewprep.h — the memory-fed callers of view_record (k_carview.h): a car's view record and draw polygons from the pose in the SoA arrays,
// for the steps and envs whose dynamics does not produce them from its registers.
// k_viewprep / k_flags_viewprep: the main envs of the three-chain step at N <= 3 — a kernel of its own instead of the last 12 us of the
// step's longest kernel (k_dynamics' epilogue: one lane per car, eight f64 sin/cos): it runs on the third stream in front of the main envs'
// bookkeeping kernel and raster, whose chain has slack (the step's critical path after the dynamics is the resume chain, on the caller's
// stream).  One lane per car like the epilogue (a wavefront per car was tried: 8192 wavefronts each issuing the whole f64 camera code for
// one car cost k_flags 20 us).
#pragma once
#include "k_carview.h"

__device__ __forceinline__ void viewprep_car(const McrShapes& S, const float* __restrict__ carf, const double* __restrict__ card, const int stride, const int ci,
                                             float* __restrict__ viewp, float* __restrict__ carpoly, const double h_ratio, const double t_now, const uint32_t parts = CARVIEW_ALL) {
  view_record(S, car_pose_load(carf, card, stride, ci, parts), t_now, h_ratio, viewp + (size_t)ci * MCR_VIEWP_FLOATS, carpoly + (size_t)ci * MCR_CARPOLY_FLOATS, parts);
}

// one lane per car of the main launch's envs (ROLE_MAIN semantics: not the contact chain's, not the deferred, not the re-spawned ones)
__device__ __forceinline__ void viewprep_block(const McrParams& p, const int blk) {
  const int g = blk * 64 + threadIdx.x;
  const int env = mcr_env_of_slot(p, g / p.G), agent = g % p.G;
  if (env >= p.env0 + p.nenv || agent >= p.N) return;
  const McrEnvState es = p.env[env];
  if (!es.active || es.just_reset) return;
  viewprep_car(*p.shapes, p.carf, p.card, p.BN, env * p.N + agent, p.viewp, p.carpoly, p.h_ratio, es.t);
}
// The view records and car polygons of a list chain's envs (ROLE_CONTACT / ROLE_DEFERRED, k_list_chain.h), right behind their dynamics: the chain is the
// step's critical path and its wavefront holds a handful of cars — a car's record is ten f64 sincos on ONE lane (13 us) when the car's lane
// computes it; here FIVE lanes share it (view_record's `parts`: camera + HUD + hull | wheel 0..3), reading the state the car lanes have just
// written back.
__device__ __forceinline__ void viewprep_list_block(const McrParams& p, const int blk) {
  if (p.obs == nullptr) return;
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");       // (same wavefront, same L1: the write-back above is complete and visible to the other lanes)
  const int lane = threadIdx.x & 63, ncars = p.list_envs_per_block * p.N;
  for (int base = 0; base < ncars * 8; base += 64) {
    const int w = base + lane, c = w >> 3, part = w & 7;
    if (c >= ncars || part >= 5) continue;
    const int env = mcr_env_of_slot(p, blk * p.list_envs_per_block + c / p.N);
    if (env >= p.env0 + p.nenv) continue;
    const McrEnvState es = p.env[env];
    if (!es.active || es.resetting) continue;                   // (an env that ended its episode here: the reset pass draws up its first record)
    viewprep_car(*p.shapes, p.carf, p.card, p.BN, env * p.N + c % p.N, p.viewp, p.carpoly, p.h_ratio, es.t, 1u << part);
  }
}
// Terminal entry of env `env` (if this step's dynamics made one): view records and car polygons from the state its cars ended the episode
// with (lanes 0 .. N-1), and the tiles' recolour flags before the reset pass clears them.  Called by the env's reset pass, one wavefront.
__device__ __forceinline__ void term_prepare(const McrParams& p, const int env) {
  if (p.term_idx == nullptr || env >= p.env0 + p.nenv) return;
  const McrEnvState es = p.env[env];
  if (!es.active || !es.resetting) return;
  const int tidx = p.term_idx[env];
  if (tidx < 0) return;
  const int lane = threadIdx.x & 63;
  const uint32_t* __restrict__ src = (const uint32_t*)(p.tile_flags + (size_t)env * MCR_TILE_CAP);
  uint32_t* __restrict__ dst = (uint32_t*)(p.term_tflags + (size_t)tidx * MCR_TILE_CAP);
  for (int i = lane; i < MCR_TILE_CAP / 2; i += 64) dst[i] = src[i];
  if (lane < p.N) viewprep_car(*p.shapes, p.term_carf, p.term_card, p.term_cap * p.N, tidx * p.N + lane, p.term_viewp, p.term_carpoly, p.h_ratio, p.term_env[tidx].t);
}
__global__ __launch_bounds__(64) void k_viewprep(McrParams p) { viewprep_block(p, (int)blockIdx.x); }
// mcr_obs_now: one lane per car of EVERY active env (ROLE_ALL semantics: no partition mark, and an env no step has followed since its reset
// is not skipped) — the record and polygons of the state as it stands, the label's value and the flag word as they stand (what a
// render("state_pixels") between two steps shows: the current reward, the current driving_backward)
__global__ __launch_bounds__(64) void k_viewprep_now(McrParams p) {
  const int ci = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (ci >= p.BN) return;
  const McrEnvState es = p.env[ci / p.N];
  if (!es.active) return;
  viewprep_car(*p.shapes, p.carf, p.card, p.BN, ci, p.viewp, p.carpoly, p.h_ratio, es.t);
  view_score(p.viewp + (size_t)ci * MCR_VIEWP_FLOATS, p.card[CD_REWARD * p.BN + ci], p.caru[CU_FLAGS * p.BN + ci]);
}
