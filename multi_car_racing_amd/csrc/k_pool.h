// k_pool.h — level pools (include/mcr.h: mcr_set_episode_pool): the device re-stages an env's next episode itself, from K episode blobs
// that stay resident in the caller's device memory, instead of waiting for the host to generate one and copy it over PCIe.
//
// The staging protocol is the host's, with the kernel as its one owner: an env whose record says `staged_ready == 0` — it installed its
// staged episode in the reset or the step in front of this launch — gets pool[level(global env, consumed)] copied into its staged slot
// (slot ^ 1, the slot it just left), then `staged_ready = 1`.  That is all mcr_stage_episodes + k_mark_staged write, and all this kernel
// writes: not `consumed`, not consumed_host, not the current slot.  Which level an env plays in its k-th episode is mcr_pool_level_of
// (mcr_common.h), a pure function of (seed, global env, k): results do not depend on B, on the sharding or on which launch did the copy.
// `level[env]` (optional) names the pool row of the env's CURRENT episode: an env with `consumed >= 1` that needs a copy has just installed
// episode consumed - 1.
//
// Shape.  A workgroup of 256 threads owns `envs_per_group` consecutive envs (1 .. 64).  Every wavefront loads the group's records, one env
// per lane, and ballots `staged_ready == 0`: the mask is the same in all four (nobody writes the word before the barrier below), so it
// needs neither LDS nor a barrier in front of the copies.  The four wavefronts then copy the flagged envs one after the other, each env's
// 97,920 bytes as 16-byte loads and stores striding over the 256 lanes, eight loads per lane ahead of their stores (32 KiB in flight per
// workgroup: what it takes to stream from HBM / the Infinity Cache); no LDS.  After the workgroup barrier lane i of the first wavefront
// flips env i's flag.  The launch sites pick the group size (mcr_derived.hip: launch_pool_restage):
//   behind a step    MCR_POOL_GROUP = 16 envs per workgroup: at B = 4096 that is 256 workgroups, one per CU and one round.  The steady state —
//                    ~B / 1000 envs re-spawn per step — is a launch whose workgroups read 16 words and leave, and a few that copy one slot;
//                    a step in which EVERY env re-spawns (all envs in phase at the TimeLimit) still has the whole machine copying.
//   around a reset   1: one workgroup per env, up to eight per CU — 4096 copies of 96 KB are a memory-bound 0.8 GB of traffic.
// The kernel computes nothing: like k_envcopy it is judged by the width of its accesses and how many are in flight.
//
// Weighted sampling (include/mcr.h: mcr_set_level_sampler; `pool.cdf` set).  The row is mcr_pool_level_cdf's — the same hash, mapped through
// the CDF in force at THIS launch — so it cannot be recomputed when the env installs the episode (other weights may be in force then): the
// lane that flips the flag keeps it in staged_level[env], and an env that needs a copy first hands staged_level[env] — what the launch that
// staged the episode it just installed drew — to level[env].  staged_level is staging state like `staged_ready`: snapshots leave it alone.
// k_level_cdf (below) rewrites the CDF in stream order: one wavefront, the running sum in index order (mcr_common.h has the definition).
#pragma once
#include "mcr_kernels.h"

#define MCR_POOL_LANES 256
#define MCR_POOL_GROUP 16          // envs per workgroup of the launch behind a step
#define MCR_POOL_AHEAD 8           // 16-byte loads per lane in flight

static_assert(MCR_SLOT_BYTES % 16 == 0, "k_pool_restage copies an episode slot in 16-byte units");
static_assert(MCR_POOL_GROUP >= 1 && MCR_POOL_GROUP <= 64, "a wavefront ballots one env per lane");

#ifndef MCR_DEVICE_FUNCTIONS_ONLY
__global__ __launch_bounds__(MCR_POOL_LANES) void k_pool_restage(McrEnvState* __restrict__ env, uint8_t* __restrict__ slots, int B, McrPool pool, int envs_per_group) {
  const int lane = threadIdx.x & 63;
  const int e0 = (int)blockIdx.x * envs_per_group;
  const int mine = e0 + lane;
  const bool in_group = lane < envs_per_group && mine < B;
  int need = 0, slot = 0, consumed = 0;
  int32_t drawn = 0;           // weighted: the row this launch stages for the lane's env
  if (in_group) { need = env[mine].staged_ready == 0; slot = env[mine].slot & 1; consumed = env[mine].consumed; }
  for (unsigned long long m = __ballot(need); m; m &= m - 1ull) {
    const int i = (int)__builtin_ctzll(m);
    const int e = e0 + i;
    const int staged = __shfl(slot, i) ^ 1;
    const uint32_t ordinal = (uint32_t)__shfl(consumed, i);
    const int32_t lv = pool.cdf ? mcr_pool_level_cdf(pool.seed, pool.env_offset + (uint32_t)e, ordinal, pool.cdf, pool.K)
                                : mcr_pool_level_of(pool.seed, pool.env_offset + (uint32_t)e, ordinal, pool.K, pool.mode);
    if (lane == i) drawn = lv;
    const uint4* __restrict__ s = (const uint4*)(pool.blobs + (size_t)lv * MCR_SLOT_BYTES);
    uint4* __restrict__ d = (uint4*)(slots + ((size_t)e * 2 + staged) * MCR_SLOT_BYTES);
    const uint32_t n = MCR_SLOT_BYTES / 16;
    uint32_t u = threadIdx.x;
    for (; u + (MCR_POOL_AHEAD - 1) * MCR_POOL_LANES < n; u += MCR_POOL_AHEAD * MCR_POOL_LANES) {
      uint4 v[MCR_POOL_AHEAD];
#pragma unroll
      for (int k = 0; k < MCR_POOL_AHEAD; ++k) v[k] = s[u + k * MCR_POOL_LANES];
#pragma unroll
      for (int k = 0; k < MCR_POOL_AHEAD; ++k) d[u + k * MCR_POOL_LANES] = v[k];
    }
    for (; u < n; u += MCR_POOL_LANES) d[u] = s[u];          // (the last 0 .. 7 units of a lane)
  }
  __syncthreads();           // every wavefront's stores of the group's copies are issued (and every wavefront has read the flags) before a flag flips
  if (threadIdx.x < 64 && need) {
    if (pool.cdf) {
      if (pool.level && consumed >= 1) pool.level[mine] = pool.staged_level[mine];
      pool.staged_level[mine] = drawn;
    }
    else if (pool.level && consumed >= 1) pool.level[mine] = mcr_pool_level_of(pool.seed, pool.env_offset + (uint32_t)mine, (uint32_t)(consumed - 1), pool.K, pool.mode);
    env[mine].staged_ready = 1;
  }
}

// mcr_level_weights: cdf[0 .. K) from weights[0 .. K), one wavefront.  64 weights per round are loaded side by side; the running sum then takes
// them in index order, one f64 add each, in every lane alike (mcr_lane_f64), and lane i keeps the sum as it stood behind its weight.  The
// second pass divides what the same lane stored by the total — or writes the uniform CDF and raises *fell_back.
__global__ __launch_bounds__(64) void k_level_cdf(const double* __restrict__ weights, double* __restrict__ cdf, int K, int32_t* __restrict__ fell_back) {
  const int lane = threadIdx.x;
  double S = 0.0;
  for (int j0 = 0; j0 < K; j0 += 64) {
    const int j = j0 + lane;
    const double w = j < K ? mcr_level_weight(weights[j]) : 0.0;
    const int n = K - j0 < 64 ? K - j0 : 64;
    double mine = 0.0;
    for (int i = 0; i < n; ++i) {
      S += mcr_lane_f64(w, i);
      if (i == lane) mine = S;
    }
    if (j < K) cdf[j] = mine;
  }
  const bool ok = mcr_level_total_ok(S);
  for (int j = lane; j < K; j += 64) cdf[j] = ok ? cdf[j] / S : mcr_level_cdf_uniform(j, K);
  if (lane == 0 && fell_back) *fell_back = ok ? 0 : 1;
}
#endif
