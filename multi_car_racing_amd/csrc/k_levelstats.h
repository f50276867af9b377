// k_levelstats.h — per-level episode statistics (include/mcr.h: mcr_set_level_stats): which level did the episode play that an env ended in this
// step, and per level the running count, truncation count, length sum and per-car return sums and sums of squares.
//
// Definition.  Behind a step (launch_step_tail: behind the derived observations, in FRONT of k_pool_restage, which overwrites level[e] for an
// env that installed its next episode), for env e with the step's `done` row set:
//   finished[e] = level[e] if that is in 0 .. K-1, else K (the "unattributed" row: a level row of -1, as load_states leaves it); -1 without `done`
//   row r = finished[e] of stats [K + 1][C], C = 3 + 2N, takes            col 0 += 1.0          col 1 += truncated[e] ? 1.0 : 0.0
//   col 2 += (double)episode_length[e]      col 3 + a += episode_return[e][a]      col 3 + N + a += episode_return[e][a] * episode_return[e][a]
// Arithmetic contract: per row and column the additions happen in step order and, within a step, in ascending env index; every addition is
// one f64 add, the square one f64 multiply in front of its add (-ffp-contract=off: no FMA).  A host that adds in that order reproduces every
// bit (tests/level_stats_ref.py).  So there are no floating-point atomics here — their arrival order is not reproducible — and no partial sums
// that would re-associate the additions: one wavefront owns a row and takes its envs in index order.
//
// Shape: ONE launch, wavefront w of it does two independent things, both from the step's `done` row and `level` (neither depends on the other):
//   the finished pass   the wavefronts share the B envs in rounds of 256, four envs per lane: `done` as one 4-byte load, `level` and `finished`
//                       as 16-byte ones (the tail and misaligned caller buffers go env by env).  Reads B + 4B bytes, writes 4B.
//   the row pass        wavefront w < K + 1 owns stats row w.  It walks the envs in index order, 1024 per round — `done` as 16-byte loads, one
//                       ballot: the steady state (~B / 1000 envs end per step) is B / 1024 such loads per wavefront, no level read, no store —
//                       and, where a round holds an ending, its 64-env chunks: lane = env, a ballot of "ended in MY row", and only behind a
//                       non-zero ballot the C loads of the lane's own env (side by side: up to 19 loads in flight per lane).  The additions
//                       then run over the ballot's bits in ascending order: mcr_lane_f64 broadcasts lane i's value (two v_readlane, scalar
//                       registers, no LDS), and every lane adds it to ITS copy of the row's C running sums — wave-uniform registers, fully
//                       unrolled over the column (static indices: no scratch).  Lane 0 stores the row once, at the end, if it changed.
//                       A step in which every env ends spreads over K + 1 wavefronts; each adds B / K envs at ~C adds + 2C readlanes apiece.
// No LDS, no barrier, no atomics, no scratch (DESIGN.md §3.4g has the compiler's resource report).  Cost model: the row pass re-reads `done`
// (B bytes) per row — (K + 1) B bytes out of L2 per step in the steady state, 1 MB at B = 4096, K = 256.
#pragma once
#include "mcr_kernels.h"

#define MCR_LS_LANES 256                       // four wavefronts per workgroup: four rows
#define MCR_LS_COLS(N) (3 + 2 * (N))

#ifndef MCR_DEVICE_FUNCTIONS_ONLY
__device__ __forceinline__ int32_t mcr_ls_row(int32_t level, int32_t K) { return (level >= 0 && level < K) ? level : K; }

__global__ __launch_bounds__(MCR_LS_LANES) void k_levelstats(McrLevelStats ls, const uint8_t* __restrict__ done, const uint8_t* __restrict__ trunc,
                                                             const double* __restrict__ ep_return, const int32_t* __restrict__ ep_len,
                                                             const int32_t* __restrict__ level, int B, int N, int K) {
  const int lane = threadIdx.x & 63;
  const int wave = (int)blockIdx.x * (MCR_LS_LANES / 64) + (int)(threadIdx.x >> 6);
  const int waves = (int)gridDim.x * (MCR_LS_LANES / 64);

  // ---- the finished pass: rounds of 256 envs, shared among the launch's wavefronts
  const bool wide4 = (((uintptr_t)done & 3u) | ((uintptr_t)level & 15u) | ((uintptr_t)ls.finished & 15u)) == 0;
  for (int base = wave * 256; base < B; base += waves * 256) {
    const int e = base + lane * 4;
    if (wide4 && e + 3 < B) {
      const uint32_t d = *(const uint32_t*)(done + e);
      int4 f = make_int4(-1, -1, -1, -1);
      if (d) {
        const int4 lv = *(const int4*)(level + e);
        if (d & 0x000000ffu) f.x = mcr_ls_row(lv.x, K);
        if (d & 0x0000ff00u) f.y = mcr_ls_row(lv.y, K);
        if (d & 0x00ff0000u) f.z = mcr_ls_row(lv.z, K);
        if (d & 0xff000000u) f.w = mcr_ls_row(lv.w, K);
      }
      *(int4*)(ls.finished + e) = f;
    }
    else
      for (int i = e; i < e + 4 && i < B; ++i) ls.finished[i] = done[i] ? mcr_ls_row(level[i], K) : -1;
  }

  // ---- the row pass
  const int r = wave;
  if (r > K) return;
  const int C = MCR_LS_COLS(N);
  double* __restrict__ row = ls.stats + (size_t)r * C;
  double a_n = 0.0, a_tr = 0.0, a_len = 0.0, a_ret[MCR_MAX_AGENTS], a_sq[MCR_MAX_AGENTS];     // the row's running sums, alike in every lane
#pragma unroll
  for (int a = 0; a < MCR_MAX_AGENTS; ++a) a_ret[a] = a_sq[a] = 0.0;
  bool loaded = false;
  const bool wide16 = ((uintptr_t)done & 15u) == 0;
  for (int base = 0; base < B; base += 1024) {
    unsigned long long sub = ~0ull;          // bit 4s .. 4s + 3: chunk s (64 envs) of the round may hold an ending
    if (wide16 && base + 1024 <= B) {
      const uint4 d = *(const uint4*)(done + base + lane * 16);
      sub = __ballot((d.x | d.y | d.z | d.w) != 0u);
      if (!sub) continue;
    }
    for (int s = 0; s < 16 && base + s * 64 < B; ++s) {
      if (!((sub >> (4 * s)) & 0xfull)) continue;
      const int e = base + s * 64 + lane;
      const bool ended = e < B && done[e] != 0;
      const bool hit = ended && mcr_ls_row(level[e], K) == r;
      unsigned long long m = __ballot(hit);
      if (!m) continue;
      double x_tr = 0.0, x_len = 0.0, x_ret[MCR_MAX_AGENTS], x_sq[MCR_MAX_AGENTS];
#pragma unroll
      for (int a = 0; a < MCR_MAX_AGENTS; ++a) x_ret[a] = x_sq[a] = 0.0;
      if (hit) {
        x_tr = (trunc && trunc[e]) ? 1.0 : 0.0;
        x_len = (double)ep_len[e];
#pragma unroll
        for (int a = 0; a < MCR_MAX_AGENTS; ++a)
          if (a < N) x_ret[a] = ep_return[(size_t)e * N + a];
#pragma unroll
        for (int a = 0; a < MCR_MAX_AGENTS; ++a) x_sq[a] = x_ret[a] * x_ret[a];
      }
      if (!loaded) {                         // (first ending of the row in this step: the sums so far)
        loaded = true;
        a_n = row[0]; a_tr = row[1]; a_len = row[2];
#pragma unroll
        for (int a = 0; a < MCR_MAX_AGENTS; ++a) { a_ret[a] = a < N ? row[3 + a] : 0.0; a_sq[a] = a < N ? row[3 + N + a] : 0.0; }
      }
      for (; m; m &= m - 1ull) {             // ascending env index
        const int i = (int)__builtin_ctzll(m);
        a_n += 1.0;
        a_tr += mcr_lane_f64(x_tr, i);
        a_len += mcr_lane_f64(x_len, i);
#pragma unroll
        for (int a = 0; a < MCR_MAX_AGENTS; ++a)
          if (a < N) { a_ret[a] += mcr_lane_f64(x_ret[a], i); a_sq[a] += mcr_lane_f64(x_sq[a], i); }
      }
    }
  }
  if (loaded && lane == 0) {
    row[0] = a_n; row[1] = a_tr; row[2] = a_len;
#pragma unroll
    for (int a = 0; a < MCR_MAX_AGENTS; ++a)
      if (a < N) { row[3 + a] = a_ret[a]; row[3 + N + a] = a_sq[a]; }
  }
}
#endif
