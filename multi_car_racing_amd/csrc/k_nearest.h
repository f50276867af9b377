// k_nearest.h — the nearest track point of a pose, as the reference's backward / on-grass block finds it (multi_car_racing.py:465-467): argmin over
// the tiles of dx dx + dy dy in f64, lowest index among ties.  The search of k_stateobs.h (feature table) and k_driver.h (the scripted driver),
// which both run one wavefront per env: a lane keeps its MCR_NT_TILES_PER_LANE strided tiles (lane, lane + 64, ..) in registers — coalesced
// 8-byte loads, once per env — and the env's cars take turns on them.  Per pose: f32 distances of the lane's tiles, wave minimum (__shfl_xor),
// exact f64 on the tiles within the rounding band of it (k_flags.h's band), wave argmin with the lowest index winning.  No LDS, no scratch:
// the tile registers are indexed by unrolled constants.  Every lane of the wavefront must call these functions (wave-wide shuffles).
#pragma once
#include "mcr_kernels.h"

#define MCR_NT_TILES_PER_LANE (MCR_TILE_CAP / 64)

// the lane's tiles of a track of T points (a tile beyond T reads as 0 and never competes)
__device__ __forceinline__ void mcr_nearest_load(const double* __restrict__ TX, const double* __restrict__ TY, int T, int lane,
                                                 double (&tx)[MCR_NT_TILES_PER_LANE], double (&ty)[MCR_NT_TILES_PER_LANE]) {
#pragma unroll
  for (int k = 0; k < MCR_NT_TILES_PER_LANE; ++k) {
    const int t = lane + 64 * k;
    tx[k] = t < T ? TX[t] : 0.0; ty[k] = t < T ? TY[t] : 0.0;
  }
}

// the nearest track point of (fpx, fpy), the same value in every lane; 0 for a non-finite pose (no tile compares: the caller's row stays defined)
__device__ __forceinline__ int mcr_nearest_tile(const double (&tx)[MCR_NT_TILES_PER_LANE], const double (&ty)[MCR_NT_TILES_PER_LANE], int T, int lane,
                                                float fpx, float fpy) {
  const double px = (double)fpx, py = (double)fpy;
  // pass 1: f32 distances, wave minimum
  float dmin = MCR_MAXFLT;
#pragma unroll
  for (int k = 0; k < MCR_NT_TILES_PER_LANE; ++k) {
    const float ddx = fpx - (float)tx[k], ddy = fpy - (float)ty[k];
    if (lane + 64 * k < T) dmin = fminf(dmin, ddx * ddx + ddy * ddy);
  }
  for (int o = 32; o > 0; o >>= 1) dmin = fminf(dmin, __shfl_xor(dmin, o));
  // pass 2: exact f64 on the tiles within the f32 error band of the minimum; within a lane the tiles ascend, so `<` keeps the lowest index
  const float band = sqrtf(dmin) * (1.0f + 1e-5f) + 2e-3f;
  const float thr = band * band;
  double bd = 1e300; int bi = 0x7fffffff;
#pragma unroll
  for (int k = 0; k < MCR_NT_TILES_PER_LANE; ++k) {
    const float ddx = fpx - (float)tx[k], ddy = fpy - (float)ty[k];
    if (lane + 64 * k < T && ddx * ddx + ddy * ddy <= thr) {
      const double dx = px - tx[k], dy = py - ty[k];
      const double dd = dx * dx + dy * dy;
      if (dd < bd) { bd = dd; bi = lane + 64 * k; }
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const double od = __shfl_xor(bd, o); const int oi = __shfl_xor(bi, o);
    if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
  }
  if (bi >= T) bi = 0;
  return bi;
}
