// k_rangeobs.h — the range-finder observation (include/mcr.h: mcr_set_range_obs): per car a fan of R rays from the hull's body origin, two
// channels per ray — the range to the track's borders and the range to the other cars' hulls — [B, N, 2, R] f32, computed from the state a
// reset or a step ended with.  Like k_stateobs it reads finished state and writes one tensor: it runs on the caller's stream behind the step,
// outside the step's three-stream topology, and reads no flags.
//
// Arithmetic, so that a host can reproduce every value bit for bit (tests/range_obs_ref.py does): every input is widened to f64; only
// + - * / in the order written below, no contraction (the build's -ffp-contract=off); the one transcendental is (s, c) = mcr_sincosf(hull
// angle), the build's sinf/cosf spec, widened; one rounding to f32 at the store.  A NaN compares false: a NaN case is no hit.
//   p = hull.position (body origin: xf_of, as k_stateobs.h), f = (-s, c) the hull's forward axis, r = (c, s) its right-hand axis
//   ray k: (ck, sk) = dir[k], the caller's table (f32, widened; it travels by value with the launch):
//          u = (ck f.x + sk r.x,  ck f.y + sk r.y)       — not renormalised: a range is the ray parameter t of p + t u
//   segment A -> B:  e = B - A,  w = A - p,
//          den = u.x e.y - u.y e.x,   t = (w.x e.y - w.y e.x) / den,   q = (w.x u.y - w.y u.x) / den
//          a hit iff den != 0 && t >= 0 && q >= 0 && q <= 1
//   range = min(max_range, min over the channel's hits of t)      (min is order-independent: any reduction order gives the same value)
// Channel 0, the borders: for tile i = 0 .. T-1 and j = (i - 1 + T) % T the segments L_j -> L_i and R_j -> R_i,
//          L_i = (TX[i] - W TC[i], TY[i] - W TS[i]),  R_i = (TX[i] + W TC[i], TY[i] + W TS[i]),  W = 40 / MCR_SCALE
//   (the slot's track points and libm's cos / sin of beta; the f64 vertices point_in_road_poly_f64 builds): two closed polylines, 2 T
//   segments.  Kerb quads are no borders.  Limit: at a folded inner hairpin the inner polyline can lie inside the union of the road quads;
//   a ray then reports that segment — the value is "the first border segment", not "the exit from the union".
// Channel 1, the opponents: for every other car j of the env (self skipped) and every polygon h = 0..3 of McrShapes::hull, the edges
//          A = V[v], B = V[(v + 1) % n], v = 0 .. n-1 (the closing edge included), in the polygon's stored vertex order (b2PolygonShape::Set's:
//          CCW from the right-most vertex, the lower one on a tie),
//          V = p_j + (c_j vx - s_j vy,  s_j vx + c_j vy)     ((s_j, c_j), p_j: car j's as above; vx, vy: the f32 body-frame vertex, widened)
//   With N = 1 every value is max_range.
// Rows of envs that are not active (never reset, frozen) are zeros; an env that re-spawned in the step shows the first state of its new episode.
//
// One wavefront per ENV (as k_stateobs / k_driver): a lane keeps the border segments of its strided tiles (lane, lane + 64, ..) as (A, e) in
// registers — computed once per env, whatever N and R are — and the slots lane, lane + 64, .. of the env's N x 4 x 8 hull edges; the env's
// cars and their rays take turns on them.  Per ray a lane runs its segments through a DIVISION-FREE necessary condition,
//          not (|w.x u.y - w.y u.x| > |den|)
// (|nq| > |den| makes the correctly rounded quotient q > 1 or <= -1, never a hit; NaN and den = 0 pass), and evaluates the definition — the two
// divisions — only on what passes: a line crosses a handful of the ~600 segments.  A passing segment is PARKED in the lane (one per lane and
// channel) and evaluated when the lane's next one arrives or at the end of the ray: the whole wavefront pays for a division pair when any lane
// divides, so dividing on the spot would cost every test two divisions again; parked, a ray costs one pair per channel.  Then a wave-wide f64
// min (__shfl_xor), and lane k keeps ray k's values for one coalesced store per car.
// Culling, exact: per car a tile whose two segments' bounding box lies farther from p than max_range * max_k |dir[k]| (1 + 1e-6) + 1e-2 (the
// host's McrRangeObs::cull; |u| <= |dir| |f| and |f| <= 1 + 2e-7) is skipped, and a run of 64 tiles no lane wants is skipped by the wavefront:
// a hit's point p + t u lies on its segment, hence in the box, so a skipped tile holds no hit with t <= max_range and min() cannot change.  The
// box is made of the lane's own f64 vertices (A and A + e, within an ulp of B), not of the slot's f32 sensor boxes (MCR_OFF_TAABB): those are
// the boxes of the WELDED hull of the tile's f32 vertices and would need a margin for the weld as well; the 1e-2 here covers 1e-13.
// No LDS, no scratch: the segment registers are indexed by unrolled constants.
#pragma once
#include "mcr_kernels.h"

#define MCR_RO_TILES_PER_LANE (MCR_TILE_CAP / 64)
#define MCR_RO_EDGE_SLOTS_PER_LANE (MCR_MAX_AGENTS * 4 * 8 / 64)    // edge slot = car * 32 + polygon * 8 + edge

#ifndef MCR_DEVICE_FUNCTIONS_ONLY
// the definition's test on a parked segment
__device__ __forceinline__ void ro_eval(const double nt, const double nq, const double den, double& best) {
  const double t = nt / den, q = nq / den;
  if (den != 0.0 && t >= 0.0 && q >= 0.0 && q <= 1.0 && t < best) best = t;
}
// segment (w, e) against ray u: park it if it can be a hit (evaluating the lane's parked one first)
__device__ __forceinline__ void ro_test(const bool on, const double wx, const double wy, const double ex, const double ey, const double ux, const double uy,
                                        bool& parked, double& pn, double& pq, double& pd, double& best) {
  const double den = ux * ey - uy * ex;
  const double nt = wx * ey - wy * ex;
  const double nq = wx * uy - wy * ux;
  if (on && !(fabs(nq) > fabs(den))) {
    if (parked) ro_eval(pn, pq, pd, best);
    pn = nt; pq = nq; pd = den; parked = true;
  }
}
__device__ __forceinline__ double ro_wave_min(double v) {
  for (int o = 32; o > 0; o >>= 1) { const double ov = __shfl_xor(v, o); v = ov < v ? ov : v; }
  return v;
}

__global__ __launch_bounds__(64) void k_rangeobs(McrParams p, McrRangeObs ro) {
  const int lane = (int)threadIdx.x;
  const int env = (int)blockIdx.x;
  if (env >= p.B) return;
  const int N = p.N, BN = p.BN, R = min(max(ro.R, 1), MCR_RANGE_RAYS_MAX);
  float* __restrict__ rows = ro.out + (size_t)env * N * 2 * R;
  const McrEnvState es = p.env[env];
  if (!es.active || es.frozen) {
    for (int i = lane; i < N * 2 * R; i += 64) rows[i] = 0.0f;
    return;
  }
  const uint8_t* __restrict__ slot = p.slots + ((size_t)env * 2 + es.slot) * MCR_SLOT_BYTES;
  const McrSlotHeader* H = (const McrSlotHeader*)slot;
  const int T = min(max(H->T, 1), MCR_TILE_CAP);               // (a live episode has 1 <= T <= MCR_TILE_CAP; the clamp keeps every index inside the slot)
  const double* __restrict__ TX = (const double*)(slot + MCR_OFF_TRACK_X); const double* __restrict__ TY = (const double*)(slot + MCR_OFF_TRACK_Y);
  const double* __restrict__ TC = (const double*)(slot + MCR_OFF_TRACK_C); const double* __restrict__ TS = (const double*)(slot + MCR_OFF_TRACK_S);
  const McrShapes& S = *p.shapes;
  const V2 lc = v2(S.hull_lcx, S.hull_lcy);
  const double W = 40 / MCR_SCALE;
  const double maxr = (double)ro.max_range, cull2 = ro.cull * ro.cull;

  // the lane's border segments: tile i = lane + 64 k, A = L_j / R_j, e = L_i - L_j / R_i - R_j
  double lax[MCR_RO_TILES_PER_LANE], lay[MCR_RO_TILES_PER_LANE], lex[MCR_RO_TILES_PER_LANE], ley[MCR_RO_TILES_PER_LANE];
  double rax[MCR_RO_TILES_PER_LANE], ray[MCR_RO_TILES_PER_LANE], rex[MCR_RO_TILES_PER_LANE], rey[MCR_RO_TILES_PER_LANE];
#pragma unroll
  for (int k = 0; k < MCR_RO_TILES_PER_LANE; ++k) {
    const int i = lane + 64 * k;
    lax[k] = lay[k] = lex[k] = ley[k] = rax[k] = ray[k] = rex[k] = rey[k] = 0.0;
    if (i < T) {
      const int j = i == 0 ? T - 1 : i - 1;
      const double xi = TX[i], yi = TY[i], ci = TC[i], si = TS[i], xj = TX[j], yj = TY[j], cj = TC[j], sj = TS[j];
      const double lix = xi - W * ci, liy = yi - W * si, rix = xi + W * ci, riy = yi + W * si;
      lax[k] = xj - W * cj; lay[k] = yj - W * sj; rax[k] = xj + W * cj; ray[k] = yj + W * sj;
      lex[k] = lix - lax[k]; ley[k] = liy - lay[k]; rex[k] = rix - rax[k]; rey[k] = riy - ray[k];
    }
  }
  // the lane's hull edges: slot m of the lane is edge (lane + 64 m) & 7 of polygon ((lane + 64 m) >> 3) & 3 of car (lane + 64 m) >> 5
  double hax[MCR_RO_EDGE_SLOTS_PER_LANE], hay[MCR_RO_EDGE_SLOTS_PER_LANE], hex_[MCR_RO_EDGE_SLOTS_PER_LANE], hey[MCR_RO_EDGE_SLOTS_PER_LANE];
  uint32_t hvalid = 0u;
#pragma unroll
  for (int m = 0; m < MCR_RO_EDGE_SLOTS_PER_LANE; ++m) {
    const int sl = lane + 64 * m, j = sl >> 5, h = (sl >> 3) & 3, v = sl & 7;
    hax[m] = hay[m] = hex_[m] = hey[m] = 0.0;
    if (N > 1 && j < N) {
      const McrPoly& P = S.hull[h];
      const int n = min(P.n, 8);
      if (v < n) {
        const int cj = env * N + j, v1 = v + 1 < n ? v + 1 : 0;
        const Xf jxf = xf_of(v2(p.carf[(CF_CX + 0) * BN + cj], p.carf[(CF_CY + 0) * BN + cj]), p.carf[(CF_A + 0) * BN + cj], lc);
        const double pjx = (double)jxf.p.x, pjy = (double)jxf.p.y, sj = (double)jxf.q.s, cj_ = (double)jxf.q.c;
        const double ax = (double)P.vx[v], ay = (double)P.vy[v], bx = (double)P.vx[v1], by = (double)P.vy[v1];
        hax[m] = pjx + (cj_ * ax - sj * ay); hay[m] = pjy + (sj * ax + cj_ * ay);
        const double wbx = pjx + (cj_ * bx - sj * by), wby = pjy + (sj * bx + cj_ * by);
        hex_[m] = wbx - hax[m]; hey[m] = wby - hay[m];
        hvalid |= 1u << m;
      }
    }
  }

  for (int a = 0; a < N; ++a) {
    const int ci = env * N + a;
    const Xf hxf = xf_of(v2(p.carf[(CF_CX + 0) * BN + ci], p.carf[(CF_CY + 0) * BN + ci]), p.carf[(CF_A + 0) * BN + ci], lc);
    const double px = (double)hxf.p.x, py = (double)hxf.p.y;
    const double s = (double)hxf.q.s, c = (double)hxf.q.c;
    const double fx = -s, fy = c, rx = c, ry = s;

    // which of the lane's tiles are within reach of this car; which runs of 64 tiles any lane wants
    uint32_t near = 0u, wave_near = 0u;
#pragma unroll
    for (int k = 0; k < MCR_RO_TILES_PER_LANE; ++k) {
      bool far = lane + 64 * k >= T;
      if (!far) {
        const double lbx = lax[k] + lex[k], lby = lay[k] + ley[k], rbx = rax[k] + rex[k], rby = ray[k] + rey[k];
        const double lox = fmin(fmin(lax[k], lbx), fmin(rax[k], rbx)), hix = fmax(fmax(lax[k], lbx), fmax(rax[k], rbx));
        const double loy = fmin(fmin(lay[k], lby), fmin(ray[k], rby)), hiy = fmax(fmax(lay[k], lby), fmax(ray[k], rby));
        const double dx = fmax(fmax(lox - px, px - hix), 0.0), dy = fmax(fmax(loy - py, py - hiy), 0.0);
        far = dx * dx + dy * dy > cull2;                        // (a NaN pose: never far; the tests then find no hit)
      }
      if (!far) near |= 1u << k;
      if (__any(!far)) wave_near |= 1u << k;
    }
    // the edge slots of the other cars
    uint32_t hon = 0u;
#pragma unroll
    for (int m = 0; m < MCR_RO_EDGE_SLOTS_PER_LANE; ++m) if (((lane + 64 * m) >> 5) != a) hon |= 1u << m;
    hon &= hvalid;

    float out0 = 0.0f, out1 = 0.0f;                             // lane k: ray k's two ranges
    for (int k = 0; k < R; ++k) {
      const double ck = (double)ro.dir[k][0], sk = (double)ro.dir[k][1];
      const double ux = ck * fx + sk * rx, uy = ck * fy + sk * ry;
      double best0 = maxr, best1 = maxr;
      double pn = 0.0, pq = 0.0, pd = 0.0;
      bool parked = false;
#pragma unroll
      for (int t = 0; t < MCR_RO_TILES_PER_LANE; ++t) {
        if (!((wave_near >> t) & 1u)) continue;
        const bool on = ((near >> t) & 1u) != 0u;
        ro_test(on, lax[t] - px, lay[t] - py, lex[t], ley[t], ux, uy, parked, pn, pq, pd, best0);
        ro_test(on, rax[t] - px, ray[t] - py, rex[t], rey[t], ux, uy, parked, pn, pq, pd, best0);
      }
      if (parked) ro_eval(pn, pq, pd, best0);
      best0 = ro_wave_min(best0);
      if (N > 1) {
        parked = false;
#pragma unroll
        for (int m = 0; m < MCR_RO_EDGE_SLOTS_PER_LANE; ++m) {
          if (2 * m >= N) continue;                             // slot m holds cars 2 m, 2 m + 1
          ro_test(((hon >> m) & 1u) != 0u, hax[m] - px, hay[m] - py, hex_[m], hey[m], ux, uy, parked, pn, pq, pd, best1);
        }
        if (parked) ro_eval(pn, pq, pd, best1);
        best1 = ro_wave_min(best1);
      }
      if (lane == k) { out0 = (float)best0; out1 = (float)best1; }
    }
    float* __restrict__ row = rows + (size_t)a * 2 * R;
    if (lane < R) { row[lane] = out0; row[R + lane] = out1; }
  }
}
#endif
