// k_driver.h — the scripted driver (include/mcr.h: mcr_set_drivers / mcr_driver_actions): a stateless track-following controller that
// writes one action row (steer, gas, brake) per car, [B, N, 3] f32, from the CURRENT state.  An action is a pure function of the env's
// state, its episode slot and the car's parameter row — nothing is carried from step to step, so snapshots, clones, level pools, sharding
// and every step path work unchanged.  The kernel reads finished state and writes one tensor: it runs on the caller's stream IN FRONT of
// the step that consumes the tensor, outside the step's streams, and reads no flags.
//
// The plain controller (k_driver<false>) promises track following on a free road: no collision avoidance, no overtaking logic, no recovery
// from a spin or from the grass.  RACECRAFT (k_driver<true>, mcr_set_racecraft; defined below the plain controller) adds a side-step round
// the car ahead, a follow rule and a speed cap off the road, for the cars of a second mask.
//
// Arithmetic — k_stateobs.h's recipe, so that a host can reproduce every value bit for bit (tests/driver_ref.py does): every input is
// widened to f64; only + - * / in the order written below, no contraction (the build's -ffp-contract=off); the one transcendental is
// (s, c) = mcr_sincosf(hull angle), the build's sinf/cosf spec, widened; no sqrt (the f32 band of the search, k_nearest.h, only picks the
// tiles the exact f64 comparison looks at and enters no value); one rounding to f32 at the store.  A unary minus, |x| and a product with
// sgn = +-1 are exact.
//   p = hull.position (body origin: xf_of), v = the hull's linear velocity, f = (-s, c) the hull's forward axis, r = (c, s) its right-hand axis,
//   v_f = v.x f.x + v.y f.y,
//   i* = the nearest track point (k_nearest.h: f64 argmin, lowest index among ties, 0 when nothing compares), T the slot's tile count,
//   sgn = d = +1 for a CCW episode, -1 for CW (slot header cw), (TX, TY) the slot's track points, (C, S) its stored cos / sin of beta.
// The car's parameter row, MCR_DRV_PARAMS = 10 floats: L1, L2, v_max, K_s, K_c, K_g, K_b, offset, gas_max, brake_max (mcr_set_drivers
// validates: L1, L2 integers 1..64, v_max > 0, gains >= 0, gas_max, brake_max in [0, 1], everything finite).
//   target(m)  t = (i* + d m) mod T;  q = (TX[t] + (sgn offset) C[t],  TY[t] + (sgn offset) S[t])  — a positive offset lies to the RIGHT of
//              the episode's driving direction;  u = q - p;  x = u.x f.x + u.y f.y;  y = u.x r.x + u.y r.y   (dots as k_stateobs.h's 0, 1)
//   kappa(m)   (2 y) / (x x + y y), or 0 when the denominator is 0: the curvature of the arc through p, tangent to f, that meets the target
//   steer      clamp(K_s kappa(L1), -1, 1)          positive action[0] turns the car towards r (the reference negates it: car.steer(-action[0]))
//   v*         v_max / (1 + K_c |kappa(L2)|),   e = v* - v_f
//   gas        clamp(K_g e, 0, gas_max)
//   brake      clamp((-K_b) e, 0, brake_max)
// clamp(a, lo, hi) is two comparisons: a < lo ? lo : a, then > hi ? hi : that.  For a finite state all three values are finite and inside the
// action space.  A NON-FINITE intermediate yields 0 for that component: steer is 0 unless K_s kappa(L1) is finite; gas (brake) is 0 unless
// kappa(L2) and K_g e ((-K_b) e) are finite — every other intermediate (x, y, v*, e) being non-finite makes one of those non-finite.
//
// Output rows: a car whose bit is set in `mask` gets the controller's action; another car gets a copy of its row of `in`, or zeros when `in`
// is null; rows of envs that are not active (never reset, frozen, parked) are zeros.  `in` is only read (`in` == `out` is allowed: a lane
// reads its row before it writes it).
//
// One wavefront per ENV, like k_stateobs: the lanes keep the track's points in registers and the env's scripted cars take turns on the search
// (k_nearest.h).  Lane a keeps what the turn of car a found — nearest point, pose, parameter row (selected from wave-uniform values, no indexed
// registers) — and when the turns are over lanes 0 .. N-1 compute their cars' three values side by side, once each, and store them.  No LDS, no scratch.
//
// Racecraft — k_driver<true>, launched when a car the launch drives has its bit in McrDriver::rc_mask; tests/racecraft_ref.py restates it.
// The same arithmetic recipe: f64, + - * / and comparisons in the written order, no contraction, no new transcendental, no sqrt, one
// rounding at the store.  min(a, b) below is `b < a ? b : a`, max(0, z) is `z < 0 ? 0 : z`.  The car's racecraft row, MCR_RC_PARAMS = 8
// floats: look (an integer 1..64), w_block, w_pass, off_max, d_safe, K_f, w_off, v_off (mcr_set_racecraft validates: finite, >= 0).
//   Per env: the search runs for EVERY car c (scripted or not) and gives i_c;  car c COUNTS iff p_c, (s_c, c_c) and v_c are all finite;
//     lat_c = sgn ((p_c.x - TX[i_c]) C[i_c] + (p_c.y - TY[i_c]) S[i_c])     — positive to the right of the driving direction, like `offset`.
//   Per car a in both masks that counts (a car that does not count gets the plain controller, whose rule below zeroes what its non-finite
//   values enter), with p, f, r, v_f, i* = i_a as above:
//     for each counting b != a:  g_b = ((i_b - i_a) d) mod T in [0, T);  u = p_b - p_a;  x_b = u.x f.x + u.y f.y;  y_b = u.x r.x + u.y r.y;
//                                vb_b = v_b.x f.x + v_b.y f.y
//     leader l   among the b with g_b <= min(look, (T - 1) / 2) (integer division) and x_b > 0: the smallest x_b, the lowest index among
//                equal x_b.  Without one only the off-road rule applies.
//     side-step  o = offset;  if |lat_l - o| < w_block:  left = lat_l - w_pass, right = lat_l + w_pass;  first = left if lat_a < lat_l else
//                right, second the other one;  o = first if -off_max <= first <= off_max, else second if -off_max <= second <= off_max,
//                else o stays.  o replaces `offset` in both target(m).
//     follow     if |y_l| < w_block:  v_cap = max(0, vb_l + K_f (x_l - d_safe));  v* = min(v*, v_cap)
//     off road   if |lat_a| > w_off:  v* = min(v*, v_off)           (after the follow rule; with or without a leader)
//   then e, gas and brake from v* as above.  Non-finite values: with a and b counting and a validated row every racecraft intermediate
//   (lat, x, y, vb, left, right, v_cap) is finite — sums and products of a few widened f32 values cannot overflow f64 — so racecraft adds no
//   exit of its own: o enters steer and, through kappa(L2), gas and brake; v_cap and v_off enter gas and brake only; and the plain rule holds
//   unchanged (min keeps a NaN v*).  A car that does not count is nobody's leader.
// The kernel: the turns run for all N cars and lane c keeps car c's (i, p, s, c); lane c then loads v_c and computes lat_c and "counts";
// in a wave-uniform loop over b every lane reads car b's (i, p, v, lat, counts) with __shfl — all 64 lanes take part, so the loop stands
// in front of the `lane >= N` exit — and keeps its leader's (x, y, vb, lat).  Still no LDS, no scratch, no indexed registers.
// k_driver<false> is the plain kernel with the instruction stream it had before racecraft existed (it reads neither `rc` nor `rc_mask`).
#pragma once
#include "mcr_kernels.h"
#include "k_nearest.h"

#define MCR_DRV_LOOKAHEAD_MAX 64

MCR_HD double mcr_drv_clamp(double a, double lo, double hi) {
  a = a < lo ? lo : a;
  return a > hi ? hi : a;
}

#ifndef MCR_DEVICE_FUNCTIONS_ONLY
template <bool RC>
__global__ __launch_bounds__(64) void k_driver(McrParams p, McrDriver drv, const float* in, uint32_t mask, float* out) {
  const int lane = (int)threadIdx.x;
  const int env = (int)blockIdx.x;
  if (env >= p.B) return;
  const int N = p.N, BN = p.BN;
  const McrEnvState es = p.env[env];
  const bool live = es.active && !es.frozen;
  const uint8_t* __restrict__ slot = p.slots + ((size_t)env * 2 + es.slot) * MCR_SLOT_BYTES;
  const McrSlotHeader* H = (const McrSlotHeader*)slot;
  const int T = min(max(H->T, 1), MCR_TILE_CAP);               // (a live episode has 1 <= T <= MCR_TILE_CAP; the clamp keeps every index inside the slot)
  const double sgn = H->cw ? -1.0 : 1.0;
  const int d = H->cw ? -1 : 1;
  const double* __restrict__ TX = (const double*)(slot + MCR_OFF_TRACK_X); const double* __restrict__ TY = (const double*)(slot + MCR_OFF_TRACK_Y);
  const double* __restrict__ TC = (const double*)(slot + MCR_OFF_TRACK_C); const double* __restrict__ TS = (const double*)(slot + MCR_OFF_TRACK_S);

  // the turns: what car a's found stays in lane a
  int bi = 0;
  float fpx = 0.0f, fpy = 0.0f, fs = 0.0f, fc = 0.0f;
  float q0 = 1.0f, q1 = 1.0f, q2 = 1.0f, q3 = 0.0f, q4 = 0.0f, q5 = 0.0f, q6 = 0.0f, q7 = 0.0f, q8 = 0.0f, q9 = 0.0f;
  float w0 = 1.0f, w1 = 0.0f, w2 = 0.0f, w3 = 0.0f, w4 = 0.0f, w5 = 0.0f, w6 = 0.0f, w7 = 0.0f;     // (RC: the lane's racecraft row)
  // (RC: the lane's leader — has: one was found; its x, y, vb and lat)
  bool race = false, has = false;
  double mylat = 0.0, lx = 0.0, ly = 0.0, lvb = 0.0, ll = 0.0;
  if (live && (mask & ((1u << N) - 1u))) {                     // (wave-uniform)
    const McrShapes& S = *p.shapes;
    const V2 lc = v2(S.hull_lcx, S.hull_lcy);
    double tx[MCR_NT_TILES_PER_LANE], ty[MCR_NT_TILES_PER_LANE];
    mcr_nearest_load(TX, TY, T, lane, tx, ty);
    for (int a = 0; a < N; ++a) {
      if (!RC && !((mask >> a) & 1u)) continue;                // (RC: every car takes its turn — a car the learner drives is seen too)
      const int ci = env * N + a;
      const Xf hxf = xf_of(v2(p.carf[(CF_CX + 0) * BN + ci], p.carf[(CF_CY + 0) * BN + ci]), p.carf[(CF_A + 0) * BN + ci], lc);
      const int i = mcr_nearest_tile(tx, ty, T, lane, hxf.p.x, hxf.p.y);
      const float* __restrict__ q = drv.prm[a];
      if (lane == a) {
        bi = i; fpx = hxf.p.x; fpy = hxf.p.y; fs = hxf.q.s; fc = hxf.q.c;
        q0 = q[0]; q1 = q[1]; q2 = q[2]; q3 = q[3]; q4 = q[4]; q5 = q[5]; q6 = q[6]; q7 = q[7]; q8 = q[8]; q9 = q[9];
      }
      if constexpr (RC) {
        const float* __restrict__ w = drv.rc[a];
        if (lane == a) { w0 = w[0]; w1 = w[1]; w2 = w[2]; w3 = w[3]; w4 = w[4]; w5 = w[5]; w6 = w[6]; w7 = w[7]; }
      }
    }
    if constexpr (RC) {
      // lane c: car c's velocity, lateral position and whether it counts (a lane beyond the cars holds zeros and does not count)
      const int cc = env * N + min(lane, N - 1);
      const float fvx = lane < N ? p.carf[(CF_VX + 0) * BN + cc] : 0.0f, fvy = lane < N ? p.carf[(CF_VY + 0) * BN + cc] : 0.0f;
      const bool cnt = lane < N && __builtin_isfinite(fpx) && __builtin_isfinite(fpy) && __builtin_isfinite(fs) && __builtin_isfinite(fc) &&
                       __builtin_isfinite(fvx) && __builtin_isfinite(fvy);
      const double px = (double)fpx, py = (double)fpy;
      const double fx = -(double)fs, fy = (double)fc, rx = (double)fc, ry = (double)fs;
      mylat = sgn * ((px - TX[bi]) * TC[bi] + (py - TY[bi]) * TS[bi]);
      race = cnt && ((mask >> lane) & 1u) && ((drv.rc_mask >> lane) & 1u);
      const int G = min(min(max((int)w0, 1), MCR_DRV_LOOKAHEAD_MAX), (T - 1) / 2);
      for (int b = 0; b < N; ++b) {                            // (wave-uniform: every lane shuffles)
        const int ib = __shfl(bi, b);
        const float bpx = __shfl(fpx, b), bpy = __shfl(fpy, b), bvx = __shfl(fvx, b), bvy = __shfl(fvy, b);
        const double blat = __shfl(mylat, b);
        const int bcnt = __shfl((int)cnt, b);
        const int g = ((((ib - bi) * d) % T) + T) % T;
        const double ux = (double)bpx - px, uy = (double)bpy - py;
        const double x = ux * fx + uy * fy, y = ux * rx + uy * ry;
        const double vb = (double)bvx * fx + (double)bvy * fy;
        if (b != lane && bcnt && g <= G && x > 0.0 && (!has || x < lx)) { has = true; lx = x; ly = y; lvb = vb; ll = blat; }
      }
    }
  }
  if (lane >= N) return;

  const int ci = env * N + lane;
  float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f;
  if (live && ((mask >> lane) & 1u)) {
    const double px = (double)fpx, py = (double)fpy;
    const double s = (double)fs, c = (double)fc;
    const double fx = -s, fy = c, rx = c, ry = s;
    const double vx = (double)p.carf[(CF_VX + 0) * BN + ci], vy = (double)p.carf[(CF_VY + 0) * BN + ci];
    const double vf = vx * fx + vy * fy;
    double off = (double)q7, cap = 0.0;
    bool capped = false;
    if constexpr (RC) {
      if (race && has) {
        if (fabs(ll - off) < (double)w1) {                     // the leader sits on the car's line: the line moves to the leader's free side
          const double left = ll - (double)w2, right = ll + (double)w2, lo = -(double)w3, hi = (double)w3;
          const bool go_left = mylat < ll;
          const double first = go_left ? left : right, second = go_left ? right : left;
          if (first >= lo && first <= hi) off = first;
          else if (second >= lo && second <= hi) off = second;
        }
        if (fabs(ly) < (double)w1) {                           // still behind the leader: no faster than it, plus what the gap allows
          cap = lvb + (double)w5 * (lx - (double)w4);
          cap = cap < 0.0 ? 0.0 : cap;
          capped = true;
        }
      }
    }
    const double so = sgn * off;
    double kap[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      // (the look-ahead is validated by mcr_set_drivers; the clamp keeps the index arithmetic small whatever the row holds)
      const int m = min(max((int)(j == 0 ? q0 : q1), 1), MCR_DRV_LOOKAHEAD_MAX);
      const int t = (((bi + d * m) % T) + T) % T;
      const double ux = (TX[t] + so * TC[t]) - px, uy = (TY[t] + so * TS[t]) - py;
      const double x = ux * fx + uy * fy, y = ux * rx + uy * ry;
      const double den = x * x + y * y;
      kap[j] = den == 0.0 ? 0.0 : (2.0 * y) / den;
    }
    const double rs = (double)q3 * kap[0];
    double vstar = (double)q2 / (1.0 + (double)q4 * fabs(kap[1]));
    if constexpr (RC) {
      if (capped) vstar = cap < vstar ? cap : vstar;
      if (race && fabs(mylat) > (double)w6) vstar = (double)w7 < vstar ? (double)w7 : vstar;
    }
    const double e = vstar - vf;
    const double rg = (double)q5 * e, rb = (-(double)q6) * e;
    const bool k2ok = __builtin_isfinite(kap[1]);
    const double steer = __builtin_isfinite(rs) ? mcr_drv_clamp(rs, -1.0, 1.0) : 0.0;
    const double gas = k2ok && __builtin_isfinite(rg) ? mcr_drv_clamp(rg, 0.0, (double)q8) : 0.0;
    const double brake = k2ok && __builtin_isfinite(rb) ? mcr_drv_clamp(rb, 0.0, (double)q9) : 0.0;
    o0 = (float)steer; o1 = (float)gas; o2 = (float)brake;
  } else if (live && in) {
    o0 = in[(size_t)ci * 3 + 0]; o1 = in[(size_t)ci * 3 + 1]; o2 = in[(size_t)ci * 3 + 2];
  }
  out[(size_t)ci * 3 + 0] = o0; out[(size_t)ci * 3 + 1] = o1; out[(size_t)ci * 3 + 2] = o2;
}
#endif
