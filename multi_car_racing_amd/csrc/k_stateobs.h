// k_stateobs.h — the low-dimensional observation (include/mcr.h: mcr_set_state_obs): one f32 row of F = 18 + 2 K + 4 (N - 1) features per car,
// [B, N, F], computed from the state a reset or a step ended with.  The kernel reads finished state and writes one tensor: it runs on the
// caller's stream behind the step, outside the step's three-stream topology, and it never reads CU_FLAGS (on the phase-word path the main
// envs' flag scans run beside the NEXT step's dynamics, k_flags.h; features 13-16 carry what the flags are computed from).
//
// Arithmetic, so that a host can reproduce every value bit for bit (tests/state_obs_ref.py does): every input is widened to f64; only
// + - * / in the order written below, no contraction (the build's -ffp-contract=off); the one transcendental is (s, c) = mcr_sincosf(hull
// angle), the build's sinf/cosf spec, widened; one rounding to f32 at the store.  A unary minus and a product with sgn = +-1 are exact.
// No scaling: raw SI / model units.
//   p = hull.position (body origin: xf_of, what mcr_get_positions returns), v, w = the hull's linear / angular velocity,
//   f = (-s, c) the hull's forward axis, r = (c, s) its right-hand axis,
//   i* = the nearest track point as the reference's backward / on-grass block finds it (multi_car_racing.py:465-467): argmin over the tiles of
//        dx dx + dy dy in f64, lowest index among ties; (C, S) = the slot's cos / sin of beta[i*], (tx, ty) its track point, (dx, dy) = p - (tx, ty),
//   sgn = +1 for a CCW episode, -1 for CW (slot header cw).
//    0, 1   v.x f.x + v.y f.y,  v.x r.x + v.y r.y
//    2      w
//    3-6    wheel omega FL FR RL RR (CD_OMEGA)
//    7      steering angle: angle of body 1 - angle of body 0
//    8-11   CU_ONROAD bits 0..3 as 0.0 / 1.0
//    12     tile_visited_count / T
//    13, 14 dx C + dy S,  (-dx) S + dy C
//    15, 16 sgn (c C + s S),  sgn (s C - c S): the heading against the track's IN THE EPISODE'S DIRECTION (cos, sin) — the direction the reference's
//           backward test measures from (desired_angle += pi for CW, :478-479): +1, 0 for a car that faces the way it was spawned
//    17     sgn
//    18 ..  waypoint m = 1..K: u = track point ((i* + d m stride) mod T) - p, then u.x f.x + u.y f.y,  u.x r.x + u.y r.y
//    then   every other car j in car-index order, self skipped: (p_j - p).f, (p_j - p).r, (v_j - v).f, (v_j - v).r  (dots as in 0, 1)
// d, the index direction the cars are spawned facing: d = +1 for CCW, -1 for CW (= sgn).  The spawn angle is beta of the spawn tile, minus pi
// for CW (mcr_host.cpp / oracle.py spawn_poses, :384-386); a body at angle beta faces (-sin beta, cos beta), the direction the track generator
// steps from tile i to tile i + 1 (the tile's edge lies along (cos beta, sin beta)).
// Rows of envs that are not active (never reset, frozen) are zeros; an env that re-spawned in the step shows the first state of its new episode.
//
// One wavefront per ENV, not per car: the search needs the T track points (2 x 8 x T bytes, ~5 KB) and all of an env's cars search the same
// track — a lane keeps its 8 strided tiles in registers (coalesced 8-byte loads, once) and the env's cars take turns on them, so the track is
// read once per env whatever N is, and "the other cars" of the last feature block are the wavefront's own env.  Per car: the search of
// k_nearest.h (shared with k_driver.h), then lane l computes feature l (and l + 64).  No LDS, no scratch.
#pragma once
#include "mcr_kernels.h"
#include "k_nearest.h"

#define MCR_SO_BASE 18             // features in front of the waypoints
#define MCR_SO_WAYPOINTS_MAX 16
#define MCR_SO_STRIDE_MAX 64
MCR_HD int mcr_so_dim(int N, int K) { return MCR_SO_BASE + 2 * K + 4 * (N - 1); }

#ifndef MCR_DEVICE_FUNCTIONS_ONLY
__global__ __launch_bounds__(64) void k_stateobs(McrParams p, McrStateObs so) {
  const int lane = (int)threadIdx.x;
  const int env = (int)blockIdx.x;
  if (env >= p.B) return;
  const int N = p.N, BN = p.BN, F = so.F, K = so.K;
  float* __restrict__ rows = so.out + (size_t)env * N * F;
  const McrEnvState es = p.env[env];
  if (!es.active || es.frozen) {
    for (int i = lane; i < N * F; i += 64) rows[i] = 0.0f;
    return;
  }
  const uint8_t* __restrict__ slot = p.slots + ((size_t)env * 2 + es.slot) * MCR_SLOT_BYTES;
  const McrSlotHeader* H = (const McrSlotHeader*)slot;
  const int T = min(max(H->T, 1), MCR_TILE_CAP);               // (a live episode has 1 <= T <= MCR_TILE_CAP; the clamp keeps every index inside the slot)
  const double sgn = H->cw ? -1.0 : 1.0;
  const int d = H->cw ? -1 : 1;
  const double* __restrict__ TX = (const double*)(slot + MCR_OFF_TRACK_X); const double* __restrict__ TY = (const double*)(slot + MCR_OFF_TRACK_Y);
  const double* __restrict__ TC = (const double*)(slot + MCR_OFF_TRACK_C); const double* __restrict__ TS = (const double*)(slot + MCR_OFF_TRACK_S);
  const McrShapes& S = *p.shapes;
  const V2 lc = v2(S.hull_lcx, S.hull_lcy);

  // the lane's tiles: lane, lane + 64, .. (k_nearest.h)
  double tx[MCR_NT_TILES_PER_LANE], ty[MCR_NT_TILES_PER_LANE];
  mcr_nearest_load(TX, TY, T, lane, tx, ty);

  for (int a = 0; a < N; ++a) {
    const int ci = env * N + a;
    const float ha = p.carf[(CF_A + 0) * BN + ci];
    const Xf hxf = xf_of(v2(p.carf[(CF_CX + 0) * BN + ci], p.carf[(CF_CY + 0) * BN + ci]), ha, lc);
    const float fpx = hxf.p.x, fpy = hxf.p.y;
    const double px = (double)fpx, py = (double)fpy;
    const int bi = mcr_nearest_tile(tx, ty, T, lane, fpx, fpy);   // (0 for a non-finite pose: no tile compares; the row stays defined)

    // the car's own values (the same in every lane)
    const double s = (double)hxf.q.s, c = (double)hxf.q.c;
    const double fx = -s, fy = c, rx = c, ry = s;
    const double vx = (double)p.carf[(CF_VX + 0) * BN + ci], vy = (double)p.carf[(CF_VY + 0) * BN + ci];
    const double C = TC[bi], Sn = TS[bi];
    const double dx = px - TX[bi], dy = py - TY[bi];
    float* __restrict__ row = rows + (size_t)a * F;
    for (int f = lane; f < F; f += 64) {
      // a feature is a value (ux) or a dot product ux ax + uy ay
      double ux = 0.0, uy = 0.0, ax = 0.0, ay = 0.0;
      bool is_dot = true;
      if (f < 2) { ux = vx; uy = vy; ax = f == 0 ? fx : rx; ay = f == 0 ? fy : ry; }
      else if (f == 2) { is_dot = false; ux = (double)p.carf[(CF_W + 0) * BN + ci]; }
      else if (f < 7) { is_dot = false; ux = p.card[(CD_OMEGA + (f - 3)) * BN + ci]; }
      else if (f == 7) { is_dot = false; ux = (double)p.carf[(CF_A + 1) * BN + ci] - (double)ha; }
      else if (f < 12) { is_dot = false; ux = ((p.caru[CU_ONROAD * BN + ci] >> (f - 8)) & 1u) ? 1.0 : 0.0; }
      else if (f == 12) { is_dot = false; ux = (double)(int32_t)p.caru[CU_TVC * BN + ci] / (double)T; }
      else if (f == 13) { ux = dx; uy = dy; ax = C; ay = Sn; }
      else if (f == 14) { ux = -dx; uy = dy; ax = Sn; ay = C; }
      else if (f == 15) { ux = c; uy = s; ax = C; ay = Sn; }
      else if (f == 16) { ux = s; uy = c; ax = C; ay = -Sn; }   // s C - c S  ==  s C + c (-S)
      else if (f == 17) { is_dot = false; ux = sgn; }
      else if (f < MCR_SO_BASE + 2 * K) {
        const int m = (f - MCR_SO_BASE) / 2 + 1;
        const int t = (((bi + d * m * so.stride) % T) + T) % T;
        ux = TX[t] - px; uy = TY[t] - py;
        const bool fwd = ((f - MCR_SO_BASE) & 1) == 0;
        ax = fwd ? fx : rx; ay = fwd ? fy : ry;
      } else {
        const int q = f - MCR_SO_BASE - 2 * K;
        const int jj = q >> 2, j = jj + (jj >= a ? 1 : 0), cj = env * N + j;
        if ((q & 2) == 0) {
          const Xf jxf = xf_of(v2(p.carf[(CF_CX + 0) * BN + cj], p.carf[(CF_CY + 0) * BN + cj]), p.carf[(CF_A + 0) * BN + cj], lc);
          ux = (double)jxf.p.x - px; uy = (double)jxf.p.y - py;
        } else {
          ux = (double)p.carf[(CF_VX + 0) * BN + cj] - vx; uy = (double)p.carf[(CF_VY + 0) * BN + cj] - vy;
        }
        const bool fwd = (q & 1) == 0;
        ax = fwd ? fx : rx; ay = fwd ? fy : ry;
      }
      double val = is_dot ? ux * ax + uy * ay : ux;
      if (f == 15 || f == 16) val = sgn * val;
      row[f] = (float)val;
    }
  }
}
#endif
