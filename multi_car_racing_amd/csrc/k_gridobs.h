// k_gridobs.h — the grid observation (include/mcr.h: mcr_set_grid_obs): per car an ego-centred H x W grid of bytes fixed to the hull — where
// road is, where this car still gets paid, where others have been, where the other cars are — [B, N, H, W] u8, computed from the state a reset
// or a step ended with.  Like k_stateobs / k_rangeobs it reads finished state and writes one tensor: it runs on the caller's stream behind
// the step, outside the step's three-stream topology and outside a replayed step graph.  It reads p.carf, the env's current slot, p.env[] and
// p.tile_flags at the point where k_stateobs reads its visit counts: k_collide, the one writer of tile_flags, is inside the step, whose tail
// makes the caller's stream wait; the k_flags launch a phase-word step defers (k_flags.h) writes CU_FLAGS alone.  So nothing is flushed.
//
// THE DEFINITION.  Row 0 is farthest ahead, column 0 leftmost, like an image; H, W in 1 .. MCR_GRID_MAX.  Arithmetic as k_rangeobs.h: every
// input is widened to f64; only + - * / in the order written, no contraction; the one transcendental is (s, c) = mcr_sincosf(hull angle) as
// xf_of gives it; a NaN compares false.
//   p = hull.position (body origin: xf_of, as k_stateobs.h / k_rangeobs.h),  f = (-s, c) forward,  r = (c, s) right
//   cell (i, j):  u = (orow - (i + 0.5)) * cell,   v = ((j + 0.5) - ocol) * cell,
//                 q = (p.x + (u * f.x + v * r.x),  p.y + (u * f.y + v * r.y))
//   (cell, orow, ocol: the caller's f32, widened — the cell size in world units and the hull origin in cell units, row and column)
//   within(poly, q): every edge cross product (x2 - x1)(q.y - y1) - (y2 - y1)(q.x - x1), edges i -> i + 1 with the closing edge, is > 0, or
//   every one is < 0 — the reference's on-grass predicate (Point.within, :470-472; point_in_road_poly_f64): the STRICT interior.  A centre
//   on an edge — the shared edge of two consecutive tiles too — is in nothing; a NaN or inf q is in nothing.
//   bit 0 GRID_ROAD   within some entry of the episode's road_poly (tile quads and kerb quads, the f64 vertices point_in_road_poly_f64 builds)
//   bit 1 GRID_FRESH  within some TILE quad t (no kerb) with bit a of tile_flags[env][t] clear: car a still gets paid there
//   bit 2 GRID_TAKEN  within some TILE quad t with tile_flags[env][t] & ((1 << N) - 1) & ~(1 << a) != 0: another car has been there
//   bit 3 GRID_CAR    within one of the four hull polygons (McrShapes::hull, n <= 8) of another car j != a; vertices
//                     V = p_j + (c_j vx - s_j vy, s_j vx + c_j vy) as k_rangeobs.h's channel 1
//   bits 4..7 are 0.  Each bit is an OR over polygons: no culling or search order can change it.  N = 1: bits 2, 3 are never set.  Rows of
//   envs that are not active (never reset, frozen) are zeros; an env that re-spawned in the step shows the first state of its new episode
//   (reset's own action-less step has marked the tiles under the cars' wheels visited, :113-120: those are not FRESH, everything else is).
//
// One wavefront per VIEW (env, car).  The bytes are gathered in LDS (atomic ORs on dwords) and stored once.
// Culling, exact.  (1) The box of the four corner centres holds every centre up to the rounding of q (a few ulp of |p| + |u| + |v|).  The
//   block boxes (MCR_OFF_QBLK) are boxes of the f32-ROUNDED vertices; rounding is monotone, so for q inside an f64 quad
//   round(min vertex) <= round(q) <= q + 6e-8 |q|: a margin of 1e-2 + 1e-6 max|box coordinate| covers both.  48 blocks, one lane each, one
//   ballot; a NaN box compares false and nothing is visited (every q is then NaN or inf: in nothing).
//   (2) Every entry of a visited block, one lane each: its f64 vertices and their GRID coordinates gi = (orow - 0.5) - ((V - p) . f) / (|f|^2
//   cell), gj = (ocol - 0.5) + ((V - p) . r) / (|r|^2 cell).  (q - p) . r = v |r|^2 exactly (f . r = 0), and a linear functional of a point
//   inside a convex polygon lies between its values at the vertices: the (i, j) of a centre within the polygon lie in [min gi, max gi] x
//   [min gj, max gj].  The margin 1e-3 + 1e-9 (|g| + |p| / cell + |origin|) cells covers the f64 rounding of g and of q (1e-15 of the same
//   magnitudes).  A cell outside that range cannot be within; a polygon with an empty range is dropped.
// The cell test.  The wavefront takes the surviving polygons in turn (their records come out of the owning lane by v_readlane: no LDS, no
//   compaction, no worst-case buffer) and spreads the cells of the polygon's (i, j) range over its lanes — a road quad covers ~30 cells of a
//   32 x 32 grid at cell 1.5, not 1024.  Per (cell, polygon) pair the cross products are evaluated in F32 relative to p:
//     E_k = ex (d.y - b) - ey (d.x - a),   (a, b) = V_k - p,  (ex, ey) = V_k+1 - V_k,  d = u f + v r
//   which is the definition's k-th cross product in real arithmetic.  With eps = 2^-24: (a, b, ex, ey) are f64 differences rounded once; u, v
//   carry two roundings each, d three more: |d32 - d| <= 5 eps Dm, Dm = max(|u| + |v|) over the grid; t = d32 - a32 is off by at most
//   7 eps (Dm + |a|); each product by 10 eps |e| (Dm + |a| or |b|), the difference adds one eps: |E32 - E| <= 12 eps (|ex| + |ey|) (Dm + |a| + |b|).
//   The f64 value the definition computes differs from E by at most 1e-15 (|ex| + |ey|) (|p| + |V_k| + |V_k+1| + Dm).  The polygon's threshold
//     thr = max_k (|ex| + |ey|) (2^-19 (|a| + |b| + Dm) + 1e-12 (|p| + |V_k| + |V_k+1|)) + 1e-30
//   (32 eps for 12; 1e-12 for 1e-15; 1e-30 for underflow and flushed denormals) therefore decides: |E32| > thr gives the sign of the
//   definition's cross product.  All > thr or all < -thr: within.  One > thr and one < -thr: not within.  Anything else — a centre in the
//   band of an edge line, NaN, a degenerate polygon — is decided by THE DEFINITION in f64 (point_in_road_poly_f64 itself for road entries).
//   Magnitudes that could overflow f32 (>= 1e18) set thr = inf: always f64.  So the result equals the definition always, not usually.
// Stores: the LDS image is shifted by the view's misalignment (base & 3), so that its dwords are the tensor's aligned dwords; the ragged
//   first and last dword go out in byte stores.  Any base and any H * W are handled.
#pragma once
#include "k_raster_common.h"

#ifndef MCR_DEVICE_FUNCTIONS_ONLY
struct GoView {
  double px, py, fx, fy, rx, ry, cell, orow, ocol;   // the definition's inputs
  double inv, invc, gi0, gj0, pabs, Dm;               // 1 / (|f|^2 cell), 1 / cell, orow - 0.5, ocol - 0.5, |p.x| + |p.y|, max (|u| + |v|)
  float fxf, fyf, rxf, ryf, cellf, orowf, ocolf;      // f32: (s, c), cell and the origin ARE f32 values
  int H, W;
};
// the definition's cell centre
__device__ __forceinline__ void go_centre(const GoView& v, const int i, const int j, double& qx, double& qy) {
  const double u = (v.orow - ((double)i + 0.5)) * v.cell;
  const double w = (((double)j + 0.5) - v.ocol) * v.cell;
  qx = v.px + (u * v.fx + w * v.rx);
  qy = v.py + (u * v.fy + w * v.ry);
}
// the definition's predicate on polygon P of a car at (pjx, pjy), (sj, cj)
__device__ inline bool go_hull_within_f64(const McrPoly& P, const double pjx, const double pjy, const double sj, const double cj, const double qx, const double qy) {
  const int n = min(P.n, 8);
  if (n < 3) return false;
  bool pos = true, neg = true;
  for (int k = 0; k < n; ++k) {
    const int k1 = k + 1 < n ? k + 1 : 0;
    const double ax = (double)P.vx[k], ay = (double)P.vy[k], bx = (double)P.vx[k1], by = (double)P.vy[k1];
    const double x1 = pjx + (cj * ax - sj * ay), y1 = pjy + (sj * ax + cj * ay);
    const double x2 = pjx + (cj * bx - sj * by), y2 = pjy + (sj * bx + cj * by);
    const double cr = (x2 - x1) * (qy - y1) - (y2 - y1) * (qx - x1);
    if (!(cr > 0)) pos = false;
    if (!(cr < 0)) neg = false;
  }
  return pos || neg;
}
__device__ __forceinline__ float go_rl(const float v, const int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// A polygon of NE edges A_k -> B_k in the lane: the f32 record, its threshold and its (i, j) range; false: no cell can be within it
template <int NE>
__device__ __forceinline__ bool go_prepare(const double (&ax)[NE], const double (&ay)[NE], const double (&bx)[NE], const double (&by)[NE], const GoView& v,
                                           float (&fa)[NE], float (&fb)[NE], float (&fex)[NE], float (&fey)[NE], float& thr, int& range) {
  double gimin = 1e300, gimax = -1e300, gjmin = 1e300, gjmax = -1e300, tmax = 0.0, amax = 0.0, emax = 0.0;
#pragma unroll
  for (int k = 0; k < NE; ++k) {
    const double dx = ax[k] - v.px, dy = ay[k] - v.py, ex = bx[k] - ax[k], ey = by[k] - ay[k];
    fa[k] = (float)dx; fb[k] = (float)dy; fex[k] = (float)ex; fey[k] = (float)ey;
    const double along = dx * v.fx + dy * v.fy, right = dx * v.rx + dy * v.ry;
    const double gi = v.gi0 - along * v.inv, gj = right * v.inv + v.gj0;
    gimin = fmin(gimin, gi); gimax = fmax(gimax, gi); gjmin = fmin(gjmin, gj); gjmax = fmax(gjmax, gj);
    const double e1 = fabs(ex) + fabs(ey), a1 = fabs(dx) + fabs(dy), s1 = fabs(ax[k]) + fabs(ay[k]) + fabs(bx[k]) + fabs(by[k]);
    tmax = fmax(tmax, e1 * (0x1p-19 * (a1 + v.Dm) + 1e-12 * (v.pabs + s1)));
    amax = fmax(amax, a1); emax = fmax(emax, e1);
  }
  thr = (float)((tmax + 1e-30) * 1.000001);
  if (!(amax + v.Dm < 1e18) || !(emax < 1e18)) thr = __builtin_inff();     // (an inf term lands here; a NaN one makes its cross product NaN: undecided)
  const double grow = 1e-9 * (v.pabs * v.invc + fabs(v.gi0) + fabs(v.gj0)) + 1e-3;
  const double mi = grow + 1e-9 * fmax(fabs(gimin), fabs(gimax)), mj = grow + 1e-9 * fmax(fabs(gjmin), fabs(gjmax));
  const double i0 = fmax(0.0, ceil(gimin - mi)), i1 = fmin((double)(v.H - 1), floor(gimax + mi));
  const double j0 = fmax(0.0, ceil(gjmin - mj)), j1 = fmin((double)(v.W - 1), floor(gjmax + mj));
  const bool some = i0 <= i1 && j0 <= j1;                                  // (then 0 <= i0 <= i1 <= H - 1: the conversions are safe)
  range = some ? ((int)i0 | ((int)i1 << 6) | ((int)j0 << 12) | ((int)j1 << 18)) : 0;
  return some;
}

// the cells of polygon record `c` (a lane of the wavefront), spread over the lanes; exact(i, j): the definition
template <int NE, class Exact>
__device__ __forceinline__ void go_cells(const int c, const float (&fa)[NE], const float (&fb)[NE], const float (&fex)[NE], const float (&fey)[NE], const float thr_, const int range_,
                                         const uint32_t bits, const GoView& v, const int lane, const int mis, uint32_t* acc, Exact exact) {
  float a[NE], b[NE], ex[NE], ey[NE];
#pragma unroll
  for (int k = 0; k < NE; ++k) { a[k] = go_rl(fa[k], c); b[k] = go_rl(fb[k], c); ex[k] = go_rl(fex[k], c); ey[k] = go_rl(fey[k], c); }
  const float thr = go_rl(thr_, c), nthr = -thr;
  const int range = __builtin_amdgcn_readlane(range_, c);
  const int i0 = range & 63, i1 = (range >> 6) & 63, j0 = (range >> 12) & 63, j1 = (range >> 18) & 63;
  const int w = j1 - j0 + 1, cells = w * (i1 - i0 + 1);
  const float rw = 1.0f / (float)w;
  for (int base = 0; base < cells; base += 64) {
    const int idx = base + lane;
    if (idx >= cells) continue;
    // idx / w: (idx + 0.5) / w is at least 0.5 / 64 away from an integer, the two f32 roundings move it by less than 1e-5
    const int di = (int)(((float)idx + 0.5f) * rw);
    const int i = i0 + di, j = j0 + (idx - di * w);
    const float uf = (v.orowf - ((float)i + 0.5f)) * v.cellf, vf = (((float)j + 0.5f) - v.ocolf) * v.cellf;
    const float dx = uf * v.fxf + vf * v.rxf, dy = uf * v.fyf + vf * v.ryf;
    bool allp = true, alln = true, anyp = false, anyn = false;
#pragma unroll
    for (int k = 0; k < NE; ++k) {
      const float cr = ex[k] * (dy - b[k]) - ey[k] * (dx - a[k]);
      const bool gp = cr > thr, gn = cr < nthr;
      allp = allp && gp; alln = alln && gn; anyp = anyp || gp; anyn = anyn || gn;
    }
    bool in = allp || alln;
    if (!in && !(anyp && anyn)) in = exact(i, j);
    if (in) { const int o = i * v.W + j + mis; atomicOr(&acc[o >> 2], bits << ((o & 3) * 8)); }
  }
}

__global__ __launch_bounds__(64) void k_gridobs(McrParams p, McrGridObs go) {
  __shared__ uint32_t acc[MCR_GRID_MAX * MCR_GRID_MAX / 4 + 1];
  const int lane = (int)threadIdx.x;
  const int N = p.N, BN = p.BN;
  const int view = (int)blockIdx.x;                              // env * N + car
  if (view >= p.B * N) return;
  const int env = view / N, a = view - env * N;
  const int H = min(max(go.rows, 1), MCR_GRID_MAX), W = min(max(go.cols, 1), MCR_GRID_MAX), total = H * W;
  uint8_t* __restrict__ out = go.out + (size_t)view * total;
  const int mis = (int)((uintptr_t)out & 3u);
  const int ndw = (total + mis + 3) >> 2;                        // <= MCR_GRID_MAX^2 / 4 + 1
  for (int k = lane; k < ndw; k += 64) acc[k] = 0u;
  __syncthreads();
  const McrEnvState es = p.env[env];
  if (es.active && !es.frozen) {
    const uint8_t* __restrict__ slot = p.slots + ((size_t)env * 2 + es.slot) * MCR_SLOT_BYTES;
    const McrSlotHeader* Hd = (const McrSlotHeader*)slot;
    const int T = min(max(Hd->T, 1), MCR_TILE_CAP), P = min(max(Hd->P, 0), MCR_QUAD_CAP);   // (a live episode is inside; the clamps keep every index inside the slot)
    const uint32_t* __restrict__ QM = (const uint32_t*)(slot + MCR_OFF_QMETA);
    const uint16_t* __restrict__ tflags = p.tile_flags + (size_t)env * MCR_TILE_CAP;
    const McrShapes& S = *p.shapes;
    const V2 lc = v2(S.hull_lcx, S.hull_lcy);
    const Xf hxf = xf_of(v2(p.carf[(CF_CX + 0) * BN + view], p.carf[(CF_CY + 0) * BN + view]), p.carf[(CF_A + 0) * BN + view], lc);
    GoView v;
    v.px = (double)hxf.p.x; v.py = (double)hxf.p.y;
    const double s = (double)hxf.q.s, c = (double)hxf.q.c;
    v.fx = -s; v.fy = c; v.rx = c; v.ry = s;
    v.cell = (double)go.cell; v.orow = (double)go.orow; v.ocol = (double)go.ocol;
    v.fxf = -hxf.q.s; v.fyf = hxf.q.c; v.rxf = hxf.q.c; v.ryf = hxf.q.s; v.cellf = go.cell; v.orowf = go.orow; v.ocolf = go.ocol;
    v.H = H; v.W = W;
    v.invc = 1.0 / v.cell; v.inv = 1.0 / ((s * s + c * c) * v.cell); v.gi0 = v.orow - 0.5; v.gj0 = v.ocol - 0.5; v.pabs = fabs(v.px) + fabs(v.py);
    {
      const double u0 = fabs((v.orow - 0.5) * v.cell), u1 = fabs((v.orow - ((double)(H - 1) + 0.5)) * v.cell);
      const double w0 = fabs((0.5 - v.ocol) * v.cell), w1 = fabs((((double)(W - 1) + 0.5) - v.ocol) * v.cell);
      v.Dm = fmax(u0, u1) + fmax(w0, w1);
    }
    // (1) the grid's world box against the slot's block boxes
    unsigned long long visit;
    {
      double x0, y0, x1, y1, x2, y2, x3, y3;
      go_centre(v, 0, 0, x0, y0); go_centre(v, 0, W - 1, x1, y1); go_centre(v, H - 1, 0, x2, y2); go_centre(v, H - 1, W - 1, x3, y3);
      const double lox = fmin(fmin(x0, x1), fmin(x2, x3)), hix = fmax(fmax(x0, x1), fmax(x2, x3));
      const double loy = fmin(fmin(y0, y1), fmin(y2, y3)), hiy = fmax(fmax(y0, y1), fmax(y2, y3));
      const double mx = 1e-2 + 1e-6 * fmax(fabs(lox), fabs(hix)), my = 1e-2 + 1e-6 * fmax(fabs(loy), fabs(hiy));
      float4 bb = make_float4(1.0f, 1.0f, -1.0f, -1.0f);
      if (lane < MCR_QUAD_CAP / MCR_QBLK) bb = ((const float4*)(slot + MCR_OFF_QBLK))[lane];
      visit = __ballot(bb.x <= bb.z && (double)bb.x <= hix + mx && (double)bb.z >= lox - mx && (double)bb.y <= hiy + my && (double)bb.w >= loy - my);
    }
    // (2) the visited blocks' entries, four blocks — one entry per lane — at a time
    const uint32_t others = ((1u << N) - 1u) & ~(1u << a);
    while (visit) {
      int blk4[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) { blk4[g] = visit ? (int)__builtin_ctzll(visit) : -1; visit &= visit - 1ull; }
      const int g = lane >> 4;
      const int blk = g == 0 ? blk4[0] : g == 1 ? blk4[1] : g == 2 ? blk4[2] : blk4[3];
      const int q = blk * MCR_QBLK + (lane & (MCR_QBLK - 1));
      bool live = blk >= 0 && q < P;
      int t = 0; bool kerb = false;
      if (live) {
        const uint32_t meta = QM[q];
        const uint32_t tile1 = (meta >> 8) & 0x3ffu, owner1 = (meta >> 18) & 0x3ffu;
        kerb = tile1 == 0u;
        t = (int)(kerb ? owner1 : tile1) - 1;
        live = t >= 0 && t < T;
      }
      float fa[4], fb[4], fex[4], fey[4], thr = 0.0f;
      int range = 0;
      uint32_t bits = MCR_GRID_ROAD;
      if (live) {
        double X[4], Y[4];
        road_poly_vertices_f64(slot, t, T, kerb, X, Y);
        const double bx[4] = {X[1], X[2], X[3], X[0]}, by[4] = {Y[1], Y[2], Y[3], Y[0]};
        live = go_prepare<4>(X, Y, bx, by, v, fa, fb, fex, fey, thr, range);
        if (!kerb) {
          const uint32_t tf = tflags[t];
          if (!((tf >> a) & 1u)) bits |= MCR_GRID_FRESH;
          if (tf & others) bits |= MCR_GRID_TAKEN;
        }
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) fa[k] = fb[k] = fex[k] = fey[k] = 0.0f;
      }
      const int tag = t | (kerb ? 0x10000 : 0) | (int)(bits << 20);
      for (unsigned long long m = __ballot(live); m; m &= m - 1ull) {
        const int cl = (int)__builtin_ctzll(m);
        const int ctag = __builtin_amdgcn_readlane(tag, cl);
        const int ct = ctag & 0xffff; const bool ckerb = (ctag & 0x10000) != 0;
        go_cells<4>(cl, fa, fb, fex, fey, thr, range, (uint32_t)ctag >> 20, v, lane, mis, acc, [&](const int i, const int j) {
          double qx, qy; go_centre(v, i, j, qx, qy);
          return point_in_road_poly_f64(slot, ct, T, ckerb, qx, qy);
        });
      }
    }
    // the other cars' hull polygons: lane = car * 4 + polygon
    if (N > 1) {
      const int j = lane >> 2, h = lane & 3;
      bool live = j < N && j != a;
      float fa[8], fb[8], fex[8], fey[8], thr = 0.0f;
      int range = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) fa[k] = fb[k] = fex[k] = fey[k] = 0.0f;
      if (live) {
        const McrPoly& Pg = S.hull[h];
        const int n = min(Pg.n, 8), cj = env * N + j;
        const Xf jxf = xf_of(v2(p.carf[(CF_CX + 0) * BN + cj], p.carf[(CF_CY + 0) * BN + cj]), p.carf[(CF_A + 0) * BN + cj], lc);
        const double pjx = (double)jxf.p.x, pjy = (double)jxf.p.y, sj = (double)jxf.q.s, cj_ = (double)jxf.q.c;
        double ax[8], ay[8], bx[8], by[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {                            // (an edge slot beyond n repeats edge 0: the same verdict twice)
          const int k0 = k < n ? k : 0, k1 = k0 + 1 < n ? k0 + 1 : 0;
          const double vax = (double)Pg.vx[k0], vay = (double)Pg.vy[k0], vbx = (double)Pg.vx[k1], vby = (double)Pg.vy[k1];
          ax[k] = pjx + (cj_ * vax - sj * vay); ay[k] = pjy + (sj * vax + cj_ * vay);
          bx[k] = pjx + (cj_ * vbx - sj * vby); by[k] = pjy + (sj * vbx + cj_ * vby);
        }
        live = n >= 3 && go_prepare<8>(ax, ay, bx, by, v, fa, fb, fex, fey, thr, range);
      }
      for (unsigned long long m = __ballot(live); m; m &= m - 1ull) {
        const int cl = (int)__builtin_ctzll(m);
        const int cj = env * N + (cl >> 2), ch = cl & 3;
        go_cells<8>(cl, fa, fb, fex, fey, thr, range, (uint32_t)MCR_GRID_CAR, v, lane, mis, acc, [&](const int i, const int jj) {
          double qx, qy; go_centre(v, i, jj, qx, qy);
          const Xf jxf = xf_of(v2(p.carf[(CF_CX + 0) * BN + cj], p.carf[(CF_CY + 0) * BN + cj]), p.carf[(CF_A + 0) * BN + cj], lc);
          return go_hull_within_f64(S.hull[ch], (double)jxf.p.x, (double)jxf.p.y, (double)jxf.q.s, (double)jxf.q.c, qx, qy);
        });
      }
    }
  }
  __syncthreads();
  // the LDS image's dword k is the aligned dword at out - mis + 4 k: whole ones as dwords, the ragged ends byte by byte
  uint32_t* __restrict__ base = (uint32_t*)(out - mis);
  for (int k = lane; k < ndw; k += 64) {
    const uint32_t w = acc[k];
    const int b0 = 4 * k - mis;
    if (b0 >= 0 && b0 + 4 <= total) base[k] = w;
    else {
#pragma unroll
      for (int t = 0; t < 4; ++t) { const int b = b0 + t; if (b >= 0 && b < total) out[b] = (uint8_t)(w >> (8 * t)); }
    }
  }
}
#endif
