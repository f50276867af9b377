// k_carview.h — what the rasteriser needs from a car's pose: the per-car view record (camera 2x3 + inverse, HUD rectangles, grass
// range; multi_car_racing.py:540-556, 634-674, 615-627) and the world-space vertices of the 12 Car.draw polygons.  ONE function,
// view_record, computes and stores them; its callers differ in where the pose comes from:
//   dynamics_block's epilogue (k_dynamics.h)   from the registers the step ends with, all parts on the car's lane; it keeps the world box;
//   viewprep_block / viewprep_list_block / term_prepare (k_viewprep.h)   from the SoA arrays (car_pose_load), live or of a terminal entry.
// VP_SCORE and VP_OLDFLAGS are not part of it: the dynamics holds their values and writes them (view_score).
#pragma once
#include "mcr_kernels.h"

// what the record and the polygons are computed from
struct CarPose {
  float cx[5], cy[5], a[5];       // sweep centre and angle of hull (0) and wheels (1..4)
  float hvx, hvy, hw;             // the hull's velocity
  double omega[4], phase[4];      // the wheels' spin and stripe phase
};
// `parts`: bit 0 camera + HUD rectangles + grass range + the hull's four polygons, bits 1..4 wheel 0..3 (box + stripe) — the list chains hand
// the parts of a car to five lanes (viewprep_list_block), everybody else computes all of them on the car's lane
#define CARVIEW_ALL 31u
struct CarBox { float xl, yl, xh, yh; };      // world box of the car's draw polygons (= its fixtures)

// (carf / card: per-car SoA fields at stride `stride` — the live state, or the state the cars of a terminal entry ended their episode with);
// only what `parts` reads is loaded
__device__ __forceinline__ CarPose car_pose_load(const float* __restrict__ carf, const double* __restrict__ card, const int stride, const int ci, const uint32_t parts) {
  CarPose c = {};
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const bool mine = (parts >> k) & 1u;
    if (mine) { c.cx[k] = carf[(CF_CX + k) * stride + ci]; c.cy[k] = carf[(CF_CY + k) * stride + ci]; }
    if (mine || (k == 1 && (parts & 1u))) c.a[k] = carf[(CF_A + k) * stride + ci];       // (the steering indicator reads wheel 0's angle)
    if (mine && k > 0) c.phase[k - 1] = card[(CD_PHASE + k - 1) * stride + ci];
  }
  if (parts & 1u) {
    c.hvx = carf[(CF_VX + 0) * stride + ci]; c.hvy = carf[(CF_VY + 0) * stride + ci]; c.hw = carf[(CF_W + 0) * stride + ci];
#pragma unroll
    for (int k = 0; k < 4; ++k) c.omega[k] = card[(CD_OMEGA + k) * stride + ci];
  }
  return c;
}
// the same fields, all of them: a terminal entry (k_dynamics.h), read back by term_prepare
__device__ __forceinline__ void car_pose_store(float* __restrict__ carf, double* __restrict__ card, const int stride, const int ci, const CarPose& c) {
#pragma unroll
  for (int k = 0; k < 5; ++k) { carf[(CF_CX + k) * stride + ci] = c.cx[k]; carf[(CF_CY + k) * stride + ci] = c.cy[k]; carf[(CF_A + k) * stride + ci] = c.a[k]; }
  carf[(CF_VX + 0) * stride + ci] = c.hvx; carf[(CF_VY + 0) * stride + ci] = c.hvy; carf[(CF_W + 0) * stride + ci] = c.hw;
#pragma unroll
  for (int k = 0; k < 4; ++k) { card[(CD_OMEGA + k) * stride + ci] = c.omega[k]; card[(CD_PHASE + k) * stride + ci] = c.phase[k]; }
}

__device__ __forceinline__ void view_score(float* __restrict__ vp, const double reward_shown, const uint32_t flags) {
  vp[VP_SCORE] = __int_as_float(mcr_label_value(reward_shown));       // the score label is drawn (:431) before the step's -0.1 (:437)
  vp[VP_OLDFLAGS] = __uint_as_float(flags);                           // :669-674 draws the flag from the value the PREVIOUS step computed
}

__device__ __forceinline__ void carbox_add(CarBox& box, const V2 v) {
  box.xl = mcr_min(box.xl, v.x); box.xh = mcr_max(box.xh, v.x); box.yl = mcr_min(box.yl, v.y); box.yh = mcr_max(box.yh, v.y);
}
// a polygon of up to 8 vertices is four 16-byte stores (the record is AoS on purpose: the raster reads a car's 832 bytes as one run)
__device__ __forceinline__ void carpoly_quad(float4* __restrict__ q, const V2* w) {
  q[0] = make_float4(w[0].x, w[0].y, w[1].x, w[1].y); q[1] = make_float4(w[2].x, w[2].y, w[3].x, w[3].y);
  q[2] = make_float4(w[3].x, w[3].y, w[3].x, w[3].y); q[3] = q[2];                  // (padding repeats the last vertex)
}

// One lane per car (or per part of a car).  `t`: the env's clock at the frame; `vp`, `carpoly`: the car's own record and polygons;
// returns the world box of the polygon vertices of `parts` (the cheap half of the touch verdict wants it; a caller that drops it does not pay for it).
// Camera (:540-556): f64 exactly as CPython evaluates it, then the f32 values gym's Transform hands to glTranslatef/glRotatef/glScalef;
// HUD rectangles (:634-674); polygon vertices: trans*v in f32, as pybox2d hands them to the viewer, each distinct vertex transformed once.
__device__ __forceinline__ CarBox view_record(const McrShapes& S, const CarPose& c, const double t, const double h_ratio,
                                              float* __restrict__ vp, float* __restrict__ carpoly, const uint32_t parts) {
  CarBox box = {MCR_MAXFLT, MCR_MAXFLT, -MCR_MAXFLT, -MCR_MAXFLT};
  float4* cp4 = (float4*)carpoly;
  float* cnt = carpoly + MCR_CARPOLY_NOFF;                             // vertex counts (int bits): a part's counts are one store
  // (the wheels before the camera: the other order costs k_dynamics<false>, which sits at 256 VGPRs, a 64-bit value copied out to AGPRs)
#pragma unroll
  for (int k = 0; k < 4; ++k) {                                      // wheel k: its box and, while the stripe faces the viewer, the stripe
    if (!((parts >> (1 + k)) & 1u)) continue;
    const Xf wxf = xf_of(v2(c.cx[1 + k], c.cy[1 + k]), c.a[1 + k], v2(0.0f, 0.0f));
    V2 w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { w[i] = xmul(wxf, v2(S.wheel.vx[i], S.wheel.vy[i])); carbox_add(box, w[i]); }
    carpoly_quad(cp4 + (2 * k) * 4, w);
    const double a1 = c.phase[k], a2 = c.phase[k] + 1.2;
    double s1, s2, c1, c2; mcr_sincos_core(a1, &s1, &c1); mcr_sincos_core(a2, &s2, &c2);   // phases stay far below the core's 1.6e6 rad range
    int ns = 0;
    if (!(s1 > 0 && s2 > 0)) {
      if (s1 > 0) c1 = np_sign(c1);
      if (s2 > 0) c2 = np_sign(c2);
      ns = 4;
      const float lx[4] = {(float)(-MCR_WHEEL_W * MCR_SIZE), (float)(+MCR_WHEEL_W * MCR_SIZE), (float)(+MCR_WHEEL_W * MCR_SIZE), (float)(-MCR_WHEEL_W * MCR_SIZE)};
      const float ly[4] = {(float)(+MCR_WHEEL_R * c1 * MCR_SIZE), (float)(+MCR_WHEEL_R * c1 * MCR_SIZE), (float)(+MCR_WHEEL_R * c2 * MCR_SIZE), (float)(+MCR_WHEEL_R * c2 * MCR_SIZE)};
      V2 u[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) u[i] = xmul(wxf, v2(lx[i], ly[i]));
      carpoly_quad(cp4 + (2 * k + 1) * 4, u);
    }
    *(float2*)(cnt + 2 * k) = make_float2(__int_as_float(S.wheel.n), __int_as_float(ns));
  }
  if (parts & 1u) {
    const Xf hxf = xf_of(v2(c.cx[0], c.cy[0]), c.a[0], v2(S.hull_lcx, S.hull_lcy));
    const double zoom = 0.1 * MCR_SCALE * fmax(1 - t, 0.0) + MCR_ZOOM * MCR_SCALE * fmin(t, 1.0);
    const double sx = (double)hxf.p.x, sy = (double)hxf.p.y;
    double angle = -(double)c.a[0];
    const double vx = (double)c.hvx, vy = (double)c.hvy;
    const double speed = sqrt(vx * vx + vy * vy);
    if (speed > 0.5) angle = atan2(vx, vy);
    double sin_a, cos_a; mcr_sincos_core(angle, &sin_a, &cos_a);     // |angle| is a few turns at most; only pixels depend on it
    const double ttx = MCR_WINDOW_W / 2 - (sx * zoom * cos_a - sy * zoom * sin_a);
    const double tty = MCR_WINDOW_H * h_ratio - (sx * zoom * sin_a + sy * zoom * cos_a);
    const float ftx = (float)ttx, fty = (float)tty, fz = (float)zoom;
    const float fdeg = (float)(57.29577951308232 * angle);
    const double rad = (double)fdeg * (3.14159265358979323846 / 180.0);
    double sin_r, cos_r; mcr_sincos_core(rad, &sin_r, &cos_r);
    const float fcs = (float)cos_r, fsn = (float)sin_r;
    const float kx = 96.0f / 1000.0f, ky = 96.0f / 800.0f;
    vp[VP_CAM + 0] = fcs * fz * kx; vp[VP_CAM + 1] = -fsn * fz * kx; vp[VP_CAM + 2] = fsn * fz * ky; vp[VP_CAM + 3] = fcs * fz * ky;
    vp[VP_CAM + 4] = ftx * kx; vp[VP_CAM + 5] = fty * ky;
    // pixel centre -> world:  world = R^T (W - t) / zoom,  W = centre * (1000/96, 800/96)
    const float inv_z = 1.0f / fz;
    const float i0 = fcs * (1000.0f / 96.0f) * inv_z, i1 = fsn * (800.0f / 96.0f) * inv_z, i2 = -(fcs * ftx + fsn * fty) * inv_z;
    const float i3 = -fsn * (1000.0f / 96.0f) * inv_z, i4 = fcs * (800.0f / 96.0f) * inv_z, i5 = (fsn * ftx - fcs * fty) * inv_z;
    vp[VP_INV + 0] = i0; vp[VP_INV + 1] = i1; vp[VP_INV + 2] = i2; vp[VP_INV + 3] = i3; vp[VP_INV + 4] = i4; vp[VP_INV + 5] = i5;
    const double sW = MCR_WINDOW_W / 40.0, hH = MCR_WINDOW_H / 40.0;
    const double vals[5] = {0.02 * speed, 0.01 * c.omega[0], 0.01 * c.omega[1], 0.01 * c.omega[2], 0.01 * c.omega[3]};
    const double places[5] = {5, 7, 8, 9, 10};
    float hud_top = 12.0f;
#pragma unroll
    for (int i = 0; i < 5; ++i) {                                   // vertical_ind (:643-648)
      const float ya = (float)(hH + hH * vals[i]) * ky, yb = (float)hH * ky;
      vp[VP_IND + i * 4 + 0] = (float)((places[i] + 0) * sW) * kx; vp[VP_IND + i * 4 + 1] = (float)((places[i] + 1) * sW) * kx;
      vp[VP_IND + i * 4 + 2] = fminf(ya, yb); vp[VP_IND + i * 4 + 3] = fmaxf(ya, yb);
      hud_top = fmaxf(hud_top, fmaxf(ya, yb) + 1.0f);
    }
    const double jang = (double)(c.a[1] - c.a[0]);
    const double hv[2] = {-10.0 * jang, -0.8 * (double)c.hw};
    const double hp[2] = {20, 30};
#pragma unroll
    for (int i = 0; i < 2; ++i) {                                   // horiz_ind (:649-654)
      const float xa = (float)((hp[i] + 0) * sW) * kx, xb = (float)((hp[i] + hv[i]) * sW) * kx;
      vp[VP_IND + (5 + i) * 4 + 0] = fminf(xa, xb); vp[VP_IND + (5 + i) * 4 + 1] = fmaxf(xa, xb);
      vp[VP_IND + (5 + i) * 4 + 2] = (float)(2 * hH) * ky; vp[VP_IND + (5 + i) * 4 + 3] = (float)(4 * hH) * ky;
    }
    vp[VP_HUDTOP] = hud_top;
    {
      // Light grass squares the viewport can see + "is the whole viewport inside the playfield", from the inverse camera at
      // the four corners of the scene rectangle, in checker units U = world.x / (2k), V = world.y / (2k), k = PLAYFIELD / 20:
      // the playfield is |U|,|V| <= 10 and light square m covers [m, m + 0.5] (:615-627).  One pixel of slack.
      const float hk = 0.5f / (float)(MCR_PLAYFIELD / 20.0);
      const float aU = i0 * hk, bU = i1 * hk, cU = i2 * hk;
      const float aV = i3 * hk, bV = i4 * hk, cV = i5 * hk;
      float umin = MCR_MAXFLT, umax = -MCR_MAXFLT, vmin = MCR_MAXFLT, vmax = -MCR_MAXFLT;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float X = (k & 1) ? 96.0f : 0.0f, Y = (k & 2) ? 96.0f : 12.0f;
        const float u = aU * X + bU * Y + cU, v = aV * X + bV * Y + cV;
        umin = fminf(umin, u); umax = fmaxf(umax, u); vmin = fminf(vmin, v); vmax = fmaxf(vmax, v);
      }
      const float mu = fabsf(aU) + fabsf(bU) + 1e-3f, mv = fabsf(aV) + fabsf(bV) + 1e-3f;
      const bool inside_field = umin - mu >= -10.0f && umax + mu <= 10.0f && vmin - mv >= -10.0f && vmax + mv <= 10.0f;
      int a0 = (int)ceilf(umin - mu - 0.5f), a1 = (int)floorf(umax + mu), b0 = (int)ceilf(vmin - mv - 0.5f), b1 = (int)floorf(vmax + mv);
      a0 = max(a0, -10); a1 = min(a1, 9); b0 = max(b0, -10); b1 = min(b1, 9);
      vp[VP_GRASS + 0] = __int_as_float(a0); vp[VP_GRASS + 1] = __int_as_float(max(a1 - a0 + 1, 0));
      vp[VP_GRASS + 2] = __int_as_float(b0); vp[VP_GRASS + 3] = __int_as_float(max(b1 - b0 + 1, 0));
      vp[VP_GRASS + 4] = __int_as_float(inside_field ? 1 : 0);
    }
    int hn[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {                                    // the hull's four polygons
      const int n = hn[k] = __builtin_amdgcn_readfirstlane(S.hull[k].n);     // the shape table is the same for every lane: scalar loads
      V2 w[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) { if (i < n) w[i] = xmul(hxf, v2(S.hull[k].vx[i], S.hull[k].vy[i])); else w[i] = w[i - 1 < 0 ? 0 : i - 1]; }
#pragma unroll
      for (int i = 0; i < 8; ++i) carbox_add(box, w[i]);
      float4* hp4 = cp4 + (8 + k) * 4;
#pragma unroll
      for (int i = 0; i < 4; ++i) hp4[i] = make_float4(w[2 * i].x, w[2 * i].y, w[2 * i + 1].x, w[2 * i + 1].y);
    }
    *(float4*)(cnt + 8) = make_float4(__int_as_float(hn[0]), __int_as_float(hn[1]), __int_as_float(hn[2]), __int_as_float(hn[3]));
  }
  return box;
}
