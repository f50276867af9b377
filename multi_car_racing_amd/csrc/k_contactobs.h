// k_contactobs.h — the car-contact observation (include/mcr.h: mcr_set_contact_obs): per car WHO it touched in the step and, per pair of cars,
// HOW HARD — Box2D's PostSolve report, reduced on the device from the env's car<->car manifold store (McrParams::cc_store; k_carcontacts.h
// has the record layout).  k_collide rewrites the store's count and records at every step's entry poses, k_dynamics ("StoreImpulses") writes
// every point's accumulated normal impulse back behind the velocity solve: behind a step the store holds what that step's solver applied.
//
// Definition, so that a host reproduces every bit (tests/contact_obs_ref.py does).  Per env, store = cc_store + env * MCR_CC_STORE_WORDS:
//   count = min(store[0], MCR_CC_MAX); record i = store + 4 + i * MCR_CC_WORDS, i < count — nothing behind record count - 1 is read;
//   key = rec[0] = carA | fixA << 4 | carB << 8 | fixB << 12 (fixture 0..3 a hull polygon, 4..7 a wheel), n = min(rec[1] >> 8, 2) points,
//   nImp of point q = rec[8 + 5 q] (f32 bits).
//   impulse[a][j] (f64 [N][N]):  acc = 0.0; for record i = 0 .. count - 1 with {carA, carB} = {a, j}: for q = 0 .. n - 1: acc = acc + (double)nImp_q
//       — one f64 add per point in store order, no partial sums, nothing re-associated; [a][j] and [j][a] take the same additions and are
//       the same bits; no record names a car twice, so the diagonal takes none.
//   mask[a] (int32 [N]):  the OR over the same records of   bit j (0..7): a record between a and j exists;   bit 8: car a's fixture in such
//       a record is a hull polygon (index < 4);   bit 9: it is a wheel (index >= 4).
// accumulate = 0: acc starts at 0.0 and the mask at 0: the row describes this store alone (an env with count 0: zeros).
// accumulate = 1 (sub-step i > 0 of a macro-step): acc starts from the value in the caller's buffer, the additions above follow, one store;
//       the mask is OR-ed into the caller's.  Over a macro-step the sum is ONE chain of adds in step order, record order, point order.
// An env that is not live (`env` given and !active || frozen — which includes MCR_PARKED, an env whose episode ended in an earlier sub-step)
// contributes nothing: its rows are zeroed by a launch that does not accumulate and left as they are by one that does.  So the sub-step in
// which an episode ends is never reported: the env is parked behind it (frame_skip > 1) or already shows its new episode, whose reset pass
// emptied the store (the last sub-step; frame_skip = 1).
// ST_CC_OVERFLOW: more than MCR_CC_MAX fixture pairs touched and k_collide dropped the excess — DESIGN.md §3.1, THE DROP RULE: the first
// MCR_CC_MAX touching pairs are kept in the order k_collide finds them (pairs of cars ascending by (a, b), a < b; within a pair of cars
// ascending by fixture of a * 8 + fixture of b), the others take no part in the step; a function of the entry poses alone, mirrored by the
// oracle's orc_set_contact_cap.  The outputs describe the MCR_CC_MAX stored records.
//
// Shape: one wavefront per env, lane l = matrix cell (a, j) = (l >> 3, l & 7).  The env index is made wave-uniform (readfirstlane), so the
// count and every record's key, point count and impulses are scalar loads shared by the 64 lanes; every lane walks the <= MCR_CC_MAX
// records in order and adds where its pair matches.  The masks come from three ballots (touched, own hull, own wheel): car a's bits are
// byte a of each.  No LDS, no atomics, no scratch.  An env without a record — by far the common case — leaves after two loads: it stores
// zeros, or nothing when accumulating.  MCR_CO_LANES / 64 envs per workgroup.
//
// Ordering.  The kernel runs on the caller's stream behind launch_step, whose tail makes that stream wait for the whole step: the store
// is final.  The NEXT writer of the store is the next step's contact pass (k_collide pass 0, or the contact chain's own) — on the caller's
// stream itself, or on an internal stream behind a wait for W_BEGIN (posted by that step's main dynamics on the caller's stream) or for
// an event recorded there: behind this kernel in stream order either way, the argument k_stateobs relies on for `carf`.
#pragma once
#include "mcr_kernels.h"

#define MCR_CO_LANES 256                                    // four wavefronts per workgroup: four envs
#define MCR_CC_STORE_WORDS (MCR_CC_MAX * MCR_CC_WORDS + 4)  // u32 words of an env's store: count, overflow mark, joint order (2), the records
#define MCR_CO_HULL_BIT 8
#define MCR_CO_WHEEL_BIT 9

#ifndef MCR_DEVICE_FUNCTIONS_ONLY
__global__ __launch_bounds__(MCR_CO_LANES) void k_contactobs(const uint32_t* __restrict__ cc_store, const McrEnvState* __restrict__ envs, int B, int N,
                                                             int accumulate, McrContactObs co) {
  const int lane = (int)(threadIdx.x & 63u);
  const int env = __builtin_amdgcn_readfirstlane((int)blockIdx.x * (MCR_CO_LANES / 64) + (int)(threadIdx.x >> 6));
  if (env >= B) return;
  const int a = lane >> 3, j = lane & 7;
  const bool cell = a < N && j < N;
  double* __restrict__ out = co.impulse + ((size_t)env * N + a) * N + j;      // (dereferenced by the lanes of a cell only)
  int32_t* __restrict__ mout = co.mask + (size_t)env * N + lane;              // (by the lanes < N only)
  const uint32_t* __restrict__ store = cc_store + (size_t)env * MCR_CC_STORE_WORDS;
  bool live = true;
  if (envs) { const int32_t act = envs[env].active, frz = envs[env].frozen; live = act && !frz; }
  const int count = live ? (int)min(store[0], (uint32_t)MCR_CC_MAX) : 0;
  if (count == 0) {
    if (!accumulate) { if (cell) *out = 0.0; if (lane < N) *mout = 0; }
    return;
  }
  double acc = (accumulate && cell) ? *out : 0.0;
  bool touched = false, hull = false, wheel = false;
  for (int i = 0; i < count; ++i) {
    const uint32_t* __restrict__ rec = store + 4 + i * MCR_CC_WORDS;
    const uint32_t key = rec[0];
    const int n = (int)(rec[1] >> 8);
    const int ca = (int)(key & 15u), fa = (int)((key >> 4) & 15u), cb = (int)((key >> 8) & 15u), fb = (int)((key >> 12) & 15u);
    const bool asA = a == ca && j == cb, asB = a == cb && j == ca;
    if (asA || asB) {
      const int own = asA ? fa : fb;
      touched = true; hull |= own < 4; wheel |= own >= 4;
      if (n > 0) acc = acc + (double)__uint_as_float(rec[8]);
      if (n > 1) acc = acc + (double)__uint_as_float(rec[13]);
    }
  }
  const unsigned long long bt = __ballot(cell && touched), bh = __ballot(cell && hull), bw = __ballot(cell && wheel);
  if (cell) *out = acc;
  if (lane < N) {
    int32_t m = (int32_t)((bt >> (8 * lane)) & 0xffull);
    if ((bh >> (8 * lane)) & 0xffull) m |= 1 << MCR_CO_HULL_BIT;
    if ((bw >> (8 * lane)) & 0xffull) m |= 1 << MCR_CO_WHEEL_BIT;
    *mout = accumulate ? (*mout | m) : m;
  }
}
#endif
