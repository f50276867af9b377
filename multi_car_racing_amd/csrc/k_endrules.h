// k_endrules.h — early episode ending on the device (include/mcr.h: mcr_set_end_rules): "no new tile for P env steps" and "off the road for
// G env steps", counted per env behind every env step taken with actions; an env whose rule is met is ARMED, and the NEXT env step taken with
// actions ends its episode through the one place that decides `done` — the bookkeeping block of k_dynamics.h, which loads the armed byte
// (McrParams::end_armed) beside the TimeLimit test.  So an episode ends one env step AFTER its rule is first met: the price of leaving the
// step's topology alone (tests/end_rules_ref.py is the same definition as a wrapper round the oracle, lag included).
//
// Definition.  Per env e: counters[e] = {idle, offroad, tvc_sum, 0} (int32 x 4, the caller's), armed[e] and reason[e] (u8, the caller's).
// The counted cars are the cars a < N with bit a of agent_mask set.  s = sum over them of CU_TVC (tile_visited_count; u32 wrapping, stored
// as int32); off(a) = CU_ONROAD of car a is 0 — no wheel has a tile under it as of the step that just ended, the bits k_stateobs publishes
// as features 8-11 (NOT CU_FLAGS: a phase-word step leaves those scans to its successor); cond = every counted car is off (mode "all", 0)
// or some counted car is off (mode "any", 1).
//   ADVANCE (behind an env step with actions; `accumulate` = a later sub-step of a macro-step):
//     was = armed[e].  reason[e] = was, or — accumulating — reason[e] |= was: the word the env entered the step with, i.e. whether and why
//     that step ended its episode by these rules (an armed env was live when the step began: only live envs are ever armed).
//     live (active, not frozen — a parked env of a macro-step is not live):
//       steps == 0 (the first state of an episode: the step re-spawned the env):  idle = offroad = 0, tvc_sum = s, armed = 0
//       else:  idle = (s != tvc_sum) ? 0 : min(idle + 1, INT32_MAX);  tvc_sum = s;  offroad = cond ? min(offroad + 1, INT32_MAX) : 0;
//              armed = (P > 0 && idle >= P ? 1 : 0) | (G > 0 && offroad >= G ? 2 : 0);  the reserved word is written 0
//     not live:  counters untouched, armed = 0
//   SETTLE (behind a reset, a restore, a clone; mcr_end_rules_now): reason untouched.  live with steps == 0: as above.  live otherwise: the
//     counters are left alone and armed is recomputed from them — a caller who restores counters[] with the states continues bit for bit.
//     not live: counters untouched, armed = 0.
//
// Shape: one lane per env, one wavefront per workgroup.  An env costs three loads of its record, 2 loads per counted car (CU_TVC, CU_ONROAD:
// SoA rows [field][BN], car index env * N + a — consecutive lanes read consecutive words for N = 1, every other word of the same lines for
// N = 2), one 16-byte load and store of the counter row and a handful of integer operations: the kernel is bound by launch and load latency,
// not by bandwidth (B = 4096, N = 2: 64 KB of counters, 64 KB of car words).  64-lane workgroups spread those few wavefronts over as many CUs
// as there are (B / 64 of them), each with one dependent chain of loads; a larger workgroup would only stack the chains on fewer CUs.  No
// LDS, no atomics, no scratch.  Every access is guarded by env < B.
//
// Ordering.  On the caller's stream behind launch_step, whose tail makes that stream wait for the whole step: record, CU_TVC and CU_ONROAD
// are final (the scans a phase-word step leaves pending write CU_FLAGS only).  The next reader of armed[] is the next step's dynamics — the
// main launch on the caller's stream itself, the list chains on internal streams behind W_BEGIN (posted by that launch) or behind an event
// recorded on the caller's stream: behind this kernel in stream order either way.
#pragma once
#include "mcr_kernels.h"

#define MCR_ER_LANES 64
#define MCR_END_IDLE 1          // bits of armed[] / reason[]
#define MCR_END_OFFROAD 2
enum { MCR_ER_ADVANCE = 0, MCR_ER_ADVANCE_ACCUMULATE = 1, MCR_ER_SETTLE = 2 };

#ifndef MCR_DEVICE_FUNCTIONS_ONLY
__device__ __forceinline__ int32_t mcr_sat_inc(int32_t v) { return v == 0x7fffffff ? v : v + 1; }

__global__ __launch_bounds__(MCR_ER_LANES) void k_endrules(const McrEnvState* __restrict__ envs, const uint32_t* __restrict__ caru, int B, int N, int pass,
                                                           McrEndRules er) {
  const int env = (int)blockIdx.x * MCR_ER_LANES + (int)threadIdx.x;
  if (env >= B) return;
  const int32_t act = envs[env].active, frz = envs[env].frozen, steps = envs[env].steps;
  const uint8_t was = er.armed[env];
  if (pass == MCR_ER_ADVANCE) er.reason[env] = was;
  else if (pass == MCR_ER_ADVANCE_ACCUMULATE && was) er.reason[env] = (uint8_t)(er.reason[env] | was);
  if (!(act && !frz)) { if (was) er.armed[env] = 0; return; }
  const int BN = B * N;
  uint32_t s = 0u;
  bool all_off = true, any_off = false;
#pragma unroll
  for (int a = 0; a < MCR_MAX_AGENTS; ++a) {
    if (a < N && ((er.agent_mask >> a) & 1u)) {
      const int ci = env * N + a;
      s += caru[CU_TVC * BN + ci];
      const bool off = caru[CU_ONROAD * BN + ci] == 0u;
      all_off = all_off && off; any_off = any_off || off;
    }
  }
  int4* __restrict__ row = reinterpret_cast<int4*>(er.counters) + env;
  int4 c = *row;
  bool store = true;
  if (steps == 0) { c.x = 0; c.y = 0; c.z = (int32_t)s; c.w = 0; }
  else if (pass != MCR_ER_SETTLE) {
    c.x = ((int32_t)s != c.z) ? 0 : mcr_sat_inc(c.x);
    c.z = (int32_t)s;
    c.y = (er.any_mode ? any_off : all_off) ? mcr_sat_inc(c.y) : 0;
    c.w = 0;
  } else store = false;
  if (store) *row = c;
  uint8_t armed = 0;
  if (steps != 0) armed = (uint8_t)(((er.patience > 0 && c.x >= er.patience) ? MCR_END_IDLE : 0) | ((er.offroad_patience > 0 && c.y >= er.offroad_patience) ? MCR_END_OFFROAD : 0));
  if (armed != was) er.armed[env] = armed;
}
#endif
