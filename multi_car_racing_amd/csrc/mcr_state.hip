// mcr_state.hip — state access of the C ABI (include/mcr.h): the synchronous getters / setters, the per-env state blob through host memory
// (mcr_get_state_blob / mcr_set_state_blob) and its batched device-side form (k_envcopy.h: mcr_save_states / mcr_load_states /
// mcr_copy_states).  Nothing here launches or orders a step; what it needs from the step's unit is declared in mcr_env.h.
#include "mcr_env.h"
#include "k_envcopy.h"
#include <cassert>
#include <cstddef>
#include <cstring>

// ---------------------------------------------------------------------------- state access (synchronous)
extern "C" int mcr_get_state(mcr_env* h, float* bodies, float* joints, double* wheels, int32_t* limit, uint8_t* on_road, float* sleep) {
  if (!h) return MCR_ERR_ARG;
  HIPCHK(sync_state(h));
  const size_t BN = h->P.BN;
  std::vector<float> cf(CF_COUNT * BN); std::vector<double> cd(CD_COUNT * BN); std::vector<uint32_t> cu(CU_COUNT * BN);
  HIPCHK(hipMemcpy(cf.data(), h->P.carf, cf.size() * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(cd.data(), h->P.card, cd.size() * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(cu.data(), h->P.caru, cu.size() * 4, hipMemcpyDeviceToHost));
  for (size_t c = 0; c < BN; ++c) {
    if (bodies) for (int k = 0; k < 5; ++k) {
      float* o = bodies + (c * 5 + k) * 6;
      o[0] = cf[(CF_CX + k) * BN + c]; o[1] = cf[(CF_CY + k) * BN + c]; o[2] = cf[(CF_A + k) * BN + c];
      o[3] = cf[(CF_VX + k) * BN + c]; o[4] = cf[(CF_VY + k) * BN + c]; o[5] = cf[(CF_W + k) * BN + c];
    }
    if (sleep) for (int k = 0; k < 5; ++k) sleep[c * 5 + k] = cf[(CF_SLEEP + k) * BN + c];
    for (int k = 0; k < 4; ++k) {
      if (joints) { float* o = joints + (c * 4 + k) * 4; o[0] = cf[(CF_JIX + k) * BN + c]; o[1] = cf[(CF_JIY + k) * BN + c]; o[2] = cf[(CF_JIZ + k) * BN + c]; o[3] = cf[(CF_JM + k) * BN + c]; }
      if (wheels) {
        double* o = wheels + (c * 4 + k) * 5;
        o[0] = k >= 2 ? cd[(CD_GAS + k - 2) * BN + c] : 0.0; o[1] = cd[CD_BRAKE * BN + c]; o[2] = k < 2 ? cd[CD_STEER * BN + c] : 0.0;
        o[3] = cd[(CD_PHASE + k) * BN + c]; o[4] = cd[(CD_OMEGA + k) * BN + c];
      }
      if (limit) limit[c * 4 + k] = (cu[CU_LIMIT * BN + c] >> (2 * k)) & 3;
      if (on_road) on_road[c * 4 + k] = (cu[CU_ONROAD * BN + c] >> k) & 1;
    }
  }
  return MCR_OK;
}

extern "C" int mcr_set_bodies(mcr_env* h, const float* bodies) {
  if (!h || !bodies) return MCR_ERR_ARG;
  HIPCHK(sync_state(h));
  const size_t BN = h->P.BN;
  std::vector<float> cf(30 * BN);
  for (size_t c = 0; c < BN; ++c) for (int k = 0; k < 5; ++k) {
    const float* o = bodies + (c * 5 + k) * 6;
    cf[(CF_CX + k) * BN + c] = o[0]; cf[(CF_CY + k) * BN + c] = o[1]; cf[(CF_A + k) * BN + c] = o[2];
    cf[(CF_VX + k) * BN + c] = o[3]; cf[(CF_VY + k) * BN + c] = o[4]; cf[(CF_W + k) * BN + c] = o[5];
  }
  HIPCHK(hipMemcpy(h->P.carf, cf.data(), cf.size() * 4, hipMemcpyHostToDevice));
  h->bp_fresh = true; h->verdict_fresh = false;      // teleported cars: their broadphase proxies are re-created by the next contact pass
  return MCR_OK;
}

// mcr_get_state's `wheels` back: phase and omega of every wheel (columns 3 and 4; the controls in columns 0..2 are not state of their own)
extern "C" int mcr_set_wheels(mcr_env* h, const double* wheels) {
  if (!h || !wheels) return MCR_ERR_ARG;
  HIPCHK(sync_state(h));
  const size_t BN = h->P.BN;
  std::vector<double> cd(8 * BN);
  static_assert(CD_PHASE == CD_OMEGA + 4 && CD_REWARD == CD_PHASE + 4, "omega and phase of the four wheels are eight consecutive rows");
  for (size_t c = 0; c < BN; ++c) for (int k = 0; k < 4; ++k) {
    const double* o = wheels + (c * 4 + k) * 5;
    cd[(size_t)k * BN + c] = o[4]; cd[(size_t)(4 + k) * BN + c] = o[3];
  }
  HIPCHK(hipMemcpy(h->P.card + CD_OMEGA * BN, cd.data(), cd.size() * 8, hipMemcpyHostToDevice));
  return MCR_OK;
}

// mcr_get_env_state's reward, t and tile_flags back — those three fields and nothing else (visit counts, flags and the rest of the env record stay)
extern "C" int mcr_set_env_state(mcr_env* h, const double* reward, const double* t, const uint16_t* tile_flags) {
  if (!h) return MCR_ERR_ARG;
  HIPCHK(sync_state(h));
  const size_t BN = h->P.BN; const int B = h->P.B;
  if (reward) HIPCHK(hipMemcpy(h->P.card + CD_REWARD * BN, reward, BN * 8, hipMemcpyHostToDevice));
  if (t) HIPCHK(hipMemcpy2D((uint8_t*)h->P.env + offsetof(McrEnvState, t), sizeof(McrEnvState), t, sizeof(double), sizeof(double), (size_t)B, hipMemcpyHostToDevice));
  if (tile_flags) HIPCHK(hipMemcpy(h->P.tile_flags, tile_flags, sizeof(uint16_t) * MCR_TILE_CAP * (size_t)B, hipMemcpyHostToDevice));
  return MCR_OK;
}

extern "C" int mcr_get_env_state(mcr_env* h, double* reward, int32_t* tvc, uint8_t* backward, uint8_t* on_grass, double* t,
                                 uint16_t* tile_flags, int32_t* num_tiles) {
  if (!h) return MCR_ERR_ARG;
  HIPCHK(sync_state(h));
  const size_t BN = h->P.BN; const int B = h->P.B;
  std::vector<double> r(BN); std::vector<uint32_t> cu(CU_COUNT * BN); std::vector<McrEnvState> es(B);
  HIPCHK(hipMemcpy(r.data(), h->P.card + CD_REWARD * BN, BN * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(cu.data(), h->P.caru, cu.size() * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(es.data(), h->P.env, sizeof(McrEnvState) * B, hipMemcpyDeviceToHost));
  for (size_t c = 0; c < BN; ++c) {
    if (reward) reward[c] = r[c];
    if (tvc) tvc[c] = (int32_t)cu[CU_TVC * BN + c];
    if (backward) backward[c] = cu[CU_FLAGS * BN + c] & 1;
    if (on_grass) on_grass[c] = (cu[CU_FLAGS * BN + c] >> 1) & 1;
  }
  if (t) for (int e = 0; e < B; ++e) t[e] = es[e].t;
  if (tile_flags) HIPCHK(hipMemcpy(tile_flags, h->P.tile_flags, sizeof(uint16_t) * MCR_TILE_CAP * (size_t)B, hipMemcpyDeviceToHost));
  if (num_tiles) for (int e = 0; e < B; ++e) {
    McrSlotHeader H;
    HIPCHK(hipMemcpy(&H, h->P.slots + ((size_t)e * 2 + es[e].slot) * MCR_SLOT_BYTES, sizeof(H), hipMemcpyDeviceToHost));
    num_tiles[e] = H.T;
  }
  return MCR_OK;
}

// ---------------------------------------------------------------------------- the state of one env: section table, blob format
namespace {
const uint32_t BLOB_MAGIC = 0x3552434du;   // "MCR5": bumped whenever the layout of a blob (McrEnvState, slot image, field lists) changes
const size_t BLOB_HEADER_BYTES = 16;       // magic (carries the layout version), N, flags (bit 0: particles, bit 1: world), total bytes

// One section of an env's state: where it lives on the device — env e's bytes are `rows` rows of `row_bytes`, `row_stride` apart, from
// base + e * env_stride (+ the current slot for EC_SLOT) — and where in the blob: rows back to back at `blob_off`, the table's order,
// each offset rounded up to `align`.  THE description of the state: the blob's size, both host calls and k_envcopy's segment table walk it,
// so a new state array is one line in state_sections() (and a new BLOB_MAGIC).
struct StateSection {
  uint8_t kind;                 // EC_PLAIN, EC_ENVREC, EC_SLOT (k_envcopy.h)
  bool present;                 // this handle has the array
  uint8_t* base;
  uint64_t env_stride, rows, row_stride, row_bytes;
  size_t blob_off;
  size_t bytes() const { return rows * row_bytes; }
};
enum { STATE_SECTIONS = 17, STATE_ALIGNED_SECTIONS = 3 };
struct StateSections { StateSection s[STATE_SECTIONS]; int n; size_t total; };
// a segment per section, a gap in front of each aligned one, the tail up to the pitch (absent sections turn into gaps, they add none)
static_assert(STATE_SECTIONS + STATE_ALIGNED_SECTIONS + 1 <= MCR_EC_MAX_SEGS, "k_envcopy's segment table must hold every state section and the gaps");

StateSections state_sections(const mcr_env* h) {
  const McrParams& P = h->P; const uint64_t N = (uint64_t)P.N, BN = (uint64_t)P.BN;
  StateSections T; T.n = 0; T.total = BLOB_HEADER_BYTES;
  // reserved: an absent section's bytes keep their place in the blob (zeros)
  auto add = [&](int kind, void* base, uint64_t env_stride, uint64_t rows, uint64_t row_stride, uint64_t row_bytes, size_t align = 1, bool present = true, bool reserved = true) {
    assert(T.n < STATE_SECTIONS);
    StateSection& s = T.s[T.n++];
    s.kind = (uint8_t)kind; s.present = present; s.base = (uint8_t*)base; s.env_stride = env_stride; s.rows = rows; s.row_stride = row_stride; s.row_bytes = row_bytes;
    s.blob_off = T.total = align_up(T.total, align);
    if (present || reserved) T.total += s.bytes();
  };
  // SoA car state: `rows` arrays of one `elem` per car, the cars of an env side by side
  auto per_car = [&](void* base, uint64_t elem, uint64_t rows, size_t align = 1) { add(EC_PLAIN, base, elem * N, rows, elem * BN, elem * N, align); };
  auto per_env = [&](void* base, uint64_t bytes, bool present = true, bool reserved = true) { add(EC_PLAIN, base, bytes, 1, 0, bytes, 1, present, reserved); };
  const bool world = P.pid_tab != nullptr;      // the env's b2World across its episodes (k_world.h): ids, free leaf stack, meta
  per_car(P.carf, sizeof(float), CF_COUNT);
  per_car(P.card, sizeof(double), CD_COUNT, 8);
  per_car(P.caru, sizeof(uint32_t), CU_COUNT);
  add(EC_ENVREC, P.env, sizeof(McrEnvState), 1, 0, sizeof(McrEnvState), 8);
  per_env(P.tile_touch, sizeof(uint32_t) * MCR_TILE_CAP);
  per_env(P.tile_flags, sizeof(uint16_t) * MCR_TILE_CAP);
  per_env(P.cc_store, sizeof(uint32_t) * (MCR_CC_MAX * MCR_CC_WORDS + 4));
  per_env(P.viewp, sizeof(float) * MCR_VIEWP_FLOATS * N);
  per_env(P.carpoly, sizeof(float) * MCR_CARPOLY_FLOATS * N);
  per_car(P.bpf, sizeof(float4) * MCR_BP_FIX, BP_COUNT);
  per_env(P.bp_stamp, sizeof(uint32_t) * MCR_TILE_CAP * 4 * N);
  per_env(P.cc_stamp, sizeof(uint32_t) * mcr_cc_stamp_words(P.N));
  add(EC_SLOT, P.slots, 2 * (uint64_t)MCR_SLOT_BYTES, 1, 0, MCR_SLOT_BYTES, 16);
  per_env(P.pid_tab, sizeof(uint16_t) * MCR_PID_TAB, world);
  per_env(P.pid_stack, sizeof(uint16_t) * MCR_PID_STACK, world);
  per_env(P.pid_meta, sizeof(int32_t) * 4, world);
  per_env(P.particles, sizeof(uint32_t) * MCR_PART_WORDS * N, P.particles != nullptr, false);
  return T;
}
void blob_header(const mcr_env* h, size_t total, uint32_t* out4) {
  out4[0] = BLOB_MAGIC; out4[1] = (uint32_t)h->P.N; out4[2] = (h->P.particles ? 1u : 0u) | (h->P.pid_tab ? 2u : 0u); out4[3] = (uint32_t)total;
}
// section s of env `env` (whose current slot is `slot`) on the device
uint8_t* section_of(const StateSection& s, int env, int slot) { return s.base + (uint64_t)env * s.env_stride + (s.kind == EC_SLOT ? (uint64_t)slot * MCR_SLOT_BYTES : 0); }
hipError_t copy_rows(void* dst, size_t dst_pitch, const void* src, size_t src_pitch, const StateSection& s, hipMemcpyKind dir) {
  return s.rows == 1 ? hipMemcpy(dst, src, s.row_bytes, dir) : hipMemcpy2D(dst, dst_pitch, src, src_pitch, s.row_bytes, s.rows, dir);
}
}  // namespace

extern "C" size_t mcr_state_blob_bytes(const mcr_env* h) { return h ? state_sections(h).total : 0; }
extern "C" size_t mcr_state_blob_pitch(const mcr_env* h) { return h ? align_up(mcr_state_blob_bytes(h), 16) : 0; }
extern "C" int mcr_state_blob_header(const mcr_env* h, uint32_t* out4) {
  if (!h || !out4) { g_err = "null argument"; return MCR_ERR_ARG; }
  blob_header(h, mcr_state_blob_bytes(h), out4);
  return MCR_OK;
}

// ---------------------------------------------------------------------------- full state snapshot / restore through host memory
extern "C" int mcr_get_state_blob(mcr_env* h, int env, void* blob_out) {
  if (!h || !blob_out) { g_err = "null argument"; return MCR_ERR_ARG; }
  if (env < 0 || env >= h->P.B) { g_err = "env out of range"; return MCR_ERR_ARG; }
  if (!h->any_reset) { g_err = "state snapshot before reset()"; return MCR_ERR_STATE; }
  HIPCHK(sync_state(h));
  const StateSections T = state_sections(h);
  uint8_t* b = (uint8_t*)blob_out;
  memset(b, 0, T.total);
  blob_header(h, T.total, (uint32_t*)b);
  McrEnvState es;                                  // first: its `slot` says which episode image is the env's
  HIPCHK(hipMemcpy(&es, h->P.env + env, sizeof(es), hipMemcpyDeviceToHost));
  for (int i = 0; i < T.n; ++i) {
    const StateSection& s = T.s[i];
    if (!s.present) continue;
    if (s.kind == EC_ENVREC) memcpy(b + s.blob_off, &es, sizeof(es));
    else HIPCHK(copy_rows(b + s.blob_off, s.row_bytes, section_of(s, env, es.slot), s.row_stride, s, hipMemcpyDeviceToHost));
  }
  return MCR_OK;
}

extern "C" int mcr_set_state_blob(mcr_env* h, int env, const void* blob) {
  if (!h || !blob) { g_err = "null argument"; return MCR_ERR_ARG; }
  if (env < 0 || env >= h->P.B) { g_err = "env out of range"; return MCR_ERR_ARG; }
  const uint8_t* b = (const uint8_t*)blob;
  const StateSections T = state_sections(h);
  uint32_t want[4]; blob_header(h, T.total, want);
  const uint32_t* got = (const uint32_t*)b;
  if (got[0] != want[0] || got[1] != want[1]) { g_err = "not a state blob of this build and num_agents"; return MCR_ERR_ARG; }
  if (got[2] != want[2] || got[3] != want[3]) { g_err = "state blob was taken from a handle with another skid_particles or fresh_world setting"; return MCR_ERR_ARG; }
  HIPCHK(sync_state(h));
  // the staging protocol (which slot is current, whether a staged episode waits, install counter) belongs to the
  // TARGET handle; everything else of the env record comes from the blob, and the episode image goes into the target's current slot
  McrEnvState cur;
  HIPCHK(hipMemcpy(&cur, h->P.env + env, sizeof(cur), hipMemcpyDeviceToHost));
  for (int i = 0; i < T.n; ++i) {
    const StateSection& s = T.s[i];
    if (!s.present) continue;
    if (s.kind == EC_ENVREC) {
      McrEnvState in;
      memcpy(&in, b + s.blob_off, sizeof(in));
      in.slot = cur.slot; in.staged_ready = cur.staged_ready; in.consumed = cur.consumed;
      HIPCHK(hipMemcpy(section_of(s, env, cur.slot), &in, sizeof(in), hipMemcpyHostToDevice));
    } else HIPCHK(copy_rows(section_of(s, env, cur.slot), s.row_stride, b + s.blob_off, s.row_bytes, s, hipMemcpyHostToDevice));
  }
  h->any_reset = true; h->verdict_fresh = false;
  return MCR_OK;
}

// ---------------------------------------------------------------------------- batched snapshot / restore / clone on the device (k_envcopy.h)
namespace {
// The segment table of k_envcopy: the present sections as they stand in state_sections(), each with the access widths its addresses allow, and
// an EC_ZERO entry for every stretch of the blob row between them that holds no state (alignment padding, a reserved section this handle
// lacks, the tail up to the row pitch).
int envcopy_table(const mcr_env* h, McrEnvCopy& a) {
  const StateSections T = state_sections(h);
  const size_t pitch = align_up(T.total, 16);
  a.nseg = 0; a.B = h->P.B; a.pitch = pitch; a.env = h->P.env;
  blob_header(h, T.total, a.hdr);
  auto width = [](uint64_t bits) { uint64_t w = 16; while (bits & (w - 1)) w >>= 1; return (uint8_t)w; };
  size_t cursor = BLOB_HEADER_BYTES;                                     // the header: the kernel's own
  bool ok = true;
  auto push = [&](const McrEcSeg& g) { if (a.nseg < MCR_EC_MAX_SEGS) a.seg[a.nseg++] = g; else ok = false; };
  auto zero_to = [&](size_t off) {
    if (off > cursor) { McrEcSeg z{}; z.kind = EC_ZERO; z.rows = 1; z.row_bytes = (uint32_t)(off - cursor); z.blob_off = (uint32_t)cursor; z.w_blob = z.w_env = width(cursor | (off - cursor)); push(z); }
    cursor = off;
  };
  for (int i = 0; i < T.n; ++i) {
    const StateSection& s = T.s[i];
    if (!s.present) continue;
    zero_to(s.blob_off);
    McrEcSeg g{}; g.kind = s.kind; g.base = s.base; g.env_stride = s.env_stride; g.rows = (uint32_t)s.rows; g.row_stride = s.row_stride;
    g.row_bytes = (uint32_t)s.row_bytes; g.blob_off = (uint32_t)s.blob_off;
    g.w_env = width((uint64_t)(uintptr_t)s.base | s.env_stride | s.row_bytes | (s.rows > 1 ? s.row_stride : 0) | (s.kind == EC_SLOT ? (uint64_t)MCR_SLOT_BYTES : 0));
    g.w_blob = width((uint64_t)g.w_env | s.blob_off);                    // (blob rows start at multiples of 16: checked by envcopy)
    push(g); cursor = s.blob_off + s.bytes();
  }
  zero_to(pitch);
  if (!ok) { g_err = "state copy: the segment table is full (MCR_EC_MAX_SEGS)"; return MCR_ERR_STATE; }
  return MCR_OK;
}
// What the three calls share behind their null checks: arguments, the capture rule, the pending flag scans in front (they read and write what
// the copy reads and writes), the launch; behind a restore / clone mcr_set_state_blob's host bookkeeping (the next step re-evaluates the touch
// verdicts and the contact list) and the state vector.
int envcopy(mcr_env* h, McrEnvCopyMode mode, const char* who, const int32_t* d_ids, const int32_t* d_src_ids, int n, void* d_blobs, int32_t* d_refused, hipStream_t st) {
  if (mode != ENV_TO_ENV && ((uintptr_t)d_blobs & 15) != 0) { g_err = std::string(who) + ": d_blobs must be 16-byte aligned"; return MCR_ERR_ARG; }
  if (n < 0 || n > h->P.B) { g_err = std::string(who) + ": n must be 0 .. num_envs"; return MCR_ERR_ARG; }
  if (capturing(st)) { g_err = std::string(who) + " inside a stream capture (the handle's host bookkeeping would not be replayed)"; return MCR_ERR_STATE; }
  if (mode != BLOB_TO_ENV && !h->any_reset) { g_err = std::string(who) + " before reset()"; return MCR_ERR_STATE; }
  if (n == 0) return MCR_OK;
  McrEnvCopy a{};
  if (int rc = envcopy_table(h, a)) return rc;
  a.ids = d_ids; a.src_ids = d_src_ids; a.blobs = (uint8_t*)d_blobs; a.refused = d_refused;
  flush_flags(h, st);
  if (mode == ENV_TO_BLOB) hipLaunchKernelGGL(k_envcopy<ENV_TO_BLOB>, dim3(n), dim3(MCR_EC_LANES), 0, st, a);
  else if (mode == BLOB_TO_ENV) hipLaunchKernelGGL(k_envcopy<BLOB_TO_ENV>, dim3(n), dim3(MCR_EC_LANES), 0, st, a);
  else hipLaunchKernelGGL(k_envcopy<ENV_TO_ENV>, dim3(n), dim3(MCR_EC_LANES), 0, st, a);
  if (mode != ENV_TO_BLOB) { h->any_reset = true; h->verdict_fresh = false; launch_derived(h, st); }
  HIPCHK(hipGetLastError());
  return MCR_OK;
}
}  // namespace

extern "C" int mcr_save_states(mcr_env* h, const int32_t* d_env_ids, int n, void* d_blobs, void* stream) {
  if (!h || !d_blobs) { g_err = "mcr_save_states: null argument"; return MCR_ERR_ARG; }
  return envcopy(h, ENV_TO_BLOB, "mcr_save_states", d_env_ids, nullptr, n, d_blobs, nullptr, (hipStream_t)stream);
}
extern "C" int mcr_load_states(mcr_env* h, const int32_t* d_env_ids, int n, const void* d_blobs, int32_t* d_refused, void* stream) {
  if (!h || !d_blobs) { g_err = "mcr_load_states: null argument"; return MCR_ERR_ARG; }
  return envcopy(h, BLOB_TO_ENV, "mcr_load_states", d_env_ids, nullptr, n, (void*)d_blobs, d_refused, (hipStream_t)stream);
}
extern "C" int mcr_copy_states(mcr_env* h, const int32_t* d_src_ids, const int32_t* d_dst_ids, int n, void* stream) {
  if (!h || !d_src_ids || !d_dst_ids) { g_err = "mcr_copy_states: null argument"; return MCR_ERR_ARG; }
  return envcopy(h, ENV_TO_ENV, "mcr_copy_states", d_dst_ids, d_src_ids, n, nullptr, nullptr, (hipStream_t)stream);
}

__global__ void k_positions(McrParams p, float* out) {
  const int ci = blockIdx.x * blockDim.x + threadIdx.x;
  if (ci >= p.BN) return;
  const McrShapes& S = *p.shapes;
  Xf xf = xf_of(v2(p.carf[CF_CX * p.BN + ci], p.carf[CF_CY * p.BN + ci]), p.carf[CF_A * p.BN + ci], v2(S.hull_lcx, S.hull_lcy));
  out[ci * 2] = xf.p.x; out[ci * 2 + 1] = xf.p.y;
}
extern "C" int mcr_get_positions(mcr_env* h, float* pos) {
  if (!h || !pos) return MCR_ERR_ARG;
  float* d = nullptr;
  HIPCHK(hipMalloc(&d, sizeof(float) * 2 * h->P.BN));
  hipLaunchKernelGGL(k_positions, dim3((h->P.BN + 63) / 64), dim3(64), 0, 0, h->P, d);
  HIPCHK(hipMemcpy(pos, d, sizeof(float) * 2 * h->P.BN, hipMemcpyDeviceToHost));
  (void)hipFree(d);
  return MCR_OK;
}
