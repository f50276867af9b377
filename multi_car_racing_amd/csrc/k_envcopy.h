// k_envcopy.h — batched snapshot / restore / clone of env states on the device (include/mcr.h: mcr_save_states, mcr_load_states,
// mcr_copy_states).  One kernel, three modes: env -> blob row, blob row -> env, env -> env.  The blob bytes are those of mcr_get_state_blob,
// header included; the kernel knows nothing about that layout: it walks a SEGMENT TABLE the host makes for every call (mcr_state.hip:
// envcopy_table) from the one description of an env's state, state_sections() — the table mcr_get_state_blob / mcr_set_state_blob walk
// too, so sections, strides and blob offsets cannot differ between the host and the device format.  One entry per section this handle has —
// where it lives on the device (base, bytes between two envs, rows, bytes between two rows, bytes per row) and where in the blob — plus
// EC_ZERO entries for the bytes the host version leaves zero (padding between sections, an absent world section, the tail up to the row pitch).
//
// One workgroup per listed env; the workgroup takes the segments one after the other, its lanes striding over each.  The kernel moves bytes
// and computes nothing: what counts is the width of the accesses and how many are in flight.  The host picks the access width per segment —
// 16 bytes where base, strides, row size and blob offset are all 16-byte multiples, else the widest power of two they share — separately for
// blob copies and for env -> env copies (no blob offset involved).  A contiguous segment (the 96 KB episode slot, bp_stamp, the tile arrays, the
// manifold store, the id tables) is read four accesses per lane ahead of its stores; the SoA sections (rows of N elements, BN apart: a few
// hundred bytes) go unit by unit.  No LDS, plain loads and stores.
//
// What stays the TARGET's on restore / clone (mcr_set_state_blob's rule): the staging protocol of its env record — slot, staged_ready, consumed —
// is never written (the other nine words are; the refill service may be setting staged_ready at that very moment), the episode image goes
// into the target's CURRENT slot, and neither the staged slot (slot ^ 1) nor consumed_host is touched.
// A restore REFUSES a row whose header is not this handle's (magic, N, flags word, total bytes) or whose env id is outside 0 .. B-1: the env
// stays untouched and the row is counted in `refused`.  A save of an id outside 0 .. B-1 writes a zero header (a later restore refuses the
// row); a clone with such an id on either side is skipped.
#pragma once
#include "mcr_kernels.h"
#include <cstddef>

#define MCR_EC_LANES 256
#define MCR_EC_MAX_SEGS 28         // every state section + the gaps between them (mcr_state.hip: a static_assert beside the section table)
enum McrEnvCopyMode { ENV_TO_BLOB = 0, BLOB_TO_ENV = 1, ENV_TO_ENV = 2 };
enum McrEcKind {
  EC_PLAIN = 0,
  EC_ENVREC = 1,    // the env record: restore / clone leave the target's staging words alone
  EC_SLOT = 2,      // the episode slot: + (the env's current slot) * MCR_SLOT_BYTES
  EC_ZERO = 3       // blob bytes [blob_off, blob_off + row_bytes) that hold no state: zeros on save, skipped otherwise
};
struct McrEcSeg {
  uint8_t* base;                 // the device array
  uint64_t env_stride;           // bytes from env e to env e + 1
  uint64_t row_stride;           // bytes from row r to row r + 1 on the device (in the blob: row_bytes)
  uint32_t rows, row_bytes;
  uint32_t blob_off;
  uint8_t kind, w_blob, w_env, pad;   // access width in bytes (16, 8, 4, 2, 1) of a copy from / to a blob, and of an env -> env copy
};
struct McrEnvCopy {
  McrEcSeg seg[MCR_EC_MAX_SEGS];
  int32_t nseg, B;
  uint32_t hdr[4];               // this handle's blob header: magic, N, flags, total bytes
  uint64_t pitch;                // bytes from blob row i to row i + 1 (a multiple of 16)
  const int32_t* ids;            // [n] env of row i (save: the source, restore / clone: the target); null: env i
  const int32_t* src_ids;        // [n] clone: the source env of row i
  uint8_t* blobs;                // [n][pitch]
  int32_t* refused;              // restore: rows skipped (may be null)
  const McrEnvState* env;        // [B] (which slot is an env's current one)
};

#ifndef MCR_DEVICE_FUNCTIONS_ONLY
static_assert(sizeof(McrEnvState) == 48 && offsetof(McrEnvState, slot) == 12 && offsetof(McrEnvState, staged_ready) == 16 && offsetof(McrEnvState, consumed) == 20,
              "k_envcopy skips words 3..5 of the env record on restore / clone");

// rows x row_bytes from s to d in units of T; a contiguous segment (rows == 1) keeps four loads per lane in flight
template <typename T>
__device__ __forceinline__ void ec_copy(uint8_t* d, uint64_t d_rs, const uint8_t* s, uint64_t s_rs, uint32_t rows, uint32_t row_bytes) {
  const uint32_t upr = row_bytes / (uint32_t)sizeof(T);
  if (rows == 1) {
    T* dd = (T*)d; const T* ss = (const T*)s;
    uint32_t i = threadIdx.x;
    for (; i + 3 * MCR_EC_LANES < upr; i += 4 * MCR_EC_LANES) {
      const T a = ss[i], b = ss[i + MCR_EC_LANES], c = ss[i + 2 * MCR_EC_LANES], e = ss[i + 3 * MCR_EC_LANES];
      dd[i] = a; dd[i + MCR_EC_LANES] = b; dd[i + 2 * MCR_EC_LANES] = c; dd[i + 3 * MCR_EC_LANES] = e;
    }
    for (; i < upr; i += MCR_EC_LANES) dd[i] = ss[i];
    return;
  }
  const uint32_t n = rows * upr;
  for (uint32_t u = threadIdx.x; u < n; u += MCR_EC_LANES) {
    const uint32_t r = u / upr, c = u - r * upr;
    ((T*)(d + r * d_rs))[c] = ((const T*)(s + r * s_rs))[c];
  }
}
template <typename T>
__device__ __forceinline__ void ec_zero(uint8_t* d, uint32_t bytes) {
  T z; memset(&z, 0, sizeof(T));
  for (uint32_t i = threadIdx.x; i < bytes / (uint32_t)sizeof(T); i += MCR_EC_LANES) ((T*)d)[i] = z;
}
#define MCR_EC_BY_WIDTH(w, call)                                                                        \
  switch (w) {                                                                                          \
    case 16: call(uint4); break;                                                                        \
    case 8: call(uint2); break;                                                                         \
    case 4: call(uint32_t); break;                                                                      \
    case 2: call(uint16_t); break;                                                                      \
    default: call(uint8_t); break;                                                                      \
  }

template <int MODE>
__global__ __launch_bounds__(MCR_EC_LANES) void k_envcopy(McrEnvCopy a) {
  const int row = (int)blockIdx.x;
  const int env = a.ids ? a.ids[row] : row;
  const bool env_ok = (uint32_t)env < (uint32_t)a.B;
  uint8_t* const blob = MODE == ENV_TO_ENV ? nullptr : a.blobs + (size_t)row * a.pitch;
  int src = env;
  if (MODE == ENV_TO_BLOB) {
    if (threadIdx.x == 0) *(uint4*)blob = env_ok ? make_uint4(a.hdr[0], a.hdr[1], a.hdr[2], a.hdr[3]) : make_uint4(0u, 0u, 0u, 0u);
    if (!env_ok) return;
  }
  if (MODE == BLOB_TO_ENV) {
    const uint4 hd = *(const uint4*)blob;          // (every lane, one address: the verdict is the workgroup's)
    if (!env_ok || hd.x != a.hdr[0] || hd.y != a.hdr[1] || hd.z != a.hdr[2] || hd.w != a.hdr[3]) {
      if (threadIdx.x == 0 && a.refused) atomicAdd(a.refused, 1);
      return;
    }
  }
  if (MODE == ENV_TO_ENV) {
    src = a.src_ids[row];
    if (!env_ok || (uint32_t)src >= (uint32_t)a.B) return;
  }
  // the current slots (restore / clone never write that word of the target's record: reading it here races with nothing in this launch)
  const uint64_t slot_env = (uint64_t)(a.env[env].slot & 1) * MCR_SLOT_BYTES;
  const uint64_t slot_src = MODE == ENV_TO_ENV ? (uint64_t)(a.env[src].slot & 1) * MCR_SLOT_BYTES : 0;
  for (int si = 0; si < a.nseg; ++si) {
    const McrEcSeg& g = a.seg[si];
    const int kind = g.kind;
    if (kind == EC_ZERO) {
      if (MODE == ENV_TO_BLOB) {
#define EC_CALL(T) ec_zero<T>(blob + g.blob_off, g.row_bytes)
        MCR_EC_BY_WIDTH(g.w_blob, EC_CALL)
#undef EC_CALL
      }
      continue;
    }
    uint8_t* const dev = g.base + (uint64_t)env * g.env_stride + (kind == EC_SLOT ? slot_env : 0);     // this row's env
    uint8_t* d; const uint8_t* s; uint64_t d_rs, s_rs; int w;
    if (MODE == ENV_TO_BLOB) { d = blob + g.blob_off; d_rs = g.row_bytes; s = dev; s_rs = g.row_stride; w = g.w_blob; }
    else if (MODE == BLOB_TO_ENV) { d = dev; d_rs = g.row_stride; s = blob + g.blob_off; s_rs = g.row_bytes; w = g.w_blob; }
    else { d = dev; d_rs = g.row_stride; s = g.base + (uint64_t)src * g.env_stride + (kind == EC_SLOT ? slot_src : 0); s_rs = g.row_stride; w = g.w_env; }
    if (kind == EC_ENVREC && MODE != ENV_TO_BLOB) {
      const uint32_t wd = threadIdx.x;
      if (wd < sizeof(McrEnvState) / 4 && (wd * 4 < offsetof(McrEnvState, slot) || wd * 4 > offsetof(McrEnvState, consumed))) ((uint32_t*)d)[wd] = ((const uint32_t*)s)[wd];
      continue;
    }
#define EC_CALL(T) ec_copy<T>(d, d_rs, s, s_rs, g.rows, g.row_bytes)
    MCR_EC_BY_WIDTH(w, EC_CALL)
#undef EC_CALL
  }
}
#endif
