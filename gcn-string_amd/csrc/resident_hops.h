// What the multi-hop propagation kernels (appnp.hip, cheb.hip) literally share: the LDS budget of the resident route (one
// workgroup per (graph, block of cb columns) that keeps the graph's rows in LDS across all hops), the row gathers of both
// routes -- one fmaf chain over the row's entries in CSR order from +0, the expression both files promise bit for bit --, the
// column-block rule and the operand checks.  Include behind common.h and conv_tile.h.  Everything is force-inlined or static
// and sits in the including file's anonymous namespace.
//
// The epilogue of a hop (APPNP's teleport, the Chebyshev recurrences), the element-to-thread maps and the rule that picks a
// route stay in their files.
#pragma once
#include <algorithm>

#include "common.h"
#include "conv_tile.h"

namespace {

constexpr int kResThreads = 1024;
constexpr int kResLdsMax = 128 * 1024;       // LDS the two z buffers and the row pointers of a block must fit
constexpr int kResLdsDevMax = 160 * 1024;    // LDS of a workgroup with its staged entries, where the device grants it
constexpr int kResU = 8;                     // entries per row per trip
constexpr int kResEntPerRow = 32;            // entries staged per row of the tallest graph, where LDS is left for more
constexpr int kResEntGoal = 16;              // entries per row the column-block rule wants staged (the project's graphs: ~15)
constexpr int kHopThreads = 256;
constexpr int kResCbMax = 256;               // a row of a block on at most one wave

#ifdef __HIPCC__
__device__ __forceinline__ float4 sel4(bool c, float4 a, float4 b) {
  return make_float4(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w);
}

// The entries of row range [ea, eb) of the staged arrays, in aligned groups of eight: one 16-byte read of the eight columns and
// two of the weights, then the eight gathers, all issued before the first fma.  A slot outside [ea, eb) or an entry outside the
// graph (column 0xFFFF) leaves the accumulator as it is and reads row 0 (one address for all such lanes: a broadcast, no
// bank cycles of its own).
template <bool WEIGHTED>
__device__ __forceinline__ float4 res_row_staged(const uint16_t* s_col, const float* s_val, const char* cur, int rowb, int sub16,
                                                 int ea, int eb, float4 acc) {
  static_assert(kResU == 8, "eight 16-bit columns per 16-byte read");
  for (int e = ea & ~7; e < eb; e += 8) {
    const uint4 cw = *reinterpret_cast<const uint4*>(s_col + e);
    float4 v0 = make_float4(1.f, 1.f, 1.f, 1.f), v1 = v0;
    if (WEIGHTED) { v0 = *reinterpret_cast<const float4*>(s_val + e); v1 = *reinterpret_cast<const float4*>(s_val + e + 4); }
    const unsigned w[4] = {cw.x, cw.y, cw.z, cw.w};
    const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    int c[8];
    bool ok[8];
    float4 h[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      c[u] = (int)((w[u >> 1] >> (16 * (u & 1))) & 0xFFFFu);
      ok[u] = e + u >= ea && e + u < eb && c[u] != 0xFFFF;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) h[u] = *reinterpret_cast<const float4*>(cur + (ok[u] ? c[u] * rowb + sub16 : 0));
#pragma unroll
    for (int u = 0; u < 8; ++u) acc = sel4(ok[u], fma4(v[u], h[u], acc), acc);
  }
  return acc;
}
// the same over entries that were not staged (a graph with more entries than the LDS left over holds): read from global memory
template <bool WEIGHTED>
__device__ __forceinline__ float4 res_row_global(const int32_t* __restrict__ colidx, const float* __restrict__ vals, int r0, int ng,
                                                 const char* cur, int rowb, int sub16, int ea, int eb, float4 acc) {
  for (int e = ea; e < eb; e += kResU) {
    int c[kResU];
    float v[kResU];
    float4 h[kResU];
#pragma unroll
    for (int u = 0; u < kResU; ++u) {
      const int eu = min(e + u, eb - 1);
      c[u] = colidx[eu] - r0;
      v[u] = WEIGHTED ? vals[eu] : 1.0f;
    }
#pragma unroll
    for (int u = 0; u < kResU; ++u)
      h[u] = *reinterpret_cast<const float4*>(cur + (e + u < eb && (unsigned)c[u] < (unsigned)ng ? c[u] * rowb + sub16 : 0));
#pragma unroll
    for (int u = 0; u < kResU; ++u) acc = sel4(e + u < eb && (unsigned)c[u] < (unsigned)ng, fma4(v[u], h[u], acc), acc);
  }
  return acc;
}

// The streamed route's row: entries [ea, eb) of `row` gathered from z (leading dimension ldz, already offset to the thread's
// columns), four columns per thread or one.  An entry whose column lies outside [0, n) contributes nothing and reads the
// thread's own row.
template <bool WEIGHTED>
__device__ __forceinline__ float4 hop_row4(const int32_t* colidx, const float* vals, const float* zc, int64_t ldz, int32_t n, int64_t row,
                                           int ea, int eb) {
  float4 acc = zero4();
  for (int e = ea; e < eb; e += kResU) {
    int c[kResU];
    float v[kResU];
    float4 h[kResU];
#pragma unroll
    for (int u = 0; u < kResU; ++u) {
      const int eu = min(e + u, eb - 1);
      c[u] = colidx[eu];
      v[u] = WEIGHTED ? vals[eu] : 1.0f;
    }
#pragma unroll
    for (int u = 0; u < kResU; ++u) h[u] = load4(zc + (int64_t)((unsigned)c[u] < (unsigned)n ? c[u] : (int)row) * ldz);
#pragma unroll
    for (int u = 0; u < kResU; ++u) acc = sel4(e + u < eb && (unsigned)c[u] < (unsigned)n, fma4(v[u], h[u], acc), acc);
  }
  return acc;
}
template <bool WEIGHTED>
__device__ __forceinline__ float hop_row1(const int32_t* colidx, const float* vals, const float* zc, int64_t ldz, int32_t n, int ea,
                                          int eb) {
  float acc = 0.f;
  for (int e = ea; e < eb; ++e) {
    const int c = colidx[e];
    const float v = WEIGHTED ? vals[e] : 1.0f;
    if ((unsigned)c < (unsigned)n) acc = fmaf(v, zc[(int64_t)c * ldz], acc);
  }
  return acc;
}
#endif  // __HIPCC__

// ---- host side ------------------------------------------------------------------------------------------------------------
size_t res_rp_bytes(int64_t rows) { return (size_t)((rows + 1 + 3) & ~3ll) * 4; }
// bytes of a staged entry: a 16-bit column inside the graph, and its weight where the operator has values
size_t res_ent_bytes(bool weighted) { return weighted ? 6 : 2; }
// a block of cb columns of a graph of `rows` rows fits: both buffers and the row pointers
bool res_fits(int64_t rows, int cb) { return rows > 0 && rows < 0xFFFF && cb >= 4 && cb % 4 == 0 && cb <= kResCbMax &&
                                             2ull * (uint64_t)rows * cb * 4 + res_rp_bytes(rows) <= (size_t)kResLdsMax; }
bool res_shape_ok(int64_t max_graph_rows, int32_t f, int64_t ldx) {
  return f > 0 && f % 4 == 0 && ldx >= f && ldx % 4 == 0 && res_fits(max_graph_rows, 4);
}
// entries staged beside a block of cb columns (a multiple of eight): what the rest of `lds_max` bytes holds, at most
// kResEntPerRow per row of the tallest graph
size_t res_ent_cap(int64_t rows, int cb, bool weighted, size_t lds_max) {
  const size_t fixed = 2ull * (size_t)rows * cb * 4 + res_rp_bytes(rows);
  return std::min((lds_max - fixed) / res_ent_bytes(weighted), (size_t)rows * kResEntPerRow) & ~(size_t)7;
}
// The library's column block: the widest of {f, 64, 32, 16, 8, 4} that fits; narrowed while the narrower block's workgroups
// still fit one round of the CUs; then narrowed on while the LDS left over stages fewer than kResEntGoal entries per row of
// the tallest graph (entries that are not staged are read from global memory on every hop: DESIGN 4.23).
int res_choose_cb(const gcnx_ctx* ctx, int64_t rows, int32_t f, int32_t b, bool weighted, size_t lds_max) {
  const int cand[6] = {f, 64, 32, 16, 8, 4};
  auto narrower = [&](int i) { int j = i + 1; while (j < 6 && cand[j] >= cand[i]) ++j; return j; };   // (f may sit below 64)
  int i = 0;
  while (i < 6 && (cand[i] > f || !res_fits(rows, cand[i]))) ++i;
  if (i == 6) return 0;
  for (int j = narrower(i); j < 6 && (int64_t)b * gcnx_cdiv(f, cand[j]) <= ctx->num_cus; j = narrower(i)) i = j;
  for (int j = narrower(i); j < 6 && res_ent_cap(rows, cand[i], weighted, lds_max) < (size_t)rows * kResEntGoal; j = narrower(i)) i = j;
  return cand[i];
}
// LDS of one workgroup: what decides whether a block FITS is 128 KiB everywhere (the *_resident_ok entry points answer without
// a device); entries are staged in whatever the device gives a workgroup beyond that (160 KiB on gfx950)
int res_lds_max(gcnx_ctx* ctx, size_t* out) {
  int v = 0;
  GCNX_HIP(ctx, hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
  *out = std::min(std::max((size_t)v, (size_t)kResLdsMax), (size_t)kResLdsDevMax);
  return GCNX_OK;
}
// threads of a resident workgroup: one per float4 of the tallest graph's slice, in whole waves, 256 .. 1024 (idle waves only
// wait at the barriers)
unsigned res_threads(int64_t max_graph_rows, int cb) {
  return (unsigned)std::min((int64_t)kResThreads, std::max((int64_t)256, (max_graph_rows * (cb / 4) + 63) / 64 * 64));
}

bool overlap(const float* a, int64_t a_floats, const float* b, int64_t b_floats) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a && b && a_floats > 0 && b_floats > 0 && a0 < b0 + (uint64_t)b_floats * 4 && b0 < a0 + (uint64_t)a_floats * 4;
}
int64_t span(int64_t n, int64_t ld, int32_t f) { return n > 0 ? (n - 1) * ld + f : 0; }

}  // namespace
