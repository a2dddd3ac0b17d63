// What the conv families' gather kernels (sage, gin, gine, gat, gatv2, resgated, transformer) literally share: the tile
// constants, the range-checked row load, float4 arithmetic, the lane-exchange steps, the row-tile prologue, the edge-feature
// register tiles and the host side's shape helpers.  Include behind common.h.  Everything is force-inlined or static and sits
// in the including file's anonymous namespace: nothing is exported and no type of this header appears in a kernel's signature,
// so moving a helper here leaves the device code of its users as it was.
//
// Only what is identical across families belongs here.  A formulation that a family chose for a measured reason -- the three
// head-group reductions, the per-family edge-feature expressions, sage's packed fma -- stays in its file, with the reason.
#pragma once
#include "common.h"

namespace {

constexpr int kTileRows = 32;         // rows per workgroup (the widest kernels of some families: 16, see conv_tile_rows)
constexpr int kTileCap = 1024;        // CSR entries of a tile staged in LDS (the rest is read from global memory)
constexpr int kTileU = 4;             // entries per row per trip
constexpr int kEdgeMax = 8;           // edge features served
constexpr unsigned kOffOut = 0xFFFFFFF0u;   // an offset no descriptor holds: the buffer load returns zeros without a fetch

#ifdef __HIPCC__
// one range-checked 16-byte load through a buffer descriptor
__device__ __forceinline__ gcnx_f32x4 buf4v(__amdgpu_buffer_rsrc_t rs, unsigned off) {
  return __builtin_bit_cast(gcnx_f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
}
__device__ __forceinline__ float4 buf4(__amdgpu_buffer_rsrc_t rs, unsigned off) {
  const gcnx_f32x4 r = buf4v(rs, off);
  return make_float4(r.x, r.y, r.z, r.w);
}

__device__ __forceinline__ float4 fma4(float v, float4 h, float4 a) {
  return make_float4(fmaf(v, h.x, a.x), fmaf(v, h.y, a.y), fmaf(v, h.z, a.z), fmaf(v, h.w, a.w));
}
__device__ __forceinline__ float4 fma44(float4 v, float4 h, float4 a) {
  return make_float4(fmaf(v.x, h.x, a.x), fmaf(v.y, h.y, a.y), fmaf(v.z, h.z, a.z), fmaf(v.w, h.w, a.w));
}
__device__ __forceinline__ float4 scale4(float v, float4 a) { return make_float4(v * a.x, v * a.y, v * a.z, v * a.w); }
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 sub4(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ float4 mul4(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
// (this association is in the bits of every score and gradient built on it: x first, then y, z, w)
__device__ __forceinline__ float dot4(float4 a, float4 b) { return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x))); }
__device__ __forceinline__ float4 load4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// sigmoid(a) for every finite a: exp(-a) = +inf gives 1 / inf = 0, exp(-a) = 0 gives 1
__device__ __forceinline__ float sigmoid1(float a) { return __builtin_amdgcn_rcpf(1.0f + __expf(-a)); }

// The value of lane ^ OFF (OFF = 16, 8, 4: a swizzle with a constant mask) and of a quad permutation (CTRL 0x4E: lanes
// [2, 3, 0, 1] of every quad, 0xB1: lanes [1, 0, 3, 2]) -- the steps of an xor butterfly over the lanes of a head: no per-lane
// address as a shuffle by a run-time offset needs.  How a family strings them together is its own (gatv2.hip, transformer.hip).
template <int OFF>
__device__ __forceinline__ float swz_xor(float v) {
  return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), (OFF << 10) | 0x1F));
}
template <int CTRL>
__device__ __forceinline__ float quad_perm(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}

// ---- what every tile kernel starts with: its rows, their entry range (s_rp: rows + 1 row pointers in LDS) ----------------
struct ConvTile {
  int r0, nr, e0, e1;
};
__device__ __forceinline__ ConvTile conv_tile(const int32_t* __restrict__ rowptr, int32_t n, int32_t* s_rp, int rows) {
  ConvTile t;
  t.r0 = gcnx_xcd_remap(blockIdx.x, gridDim.x) * rows;
  t.nr = min(n - t.r0, rows);
  if ((int)threadIdx.x <= t.nr) s_rp[threadIdx.x] = rowptr[t.r0 + threadIdx.x];
  t.e0 = rowptr[t.r0];
  t.e1 = rowptr[t.r0 + t.nr];
  return t;
}

// the row of stored entry e: the last r with rowptr[r] <= e (rows without entries are skipped over) -- for the kernels that
// run a thread per entry (explain.hip, pdn.hip)
__device__ __forceinline__ int row_of(const int32_t* __restrict__ rowptr, int n, int e) {
  int lo = 0, hi = n;                                       // rowptr[lo] <= e < rowptr[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (rowptr[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

// W_e [edge_dim, HC]: this lane's float4 of every row, rows >= edge_dim zero and never used
template <int E> struct EdgeW { float4 w[E > 0 ? E : 1]; };
template <int E>
__device__ __forceinline__ EdgeW<E> load_edge_w(const float* __restrict__ w_e, int edge_dim, int hc, int sub) {
  EdgeW<E> r;
  r.w[0] = zero4();
#pragma unroll
  for (int d = 0; d < E; ++d) r.w[d] = d < edge_dim ? load4(w_e + (int64_t)d * hc + 4 * sub) : zero4();
  return r;
}
// one entry's edge features (uniform over the lane group)
template <int E> struct EdgeF { float v[E > 0 ? E : 1]; };
#endif  // __HIPCC__

// ---- host side ------------------------------------------------------------------------------------------------------------
// a leading dimension of `width` float4-addressed columns whose row offsets in bytes stay far inside 32 bits
bool conv_ld_ok(int64_t ld, int width) { return ld >= width && ld % 4 == 0 && ld < (1ll << 30); }
// rows per workgroup of the kernels that keep W_e (and a gradient of its shape) in registers: 16 at width 128, where 32 rows
// are 1024 threads with 128 registers each and the tile did not fit (it spilled); 512 threads may hold 256
int conv_tile_rows(int width) { return width == 128 ? 16 : kTileRows; }

// LAUNCH(width, rows, E): the kernels are built for widths 16, 32, 64, 128 (rows as conv_tile_rows) and for 0, up to 2 and up
// to 8 edge features -- the register tiles of W_e hold that many float4 per lane, and registers decide how many workgroups a
// CU keeps in flight
#define GCNX_CONV_DISPATCH_E(ed, W_, R_, LAUNCH) \
  do { if ((ed) == 0) { LAUNCH(W_, R_, 0); } else if ((ed) <= 2) { LAUNCH(W_, R_, 2); } else { LAUNCH(W_, R_, 8); } } while (0)
#define GCNX_CONV_DISPATCH(w, ed, LAUNCH)                                                        \
  do {                                                                                           \
    if ((w) == 128) GCNX_CONV_DISPATCH_E(ed, 128, 16, LAUNCH); else if ((w) == 64) GCNX_CONV_DISPATCH_E(ed, 64, 32, LAUNCH); \
    else if ((w) == 32) GCNX_CONV_DISPATCH_E(ed, 32, 32, LAUNCH); else GCNX_CONV_DISPATCH_E(ed, 16, 32, LAUNCH);             \
  } while (0)

}  // namespace
