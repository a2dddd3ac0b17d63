// GINConv as ONE launch in the small-feature regime (widths <= 128): the Graph Isomorphism Network convolution for the slot the
// reference's author left open ("consider using class SAGEConv instead", gcn_utills.py:804-806).
//
//     T = (1 + eps) x + A x        A: the stored pattern as all ones (values are not an operand)
//     U = relu(T W_a + b_a)        [n, k1]
//     out = U W_b + b_b            [n, k2]
//
// composed from existing calls this is a neighbour sum, a scaled add, and two gcnx_gemm, with two [N, F] intermediates written
// and read back -- at N = 600 ... 20 000 each of them is a launch latency, not a throughput.  Here a workgroup owns 32 rows
// from the gather to the second bias, like sage_conv_kernel (sage.hip; the device helpers they share: conv_tile.h):
//     gather the neighbours' rows of x, add (1 + eps) times the row's own -> T tile [32, K0] in LDS
//     -> MFMA of T with W_a -> bias, ReLU in registers -> U tile [32, k1] in LDS, in the A-operand layout
//     -> MFMA of U with W_b -> bias -> out
// Single stage (w_b == NULL): out = T W_a (+ b_a), no ReLU, no second tile.  The backward with respect to x is that form on
// the transposed pattern with the weight read as stored:  dX = ((1 + eps) dU + A^T dU) W_a^T   (w_transposed = 1: [k1, k0]).
// T and U, which the forward can store, are the operands of dW_a = T^T dU and dW_b = U^T dZ; U is also the ReLU mask.
//
// Shape of a workgroup: 512 threads, 32 rows.
//   gather   K0 / 4 lanes per row (float4 each), four row groups per wave (two at K0 = 128, which walk two rows each).  Four
//            entries per row and trip, every load of a trip issued before the first is consumed.  Range-checked buffer loads:
//            slots past a row's end fetch nothing and add +0.  The tile's CSR entries are staged in LDS first (1024 of them; a
//            tile with more reads the rest from global memory, entry by entry).  One lane group accumulates a row in CSR order
//            from +0, then T = fma(1 + eps, own row, sum): no atomics, the same bits on every call, and the bits of
//            gin_aggregate_kernel's float4 form.  The row's own piece is loaded before the staging barrier.
//   products v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulate): wave w owns columns [16w, 16w + 16) of both 16-row
//            halves, of U in the first stage and of out in the second (a wave past the width of a stage skips it).  Its slice
//            of the weight sits in registers in the B-operand layout (lane l holds k = 4 kk + (l >> 4), column l & 15).
//            A operand: tile[row = l & 15][k = 4 kk + (l >> 4)], row stride width + 4 floats: the word address is
//            (width + 4) row + k, and with width a multiple of 16, (width + 4) row = 4 (odd) row mod 64 walks the 16 rows over
//            16 distinct multiples of 4 -- the 64 lanes of a read fall on the 64 banks.
//   between  the first stage's accumulators are in the C layout (column = lane & 15, rows 4 (lane >> 4) + reg): bias, ReLU, and
//            each register goes to U tile[row][16w + column] -- four rows x 16 consecutive words per store, 16 banks apart.  One
//            barrier, then the second stage reads the tile as the first read T's.
//   epilogue in registers: bias, stores of 4 rows x 64 bytes per instruction.  Rows of the last tile at or past n are
//            computed (on zeros) and never stored.
// LDS: T tile 32 x (K0 + 4) floats, U tile 32 x 132 floats, 4 KiB of entries -- 37.2 KiB at K0 = 128, four workgroups per CU by
// LDS (the registers allow three).
//
// gin_aggregate_kernel is T alone for any width; gin_eps_* is the gradient with respect to eps, sum_i <x_i, dT_i>.
#include "common.h"
#include "conv_tile.h"

namespace {

constexpr int kGMaxW = 128;       // widest stage

struct GinArgs {
  const int32_t* rowptr; const int32_t* colidx;
  const float* x; int64_t ldx;           // [n, K0]: gathered, and read row by row for the (1 + eps) term
  int32_t n;
  const float* eps;                      // device scalar, or NULL = 0
  const float* w_a; const float* b_a;    // w_t == 0: [K0, k1];  w_t == 1: [k1, K0]
  int32_t k1;
  const float* w_b; const float* b_b;    // w_t == 0: [k1, k2];  w_t == 1: [k2, k1];  w_b == NULL: single stage
  int32_t k2; int w_t;
  float* t; int64_t ldt;                 // T (may be NULL)
  float* u; int64_t ldu;                 // U (may be NULL)
  float* out; int64_t ldo;
};

template <int K>
__global__ __launch_bounds__(512) void gin_conv_kernel(GinArgs p) {
  constexpr int LPR = K / 4;                 // lanes per gathered row
  constexpr int GW = 64 / LPR < 4 ? 64 / LPR : 4;   // row groups per wave that hold rows (the lanes behind them idle in the gather)
  constexpr int NG = 8 * GW;                 // row groups per workgroup
  constexpr int RPG = kTileRows / NG;        // rows per group (2 at K = 128)
  constexpr int U = 4;                       // entries per row per trip
  constexpr int SL = 2 * U;                  // slack entries behind the staged ones
  static_assert(K == 16 || K == 32 || K == 64 || K == 128, "gather width");
  static_assert(NG * RPG == kTileRows, "every row of the tile has a lane group");
  __shared__ __attribute__((aligned(16))) float tile_t[kTileRows][K + 4];        // row stride K + 4: see the A-operand read
  __shared__ __attribute__((aligned(16))) float tile_u[kTileRows * (kGMaxW + 4)];   // row stride k1 + 4
  __shared__ int32_t s_ent[kTileCap + SL];   // staged CSR entries: byte offset of the gathered row = column * ldx * 4
  __shared__ int32_t s_rp[kTileRows + 1];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ntiles = gridDim.x;
  const int tl = gcnx_xcd_remap(blockIdx.x, ntiles);
  const int r0 = tl * kTileRows, nr = min(p.n - r0, kTileRows);
  if (tid <= nr) s_rp[tid] = p.rowptr[r0 + tid];
  const int e0 = p.rowptr[r0], e1 = p.rowptr[r0 + nr];
  const int staged = min(e1 - e0, kTileCap);
  const unsigned ld4 = (unsigned)p.ldx * 4u;             // bytes per row of x
  for (int i = tid; i < staged + SL; i += 512) s_ent[i] = i < staged ? (int)((unsigned)p.colidx[e0 + i] * ld4) : 0;
  // ---- the rows' own pieces: in flight from here to the end of the gather -----------------------------------------------
  const int grp = lane / LPR, sub = lane % LPR;
  const bool has_rows = grp < GW;
  const int gid = wave * GW + (has_rows ? grp : 0);
  float4 own[RPG];
#pragma unroll
  for (int j = 0; j < RPG; ++j) {
    const int r = gid + j * NG;
    own[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (has_rows && r < nr) own[j] = *reinterpret_cast<const float4*>(p.x + (int64_t)(r0 + r) * p.ldx + 4 * sub);
  }
  const float scale = 1.0f + (p.eps ? p.eps[0] : 0.f);
  // ---- gather --------------------------------------------------------------------------------------------------------
  // the descriptor ends behind the last row's K columns (a column slice of a wider array: nothing past them is addressed)
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.x, (short)0, (int)((unsigned)(p.n - 1) * ld4 + (unsigned)K * 4u), 0x00020000);
  __syncthreads();
  float4 acc[RPG];
  int ea[RPG], eb[RPG], ebf[RPG];
  int len = 0;
#pragma unroll
  for (int j = 0; j < RPG; ++j) {
    const int r = gid + j * NG;
    acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool live = has_rows && r < nr;
    ea[j] = live ? s_rp[r] - e0 : 0;
    eb[j] = live ? s_rp[r + 1] - e0 : 0;
    ebf[j] = min(eb[j], kTileCap);                   // the staged part of the row ...
    ea[j] = min(ea[j], kTileCap);                    // ... (empty if the row starts past it)
    len = max(len, ebf[j] - ea[j]);
  }
  const unsigned sub16 = (unsigned)sub * 16u;
  // Branch-free: a load inside a branch makes hipcc close the trip with s_waitcnt vmcnt(0).  Slots past the row's end get an
  // out-of-range offset: the buffer load returns zeros without a fetch, and the sum takes +0.
  for (int tt = 0; __builtin_amdgcn_ballot_w64(tt < len) != 0; tt += U) {
    float4 hv[RPG][U];
#pragma unroll
    for (int j = 0; j < RPG; ++j) {
      const int eb_ = min(ea[j] + tt, ebf[j]);         // a row that is done stays at its end: the reads stay inside the slack
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int e = eb_ + u;
        hv[j][u] = buf4(xr, e < ebf[j] ? (unsigned)s_ent[e] + sub16 : kOffOut);
      }
    }
    __builtin_amdgcn_sched_barrier(0);                 // all loads of the trip go out before the first is consumed
#pragma unroll
    for (int j = 0; j < RPG; ++j)
#pragma unroll
      for (int u = 0; u < U; ++u) acc[j] = add4(acc[j], hv[j][u]);
  }
  if (e1 - e0 > kTileCap) {       // uniform per workgroup, rare: entries beyond the staged ones, one at a time from global memory
#pragma unroll
    for (int j = 0; j < RPG; ++j)
      for (int e = max(eb[j] > 0 ? s_rp[gid + j * NG] - e0 : 0, kTileCap); e < eb[j]; ++e)   // (ea is clamped: the row's true start)
        acc[j] = add4(acc[j], buf4(xr, (unsigned)p.colidx[e0 + e] * ld4 + sub16));
  }
  // ---- this wave's slice of W_a, in the MFMA B layout; in flight while the tile is written -----------------------------
  const int c16 = lane & 15, kq = lane >> 4;
  const bool two = p.w_b != nullptr;
  const bool on1 = 16 * wave < p.k1;
  const int col = 16 * wave + c16;
  // element (k, col) of a weight: [K, nc] rows are 64-byte pieces per k; [nc, K] (w_t) is read strided, as stored
  const int64_t wstep = p.w_t ? 4 : 4 * (int64_t)p.k1;                                    // k -> k + 4
  const int64_t woff = p.w_t ? (int64_t)col * K + kq : (int64_t)kq * p.k1 + col;           // k = kq
  float wreg[K / 4];
  if (on1) {
#pragma unroll
    for (int e = 0; e < K / 4; ++e) wreg[e] = p.w_a[woff + e * wstep];
  }
  if (has_rows) {
#pragma unroll
    for (int j = 0; j < RPG; ++j) {
      const int r = gid + j * NG;
      const float4 tv = fma4(scale, own[j], acc[j]);
      if (p.t && r < nr) *reinterpret_cast<float4*>(p.t + (int64_t)(r0 + r) * p.ldt + sub * 4) = tv;
      *reinterpret_cast<float4*>(&tile_t[r][sub * 4]) = tv;          // rows past the end hold zeros
    }
  }
  __syncthreads();
  // ---- first product: wave w owns columns [16w, 16w + 16) of all 32 rows ------------------------------------------------
  // C layout of the 16 x 16 tile: column = lane & 15, rows 4 (lane >> 4) + reg.
  const int su = p.k1 + 4;                             // row stride of the U tile
  if (on1) {
    const float bcol = p.b_a ? p.b_a[col] : 0.f;
    gcnx_f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = c0;
#pragma unroll
    for (int kk = 0; kk < K / 4; ++kk) {
      const float a0 = tile_t[c16][4 * kk + kq];
      const float a1 = tile_t[16 + c16][4 * kk + kq];
      c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, wreg[kk], c0, 0, 0, 0);
      c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, wreg[kk], c1, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int row = 16 * (r >> 2) + 4 * kq + (r & 3);
      float v = (r < 4 ? c0[r & 3] : c1[r & 3]) + bcol;
      if (!two) {
        if (row < nr) p.out[(int64_t)(r0 + row) * p.ldo + col] = v;
      } else {
        v = v > 0.f ? v : 0.f;
        tile_u[row * su + col] = v;
        if (p.u && row < nr) p.u[(int64_t)(r0 + row) * p.ldu + col] = v;
      }
    }
  }
  if (!two) return;                                    // (a kernel argument: the whole grid leaves here)
  // ---- second product: this wave's slice of W_b, loaded while the other waves finish the U tile --------------------------
  const bool on2 = 16 * wave < p.k2;
  const int64_t wstep2 = p.w_t ? 4 : 4 * (int64_t)p.k2;
  const int64_t woff2 = p.w_t ? (int64_t)col * p.k1 + kq : (int64_t)kq * p.k2 + col;
  float w2[kGMaxW / 4];
#pragma unroll
  for (int g = 0; g < kGMaxW / 16; ++g) {
#pragma unroll
    for (int i = 0; i < 4; ++i) w2[4 * g + i] = 0.f;
    if (on2 && 16 * g < p.k1) {                        // k1 is a multiple of 16: four k steps at a time
#pragma unroll
      for (int i = 0; i < 4; ++i) w2[4 * g + i] = p.w_b[woff2 + (4 * g + i) * wstep2];
    }
  }
  __syncthreads();
  if (!on2) return;
  const float bcol2 = p.b_b ? p.b_b[col] : 0.f;
  gcnx_f32x4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = d0;
#pragma unroll
  for (int g = 0; g < kGMaxW / 16; ++g) {
    if (16 * g < p.k1) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int kk = 4 * g + i;
        const float a0 = tile_u[c16 * su + 4 * kk + kq];
        const float a1 = tile_u[(16 + c16) * su + 4 * kk + kq];
        d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, w2[kk], d0, 0, 0, 0);
        d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, w2[kk], d1, 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int row = 16 * (r >> 2) + 4 * kq + (r & 3);
    const float v = (r < 4 ? d0[r & 3] : d1[r & 3]) + bcol2;
    if (row < nr) p.out[(int64_t)(r0 + row) * p.ldo + col] = v;
  }
}

bool gin_width_ok(int32_t k) { return k >= 16 && k <= kGMaxW && k % 16 == 0; }

bool gin_shape_ok(int64_t n, int32_t k0, int32_t k1, int32_t k2, int64_t ldx) {
  return n >= 0 && n <= 0x7FFFFFFFll && (k0 == 16 || k0 == 32 || k0 == 64 || k0 == 128) && gin_width_ok(k1) &&
         (k2 == 0 || gin_width_ok(k2)) && ldx >= k0 && ldx % 4 == 0 && (uint64_t)n * (uint64_t)ldx * 4u < 0xFFFFFFF0ull;
}

int launch_gin(gcnx_ctx* ctx, const GinArgs& a, int k0) {
  const int tiles = gcnx_cdiv(a.n, kTileRows);
  if (k0 == 128) hipLaunchKernelGGL((gin_conv_kernel<128>), dim3(tiles), dim3(512), 0, ctx->stream, a);
  else if (k0 == 64) hipLaunchKernelGGL((gin_conv_kernel<64>), dim3(tiles), dim3(512), 0, ctx->stream, a);
  else if (k0 == 32) hipLaunchKernelGGL((gin_conv_kernel<32>), dim3(tiles), dim3(512), 0, ctx->stream, a);
  else hipLaunchKernelGGL((gin_conv_kernel<16>), dim3(tiles), dim3(512), 0, ctx->stream, a);
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

// ---- T alone, any width: one group of (1 << lpr_log2) lanes per row, blockIdx.y = column block of LPR * VEC columns ------
template <int VEC> struct GinVec;
template <> struct GinVec<4> {
  float4 v;
  __device__ __forceinline__ void zero() { v = make_float4(0.f, 0.f, 0.f, 0.f); }
  __device__ __forceinline__ void load(const float* p) { v = *reinterpret_cast<const float4*>(p); }
  __device__ __forceinline__ void store(float* p) const { *reinterpret_cast<float4*>(p) = v; }
  __device__ __forceinline__ void add(const GinVec& o) { v = add4(v, o.v); }
  __device__ __forceinline__ void scale_add(float s, const GinVec& o) { v = fma4(s, o.v, v); }
};
template <> struct GinVec<1> {
  float v;
  __device__ __forceinline__ void zero() { v = 0.f; }
  __device__ __forceinline__ void load(const float* p) { v = *p; }
  __device__ __forceinline__ void store(float* p) const { *p = v; }
  __device__ __forceinline__ void add(const GinVec& o) { v += o.v; }
  __device__ __forceinline__ void scale_add(float s, const GinVec& o) { v = fmaf(s, o.v, v); }
};

template <int VEC>
__global__ __launch_bounds__(256) void gin_aggregate_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                                            const float* __restrict__ x, int64_t ldx, const float* __restrict__ eps,
                                                            float* __restrict__ out, int64_t ldo, int32_t n, int32_t f, int lpr_log2) {
  const int lpr = 1 << lpr_log2, rpb = 256 >> lpr_log2;
  const int g = threadIdx.x >> lpr_log2, sub = threadIdx.x & (lpr - 1);
  const int64_t r = (int64_t)blockIdx.x * rpb + g;
  const int col = (blockIdx.y * lpr + sub) * VEC;
  if (r >= n || col >= f) return;
  const float scale = 1.0f + (eps ? eps[0] : 0.f);
  const int b = rowptr[r], e = rowptr[r + 1];
  GinVec<VEC> own, acc;
  own.load(x + r * ldx + col);
  acc.zero();
  int i = b;
  for (; i + 4 <= e; i += 4) {                // stored order: the sum of a row is the same bits in every run
    GinVec<VEC> h[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) h[q].load(x + (int64_t)colidx[i + q] * ldx + col);
#pragma unroll
    for (int q = 0; q < 4; ++q) acc.add(h[q]);
  }
  for (; i < e; ++i) {
    GinVec<VEC> h;
    h.load(x + (int64_t)colidx[i] * ldx + col);
    acc.add(h);
  }
  acc.scale_add(scale, own);
  acc.store(out + r * ldo + col);
}

// ---- d eps = sum_i <x_i, dT_i>: per-workgroup partials over kEpsRows rows each, then one workgroup over the partials --------
constexpr int kEpsRows = 64;

__device__ __forceinline__ float gin_tree256(float v, float* s) {   // fixed tree over the 256 threads; the sum in s[0]
  s[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
    __syncthreads();
  }
  return s[0];
}

// A group of (1 << lpr_log2) lanes walks a row, column on the lane (consecutive lanes read consecutive floats); the 256 >> lpr_log2
// groups take the workgroup's rows in turn.  Every thread adds its products in the same order on every call.
__global__ __launch_bounds__(256) void gin_eps_part_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ dt,
                                                           int64_t lddt, int64_t n, int32_t f, float* __restrict__ parts, int lpr_log2) {
  __shared__ float s[256];
  const int64_t r0 = (int64_t)blockIdx.x * kEpsRows;
  const int nr = (int)(n - r0 < kEpsRows ? n - r0 : kEpsRows);
  const int lpr = 1 << lpr_log2, rpb = 256 >> lpr_log2;
  const int g = threadIdx.x >> lpr_log2, sub = threadIdx.x & (lpr - 1);
  float acc = 0.f;
  for (int row = g; row < nr; row += rpb) {
    const float* xr = x + (r0 + row) * ldx;
    const float* dr = dt + (r0 + row) * lddt;
    for (int c = sub; c < f; c += lpr) acc = fmaf(xr[c], dr[c], acc);
  }
  const float tot = gin_tree256(acc, s);
  if (threadIdx.x == 0) parts[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void gin_eps_final_kernel(const float* __restrict__ parts, int64_t nparts, float* __restrict__ deps) {
  __shared__ float s[256];
  float acc = 0.f;
  for (int64_t i = threadIdx.x; i < nparts; i += 256) acc += parts[i];
  const float tot = gin_tree256(acc, s);
  if (threadIdx.x == 0) deps[0] = tot;
}

}  // namespace

extern "C" {

int gcnx_gin_conv_ok(int64_t n, int32_t k0, int32_t k1, int32_t k2, int64_t ldx) { return gin_shape_ok(n, k0, k1, k2, ldx) ? 1 : 0; }

int gcnx_gin_conv(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* x, int64_t ldx, int32_t n, int32_t k0,
                  const float* eps, const float* w_a, const float* b_a, int32_t k1, const float* w_b, const float* b_b, int32_t k2,
                  int w_transposed, float* t, int64_t ldt, float* u, int64_t ldu, float* out, int64_t ldo) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "GINConv (one launch)");
  GCNX_REQUIRE(ctx, n >= 0 && k0 >= 0 && k1 >= 0 && k2 >= 0, "gcnx_gin_conv: negative size");
  GCNX_REQUIRE(ctx, (w_b != nullptr) == (k2 != 0), "gcnx_gin_conv: w_b and k2 go together (both given: two stages; NULL and 0: one)");
  GCNX_REQUIRE(ctx, w_b || (!u && !b_b), "gcnx_gin_conv: u and b_b belong to the second stage and must be NULL without it");
  if (!gin_shape_ok(n, k0, k1, k2, ldx))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_gin_conv: needs k0 in {16, 32, 64, 128}, k1 and k2 multiples of 16 up to 128 (k2 = 0: "
                     "single stage), ldx >= k0 in multiples of 4 floats and n * ldx * 4 < 2^32 (got n=%d k0=%d k1=%d k2=%d ldx=%lld): use "
                     "gcnx_gin_aggregate + gcnx_gemm", n, k0, k1, k2, (long long)ldx);
  const int32_t ko = w_b ? k2 : k1;                    // width of out
  if (!gcnx_aligned16(x) || !gcnx_aligned16(w_a) || !gcnx_aligned16(w_b) || !gcnx_aligned16(out) || ldo < ko || ldo % 4 != 0 ||
      (t && (!gcnx_aligned16(t) || ldt < k0 || ldt % 4 != 0)) || (u && (!gcnx_aligned16(u) || ldu < k1 || ldu % 4 != 0)))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_gin_conv: x, w_a, w_b, t, u and out must be 16-byte aligned, with ldt >= k0, "
                     "ldu >= k1 and ldo >= the width of out in multiples of 4 floats");
  if (n == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, rowptr && colidx && x && w_a && out, "gcnx_gin_conv: NULL pointer");
  GCNX_REQUIRE(ctx, x != out && x != t && x != u && (!t || (t != out && t != u)) && (!u || u != out),
               "gcnx_gin_conv: the outputs must not alias x or each other");
  GinArgs a{};
  a.rowptr = rowptr; a.colidx = colidx; a.x = x; a.ldx = ldx; a.n = n; a.eps = eps; a.w_a = w_a; a.b_a = b_a; a.k1 = k1;
  a.w_b = w_b; a.b_b = b_b; a.k2 = k2; a.w_t = w_transposed ? 1 : 0; a.t = t; a.ldt = ldt; a.u = u; a.ldu = ldu; a.out = out; a.ldo = ldo;
  return launch_gin(ctx, a, k0);
}

int gcnx_gin_aggregate(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* x, int64_t ldx, const float* eps,
                       float* out, int64_t ldo, int32_t n, int32_t f) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "GINConv aggregate");
  GCNX_REQUIRE(ctx, n >= 0 && f >= 1 && ldx >= f && ldo >= f, "gcnx_gin_aggregate: needs n >= 0, f >= 1, ldx >= f and ldo >= f");
  if (n == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, rowptr && colidx && x && out, "gcnx_gin_aggregate: NULL pointer");
  GCNX_REQUIRE(ctx, x != out, "gcnx_gin_aggregate: out must not alias x");
  const bool vec = f % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && gcnx_aligned16(x) && gcnx_aligned16(out);
  const int units = vec ? f / 4 : f;                   // lanes a row needs
  int lpr_log2 = 0;
  while ((1 << lpr_log2) < units && lpr_log2 < 6) ++lpr_log2;
  const int rpb = 256 >> lpr_log2;
  const int ny = gcnx_cdiv(units, 1 << lpr_log2);
  GCNX_REQUIRE(ctx, ny <= 65535, "gcnx_gin_aggregate: f=%d is too wide", f);
  const dim3 grid(gcnx_cdiv(n, rpb), ny);
  if (vec) hipLaunchKernelGGL((gin_aggregate_kernel<4>), grid, dim3(256), 0, ctx->stream, rowptr, colidx, x, ldx, eps, out, ldo, n, f, lpr_log2);
  else hipLaunchKernelGGL((gin_aggregate_kernel<1>), grid, dim3(256), 0, ctx->stream, rowptr, colidx, x, ldx, eps, out, ldo, n, f, lpr_log2);
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

int gcnx_gin_eps_grad(gcnx_ctx* ctx, const float* x, int64_t ldx, const float* dt, int64_t lddt, int64_t n, int32_t f, float* parts,
                      float* deps) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "GINConv d eps");
  GCNX_REQUIRE(ctx, n >= 0 && n <= 0x7FFFFFFFll && f >= 1 && ldx >= f && lddt >= f,
               "gcnx_gin_eps_grad: needs 0 <= n < 2^31, f >= 1, ldx >= f and lddt >= f");
  GCNX_REQUIRE(ctx, deps && (n == 0 || (x && dt && parts)), "gcnx_gin_eps_grad: NULL pointer");
  const int64_t nparts = (n + kEpsRows - 1) / kEpsRows;
  if (nparts > 0) {
    int lpr_log2 = 0;                                  // lanes per row: the power of two that covers f, 256 at the most
    while ((1 << lpr_log2) < f && lpr_log2 < 8) ++lpr_log2;
    hipLaunchKernelGGL(gin_eps_part_kernel, dim3((unsigned)nparts), dim3(256), 0, ctx->stream, x, ldx, dt, lddt, n, f, parts, lpr_log2);
    GCNX_LAUNCH_OK(ctx);
  }
  hipLaunchKernelGGL(gin_eps_final_kernel, dim3(1), dim3(256), 0, ctx->stream, (const float*)parts, nparts, deps);
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

}  // extern "C"
