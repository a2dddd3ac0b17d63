// SAGEConv as ONE launch in the small-feature regime (F <= 128): the GraphSAGE layer the reference's torch model names as
// its next step ("consider using class SAGEConv instead", gcn_utills.py:804-806).
//
//     out = (A x) W_nb + x W_root + b  =  [A x | x] [W_nb ; W_root] + b          A: the row-mean operator, passed as values
//
// composed from existing calls this is gcnx_spmm_csr, two gcnx_gemm and a gcnx_add, with three [N, F] intermediates written
// and read back -- at N = 600 ... 20 000 each of them is a launch latency, not a throughput.  As one product over a doubled
// K a workgroup owns 32 rows end to end, like gcn_conv_fused_kernel (fused.hip, which keeps its own copies of the device helpers:
// that file is on the benchmark's path; what the conv families share is conv_tile.h):
//     gather + weight the neighbours' rows of x -> S tile [32, K] in LDS |  the tile's own rows of x -> X tile [32, K] in LDS
//     -> MFMA of S with W_nb, then of X with W_root into the same accumulators -> bias -> out
// The backward with respect to x is the same launch on the transposed operator with the weights read as stored:
//     dX = (A^T dZ) W_nb^T + dZ W_root^T          (w_transposed = 1: both weights [fo, fi] of THIS call)
// and S = A x, which the forward can store, is the operand of dW_nb = S^T dZ (dW_root = x^T dZ; both: gcnx_gemm_dw2).
//
// Shape of a workgroup: 512 threads, 32 rows.
//   gather   K / 4 lanes per row (float4 each), four row groups per wave (two at K = 128, which walk two rows each): all eight
//            waves hold rows at every K.  Four entries per row and trip, every load of a trip issued before the first is
//            consumed.  Range-checked buffer loads: slots past a row's end fetch nothing.  The tile's CSR entries are staged
//            in LDS first (1024 of them; a tile with more reads the rest from global memory, entry by entry).
//            One lane group accumulates a row in CSR order from +0: no atomics, the same bits on every call.
//   own rows plain coalesced 16-byte loads, issued before the staging barrier: in flight under the gather.
//   product  v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulate): wave w owns output columns [16w, 16w + 16) of
//            both 16-row halves.  Its slice of W_nb sits in registers in the B-operand layout (lane l holds k = 4 kk + (l >> 4),
//            column l & 15); every register is reloaded with the W_root element of the same (k, column) behind the MFMA that
//            consumed it, so both slices pass through the same K / 4 registers.  A operand: tile[row = l & 15][k], row stride
//            K + 4 floats (4 row + k spreads the 64 lanes over the 64 banks).
//   epilogue in registers: bias, stores of 4 rows x 64 bytes per instruction; no barrier behind the last MFMA.
// LDS: two tiles of 32 x (K + 4) floats + 8 KiB of entries -- 41.4 KiB at K = 128, three workgroups per CU.
#include "common.h"
#include "conv_tile.h"

namespace {

typedef float s32x2 __attribute__((ext_vector_type(2)));

struct SageArgs {
  const int32_t* rowptr; const int32_t* colidx; const float* vals;
  const float* x; int64_t ldx;           // [n, K]: gathered, and read row by row for the root term
  int32_t n;
  const float* w_nb; const float* w_root;  // w_t == 0: [K, nc];  w_t == 1: [nc, K]
  int32_t nc; int w_t;                   // output columns (multiple of 16, <= 128)
  const float* bias;
  float* s; int64_t lds;                 // S = A x (may be NULL)
  float* out; int64_t ldo;
};

// (not conv_tile.h's fma4: two packed fmas)
__device__ __forceinline__ float4 s4fma(float v, float4 h, float4 a) {
  const s32x2 w = {v, v};
  const s32x2 lo = __builtin_elementwise_fma(w, s32x2{h.x, h.y}, s32x2{a.x, a.y});
  const s32x2 hi = __builtin_elementwise_fma(w, s32x2{h.z, h.w}, s32x2{a.z, a.w});
  return make_float4(lo[0], lo[1], hi[0], hi[1]);
}

template <int K, bool WEIGHTED>
__global__ __launch_bounds__(512, 6) void sage_conv_kernel(SageArgs p) {
  constexpr int LPR = K / 4;                 // lanes per gathered row
  constexpr int GW = 64 / LPR < 4 ? 64 / LPR : 4;   // row groups per wave that hold rows (the lanes behind them idle in the gather)
  constexpr int NG = 8 * GW;                 // row groups per workgroup
  constexpr int RPG = kTileRows / NG;        // rows per group (2 at K = 128)
  constexpr int U = 4;                       // entries per row per trip
  constexpr int SL = 2 * U;                  // slack entries behind the staged ones
  constexpr int NQ = (kTileRows * LPR + 511) / 512;   // 16-byte pieces of the tile's own rows per thread (2 at K = 128)
  static_assert(K == 16 || K == 32 || K == 64 || K == 128, "gather width");
  static_assert(NG * RPG == kTileRows, "every row of the tile has a lane group");
  __shared__ __attribute__((aligned(16))) float tile_s[kTileRows][K + 4];   // row stride K + 4: see the A-operand read
  __shared__ __attribute__((aligned(16))) float tile_x[kTileRows][K + 4];
  // staged CSR entries: {byte offset of the gathered row = column * ldx * 4, weight}; the slack entries carry weight 0
  __shared__ __attribute__((aligned(8))) int2 s_ent[kTileCap + SL];
  __shared__ int32_t s_rp[kTileRows + 1];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ntiles = gridDim.x;
  const int t = gcnx_xcd_remap(blockIdx.x, ntiles);
  const int r0 = t * kTileRows, nr = min(p.n - r0, kTileRows);
  if (tid <= nr) s_rp[tid] = p.rowptr[r0 + tid];
  const int e0 = p.rowptr[r0], e1 = p.rowptr[r0 + nr];
  const int staged = min(e1 - e0, kTileCap);
  const unsigned ld4 = (unsigned)p.ldx * 4u;             // bytes per row of x
  for (int i = tid; i < staged + SL; i += 512) {
    int2 en = make_int2(0, 0);
    if (i < staged) {
      en.x = (int)((unsigned)p.colidx[e0 + i] * ld4);
      en.y = WEIGHTED ? __float_as_int(p.vals[e0 + i]) : 0x3f800000;
    }
    s_ent[i] = en;
  }
  // ---- the tile's own rows: in flight from here to the tile write ---------------------------------------------------
  float4 own[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int i = tid + 512 * q, row = i / LPR, c4 = i - row * LPR;
    own[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < nr) own[q] = *reinterpret_cast<const float4*>(p.x + (int64_t)(r0 + row) * p.ldx + 4 * c4);
  }
  // ---- gather --------------------------------------------------------------------------------------------------------
  const int grp = lane / LPR, sub = lane % LPR;
  const bool has_rows = grp < GW;
  const int gid = wave * GW + (has_rows ? grp : 0);
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
  // out-of-range offset (the buffer load returns zeros without a fetch); their weight is whatever the next row's entry
  // holds -- finite -- times zero.
  for (int tt = 0; __builtin_amdgcn_ballot_w64(tt < len) != 0; tt += U) {
    float4 hv[RPG][U];
    float wv[RPG][U];
#pragma unroll
    for (int j = 0; j < RPG; ++j) {
      const int eb_ = min(ea[j] + tt, ebf[j]);         // a row that is done stays at its end: the reads stay inside the slack
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int e = eb_ + u;
        const int2 en = s_ent[e];
        wv[j][u] = __int_as_float(en.y);
        hv[j][u] = buf4(xr, e < ebf[j] ? (unsigned)en.x + sub16 : kOffOut);
      }
    }
    __builtin_amdgcn_sched_barrier(0);                 // all loads of the trip go out before the first is consumed
#pragma unroll
    for (int j = 0; j < RPG; ++j)
#pragma unroll
      for (int u = 0; u < U; ++u) acc[j] = s4fma(wv[j][u], hv[j][u], acc[j]);
  }
  if (e1 - e0 > kTileCap) {       // uniform per workgroup, rare: entries beyond the staged ones, one at a time from global memory
#pragma unroll
    for (int j = 0; j < RPG; ++j)
      for (int e = max(eb[j] > 0 ? s_rp[gid + j * NG] - e0 : 0, kTileCap); e < eb[j]; ++e) {   // (ea is clamped: the row's true start)
        const float v = WEIGHTED ? p.vals[e0 + e] : 1.0f;
        acc[j] = s4fma(v, buf4(xr, (unsigned)p.colidx[e0 + e] * ld4 + sub16), acc[j]);
      }
  }
  // ---- this wave's slice of W_nb, in the MFMA B layout; in flight while the tiles are written ------------------------
  const int c16 = lane & 15, kq = lane >> 4;
  const bool wave_on = 16 * wave < p.nc;
  const int col = 16 * wave + c16;
  // element (k, col) of either weight: [K, nc] rows are 64-byte pieces per k; [nc, K] (w_t) is read strided, as stored
  const int64_t wstep = p.w_t ? 4 : 4 * (int64_t)p.nc;                                    // k -> k + 4
  const int64_t woff = p.w_t ? (int64_t)col * K + kq : (int64_t)kq * p.nc + col;           // k = kq
  float wreg[K / 4];
  if (wave_on) {
#pragma unroll
    for (int e = 0; e < K / 4; ++e) wreg[e] = p.w_nb[woff + e * wstep];
  }
  if (has_rows) {
#pragma unroll
    for (int j = 0; j < RPG; ++j) {
      const int r = gid + j * NG;
      if (p.s && r < nr) *reinterpret_cast<float4*>(p.s + (int64_t)(r0 + r) * p.lds + sub * 4) = acc[j];
      *reinterpret_cast<float4*>(&tile_s[r][sub * 4]) = acc[j];      // rows past the end hold zeros
    }
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int i = tid + 512 * q, row = i / LPR, c4 = i - row * LPR;
    if (row < kTileRows) *reinterpret_cast<float4*>(&tile_x[row][4 * c4]) = own[q];
  }
  __syncthreads();
  // ---- product and epilogue, in registers: wave w owns output columns [16w, 16w + 16) of all 32 rows ------------------
  // C layout of the 16 x 16 tile: column = lane & 15, rows 4 (lane >> 4) + reg.
  if (!wave_on) return;
  const float bcol = p.bias ? p.bias[col] : 0.f;
  gcnx_f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = c0;
#pragma unroll
  for (int kk = 0; kk < K / 4; ++kk) {
    const float a0 = tile_s[c16][4 * kk + kq];
    const float a1 = tile_s[16 + c16][4 * kk + kq];
    c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, wreg[kk], c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, wreg[kk], c1, 0, 0, 0);
    wreg[kk] = p.w_root[woff + kk * wstep];            // the same register, behind the MFMAs that read it
  }
#pragma unroll
  for (int kk = 0; kk < K / 4; ++kk) {
    const float a0 = tile_x[c16][4 * kk + kq];
    const float a1 = tile_x[16 + c16][4 * kk + kq];
    c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, wreg[kk], c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, wreg[kk], c1, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int row = 16 * (r >> 2) + 4 * kq + (r & 3);
    const float v = (r < 4 ? c0[r & 3] : c1[r & 3]) + bcol;
    if (row < nr) p.out[(int64_t)(r0 + row) * p.ldo + col] = v;
  }
}

bool sage_shape_ok(int64_t n, int32_t k, int32_t nc, int64_t ldx) {
  return n >= 0 && n <= 0x7FFFFFFFll && (k == 16 || k == 32 || k == 64 || k == 128) && nc >= 16 && nc <= 128 && nc % 16 == 0 &&
         ldx >= k && ldx % 4 == 0 && (uint64_t)n * (uint64_t)ldx * 4u < 0xFFFFFFF0ull;
}

int launch_sage(gcnx_ctx* ctx, const SageArgs& a, int k) {
  const int tiles = gcnx_cdiv(a.n, kTileRows);
#define GCNX_SAGE_LAUNCH(K_)                                                                                       \
  do {                                                                                                             \
    if (a.vals) hipLaunchKernelGGL((sage_conv_kernel<K_, true>), dim3(tiles), dim3(512), 0, ctx->stream, a);        \
    else hipLaunchKernelGGL((sage_conv_kernel<K_, false>), dim3(tiles), dim3(512), 0, ctx->stream, a);              \
  } while (0)
  if (k == 128) GCNX_SAGE_LAUNCH(128);
  else if (k == 64) GCNX_SAGE_LAUNCH(64);
  else if (k == 32) GCNX_SAGE_LAUNCH(32);
  else GCNX_SAGE_LAUNCH(16);
#undef GCNX_SAGE_LAUNCH
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

}  // namespace

extern "C" {

int gcnx_sage_conv_ok(int64_t n, int32_t fi, int32_t fo, int64_t ldx) { return sage_shape_ok(n, fi, fo, ldx) ? 1 : 0; }

int gcnx_sage_conv(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* vals, const float* x, int64_t ldx,
                   int32_t n, int32_t fi, const float* w_nb, const float* w_root, int32_t fo, int w_transposed, const float* bias,
                   float* s, int64_t lds, float* out, int64_t ldo) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "SAGEConv (one launch)");
  GCNX_REQUIRE(ctx, n >= 0 && fi >= 0 && fo >= 0, "gcnx_sage_conv: negative size");
  if (!sage_shape_ok(n, fi, fo, ldx))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_sage_conv: needs fi in {16, 32, 64, 128}, fo a multiple of 16 up to 128, ldx >= fi in "
                     "multiples of 4 floats and n * ldx * 4 < 2^32 (got n=%d fi=%d fo=%d ldx=%lld): use gcnx_spmm_csr + gcnx_gemm + gcnx_add",
                     n, fi, fo, (long long)ldx);
  if (!gcnx_aligned16(x) || !gcnx_aligned16(w_nb) || !gcnx_aligned16(w_root) || !gcnx_aligned16(out) || ldo < fo || ldo % 4 != 0 ||
      (s && (!gcnx_aligned16(s) || lds < fi || lds % 4 != 0)))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_sage_conv: x, w_nb, w_root, s and out must be 16-byte aligned, with lds >= fi and "
                     "ldo >= fo in multiples of 4 floats");
  if (n == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, rowptr && colidx && x && w_nb && w_root && out, "gcnx_sage_conv: NULL pointer");
  GCNX_REQUIRE(ctx, x != out && x != s && (!s || s != out), "gcnx_sage_conv: the outputs must not alias x or each other");
  SageArgs a{};
  a.rowptr = rowptr; a.colidx = colidx; a.vals = vals; a.x = x; a.ldx = ldx; a.n = n; a.w_nb = w_nb; a.w_root = w_root;
  a.nc = fo; a.w_t = w_transposed ? 1 : 0; a.bias = bias; a.s = s; a.lds = lds; a.out = out; a.ldo = ldo;
  return launch_sage(ctx, a, fi);
}

}  // extern "C"
