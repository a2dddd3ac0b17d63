// RGCNConv (Schlichtkrull et al. 2018; PyG's RGCNConv(aggr="mean", root_weight, bias) without a decomposition): every stored
// entry carries one of R <= 4 relations -- in the reference's graphs an intra-chain contact or an inter-chain DCA bridge
// (gcn_utills.py:319-443) -- and each relation has its own weight matrix,
//
//     out_i = x_i W_root + b + sum_{r < R} mean_{k in N_r(i)} x_col(k) W_r
//           = [A_0 x | .. | A_{R-1} x | x] [W_0 ; .. ; W_{R-1} ; W_root] + b       A_r: the row-mean operator of relation r
//
// gcnx_rgcn_operator   rel[k] (one byte) and val[k] = 1 / |N_rel(k)(row(k))| from the edge features, one thread per row, and
//                      their copies in the order of the transposed pattern (a second, entry-parallel launch through perm_t).
// gcnx_rgcn_conv       ONE launch: sage.hip's workgroup (512 threads own 32 rows end to end) with R neighbour tiles.  A row's
//                      entries are gathered once; each is steered into its relation's accumulator.
// gcnx_rgcn_aggregate  the panel M = [A_0 x | .. | A_{R-1} x] alone, for any width, stride and alignment (the composed route:
//                      this, then gcnx_gemm over M and over x).
// Every accumulator of both kernels evaluates acc_r = fma(val_k, x_j, acc_r) over the row's entries of relation r in CSR order
// from +0, an entry of another relation leaving it untouched (a select, not a product with 0): M has the same bits on both
// routes and on every call.  No atomics.
//
// Shape of the one launch (what differs from sage.hip):
//   entries  staged in LDS as {byte offset of the gathered row | relation, val}: the offset is a multiple of 16 (ldx in
//            multiples of 4 floats), so the relation rides in its low bits and an entry stays 8 bytes (7: no relation -- a
//            slack entry, or an entry whose column lies outside [0, n), checked before the multiply).
//   gather   K / 4 lanes per row as in sage.hip, R float4 accumulators per row.  A slot past the row's end gets the relation 7,
//            which no accumulator answers to.
//   tiles    (R + 1) x 32 x (K + 4) floats: the R means, then the tile's own rows (not written without root_weight).
//   product  v_mfma_f32_16x16x4_f32, wave w owns output columns [16w, 16w + 16) of both 16-row halves.  The A operand is read
//            as ds_read_b64: lane (row = l & 15, q = l >> 4) takes tile[row][8 j + 2 q .. + 1] and feeds two MFMAs, so the
//            products run over k in the order 8 j + 2 q + s and the B registers hold W[8 j + 2 q + s][column].  Banks of
//            ds_read_b64 are (address / 4) mod 64 within each 32-lane half: with the row stride K + 4 the 16 rows start on
//            16 distinct multiples of 4 (K + 4 = 20, 36, 68, 132: 4 (K / 4 + 1) with K / 4 + 1 odd) and q adds 0 or 2 -- 32
//            lanes on 32 distinct bank pairs, no conflict; the stride stays a multiple of 4 floats, so the tile is written
//            with 16-byte stores.  (A ds_read_b32 has 32 banks: the same stride would put rows r and r + 8 on one bank.)
//            The B registers of block b are reloaded with block b + 1 behind the MFMAs that consumed them, as in sage.hip.
// LDS: (R + 1) * 32 * (K + 4) * 4 + 8.2 KiB of entries; at (R + 1) * K = 5 * 128 that is 90.7 KiB, one workgroup (8 waves) per
// CU; at R = 3: 74.2 KiB (K = 128, two per CU), 42.2 KiB (K = 64, three), 26.2 KiB (K = 32), 18.2 KiB (K = 16).
#include "common.h"
#include "conv_tile.h"

namespace {

typedef float r32x2 __attribute__((ext_vector_type(2)));

constexpr int kRelMax = 4;            // relations served
constexpr int kRelNone = 7;           // the relation of a gather slot that holds no entry

struct RgcnArgs {
  const int32_t* rowptr; const int32_t* colidx; const uint8_t* rel; const float* val;
  const float* x; int64_t ldx;           // [n, K]: gathered, and read row by row for the root term
  int32_t n;
  const float* w;                        // nb row-stacked blocks; w_t == 0: each [K, nc];  w_t == 1: each [nc, K]
  int32_t nc; int w_t; int root;         // output columns (16, 32, 64 or 128); root: the last block multiplies the own rows
  const float* bias;
  float* m; int64_t ldm;                 // M = [A_0 x | .. | A_{R-1} x] (may be NULL)
  float* out; int64_t ldo;
};

// (sage.hip's packed form: two v_pk_fma_f32, each component one IEEE fma)
__device__ __forceinline__ float4 r4fma(float v, float4 h, float4 a) {
  const r32x2 w = {v, v};
  const r32x2 lo = __builtin_elementwise_fma(w, r32x2{h.x, h.y}, r32x2{a.x, a.y});
  const r32x2 hi = __builtin_elementwise_fma(w, r32x2{h.z, h.w}, r32x2{a.z, a.w});
  return make_float4(lo[0], lo[1], hi[0], hi[1]);
}
__device__ __forceinline__ float4 sel4(bool c, float4 a, float4 b) {
  return make_float4(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w);
}

// (launch bounds: the waves per SIMD that LDS admits -- one workgroup per CU at (R + 1) K = 640, two or more below)
template <int K, int R>
__global__ __launch_bounds__(512, (R + 1) * K > 512 ? 2 : 4) void rgcn_conv_kernel(RgcnArgs p) {
  constexpr int LPR = K / 4;                 // lanes per gathered row
  constexpr int GW = 64 / LPR < 4 ? 64 / LPR : 4;   // row groups per wave that hold rows
  constexpr int NG = 8 * GW;                 // row groups per workgroup
  constexpr int RPG = kTileRows / NG;        // rows per group (2 at K = 128)
  constexpr int U = 4;                       // entries per row per trip
  constexpr int SL = 2 * U;                  // slack entries behind the staged ones
  constexpr int NQ = (kTileRows * LPR + 511) / 512;   // 16-byte pieces of the tile's own rows per thread (2 at K = 128)
  constexpr int LD = K + 4;                  // row stride of a tile: see the A-operand read
  static_assert(K == 16 || K == 32 || K == 64 || K == 128, "gather width");
  static_assert(R >= 1 && R <= kRelMax, "relations");
  static_assert(NG * RPG == kTileRows, "every row of the tile has a lane group");
  __shared__ __attribute__((aligned(16))) float tile[R + 1][kTileRows][LD];   // the R means, then the own rows
  __shared__ __attribute__((aligned(8))) int2 s_ent[kTileCap + SL];            // {row offset in bytes | relation, val}
  __shared__ int32_t s_rp[kTileRows + 1];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = gcnx_xcd_remap(blockIdx.x, gridDim.x);
  const int r0 = t * kTileRows, nr = min(p.n - r0, kTileRows);
  if (tid <= nr) s_rp[tid] = p.rowptr[r0 + tid];
  const int e0 = p.rowptr[r0], e1 = p.rowptr[r0 + nr];
  const int staged = min(e1 - e0, kTileCap);
  const unsigned ld4 = (unsigned)p.ldx * 4u;             // bytes per row of x (a multiple of 16)
  for (int i = tid; i < staged + SL; i += 512) {
    int2 en = make_int2(kRelNone, 0);
    if (i < staged) {
      const unsigned j = (unsigned)p.colidx[e0 + i];
      // a column outside [0, n) is checked here, before the multiply can wrap it back into range: such an entry adds nothing
      if (j < (unsigned)p.n) en.x = (int)(j * ld4 | (unsigned)(p.rel[e0 + i] & 3u));
      en.y = __float_as_int(p.val[e0 + i]);
    }
    s_ent[i] = en;
  }
  // ---- the tile's own rows: in flight from here to the tile write ---------------------------------------------------
  float4 own[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int i = tid + 512 * q, row = i / LPR, c4 = i - row * LPR;
    own[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.root && row < nr) own[q] = *reinterpret_cast<const float4*>(p.x + (int64_t)(r0 + row) * p.ldx + 4 * c4);
  }
  // ---- gather --------------------------------------------------------------------------------------------------------
  const int grp = lane / LPR, sub = lane % LPR;
  const bool has_rows = grp < GW;
  const int gid = wave * GW + (has_rows ? grp : 0);
  // the descriptor ends behind the last row's K columns (a column slice of a wider array: nothing past them is addressed)
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.x, (short)0, (int)((unsigned)(p.n - 1) * ld4 + (unsigned)K * 4u), 0x00020000);
  __syncthreads();
  float4 acc[RPG][R];
  int ea[RPG], eb[RPG], ebf[RPG];
  int len = 0;
#pragma unroll
  for (int j = 0; j < RPG; ++j) {
    const int r = gid + j * NG;
#pragma unroll
    for (int q = 0; q < R; ++q) acc[j][q] = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool live = has_rows && r < nr;
    ea[j] = live ? s_rp[r] - e0 : 0;
    eb[j] = live ? s_rp[r + 1] - e0 : 0;
    ebf[j] = min(eb[j], kTileCap);                   // the staged part of the row ...
    ea[j] = min(ea[j], kTileCap);                    // ... (empty if the row starts past it)
    len = max(len, ebf[j] - ea[j]);
  }
  const unsigned sub16 = (unsigned)sub * 16u;
  // Branch-free, as sage.hip: slots past the row's end get an out-of-range offset (the buffer load returns zeros without a
  // fetch) and the relation kRelNone.
  for (int tt = 0; __builtin_amdgcn_ballot_w64(tt < len) != 0; tt += U) {
    float4 hv[RPG][U];
    float wv[RPG][U];
    int rl[RPG][U];
#pragma unroll
    for (int j = 0; j < RPG; ++j) {
      const int eb_ = min(ea[j] + tt, ebf[j]);         // a row that is done stays at its end: the reads stay inside the slack
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int e = eb_ + u;
        const int2 en = s_ent[e];
        const bool in = e < ebf[j];
        wv[j][u] = __int_as_float(en.y);
        rl[j][u] = in ? (en.x & 7) : kRelNone;
        hv[j][u] = buf4(xr, in ? ((unsigned)en.x & ~15u) + sub16 : kOffOut);
      }
    }
    __builtin_amdgcn_sched_barrier(0);                 // all loads of the trip go out before the first is consumed
#pragma unroll
    for (int j = 0; j < RPG; ++j)
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int q = 0; q < R; ++q) acc[j][q] = sel4(rl[j][u] == q, r4fma(wv[j][u], hv[j][u], acc[j][q]), acc[j][q]);
  }
  if (e1 - e0 > kTileCap) {       // uniform per workgroup, rare: entries beyond the staged ones, one at a time from global memory
#pragma unroll
    for (int j = 0; j < RPG; ++j)
      for (int e = max(eb[j] > 0 ? s_rp[gid + j * NG] - e0 : 0, kTileCap); e < eb[j]; ++e) {   // (ea is clamped: the row's true start)
        const float v = p.val[e0 + e];
        const unsigned jc = (unsigned)p.colidx[e0 + e];
        const bool inside = jc < (unsigned)p.n;                                        // (as the staging loop)
        const int rr = inside ? p.rel[e0 + e] : kRelNone;
        const float4 h = buf4(xr, inside ? jc * ld4 + sub16 : kOffOut);
#pragma unroll
        for (int q = 0; q < R; ++q) acc[j][q] = sel4(rr == q, r4fma(v, h, acc[j][q]), acc[j][q]);
      }
  }
  // ---- this wave's slice of block 0 of W, in the MFMA B layout; in flight while the tiles are written ----------------
  const int c16 = lane & 15, kq = lane >> 4;
  const bool wave_on = 16 * wave < p.nc;
  const int col = 16 * wave + c16;
  const int nb = R + (p.root ? 1 : 0);
  // element (k, col) of a block: [K, nc] or, w_t, [nc, K] as stored; register 2 j + s holds k = 8 j + 2 kq + s
  const int64_t wk = p.w_t ? 1 : (int64_t)p.nc;                                          // k -> k + 1
  const int64_t woff = p.w_t ? (int64_t)col * K + 2 * kq : (int64_t)(2 * kq) * p.nc + col;
  const int64_t wblk = (int64_t)K * p.nc;
  float wreg[K / 4];
  if (wave_on) {
#pragma unroll
    for (int e = 0; e < K / 4; ++e) wreg[e] = p.w[woff + (8 * (e >> 1) + (e & 1)) * wk];
  }
  if (has_rows) {
#pragma unroll
    for (int j = 0; j < RPG; ++j) {
      const int r = gid + j * NG;
#pragma unroll
      for (int q = 0; q < R; ++q) {
        if (p.m && r < nr) *reinterpret_cast<float4*>(p.m + (int64_t)(r0 + r) * p.ldm + q * K + sub * 4) = acc[j][q];
        *reinterpret_cast<float4*>(&tile[q][r][sub * 4]) = acc[j][q];      // rows past the end hold zeros
      }
    }
  }
  if (p.root) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int i = tid + 512 * q, row = i / LPR, c4 = i - row * LPR;
      if (row < kTileRows) *reinterpret_cast<float4*>(&tile[R][row][4 * c4]) = own[q];
    }
  }
  __syncthreads();
  // ---- product and epilogue, in registers: wave w owns output columns [16w, 16w + 16) of all 32 rows ------------------
  // C layout of the 16 x 16 tile: column = lane & 15, rows 4 (lane >> 4) + reg.
  if (!wave_on) return;
  const float bcol = p.bias ? p.bias[col] : 0.f;
  gcnx_f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = c0;
#pragma unroll
  for (int b = 0; b <= R; ++b) {
    if (b < nb) {
      const bool more = b + 1 < nb;
      const float* wn = p.w + (int64_t)(b + 1) * wblk + woff;
#pragma unroll
      for (int j = 0; j < K / 8; ++j) {
        const r32x2 a0 = *reinterpret_cast<const r32x2*>(&tile[b][c16][8 * j + 2 * kq]);
        const r32x2 a1 = *reinterpret_cast<const r32x2*>(&tile[b][16 + c16][8 * j + 2 * kq]);
        c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[0], wreg[2 * j], c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[0], wreg[2 * j], c1, 0, 0, 0);
        c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[1], wreg[2 * j + 1], c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[1], wreg[2 * j + 1], c1, 0, 0, 0);
        if (more) {                                      // the same registers, behind the MFMAs that read them
          wreg[2 * j] = wn[(8 * j) * wk];
          wreg[2 * j + 1] = wn[(8 * j + 1) * wk];
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int row = 16 * (r >> 2) + 4 * kq + (r & 3);
    const float v = (r < 4 ? c0[r & 3] : c1[r & 3]) + bcol;
    if (row < nr) p.out[(int64_t)(r0 + row) * p.ldo + col] = v;
  }
}

// ---- the panel alone, any width: a group of lanes walks a row, the column on the lane ---------------------------------------
template <int VEC> struct RgcnVec;
template <> struct RgcnVec<4> {
  float4 v;
  __device__ __forceinline__ void zero() { v = make_float4(0.f, 0.f, 0.f, 0.f); }
  __device__ __forceinline__ void load(const float* p) { v = *reinterpret_cast<const float4*>(p); }
  __device__ __forceinline__ void store(float* p) const { *reinterpret_cast<float4*>(p) = v; }
  __device__ __forceinline__ void fma_if(bool c, float s, const RgcnVec& h) { v = sel4(c, fma4(s, h.v, v), v); }
};
template <> struct RgcnVec<1> {
  float v;
  __device__ __forceinline__ void zero() { v = 0.f; }
  __device__ __forceinline__ void load(const float* p) { v = *p; }
  __device__ __forceinline__ void store(float* p) const { *p = v; }
  __device__ __forceinline__ void fma_if(bool c, float s, const RgcnVec& h) { v = c ? fmaf(s, h.v, v) : v; }
};

template <int VEC>
__global__ __launch_bounds__(256) void rgcn_aggregate_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                                             const uint8_t* __restrict__ rel, const float* __restrict__ val,
                                                             const float* __restrict__ x, int64_t ldx, float* __restrict__ m,
                                                             int64_t ldm, int32_t n, int32_t f, int32_t nrel, int lpr_log2) {
  const int lpr = 1 << lpr_log2, rpb = 256 >> lpr_log2;
  const int g = threadIdx.x >> lpr_log2, sub = threadIdx.x & (lpr - 1);
  const int64_t r = (int64_t)blockIdx.x * rpb + g;
  const int col = (blockIdx.y * lpr + sub) * VEC;
  if (r >= n || col >= f) return;
  const int b = rowptr[r], e = rowptr[r + 1];
  RgcnVec<VEC> acc[kRelMax];
#pragma unroll
  for (int q = 0; q < kRelMax; ++q) acc[q].zero();
  for (int i = b; i < e; ++i) {               // stored order: a row's sums are the same bits in every run
    const unsigned j = (unsigned)colidx[i];
    if (j >= (unsigned)n) continue;           // (the one launch's range-checked load fetches nothing there)
    const int rr = rel[i];
    const float v = val[i];
    RgcnVec<VEC> h;
    h.load(x + (int64_t)j * ldx + col);
#pragma unroll
    for (int q = 0; q < kRelMax; ++q) acc[q].fma_if(rr == q, v, h);
  }
#pragma unroll
  for (int q = 0; q < kRelMax; ++q)
    if (q < nrel) acc[q].store(m + r * ldm + (int64_t)q * f + col);
}

// ---- relations and values ---------------------------------------------------------------------------------------------------
// rule 0 ("nonzero"): the first column d with e[k, d] != 0, edge_dim if there is none (nrel = edge_dim + 1).
// rule 1 ("index"): column 0 as an integer, clamped to 0 .. nrel - 1 (a NaN reads 0).
__device__ __forceinline__ int rgcn_rel_of(const float* __restrict__ e, int64_t lde, int edge_dim, int rule, int nrel, int64_t k) {
  const float* ek = e + k * lde;
  if (rule == 0) {
    int d = 0;
    while (d < edge_dim && !(ek[d] != 0.f)) ++d;
    return d;
  }
  const float v = ek[0];
  return v >= 1.f ? (int)fminf(v, (float)(nrel - 1)) : 0;
}

__global__ __launch_bounds__(256) void rgcn_rows_kernel(const int32_t* __restrict__ rowptr, const float* __restrict__ e, int64_t lde,
                                                        int edge_dim, int rule, int nrel, int32_t n, uint8_t* __restrict__ rel,
                                                        float* __restrict__ val) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int b = rowptr[i], en = rowptr[i + 1];
  int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  for (int k = b; k < en; ++k) {
    const int r = rgcn_rel_of(e, lde, edge_dim, rule, nrel, k);
    rel[k] = (uint8_t)r;
    c0 += r == 0; c1 += r == 1; c2 += r == 2; c3 += r == 3;
  }
  const float v0 = 1.0f / (float)max(c0, 1), v1 = 1.0f / (float)max(c1, 1), v2 = 1.0f / (float)max(c2, 1), v3 = 1.0f / (float)max(c3, 1);
  for (int k = b; k < en; ++k) {
    const int r = rgcn_rel_of(e, lde, edge_dim, rule, nrel, k);
    val[k] = r == 0 ? v0 : r == 1 ? v1 : r == 2 ? v2 : v3;
  }
}

__global__ __launch_bounds__(256) void rgcn_perm_kernel(const int32_t* __restrict__ perm_t, int64_t nnz, const uint8_t* __restrict__ rel,
                                                        const float* __restrict__ val, uint8_t* __restrict__ rel_t,
                                                        float* __restrict__ val_t) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= nnz) return;
  const int64_t s = perm_t[k];
  const bool ok = s >= 0 && s < nnz;
  rel_t[k] = ok ? rel[s] : (uint8_t)0;
  val_t[k] = ok ? val[s] : 0.f;
}

// ---- host side ------------------------------------------------------------------------------------------------------------
bool rgcn_width_ok(int32_t w) { return w == 16 || w == 32 || w == 64 || w == 128; }
bool rgcn_shape_ok(int64_t n, int32_t k, int32_t nc, int32_t nrel, int64_t ldx) {
  return n >= 0 && n <= 0x7FFFFFFFll && rgcn_width_ok(k) && rgcn_width_ok(nc) && nrel >= 1 && nrel <= kRelMax && ldx >= k &&
         ldx % 4 == 0 && (uint64_t)n * (uint64_t)ldx * 4u < 0xFFFFFFF0ull;
}

template <int K_>
void launch_rgcn_k(gcnx_ctx* ctx, const RgcnArgs& a, int nrel, int tiles) {
  if (nrel == 1) hipLaunchKernelGGL((rgcn_conv_kernel<K_, 1>), dim3(tiles), dim3(512), 0, ctx->stream, a);
  else if (nrel == 2) hipLaunchKernelGGL((rgcn_conv_kernel<K_, 2>), dim3(tiles), dim3(512), 0, ctx->stream, a);
  else if (nrel == 3) hipLaunchKernelGGL((rgcn_conv_kernel<K_, 3>), dim3(tiles), dim3(512), 0, ctx->stream, a);
  else hipLaunchKernelGGL((rgcn_conv_kernel<K_, 4>), dim3(tiles), dim3(512), 0, ctx->stream, a);
}

int launch_rgcn(gcnx_ctx* ctx, const RgcnArgs& a, int k, int nrel) {
  const int tiles = gcnx_cdiv(a.n, kTileRows);
  if (k == 128) launch_rgcn_k<128>(ctx, a, nrel, tiles);
  else if (k == 64) launch_rgcn_k<64>(ctx, a, nrel, tiles);
  else if (k == 32) launch_rgcn_k<32>(ctx, a, nrel, tiles);
  else launch_rgcn_k<16>(ctx, a, nrel, tiles);
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

}  // namespace

extern "C" {

int gcnx_rgcn_operator(gcnx_ctx* ctx, const int32_t* rowptr, const float* e, int64_t lde, int32_t edge_dim, int32_t rule,
                       int32_t num_relations, const int32_t* perm_t, int32_t n, int64_t nnz, uint8_t* rel, float* val, uint8_t* rel_t,
                       float* val_t) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "RGCNConv relations and values");
  GCNX_REQUIRE(ctx, n >= 0 && nnz >= 0 && nnz <= 0x7FFFFFFFll, "gcnx_rgcn_operator: needs n >= 0 and 0 <= nnz < 2^31");
  GCNX_REQUIRE(ctx, rule == GCNX_RGCN_NONZERO || rule == GCNX_RGCN_INDEX, "gcnx_rgcn_operator: rule = %d must be GCNX_RGCN_NONZERO or "
               "GCNX_RGCN_INDEX", rule);
  GCNX_REQUIRE(ctx, num_relations >= 1 && num_relations <= kRelMax, "gcnx_rgcn_operator: num_relations = %d must be in 1 .. %d",
               num_relations, kRelMax);
  GCNX_REQUIRE(ctx, edge_dim >= 1 && lde >= edge_dim, "gcnx_rgcn_operator: needs edge_dim >= 1 and lde >= edge_dim");
  GCNX_REQUIRE(ctx, rule != GCNX_RGCN_NONZERO || num_relations == edge_dim + 1,
               "gcnx_rgcn_operator: the rule GCNX_RGCN_NONZERO has num_relations = edge_dim + 1 (got %d and edge_dim = %d)", num_relations,
               edge_dim);
  GCNX_REQUIRE(ctx, (rel_t == nullptr) == (val_t == nullptr) && (rel_t == nullptr) == (perm_t == nullptr),
               "gcnx_rgcn_operator: perm_t, rel_t and val_t must all be given or all be NULL");
  if (n == 0 || nnz == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, rowptr && e && rel && val, "gcnx_rgcn_operator: NULL pointer");
  hipLaunchKernelGGL(rgcn_rows_kernel, dim3(gcnx_cdiv(n, 256)), dim3(256), 0, ctx->stream, rowptr, e, lde, edge_dim, rule, num_relations, n,
                     rel, val);
  GCNX_LAUNCH_OK(ctx);
  if (perm_t) {
    hipLaunchKernelGGL(rgcn_perm_kernel, dim3((unsigned)gcnx_cdiv(nnz, 256)), dim3(256), 0, ctx->stream, perm_t, nnz, rel, val, rel_t, val_t);
    GCNX_LAUNCH_OK(ctx);
  }
  return GCNX_OK;
}

int gcnx_rgcn_conv_ok(int64_t n, int32_t fi, int32_t fo, int32_t num_relations, int64_t ldx) {
  return rgcn_shape_ok(n, fi, fo, num_relations, ldx) ? 1 : 0;
}

int gcnx_rgcn_conv(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const uint8_t* rel, const float* val, const float* x,
                   int64_t ldx, int32_t n, int32_t fi, const float* w, int root_weight, int32_t fo, int32_t num_relations,
                   int w_transposed, const float* bias, float* m, int64_t ldm, float* out, int64_t ldo) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "RGCNConv (one launch)");
  GCNX_REQUIRE(ctx, n >= 0 && fi >= 0 && fo >= 0, "gcnx_rgcn_conv: negative size");
  if (!rgcn_shape_ok(n, fi, fo, num_relations, ldx))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_rgcn_conv: needs fi and fo in {16, 32, 64, 128}, num_relations in 1 .. 4, ldx >= fi in "
                     "multiples of 4 floats and n * ldx * 4 < 2^32 (got n=%d fi=%d fo=%d num_relations=%d ldx=%lld): use "
                     "gcnx_rgcn_aggregate + gcnx_gemm", n, fi, fo, num_relations, (long long)ldx);
  if (!gcnx_aligned16(x) || !gcnx_aligned16(w) || !gcnx_aligned16(out) || ldo < fo || ldo % 4 != 0 ||
      (m && (!gcnx_aligned16(m) || ldm < (int64_t)num_relations * fi || ldm % 4 != 0)))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_rgcn_conv: x, w, m and out must be 16-byte aligned, with ldm >= num_relations * fi and "
                     "ldo >= fo in multiples of 4 floats");
  if (n == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, rowptr && colidx && rel && val && x && w && out, "gcnx_rgcn_conv: NULL pointer");
  GCNX_REQUIRE(ctx, x != out && x != m && (!m || m != out), "gcnx_rgcn_conv: the outputs must not alias x or each other");
  RgcnArgs a{};
  a.rowptr = rowptr; a.colidx = colidx; a.rel = rel; a.val = val; a.x = x; a.ldx = ldx; a.n = n; a.w = w; a.nc = fo;
  a.w_t = w_transposed ? 1 : 0; a.root = root_weight ? 1 : 0; a.bias = bias; a.m = m; a.ldm = ldm; a.out = out; a.ldo = ldo;
  return launch_rgcn(ctx, a, fi, num_relations);
}

int gcnx_rgcn_aggregate(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const uint8_t* rel, const float* val, const float* x,
                        int64_t ldx, int32_t n, int32_t f, int32_t num_relations, float* m, int64_t ldm) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "RGCNConv aggregate");
  GCNX_REQUIRE(ctx, num_relations >= 1 && num_relations <= kRelMax, "gcnx_rgcn_aggregate: num_relations = %d must be in 1 .. %d",
               num_relations, kRelMax);
  GCNX_REQUIRE(ctx, n >= 0 && f >= 1 && ldx >= f && ldm >= (int64_t)num_relations * f,
               "gcnx_rgcn_aggregate: needs n >= 0, f >= 1, ldx >= f and ldm >= num_relations * f");
  if (n == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, rowptr && colidx && rel && val && x && m, "gcnx_rgcn_aggregate: NULL pointer");
  GCNX_REQUIRE(ctx, x != m, "gcnx_rgcn_aggregate: m must not alias x");
  const bool vec = f % 4 == 0 && ldx % 4 == 0 && ldm % 4 == 0 && gcnx_aligned16(x) && gcnx_aligned16(m);
  const int units = vec ? f / 4 : f;                   // lanes a row needs
  int lpr_log2 = 0;
  while ((1 << lpr_log2) < units && lpr_log2 < 6) ++lpr_log2;
  const int rpb = 256 >> lpr_log2;
  const int ny = gcnx_cdiv(units, 1 << lpr_log2);
  GCNX_REQUIRE(ctx, ny <= 65535, "gcnx_rgcn_aggregate: f=%d is too wide", f);
  const dim3 grid(gcnx_cdiv(n, rpb), ny);
  if (vec) hipLaunchKernelGGL((rgcn_aggregate_kernel<4>), grid, dim3(256), 0, ctx->stream, rowptr, colidx, rel, val, x, ldx, m, ldm, n, f,
                              num_relations, lpr_log2);
  else hipLaunchKernelGGL((rgcn_aggregate_kernel<1>), grid, dim3(256), 0, ctx->stream, rowptr, colidx, rel, val, x, ldx, m, ldm, n, f,
                          num_relations, lpr_log2);
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

}  // extern "C"
