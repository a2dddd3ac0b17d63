// GINEConv: GINConv whose neighbour sum reads the edge features (PyG GINEConv(nn, eps, train_eps, edge_dim); Hu et al.,
// "Strategies for Pre-training Graph Neural Networks") -- the cheapest way to put the dca / proximity values the reference
// computes on every contact and bridge and then drops (gcn_utills.py:319-443; gcn.py:71) into a message: one add and one ReLU
// per gathered element.
//
//     m_ij = x_j + (e_ij W_e + b_e)        msg_ij = relu(m_ij)           W_e [edge_dim, K0], 1 <= edge_dim <= 8
//     T = (1 + eps) x + sum_j msg_ij       U = relu(T W_a + b_a)         out = U W_b + b_b
//
// The ReLU sits between the edge term and the sum, so neither gin_conv_kernel nor a SpMM can form T, and the transposed
// single-stage form GIN uses for dX does not exist (the mask depends on the entry).  m is stored nowhere: the three kernels
// that need it recompute it in fp32 EXACTLY as include/gcnx.h writes it down (gine_msg below: every product and every sum
// rounded on its own, no FMA, edge features added in ascending order, then the bias, then x_j; the positive side is m > 0), so
// they agree on the side of every kink.
//
// gine_conv_kernel is gin_conv_kernel's workgroup (gin.hip; the device helpers they share: conv_tile.h): 512 threads, 32 rows,
// K0 / 4 lanes per gathered row, the tile's CSR entries staged
// in LDS, four entries per row and trip with every load of a trip issued before the first is consumed, then two chained
// v_mfma_f32_16x16x4_f32 stages through LDS tiles.  What differs in the gather:
//   e        an entry's features are read by every lane of its row's group with range-checked scalar-width buffer loads from a
//            descriptor over the TILE's rows of e (the lanes of a group read one address: one request); the loads of a trip go
//            out with the trip's row loads.  edge_dim is a kernel argument; the instance fixes the number of slots (DM = 2 or
//            8), and a slot at or past edge_dim gets an out-of-range offset: no fetch, and its term is dropped by a select.
//   w_e, b_e the lane's four columns of every row of W_e and of b_e sit in registers (4 DM + 4 floats), loaded before the
//            staging barrier.
//   padding  a slot past the row's end would add relu(0 + v), not +0: its message is replaced by +0 explicitly.  (Adding +0
//            leaves the sum's bits alone: the sum starts at +0 and no message is negative, so it is never -0.)
// LDS as gin_conv_kernel: T tile, U tile, 4 KiB of entries.
//
// gine_aggregate_kernel is T alone for any width (float4 lanes: the bits of gine_conv_kernel's T); gine_bwd_edges_* the pass
// over the forward CSR for dW_e and db_e (per-workgroup parts, then one small launch over them, both in a fixed order);
// gine_bwd_nodes_kernel the pass over the transposed pattern for dx.
#include "common.h"
#include "conv_tile.h"

namespace {

constexpr int kEMaxW = 128;       // widest stage
constexpr int kEdgeRows = 32;     // rows per workgroup of the dW_e / db_e pass

struct GineArgs {
  const int32_t* rowptr; const int32_t* colidx;
  const float* x; int64_t ldx;           // [n, K0]: gathered, and read row by row for the (1 + eps) term
  int32_t n;
  const float* eps;                      // device scalar, or NULL = 0
  const float* e; int64_t lde; int32_t edge_dim;   // [nnz, edge_dim] in the CSR's entry order
  const float* w_e; const float* b_e;    // [edge_dim, K0], [K0] (may be NULL)
  const float* w_a; const float* b_a;    // [K0, k1]
  int32_t k1;
  const float* w_b; const float* b_b;    // [k1, k2]
  int32_t k2;
  float* t; int64_t ldt;                 // T (may be NULL)
  float* u; int64_t ldu;                 // U (may be NULL)
  float* out; int64_t ldo;
};

__device__ __forceinline__ float ebuf1(__amdgpu_buffer_rsrc_t rs, unsigned off) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0));
}

// The contract's m for one channel: ev = the entry's features (slots at or past d_n hold anything), w = the channel's column
// of W_e, b = its bias (has_b false: no bias), xj = the source's value.
template <int DM>
__device__ __forceinline__ float gine_msg(const float (&ev)[DM], const float (&w)[DM], float b, bool has_b, int d_n, float xj) {
  // Plain operators under contract(off): hipcc contracts a * b + c into an FMA by default, and __fmul_rn / __fadd_rn are plain
  // operators compiled under that default, so they do not keep a product and a sum apart.
#pragma clang fp contract(off)
  float t = ev[0] * w[0];
#pragma unroll
  for (int d = 1; d < DM; ++d) {
    const float s = t + ev[d] * w[d];
    t = d < d_n ? s : t;
  }
  const float v = has_b ? t + b : t;
  return xj + v;
}

template <int K, int DM>
__global__ __launch_bounds__(512) void gine_conv_kernel(GineArgs p) {
  constexpr int LPR = K / 4;                 // lanes per gathered row
  constexpr int GW = 64 / LPR < 4 ? 64 / LPR : 4;   // row groups per wave that hold rows (the lanes behind them idle in the gather)
  constexpr int NG = 8 * GW;                 // row groups per workgroup
  constexpr int RPG = kTileRows / NG;        // rows per group (2 at K = 128)
  constexpr int U = 4;                       // entries per row per trip
  constexpr int SL = 2 * U;                  // slack entries behind the staged ones
  static_assert(K == 16 || K == 32 || K == 64 || K == 128, "gather width");
  static_assert(NG * RPG == kTileRows, "every row of the tile has a lane group");
  __shared__ __attribute__((aligned(16))) float tile_t[kTileRows][K + 4];        // row stride K + 4: see gin.hip, the A-operand read
  __shared__ __attribute__((aligned(16))) float tile_u[kTileRows * (kEMaxW + 4)];   // row stride k1 + 4
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
  // ---- the rows' own pieces and the lane's columns of W_e / b_e: in flight from here to the end of the gather ------------
  const int grp = lane / LPR, sub = lane % LPR;
  const bool has_rows = grp < GW;
  const int gid = wave * GW + (has_rows ? grp : 0);
  const int dn = p.edge_dim;
  const bool has_b = p.b_e != nullptr;
  float we[4][DM], be[4];
#pragma unroll
  for (int d = 0; d < DM; ++d) {
    float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
    if (d < dn) w = *reinterpret_cast<const float4*>(p.w_e + (int64_t)d * K + 4 * sub);
    we[0][d] = w.x; we[1][d] = w.y; we[2][d] = w.z; we[3][d] = w.w;
  }
  {
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    if (has_b) b = *reinterpret_cast<const float4*>(p.b_e + 4 * sub);
    be[0] = b.x; be[1] = b.y; be[2] = b.z; be[3] = b.w;
  }
  float4 own[RPG];
#pragma unroll
  for (int j = 0; j < RPG; ++j) {
    const int r = gid + j * NG;
    own[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (has_rows && r < nr) own[j] = *reinterpret_cast<const float4*>(p.x + (int64_t)(r0 + r) * p.ldx + 4 * sub);
  }
  const float scale = 1.0f + (p.eps ? p.eps[0] : 0.f);
  // ---- gather --------------------------------------------------------------------------------------------------------
  // the descriptors end behind the last row's columns (a column slice of a wider array: nothing past them is addressed);
  // the one over e covers the tile's entries only, so its 32-bit offsets never see the whole array
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.x, (short)0, (int)((unsigned)(p.n - 1) * ld4 + (unsigned)K * 4u), 0x00020000);
  const unsigned lde4 = (unsigned)p.lde * 4u;
  const uint64_t ebytes = e1 > e0 ? (uint64_t)(e1 - e0 - 1) * lde4 + (uint64_t)dn * 4u : 0u;
  const __amdgpu_buffer_rsrc_t er = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(p.e + (int64_t)e0 * p.lde), (short)0, (int)(unsigned)(ebytes < 0xFFFFFF00ull ? ebytes : 0xFFFFFF00ull), 0x00020000);
  __syncthreads();
  float acc[RPG][4];
  int ea[RPG], eb[RPG], ebf[RPG];
  int len = 0;
#pragma unroll
  for (int j = 0; j < RPG; ++j) {
    const int r = gid + j * NG;
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[j][c] = 0.f;
    const bool live = has_rows && r < nr;
    ea[j] = live ? s_rp[r] - e0 : 0;
    eb[j] = live ? s_rp[r + 1] - e0 : 0;
    ebf[j] = min(eb[j], kTileCap);                   // the staged part of the row ...
    ea[j] = min(ea[j], kTileCap);                    // ... (empty if the row starts past it)
    len = max(len, ebf[j] - ea[j]);
  }
  const unsigned sub16 = (unsigned)sub * 16u;
  // Branch-free, as in gin.hip: slots past the row's end get out-of-range offsets and fetch nothing.
  for (int tt = 0; __builtin_amdgcn_ballot_w64(tt < len) != 0; tt += U) {
    gcnx_f32x4 hv[RPG][U];
    float ev[RPG][U][DM];
#pragma unroll
    for (int j = 0; j < RPG; ++j) {
      const int eb_ = min(ea[j] + tt, ebf[j]);         // a row that is done stays at its end: the reads stay inside the slack
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int e = eb_ + u;
        const bool live = e < ebf[j];
        hv[j][u] = buf4v(xr, live ? (unsigned)s_ent[e] + sub16 : kOffOut);
#pragma unroll
        for (int d = 0; d < DM; ++d) ev[j][u][d] = ebuf1(er, live && d < dn ? (unsigned)e * lde4 + 4u * d : kOffOut);
      }
    }
    __builtin_amdgcn_sched_barrier(0);                 // all loads of the trip go out before the first is consumed
#pragma unroll
    for (int j = 0; j < RPG; ++j) {
      const int eb_ = min(ea[j] + tt, ebf[j]);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool live = eb_ + u < ebf[j];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float m = gine_msg<DM>(ev[j][u], we[c], be[c], has_b, dn, hv[j][u][c]);
          acc[j][c] += live && m > 0.f ? m : 0.f;      // a padding slot adds +0, not relu(0 + v)
        }
      }
    }
  }
  if (e1 - e0 > kTileCap) {       // uniform per workgroup, rare: entries beyond the staged ones, one at a time from global memory
#pragma unroll
    for (int j = 0; j < RPG; ++j)
      for (int e = max(eb[j] > 0 ? s_rp[gid + j * NG] - e0 : 0, kTileCap); e < eb[j]; ++e) {   // (ea is clamped: the row's true start)
        const gcnx_f32x4 h = buf4v(xr, (unsigned)p.colidx[e0 + e] * ld4 + sub16);
        float ev1[DM];
#pragma unroll
        for (int d = 0; d < DM; ++d) ev1[d] = d < dn ? p.e[(int64_t)(e0 + e) * p.lde + d] : 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float m = gine_msg<DM>(ev1, we[c], be[c], has_b, dn, h[c]);
          acc[j][c] += m > 0.f ? m : 0.f;
        }
      }
  }
  // ---- this wave's slice of W_a, in the MFMA B layout; in flight while the tile is written -----------------------------
  const int c16 = lane & 15, kq = lane >> 4;
  const bool on1 = 16 * wave < p.k1;
  const int col = 16 * wave + c16;
  const int64_t wstep = 4 * (int64_t)p.k1;                                    // k -> k + 4
  const int64_t woff = (int64_t)kq * p.k1 + col;                              // k = kq
  float wreg[K / 4];
  if (on1) {
#pragma unroll
    for (int e = 0; e < K / 4; ++e) wreg[e] = p.w_a[woff + e * wstep];
  }
  if (has_rows) {
#pragma unroll
    for (int j = 0; j < RPG; ++j) {
      const int r = gid + j * NG;
      const float4 tv = make_float4(fmaf(scale, own[j].x, acc[j][0]), fmaf(scale, own[j].y, acc[j][1]),
                                    fmaf(scale, own[j].z, acc[j][2]), fmaf(scale, own[j].w, acc[j][3]));
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
      v = v > 0.f ? v : 0.f;
      tile_u[row * su + col] = v;
      if (p.u && row < nr) p.u[(int64_t)(r0 + row) * p.ldu + col] = v;
    }
  }
  // ---- second product: this wave's slice of W_b, loaded while the other waves finish the U tile --------------------------
  const bool on2 = 16 * wave < p.k2;
  const int64_t wstep2 = 4 * (int64_t)p.k2;
  const int64_t woff2 = (int64_t)kq * p.k2 + col;
  float w2[kEMaxW / 4];
#pragma unroll
  for (int g = 0; g < kEMaxW / 16; ++g) {
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
  for (int g = 0; g < kEMaxW / 16; ++g) {
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

bool gine_width_ok(int32_t k) { return k >= 16 && k <= kEMaxW && k % 16 == 0; }
bool gine_dim_ok(int32_t d) { return d >= 1 && d <= kEdgeMax; }

bool gine_shape_ok(int64_t n, int32_t k0, int32_t k1, int32_t k2, int64_t ldx, int32_t edge_dim) {
  return n >= 0 && n <= 0x7FFFFFFFll && (k0 == 16 || k0 == 32 || k0 == 64 || k0 == 128) && gine_width_ok(k1) && gine_width_ok(k2) &&
         ldx >= k0 && ldx % 4 == 0 && (uint64_t)n * (uint64_t)ldx * 4u < 0xFFFFFFF0ull && gine_dim_ok(edge_dim);
}

template <int DM>
int launch_gine(gcnx_ctx* ctx, const GineArgs& a, int k0) {
  const int tiles = gcnx_cdiv(a.n, kTileRows);
  if (k0 == 128) hipLaunchKernelGGL((gine_conv_kernel<128, DM>), dim3(tiles), dim3(512), 0, ctx->stream, a);
  else if (k0 == 64) hipLaunchKernelGGL((gine_conv_kernel<64, DM>), dim3(tiles), dim3(512), 0, ctx->stream, a);
  else if (k0 == 32) hipLaunchKernelGGL((gine_conv_kernel<32, DM>), dim3(tiles), dim3(512), 0, ctx->stream, a);
  else hipLaunchKernelGGL((gine_conv_kernel<16, DM>), dim3(tiles), dim3(512), 0, ctx->stream, a);
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

// ---- the lanes of the any-width kernels: VEC = 4 (float4 accesses) or 1 ------------------------------------------------------
template <int VEC> struct GineVec {
  float v[VEC];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int c = 0; c < VEC; ++c) v[c] = 0.f;
  }
  __device__ __forceinline__ void load(const float* p) {
    if constexpr (VEC == 4) {
      const float4 q = *reinterpret_cast<const float4*>(p);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
      v[0] = *p;
    }
  }
  __device__ __forceinline__ void store(float* p) const {
    if constexpr (VEC == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else *p = v[0];
  }
};

// The lane's columns of W_e [d_n, f] and b_e: w[c][d] = W_e[d, col + c].  DM = the instance's slots (2 or 8), d_n <= DM.
template <int VEC, int DM>
struct GineEdgeW {
  float w[VEC][DM], b[VEC];
  bool has_b;
  __device__ __forceinline__ void load(const float* w_e, const float* b_e, int d_n, int f, int col) {
#pragma unroll
    for (int d = 0; d < DM; ++d) {
      GineVec<VEC> t;
      t.zero();
      if (d < d_n) t.load(w_e + (int64_t)d * f + col);
#pragma unroll
      for (int c = 0; c < VEC; ++c) w[c][d] = t.v[c];
    }
    has_b = b_e != nullptr;
    GineVec<VEC> t;
    t.zero();
    if (has_b) t.load(b_e + col);
#pragma unroll
    for (int c = 0; c < VEC; ++c) b[c] = t.v[c];
  }
};

// An entry's features, slots at or past d_n as 0.  Branch-free (a load inside a branch would close the trip it belongs to with
// s_waitcnt vmcnt(0)): such a slot reads feature 0 again, which is there since d_n >= 1.
template <int DM>
__device__ __forceinline__ void gine_load_e(float (&ev)[DM], const float* e_row, int d_n) {
#pragma unroll
  for (int d = 0; d < DM; ++d) {
    const float v = e_row[d < d_n ? d : 0];
    ev[d] = d < d_n ? v : 0.f;
  }
}

constexpr int kEU = 4;            // entries per trip of the any-width kernels: a trip's loads go out before its first use

// ---- T alone, any width: one group of (1 << lpr_log2) lanes per row, blockIdx.y = column block of LPR * VEC columns ------
template <int VEC, int DM>
__global__ __launch_bounds__(256) void gine_aggregate_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                                             const float* __restrict__ x, int64_t ldx, const float* __restrict__ eps,
                                                             const float* __restrict__ e, int64_t lde, int d_n,
                                                             const float* __restrict__ w_e, const float* __restrict__ b_e,
                                                             float* __restrict__ out, int64_t ldo, int32_t n, int32_t f, int lpr_log2) {
  const int lpr = 1 << lpr_log2, rpb = 256 >> lpr_log2;
  const int g = threadIdx.x >> lpr_log2, sub = threadIdx.x & (lpr - 1);
  const int64_t r = (int64_t)blockIdx.x * rpb + g;
  const int col = (blockIdx.y * lpr + sub) * VEC;
  if (r >= n || col >= f) return;
  const float scale = 1.0f + (eps ? eps[0] : 0.f);
  const int b = rowptr[r], en = rowptr[r + 1];
  GineEdgeW<VEC, DM> ew;
  ew.load(w_e, b_e, d_n, f, col);
  GineVec<VEC> own, acc;
  own.load(x + r * ldx + col);
  acc.zero();
  auto add = [&](const GineVec<VEC>& h, const float (&ev)[DM]) {
#pragma unroll
    for (int c = 0; c < VEC; ++c) {
      const float m = gine_msg<DM>(ev, ew.w[c], ew.b[c], ew.has_b, d_n, h.v[c]);
      acc.v[c] += m > 0.f ? m : 0.f;
    }
  };
  int i = b;
  for (; i + kEU <= en; i += kEU) {             // stored order: the sum of a row is the same bits in every run
    GineVec<VEC> h[kEU];
    float ev[kEU][DM];
#pragma unroll
    for (int q = 0; q < kEU; ++q) {
      h[q].load(x + (int64_t)colidx[i + q] * ldx + col);
      gine_load_e<DM>(ev[q], e + (int64_t)(i + q) * lde, d_n);
    }
#pragma unroll
    for (int q = 0; q < kEU; ++q) add(h[q], ev[q]);
  }
  for (; i < en; ++i) {
    GineVec<VEC> h;
    float ev[DM];
    h.load(x + (int64_t)colidx[i] * ldx + col);
    gine_load_e<DM>(ev, e + (int64_t)i * lde, d_n);
    add(h, ev);
  }
#pragma unroll
  for (int c = 0; c < VEC; ++c) acc.v[c] = fmaf(scale, own.v[c], acc.v[c]);
  acc.store(out + r * ldo + col);
}

// ---- dW_e, db_e: the pass over the forward CSR ------------------------------------------------------------------------------
// Workgroup bx owns rows [32 bx, 32 bx + 32); a group of (1 << lpr_log2) lanes walks a row's entries in CSR order, column on the
// lane, and the 256 >> lpr_log2 groups take the rows in turn.  Every thread adds in the same order on every call; the groups'
// sums are then added in group order through LDS.  parts[bx][k][f]: k = 0 the db_e part, k = 1 + d the part of row d of dW_e.
template <int VEC, int DM>
__global__ __launch_bounds__(256) void gine_bwd_edges_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                                             const float* __restrict__ x, int64_t ldx, const float* __restrict__ e,
                                                             int64_t lde, int d_n, const float* __restrict__ w_e,
                                                             const float* __restrict__ b_e, const float* __restrict__ dt, int64_t lddt,
                                                             int32_t n, int32_t f, float* __restrict__ parts, int lpr_log2) {
  constexpr int NA = (1 + DM) * VEC;
  __shared__ float s[256][NA + 1];
  const int lpr = 1 << lpr_log2, rpb = 256 >> lpr_log2;
  const int g = threadIdx.x >> lpr_log2, sub = threadIdx.x & (lpr - 1);
  const int col = (blockIdx.y * lpr + sub) * VEC;
  const bool active = col < f;
  const int64_t r0 = (int64_t)blockIdx.x * kEdgeRows;
  const int nr = (int)(n - r0 < kEdgeRows ? n - r0 : kEdgeRows);
  float acc[1 + DM][VEC];
#pragma unroll
  for (int k = 0; k <= DM; ++k)
#pragma unroll
    for (int c = 0; c < VEC; ++c) acc[k][c] = 0.f;
  if (active) {
    GineEdgeW<VEC, DM> ew;
    ew.load(w_e, b_e, d_n, f, col);
    for (int row = g; row < nr; row += rpb) {
      const int64_t r = r0 + row;
      GineVec<VEC> dti;
      dti.load(dt + r * lddt + col);
      auto add = [&](const GineVec<VEC>& h, const float (&ev)[DM]) {
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
          const float m = gine_msg<DM>(ev, ew.w[c], ew.b[c], ew.has_b, d_n, h.v[c]);
          const float gv = m > 0.f ? dti.v[c] : 0.f;
          acc[0][c] += gv;
#pragma unroll
          for (int d = 0; d < DM; ++d) acc[1 + d][c] = fmaf(ev[d], gv, acc[1 + d][c]);   // (slots past d_n hold 0)
        }
      };
      const int en = rowptr[r + 1];
      int i = rowptr[r];
      for (; i + kEU <= en; i += kEU) {
        GineVec<VEC> h[kEU];
        float ev[kEU][DM];
#pragma unroll
        for (int q = 0; q < kEU; ++q) {
          h[q].load(x + (int64_t)colidx[i + q] * ldx + col);
          gine_load_e<DM>(ev[q], e + (int64_t)(i + q) * lde, d_n);
        }
#pragma unroll
        for (int q = 0; q < kEU; ++q) add(h[q], ev[q]);
      }
      for (; i < en; ++i) {
        GineVec<VEC> h;
        float ev[DM];
        h.load(x + (int64_t)colidx[i] * ldx + col);
        gine_load_e<DM>(ev, e + (int64_t)i * lde, d_n);
        add(h, ev);
      }
    }
  }
#pragma unroll
  for (int k = 0; k <= DM; ++k)
#pragma unroll
    for (int c = 0; c < VEC; ++c) s[threadIdx.x][k * VEC + c] = acc[k][c];
  __syncthreads();
  if (g != 0 || !active) return;
  for (int k = 0; k <= d_n; ++k) {
    GineVec<VEC> tot;
    tot.zero();
    for (int gg = 0; gg < rpb; ++gg)
#pragma unroll
      for (int c = 0; c < VEC; ++c) tot.v[c] += s[gg * lpr + sub][k * VEC + c];
    tot.store(parts + ((int64_t)blockIdx.x * (d_n + 1) + k) * f + col);
  }
}

// The parts of 16 outputs (k, column) per workgroup: slice sl of 16 adds parts sl, sl + 16, ... in ascending order from +0, then
// one thread per output adds the 16 slices in slice order.  Written, never accumulated; nparts == 0 writes zeros.
__global__ __launch_bounds__(256) void gine_bwd_edges_final_kernel(const float* __restrict__ parts, int64_t nparts, int d_n, int32_t f,
                                                                   float* __restrict__ dw_e, float* __restrict__ db_e) {
  __shared__ float s[16][17];
  const int o = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int64_t idx = (int64_t)blockIdx.x * 16 + o, per = (int64_t)(d_n + 1) * f;
  float acc = 0.f;
  if (idx < per)
    for (int64_t q = sl; q < nparts; q += 16) acc += parts[q * per + idx];
  s[sl][o] = acc;
  __syncthreads();
  if (sl != 0 || idx >= per) return;
  float tot = 0.f;
#pragma unroll
  for (int q = 0; q < 16; ++q) tot += s[q][o];
  if (idx < f) {
    if (db_e) db_e[idx] = tot;
  } else {
    dw_e[idx - f] = tot;
  }
}

// ---- dx: the pass over the transposed pattern; the row is the SOURCE j, so m reads the row's own x and the entry's e ------------
template <int VEC, int DM>
__global__ __launch_bounds__(256) void gine_bwd_nodes_kernel(const int32_t* __restrict__ rowptr_t, const int32_t* __restrict__ colidx_t,
                                                             const int32_t* __restrict__ perm_t, const float* __restrict__ x, int64_t ldx,
                                                             const float* __restrict__ eps, const float* __restrict__ e, int64_t lde,
                                                             int d_n, const float* __restrict__ w_e, const float* __restrict__ b_e,
                                                             const float* __restrict__ dt, int64_t lddt, float* __restrict__ dx,
                                                             int64_t lddx, int32_t n, int32_t f, int lpr_log2) {
  const int lpr = 1 << lpr_log2, rpb = 256 >> lpr_log2;
  const int g = threadIdx.x >> lpr_log2, sub = threadIdx.x & (lpr - 1);
  const int64_t r = (int64_t)blockIdx.x * rpb + g;
  const int col = (blockIdx.y * lpr + sub) * VEC;
  if (r >= n || col >= f) return;
  const float scale = 1.0f + (eps ? eps[0] : 0.f);
  const int b = rowptr_t[r], en = rowptr_t[r + 1];
  GineEdgeW<VEC, DM> ew;
  ew.load(w_e, b_e, d_n, f, col);
  GineVec<VEC> xj, own, acc;
  xj.load(x + r * ldx + col);
  own.load(dt + r * lddt + col);
  acc.zero();
  auto add = [&](const GineVec<VEC>& h, const float (&ev)[DM]) {
#pragma unroll
    for (int c = 0; c < VEC; ++c) {
      const float m = gine_msg<DM>(ev, ew.w[c], ew.b[c], ew.has_b, d_n, xj.v[c]);
      acc.v[c] += m > 0.f ? h.v[c] : 0.f;
    }
  };
  int q0 = b;
  for (; q0 + kEU <= en; q0 += kEU) {           // the transposed pattern's stored order
    GineVec<VEC> h[kEU];
    float ev[kEU][DM];
#pragma unroll
    for (int q = 0; q < kEU; ++q) {
      h[q].load(dt + (int64_t)colidx_t[q0 + q] * lddt + col);
      gine_load_e<DM>(ev[q], e + (int64_t)perm_t[q0 + q] * lde, d_n);
    }
#pragma unroll
    for (int q = 0; q < kEU; ++q) add(h[q], ev[q]);
  }
  for (; q0 < en; ++q0) {
    GineVec<VEC> h;
    float ev[DM];
    h.load(dt + (int64_t)colidx_t[q0] * lddt + col);
    gine_load_e<DM>(ev, e + (int64_t)perm_t[q0] * lde, d_n);
    add(h, ev);
  }
#pragma unroll
  for (int c = 0; c < VEC; ++c) acc.v[c] = fmaf(scale, own.v[c], acc.v[c]);
  acc.store(dx + r * lddx + col);
}

// A launch of an any-width kernel on its (lanes, slots) instance: float4 or scalar lanes, 2 or 8 feature slots.
#define GINE_LAUNCH(KERNEL, vec, d_n, ...)                                                    \
  do {                                                                                        \
    if (vec) {                                                                                \
      if ((d_n) <= 2) hipLaunchKernelGGL((KERNEL<4, 2>), __VA_ARGS__);                        \
      else hipLaunchKernelGGL((KERNEL<4, kEdgeMax>), __VA_ARGS__);                            \
    } else {                                                                                  \
      if ((d_n) <= 2) hipLaunchKernelGGL((KERNEL<1, 2>), __VA_ARGS__);                        \
      else hipLaunchKernelGGL((KERNEL<1, kEdgeMax>), __VA_ARGS__);                            \
    }                                                                                         \
  } while (0)

// Lanes per row of the any-width kernels: the power of two that covers the row's units (float4 or float), 64 at the most.
struct GineLanes { int lpr_log2, rpb, ny; };
GineLanes gine_lanes(int units) {
  int l = 0;
  while ((1 << l) < units && l < 6) ++l;
  return GineLanes{l, 256 >> l, gcnx_cdiv(units, 1 << l)};
}

}  // namespace

extern "C" {

int gcnx_gine_conv_ok(int64_t n, int32_t k0, int32_t k1, int32_t k2, int64_t ldx, int32_t edge_dim) {
  return gine_shape_ok(n, k0, k1, k2, ldx, edge_dim) ? 1 : 0;
}

int gcnx_gine_conv(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* x, int64_t ldx, int32_t n, int32_t k0,
                   const float* eps, const float* e, int64_t lde, int32_t edge_dim, const float* w_e, const float* b_e,
                   const float* w_a, const float* b_a, int32_t k1, const float* w_b, const float* b_b, int32_t k2, float* t,
                   int64_t ldt, float* u, int64_t ldu, float* out, int64_t ldo) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "GINEConv (one launch)");
  GCNX_REQUIRE(ctx, n >= 0 && k0 >= 0 && k1 >= 0 && k2 >= 0 && edge_dim >= 0, "gcnx_gine_conv: negative size");
  if (!gine_shape_ok(n, k0, k1, k2, ldx, edge_dim))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_gine_conv: needs k0 in {16, 32, 64, 128}, k1 and k2 multiples of 16 up to 128, "
                     "ldx >= k0 in multiples of 4 floats, n * ldx * 4 < 2^32 and 1 <= edge_dim <= 8 (got n=%d k0=%d k1=%d k2=%d "
                     "ldx=%lld edge_dim=%d): use gcnx_gine_aggregate + gcnx_gemm", n, k0, k1, k2, (long long)ldx, edge_dim);
  if (!gcnx_aligned16(x) || !gcnx_aligned16(w_e) || !gcnx_aligned16(b_e) || !gcnx_aligned16(w_a) || !gcnx_aligned16(w_b) ||
      !gcnx_aligned16(out) || ldo < k2 || ldo % 4 != 0 || (t && (!gcnx_aligned16(t) || ldt < k0 || ldt % 4 != 0)) ||
      (u && (!gcnx_aligned16(u) || ldu < k1 || ldu % 4 != 0)))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_gine_conv: x, w_e, b_e, w_a, w_b, t, u and out must be 16-byte aligned, with "
                     "ldt >= k0, ldu >= k1 and ldo >= k2 in multiples of 4 floats");
  GCNX_REQUIRE(ctx, lde >= edge_dim, "gcnx_gine_conv: lde=%lld < edge_dim=%d", (long long)lde, edge_dim);
  if (n == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, rowptr && colidx && x && e && w_e && w_a && w_b && out, "gcnx_gine_conv: NULL pointer");
  GCNX_REQUIRE(ctx, x != out && x != t && x != u && (!t || (t != out && t != u)) && (!u || u != out),
               "gcnx_gine_conv: the outputs must not alias x or each other");
  GineArgs a{};
  a.rowptr = rowptr; a.colidx = colidx; a.x = x; a.ldx = ldx; a.n = n; a.eps = eps; a.e = e; a.lde = lde; a.edge_dim = edge_dim;
  a.w_e = w_e; a.b_e = b_e; a.w_a = w_a; a.b_a = b_a; a.k1 = k1; a.w_b = w_b; a.b_b = b_b; a.k2 = k2;
  a.t = t; a.ldt = ldt; a.u = u; a.ldu = ldu; a.out = out; a.ldo = ldo;
  return edge_dim <= 2 ? launch_gine<2>(ctx, a, k0) : launch_gine<kEdgeMax>(ctx, a, k0);
}

int gcnx_gine_aggregate(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* x, int64_t ldx, const float* eps,
                        const float* e, int64_t lde, int32_t edge_dim, const float* w_e, const float* b_e, float* out, int64_t ldo,
                        int32_t n, int32_t f) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "GINEConv aggregate");
  GCNX_REQUIRE(ctx, n >= 0 && f >= 1 && ldx >= f && ldo >= f && gine_dim_ok(edge_dim) && lde >= edge_dim,
               "gcnx_gine_aggregate: needs n >= 0, f >= 1, ldx >= f, ldo >= f, 1 <= edge_dim <= 8 and lde >= edge_dim");
  if (n == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, rowptr && colidx && x && e && w_e && out, "gcnx_gine_aggregate: NULL pointer");
  GCNX_REQUIRE(ctx, x != out, "gcnx_gine_aggregate: out must not alias x");
  const bool vec = f % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && gcnx_aligned16(x) && gcnx_aligned16(out) && gcnx_aligned16(w_e) &&
                   gcnx_aligned16(b_e);
  const GineLanes l = gine_lanes(vec ? f / 4 : f);
  GCNX_REQUIRE(ctx, l.ny <= 65535, "gcnx_gine_aggregate: f=%d is too wide", f);
  const dim3 grid(gcnx_cdiv(n, l.rpb), l.ny);
  GINE_LAUNCH(gine_aggregate_kernel, vec, edge_dim, grid, dim3(256), 0, ctx->stream, rowptr, colidx, x, ldx, eps, e, lde, edge_dim, w_e,
              b_e, out, ldo, n, f, l.lpr_log2);
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

int64_t gcnx_gine_bwd_scratch_floats(int64_t n, int32_t k0, int32_t edge_dim) {
  if (n < 0 || k0 < 1 || !gine_dim_ok(edge_dim)) return 0;
  return ((n + kEdgeRows - 1) / kEdgeRows) * (int64_t)(edge_dim + 1) * k0;
}

int gcnx_gine_bwd_edges(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* x, int64_t ldx, const float* e,
                        int64_t lde, int32_t edge_dim, const float* w_e, const float* b_e, const float* dt, int64_t lddt, int32_t n,
                        int32_t f, float* dw_e, float* db_e, float* scratch) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "GINEConv backward (edges)");
  GCNX_REQUIRE(ctx, n >= 0 && f >= 1 && ldx >= f && lddt >= f && gine_dim_ok(edge_dim) && lde >= edge_dim,
               "gcnx_gine_bwd_edges: needs n >= 0, f >= 1, ldx >= f, lddt >= f, 1 <= edge_dim <= 8 and lde >= edge_dim");
  GCNX_REQUIRE(ctx, dw_e && (n == 0 || (rowptr && colidx && x && e && w_e && dt && scratch)), "gcnx_gine_bwd_edges: NULL pointer");
  const int64_t nparts = ((int64_t)n + kEdgeRows - 1) / kEdgeRows;
  if (nparts > 0) {
    const bool vec = f % 4 == 0 && ldx % 4 == 0 && lddt % 4 == 0 && gcnx_aligned16(x) && gcnx_aligned16(dt) && gcnx_aligned16(w_e) &&
                     gcnx_aligned16(b_e) && gcnx_aligned16(scratch);
    const GineLanes l = gine_lanes(vec ? f / 4 : f);
    GCNX_REQUIRE(ctx, l.ny <= 65535, "gcnx_gine_bwd_edges: f=%d is too wide", f);
    const dim3 grid((unsigned)nparts, l.ny);
    GINE_LAUNCH(gine_bwd_edges_kernel, vec, edge_dim, grid, dim3(256), 0, ctx->stream, rowptr, colidx, x, ldx, e, lde, edge_dim, w_e,
                b_e, dt, lddt, n, f, scratch, l.lpr_log2);
    GCNX_LAUNCH_OK(ctx);
  }
  hipLaunchKernelGGL(gine_bwd_edges_final_kernel, dim3(gcnx_cdiv((int64_t)(edge_dim + 1) * f, 16)), dim3(256), 0, ctx->stream,
                     (const float*)scratch, nparts, edge_dim, f, dw_e, db_e);
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

int gcnx_gine_bwd_nodes(gcnx_ctx* ctx, const int32_t* rowptr_t, const int32_t* colidx_t, const int32_t* perm_t, const float* x,
                        int64_t ldx, const float* eps, const float* e, int64_t lde, int32_t edge_dim, const float* w_e,
                        const float* b_e, const float* dt, int64_t lddt, float* dx, int64_t lddx, int32_t n, int32_t f) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "GINEConv backward (nodes)");
  GCNX_REQUIRE(ctx, n >= 0 && f >= 1 && ldx >= f && lddt >= f && lddx >= f && gine_dim_ok(edge_dim) && lde >= edge_dim,
               "gcnx_gine_bwd_nodes: needs n >= 0, f >= 1, ldx >= f, lddt >= f, lddx >= f, 1 <= edge_dim <= 8 and lde >= edge_dim");
  if (n == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, rowptr_t && colidx_t && perm_t && x && e && w_e && dt && dx, "gcnx_gine_bwd_nodes: NULL pointer");
  GCNX_REQUIRE(ctx, dx != dt && dx != x, "gcnx_gine_bwd_nodes: dx must not alias dt or x");
  const bool vec = f % 4 == 0 && ldx % 4 == 0 && lddt % 4 == 0 && lddx % 4 == 0 && gcnx_aligned16(x) && gcnx_aligned16(dt) &&
                   gcnx_aligned16(dx) && gcnx_aligned16(w_e) && gcnx_aligned16(b_e);
  const GineLanes l = gine_lanes(vec ? f / 4 : f);
  GCNX_REQUIRE(ctx, l.ny <= 65535, "gcnx_gine_bwd_nodes: f=%d is too wide", f);
  const dim3 grid(gcnx_cdiv(n, l.rpb), l.ny);
  GINE_LAUNCH(gine_bwd_nodes_kernel, vec, edge_dim, grid, dim3(256), 0, ctx->stream, rowptr_t, colidx_t, perm_t, x, ldx, eps, e, lde,
              edge_dim, w_e, b_e, dt, lddt, dx, lddx, n, f, l.lpr_log2);
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

}  // extern "C"
