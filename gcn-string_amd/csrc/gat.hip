// GATConv (PyG's GATConv(heads = H, concat = True), one weight for sources and targets) in the small-feature regime
// (H C <= 128): the attention layer that drops into the slot the reference's author marked as open ("consider using class
// SAGEConv instead", gcn_utills.py:804-806).  Row i of the CSR is the target, its stored entries j the sources, values ignored:
//
//     Hf = x W  (gcnx_gemm)      a_src[j,h] = <Hf[j,h,:], att_src[h,:]>      a_dst[i,h] = <Hf[i,h,:], att_dst[h,:]>     gat_scores
//     z = a_src[j,h] + a_dst[i,h]   e = z > 0 ? z : slope z   alpha = exp(e - m_i) / l_i   O[i,h,:] = sum_j alpha Hf[j,h,:]   gat_aggregate
//     r = <dO, O>   dz = alpha (<dO[i,h,:], Hf[j,h,:]> - r) (z > 0 ? 1 : slope)   da_dst[i,h] = sum_j dz                 gat_bwd_edges
//     dHf[j] = sum_i alpha dO[i] + da_src[j] att_src + da_dst[j] att_dst   da_src[j,h] = sum_i dz   datt_* = sum_j da_* Hf[j]   gat_bwd_nodes
//
// The softmax runs over the stored entries of a row with scores that depend on both endpoints, so no existing aggregation
// (fixed coefficients) composes it.  fp32 throughout, no float atomics, every sum in a fixed order: the same call leaves the
// same bits, eagerly and replayed from a captured graph.
//
// Shape of a workgroup (sage.hip's; the device helpers they share: conv_tile.h): 32 rows, one lane group of HC / 4 lanes per
// row with one float4 of the row each -- 8 HC threads.  Head h owns the c / 4 consecutive lanes [h c / 4, (h + 1) c / 4) of a group, always
// inside one wave: per-head dot products, maxima and sums are xor butterflies over those lanes (every lane ends with the same
// bits), no LDS round trip.  The tile's CSR entries are staged in LDS (1024 of them; a tile with more -- the hub rows of a
// power-law graph -- reads the rest from global memory, entry by entry, in every pass).  Feature rows are gathered with
// range-checked buffer loads, four entries per trip, slots past a row's end fetch nothing.  One lane group accumulates a
// row in CSR order from +0.
#include <cmath>

#include "common.h"
#include "conv_tile.h"

namespace {

// over the lph (a power of two) consecutive lanes of a head: every lane gets the same bits
__device__ __forceinline__ float head_sum(float v, int lph) {
  for (int off = lph >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ float head_max(float v, int lph) {
  for (int off = lph >> 1; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}
// the score of one entry: ONE fp32 add of the stored halves, positive side z > 0 (the backward decides the side the same way)
__device__ __forceinline__ float gscore(float asrc, float adst, float slope) {
  const float z = asrc + adst;
  return z > 0.f ? z : slope * z;
}

// ---- a_src, a_dst: one pass over Hf ------------------------------------------------------------------------------------
template <int HC>
__global__ __launch_bounds__(256) void gat_scores_kernel(const float* __restrict__ hf, int64_t ldh, int32_t n, int32_t heads, int32_t lph,
                                                         const float* __restrict__ att_src, const float* __restrict__ att_dst,
                                                         float* __restrict__ a_src, float* __restrict__ a_dst) {
  constexpr int LPR = HC / 4, RPB = 256 / LPR;
  const int tid = threadIdx.x, sub = tid % LPR;
  const int64_t row = (int64_t)blockIdx.x * RPB + tid / LPR;
  const bool live = row < n;
  float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) h = load4(hf + row * ldh + 4 * sub);
  const float s = head_sum(dot4(h, load4(att_src + 4 * sub)), lph);
  const float d = head_sum(dot4(h, load4(att_dst + 4 * sub)), lph);
  if (live && sub % lph == 0) {
    a_src[row * heads + sub / lph] = s;
    a_dst[row * heads + sub / lph] = d;
  }
}

struct GatFwdArgs {
  const int32_t* rowptr; const int32_t* colidx;
  const float* hf; int64_t ldh;
  int32_t n, heads, lph;
  const float* a_src; const float* a_dst; const float* bias;
  float slope;
  float* out; int64_t ldo;
  float* alpha;                     // [nnz, heads] or NULL
  float* o_pre; int64_t ldp;        // O before the bias, or NULL
};

// ---- softmax over the row's entries + weighted gather -------------------------------------------------------------------
// dynamic LDS: kTileCap * heads floats, the staged entries' scores e, then their weights exp(e - m)
template <int HC>
__global__ __launch_bounds__(8 * HC) void gat_aggregate_kernel(GatFwdArgs p) {
  constexpr int LPR = HC / 4, NT = 8 * HC;
  extern __shared__ float s_w[];
  __shared__ int32_t s_col[kTileCap];
  __shared__ int32_t s_rp[kTileRows + 1];
  const int tid = threadIdx.x, r = tid / LPR, sub = tid % LPR;
  const int heads = p.heads, lph = p.lph, h = sub / lph, k = sub % lph;
  const ConvTile t = conv_tile(p.rowptr, p.n, s_rp, kTileRows);
  const int staged = min(t.e1 - t.e0, kTileCap);
  for (int i = tid; i < staged; i += NT) s_col[i] = p.colidx[t.e0 + i];
  __syncthreads();
  const bool live = r < t.nr;
  const int ea = live ? s_rp[r] - t.e0 : 0, eb = live ? s_rp[r + 1] - t.e0 : 0;
  const float adst = live ? p.a_dst[(int64_t)(t.r0 + r) * heads + h] : 0.f;
  const float slope = p.slope;
  const int32_t* __restrict__ gcol = p.colidx + t.e0;
  // pass 1: the row maximum of e; lane k of the head takes entries k, k + lph, ...
  float m = -INFINITY;
  for (int e = ea + k; e < eb; e += lph) {
    const bool st = e < kTileCap;
    const int col = st ? s_col[e] : gcol[e];
    const float ev = gscore(p.a_src[(int64_t)col * heads + h], adst, slope);
    if (st) s_w[e * heads + h] = ev;
    m = fmaxf(m, ev);
  }
  m = head_max(m, lph);
  // pass 2: the weights exp(e - m) <= 1 and their sum l >= 1 (the maximum's own weight is 1: no overflow, no 0 / 0)
  float l = 0.f;
  for (int e = ea + k; e < eb; e += lph) {
    const bool st = e < kTileCap;
    const float ev = st ? s_w[e * heads + h] : gscore(p.a_src[(int64_t)gcol[e] * heads + h], adst, slope);
    const float w = expf(ev - m);
    if (st) s_w[e * heads + h] = w;
    l += w;
  }
  l = head_sum(l, lph);
  const float inv = eb > ea ? 1.0f / l : 0.f;
  if (p.alpha) {
    float* __restrict__ al = p.alpha + (int64_t)t.e0 * heads + h;
    for (int e = ea + k; e < eb; e += lph) {
      const float w = e < kTileCap ? s_w[e * heads + h] : expf(gscore(p.a_src[(int64_t)gcol[e] * heads + h], adst, slope) - m);
      al[(int64_t)e * heads] = w * inv;
    }
  }
  __syncthreads();
  // gather: sum_j w_j Hf[j, 4 sub .. 4 sub + 3] in CSR order
  const unsigned ld4 = (unsigned)p.ldh * 4u, sub16 = (unsigned)sub * 16u;
  // the descriptor ends behind the last row's HC columns (a column slice of a wider array: nothing past them is addressed)
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.hf, (short)0, (int)((unsigned)(p.n - 1) * ld4 + (unsigned)HC * 4u), 0x00020000);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  const int eaf = min(ea, kTileCap), ebf = min(eb, kTileCap);
  for (int e = eaf; e < ebf; e += kTileU) {
    float4 hv[kTileU];
    float wv[kTileU];
#pragma unroll
    for (int u = 0; u < kTileU; ++u) {
      const bool ok = e + u < ebf;
      const int ee = ok ? e + u : e;
      wv[u] = ok ? s_w[ee * heads + h] : 0.f;
      hv[u] = buf4(xr, ok ? (unsigned)s_col[ee] * ld4 + sub16 : kOffOut);
    }
#pragma unroll
    for (int u = 0; u < kTileU; ++u) acc = fma4(wv[u], hv[u], acc);
  }
  for (int e = max(ea, kTileCap); e < eb; ++e) {      // rare: entries beyond the staged ones
    const int col = gcol[e];
    const float w = expf(gscore(p.a_src[(int64_t)col * heads + h], adst, slope) - m);
    acc = fma4(w, buf4(xr, (unsigned)col * ld4 + sub16), acc);
  }
  if (!live) return;
  const float4 o = make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv);     // a row without entries: exact zeros
  const int64_t row = t.r0 + r;
  if (p.o_pre) *reinterpret_cast<float4*>(p.o_pre + row * p.ldp + 4 * sub) = o;
  float4 y = o;
  if (p.bias) {
    const float4 b = load4(p.bias + 4 * sub);
    y = eb > ea ? make_float4(o.x + b.x, o.y + b.y, o.z + b.z, o.w + b.w) : b;          // (no entries: the bias, bit for bit)
  }
  *reinterpret_cast<float4*>(p.out + row * p.ldo + 4 * sub) = y;
}

struct GatEdgeArgs {
  const int32_t* rowptr; const int32_t* colidx;
  const float* hf; int64_t ldh;
  int32_t n, heads, lph;
  const float* a_src; const float* a_dst;
  float slope;
  const float* alpha;
  const float* d_out; int64_t ldd;
  const float* o; int64_t ldo; const float* o_bias;     // O = o - o_bias (o_bias NULL: o is O)
  float* dz; float* da_dst;
};

// ---- backward on the forward CSR: dz per entry, da_dst per target row ------------------------------------------------------
template <int HC>
__global__ __launch_bounds__(8 * HC) void gat_bwd_edges_kernel(GatEdgeArgs p) {
  constexpr int LPR = HC / 4, NT = 8 * HC;
  __shared__ int32_t s_col[kTileCap];
  __shared__ int32_t s_rp[kTileRows + 1];
  const int tid = threadIdx.x, r = tid / LPR, sub = tid % LPR;
  const int heads = p.heads, lph = p.lph, h = sub / lph, k = sub % lph;
  const ConvTile t = conv_tile(p.rowptr, p.n, s_rp, kTileRows);
  const int staged = min(t.e1 - t.e0, kTileCap);
  for (int i = tid; i < staged; i += NT) s_col[i] = p.colidx[t.e0 + i];
  __syncthreads();
  const bool live = r < t.nr;
  const int ea = live ? s_rp[r] - t.e0 : 0, eb = live ? s_rp[r + 1] - t.e0 : 0;
  const int64_t row = t.r0 + r;
  float4 dO = make_float4(0.f, 0.f, 0.f, 0.f), O = dO;
  float adst = 0.f;
  if (live) {
    dO = load4(p.d_out + row * p.ldd + 4 * sub);
    O = load4(p.o + row * p.ldo + 4 * sub);
    if (p.o_bias) {
      const float4 b = load4(p.o_bias + 4 * sub);
      O = make_float4(O.x - b.x, O.y - b.y, O.z - b.z, O.w - b.w);
    }
    adst = p.a_dst[row * heads + h];
  }
  const float rr = head_sum(dot4(dO, O), lph);          // = sum_k alpha_ik dalpha_ik: no second pass over the row
  const unsigned ld4 = (unsigned)p.ldh * 4u, sub16 = (unsigned)sub * 16u;
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.hf, (short)0, (int)((unsigned)(p.n - 1) * ld4 + (unsigned)HC * 4u), 0x00020000);
  const int32_t* __restrict__ gcol = p.colidx + t.e0;
  const float* __restrict__ al = p.alpha + (int64_t)t.e0 * heads + h;
  float* __restrict__ dzo = p.dz + (int64_t)t.e0 * heads + h;
  const float slope = p.slope;
  float dsum = 0.f;
  for (int e = ea; e < eb; e += kTileU) {                   // (the lanes of a row share ea and eb: they shuffle together)
    float4 hv[kTileU];
    float as[kTileU], av[kTileU];
#pragma unroll
    for (int u = 0; u < kTileU; ++u) {
      const bool ok = e + u < eb;
      const int ee = ok ? e + u : e;
      const int col = ee < kTileCap ? s_col[ee] : gcol[ee];
      hv[u] = buf4(xr, ok ? (unsigned)col * ld4 + sub16 : kOffOut);
      as[u] = p.a_src[(int64_t)col * heads + h];
      av[u] = al[(int64_t)ee * heads];
    }
#pragma unroll
    for (int u = 0; u < kTileU; ++u) {
      const float d = head_sum(dot4(dO, hv[u]), lph);
      if (e + u < eb) {
        const float z = as[u] + adst;
        const float g = av[u] * (d - rr) * (z > 0.f ? 1.0f : slope);
        dsum += g;                                       // CSR order
        if (k == 0) dzo[(int64_t)(e + u) * heads] = g;
      }
    }
  }
  if (live && k == 0) p.da_dst[row * heads + h] = dsum;
}

struct GatNodeArgs {
  const int32_t* rowptr; const int32_t* colidx; const int32_t* perm;     // the transposed pattern and its entry permutation
  int32_t n, heads, lph;
  const float* alpha; const float* dz;                                   // [nnz, heads], forward entry order
  const float* d_out; int64_t ldd;
  const float* hf; int64_t ldh;
  const float* da_dst; const float* att_src; const float* att_dst;
  float* dhf; int64_t ldg;
  float* da_src;
  float* part;                                                           // [tiles][2 HC]: this tile's datt_src | datt_dst
};

// ---- backward on the transposed pattern: dHf and da_src per source row, the tile's part of datt_src / datt_dst --------------
template <int HC>
__global__ __launch_bounds__(8 * HC) void gat_bwd_nodes_kernel(GatNodeArgs p) {
  constexpr int LPR = HC / 4, NT = 8 * HC;
  __shared__ int32_t s_col[kTileCap];
  __shared__ int32_t s_q[kTileCap];
  __shared__ int32_t s_rp[kTileRows + 1];
  __shared__ __attribute__((aligned(16))) float4 s_p[2][kTileRows][LPR];
  const int tid = threadIdx.x, r = tid / LPR, sub = tid % LPR;
  const int heads = p.heads, lph = p.lph, h = sub / lph, k = sub % lph;
  const ConvTile t = conv_tile(p.rowptr, p.n, s_rp, kTileRows);
  const int staged = min(t.e1 - t.e0, kTileCap);
  for (int i = tid; i < staged; i += NT) {
    s_col[i] = p.colidx[t.e0 + i];
    s_q[i] = p.perm[t.e0 + i];
  }
  __syncthreads();
  const bool live = r < t.nr;
  const int ea = live ? s_rp[r] - t.e0 : 0, eb = live ? s_rp[r + 1] - t.e0 : 0;
  const int64_t row = t.r0 + r;
  const unsigned ld4 = (unsigned)p.ldd * 4u, sub16 = (unsigned)sub * 16u;
  const __amdgpu_buffer_rsrc_t dr = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.d_out, (short)0, (int)((unsigned)(p.n - 1) * ld4 + (unsigned)HC * 4u), 0x00020000);
  const int32_t* __restrict__ gcol = p.colidx + t.e0;
  const int32_t* __restrict__ gq = p.perm + t.e0;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  float dsrc = 0.f;
  for (int e = ea; e < eb; e += kTileU) {
    float4 hv[kTileU];
    float av[kTileU], zv[kTileU];
#pragma unroll
    for (int u = 0; u < kTileU; ++u) {
      const bool ok = e + u < eb;
      const int ee = ok ? e + u : e;
      const bool st = ee < kTileCap;
      const int col = st ? s_col[ee] : gcol[ee];
      const int64_t q = (int64_t)(st ? s_q[ee] : gq[ee]) * heads + h;
      hv[u] = buf4(dr, ok ? (unsigned)col * ld4 + sub16 : kOffOut);
      av[u] = ok ? p.alpha[q] : 0.f;
      zv[u] = ok ? p.dz[q] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kTileU; ++u) {
      acc = fma4(av[u], hv[u], acc);
      dsrc += zv[u];                                     // the transposed CSR's order
    }
  }
  float ddst = 0.f;
  float4 own = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) {
    ddst = p.da_dst[row * heads + h];
    own = load4(p.hf + row * p.ldh + 4 * sub);
    acc = fma4(dsrc, load4(p.att_src + 4 * sub), acc);
    acc = fma4(ddst, load4(p.att_dst + 4 * sub), acc);
    *reinterpret_cast<float4*>(p.dhf + row * p.ldg + 4 * sub) = acc;
    if (k == 0) p.da_src[row * heads + h] = dsrc;
  }
  // datt_src[h, :] = sum_j da_src[j, h] Hf[j, h, :] (datt_dst likewise): this tile's 32 rows, in row order
  s_p[0][r][sub] = make_float4(dsrc * own.x, dsrc * own.y, dsrc * own.z, dsrc * own.w);
  s_p[1][r][sub] = make_float4(ddst * own.x, ddst * own.y, ddst * own.z, ddst * own.w);
  __syncthreads();
  if (tid < 2 * LPR) {
    const int which = tid / LPR, c4 = tid % LPR;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
    for (int i = 0; i < kTileRows; ++i) {
      const float4 v = s_p[which][i][c4];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    *reinterpret_cast<float4*>(p.part + ((int64_t)(t.r0 / kTileRows) * 2 + which) * HC + 4 * c4) = s;
  }
}

// the tiles' parts summed in a fixed order (gcnx_colpart_reduce_sum): columns [0, hc) are datt_src, [hc, 2 hc) datt_dst
__global__ __launch_bounds__(256) void gat_datt_reduce_kernel(const float* __restrict__ part, int64_t tiles, int32_t hc,
                                                              float* __restrict__ datt_src, float* __restrict__ datt_dst) {
  __shared__ float4 s[128][2];
  const float4 v = gcnx_colpart_reduce_sum(part, tiles, 2 * hc, blockIdx.x, s);
  const int c = blockIdx.x * 8 + (threadIdx.x & 1) * 4;
  if ((threadIdx.x >> 1) == 0 && c < 2 * hc) *reinterpret_cast<float4*>(c < hc ? datt_src + c : datt_dst + (c - hc)) = v;
}

bool gat_shape_ok(int64_t n, int32_t heads, int32_t c, int64_t ldh) {
  if (n < 0 || !(heads == 1 || heads == 2 || heads == 4 || heads == 8) || c < 4 || c > 128) return false;
  const int hc = heads * c;
  return (hc == 16 || hc == 32 || hc == 64 || hc == 128) && ldh >= hc && ldh % 4 == 0 &&
         (uint64_t)n * (uint64_t)ldh * 4u < 0x100000000ull;
}
bool gat_ld_ok(int64_t ld, int hc) { return ld >= hc && ld % 4 == 0; }     // (conv_ld_ok without its 2^30 bound: what this ABI accepts)

const char* kGatShapes = "needs heads in {1, 2, 4, 8}, heads * c in {16, 32, 64, 128}, c >= 4, ld >= heads * c in multiples of 4 "
                         "floats and n * ld * 4 < 2^32";

#define GCNX_GAT_DISPATCH(hc, LAUNCH) \
  do { if ((hc) == 128) { LAUNCH(128); } else if ((hc) == 64) { LAUNCH(64); } else if ((hc) == 32) { LAUNCH(32); } else { LAUNCH(16); } } while (0)

}  // namespace

extern "C" {

int gcnx_gat_conv_ok(int64_t n, int32_t heads, int32_t c, int64_t ldh) { return gat_shape_ok(n, heads, c, ldh) ? 1 : 0; }

int64_t gcnx_gat_bwd_scratch_floats(int64_t n, int32_t heads, int32_t c) {
  if (n < 0 || heads < 0 || c < 0) return 0;
  return (int64_t)gcnx_cdiv(n, kTileRows) * 2 * heads * c;
}

int gcnx_gat_scores(gcnx_ctx* ctx, const float* hf, int64_t ldh, int32_t n, int32_t heads, int32_t c, const float* att_src,
                    const float* att_dst, float* a_src, float* a_dst) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "GATConv scores");
  GCNX_REQUIRE(ctx, n >= 0 && heads >= 0 && c >= 0, "gcnx_gat_scores: negative size");
  if (!gat_shape_ok(n, heads, c, ldh))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_gat_scores: %s (got n=%d heads=%d c=%d ld=%lld)", kGatShapes, n, heads, c, (long long)ldh);
  if (!gcnx_aligned16(hf) || !gcnx_aligned16(att_src) || !gcnx_aligned16(att_dst))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_gat_scores: hf, att_src and att_dst must be 16-byte aligned");
  if (n == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, hf && att_src && att_dst && a_src && a_dst, "gcnx_gat_scores: NULL pointer");
  const int hc = heads * c, lph = c / 4;
#define GCNX_GAT_SCORES(HC_) \
  hipLaunchKernelGGL((gat_scores_kernel<HC_>), dim3(gcnx_cdiv(n, 1024 / HC_)), dim3(256), 0, ctx->stream, hf, ldh, n, heads, lph, \
                     att_src, att_dst, a_src, a_dst)
  GCNX_GAT_DISPATCH(hc, GCNX_GAT_SCORES);
#undef GCNX_GAT_SCORES
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

int gcnx_gat_aggregate(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* hf, int64_t ldh, int32_t n,
                       int32_t heads, int32_t c, const float* a_src, const float* a_dst, const float* bias, float slope, float* out,
                       int64_t ldo, float* alpha, float* o_pre, int64_t ldp) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "GATConv aggregate");
  GCNX_REQUIRE(ctx, n >= 0 && heads >= 0 && c >= 0, "gcnx_gat_aggregate: negative size");
  if (!gat_shape_ok(n, heads, c, ldh))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_gat_aggregate: %s (got n=%d heads=%d c=%d ld=%lld)", kGatShapes, n, heads, c, (long long)ldh);
  const int hc = heads * c;
  if (!gcnx_aligned16(hf) || !gcnx_aligned16(bias) || !gcnx_aligned16(out) || !gat_ld_ok(ldo, hc) ||
      (o_pre && (!gcnx_aligned16(o_pre) || !gat_ld_ok(ldp, hc))))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_gat_aggregate: hf, bias, out and o_pre must be 16-byte aligned, with ldo and ldp "
                     ">= heads * c in multiples of 4 floats");
  if (n == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, rowptr && colidx && hf && a_src && a_dst && out, "gcnx_gat_aggregate: NULL pointer");
  GCNX_REQUIRE(ctx, hf != out && hf != o_pre && out != o_pre, "gcnx_gat_aggregate: the outputs must not alias hf or each other");
  GatFwdArgs a{};
  a.rowptr = rowptr; a.colidx = colidx; a.hf = hf; a.ldh = ldh; a.n = n; a.heads = heads; a.lph = c / 4; a.a_src = a_src; a.a_dst = a_dst;
  a.bias = bias; a.slope = slope; a.out = out; a.ldo = ldo; a.alpha = alpha; a.o_pre = o_pre; a.ldp = ldp;
  const int tiles = gcnx_cdiv(n, kTileRows);
  const size_t dyn = (size_t)kTileCap * heads * sizeof(float);
#define GCNX_GAT_AGG(HC_) hipLaunchKernelGGL((gat_aggregate_kernel<HC_>), dim3(tiles), dim3(8 * HC_), dyn, ctx->stream, a)
  GCNX_GAT_DISPATCH(hc, GCNX_GAT_AGG);
#undef GCNX_GAT_AGG
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

int gcnx_gat_bwd_edges(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* hf, int64_t ldh, int32_t n,
                       int32_t heads, int32_t c, const float* a_src, const float* a_dst, float slope, const float* alpha,
                       const float* d_out, int64_t ldd, const float* o, int64_t ldo, const float* o_bias, float* dz, float* da_dst) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "GATConv backward (edges)");
  GCNX_REQUIRE(ctx, n >= 0 && heads >= 0 && c >= 0, "gcnx_gat_bwd_edges: negative size");
  if (!gat_shape_ok(n, heads, c, ldh))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_gat_bwd_edges: %s (got n=%d heads=%d c=%d ld=%lld)", kGatShapes, n, heads, c, (long long)ldh);
  const int hc = heads * c;
  if (!gcnx_aligned16(hf) || !gcnx_aligned16(d_out) || !gcnx_aligned16(o) || !gcnx_aligned16(o_bias) || !gat_ld_ok(ldd, hc) ||
      !gat_ld_ok(ldo, hc))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_gat_bwd_edges: hf, d_out, o and o_bias must be 16-byte aligned, with ldd and ldo "
                     ">= heads * c in multiples of 4 floats");
  if (n == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, rowptr && colidx && hf && a_src && a_dst && alpha && d_out && o && dz && da_dst, "gcnx_gat_bwd_edges: NULL pointer");
  GatEdgeArgs a{};
  a.rowptr = rowptr; a.colidx = colidx; a.hf = hf; a.ldh = ldh; a.n = n; a.heads = heads; a.lph = c / 4; a.a_src = a_src; a.a_dst = a_dst;
  a.slope = slope; a.alpha = alpha; a.d_out = d_out; a.ldd = ldd; a.o = o; a.ldo = ldo; a.o_bias = o_bias; a.dz = dz; a.da_dst = da_dst;
  const int tiles = gcnx_cdiv(n, kTileRows);
#define GCNX_GAT_BE(HC_) hipLaunchKernelGGL((gat_bwd_edges_kernel<HC_>), dim3(tiles), dim3(8 * HC_), 0, ctx->stream, a)
  GCNX_GAT_DISPATCH(hc, GCNX_GAT_BE);
#undef GCNX_GAT_BE
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

int gcnx_gat_bwd_nodes(gcnx_ctx* ctx, const int32_t* rowptr_t, const int32_t* colidx_t, const int32_t* perm_t, int32_t n, int32_t heads,
                       int32_t c, const float* alpha, const float* dz, const float* d_out, int64_t ldd, const float* hf, int64_t ldh,
                       const float* da_dst, const float* att_src, const float* att_dst, float* dhf, int64_t ldg, float* da_src,
                       float* datt_src, float* datt_dst, float* scratch) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "GATConv backward (nodes)");
  GCNX_REQUIRE(ctx, n >= 0 && heads >= 0 && c >= 0, "gcnx_gat_bwd_nodes: negative size");
  if (!gat_shape_ok(n, heads, c, ldd))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_gat_bwd_nodes: %s (got n=%d heads=%d c=%d ld=%lld)", kGatShapes, n, heads, c, (long long)ldd);
  const int hc = heads * c;
  if (!gcnx_aligned16(d_out) || !gcnx_aligned16(hf) || !gcnx_aligned16(att_src) || !gcnx_aligned16(att_dst) || !gcnx_aligned16(dhf) ||
      !gcnx_aligned16(datt_src) || !gcnx_aligned16(datt_dst) || !gcnx_aligned16(scratch) || !gat_ld_ok(ldh, hc) || !gat_ld_ok(ldg, hc))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_gat_bwd_nodes: d_out, hf, att_src, att_dst, dhf, datt_src, datt_dst and scratch must be "
                     "16-byte aligned, with ldh and ldg >= heads * c in multiples of 4 floats");
  if (n == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, rowptr_t && colidx_t && perm_t && alpha && dz && d_out && hf && da_dst && att_src && att_dst && dhf && da_src &&
               datt_src && datt_dst && scratch, "gcnx_gat_bwd_nodes: NULL pointer");
  GCNX_REQUIRE(ctx, dhf != d_out && dhf != hf, "gcnx_gat_bwd_nodes: dhf must not alias d_out or hf");
  GatNodeArgs a{};
  a.rowptr = rowptr_t; a.colidx = colidx_t; a.perm = perm_t; a.n = n; a.heads = heads; a.lph = c / 4; a.alpha = alpha; a.dz = dz;
  a.d_out = d_out; a.ldd = ldd; a.hf = hf; a.ldh = ldh; a.da_dst = da_dst; a.att_src = att_src; a.att_dst = att_dst; a.dhf = dhf;
  a.ldg = ldg; a.da_src = da_src; a.part = scratch;
  const int tiles = gcnx_cdiv(n, kTileRows);
#define GCNX_GAT_BN(HC_) hipLaunchKernelGGL((gat_bwd_nodes_kernel<HC_>), dim3(tiles), dim3(8 * HC_), 0, ctx->stream, a)
  GCNX_GAT_DISPATCH(hc, GCNX_GAT_BN);
#undef GCNX_GAT_BN
  GCNX_LAUNCH_OK(ctx);
  hipLaunchKernelGGL(gat_datt_reduce_kernel, dim3(2 * hc / 8), dim3(256), 0, ctx->stream, (const float*)scratch, (int64_t)tiles, hc,
                     datt_src, datt_dst);
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

}  // extern "C"
