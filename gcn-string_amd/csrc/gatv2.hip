// GATv2Conv (Brody et al.; PyG's GATv2Conv(heads = H, concat = True, share_weights = False, edge_dim = D)) in the small-feature
// regime (H C <= 128): attention whose score reads the edge features.  The LeakyReLU comes BEFORE the dot with att, so the
// score of an entry depends jointly on target, source and edge.  Row i of the CSR is the target, its stored entries j the
// sources, values ignored; Xl | Xr [n, 2 HC] is ONE array (one gcnx_gemm with the stacked weight), head h owns columns
// [h c, h c + c) of each half:
//
//     t_ij[hc] = sum_d e_ij[d] W_e[d, hc]       s_ij = (Xl[j] + Xr[i]) + t_ij       g = s > 0 ? s : slope s
//     score_ij,h = <att[h,:], g_ij[h,:]>    alpha = softmax over the row's entries    O[i,h,:] = sum_j alpha Xl[j,h,:]      gatv2_aggregate
//     r = <dO, O>   dscore = alpha (<dO[i,h,:], Xl[j,h,:]> - r)   ds = dscore att (s > 0 ? 1 : slope)
//     dXr[i] = sum_j ds   datt = sum_ij dscore g   dW_e[d] = sum_ij e_ij[d] ds                                             gatv2_bwd_edges
//     dXl[j] = sum_i (alpha dO[i] + ds)                                                                                    gatv2_bwd_nodes
//
// Nobody stores s (nnz H C floats): the three kernels recompute it with ONE expression, gv2_t / gv2_s below -- separately rounded
// products and adds in a fixed order, no FMA -- so they agree on the side of every kink, and NumPy float32 reproduces it.
// fp32 throughout, no float atomics, every sum in a fixed order: the same call leaves the same bits.
//
// Shape of a workgroup (gat.hip's; the device helpers they share: conv_tile.h): 32 rows, one lane group of HC / 4 lanes per row
// with one float4 of the row each -- 8 HC threads (the two backward kernels at HC = 128: 16 rows, see conv_tile_rows).  Head h
// owns the c / 4 consecutive lanes [h c / 4, (h + 1) c / 4) of a group,
// always inside one wave: per-head dot products are xor butterflies over those lanes (every lane ends with the same bits).
// The tile's CSR entries are staged in LDS (1024 of them; a tile with more reads the rest from global memory).  Feature rows
// are gathered with range-checked buffer loads, slots past a row's end fetch nothing.  W_e sits in registers: E float4 per lane
// in the kernel built for up to E in {0, 2, 8} edge features, addressed under nested uniform tests d < edge_dim (no indexed
// register array).
//
// The forward gathers Xl[j] ONCE: the score needs the whole row, the same bytes the weighted sum reads, so a score pass of
// its own (gat.hip's, which reads `heads` floats per entry) would double the gather.  A running maximum m and a rescaled
// accumulator take its place, one rescale per trip of four entries: m' = max(m, the trip's scores), acc = acc exp(m - m') +
// sum_u exp(score_u - m') Xl[j_u], l likewise -- in CSR order.  The maximum's own weight is exp(0) = 1 when it enters and every
// later rescale is followed by such a term, so l >= 1: no overflow, no 0 / 0.  alpha, if asked for, is exp(score - m) / l from
// the scores kept in LDS, written behind the loop.
#include <cmath>

#include "common.h"
#include "conv_tile.h"

namespace {

// over the lph (a power of two) consecutive lanes of a head: every lane gets the same bits
// (the partner lane^off comes from a swizzle with a constant mask -- off = 16, 8, 4 -- or a quad permutation -- off = 2, 1 --
// under uniform tests of lph: no per-lane address as a shuffle by a run-time offset needs, the same additions in the same order)
__device__ __forceinline__ float vhead_sum(float v, int lph) {
  if (lph > 16) v += swz_xor<16>(v);
  if (lph > 8) v += swz_xor<8>(v);
  if (lph > 4) v += swz_xor<4>(v);
  if (lph > 2) v += quad_perm<0x4E>(v);                      // lanes [2, 3, 0, 1] of every quad
  if (lph > 1) v += quad_perm<0xB1>(v);                      // lanes [1, 0, 3, 2]
  return v;
}

// the edge features of the U entries of a trip; ok[u] = false: zeros.  Feature d is touched inside the (uniform) test of
// feature d - 1, so a trip costs edge_dim + 1 branches, not one per (entry, channel, feature), and every index is a constant.
template <int Dd, int E, int U>
__device__ __forceinline__ void vload_e_from(EdgeF<E> (&r)[U], const float* __restrict__ e, int64_t lde, int edge_dim,
                                             const int64_t (&entry)[U], const bool (&ok)[U]) {
  if constexpr (Dd < E) {
    if (Dd < edge_dim) {
#pragma unroll
      for (int u = 0; u < U; ++u) r[u].v[Dd] = ok[u] ? e[entry[u] * lde + Dd] : 0.f;
      vload_e_from<Dd + 1, E, U>(r, e, lde, edge_dim, entry, ok);
    }
  }
}
template <int E, int U>
__device__ __forceinline__ void vload_e(EdgeF<E> (&r)[U], const float* __restrict__ e, int64_t lde, int edge_dim, const int64_t (&entry)[U],
                                        const bool (&ok)[U]) {
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int d = 0; d < (E > 0 ? E : 1); ++d) r[u].v[d] = 0.f;
  vload_e_from<0, E, U>(r, e, lde, edge_dim, entry, ok);
}

// THE expression of s (contract): t from the rounded product of d = 0, then the separately rounded products of d = 1 ..
// edge_dim - 1 added in that order (edge_dim = 0: t = 0); one add forms Xl + Xr, one more adds t.  No contraction into an FMA.
__device__ __forceinline__ float4 v4mul_rn(float v, float4 a) {
  return make_float4(__fmul_rn(v, a.x), __fmul_rn(v, a.y), __fmul_rn(v, a.z), __fmul_rn(v, a.w));
}
__device__ __forceinline__ float4 v4add_rn(float4 a, float4 b) {
  return make_float4(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z), __fadd_rn(a.w, b.w));
}
// t of the U entries of a trip (nested as vload_e_from)
template <int Dd, int E, int U>
__device__ __forceinline__ void gv2_t_from(float4 (&t)[U], const EdgeF<E> (&e)[U], const EdgeW<E>& w, int edge_dim) {
  if constexpr (Dd < E) {
    if (Dd < edge_dim) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float4 pr = v4mul_rn(e[u].v[Dd], w.w[Dd]);
        t[u] = Dd == 0 ? pr : v4add_rn(t[u], pr);
      }
      gv2_t_from<Dd + 1, E, U>(t, e, w, edge_dim);
    }
  }
}
template <int E, int U>
__device__ __forceinline__ void gv2_t(float4 (&t)[U], const EdgeF<E> (&e)[U], const EdgeW<E>& w, int edge_dim) {
#pragma unroll
  for (int u = 0; u < U; ++u) t[u] = zero4();
  gv2_t_from<0, E, U>(t, e, w, edge_dim);
}
// t of the U entries of a trip straight from memory, for the kernels that need the features for nothing else: feature d of
// the U entries is loaded and used inside the test of feature d - 1 (no register copy of e)
template <int Dd, int E, int U>
__device__ __forceinline__ void gv2_t_load_from(float4 (&t)[U], const float* __restrict__ e, int64_t lde, const int64_t (&entry)[U],
                                                const bool (&ok)[U], const EdgeW<E>& w, int edge_dim) {
  if constexpr (Dd < E) {
    if (Dd < edge_dim) {
      float ev[U];
#pragma unroll
      for (int u = 0; u < U; ++u) ev[u] = ok[u] ? e[entry[u] * lde + Dd] : 0.f;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float4 pr = v4mul_rn(ev[u], w.w[Dd]);
        t[u] = Dd == 0 ? pr : v4add_rn(t[u], pr);
      }
      gv2_t_load_from<Dd + 1, E, U>(t, e, lde, entry, ok, w, edge_dim);
    }
  }
}
template <int E, int U>
__device__ __forceinline__ void gv2_t_load(float4 (&t)[U], const float* __restrict__ e, int64_t lde, const int64_t (&entry)[U],
                                           const bool (&ok)[U], const EdgeW<E>& w, int edge_dim) {
#pragma unroll
  for (int u = 0; u < U; ++u) t[u] = zero4();
  gv2_t_load_from<0, E, U>(t, e, lde, entry, ok, w, edge_dim);
}
// dW_e += e (x) ds of one entry (nested the same way)
template <int Dd, int E>
__device__ __forceinline__ void gv2_dwe_from(EdgeW<E>& dwe, const EdgeF<E>& e, float4 ds, int edge_dim) {
  if constexpr (Dd < E) {
    if (Dd < edge_dim) {
      dwe.w[Dd] = fma4(e.v[Dd], ds, dwe.w[Dd]);
      gv2_dwe_from<Dd + 1, E>(dwe, e, ds, edge_dim);
    }
  }
}
__device__ __forceinline__ float4 gv2_s(float4 xl, float4 xr, float4 t) { return v4add_rn(v4add_rn(xl, xr), t); }
// the positive side is s > 0
__device__ __forceinline__ float4 gv2_leaky(float4 s, float slope) {
  return make_float4(s.x > 0.f ? s.x : slope * s.x, s.y > 0.f ? s.y : slope * s.y, s.z > 0.f ? s.z : slope * s.z,
                     s.w > 0.f ? s.w : slope * s.w);
}
// ds = dscore att (s > 0 ? 1 : slope)
__device__ __forceinline__ float4 gv2_ds(float dscore, float4 att, float4 s, float slope) {
  return make_float4(dscore * att.x * (s.x > 0.f ? 1.0f : slope), dscore * att.y * (s.y > 0.f ? 1.0f : slope),
                     dscore * att.z * (s.z > 0.f ? 1.0f : slope), dscore * att.w * (s.w > 0.f ? 1.0f : slope));
}

struct V2FwdArgs {
  const int32_t* rowptr; const int32_t* colidx;
  const float* xlr; int64_t ldx;                 // Xl | Xr
  int32_t n, heads, lph, edge_dim;
  const float* e; int64_t lde;                   // [nnz, edge_dim] (edge_dim = 0: unused)
  const float* w_e; const float* att; const float* bias;
  float slope;
  float* out; int64_t ldo;
  float* alpha;                                  // [nnz, heads] or NULL
  float* o_pre; int64_t ldp;                     // O before the bias, or NULL
};

// ---- scores, softmax over the row's entries and the weighted sum from ONE gather of Xl[j] -------------------------------
template <int HC, int E>
__global__ __launch_bounds__(8 * HC) void gatv2_aggregate_kernel(V2FwdArgs p) {
  constexpr int LPR = HC / 4, NT = 8 * HC;
  extern __shared__ float s_sc[];                        // with alpha: the staged entries' scores, kTileCap * heads floats
  __shared__ int32_t s_col[kTileCap];
  __shared__ int32_t s_rp[kTileRows + 1];
  const int tid = threadIdx.x, r = tid / LPR, sub = tid % LPR;
  const int heads = p.heads, lph = p.lph, h = sub / lph, k = sub % lph, ed = p.edge_dim;
  const ConvTile t = conv_tile(p.rowptr, p.n, s_rp, kTileRows);
  const int staged = min(t.e1 - t.e0, kTileCap);
  for (int i = tid; i < staged; i += NT) s_col[i] = p.colidx[t.e0 + i];
  __syncthreads();
  const bool live = r < t.nr;
  const int ea = live ? s_rp[r] - t.e0 : 0, eb = live ? s_rp[r + 1] - t.e0 : 0;
  const int64_t row = t.r0 + r;
  const float slope = p.slope;
  const int32_t* __restrict__ gcol = p.colidx + t.e0;
  const float4 att = load4(p.att + 4 * sub);
  const EdgeW<E> we = load_edge_w<E>(p.w_e, ed, HC, sub);
  const float4 xr = live ? load4(p.xlr + row * p.ldx + HC + 4 * sub) : zero4();
  const unsigned ld4 = (unsigned)p.ldx * 4u, sub16 = (unsigned)sub * 16u;
  // the descriptor ends behind the last row's HC columns of Xl (nothing past them is addressed)
  const __amdgpu_buffer_rsrc_t xd = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.xlr, (short)0, (int)((unsigned)(p.n - 1) * ld4 + (unsigned)HC * 4u), 0x00020000);
  float* __restrict__ al = p.alpha ? p.alpha + (int64_t)t.e0 * heads + h : nullptr;
  float4 acc = zero4();
  float m = -INFINITY, l = 0.f;
  for (int e = ea; e < eb; e += kTileU) {                   // (the lanes of a row share ea and eb: they shuffle together)
    float4 xv[kTileU], tv[kTileU];
    int64_t en[kTileU];
    bool ok[kTileU];
#pragma unroll
    for (int u = 0; u < kTileU; ++u) {
      ok[u] = e + u < eb;
      const int ee = ok[u] ? e + u : e;
      const int col = ee < kTileCap ? s_col[ee] : gcol[ee];
      xv[u] = buf4(xd, ok[u] ? (unsigned)col * ld4 + sub16 : kOffOut);
      en[u] = (int64_t)t.e0 + ee;
    }
    gv2_t_load(tv, p.e, p.lde, en, ok, we, ed);
    float sc[kTileU];
    float mt = m;
#pragma unroll
    for (int u = 0; u < kTileU; ++u) {
      const float4 g = gv2_leaky(gv2_s(xv[u], xr, tv[u]), slope);
      sc[u] = vhead_sum(dot4(att, g), lph);
      if (e + u < eb) {
        mt = fmaxf(mt, sc[u]);
        // the raw score, turned into alpha behind the loop: kept in LDS (a store to global memory here would sit in the
        // gathers' queue); an entry beyond the staged ones goes through alpha itself
        if (al && k == 0) {
          if (e + u < kTileCap) s_sc[(e + u) * heads + h] = sc[u];
          else al[(int64_t)(e + u) * heads] = sc[u];
        }
      }
    }
    const float scale = expf(m - mt);                    // (first trip: exp(-inf) = 0 on acc = 0, l = 0)
    acc = scale4(scale, acc);
    l *= scale;
#pragma unroll
    for (int u = 0; u < kTileU; ++u) {
      const float w = e + u < eb ? expf(sc[u] - mt) : 0.f;
      acc = fma4(w, xv[u], acc);                        // CSR order
      l += w;
    }
    m = mt;
  }
  const float inv = eb > ea ? 1.0f / l : 0.f;
  if (p.alpha) {                                         // (uniform)
    __syncthreads();
    const int ebs = min(eb, kTileCap);
    for (int e = ea + k; e < ebs; e += lph) al[(int64_t)e * heads] = expf(s_sc[e * heads + h] - m) * inv;     // lane k: entries k, k + lph, ...
    if (k == 0)                                          // rare: this lane's own stores read back
      for (int e = max(ea, kTileCap); e < eb; ++e) al[(int64_t)e * heads] = expf(al[(int64_t)e * heads] - m) * inv;
  }
  if (!live) return;
  const float4 o = scale4(inv, acc);                    // a row without entries: exact zeros
  if (p.o_pre) *reinterpret_cast<float4*>(p.o_pre + row * p.ldp + 4 * sub) = o;
  float4 y = o;
  if (p.bias) {
    const float4 b = load4(p.bias + 4 * sub);
    y = eb > ea ? add4(o, b) : b;                       // (no entries: the bias, bit for bit)
  }
  *reinterpret_cast<float4*>(p.out + row * p.ldo + 4 * sub) = y;
}

struct V2EdgeArgs {
  const int32_t* rowptr; const int32_t* colidx;
  const float* xlr; int64_t ldx;
  int32_t n, heads, lph, edge_dim;
  const float* e; int64_t lde;
  const float* w_e; const float* att;
  float slope;
  const float* alpha;
  const float* d_out; int64_t ldd;
  const float* o; int64_t ldo;                   // O (before the bias)
  float* dscore;                                 // [nnz, heads]
  float* dxr; int64_t ldg;                       // dXr [n, HC]
  float* part;                                   // [tiles][(1 + edge_dim) HC]: this tile's datt | dW_e
};

// ---- backward on the forward CSR: dscore per entry, dXr per target row, the tile's part of datt and dW_e ------------------
template <int HC, int ROWS, int E>
__global__ __launch_bounds__(ROWS * HC / 4) void gatv2_bwd_edges_kernel(V2EdgeArgs p) {
  constexpr int LPR = HC / 4, NT = ROWS * LPR;
  __shared__ int32_t s_col[kTileCap];
  __shared__ int32_t s_rp[kTileRows + 1];
  __shared__ __attribute__((aligned(16))) float4 s_p[ROWS][LPR];
  const int tid = threadIdx.x, r = tid / LPR, sub = tid % LPR;
  const int heads = p.heads, lph = p.lph, h = sub / lph, k = sub % lph, ed = p.edge_dim;
  const ConvTile t = conv_tile(p.rowptr, p.n, s_rp, ROWS);
  const int staged = min(t.e1 - t.e0, kTileCap);
  for (int i = tid; i < staged; i += NT) s_col[i] = p.colidx[t.e0 + i];
  __syncthreads();
  const bool live = r < t.nr;
  const int ea = live ? s_rp[r] - t.e0 : 0, eb = live ? s_rp[r + 1] - t.e0 : 0;
  const int64_t row = t.r0 + r;
  const float slope = p.slope;
  const float4 att = load4(p.att + 4 * sub);
  const EdgeW<E> we = load_edge_w<E>(p.w_e, ed, HC, sub);
  float4 dO = zero4(), O = dO, xr = dO;
  if (live) {
    dO = load4(p.d_out + row * p.ldd + 4 * sub);
    O = load4(p.o + row * p.ldo + 4 * sub);
    xr = load4(p.xlr + row * p.ldx + HC + 4 * sub);
  }
  const float rr = vhead_sum(dot4(dO, O), lph);         // = sum_k alpha_ik dalpha_ik: no second pass over the row
  const unsigned ld4 = (unsigned)p.ldx * 4u, sub16 = (unsigned)sub * 16u;
  const __amdgpu_buffer_rsrc_t xd = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.xlr, (short)0, (int)((unsigned)(p.n - 1) * ld4 + (unsigned)HC * 4u), 0x00020000);
  const int32_t* __restrict__ gcol = p.colidx + t.e0;
  const float* __restrict__ al = p.alpha + (int64_t)t.e0 * heads + h;
  float* __restrict__ dso = p.dscore + (int64_t)t.e0 * heads + h;
  float4 dxr = zero4(), datt = zero4();
  EdgeW<E> dwe;
#pragma unroll
  for (int d = 0; d < (E > 0 ? E : 1); ++d) dwe.w[d] = zero4();
  for (int e = ea; e < eb; e += kTileU) {
    float4 xv[kTileU], tv[kTileU];
    EdgeF<E> ev[kTileU];
    float av[kTileU];
    int64_t en[kTileU];
    bool ok[kTileU];
#pragma unroll
    for (int u = 0; u < kTileU; ++u) {
      ok[u] = e + u < eb;
      const int ee = ok[u] ? e + u : e;
      const int col = ee < kTileCap ? s_col[ee] : gcol[ee];
      xv[u] = buf4(xd, ok[u] ? (unsigned)col * ld4 + sub16 : kOffOut);
      en[u] = (int64_t)t.e0 + ee;
      av[u] = al[(int64_t)ee * heads];
    }
    vload_e(ev, p.e, p.lde, ed, en, ok);
    gv2_t(tv, ev, we, ed);
#pragma unroll
    for (int u = 0; u < kTileU; ++u) {
      const float d = vhead_sum(dot4(dO, xv[u]), lph);
      if (e + u < eb) {
        const float dsc = av[u] * (d - rr);
        if (k == 0) dso[(int64_t)(e + u) * heads] = dsc;
        const float4 s = gv2_s(xv[u], xr, tv[u]);
        const float4 g = gv2_leaky(s, slope);
        const float4 ds = gv2_ds(dsc, att, s, slope);
        dxr = add4(dxr, ds);                            // CSR order
        datt = fma4(dsc, g, datt);
        gv2_dwe_from<0, E>(dwe, ev[u], ds, ed);
      }
    }
  }
  if (live) *reinterpret_cast<float4*>(p.dxr + row * p.ldg + 4 * sub) = dxr;
  // datt and dW_e[d]: this tile's 32 rows, in row order, one quantity after the other through the same LDS rows
  float* __restrict__ part = p.part + (int64_t)(t.r0 / ROWS) * (1 + ed) * HC;
#pragma unroll
  for (int q = 0; q <= E; ++q) {
    if (q <= ed) {                                       // (uniform)
      s_p[r][sub] = q == 0 ? datt : dwe.w[q > 0 ? q - 1 : 0];
      __syncthreads();
      if (tid < LPR) {
        float4 s = zero4();
#pragma unroll 8
        for (int i = 0; i < ROWS; ++i) s = add4(s, s_p[i][tid]);
        *reinterpret_cast<float4*>(part + q * HC + 4 * tid) = s;
      }
      __syncthreads();
    }
  }
}

// the tiles' parts summed in a fixed order (gcnx_colpart_reduce_sum): columns [0, hc) are datt, the rest dW_e
__global__ __launch_bounds__(256) void gatv2_part_reduce_kernel(const float* __restrict__ part, int64_t tiles, int32_t hc, int32_t f,
                                                                float* __restrict__ datt, float* __restrict__ dw_e) {
  __shared__ float4 s[128][2];
  const float4 v = gcnx_colpart_reduce_sum(part, tiles, f, blockIdx.x, s);
  const int c = blockIdx.x * 8 + (threadIdx.x & 1) * 4;
  if ((threadIdx.x >> 1) == 0 && c < f) *reinterpret_cast<float4*>(c < hc ? datt + c : dw_e + (c - hc)) = v;
}

struct V2NodeArgs {
  const int32_t* rowptr; const int32_t* colidx; const int32_t* perm;     // the transposed pattern and its entry permutation
  const float* xlr; int64_t ldx;
  int32_t n, heads, lph, edge_dim;
  const float* e; int64_t lde;                                           // forward entry order
  const float* w_e; const float* att;
  float slope;
  const float* alpha; const float* dscore;                               // [nnz, heads], forward entry order
  const float* d_out; int64_t ldd;
  float* dxl; int64_t ldg;                                               // dXl [n, HC]
};

// ---- backward on the transposed pattern: dXl per source row -----------------------------------------------------------------
template <int HC, int ROWS, int E>
__global__ __launch_bounds__(ROWS * HC / 4) void gatv2_bwd_nodes_kernel(V2NodeArgs p) {
  constexpr int LPR = HC / 4, NT = ROWS * LPR;
  __shared__ int32_t s_col[kTileCap];
  __shared__ int32_t s_q[kTileCap];
  __shared__ int32_t s_rp[kTileRows + 1];
  const int tid = threadIdx.x, r = tid / LPR, sub = tid % LPR;
  const int heads = p.heads, lph = p.lph, h = sub / lph, ed = p.edge_dim;
  const ConvTile t = conv_tile(p.rowptr, p.n, s_rp, ROWS);
  const int staged = min(t.e1 - t.e0, kTileCap);
  for (int i = tid; i < staged; i += NT) {
    s_col[i] = p.colidx[t.e0 + i];
    s_q[i] = p.perm[t.e0 + i];
  }
  __syncthreads();
  const bool live = r < t.nr;
  const int ea = live ? s_rp[r] - t.e0 : 0, eb = live ? s_rp[r + 1] - t.e0 : 0;
  const int64_t row = t.r0 + r;
  const float slope = p.slope;
  const float4 att = load4(p.att + 4 * sub);
  const EdgeW<E> we = load_edge_w<E>(p.w_e, ed, HC, sub);
  const float4 xl = live ? load4(p.xlr + row * p.ldx + 4 * sub) : zero4();
  const unsigned ldd4 = (unsigned)p.ldd * 4u, ldx4 = (unsigned)p.ldx * 4u, sub16 = (unsigned)sub * 16u;
  const __amdgpu_buffer_rsrc_t dd = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.d_out, (short)0, (int)((unsigned)(p.n - 1) * ldd4 + (unsigned)HC * 4u), 0x00020000);
  // Xr = columns [HC, 2 HC) of Xl | Xr: the descriptor ends behind the last row's 2 HC columns
  const __amdgpu_buffer_rsrc_t xd = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.xlr, (short)0, (int)((unsigned)(p.n - 1) * ldx4 + (unsigned)HC * 8u), 0x00020000);
  const int32_t* __restrict__ gcol = p.colidx + t.e0;
  const int32_t* __restrict__ gq = p.perm + t.e0;
  float4 acc = zero4();
  for (int e = ea; e < eb; e += kTileU) {
    float4 dv[kTileU], xv[kTileU], tv[kTileU];
    float av[kTileU], zv[kTileU];
    int64_t en[kTileU];
    bool ok[kTileU];
#pragma unroll
    for (int u = 0; u < kTileU; ++u) {
      ok[u] = e + u < eb;
      const int ee = ok[u] ? e + u : e;
      const bool st = ee < kTileCap;
      const int col = st ? s_col[ee] : gcol[ee];
      en[u] = st ? s_q[ee] : gq[ee];
      dv[u] = buf4(dd, ok[u] ? (unsigned)col * ldd4 + sub16 : kOffOut);
      xv[u] = buf4(xd, ok[u] ? (unsigned)col * ldx4 + (unsigned)HC * 4u + sub16 : kOffOut);
      av[u] = ok[u] ? p.alpha[en[u] * heads + h] : 0.f;
      zv[u] = ok[u] ? p.dscore[en[u] * heads + h] : 0.f;
    }
    gv2_t_load(tv, p.e, p.lde, en, ok, we, ed);
#pragma unroll
    for (int u = 0; u < kTileU; ++u) {
      if (e + u < eb) {
        const float4 s = gv2_s(xl, xv[u], tv[u]);
        acc = add4(fma4(av[u], dv[u], acc), gv2_ds(zv[u], att, s, slope));      // the transposed CSR's order
      }
    }
  }
  if (live) *reinterpret_cast<float4*>(p.dxl + row * p.ldg + 4 * sub) = acc;
}

bool v2_shape_ok(int64_t n, int32_t heads, int32_t c, int64_t ldx, int32_t edge_dim) {
  if (n < 0 || !(heads == 1 || heads == 2 || heads == 4 || heads == 8) || c < 4 || c > 128) return false;
  if (edge_dim < 0 || edge_dim > kEdgeMax) return false;
  const int hc = heads * c;
  return (hc == 16 || hc == 32 || hc == 64 || hc == 128) && ldx >= 2 * hc && ldx % 4 == 0 &&
         (uint64_t)n * (uint64_t)ldx * 4u < 0x100000000ull;
}
// (the two backward kernels run conv_tile_rows rows per workgroup: at HC = 128 W_e, its gradient and a trip's operands do not
// fit beside 32 rows; the forward keeps 32 at every width)

const char* kV2Shapes = "needs heads in {1, 2, 4, 8}, heads * c in {16, 32, 64, 128}, c >= 4, ldx >= 2 * heads * c in multiples of 4 "
                        "floats, n * ldx * 4 < 2^32 and 0 <= edge_dim <= 8";

}  // namespace

extern "C" {

int gcnx_gatv2_conv_ok(int64_t n, int32_t heads, int32_t c, int64_t ldx, int32_t edge_dim) {
  return v2_shape_ok(n, heads, c, ldx, edge_dim) ? 1 : 0;
}

int64_t gcnx_gatv2_bwd_scratch_floats(int64_t n, int32_t heads, int32_t c, int32_t edge_dim) {
  if (n < 0 || heads < 0 || c < 0 || edge_dim < 0) return 0;
  return (int64_t)gcnx_cdiv(n, conv_tile_rows(heads * c)) * (1 + edge_dim) * heads * c;
}

int gcnx_gatv2_aggregate(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* xlr, int64_t ldx, int32_t n,
                         int32_t heads, int32_t c, const float* e, int64_t lde, int32_t edge_dim, const float* w_e, const float* att,
                         const float* bias, float slope, float* out, int64_t ldo, float* alpha, float* o_pre, int64_t ldp) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "GATv2Conv aggregate");
  GCNX_REQUIRE(ctx, n >= 0 && heads >= 0 && c >= 0 && edge_dim >= 0, "gcnx_gatv2_aggregate: negative size");
  if (!v2_shape_ok(n, heads, c, ldx, edge_dim))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_gatv2_aggregate: %s (got n=%d heads=%d c=%d ldx=%lld edge_dim=%d)", kV2Shapes, n,
                     heads, c, (long long)ldx, edge_dim);
  const int hc = heads * c;
  if (!gcnx_aligned16(xlr) || !gcnx_aligned16(w_e) || !gcnx_aligned16(att) || !gcnx_aligned16(bias) || !gcnx_aligned16(out) ||
      !conv_ld_ok(ldo, hc) || (o_pre && (!gcnx_aligned16(o_pre) || !conv_ld_ok(ldp, hc))))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_gatv2_aggregate: xlr, w_e, att, bias, out and o_pre must be 16-byte aligned, with ldo "
                     "and ldp >= heads * c in multiples of 4 floats");
  if (n == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, rowptr && colidx && xlr && att && out, "gcnx_gatv2_aggregate: NULL pointer");
  GCNX_REQUIRE(ctx, edge_dim == 0 || (e && w_e && lde >= edge_dim), "gcnx_gatv2_aggregate: edge_dim > 0 needs e (lde >= edge_dim) and w_e");
  GCNX_REQUIRE(ctx, xlr != out && xlr != o_pre && out != o_pre, "gcnx_gatv2_aggregate: the outputs must not alias xlr or each other");
  V2FwdArgs a{};
  a.rowptr = rowptr; a.colidx = colidx; a.xlr = xlr; a.ldx = ldx; a.n = n; a.heads = heads; a.lph = c / 4; a.edge_dim = edge_dim;
  a.e = e; a.lde = lde; a.w_e = w_e; a.att = att; a.bias = bias; a.slope = slope; a.out = out; a.ldo = ldo; a.alpha = alpha;
  a.o_pre = o_pre; a.ldp = ldp;
  const int tiles = gcnx_cdiv(n, kTileRows);
  const size_t dyn = alpha ? (size_t)kTileCap * heads * sizeof(float) : 0;
#define GCNX_V2_AGG(HC_, BR_, E_) hipLaunchKernelGGL((gatv2_aggregate_kernel<HC_, E_>), dim3(tiles), dim3(8 * HC_), dyn, ctx->stream, a)
  GCNX_CONV_DISPATCH(hc, edge_dim, GCNX_V2_AGG);
#undef GCNX_V2_AGG
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

int gcnx_gatv2_bwd_edges(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* xlr, int64_t ldx, int32_t n,
                         int32_t heads, int32_t c, const float* e, int64_t lde, int32_t edge_dim, const float* w_e, const float* att,
                         float slope, const float* alpha, const float* d_out, int64_t ldd, const float* o, int64_t ldo, float* dscore,
                         float* dxr, int64_t ldg, float* datt, float* dw_e, float* scratch) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "GATv2Conv backward (edges)");
  GCNX_REQUIRE(ctx, n >= 0 && heads >= 0 && c >= 0 && edge_dim >= 0, "gcnx_gatv2_bwd_edges: negative size");
  if (!v2_shape_ok(n, heads, c, ldx, edge_dim))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_gatv2_bwd_edges: %s (got n=%d heads=%d c=%d ldx=%lld edge_dim=%d)", kV2Shapes, n,
                     heads, c, (long long)ldx, edge_dim);
  const int hc = heads * c;
  if (!gcnx_aligned16(xlr) || !gcnx_aligned16(w_e) || !gcnx_aligned16(att) || !gcnx_aligned16(d_out) || !gcnx_aligned16(o) ||
      !gcnx_aligned16(dxr) || !gcnx_aligned16(datt) || !gcnx_aligned16(dw_e) || !gcnx_aligned16(scratch) || !conv_ld_ok(ldd, hc) ||
      !conv_ld_ok(ldo, hc) || !conv_ld_ok(ldg, hc))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_gatv2_bwd_edges: xlr, w_e, att, d_out, o, dxr, datt, dw_e and scratch must be 16-byte "
                     "aligned, with ldd, ldo and ldg >= heads * c in multiples of 4 floats");
  if (n == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, rowptr && colidx && xlr && att && alpha && d_out && o && dscore && dxr && datt && scratch,
               "gcnx_gatv2_bwd_edges: NULL pointer");
  GCNX_REQUIRE(ctx, edge_dim == 0 || (e && w_e && dw_e && lde >= edge_dim),
               "gcnx_gatv2_bwd_edges: edge_dim > 0 needs e (lde >= edge_dim), w_e and dw_e");
  GCNX_REQUIRE(ctx, dxr != d_out && dxr != o && dxr != xlr, "gcnx_gatv2_bwd_edges: dxr must not alias d_out, o or xlr");
  V2EdgeArgs a{};
  a.rowptr = rowptr; a.colidx = colidx; a.xlr = xlr; a.ldx = ldx; a.n = n; a.heads = heads; a.lph = c / 4; a.edge_dim = edge_dim;
  a.e = e; a.lde = lde; a.w_e = w_e; a.att = att; a.slope = slope; a.alpha = alpha; a.d_out = d_out; a.ldd = ldd; a.o = o; a.ldo = ldo;
  a.dscore = dscore; a.dxr = dxr; a.ldg = ldg; a.part = scratch;
  const int tiles = gcnx_cdiv(n, conv_tile_rows(hc));
#define GCNX_V2_BE(HC_, BR_, E_) hipLaunchKernelGGL((gatv2_bwd_edges_kernel<HC_, BR_, E_>), dim3(tiles), dim3(BR_ * HC_ / 4), 0, ctx->stream, a)
  GCNX_CONV_DISPATCH(hc, edge_dim, GCNX_V2_BE);
#undef GCNX_V2_BE
  GCNX_LAUNCH_OK(ctx);
  const int f = (1 + edge_dim) * hc;
  hipLaunchKernelGGL(gatv2_part_reduce_kernel, dim3(f / 8), dim3(256), 0, ctx->stream, (const float*)scratch, (int64_t)tiles, hc, f, datt,
                     dw_e);
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

int gcnx_gatv2_bwd_nodes(gcnx_ctx* ctx, const int32_t* rowptr_t, const int32_t* colidx_t, const int32_t* perm_t, const float* xlr,
                         int64_t ldx, int32_t n, int32_t heads, int32_t c, const float* e, int64_t lde, int32_t edge_dim,
                         const float* w_e, const float* att, float slope, const float* alpha, const float* dscore, const float* d_out,
                         int64_t ldd, float* dxl, int64_t ldg) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "GATv2Conv backward (nodes)");
  GCNX_REQUIRE(ctx, n >= 0 && heads >= 0 && c >= 0 && edge_dim >= 0, "gcnx_gatv2_bwd_nodes: negative size");
  if (!v2_shape_ok(n, heads, c, ldx, edge_dim))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_gatv2_bwd_nodes: %s (got n=%d heads=%d c=%d ldx=%lld edge_dim=%d)", kV2Shapes, n,
                     heads, c, (long long)ldx, edge_dim);
  const int hc = heads * c;
  if (!gcnx_aligned16(xlr) || !gcnx_aligned16(w_e) || !gcnx_aligned16(att) || !gcnx_aligned16(d_out) || !gcnx_aligned16(dxl) ||
      !conv_ld_ok(ldd, hc) || !conv_ld_ok(ldg, hc) || !gcnx_fits_buffer(n, ldd, 4))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_gatv2_bwd_nodes: xlr, w_e, att, d_out and dxl must be 16-byte aligned, with ldd and "
                     "ldg >= heads * c in multiples of 4 floats and n * ldd * 4 < 2^32");
  if (n == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, rowptr_t && colidx_t && perm_t && xlr && att && alpha && dscore && d_out && dxl, "gcnx_gatv2_bwd_nodes: NULL pointer");
  GCNX_REQUIRE(ctx, edge_dim == 0 || (e && w_e && lde >= edge_dim), "gcnx_gatv2_bwd_nodes: edge_dim > 0 needs e (lde >= edge_dim) and w_e");
  GCNX_REQUIRE(ctx, dxl != d_out && dxl != xlr, "gcnx_gatv2_bwd_nodes: dxl must not alias d_out or xlr");
  V2NodeArgs a{};
  a.rowptr = rowptr_t; a.colidx = colidx_t; a.perm = perm_t; a.xlr = xlr; a.ldx = ldx; a.n = n; a.heads = heads; a.lph = c / 4;
  a.edge_dim = edge_dim; a.e = e; a.lde = lde; a.w_e = w_e; a.att = att; a.slope = slope; a.alpha = alpha; a.dscore = dscore;
  a.d_out = d_out; a.ldd = ldd; a.dxl = dxl; a.ldg = ldg;
  const int tiles = gcnx_cdiv(n, conv_tile_rows(hc));
#define GCNX_V2_BN(HC_, BR_, E_) hipLaunchKernelGGL((gatv2_bwd_nodes_kernel<HC_, BR_, E_>), dim3(tiles), dim3(BR_ * HC_ / 4), 0, ctx->stream, a)
  GCNX_CONV_DISPATCH(hc, edge_dim, GCNX_V2_BN);
#undef GCNX_V2_BN
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

}  // extern "C"
