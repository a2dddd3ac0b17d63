// TransformerConv (Shi et al., UniMP; PyG's TransformerConv(in, C, heads = H, concat = True, beta, edge_dim = D, root_weight))
// in the small-feature regime (H C <= 128): scaled dot-product attention whose keys AND values carry the edge features.
// Row i of the CSR is the target, its stored entries j the sources, values ignored; P = Q | K | V (| S) [n, 3 HC (4 HC)] is ONE
// array (one gcnx_gemm with the stacked weight), head h owns columns [h c, h c + c) of every block, w_e [edge_dim, HC]:
//
//     T_ij = sum_d e_ij[d] W_e[d]      k_ij = K[j] + T_ij      v_ij = V[j] + T_ij      score_ij,h = <Q[i,h,:], k_ij[h,:]> s
//     alpha = softmax over the row's entries     O[i,h,:] = sum_j alpha v_ij[h,:]
//     out = O | O + S | b S + (1 - b) O,  b_i = sigmoid(<w1, O_i> + <w2, S_i> + <w3, O_i - S_i>)                      transformer_aggregate
//     g_i = <d_out_i, S_i - O_i> b_i (1 - b_i)    dO = (1 - b) d_out + g (w1 + w3)    dS = b d_out + g (w2 - w3)
//     dw1 = sum_i g O    dw2 = sum_i g S    dw3 = sum_i g (O - S)                                                     transformer_beta_bwd
//     r = <dO, O>    dscore = alpha (<dO[i,h,:], v_ij[h,:]> - r)    dQ[i] = s sum_j dscore k_ij
//     dW_e[d,h,:] = sum_i (s Q[i,h,:] A_i[d,h] + dO[i,h,:] B_i[d,h]),  A = sum_j e_ij[d] dscore,  B = sum_j e_ij[d] alpha  transformer_bwd_targets
//     dK[j] = s sum_i dscore Q[i]      dV[j] = sum_i alpha dO[i]                                                      transformer_bwd_sources
//
// Softmax, dot and sigmoid have no kink, so the kernels need not agree bit for bit on anything they recompute (gatv2.hip's
// separately rounded expression is not needed): products and adds contract into FMAs.  sigmoid(a) = rcp(1 + exp(-a)) as in
// resgated.hip: exp(-a) = +inf gives 0, exp(-a) = 0 gives 1, b (1 - b) is finite for every finite a.
// fp32 throughout, no float atomics, every sum in a fixed order: the same call leaves the same bits.
//
// Shape of a workgroup (gatv2.hip's and resgated.hip's; the device helpers they share: conv_tile.h): 32 rows, one lane group
// of HC / 4 lanes per row with one float4 of the row each -- 8 HC threads (HC = 128: 16 rows, see conv_tile_rows: W_e with a
// trip's three float4 per entry does not fit beside 32 rows at E = 8).  Head h owns the c / 4 consecutive lanes
// [h c / 4, (h + 1) c / 4) of a group, always inside one wave: per-head dots are xor butterflies over those lanes, the beta
// gate's row dot the same butterfly over the whole group.  The tile's CSR entries are staged in LDS (1024 of them; a tile
// with more reads the rest from global memory).  K[j] | V[j] are adjacent in P: one entry costs one contiguous 2 HC piece of
// row j, gathered with range-checked buffer loads -- slots past a row's end fetch nothing.  W_e sits in registers: E float4
// per lane in the kernel built for up to E in {0, 2, 8} edge features, addressed under nested uniform tests d < edge_dim (no
// indexed register array).  The dW_e pass keeps 2 edge_dim SCALARS per lane (A and B above), not float4 vectors per
// feature: the outer products with Q[i] and dO[i] are formed once per row, behind the loop.
//
// The forward keeps a running maximum m and a rescaled accumulator, one rescale per trip of four entries (gatv2.hip): the
// maximum's own weight is exp(0) = 1 and every later rescale is followed by such a term, so l >= 1: no overflow, no 0 / 0.
#include <cmath>

#include "common.h"
#include "conv_tile.h"

namespace {

// over lph (a power of two <= 32) consecutive lanes: every lane gets the same bits (the partner lane^off comes from a swizzle
// with a constant mask -- off = 16, 8, 4 -- or a quad permutation -- off = 2, 1).  No branches on lph: a step wider than the
// group multiplies its partner by 0 (the 0 / 1 factors are formed once per kernel; five tests of lph kept as lane masks
// through the entry loop cost the scalar registers that spilled).
struct TGroup { float m16, m8, m4, m2, m1; };
__device__ __forceinline__ TGroup tgroup(int lph) {
  TGroup g;
  g.m16 = lph > 16 ? 1.f : 0.f; g.m8 = lph > 8 ? 1.f : 0.f; g.m4 = lph > 4 ? 1.f : 0.f; g.m2 = lph > 2 ? 1.f : 0.f;
  g.m1 = lph > 1 ? 1.f : 0.f;
  return g;
}
__device__ __forceinline__ float tgroup_sum(float v, const TGroup& g) {
  v = fmaf(g.m16, swz_xor<16>(v), v);
  v = fmaf(g.m8, swz_xor<8>(v), v);
  v = fmaf(g.m4, swz_xor<4>(v), v);
  v = fmaf(g.m2, quad_perm<0x4E>(v), v);                     // lanes [2, 3, 0, 1] of every quad
  v = fmaf(g.m1, quad_perm<0xB1>(v), v);                     // lanes [1, 0, 3, 2]
  return v;
}

// t = e W_e of the U entries of a trip, d ascending.  Feature d is loaded and used inside the (uniform) test of feature
// d - 1, so a trip costs edge_dim + 1 branches and every register index is a constant.  No mask: the slots past a row's end
// name the trip's first entry again (a valid address; what they compute is weighted with 0 or never stored).
// The features stay in r for the kernel that needs them again (dw_e).
template <int Dd, int E, int U>
__device__ __forceinline__ void tf_edge_from(float4 (&t)[U], EdgeF<E> (&r)[U], const float* __restrict__ e, int64_t lde,
                                             const int64_t (&entry)[U], const EdgeW<E>& w, int edge_dim) {
  if constexpr (Dd < E) {
    if (Dd < edge_dim) {
#pragma unroll
      for (int u = 0; u < U; ++u) r[u].v[Dd] = e[entry[u] * lde + Dd];
#pragma unroll
      for (int u = 0; u < U; ++u) t[u] = fma4(r[u].v[Dd], w.w[Dd], t[u]);
      tf_edge_from<Dd + 1, E, U>(t, r, e, lde, entry, w, edge_dim);
    }
  }
}
template <int E, int U>
__device__ __forceinline__ void tf_edge(float4 (&t)[U], EdgeF<E> (&r)[U], const float* __restrict__ e, int64_t lde,
                                        const int64_t (&entry)[U], const EdgeW<E>& w, int edge_dim) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    t[u] = zero4();
#pragma unroll
    for (int d = 0; d < (E > 0 ? E : 1); ++d) r[u].v[d] = 0.f;
  }
  tf_edge_from<0, E, U>(t, r, e, lde, entry, w, edge_dim);
}
// A[d] += e[d] dscore, B[d] += e[d] alpha of one entry (nested the same way)
template <int E> struct TEdgeS { float a[E > 0 ? E : 1]; float b[E > 0 ? E : 1]; };
template <int Dd, int E>
__device__ __forceinline__ void tf_ab_from(TEdgeS<E>& s, const EdgeF<E>& e, float dsc, float al, int edge_dim) {
  if constexpr (Dd < E) {
    if (Dd < edge_dim) {
      s.a[Dd] = fmaf(e.v[Dd], dsc, s.a[Dd]);
      s.b[Dd] = fmaf(e.v[Dd], al, s.b[Dd]);
      tf_ab_from<Dd + 1, E>(s, e, dsc, al, edge_dim);
    }
  }
}

struct TFFwdArgs {
  const int32_t* rowptr; const int32_t* colidx;
  const float* p; int64_t ldp;                   // Q | K | V
  int32_t n, heads, lph, edge_dim;
  const float* e; int64_t lde;                   // [nnz, edge_dim] (edge_dim = 0: unused)
  const float* w_e;
  const float* skip; int64_t lds;                // S, or NULL
  const float* w_beta;                           // [3 HC] = w1 | w2 | w3, or NULL
  float scale;                                   // fp32(1 / sqrt(c))
  float* out; int64_t ldo;
  float* alpha;                                  // [nnz, heads] or NULL
  float* o_pre; int64_t ldpre;                   // O before the root connection, or NULL
};

// ---- scores, softmax over the row's entries and the weighted sum from ONE gather of K[j] | V[j]; root and beta gate ---------
template <int HC, int ROWS, int E>
__global__ __launch_bounds__(ROWS * HC / 4) void transformer_aggregate_kernel(TFFwdArgs p) {
  constexpr int LPR = HC / 4, NT = ROWS * LPR;
  extern __shared__ float s_sc[];                        // with alpha: the staged entries' scores, kTileCap * heads floats
  __shared__ int32_t s_col[kTileCap];
  __shared__ int32_t s_rp[kTileRows + 1];
  const int tid = threadIdx.x, r = tid / LPR, sub = tid % LPR;
  const int heads = p.heads, lph = p.lph, h = sub / lph, k = sub % lph, ed = p.edge_dim;
  const ConvTile t = conv_tile(p.rowptr, p.n, s_rp, ROWS);
  const int staged = min(t.e1 - t.e0, kTileCap);
  for (int i = tid; i < staged; i += NT) s_col[i] = p.colidx[t.e0 + i];
  __syncthreads();
  const bool live = r < t.nr;
  const int ea = live ? s_rp[r] - t.e0 : 0, eb = live ? s_rp[r + 1] - t.e0 : 0;
  const int64_t row = t.r0 + r;
  const float scale = p.scale;
  const TGroup gh = tgroup(lph);
  const int32_t* __restrict__ gcol = p.colidx + t.e0;
  const EdgeW<E> we = load_edge_w<E>(p.w_e, ed, HC, sub);
  const float4 q = live ? load4(p.p + row * p.ldp + 4 * sub) : zero4();
  const unsigned ld4 = (unsigned)p.ldp * 4u, koff = (unsigned)HC * 4u + (unsigned)sub * 16u, voff = koff + (unsigned)HC * 4u;
  // the descriptor ends behind the last row's 3 HC columns (nothing past them is addressed)
  const __amdgpu_buffer_rsrc_t pd = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.p, (short)0, (int)((unsigned)(p.n - 1) * ld4 + (unsigned)HC * 12u), 0x00020000);
  float* __restrict__ al = p.alpha ? p.alpha + (int64_t)t.e0 * heads + h : nullptr;
  float4 acc = zero4();
  float m = -INFINITY, l = 0.f;
  for (int e = ea; e < eb; e += kTileU) {                   // (the lanes of a row share ea and eb: they shuffle together)
    float4 kv[kTileU], vv[kTileU], tv[kTileU];
    EdgeF<E> ev[kTileU];
    int64_t en[kTileU];
#pragma unroll
    for (int u = 0; u < kTileU; ++u) {
      const bool ok = e + u < eb;
      const int ee = ok ? e + u : e;
      const int col = ee < kTileCap ? s_col[ee] : gcol[ee];
      kv[u] = buf4(pd, ok ? (unsigned)col * ld4 + koff : kOffOut);
      vv[u] = buf4(pd, ok ? (unsigned)col * ld4 + voff : kOffOut);
      en[u] = (int64_t)t.e0 + ee;
    }
    tf_edge(tv, ev, p.e, p.lde, en, we, ed);
    float sc[kTileU];
    float mt = m;
#pragma unroll
    for (int u = 0; u < kTileU; ++u) {
      sc[u] = tgroup_sum(dot4(q, add4(kv[u], tv[u])), gh) * scale;
      vv[u] = add4(vv[u], tv[u]);
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
    const float resc = expf(m - mt);                     // (first trip: exp(-inf) = 0 on acc = 0, l = 0)
    acc = scale4(resc, acc);
    l *= resc;
#pragma unroll
    for (int u = 0; u < kTileU; ++u) {
      const float w = e + u < eb ? expf(sc[u] - mt) : 0.f;
      acc = fma4(w, vv[u], acc);                        // CSR order
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
  if (p.o_pre) *reinterpret_cast<float4*>(p.o_pre + row * p.ldpre + 4 * sub) = o;
  float4 y = o;
  if (p.skip) {
    const float4 s = load4(p.skip + row * p.lds + 4 * sub);
    if (p.w_beta) {
      const float4 w1 = load4(p.w_beta + 4 * sub), w2 = load4(p.w_beta + HC + 4 * sub), w3 = load4(p.w_beta + 2 * HC + 4 * sub);
      const float a = tgroup_sum(dot4(w1, o) + dot4(w2, s) + dot4(w3, sub4(o, s)), tgroup(LPR));      // the whole row
      const float b = sigmoid1(a);
      y = fma4(b, s, scale4(1.0f - b, o));
    } else {
      y = eb > ea ? add4(o, s) : s;                     // (no entries: S, bit for bit)
    }
  }
  *reinterpret_cast<float4*>(p.out + row * p.ldo + 4 * sub) = y;
}

struct TFBetaArgs {
  const float* d_out; int64_t ldd;
  const float* o; int64_t ldo;
  const float* skip; int64_t lds;
  const float* w_beta;
  int32_t n;
  float* d_o; int64_t ldgo;
  float* d_s; int64_t ldgs;
  float* part;                                   // [tiles][3 HC]: this tile's dw1 | dw2 | dw3
};

// ---- backward of the beta gate, row by row: dO, dS, the tile's part of dw_beta ----------------------------------------------
template <int HC, int ROWS>
__global__ __launch_bounds__(ROWS * HC / 4) void transformer_beta_bwd_kernel(TFBetaArgs p) {
  constexpr int LPR = HC / 4;
  __shared__ __attribute__((aligned(16))) float4 s_p[ROWS][LPR];
  const int tid = threadIdx.x, r = tid / LPR, sub = tid % LPR;
  const int r0 = blockIdx.x * ROWS;
  const int64_t row = r0 + r;
  const bool live = row < p.n;
  float4 d = zero4(), o = d, s = d;
  if (live) {
    d = load4(p.d_out + row * p.ldd + 4 * sub);
    o = load4(p.o + row * p.ldo + 4 * sub);
    s = load4(p.skip + row * p.lds + 4 * sub);
  }
  const float4 w1 = load4(p.w_beta + 4 * sub), w2 = load4(p.w_beta + HC + 4 * sub), w3 = load4(p.w_beta + 2 * HC + 4 * sub);
  const float4 os = sub4(o, s);
  const TGroup gr = tgroup(LPR);
  const float a = tgroup_sum(dot4(w1, o) + dot4(w2, s) + dot4(w3, os), gr);
  const float b = sigmoid1(a);
  const float g = -tgroup_sum(dot4(d, os), gr) * (b * (1.0f - b));       // <d_out, S - O> b (1 - b); a dead row: 0
  if (live) {
    *reinterpret_cast<float4*>(p.d_o + row * p.ldgo + 4 * sub) = fma4(g, add4(w1, w3), scale4(1.0f - b, d));
    *reinterpret_cast<float4*>(p.d_s + row * p.ldgs + 4 * sub) = fma4(g, sub4(w2, w3), scale4(b, d));
  }
  // dw1 | dw2 | dw3: this tile's rows, in row order, one block after the other through the same LDS rows
  float* __restrict__ part = p.part + (int64_t)blockIdx.x * 3 * HC;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    s_p[r][sub] = scale4(g, q == 0 ? o : q == 1 ? s : os);
    __syncthreads();
    if (tid < LPR) {
      float4 v = zero4();
#pragma unroll 8
      for (int i = 0; i < ROWS; ++i) v = add4(v, s_p[i][tid]);
      *reinterpret_cast<float4*>(part + q * HC + 4 * tid) = v;
    }
    __syncthreads();
  }
}

// the tiles' parts [tiles][f] summed in a fixed order (gcnx_colpart_reduce_sum) into out [f]
__global__ __launch_bounds__(256) void transformer_part_reduce_kernel(const float* __restrict__ part, int64_t tiles, int32_t f,
                                                                      float* __restrict__ out) {
  __shared__ float4 s[128][2];
  const float4 v = gcnx_colpart_reduce_sum(part, tiles, f, blockIdx.x, s);
  const int c = blockIdx.x * 8 + (threadIdx.x & 1) * 4;
  if ((threadIdx.x >> 1) == 0 && c < f) *reinterpret_cast<float4*>(out + c) = v;
}

struct TFTargetArgs {
  const int32_t* rowptr; const int32_t* colidx;
  const float* p; int64_t ldp;
  int32_t n, heads, lph, edge_dim;
  const float* e; int64_t lde;
  const float* w_e;
  const float* alpha;
  const float* d_o; int64_t ldd;
  const float* o; int64_t ldo;                   // O (before the root connection)
  float scale;
  float* dscore;                                 // [nnz, heads]
  float* dq; int64_t ldg;                        // dQ [n, HC]
  float* ds; int64_t ldgs;                       // dS [n, HC] = d_o, or NULL
  float* part;                                   // [tiles][edge_dim HC]: this tile's dW_e
};

// ---- backward on the forward CSR: dscore per entry, dQ per target row, the copy dS = dO, the tile's part of dW_e ------------
template <int HC, int ROWS, int E>
__global__ __launch_bounds__(ROWS * HC / 4) void transformer_bwd_targets_kernel(TFTargetArgs p) {
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
  const EdgeW<E> we = load_edge_w<E>(p.w_e, ed, HC, sub);
  float4 dO = zero4(), O = dO, q = dO;
  if (live) {
    dO = load4(p.d_o + row * p.ldd + 4 * sub);
    O = load4(p.o + row * p.ldo + 4 * sub);
    q = load4(p.p + row * p.ldp + 4 * sub);
  }
  const TGroup gh = tgroup(lph);
  const float rr = tgroup_sum(dot4(dO, O), gh);         // = sum_k alpha_ik dalpha_ik: no second pass over the row
  const unsigned ld4 = (unsigned)p.ldp * 4u, koff = (unsigned)HC * 4u + (unsigned)sub * 16u, voff = koff + (unsigned)HC * 4u;
  const __amdgpu_buffer_rsrc_t pd = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.p, (short)0, (int)((unsigned)(p.n - 1) * ld4 + (unsigned)HC * 12u), 0x00020000);
  const int32_t* __restrict__ gcol = p.colidx + t.e0;
  const float* __restrict__ al = p.alpha + (int64_t)t.e0 * heads + h;
  float* __restrict__ dso = p.dscore + (int64_t)t.e0 * heads + h;
  float4 dq = zero4();
  TEdgeS<E> ab;
#pragma unroll
  for (int d = 0; d < (E > 0 ? E : 1); ++d) ab.a[d] = ab.b[d] = 0.f;
  for (int e = ea; e < eb; e += kTileU) {
    float4 kv[kTileU], vv[kTileU], tv[kTileU];
    EdgeF<E> ev[kTileU];
    float av[kTileU];
    int64_t en[kTileU];
#pragma unroll
    for (int u = 0; u < kTileU; ++u) {
      const bool ok = e + u < eb;
      const int ee = ok ? e + u : e;
      const int col = ee < kTileCap ? s_col[ee] : gcol[ee];
      kv[u] = buf4(pd, ok ? (unsigned)col * ld4 + koff : kOffOut);
      vv[u] = buf4(pd, ok ? (unsigned)col * ld4 + voff : kOffOut);
      en[u] = (int64_t)t.e0 + ee;
      av[u] = ok ? al[(int64_t)ee * heads] : 0.f;
    }
    tf_edge(tv, ev, p.e, p.lde, en, we, ed);
#pragma unroll
    for (int u = 0; u < kTileU; ++u) {
      const float d = tgroup_sum(dot4(dO, add4(vv[u], tv[u])), gh);
      const float dsc = av[u] * (d - rr);                // a slot past the row's end: alpha = 0, adds zeros below
      if (e + u < eb && k == 0) dso[(int64_t)(e + u) * heads] = dsc;
      dq = fma4(dsc, add4(kv[u], tv[u]), dq);          // CSR order
      tf_ab_from<0, E>(ab, ev[u], dsc, av[u], ed);
    }
  }
  if (live) {
    *reinterpret_cast<float4*>(p.dq + row * p.ldg + 4 * sub) = scale4(p.scale, dq);
    if (p.ds) *reinterpret_cast<float4*>(p.ds + row * p.ldgs + 4 * sub) = dO;
  }
  // dW_e[d]: s Q[i] A_i[d] + dO[i] B_i[d] of this tile's rows, in row order, one feature after the other through the same LDS rows
  if constexpr (E > 0) {
    float* __restrict__ part = p.part + (int64_t)(t.r0 / ROWS) * ed * HC;
    const float4 qs = scale4(p.scale, q);
#pragma unroll
    for (int d = 0; d < E; ++d) {
      if (d < ed) {                                      // (uniform)
        s_p[r][sub] = fma4(ab.a[d], qs, scale4(ab.b[d], dO));
        __syncthreads();
        if (tid < LPR) {
          float4 s = zero4();
#pragma unroll 8
          for (int i = 0; i < ROWS; ++i) s = add4(s, s_p[i][tid]);
          *reinterpret_cast<float4*>(part + d * HC + 4 * tid) = s;
        }
        __syncthreads();
      }
    }
  }
}

struct TFSourceArgs {
  const int32_t* rowptr; const int32_t* colidx; const int32_t* perm;     // the transposed pattern and its entry permutation
  const float* p; int64_t ldp;                                           // Q = its first HC columns
  int32_t n, heads, lph;
  const float* alpha; const float* dscore;                               // [nnz, heads], forward entry order
  const float* d_o; int64_t ldd;
  float scale;
  float* dkv; int64_t ldg;                                               // dK | dV [n, 2 HC]
};

// ---- backward on the transposed pattern: dK | dV per source row; reads neither e nor W_e -------------------------------------
template <int HC, int ROWS>
__global__ __launch_bounds__(ROWS * HC / 4) void transformer_bwd_sources_kernel(TFSourceArgs p) {
  constexpr int LPR = HC / 4, NT = ROWS * LPR;
  __shared__ int32_t s_col[kTileCap];
  __shared__ int32_t s_q[kTileCap];
  __shared__ int32_t s_rp[kTileRows + 1];
  const int tid = threadIdx.x, r = tid / LPR, sub = tid % LPR;
  const int heads = p.heads, h = sub / p.lph;
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
  const unsigned ldd4 = (unsigned)p.ldd * 4u, ldp4 = (unsigned)p.ldp * 4u, sub16 = (unsigned)sub * 16u;
  const __amdgpu_buffer_rsrc_t dd = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.d_o, (short)0, (int)((unsigned)(p.n - 1) * ldd4 + (unsigned)HC * 4u), 0x00020000);
  // Q = columns [0, HC) of P: the descriptor ends behind the last row's HC columns
  const __amdgpu_buffer_rsrc_t qd = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.p, (short)0, (int)((unsigned)(p.n - 1) * ldp4 + (unsigned)HC * 4u), 0x00020000);
  const int32_t* __restrict__ gcol = p.colidx + t.e0;
  const int32_t* __restrict__ gq = p.perm + t.e0;
  float4 dk = zero4(), dv = dk;
  for (int e = ea; e < eb; e += kTileU) {
    float4 dov[kTileU], qv[kTileU];
    float av[kTileU], zv[kTileU];
#pragma unroll
    for (int u = 0; u < kTileU; ++u) {
      const bool ok = e + u < eb;
      const int ee = ok ? e + u : e;
      const bool st = ee < kTileCap;
      const int col = st ? s_col[ee] : gcol[ee];
      const int64_t en = st ? s_q[ee] : gq[ee];
      dov[u] = buf4(dd, ok ? (unsigned)col * ldd4 + sub16 : kOffOut);
      qv[u] = buf4(qd, ok ? (unsigned)col * ldp4 + sub16 : kOffOut);
      av[u] = ok ? p.alpha[en * heads + h] : 0.f;
      zv[u] = ok ? p.dscore[en * heads + h] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kTileU; ++u) {
      if (e + u < eb) {
        dk = fma4(zv[u], qv[u], dk);                    // the transposed CSR's order
        dv = fma4(av[u], dov[u], dv);
      }
    }
  }
  if (live) {
    *reinterpret_cast<float4*>(p.dkv + row * p.ldg + 4 * sub) = scale4(p.scale, dk);
    *reinterpret_cast<float4*>(p.dkv + row * p.ldg + HC + 4 * sub) = dv;
  }
}

bool tf_hc_ok(int32_t hc) { return hc == 16 || hc == 32 || hc == 64 || hc == 128; }
bool tf_shape_ok(int64_t n, int32_t heads, int32_t c, int64_t ldp, int32_t edge_dim) {
  if (n < 0 || n > 0x7FFFFFFF || !(heads == 1 || heads == 2 || heads == 4 || heads == 8) || c < 4 || c > 128) return false;
  if (edge_dim < 0 || edge_dim > kEdgeMax) return false;
  const int hc = heads * c;
  return tf_hc_ok(hc) && ldp >= 3 * (int64_t)hc && ldp % 4 == 0 && (uint64_t)n * (uint64_t)ldp * 4u < 0x100000000ull;
}
float tf_scale(int32_t c) { return (float)(1.0 / std::sqrt((double)c)); }

const char* kTFShapes = "needs heads in {1, 2, 4, 8}, heads * c in {16, 32, 64, 128}, c >= 4, ldp >= 3 * heads * c in multiples of 4 "
                        "floats, n * ldp * 4 < 2^32 and 0 <= edge_dim <= 8";

// the kernels that read no edge features: LAUNCH(width, rows) as GCNX_CONV_DISPATCH picks them
#define GCNX_TF_DISPATCH_HC(hc, LAUNCH)                                                         \
  do {                                                                                          \
    if ((hc) == 128) { LAUNCH(128, 16); } else if ((hc) == 64) { LAUNCH(64, 32); } else if ((hc) == 32) { LAUNCH(32, 32); } \
    else { LAUNCH(16, 32); }                                                                    \
  } while (0)

}  // namespace

extern "C" {

int gcnx_transformer_conv_ok(int64_t n, int32_t heads, int32_t c, int64_t ldp, int32_t edge_dim) {
  return tf_shape_ok(n, heads, c, ldp, edge_dim) ? 1 : 0;
}

int gcnx_transformer_bwd_scratch_floats(int64_t n, int32_t heads, int32_t c, int32_t edge_dim, int32_t beta, int64_t* out) {
  if (!out) return gcnx_fail(nullptr, GCNX_ERR_INVALID, "gcnx_transformer_bwd_scratch_floats: out is NULL");
  if (n < 0 || heads <= 0 || c <= 0 || edge_dim < 0)
    return gcnx_fail(nullptr, GCNX_ERR_INVALID, "gcnx_transformer_bwd_scratch_floats: needs n >= 0, heads > 0, c > 0 and edge_dim >= 0");
  const int64_t hc = (int64_t)heads * c;
  const int64_t per = edge_dim > (beta ? 3 : 0) ? edge_dim : (beta ? 3 : 0);       // the two calls use it one after the other
  *out = (int64_t)gcnx_cdiv(n, conv_tile_rows((int)hc)) * per * hc;
  return GCNX_OK;
}

int gcnx_transformer_aggregate(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* p, int64_t ldp, int32_t n,
                               int32_t heads, int32_t c, const float* e, int64_t lde, int32_t edge_dim, const float* w_e,
                               const float* skip, int64_t lds, const float* w_beta, float* out, int64_t ldo, float* alpha, float* o_pre,
                               int64_t ldpre) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "TransformerConv aggregate");
  GCNX_REQUIRE(ctx, n >= 0 && heads >= 0 && c >= 0 && edge_dim >= 0, "gcnx_transformer_aggregate: negative size");
  GCNX_REQUIRE(ctx, !w_beta || skip, "gcnx_transformer_aggregate: w_beta needs skip");
  if (!tf_shape_ok(n, heads, c, ldp, edge_dim))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_transformer_aggregate: %s (got n=%d heads=%d c=%d ldp=%lld edge_dim=%d)", kTFShapes,
                     n, heads, c, (long long)ldp, edge_dim);
  const int hc = heads * c;
  if (!gcnx_aligned16(p) || !gcnx_aligned16(w_e) || !gcnx_aligned16(skip) || !gcnx_aligned16(w_beta) || !gcnx_aligned16(out) ||
      !gcnx_aligned16(o_pre) || !conv_ld_ok(ldo, hc) || (skip && !conv_ld_ok(lds, hc)) || (o_pre && !conv_ld_ok(ldpre, hc)))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_transformer_aggregate: p, w_e, skip, w_beta, out and o_pre must be 16-byte aligned, "
                     "with ldo, lds and ldpre >= heads * c in multiples of 4 floats");
  if (n == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, rowptr && colidx && p && out, "gcnx_transformer_aggregate: NULL pointer");
  GCNX_REQUIRE(ctx, edge_dim == 0 || (e && w_e && lde >= edge_dim), "gcnx_transformer_aggregate: edge_dim > 0 needs e (lde >= edge_dim) and w_e");
  GCNX_REQUIRE(ctx, p != out && p != o_pre && out != o_pre && skip != out && (!skip || skip != o_pre),
               "gcnx_transformer_aggregate: the outputs must not alias p, skip or each other");
  TFFwdArgs a{};
  a.rowptr = rowptr; a.colidx = colidx; a.p = p; a.ldp = ldp; a.n = n; a.heads = heads; a.lph = c / 4; a.edge_dim = edge_dim;
  a.e = e; a.lde = lde; a.w_e = w_e; a.skip = skip; a.lds = lds; a.w_beta = w_beta; a.scale = tf_scale(c); a.out = out; a.ldo = ldo;
  a.alpha = alpha; a.o_pre = o_pre; a.ldpre = ldpre;
  const int tiles = gcnx_cdiv(n, conv_tile_rows(hc));
  const size_t dyn = alpha ? (size_t)kTileCap * heads * sizeof(float) : 0;
#define GCNX_TF_AGG(HC_, R_, E_) \
  hipLaunchKernelGGL((transformer_aggregate_kernel<HC_, R_, E_>), dim3(tiles), dim3(R_ * HC_ / 4), dyn, ctx->stream, a)
  GCNX_CONV_DISPATCH(hc, edge_dim, GCNX_TF_AGG);
#undef GCNX_TF_AGG
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

int gcnx_transformer_beta_bwd(gcnx_ctx* ctx, const float* d_out, int64_t ldd, const float* o, int64_t ldo, const float* skip, int64_t lds,
                              const float* w_beta, int32_t n, int32_t hc, float* d_o, int64_t ldgo, float* d_s, int64_t ldgs,
                              float* dw_beta, float* scratch) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "TransformerConv backward (beta gate)");
  GCNX_REQUIRE(ctx, n >= 0 && hc >= 0, "gcnx_transformer_beta_bwd: negative size");
  if (!tf_hc_ok(hc))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_transformer_beta_bwd: needs hc in {16, 32, 64, 128} (got %d)", hc);
  if (!gcnx_aligned16(d_out) || !gcnx_aligned16(o) || !gcnx_aligned16(skip) || !gcnx_aligned16(w_beta) || !gcnx_aligned16(d_o) ||
      !gcnx_aligned16(d_s) || !gcnx_aligned16(dw_beta) || !gcnx_aligned16(scratch) || !conv_ld_ok(ldd, hc) || !conv_ld_ok(ldo, hc) ||
      !conv_ld_ok(lds, hc) || !conv_ld_ok(ldgo, hc) || !conv_ld_ok(ldgs, hc))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_transformer_beta_bwd: d_out, o, skip, w_beta, d_o, d_s, dw_beta and scratch must be "
                     "16-byte aligned, with ldd, ldo, lds, ldgo and ldgs >= hc in multiples of 4 floats");
  if (n == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, d_out && o && skip && w_beta && d_o && d_s && dw_beta && scratch, "gcnx_transformer_beta_bwd: NULL pointer");
  GCNX_REQUIRE(ctx, d_o != d_out && d_o != o && d_o != skip && d_s != d_out && d_s != o && d_s != skip && d_o != d_s,
               "gcnx_transformer_beta_bwd: d_o and d_s must not alias d_out, o, skip or each other");
  TFBetaArgs a{};
  a.d_out = d_out; a.ldd = ldd; a.o = o; a.ldo = ldo; a.skip = skip; a.lds = lds; a.w_beta = w_beta; a.n = n; a.d_o = d_o; a.ldgo = ldgo;
  a.d_s = d_s; a.ldgs = ldgs; a.part = scratch;
  const int tiles = gcnx_cdiv(n, conv_tile_rows(hc));
#define GCNX_TF_BB(HC_, R_) hipLaunchKernelGGL((transformer_beta_bwd_kernel<HC_, R_>), dim3(tiles), dim3(R_ * HC_ / 4), 0, ctx->stream, a)
  GCNX_TF_DISPATCH_HC(hc, GCNX_TF_BB);
#undef GCNX_TF_BB
  GCNX_LAUNCH_OK(ctx);
  hipLaunchKernelGGL(transformer_part_reduce_kernel, dim3(gcnx_cdiv(3 * hc, 8)), dim3(256), 0, ctx->stream, (const float*)scratch,
                     (int64_t)tiles, 3 * hc, dw_beta);
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

int gcnx_transformer_bwd_targets(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* p, int64_t ldp, int32_t n,
                                 int32_t heads, int32_t c, const float* e, int64_t lde, int32_t edge_dim, const float* w_e,
                                 const float* alpha, const float* d_o, int64_t ldd, const float* o, int64_t ldo, float* dscore, float* dq,
                                 int64_t ldg, float* ds, int64_t ldgs, float* dw_e, float* scratch) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "TransformerConv backward (targets)");
  GCNX_REQUIRE(ctx, n >= 0 && heads >= 0 && c >= 0 && edge_dim >= 0, "gcnx_transformer_bwd_targets: negative size");
  if (!tf_shape_ok(n, heads, c, ldp, edge_dim))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_transformer_bwd_targets: %s (got n=%d heads=%d c=%d ldp=%lld edge_dim=%d)", kTFShapes,
                     n, heads, c, (long long)ldp, edge_dim);
  const int hc = heads * c;
  if (!gcnx_aligned16(p) || !gcnx_aligned16(w_e) || !gcnx_aligned16(d_o) || !gcnx_aligned16(o) || !gcnx_aligned16(dq) ||
      !gcnx_aligned16(ds) || !gcnx_aligned16(dw_e) || !gcnx_aligned16(scratch) || !conv_ld_ok(ldd, hc) || !conv_ld_ok(ldo, hc) ||
      !conv_ld_ok(ldg, hc) || (ds && !conv_ld_ok(ldgs, hc)))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_transformer_bwd_targets: p, w_e, d_o, o, dq, ds, dw_e and scratch must be 16-byte "
                     "aligned, with ldd, ldo, ldg and ldgs >= heads * c in multiples of 4 floats");
  if (n == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, rowptr && colidx && p && alpha && d_o && o && dscore && dq, "gcnx_transformer_bwd_targets: NULL pointer");
  GCNX_REQUIRE(ctx, edge_dim == 0 || (e && w_e && dw_e && scratch && lde >= edge_dim),
               "gcnx_transformer_bwd_targets: edge_dim > 0 needs e (lde >= edge_dim), w_e, dw_e and scratch");
  GCNX_REQUIRE(ctx, dq != d_o && dq != o && dq != p && ds != d_o && ds != o && ds != p && (!ds || ds != dq),
               "gcnx_transformer_bwd_targets: dq and ds must not alias d_o, o, p or each other");
  TFTargetArgs a{};
  a.rowptr = rowptr; a.colidx = colidx; a.p = p; a.ldp = ldp; a.n = n; a.heads = heads; a.lph = c / 4; a.edge_dim = edge_dim;
  a.e = e; a.lde = lde; a.w_e = w_e; a.alpha = alpha; a.d_o = d_o; a.ldd = ldd; a.o = o; a.ldo = ldo; a.scale = tf_scale(c);
  a.dscore = dscore; a.dq = dq; a.ldg = ldg; a.ds = ds; a.ldgs = ldgs; a.part = scratch;
  const int tiles = gcnx_cdiv(n, conv_tile_rows(hc));
#define GCNX_TF_BT(HC_, R_, E_) \
  hipLaunchKernelGGL((transformer_bwd_targets_kernel<HC_, R_, E_>), dim3(tiles), dim3(R_ * HC_ / 4), 0, ctx->stream, a)
  GCNX_CONV_DISPATCH(hc, edge_dim, GCNX_TF_BT);
#undef GCNX_TF_BT
  GCNX_LAUNCH_OK(ctx);
  if (edge_dim > 0) {
    hipLaunchKernelGGL(transformer_part_reduce_kernel, dim3(edge_dim * hc / 8), dim3(256), 0, ctx->stream, (const float*)scratch,
                       (int64_t)tiles, edge_dim * hc, dw_e);
    GCNX_LAUNCH_OK(ctx);
  }
  return GCNX_OK;
}

int gcnx_transformer_bwd_sources(gcnx_ctx* ctx, const int32_t* rowptr_t, const int32_t* colidx_t, const int32_t* perm_t, const float* p,
                                 int64_t ldp, int32_t n, int32_t heads, int32_t c, const float* alpha, const float* dscore,
                                 const float* d_o, int64_t ldd, float* dkv, int64_t ldg) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "TransformerConv backward (sources)");
  GCNX_REQUIRE(ctx, n >= 0 && heads >= 0 && c >= 0, "gcnx_transformer_bwd_sources: negative size");
  if (!tf_shape_ok(n, heads, c, ldp, 0))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_transformer_bwd_sources: %s (got n=%d heads=%d c=%d ldp=%lld)", kTFShapes, n, heads,
                     c, (long long)ldp);
  const int hc = heads * c;
  if (!gcnx_aligned16(p) || !gcnx_aligned16(d_o) || !gcnx_aligned16(dkv) || !conv_ld_ok(ldd, hc) || !conv_ld_ok(ldg, 2 * hc) ||
      !gcnx_fits_buffer(n, ldd, 4))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_transformer_bwd_sources: p, d_o and dkv must be 16-byte aligned, with ldd >= heads * c "
                     "and ldg >= 2 * heads * c in multiples of 4 floats and n * ldd * 4 < 2^32");
  if (n == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, rowptr_t && colidx_t && perm_t && p && alpha && dscore && d_o && dkv, "gcnx_transformer_bwd_sources: NULL pointer");
  GCNX_REQUIRE(ctx, dkv != d_o && dkv != p, "gcnx_transformer_bwd_sources: dkv must not alias d_o or p");
  TFSourceArgs a{};
  a.rowptr = rowptr_t; a.colidx = colidx_t; a.perm = perm_t; a.p = p; a.ldp = ldp; a.n = n; a.heads = heads; a.lph = c / 4;
  a.alpha = alpha; a.dscore = dscore; a.d_o = d_o; a.ldd = ldd; a.scale = tf_scale(c); a.dkv = dkv; a.ldg = ldg;
  const int tiles = gcnx_cdiv(n, conv_tile_rows(hc));
#define GCNX_TF_BS(HC_, R_) hipLaunchKernelGGL((transformer_bwd_sources_kernel<HC_, R_>), dim3(tiles), dim3(R_ * HC_ / 4), 0, ctx->stream, a)
  GCNX_TF_DISPATCH_HC(hc, GCNX_TF_BS);
#undef GCNX_TF_BS
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

}  // extern "C"
