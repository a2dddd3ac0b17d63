// ResGatedGraphConv (Bresson & Laurent's GatedGCN as PyG ships it: ResGatedGraphConv(in, H, act = Sigmoid(), edge_dim = D,
// root_weight, bias), aggr = add) in the small-feature regime (H <= 128): every message is multiplied channel by channel by a
// sigmoid gate that reads target, source and edge together.  No softmax: a row's messages do not compete.  Row i of the CSR is
// the target, its stored entries j the sources, values ignored; P = K | Q | V (| S) [n, 3 H (4 H)] is ONE array (one gcnx_gemm
// with the stacked weight), w_e [edge_dim, 3 H] = W_ke | W_qe | W_ve:
//
//     a_ij = K[i] + Q[j] + sum_d e_ij[d] (W_ke[d] + W_qe[d])     g_ij = sigmoid(a_ij)     m_ij = V[j] + sum_d e_ij[d] W_ve[d]
//     out[i] = S[i] + bias + sum_j g_ij * m_ij                                                                resgated_aggregate
//     da_ij = dO[i] m_ij g_ij (1 - g_ij)    dm_ij = dO[i] g_ij
//     dK[i] = sum_j da_ij    dS = dO    dW_ke[d] = dW_qe[d] = sum_ij e_ij[d] da_ij    dW_ve[d] = sum_ij e_ij[d] dm_ij      resgated_bwd_targets
//     dQ[j] = sum_i da_ij    dV[j] = sum_i dm_ij                                                              resgated_bwd_sources
//
// Nobody stores g or m (nnz H floats each): the backward kernels recompute them.  The sigmoid has no kink, so the kernels need
// not agree on it bit for bit (gatv2.hip's separately rounded expression is not needed here): products and adds contract
// into FMAs.  sigmoid(a) = 1 / (1 + exp(-a)): exp(-a) overflows to +inf for a < -88 and the reciprocal of +inf is 0, it
// underflows to 0 for a > 88 and g = 1 -- g in [0, 1] and g (1 - g) finite (0 at both ends) for every finite a, no 0 * inf.
// fp32 throughout, no float atomics, every sum in a fixed order: the same call leaves the same bits.
//
// Shape of a workgroup (gatv2.hip's; the device helpers they share: conv_tile.h): 32 rows, one lane group of H / 4 lanes per
// row with one float4 of the row each -- 8 H threads (H = 128: 16 rows, see conv_tile_rows: the two blocks of W_e, their
// gradients and a trip's operands do not fit beside 32 rows).  The tile's CSR entries are
// staged in LDS (1024 of them; a tile with more reads the rest from global memory).  Q[j] | V[j] are adjacent in P: one
// entry costs one contiguous 2 H piece of row j, gathered with range-checked buffer loads -- slots past a row's end fetch
// nothing.  W_ke + W_qe (summed as they are loaded) and W_ve sit in registers: 2 E float4 per lane in the kernel built for
// up to E in {0, 2, 8} edge features, addressed under nested uniform tests d < edge_dim (no indexed register array).
#include <cmath>

#include "common.h"
#include "conv_tile.h"

namespace {

__device__ __forceinline__ float4 rg_sig(float4 a) { return make_float4(sigmoid1(a.x), sigmoid1(a.y), sigmoid1(a.z), sigmoid1(a.w)); }
// g (1 - g): 0 at g = 0 and at g = 1
__device__ __forceinline__ float4 rg_dsig(float4 g) {
  return make_float4(g.x * (1.0f - g.x), g.y * (1.0f - g.y), g.z * (1.0f - g.z), g.w * (1.0f - g.w));
}

// w_e [edge_dim, 3 H] = W_ke | W_qe | W_ve: this lane's float4 of the summed gate block and of the value block of every row,
// rows >= edge_dim zero and never used
template <int E> struct RGEdgeW { float4 g[E > 0 ? E : 1]; float4 v[E > 0 ? E : 1]; };
template <int E>
__device__ __forceinline__ RGEdgeW<E> rg_load_we(const float* __restrict__ w_e, int edge_dim, int h, int sub) {
  RGEdgeW<E> r;
  r.g[0] = zero4();
  r.v[0] = zero4();
#pragma unroll
  for (int d = 0; d < E; ++d) {
    const float* row = w_e + (int64_t)d * 3 * h + 4 * sub;
    r.g[d] = d < edge_dim ? add4(load4(row), load4(row + h)) : zero4();
    r.v[d] = d < edge_dim ? load4(row + 2 * h) : zero4();
  }
  return r;
}
// a += e (W_ke + W_qe), m += e W_ve for the U entries of a trip, d ascending; ok[u] = false: the features read as zeros.
// Feature d is loaded and used inside the (uniform) test of feature d - 1, so a trip costs edge_dim + 1 branches and every
// register index is a constant.  The features stay in r for the kernel that needs them again (dw_e).
template <int Dd, int E, int U>
__device__ __forceinline__ void rg_edge_from(float4 (&a)[U], float4 (&m)[U], EdgeF<E> (&r)[U], const float* __restrict__ e, int64_t lde,
                                             const int64_t (&entry)[U], const bool (&ok)[U], const RGEdgeW<E>& w, int edge_dim) {
  if constexpr (Dd < E) {
    if (Dd < edge_dim) {
#pragma unroll
      for (int u = 0; u < U; ++u) r[u].v[Dd] = ok[u] ? e[entry[u] * lde + Dd] : 0.f;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        a[u] = fma4(r[u].v[Dd], w.g[Dd], a[u]);
        m[u] = fma4(r[u].v[Dd], w.v[Dd], m[u]);
      }
      rg_edge_from<Dd + 1, E, U>(a, m, r, e, lde, entry, ok, w, edge_dim);
    }
  }
}
template <int E, int U>
__device__ __forceinline__ void rg_edge(float4 (&a)[U], float4 (&m)[U], EdgeF<E> (&r)[U], const float* __restrict__ e, int64_t lde,
                                        const int64_t (&entry)[U], const bool (&ok)[U], const RGEdgeW<E>& w, int edge_dim) {
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int d = 0; d < (E > 0 ? E : 1); ++d) r[u].v[d] = 0.f;
  rg_edge_from<0, E, U>(a, m, r, e, lde, entry, ok, w, edge_dim);
}
// dW_ke + dW_qe's common block += e (x) da, dW_ve += e (x) dm of one entry (nested the same way)
template <int Dd, int E>
__device__ __forceinline__ void rg_dwe_from(RGEdgeW<E>& dwe, const EdgeF<E>& e, float4 da, float4 dm, int edge_dim) {
  if constexpr (Dd < E) {
    if (Dd < edge_dim) {
      dwe.g[Dd] = fma4(e.v[Dd], da, dwe.g[Dd]);
      dwe.v[Dd] = fma4(e.v[Dd], dm, dwe.v[Dd]);
      rg_dwe_from<Dd + 1, E>(dwe, e, da, dm, edge_dim);
    }
  }
}

struct RGFwdArgs {
  const int32_t* rowptr; const int32_t* colidx;
  const float* p; int64_t ldp;                   // K | Q | V
  int32_t n, edge_dim;
  const float* e; int64_t lde;                   // [nnz, edge_dim] (edge_dim = 0: unused)
  const float* w_e;
  const float* skip; int64_t lds;                // S, or NULL
  const float* bias;
  float* out; int64_t ldo;
};

// ---- gates, messages and their sum from ONE gather of Q[j] | V[j] ----------------------------------------------------------
template <int H, int ROWS, int E>
__global__ __launch_bounds__(ROWS * H / 4) void resgated_aggregate_kernel(RGFwdArgs p) {
  constexpr int LPR = H / 4, NT = ROWS * LPR;
  __shared__ int32_t s_col[kTileCap];
  __shared__ int32_t s_rp[kTileRows + 1];
  const int tid = threadIdx.x, r = tid / LPR, sub = tid % LPR, ed = p.edge_dim;
  const ConvTile t = conv_tile(p.rowptr, p.n, s_rp, ROWS);
  const int staged = min(t.e1 - t.e0, kTileCap);
  for (int i = tid; i < staged; i += NT) s_col[i] = p.colidx[t.e0 + i];
  __syncthreads();
  const bool live = r < t.nr;
  const int ea = live ? s_rp[r] - t.e0 : 0, eb = live ? s_rp[r + 1] - t.e0 : 0;
  const int64_t row = t.r0 + r;
  const int32_t* __restrict__ gcol = p.colidx + t.e0;
  const RGEdgeW<E> we = rg_load_we<E>(p.w_e, ed, H, sub);
  const float4 k = live ? load4(p.p + row * p.ldp + 4 * sub) : zero4();
  const unsigned ld4 = (unsigned)p.ldp * 4u, qoff = (unsigned)H * 4u + (unsigned)sub * 16u, voff = qoff + (unsigned)H * 4u;
  // the descriptor ends behind the last row's 3 H columns (nothing past them is addressed)
  const __amdgpu_buffer_rsrc_t pd = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.p, (short)0, (int)((unsigned)(p.n - 1) * ld4 + (unsigned)H * 12u), 0x00020000);
  float4 acc = zero4();
  for (int e = ea; e < eb; e += kTileU) {
    float4 av[kTileU], mv[kTileU];
    EdgeF<E> ev[kTileU];
    int64_t en[kTileU];
    bool ok[kTileU];
#pragma unroll
    for (int u = 0; u < kTileU; ++u) {
      ok[u] = e + u < eb;
      const int ee = ok[u] ? e + u : e;
      const int col = ee < kTileCap ? s_col[ee] : gcol[ee];
      av[u] = buf4(pd, ok[u] ? (unsigned)col * ld4 + qoff : kOffOut);
      mv[u] = buf4(pd, ok[u] ? (unsigned)col * ld4 + voff : kOffOut);
      en[u] = (int64_t)t.e0 + ee;
    }
#pragma unroll
    for (int u = 0; u < kTileU; ++u) av[u] = add4(k, av[u]);
    rg_edge(av, mv, ev, p.e, p.lde, en, ok, we, ed);
#pragma unroll
    for (int u = 0; u < kTileU; ++u)
      if (e + u < eb) acc = fma44(rg_sig(av[u]), mv[u], acc);     // CSR order
  }
  if (!live) return;
  float4 y = acc;                                        // a row without entries: S + bias
  if (p.skip) y = add4(load4(p.skip + row * p.lds + 4 * sub), y);
  if (p.bias) y = add4(y, load4(p.bias + 4 * sub));
  *reinterpret_cast<float4*>(p.out + row * p.ldo + 4 * sub) = y;
}

struct RGTargetArgs {
  const int32_t* rowptr; const int32_t* colidx;
  const float* p; int64_t ldp;
  int32_t n, edge_dim;
  const float* e; int64_t lde;
  const float* w_e;
  const float* d_out; int64_t ldd;
  float* dk; int64_t ldg;                        // dK [n, H]
  float* ds; int64_t ldgs;                       // dS [n, H] = d_out, or NULL
  float* part;                                   // [tiles][2 edge_dim H]: this tile's gate blocks, then its value blocks
};

// ---- backward on the forward CSR: dK per target row, the copy dS = dO, the tile's part of dW_e ------------------------------
template <int H, int ROWS, int E>
__global__ __launch_bounds__(ROWS * H / 4) void resgated_bwd_targets_kernel(RGTargetArgs p) {
  constexpr int LPR = H / 4, NT = ROWS * LPR;
  __shared__ int32_t s_col[kTileCap];
  __shared__ int32_t s_rp[kTileRows + 1];
  __shared__ __attribute__((aligned(16))) float4 s_p[ROWS][LPR];
  const int tid = threadIdx.x, r = tid / LPR, sub = tid % LPR, ed = p.edge_dim;
  const ConvTile t = conv_tile(p.rowptr, p.n, s_rp, ROWS);
  const int staged = min(t.e1 - t.e0, kTileCap);
  for (int i = tid; i < staged; i += NT) s_col[i] = p.colidx[t.e0 + i];
  __syncthreads();
  const bool live = r < t.nr;
  const int ea = live ? s_rp[r] - t.e0 : 0, eb = live ? s_rp[r + 1] - t.e0 : 0;
  const int64_t row = t.r0 + r;
  const int32_t* __restrict__ gcol = p.colidx + t.e0;
  const RGEdgeW<E> we = rg_load_we<E>(p.w_e, ed, H, sub);
  float4 dO = zero4(), k = dO;
  if (live) {
    dO = load4(p.d_out + row * p.ldd + 4 * sub);
    k = load4(p.p + row * p.ldp + 4 * sub);
  }
  const unsigned ld4 = (unsigned)p.ldp * 4u, qoff = (unsigned)H * 4u + (unsigned)sub * 16u, voff = qoff + (unsigned)H * 4u;
  const __amdgpu_buffer_rsrc_t pd = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.p, (short)0, (int)((unsigned)(p.n - 1) * ld4 + (unsigned)H * 12u), 0x00020000);
  float4 dk = zero4();
  RGEdgeW<E> dwe;
#pragma unroll
  for (int d = 0; d < (E > 0 ? E : 1); ++d) dwe.g[d] = dwe.v[d] = zero4();
  for (int e = ea; e < eb; e += kTileU) {
    float4 av[kTileU], mv[kTileU];
    EdgeF<E> ev[kTileU];
    int64_t en[kTileU];
    bool ok[kTileU];
#pragma unroll
    for (int u = 0; u < kTileU; ++u) {
      ok[u] = e + u < eb;
      const int ee = ok[u] ? e + u : e;
      const int col = ee < kTileCap ? s_col[ee] : gcol[ee];
      av[u] = buf4(pd, ok[u] ? (unsigned)col * ld4 + qoff : kOffOut);
      mv[u] = buf4(pd, ok[u] ? (unsigned)col * ld4 + voff : kOffOut);
      en[u] = (int64_t)t.e0 + ee;
    }
#pragma unroll
    for (int u = 0; u < kTileU; ++u) av[u] = add4(k, av[u]);
    rg_edge(av, mv, ev, p.e, p.lde, en, ok, we, ed);
#pragma unroll
    for (int u = 0; u < kTileU; ++u) {
      if (e + u < eb) {
        const float4 g = rg_sig(av[u]);
        const float4 dm = mul4(dO, g);
        const float4 da = mul4(mul4(dO, mv[u]), rg_dsig(g));
        dk = add4(dk, da);                              // CSR order
        rg_dwe_from<0, E>(dwe, ev[u], da, dm, ed);
      }
    }
  }
  if (live) {
    *reinterpret_cast<float4*>(p.dk + row * p.ldg + 4 * sub) = dk;
    if (p.ds) *reinterpret_cast<float4*>(p.ds + row * p.ldgs + 4 * sub) = dO;
  }
  // dW_e: this tile's rows, in row order, one block after the other through the same LDS rows
  if constexpr (E > 0) {
    float* __restrict__ part = p.part + (int64_t)(t.r0 / ROWS) * 2 * ed * H;
#pragma unroll
    for (int q = 0; q < 2 * E; ++q) {
      const int d = q < E ? q : q - E;
      if (d < ed) {                                      // (uniform)
        s_p[r][sub] = q < E ? dwe.g[d] : dwe.v[d];
        __syncthreads();
        if (tid < LPR) {
          float4 s = zero4();
#pragma unroll 8
          for (int i = 0; i < ROWS; ++i) s = add4(s, s_p[i][tid]);
          *reinterpret_cast<float4*>(part + ((q < E ? 0 : ed) + d) * H + 4 * tid) = s;
        }
        __syncthreads();
      }
    }
  }
}

// the tiles' parts summed in a fixed order (gcnx_colpart_reduce_sum): block q < edge_dim of a part is the gate block of
// feature q -- written to W_ke's AND W_qe's gradient --, block edge_dim + d the value block of feature d
__global__ __launch_bounds__(256) void resgated_part_reduce_kernel(const float* __restrict__ part, int64_t tiles, int32_t h, int32_t edge_dim,
                                                                   float* __restrict__ dw_e) {
  __shared__ float4 s[128][2];
  const int f = 2 * edge_dim * h;
  const float4 v = gcnx_colpart_reduce_sum(part, tiles, f, blockIdx.x, s);
  const int c = blockIdx.x * 8 + (threadIdx.x & 1) * 4;
  if ((threadIdx.x >> 1) == 0 && c < f) {
    const int q = c / h, w = c % h;
    if (q < edge_dim) {
      *reinterpret_cast<float4*>(dw_e + (int64_t)q * 3 * h + w) = v;
      *reinterpret_cast<float4*>(dw_e + (int64_t)q * 3 * h + h + w) = v;
    } else {
      *reinterpret_cast<float4*>(dw_e + (int64_t)(q - edge_dim) * 3 * h + 2 * h + w) = v;
    }
  }
}

struct RGSourceArgs {
  const int32_t* rowptr; const int32_t* colidx; const int32_t* perm;     // the transposed pattern and its entry permutation
  const float* p; int64_t ldp;
  int32_t n, edge_dim;
  const float* e; int64_t lde;                                           // forward entry order
  const float* w_e;
  const float* d_out; int64_t ldd;
  float* dqv; int64_t ldg;                                               // dQ | dV [n, 2 H]
};

// ---- backward on the transposed pattern: dQ | dV per source row ---------------------------------------------------------------
template <int H, int ROWS, int E>
__global__ __launch_bounds__(ROWS * H / 4) void resgated_bwd_sources_kernel(RGSourceArgs p) {
  constexpr int LPR = H / 4, NT = ROWS * LPR;
  __shared__ int32_t s_col[kTileCap];
  __shared__ int32_t s_q[kTileCap];
  __shared__ int32_t s_rp[kTileRows + 1];
  const int tid = threadIdx.x, r = tid / LPR, sub = tid % LPR, ed = p.edge_dim;
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
  const RGEdgeW<E> we = rg_load_we<E>(p.w_e, ed, H, sub);
  float4 q = zero4(), v = q;
  if (live) {
    q = load4(p.p + row * p.ldp + H + 4 * sub);
    v = load4(p.p + row * p.ldp + 2 * H + 4 * sub);
  }
  const unsigned ldd4 = (unsigned)p.ldd * 4u, ldp4 = (unsigned)p.ldp * 4u, sub16 = (unsigned)sub * 16u;
  const __amdgpu_buffer_rsrc_t dd = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.d_out, (short)0, (int)((unsigned)(p.n - 1) * ldd4 + (unsigned)H * 4u), 0x00020000);
  // K = columns [0, H) of P: the descriptor ends behind the last row's H columns
  const __amdgpu_buffer_rsrc_t kd = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.p, (short)0, (int)((unsigned)(p.n - 1) * ldp4 + (unsigned)H * 4u), 0x00020000);
  const int32_t* __restrict__ gcol = p.colidx + t.e0;
  const int32_t* __restrict__ gq = p.perm + t.e0;
  float4 dq = zero4(), dv = dq;
  for (int e = ea; e < eb; e += kTileU) {
    float4 dov[kTileU], av[kTileU], mv[kTileU];
    EdgeF<E> ev[kTileU];
    int64_t en[kTileU];
    bool ok[kTileU];
#pragma unroll
    for (int u = 0; u < kTileU; ++u) {
      ok[u] = e + u < eb;
      const int ee = ok[u] ? e + u : e;
      const bool st = ee < kTileCap;
      const int col = st ? s_col[ee] : gcol[ee];
      en[u] = st ? s_q[ee] : gq[ee];
      dov[u] = buf4(dd, ok[u] ? (unsigned)col * ldd4 + sub16 : kOffOut);
      av[u] = buf4(kd, ok[u] ? (unsigned)col * ldp4 + sub16 : kOffOut);
    }
#pragma unroll
    for (int u = 0; u < kTileU; ++u) {
      av[u] = add4(av[u], q);
      mv[u] = v;
    }
    rg_edge(av, mv, ev, p.e, p.lde, en, ok, we, ed);
#pragma unroll
    for (int u = 0; u < kTileU; ++u) {
      if (e + u < eb) {
        const float4 g = rg_sig(av[u]);
        dv = fma44(dov[u], g, dv);                      // the transposed CSR's order
        dq = fma44(mul4(dov[u], mv[u]), rg_dsig(g), dq);
      }
    }
  }
  if (live) {
    *reinterpret_cast<float4*>(p.dqv + row * p.ldg + 4 * sub) = dq;
    *reinterpret_cast<float4*>(p.dqv + row * p.ldg + H + 4 * sub) = dv;
  }
}

bool rg_shape_ok(int64_t n, int32_t h, int64_t ldp, int32_t edge_dim) {
  if (n < 0 || n > 0x7FFFFFFF || !(h == 16 || h == 32 || h == 64 || h == 128)) return false;
  if (edge_dim < 0 || edge_dim > kEdgeMax) return false;
  return ldp >= 3 * (int64_t)h && ldp % 4 == 0 && (uint64_t)n * (uint64_t)ldp * 4u < 0x100000000ull;
}

const char* kRGShapes = "needs h in {16, 32, 64, 128}, ldp >= 3 h in multiples of 4 floats, n * ldp * 4 < 2^32 and 0 <= edge_dim <= 8";

}  // namespace

extern "C" {

int gcnx_resgated_conv_ok(int64_t n, int32_t h, int64_t ldp, int32_t edge_dim) { return rg_shape_ok(n, h, ldp, edge_dim) ? 1 : 0; }

int gcnx_resgated_bwd_scratch_floats(int64_t n, int32_t h, int32_t edge_dim, int64_t* out) {
  if (!out) return gcnx_fail(nullptr, GCNX_ERR_INVALID, "gcnx_resgated_bwd_scratch_floats: out is NULL");
  if (n < 0 || h <= 0 || edge_dim < 0)
    return gcnx_fail(nullptr, GCNX_ERR_INVALID, "gcnx_resgated_bwd_scratch_floats: needs n >= 0, h > 0 and edge_dim >= 0");
  *out = (int64_t)gcnx_cdiv(n, conv_tile_rows(h)) * 2 * edge_dim * h;
  return GCNX_OK;
}

int gcnx_resgated_aggregate(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* p, int64_t ldp, int32_t n,
                            int32_t h, const float* e, int64_t lde, int32_t edge_dim, const float* w_e, const float* skip, int64_t lds,
                            const float* bias, float* out, int64_t ldo) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "ResGatedGraphConv aggregate");
  GCNX_REQUIRE(ctx, n >= 0 && h >= 0 && edge_dim >= 0, "gcnx_resgated_aggregate: negative size");
  if (!rg_shape_ok(n, h, ldp, edge_dim))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_resgated_aggregate: %s (got n=%d h=%d ldp=%lld edge_dim=%d)", kRGShapes, n, h,
                     (long long)ldp, edge_dim);
  if (!gcnx_aligned16(p) || !gcnx_aligned16(w_e) || !gcnx_aligned16(skip) || !gcnx_aligned16(bias) || !gcnx_aligned16(out) ||
      !conv_ld_ok(ldo, h) || (skip && !conv_ld_ok(lds, h)))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_resgated_aggregate: p, w_e, skip, bias and out must be 16-byte aligned, with ldo "
                     "and lds >= h in multiples of 4 floats");
  if (n == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, rowptr && colidx && p && out, "gcnx_resgated_aggregate: NULL pointer");
  GCNX_REQUIRE(ctx, edge_dim == 0 || (e && w_e && lde >= edge_dim), "gcnx_resgated_aggregate: edge_dim > 0 needs e (lde >= edge_dim) and w_e");
  GCNX_REQUIRE(ctx, p != out && skip != out, "gcnx_resgated_aggregate: out must not alias p or skip");
  RGFwdArgs a{};
  a.rowptr = rowptr; a.colidx = colidx; a.p = p; a.ldp = ldp; a.n = n; a.edge_dim = edge_dim; a.e = e; a.lde = lde; a.w_e = w_e;
  a.skip = skip; a.lds = lds; a.bias = bias; a.out = out; a.ldo = ldo;
  const int tiles = gcnx_cdiv(n, conv_tile_rows(h));
#define GCNX_RG_AGG(H_, R_, E_) hipLaunchKernelGGL((resgated_aggregate_kernel<H_, R_, E_>), dim3(tiles), dim3(R_ * H_ / 4), 0, ctx->stream, a)
  GCNX_CONV_DISPATCH(h, edge_dim, GCNX_RG_AGG);
#undef GCNX_RG_AGG
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

int gcnx_resgated_bwd_targets(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* p, int64_t ldp, int32_t n,
                              int32_t h, const float* e, int64_t lde, int32_t edge_dim, const float* w_e, const float* d_out, int64_t ldd,
                              float* dk, int64_t ldg, float* ds, int64_t ldgs, float* dw_e, float* scratch) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "ResGatedGraphConv backward (targets)");
  GCNX_REQUIRE(ctx, n >= 0 && h >= 0 && edge_dim >= 0, "gcnx_resgated_bwd_targets: negative size");
  if (!rg_shape_ok(n, h, ldp, edge_dim))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_resgated_bwd_targets: %s (got n=%d h=%d ldp=%lld edge_dim=%d)", kRGShapes, n, h,
                     (long long)ldp, edge_dim);
  if (!gcnx_aligned16(p) || !gcnx_aligned16(w_e) || !gcnx_aligned16(d_out) || !gcnx_aligned16(dk) || !gcnx_aligned16(ds) ||
      !gcnx_aligned16(dw_e) || !gcnx_aligned16(scratch) || !conv_ld_ok(ldd, h) || !conv_ld_ok(ldg, h) || (ds && !conv_ld_ok(ldgs, h)))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_resgated_bwd_targets: p, w_e, d_out, dk, ds, dw_e and scratch must be 16-byte "
                     "aligned, with ldd, ldg and ldgs >= h in multiples of 4 floats");
  if (n == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, rowptr && colidx && p && d_out && dk, "gcnx_resgated_bwd_targets: NULL pointer");
  GCNX_REQUIRE(ctx, edge_dim == 0 || (e && w_e && dw_e && scratch && lde >= edge_dim),
               "gcnx_resgated_bwd_targets: edge_dim > 0 needs e (lde >= edge_dim), w_e, dw_e and scratch");
  GCNX_REQUIRE(ctx, dk != d_out && dk != p && ds != d_out && ds != p && (!ds || ds != dk),
               "gcnx_resgated_bwd_targets: dk and ds must not alias d_out, p or each other");
  RGTargetArgs a{};
  a.rowptr = rowptr; a.colidx = colidx; a.p = p; a.ldp = ldp; a.n = n; a.edge_dim = edge_dim; a.e = e; a.lde = lde; a.w_e = w_e;
  a.d_out = d_out; a.ldd = ldd; a.dk = dk; a.ldg = ldg; a.ds = ds; a.ldgs = ldgs; a.part = scratch;
  const int tiles = gcnx_cdiv(n, conv_tile_rows(h));
#define GCNX_RG_BT(H_, R_, E_) hipLaunchKernelGGL((resgated_bwd_targets_kernel<H_, R_, E_>), dim3(tiles), dim3(R_ * H_ / 4), 0, ctx->stream, a)
  GCNX_CONV_DISPATCH(h, edge_dim, GCNX_RG_BT);
#undef GCNX_RG_BT
  GCNX_LAUNCH_OK(ctx);
  if (edge_dim > 0) {
    hipLaunchKernelGGL(resgated_part_reduce_kernel, dim3(2 * edge_dim * h / 8), dim3(256), 0, ctx->stream, (const float*)scratch,
                       (int64_t)tiles, h, edge_dim, dw_e);
    GCNX_LAUNCH_OK(ctx);
  }
  return GCNX_OK;
}

int gcnx_resgated_bwd_sources(gcnx_ctx* ctx, const int32_t* rowptr_t, const int32_t* colidx_t, const int32_t* perm_t, const float* p,
                              int64_t ldp, int32_t n, int32_t h, const float* e, int64_t lde, int32_t edge_dim, const float* w_e,
                              const float* d_out, int64_t ldd, float* dqv, int64_t ldg) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "ResGatedGraphConv backward (sources)");
  GCNX_REQUIRE(ctx, n >= 0 && h >= 0 && edge_dim >= 0, "gcnx_resgated_bwd_sources: negative size");
  if (!rg_shape_ok(n, h, ldp, edge_dim))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_resgated_bwd_sources: %s (got n=%d h=%d ldp=%lld edge_dim=%d)", kRGShapes, n, h,
                     (long long)ldp, edge_dim);
  if (!gcnx_aligned16(p) || !gcnx_aligned16(w_e) || !gcnx_aligned16(d_out) || !gcnx_aligned16(dqv) || !conv_ld_ok(ldd, h) ||
      !conv_ld_ok(ldg, 2 * h) || !gcnx_fits_buffer(n, ldd, 4))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_resgated_bwd_sources: p, w_e, d_out and dqv must be 16-byte aligned, with ldd >= h "
                     "and ldg >= 2 h in multiples of 4 floats and n * ldd * 4 < 2^32");
  if (n == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, rowptr_t && colidx_t && perm_t && p && d_out && dqv, "gcnx_resgated_bwd_sources: NULL pointer");
  GCNX_REQUIRE(ctx, edge_dim == 0 || (e && w_e && lde >= edge_dim), "gcnx_resgated_bwd_sources: edge_dim > 0 needs e (lde >= edge_dim) and w_e");
  GCNX_REQUIRE(ctx, dqv != d_out && dqv != p, "gcnx_resgated_bwd_sources: dqv must not alias d_out or p");
  RGSourceArgs a{};
  a.rowptr = rowptr_t; a.colidx = colidx_t; a.perm = perm_t; a.p = p; a.ldp = ldp; a.n = n; a.edge_dim = edge_dim; a.e = e; a.lde = lde;
  a.w_e = w_e; a.d_out = d_out; a.ldd = ldd; a.dqv = dqv; a.ldg = ldg;
  const int tiles = gcnx_cdiv(n, conv_tile_rows(h));
#define GCNX_RG_BS(H_, R_, E_) hipLaunchKernelGGL((resgated_bwd_sources_kernel<H_, R_, E_>), dim3(tiles), dim3(R_ * H_ / 4), 0, ctx->stream, a)
  GCNX_CONV_DISPATCH(h, edge_dim, GCNX_RG_BS);
#undef GCNX_RG_BS
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

}  // extern "C"
