// GraphNorm (Cai et al. 2021; torch_geometric.nn.GraphNorm) fused with PReLU, and its backward: per graph g with m rows and
// per channel, with the learned parameters a (mean_scale), gamma, beta:
//   mu = mean_i z_i    o_i = z_i - a mu    v = mean_i o_i^2    r = 1 / sqrt(v + eps)    xh_i = o_i r    t_i = gamma xh_i + beta
//   y_i = act(t_i)
// The statistics never leave the graph: a segmented pass over each graph's rows, HBM-bound like the pools of reduce.hip and
// attn_pool.hip.  fp32, no atomics, every sum in a fixed order (bitwise reproducible).  The variance is the mean of the
// CENTRED squares, taken in a second walk over the graph's rows (as gcnx_bn_moments takes its variance), never E[z^2] - c mu^2.
//
// Lane layout (the one of attn_pool.hip): a row is held by LPR lanes of one wave, a float4 of columns each (LPR = 4 .. 64, the
// power of two that covers f / 4); the 256 / LPR "row groups" of a workgroup walk rows lo + rg, lo + rg + NG, ...  Every sum
// here runs down the columns, so a thread's running sums are its own; the row groups' sums meet in LDS and every thread adds
// them in ascending group order, so all threads of a column hold the same bits.
//
// Two routes per direction.  WHOLE: workgroup g owns graph g and walks its rows two (backward) or three (forward) times; the
// later walks hit L2 at these graph sizes.  SLICED: slices of S rows are spread over workgroups with the slot arithmetic of
// attn_pool.hip; per-slice partial rows go to the caller's scratch and every workgroup of a graph adds that graph's partial rows
// itself, in slice order (the same bits in each), so a direction is three launches forward (sums, centred squares, apply)
// and two backward (sums, apply).  The parameter gradients are per-graph rows in the ctx workspace, summed over the graphs by
// one more small launch.
#include "common.h"

#include <cmath>

namespace {

constexpr int kAutoSliceAvgRows = 384; // slice_rows == 0: graphs that average more rows than this are sliced (when b < 2 CUs): attn_pool's rule
constexpr int kAutoSliceMin = 64;      // slice_rows == 0: the library's slices are never shorter (gcnx_graph_norm_scratch_floats counts on it)
constexpr int kLoads = 4;              // rows in flight per thread and operand

inline int64_t fstride(int32_t f) { return ((int64_t)f + 3) & ~(int64_t)3; }      // row stride of the partial rows
inline int64_t slots_of(int64_t n, int32_t b, int64_t s) { return n / s + b; }     // slices: graph g owns slots from gp[g] / s + g

template <bool VEC>
__device__ __forceinline__ float4 ldq(const float* p, int valid) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (VEC) {
    if (valid > 0) v = *reinterpret_cast<const float4*>(p);
    return v;
  }
  if (valid > 0) v.x = p[0];
  if (valid > 1) v.y = p[1];
  if (valid > 2) v.z = p[2];
  if (valid > 3) v.w = p[3];
  return v;
}
template <bool VEC>
__device__ __forceinline__ void stq(float* p, float4 v, int valid) {
  if (VEC) {
    if (valid > 0) *reinterpret_cast<float4*>(p) = v;
    return;
  }
  if (valid > 0) p[0] = v.x;
  if (valid > 1) p[1] = v.y;
  if (valid > 2) p[2] = v.z;
  if (valid > 3) p[3] = v.w;
}
__device__ __forceinline__ float4 f4(float a) { return make_float4(a, a, a, a); }

#define GN_EACH(M) M(x) M(y) M(z) M(w)

// one element, as the forward AND the backward evaluate it (the backward recomputes t from z, mean and inv)
// o = z - a mu is ONE rounding (a fused multiply-add): where a mu nearly cancels z -- a one-row graph at a close to 1 -- a rounded
// product would leave o, and with it r and the backward, a relative error of 6e-8 / |1 - a|
__device__ __forceinline__ float gn_o(float z, float a, float mu) { return __builtin_fmaf(-a, mu, z); }
__device__ __forceinline__ float gn_xhat(float z, float a, float mu, float r) { return gn_o(z, a, mu) * r; }
__device__ __forceinline__ float gn_t(float xh, float ga, float be) { return __builtin_fmaf(xh, ga, be); }

// the row groups' running sums, added in ascending group order by every thread (LDS is free again on return)
template <int LPR>
__device__ __forceinline__ float4 fold(float4 acc, float4 (*s)[LPR]) {
  constexpr int NG = 256 / LPR;
  const int cl = threadIdx.x % LPR, rg = threadIdx.x / LPR;
  s[rg][cl] = acc;
  __syncthreads();
  float4 t = s[0][cl];
#pragma unroll 4                                           // (unrolled whole, NG = 64 reads cost 256 VGPRs)
  for (int q = 1; q < NG; ++q) {
    const float4 o = s[q][cl];
    t.x += o.x; t.y += o.y; t.z += o.z; t.w += o.w;
  }
  __syncthreads();
  return t;
}

// sum over rows lo .. hi of z (CENTRED: of (z - a mu)^2), the thread's four columns
template <int LPR, bool VEC, bool CENTRED>
__device__ __forceinline__ float4 sum_rows(const float* z, int64_t ldz, int64_t lo, int64_t hi, int c, int valid, float4 a, float4 mu) {
  constexpr int NG = 256 / LPR;
  const int rg = threadIdx.x / LPR;
  float4 acc = f4(0.f);
  for (int64_t base = lo + rg; base < hi; base += kLoads * NG) {
    float4 v[kLoads];
#pragma unroll
    for (int u = 0; u < kLoads; ++u) {
      const int64_t r = base + u * NG;
      v[u] = r < hi ? ldq<VEC>(z + r * ldz + c, valid) : f4(0.f);
    }
#pragma unroll
    for (int u = 0; u < kLoads; ++u) {
      if (base + u * NG >= hi) continue;
#define GN_TERM(q) { const float d = CENTRED ? gn_o(v[u].q, a.q, mu.q) : v[u].q; acc.q += CENTRED ? d * d : d; }
      GN_EACH(GN_TERM)
#undef GN_TERM
    }
  }
  return acc;
}

// sum of the partial rows base .. base + cnt (stride fs floats; `which` of `per` rows each), in ascending order per thread, then folded
template <int LPR, bool VEC>
__device__ __forceinline__ float4 sum_parts(const float* __restrict__ part, int64_t fs, int per, int which, int64_t base, int cnt,
                                            int c, int valid, float4 (*s)[LPR]) {
  constexpr int NG = 256 / LPR;
  const int rg = threadIdx.x / LPR;
  float4 acc = f4(0.f);
  for (int k = rg; k < cnt; k += NG) {
    const float4 v = ldq<true>(part + ((base + k) * per + which) * fs + c, valid);     // (partial rows are padded to float4s)
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  return fold<LPR>(acc, s);
}

// slot w of the sliced routes: slice k = w - base_g of graph g, base_g = gp[g] / S + g (strictly increasing in g and
// base_{g+1} - base_g >= the slices of g, so slots never collide; a slot past its graph's last slice has nothing to do)
struct Slice {
  int g, k, cnt;
  int64_t lo, hi, base;
};
__device__ __forceinline__ Slice slice_of(const int32_t* __restrict__ gp, int32_t b, int32_t S, int w) {
  int glo = 0, ghi = b;                                    // the largest g with base_g <= w (base_0 = 0)
  while (ghi - glo > 1) {
    const int mid = (glo + ghi) >> 1;
    if (gp[mid] / S + mid <= w) glo = mid; else ghi = mid;
  }
  Slice s;
  const int64_t g0 = gp[glo], g1 = gp[glo + 1];
  s.g = glo;
  s.base = g0 / S + glo;
  s.k = (int)(w - s.base);
  s.cnt = (int)((g1 - g0 + S - 1) / S);
  s.lo = g0 + (int64_t)s.k * S;
  s.hi = g1 < s.lo + S ? g1 : s.lo + S;
  return s;
}

// y = act(gamma xh + beta) over rows lo .. hi.  y may alias z exactly: a thread reads its own elements of a trip before it
// writes them, and nobody else touches them.
template <int LPR, bool VEC>
__device__ __forceinline__ void apply_rows(const float* z, int64_t ldz, float* y, int64_t ldy, int64_t lo, int64_t hi, int c,
                                           int valid, float4 a, float4 mu, float4 r, float4 ga, float4 be, bool prelu, float sl) {
  constexpr int NG = 256 / LPR;
  const int rg = threadIdx.x / LPR;
  for (int64_t base = lo + rg; base < hi; base += kLoads * NG) {
    float4 v[kLoads];
#pragma unroll
    for (int u = 0; u < kLoads; ++u) {
      const int64_t row = base + u * NG;
      v[u] = row < hi ? ldq<VEC>(z + row * ldz + c, valid) : f4(0.f);
    }
#pragma unroll
    for (int u = 0; u < kLoads; ++u) {
      const int64_t row = base + u * NG;
      if (row >= hi) continue;
      float4 o;
#define GN_OUT(q) { const float t = gn_t(gn_xhat(v[u].q, a.q, mu.q, r.q), ga.q, be.q); o.q = (!prelu || t > 0.f) ? t : sl * t; }
      GN_EACH(GN_OUT)
#undef GN_OUT
      stq<VEC>(y + row * ldy + c, o, valid);
    }
  }
}

__device__ __forceinline__ float4 inv_std(float4 sq, float m, float eps) {
  return make_float4(1.0f / sqrtf(sq.x / m + eps), 1.0f / sqrtf(sq.y / m + eps), 1.0f / sqrtf(sq.z / m + eps),
                     1.0f / sqrtf(sq.w / m + eps));
}
__device__ __forceinline__ float4 mul4(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 div4(float4 a, float m) { return make_float4(a.x / m, a.y / m, a.z / m, a.w / m); }

// ---- forward --------------------------------------------------------------------------------------------------------------
// PHASE 0: the whole route (grid = b).  Sliced (grid = slots): 1 = partial row sums -> p1; 2 = mean from p1, partial centred
// squares -> p2; 3 = inv from p2, y.  An empty graph's mean and inv rows are zero.
template <int LPR, bool VEC, int PHASE>
__global__ __launch_bounds__(256) void graph_norm_fwd_kernel(const int32_t* __restrict__ gp, const float* z, int64_t ldz,
                                                             const float* __restrict__ a, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float eps, int prelu,
                                                             const float* __restrict__ alpha, int32_t b, int32_t f, int32_t S,
                                                             float* y, int64_t ldy, float* mean, float* inv, float* p1, float* p2,
                                                             int64_t fs) {
  __shared__ float4 s[256 / LPR][LPR];
  const int cl = threadIdx.x % LPR, rg = threadIdx.x / LPR;
  const int c = cl * 4, valid = f - c;
  const float4 zero = f4(0.f);
  if (PHASE == 0) {
    const int g = blockIdx.x;
    const int64_t lo = gp[g], hi = gp[g + 1];
    float* mrow = mean + (int64_t)g * f + c;
    float* irow = inv + (int64_t)g * f + c;
    if (lo >= hi) {                                        // (the whole workgroup, before any barrier)
      if (rg == 0) { stq<VEC>(mrow, zero, valid); stq<VEC>(irow, zero, valid); }
      return;
    }
    const float m = (float)(hi - lo);
    const float4 av = ldq<VEC>(a + c, valid);
    const float4 mu = div4(fold<LPR>(sum_rows<LPR, VEC, false>(z, ldz, lo, hi, c, valid, zero, zero), s), m);
    const float4 r = inv_std(fold<LPR>(sum_rows<LPR, VEC, true>(z, ldz, lo, hi, c, valid, av, mu), s), m, eps);
    if (rg == 0) { stq<VEC>(mrow, mu, valid); stq<VEC>(irow, r, valid); }
    apply_rows<LPR, VEC>(z, ldz, y, ldy, lo, hi, c, valid, av, mu, r, ldq<VEC>(gamma + c, valid), ldq<VEC>(beta + c, valid), prelu != 0,
                         prelu ? alpha[0] : 0.f);
    return;
  }
  const Slice sl = slice_of(gp, b, S, blockIdx.x);
  float* mrow = mean + (int64_t)sl.g * f + c;
  float* irow = inv + (int64_t)sl.g * f + c;
  if (sl.lo >= sl.hi) {                                    // (the whole workgroup, before any barrier)
    if (PHASE == 2 && sl.k == 0 && rg == 0) { stq<VEC>(mrow, zero, valid); stq<VEC>(irow, zero, valid); }   // an empty graph
    return;
  }
  if (PHASE == 1) {
    const float4 t = fold<LPR>(sum_rows<LPR, VEC, false>(z, ldz, sl.lo, sl.hi, c, valid, zero, zero), s);
    if (rg == 0) stq<true>(p1 + (int64_t)blockIdx.x * fs + c, t, valid);
    return;
  }
  const float m = (float)((int64_t)gp[sl.g + 1] - (int64_t)gp[sl.g]);
  if (PHASE == 2) {
    const float4 mu = div4(sum_parts<LPR, VEC>(p1, fs, 1, 0, sl.base, sl.cnt, c, valid, s), m);
    const float4 t = fold<LPR>(sum_rows<LPR, VEC, true>(z, ldz, sl.lo, sl.hi, c, valid, ldq<VEC>(a + c, valid), mu), s);
    if (rg == 0) {
      stq<true>(p2 + (int64_t)blockIdx.x * fs + c, t, valid);
      if (sl.k == 0) stq<VEC>(mrow, mu, valid);
    }
    return;
  }
  const float4 r = inv_std(sum_parts<LPR, VEC>(p2, fs, 1, 0, sl.base, sl.cnt, c, valid, s), m, eps);
  if (sl.k == 0 && rg == 0) stq<VEC>(irow, r, valid);
  apply_rows<LPR, VEC>(z, ldz, y, ldy, sl.lo, sl.hi, c, valid, ldq<VEC>(a + c, valid), ldq<VEC>(mrow, valid), r, ldq<VEC>(gamma + c, valid), ldq<VEC>(beta + c, valid), prelu != 0,
                       prelu ? alpha[0] : 0.f);
}

// ---- backward -------------------------------------------------------------------------------------------------------------
// with dt = dy act'(t):  S1 = sum dt, S2 = sum dt xh, ds = sum dy min(t, 0) per column;
// D = r gamma (S1 - S2 X / m) with X / m = r mu (1 - a);  dz = r gamma (dt - xh S2 / m) - a D / m;  d a = - mu D.
struct BwdCols {
  float4 a, mu, r, ga, be;
  bool prelu;
  float sl;
};

template <int LPR, bool VEC>
__device__ __forceinline__ void bwd_sums(const float* dy, int64_t lddy, const float* z, int64_t ldz, int64_t lo, int64_t hi, int c,
                                         int valid, const BwdCols& q, float4& s1, float4& s2, float4& ds) {
  constexpr int NG = 256 / LPR;
  const int rg = threadIdx.x / LPR;
  s1 = s2 = ds = f4(0.f);
  for (int64_t base = lo + rg; base < hi; base += kLoads * NG) {
    float4 v[kLoads], d[kLoads];
#pragma unroll
    for (int u = 0; u < kLoads; ++u) {
      const int64_t row = base + u * NG;
      v[u] = row < hi ? ldq<VEC>(z + row * ldz + c, valid) : f4(0.f);
      d[u] = row < hi ? ldq<VEC>(dy + row * lddy + c, valid) : f4(0.f);
    }
#pragma unroll
    for (int u = 0; u < kLoads; ++u) {
      if (base + u * NG >= hi) continue;
#define GN_SUM(e)                                                             \
  {                                                                           \
    const float xh = gn_xhat(v[u].e, q.a.e, q.mu.e, q.r.e), t = gn_t(xh, q.ga.e, q.be.e); \
    const float dt = (!q.prelu || t > 0.f) ? d[u].e : q.sl * d[u].e;          \
    s1.e += dt;                                                               \
    s2.e += dt * xh;                                                          \
    if (q.prelu) ds.e += d[u].e * fminf(t, 0.f);                              \
  }
      GN_EACH(GN_SUM)
#undef GN_SUM
    }
  }
}

// dz over rows lo .. hi from the graph's sums; dz may alias dy exactly (a thread reads its own elements of a trip first)
template <int LPR, bool VEC>
__device__ __forceinline__ void bwd_apply(const float* dy, int64_t lddy, const float* z, int64_t ldz, float* dz, int64_t lddz,
                                          int64_t lo, int64_t hi, int c, int valid, const BwdCols& q, float4 s2m, float4 adm) {
  constexpr int NG = 256 / LPR;
  const int rg = threadIdx.x / LPR;
  const float4 rg4 = mul4(q.r, q.ga);
  for (int64_t base = lo + rg; base < hi; base += kLoads * NG) {
    float4 v[kLoads], d[kLoads];
#pragma unroll
    for (int u = 0; u < kLoads; ++u) {
      const int64_t row = base + u * NG;
      v[u] = row < hi ? ldq<VEC>(z + row * ldz + c, valid) : f4(0.f);
      d[u] = row < hi ? ldq<VEC>(dy + row * lddy + c, valid) : f4(0.f);
    }
#pragma unroll
    for (int u = 0; u < kLoads; ++u) {
      const int64_t row = base + u * NG;
      if (row >= hi) continue;
      float4 o;
#define GN_DZ(e)                                                              \
  {                                                                           \
    const float xh = gn_xhat(v[u].e, q.a.e, q.mu.e, q.r.e), t = gn_t(xh, q.ga.e, q.be.e); \
    const float dt = (!q.prelu || t > 0.f) ? d[u].e : q.sl * d[u].e;          \
    o.e = rg4.e * (dt - xh * s2m.e) - adm.e;                                  \
  }
      GN_EACH(GN_DZ)
#undef GN_DZ
      stq<VEC>(dz + row * lddz + c, o, valid);
    }
  }
}

// PHASE 0: the whole route (grid = b).  Sliced (grid = slots): 1 = the slice's three partial rows -> part[slot][3]; 2 = the
// graph's sums from them, dz.  gpart (may be NULL) receives the graph's rows [g][4]: S1, S2, -mu D, ds.
template <int LPR, bool VEC, int PHASE>
__global__ __launch_bounds__(256) void graph_norm_bwd_kernel(const int32_t* __restrict__ gp, const float* dy, int64_t lddy,
                                                             const float* __restrict__ z, int64_t ldz,
                                                             const float* __restrict__ mean, const float* __restrict__ inv,
                                                             const float* __restrict__ a, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, int prelu,
                                                             const float* __restrict__ alpha, int32_t b, int32_t f, int32_t S,
                                                             float* dz, int64_t lddz, float* part, float* __restrict__ gpart,
                                                             int64_t fs) {
  __shared__ float4 s[256 / LPR][LPR];
  const int cl = threadIdx.x % LPR, rg = threadIdx.x / LPR;
  const int c = cl * 4, valid = f - c;
  int g, k = 0, cnt = 0;
  int64_t lo, hi, base = 0;
  if (PHASE == 0) {
    g = blockIdx.x;
    lo = gp[g];
    hi = gp[g + 1];
  } else {
    const Slice sl = slice_of(gp, b, S, blockIdx.x);
    g = sl.g; k = sl.k; cnt = sl.cnt; lo = sl.lo; hi = sl.hi; base = sl.base;
  }
  if (lo >= hi) {                                          // (the whole workgroup, before any barrier)
    if (PHASE != 1 && gpart && k == 0 && rg == 0)          // an empty graph adds nothing
      for (int j = 0; j < 4; ++j) stq<true>(gpart + ((int64_t)g * 4 + j) * fs + c, f4(0.f), valid);
    return;
  }
  const float4 mu = ldq<VEC>(mean + (int64_t)g * f + c, valid), av = ldq<VEC>(a + c, valid);
  BwdCols q;
  q.a = av;
  q.mu = mu;
  q.r = ldq<VEC>(inv + (int64_t)g * f + c, valid);
  q.ga = ldq<VEC>(gamma + c, valid);
  q.be = ldq<VEC>(beta + c, valid);
  q.prelu = prelu != 0;
  q.sl = prelu ? alpha[0] : 0.f;
  float4 s1, s2, ds;
  if (PHASE != 2) {
    bwd_sums<LPR, VEC>(dy, lddy, z, ldz, lo, hi, c, valid, q, s1, s2, ds);
    s1 = fold<LPR>(s1, s);
    s2 = fold<LPR>(s2, s);
    ds = fold<LPR>(ds, s);
    if (PHASE == 1) {
      if (rg == 0) {
        float* row = part + (int64_t)blockIdx.x * 3 * fs + c;
        stq<true>(row, s1, valid); stq<true>(row + fs, s2, valid); stq<true>(row + 2 * fs, ds, valid);
      }
      return;
    }
  } else {
    s1 = sum_parts<LPR, VEC>(part, fs, 3, 0, base, cnt, c, valid, s);
    s2 = sum_parts<LPR, VEC>(part, fs, 3, 1, base, cnt, c, valid, s);
    ds = sum_parts<LPR, VEC>(part, fs, 3, 2, base, cnt, c, valid, s);
  }
  const float m = (float)((int64_t)gp[g + 1] - (int64_t)gp[g]);
  float4 dd, s2m, adm, dag;
#define GN_FIN(e)                                                             \
  {                                                                           \
    const float xm = q.r.e * mu.e * (1.f - av.e);                             \
    dd.e = q.r.e * q.ga.e * (s1.e - s2.e * xm);                               \
    s2m.e = s2.e / m;                                                         \
    adm.e = av.e * dd.e / m;                                                  \
    dag.e = -mu.e * dd.e;                                                     \
  }
  GN_EACH(GN_FIN)
#undef GN_FIN
  if (gpart && k == 0 && rg == 0) {
    float* row = gpart + (int64_t)g * 4 * fs + c;
    stq<true>(row, s1, valid); stq<true>(row + fs, s2, valid); stq<true>(row + 2 * fs, dag, valid); stq<true>(row + 3 * fs, ds, valid);
  }
  bwd_apply<LPR, VEC>(dy, lddy, z, ldz, dz, lddz, lo, hi, c, valid, q, s2m, adm);
}

// The parameter gradients from the graphs' rows gpart[g][4][fs]: workgroup k sums row k over the graphs -- four graph groups,
// each ascending, folded in order -- into dbeta, dgamma, d mean_scale; k = 3 also sums over the columns (fixed tree): dslope[0].
__global__ __launch_bounds__(256) void graph_norm_param_kernel(const float* __restrict__ gpart, int32_t b, int32_t f, int64_t fs,
                                                               float* __restrict__ dbeta, float* __restrict__ dgamma,
                                                               float* __restrict__ da, float* __restrict__ dslope) {
  __shared__ float s[4][256];
  const int k = blockIdx.x, t = threadIdx.x, col = t & 63, grp = t >> 6;
  float* out = k == 0 ? dbeta : (k == 1 ? dgamma : (k == 2 ? da : dslope));
  if (!out) return;                                        // (the whole workgroup)
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int g = grp; g < b; g += 4) {
    const float* row = gpart + ((int64_t)g * 4 + k) * fs;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (col + 64 * j < f) acc[j] += row[col + 64 * j];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) s[grp][col + 64 * j] = acc[j];
  __syncthreads();
  const float tot = t < f ? ((s[0][t] + s[1][t]) + s[2][t]) + s[3][t] : 0.f;
  if (k < 3) {
    if (t < f) out[t] = tot;
    return;
  }
  __syncthreads();
  s[0][t] = tot;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (t < off) s[0][t] += s[0][t + off];
    __syncthreads();
  }
  if (t == 0) out[0] = s[0][0];
}

int lanes_per_row(int32_t f) {
  int lpr = 4;
  while (lpr * 4 < f) lpr *= 2;
  return lpr;                                              // 4 .. 64 for f <= 256
}

// LAUNCH(LPR, VEC): the site's launch text with the two template arguments left open
#define GRAPH_NORM_DISPATCH(lpr, vec, LAUNCH)                                  \
  do {                                                                         \
    switch (lpr) {                                                             \
      case 4: if (vec) { LAUNCH(4, true); } else { LAUNCH(4, false); } break;   \
      case 8: if (vec) { LAUNCH(8, true); } else { LAUNCH(8, false); } break;   \
      case 16: if (vec) { LAUNCH(16, true); } else { LAUNCH(16, false); } break; \
      case 32: if (vec) { LAUNCH(32, true); } else { LAUNCH(32, false); } break; \
      default: if (vec) { LAUNCH(64, true); } else { LAUNCH(64, false); } break; \
    }                                                                          \
  } while (0)

// the library's choice of slice_rows == 0 (attn_pool's rule: no threshold of this kernel's own has been measured): slices
// where one workgroup per graph would leave most CUs idle AND the graphs are tall enough (kAutoSliceAvgRows on average) for
// the extra launches to pay; slices of at least kAutoSliceMin rows, about two per CU
int64_t slice_rows_of(const gcnx_ctx* ctx, int32_t n, int32_t b, int32_t slice_rows, const float* scratch) {
  int64_t S = slice_rows;
  if (S == 0 && scratch && b < 2 * ctx->num_cus && (int64_t)n > kAutoSliceAvgRows * (int64_t)b) {
    S = ((int64_t)n + 2 * ctx->num_cus - 1) / (2 * ctx->num_cus);
    if (S < kAutoSliceMin) S = kAutoSliceMin;
  }
  return S;
}

}  // namespace

extern "C" {

int64_t gcnx_graph_norm_scratch_floats(int64_t n, int32_t b, int32_t f, int32_t slice_rows) {
  if (n <= 0 || b <= 0 || f <= 0 || slice_rows < 0) return 0;
  return 3 * slots_of(n, b, slice_rows > 0 ? slice_rows : kAutoSliceMin) * fstride(f);     // (forward: two partial rows per slot)
}

int gcnx_graph_norm_act(gcnx_ctx* ctx, const int32_t* graph_ptr, const float* z, int64_t ldz, const float* mean_scale,
                        const float* gamma, const float* beta, float eps, int act, const float* alpha, int32_t n, int32_t b,
                        int32_t f, int32_t slice_rows, float* y, int64_t ldy, float* mean, float* inv, float* scratch) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "graph norm");
  GCNX_REQUIRE(ctx, n >= 0 && b >= 0 && f >= 0 && slice_rows >= 0, "gcnx_graph_norm_act: negative size");
  if (act != GCNX_ACT_NONE && act != GCNX_ACT_PRELU_SHARED)
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_graph_norm_act: act = %d (GCNX_ACT_NONE and GCNX_ACT_PRELU_SHARED are served)", act);
  if (n == 0 || b == 0 || f == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, graph_ptr && z && mean_scale && gamma && beta && y && mean && inv, "gcnx_graph_norm_act: NULL pointer");
  GCNX_REQUIRE(ctx, act == GCNX_ACT_NONE || alpha, "gcnx_graph_norm_act: PReLU needs alpha");
  GCNX_REQUIRE(ctx, f <= 256, "gcnx_graph_norm_act: f = %d, at most 256 columns", f);
  GCNX_REQUIRE(ctx, ldz >= f && ldy >= f, "gcnx_graph_norm_act: leading dimension too small");
  GCNX_REQUIRE(ctx, slice_rows == 0 || scratch, "gcnx_graph_norm_act: slice_rows > 0 needs scratch");
  GCNX_REQUIRE(ctx, gcnx_aligned16(scratch), "gcnx_graph_norm_act: scratch must be 16-byte aligned");
  const int64_t S = slice_rows_of(ctx, n, b, slice_rows, scratch);
  const int lpr = lanes_per_row(f);
  const int vec = f % 4 == 0 && ldz % 4 == 0 && ldy % 4 == 0 && gcnx_aligned16(z) && gcnx_aligned16(y) && gcnx_aligned16(mean_scale) &&
                  gcnx_aligned16(gamma) && gcnx_aligned16(beta) && gcnx_aligned16(mean) && gcnx_aligned16(inv);
  const int64_t fs = fstride(f);
  const int prelu = act == GCNX_ACT_PRELU_SHARED;
  const int64_t slots = S ? slots_of(n, b, S) : 0;
  GCNX_REQUIRE(ctx, slots <= INT32_MAX, "gcnx_graph_norm_act: too many slices");
  const int32_t S32 = (int32_t)S;
  float* p1 = scratch;
  float* p2 = scratch ? scratch + slots * fs : nullptr;
#define LAUNCH_PHASE(LPR, VEC, PHASE, GRID)                                                                                     \
  hipLaunchKernelGGL((graph_norm_fwd_kernel<LPR, VEC, PHASE>), dim3((unsigned)(GRID)), dim3(256), 0, ctx->stream, graph_ptr, z, \
                     ldz, mean_scale, gamma, beta, eps, prelu, alpha, b, f, S32, y, ldy, mean, inv, p1, p2, fs)
  if (S == 0) {
#define LAUNCH(LPR, VEC) LAUNCH_PHASE(LPR, VEC, 0, b)
    GRAPH_NORM_DISPATCH(lpr, vec, LAUNCH);
#undef LAUNCH
    GCNX_LAUNCH_OK(ctx);
    return GCNX_OK;
  }
#define LAUNCH(LPR, VEC) LAUNCH_PHASE(LPR, VEC, 1, slots)
  GRAPH_NORM_DISPATCH(lpr, vec, LAUNCH);
#undef LAUNCH
  GCNX_LAUNCH_OK(ctx);
#define LAUNCH(LPR, VEC) LAUNCH_PHASE(LPR, VEC, 2, slots)
  GRAPH_NORM_DISPATCH(lpr, vec, LAUNCH);
#undef LAUNCH
  GCNX_LAUNCH_OK(ctx);
#define LAUNCH(LPR, VEC) LAUNCH_PHASE(LPR, VEC, 3, slots)
  GRAPH_NORM_DISPATCH(lpr, vec, LAUNCH);
#undef LAUNCH
#undef LAUNCH_PHASE
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

int gcnx_graph_norm_act_bwd(gcnx_ctx* ctx, const int32_t* graph_ptr, const float* dy, int64_t lddy, const float* z, int64_t ldz,
                            const float* mean, const float* inv, const float* mean_scale, const float* gamma, const float* beta,
                            int act, const float* alpha, int32_t n, int32_t b, int32_t f, int32_t slice_rows, float* dz,
                            int64_t lddz, float* dgamma, float* dbeta, float* dmean_scale, float* dalpha, float* scratch) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "graph norm bwd");
  GCNX_REQUIRE(ctx, n >= 0 && b >= 0 && f >= 0 && slice_rows >= 0, "gcnx_graph_norm_act_bwd: negative size");
  if (act != GCNX_ACT_NONE && act != GCNX_ACT_PRELU_SHARED)
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_graph_norm_act_bwd: act = %d (GCNX_ACT_NONE and GCNX_ACT_PRELU_SHARED are served)", act);
  if (n == 0 || b == 0 || f == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, graph_ptr && dy && z && mean && inv && mean_scale && gamma && beta && dz, "gcnx_graph_norm_act_bwd: NULL pointer");
  GCNX_REQUIRE(ctx, act == GCNX_ACT_NONE || alpha, "gcnx_graph_norm_act_bwd: PReLU needs alpha");
  GCNX_REQUIRE(ctx, f <= 256, "gcnx_graph_norm_act_bwd: f = %d, at most 256 columns", f);
  GCNX_REQUIRE(ctx, lddy >= f && ldz >= f && lddz >= f, "gcnx_graph_norm_act_bwd: leading dimension too small");
  GCNX_REQUIRE(ctx, slice_rows == 0 || scratch, "gcnx_graph_norm_act_bwd: slice_rows > 0 needs scratch");
  GCNX_REQUIRE(ctx, gcnx_aligned16(scratch), "gcnx_graph_norm_act_bwd: scratch must be 16-byte aligned");
  const int64_t S = slice_rows_of(ctx, n, b, slice_rows, scratch);
  const int lpr = lanes_per_row(f);
  const int vec = f % 4 == 0 && lddy % 4 == 0 && ldz % 4 == 0 && lddz % 4 == 0 && gcnx_aligned16(dy) && gcnx_aligned16(z) &&
                  gcnx_aligned16(dz) && gcnx_aligned16(mean_scale) && gcnx_aligned16(gamma) && gcnx_aligned16(beta) &&
                  gcnx_aligned16(mean) && gcnx_aligned16(inv);
  const int64_t fs = fstride(f);
  const int prelu = act == GCNX_ACT_PRELU_SHARED;
  const int64_t slots = S ? slots_of(n, b, S) : 0;
  GCNX_REQUIRE(ctx, slots <= INT32_MAX, "gcnx_graph_norm_act_bwd: too many slices");
  const int32_t S32 = (int32_t)S;
  float* gpart = nullptr;                                  // the graphs' rows of the parameter gradients: ctx workspace
  if (dgamma || dbeta || dmean_scale || dalpha) {
    const int rc = gcnx_ws_reserve(ctx, (size_t)b * 4 * fs * sizeof(float));
    if (rc) return rc;
    gpart = (float*)ctx->ws;
  }
#define LAUNCH_PHASE(LPR, VEC, PHASE, GRID)                                                                                      \
  hipLaunchKernelGGL((graph_norm_bwd_kernel<LPR, VEC, PHASE>), dim3((unsigned)(GRID)), dim3(256), 0, ctx->stream, graph_ptr, dy, \
                     lddy, z, ldz, mean, inv, mean_scale, gamma, beta, prelu, alpha, b, f, S32, dz, lddz, scratch, gpart, fs)
  if (S == 0) {
#define LAUNCH(LPR, VEC) LAUNCH_PHASE(LPR, VEC, 0, b)
    GRAPH_NORM_DISPATCH(lpr, vec, LAUNCH);
#undef LAUNCH
  } else {
#define LAUNCH(LPR, VEC) LAUNCH_PHASE(LPR, VEC, 1, slots)
    GRAPH_NORM_DISPATCH(lpr, vec, LAUNCH);
#undef LAUNCH
    GCNX_LAUNCH_OK(ctx);
#define LAUNCH(LPR, VEC) LAUNCH_PHASE(LPR, VEC, 2, slots)
    GRAPH_NORM_DISPATCH(lpr, vec, LAUNCH);
#undef LAUNCH
  }
#undef LAUNCH_PHASE
  GCNX_LAUNCH_OK(ctx);
  if (gpart) {
    hipLaunchKernelGGL(graph_norm_param_kernel, dim3(4), dim3(256), 0, ctx->stream, (const float*)gpart, b, f, fs, dbeta, dgamma,
                       dmean_scale, dalpha);
    GCNX_LAUNCH_OK(ctx);
  }
  return GCNX_OK;
}

}  // extern "C"
