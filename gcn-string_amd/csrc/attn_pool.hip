// GlobalAttnSumPool: the learned readout  s_i = <x_i, a>,  alpha = softmax of s over the rows of one graph,
// P[g] = sum_i alpha_i x_i  -- a segmented ONLINE softmax fused with the weighted row sum (one pass over x), and its backward.
// HBM-bound like the pools of reduce.hip; fp32, no atomics, every sum in a fixed order (bitwise reproducible).
//
// Lane layout (forward and backward): a row is held by LPR lanes of one wave, a float4 of columns each (LPR = 4 .. 64, the power
// of two that covers f / 4), so a wave instruction reads 64 / LPR whole rows; the 256 / LPR "row groups" of a workgroup walk
// rows lo + rg, lo + rg + NG, ...  A row's dot products are xor butterflies inside its LPR lanes: every lane of the group ends
// with the same bits (fp32 addition commutes), so the running (m, l) are kept per lane without a broadcast.
#include "common.h"

#include <cmath>

namespace {

constexpr int kAutoSliceAvgRows = 384; // slice_rows == 0: graphs that average more rows than this are sliced (when b < 2 CUs)
constexpr int kAutoSliceMin = 64;      // slice_rows == 0: the library's slices are never shorter (gcnx_attn_pool_scratch_floats counts on it)
constexpr int kBwdRowsMin = 64;        // backward: rows per workgroup, at least; at most 1024 partial rows of da
constexpr int kBwdPartsMax = 1024;
constexpr int kFwdLoads = 8;           // forward: rows in flight per row group (a workgroup's walk is a chain of round trips)

inline int64_t fstride(int32_t f) { return ((int64_t)f + 3) & ~(int64_t)3; }      // row stride of the partial rows in scratch
inline int64_t fwd_slots(int64_t n, int32_t b, int64_t s) { return n / s + b; }    // slices: graph g owns slots from gp[g] / s + g
inline int64_t bwd_rows(int64_t n) { const int64_t r = (n + kBwdPartsMax - 1) / kBwdPartsMax; return r < kBwdRowsMin ? kBwdRowsMin : r; }

template <int LPR>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int off = LPR >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// the lane's four columns of a row (valid = columns it really owns; <= 0: none).  VEC: f % 4 == 0, 16-byte aligned rows.
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
__device__ __forceinline__ float dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// Forward, both routes.  whole (SLICED = false): workgroup g owns graph g, folds its row groups' (m, l, acc) through LDS, writes
// pooled[g] and turns the scores it stored in alpha into coefficients (a second pass over alpha alone, behind a barrier).
// SLICED: workgroup w owns slot w: slice k = w - base_g of graph g, base_g = gp[g] / S + g (strictly increasing in g and
// base_{g+1} - base_g >= the slices of g, so slots never collide; a slot past its graph's last slice has nothing to do) and
// writes (m, l) to ml[w] and acc to part[w]; attn_pool_combine_kernel finishes.
template <int LPR, bool VEC, bool SLICED>
__global__ __launch_bounds__(256) void attn_pool_fwd_kernel(const int32_t* __restrict__ gp, const float* __restrict__ x, int64_t ldx,
                                                            const float* __restrict__ a, int32_t b, int32_t f, int32_t S,
                                                            float* __restrict__ pooled, int64_t ldp, float* alpha,
                                                            float* __restrict__ ml, float* __restrict__ part, int64_t fs) {
  constexpr int NG = 256 / LPR;
  __shared__ float sm[NG], sl[NG], sML[2];
  __shared__ float4 sacc[NG][LPR];
  const int cl = threadIdx.x % LPR, rg = threadIdx.x / LPR;
  const int c = cl * 4, valid = f - c;
  int g;
  int64_t lo, hi;
  if (SLICED) {
    const int w = blockIdx.x;
    int glo = 0, ghi = b;                                  // the largest g with base_g <= w (base_0 = 0)
    while (ghi - glo > 1) {
      const int mid = (glo + ghi) >> 1;
      if (gp[mid] / S + mid <= w) glo = mid; else ghi = mid;
    }
    g = glo;
    const int64_t k = w - (gp[g] / S + g);
    lo = gp[g] + k * S;
    hi = gp[g + 1];
    if (lo >= hi) return;                                  // (the whole workgroup, before any barrier)
    if (hi > lo + S) hi = lo + S;
  } else {
    g = blockIdx.x;
    lo = gp[g];
    hi = gp[g + 1];
  }
  const float4 av = ldq<VEC>(a + c, valid);
  float m = -INFINITY, l = 0.f;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t base = lo; base < hi; base += kFwdLoads * NG) {     // (uniform trip count: the butterflies run in every lane)
    float4 v[kFwdLoads];
#pragma unroll
    for (int u = 0; u < kFwdLoads; ++u) {
      const int64_t r = base + rg + u * NG;
      v[u] = r < hi ? ldq<VEC>(x + r * ldx + c, valid) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < kFwdLoads; ++u) {
      const int64_t r = base + rg + u * NG;
      const float s = group_sum<LPR>(dot4(v[u], av));
      if (r < hi) {
        if (alpha && cl == 0) alpha[r] = s;                // the score; a coefficient after the second pass
        // one exponential per row: the new maximum is s or m, the other side gets exp(-|s - m|)
        const float d = s - m, e = expf(-fabsf(d));
        const float keep = d > 0.f ? e : 1.f, p = d > 0.f ? 1.f : e;      // (m = -inf: d = +inf, keep = 0, p = 1)
        l = l * keep + p;
        acc.x = acc.x * keep + p * v[u].x; acc.y = acc.y * keep + p * v[u].y;
        acc.z = acc.z * keep + p * v[u].z; acc.w = acc.w * keep + p * v[u].w;
        m = fmaxf(m, s);
      }
    }
  }
  if (cl == 0) { sm[rg] = m; sl[rg] = l; }
  sacc[rg][cl] = acc;
  __syncthreads();
  if (rg == 0) {                                           // row groups in ascending order; a group without rows weighs 0
    float M = -INFINITY, Lsum = 0.f;
    for (int q = 0; q < NG; ++q) M = fmaxf(M, sm[q]);
    float4 A = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int q = 0; q < NG; ++q) {
      const float w = sm[q] == -INFINITY ? 0.f : expf(sm[q] - M);
      const float4 o = sacc[q][cl];
      Lsum += sl[q] * w;
      A.x += o.x * w; A.y += o.y * w; A.z += o.z * w; A.w += o.w * w;
    }
    if (SLICED) {
      if (cl == 0) { ml[2 * (int64_t)blockIdx.x] = M; ml[2 * (int64_t)blockIdx.x + 1] = Lsum; }
      stq<VEC>(part + (int64_t)blockIdx.x * fs + c, A, valid);
    } else {
      if (Lsum > 0.f) { A.x /= Lsum; A.y /= Lsum; A.z /= Lsum; A.w /= Lsum; }
      else A = make_float4(0.f, 0.f, 0.f, 0.f);            // an empty graph pools to a zero row
      stq<VEC>(pooled + (int64_t)g * ldp + c, A, valid);
      if (cl == 0) { sML[0] = M; sML[1] = Lsum; }
    }
  }
  if (SLICED || !alpha) return;
  __syncthreads();                                         // (and the scores, written before the barrier above, are the workgroup's to read)
  const float M = sML[0], L = sML[1];
  for (int64_t r = lo + threadIdx.x; r < hi; r += 256) alpha[r] = expf(alpha[r] - M) / L;
}

// Second launch of the sliced route: workgroup g rescales the parts of graph g's slices to their common maximum and adds them
// in slice order, writes pooled[g], and turns the graph's stored scores into coefficients.  The slices' weights exp(m_k - M)
// are staged in LDS, 256 slices at a time; l is summed per thread over k = t, t + 256, ... and then over the threads in a
// fixed tree.
__global__ __launch_bounds__(256) void attn_pool_combine_kernel(const int32_t* __restrict__ gp, int32_t f, int32_t S,
                                                                const float* __restrict__ ml, const float* __restrict__ part,
                                                                int64_t fs, float* __restrict__ pooled, int64_t ldp,
                                                                float* __restrict__ alpha) {
  __shared__ float red[256], sw[256];
  const int g = blockIdx.x, t = threadIdx.x;
  const int64_t lo = gp[g], hi = gp[g + 1];
  const int64_t base = lo / S + g;
  const int cnt = (int)((hi - lo + S - 1) / S);            // (every slice holds at least one row: its m is finite)
  float m = -INFINITY;
  for (int k = t; k < cnt; k += 256) m = fmaxf(m, ml[2 * (base + k)]);
  red[t] = m;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (t < off) red[t] = fmaxf(red[t], red[t + off]);
    __syncthreads();
  }
  const float M = red[0];
  __syncthreads();
  float l = 0.f;
  for (int k = t; k < cnt; k += 256) l += ml[2 * (base + k) + 1] * expf(ml[2 * (base + k)] - M);
  red[t] = l;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (t < off) red[t] += red[t + off];
    __syncthreads();
  }
  const float L = red[0];
  float acc = 0.f;                                         // column t (f <= 256)
  for (int k0 = 0; k0 < cnt; k0 += 256) {
    const int kn = cnt - k0 < 256 ? cnt - k0 : 256;
    __syncthreads();
    if (t < kn) sw[t] = expf(ml[2 * (base + k0 + t)] - M);
    __syncthreads();
    if (t < f) {
      const float* pp = part + (base + k0) * fs + t;
#pragma unroll 4
      for (int k = 0; k < kn; ++k) acc += pp[k * fs] * sw[k];
    }
  }
  if (t < f) pooled[(int64_t)g * ldp + t] = L > 0.f ? acc / L : 0.f;
  if (alpha)
    for (int64_t r = lo + t; r < hi; r += 256) alpha[r] = expf(alpha[r] - M) / L;
}

// Backward over row blocks, regardless of graph boundaries (as pool_bwd_kernel): with t_i = <dP[g], x_i - P[g]> and
// w_i = alpha_i t_i:  dx_i = alpha_i dP[g] + w_i a,  part[workgroup] = sum_i w_i x_i.  A row group finds the graph of its first
// row by one binary search and steps the graph index forward from there (empty graphs are stepped over).
template <int LPR, bool VEC>
__global__ __launch_bounds__(256) void attn_pool_bwd_kernel(const int32_t* __restrict__ gp, int32_t b, const float* __restrict__ x,
                                                            int64_t ldx, const float* __restrict__ a, const float* __restrict__ alpha,
                                                            const float* __restrict__ pooled, int64_t ldp,
                                                            const float* __restrict__ dp, int64_t lddp, int32_t n, int32_t f,
                                                            int64_t rows_per_wg, float* __restrict__ dx, int64_t lddx,
                                                            float* __restrict__ part, int64_t fs) {
  constexpr int NG = 256 / LPR;
  __shared__ float4 sacc[NG][LPR];
  const int cl = threadIdx.x % LPR, rg = threadIdx.x / LPR;
  const int c = cl * 4, valid = f - c;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_wg;
  const int64_t r1 = r0 + rows_per_wg < n ? r0 + rows_per_wg : n;
  const float4 av = ldq<VEC>(a + c, valid);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 dpv = acc, pv = acc;
  int g = -1;
  int64_t gend = 0;
  for (int64_t base = r0; base < r1; base += NG) {          // (uniform trip count: the butterfly runs in every lane)
    const int64_t r = base + rg;
    const bool act = r < r1;
    if (act && r >= gend) {
      if (g < 0) {                                         // the largest g with gp[g] <= r: its graph holds r
        int glo = 0, ghi = b;
        while (ghi - glo > 1) {
          const int mid = (glo + ghi) >> 1;
          if (gp[mid] <= r) glo = mid; else ghi = mid;
        }
        g = glo;
      } else {
        do ++g; while (g + 1 < b && gp[g + 1] <= r);
      }
      gend = gp[g + 1];
      dpv = ldq<VEC>(dp + (int64_t)g * lddp + c, valid);
      pv = ldq<VEC>(pooled + (int64_t)g * ldp + c, valid);
    }
    float4 xv = make_float4(0.f, 0.f, 0.f, 0.f);
    float al = 0.f;
    if (act) { xv = ldq<VEC>(x + r * ldx + c, valid); al = alpha[r]; }
    const float t = group_sum<LPR>(dpv.x * (xv.x - pv.x) + dpv.y * (xv.y - pv.y) + dpv.z * (xv.z - pv.z) + dpv.w * (xv.w - pv.w));
    if (act) {
      const float w = al * t;
      if (dx)
        stq<VEC>(dx + r * lddx + c, make_float4(al * dpv.x + w * av.x, al * dpv.y + w * av.y, al * dpv.z + w * av.z, al * dpv.w + w * av.w),
                 valid);
      acc.x += w * xv.x; acc.y += w * xv.y; acc.z += w * xv.z; acc.w += w * xv.w;
    }
  }
  if (!part) return;
  sacc[rg][cl] = acc;
  __syncthreads();
  if (rg == 0) {
    float4 t = sacc[0][cl];
    for (int q = 1; q < NG; ++q) { const float4 o = sacc[q][cl]; t.x += o.x; t.y += o.y; t.z += o.z; t.w += o.w; }
    stq<VEC>(part + (int64_t)blockIdx.x * fs + c, t, valid);
  }
}

// da[c] = sum over the partial rows, ascending: 16 columns x 16 row groups per workgroup, the groups folded through LDS in order.
__global__ __launch_bounds__(256) void attn_pool_da_kernel(const float* __restrict__ part, int64_t rows, int32_t f, int64_t fs,
                                                           float* __restrict__ da) {
  __shared__ float s[16][16];
  const int cl = threadIdx.x & 15, rg = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  float acc = 0.f;
  if (c < f)
    for (int64_t r = rg; r < rows; r += 16) acc += part[r * fs + c];
  s[rg][cl] = acc;
  __syncthreads();
  if (rg == 0 && c < f) {
    float t = s[0][cl];
    for (int q = 1; q < 16; ++q) t += s[q][cl];
    da[c] = t;
  }
}

int lanes_per_row(int32_t f) {
  int lpr = 4;
  while (lpr * 4 < f) lpr *= 2;
  return lpr;                                              // 4 .. 64 for f <= 256
}

// LAUNCH(LPR, VEC): the site's launch text with the two template arguments left open
#define ATTN_POOL_DISPATCH(lpr, vec, LAUNCH)                                   \
  do {                                                                         \
    switch (lpr) {                                                             \
      case 4: if (vec) { LAUNCH(4, true); } else { LAUNCH(4, false); } break;   \
      case 8: if (vec) { LAUNCH(8, true); } else { LAUNCH(8, false); } break;   \
      case 16: if (vec) { LAUNCH(16, true); } else { LAUNCH(16, false); } break; \
      case 32: if (vec) { LAUNCH(32, true); } else { LAUNCH(32, false); } break; \
      default: if (vec) { LAUNCH(64, true); } else { LAUNCH(64, false); } break; \
    }                                                                          \
  } while (0)

}  // namespace

extern "C" {

int64_t gcnx_attn_pool_scratch_floats(int64_t n, int32_t b, int32_t f, int32_t slice_rows) {
  if (n <= 0 || b <= 0 || f <= 0 || slice_rows < 0) return 0;
  const int64_t fs = fstride(f);
  const int64_t slots = fwd_slots(n, b, slice_rows > 0 ? slice_rows : kAutoSliceMin);
  const int64_t fwd = ((2 * slots + 3) & ~(int64_t)3) + slots * fs;
  const int64_t bwd = ((n + bwd_rows(n) - 1) / bwd_rows(n)) * fs;
  return fwd > bwd ? fwd : bwd;
}

int gcnx_attn_pool(gcnx_ctx* ctx, const int32_t* graph_ptr, const float* x, int64_t ldx, const float* a, int32_t n, int32_t b,
                   int32_t f, int32_t slice_rows, float* pooled, int64_t ldp, float* alpha, float* scratch) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "attention pool");
  GCNX_REQUIRE(ctx, n >= 0 && b >= 0 && f >= 0 && slice_rows >= 0, "gcnx_attn_pool: negative size");
  if (n == 0 || b == 0 || f == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, graph_ptr && x && a && pooled, "gcnx_attn_pool: NULL pointer");
  GCNX_REQUIRE(ctx, f <= 256, "gcnx_attn_pool: f = %d, at most 256 columns", f);
  GCNX_REQUIRE(ctx, ldx >= f && ldp >= f, "gcnx_attn_pool: leading dimension too small");
  GCNX_REQUIRE(ctx, slice_rows == 0 || scratch, "gcnx_attn_pool: slice_rows > 0 needs scratch");
  GCNX_REQUIRE(ctx, gcnx_aligned16(scratch), "gcnx_attn_pool: scratch must be 16-byte aligned");
  // the library's choice: slices where one workgroup per graph would leave most CUs idle AND the graphs are tall enough
  // (kAutoSliceAvgRows on average) for the second launch to pay; slices of at least kAutoSliceMin rows, about two per CU
  int64_t S = slice_rows;
  if (S == 0 && scratch && b < 2 * ctx->num_cus && (int64_t)n > kAutoSliceAvgRows * (int64_t)b) {
    S = ((int64_t)n + 2 * ctx->num_cus - 1) / (2 * ctx->num_cus);
    if (S < kAutoSliceMin) S = kAutoSliceMin;
  }
  if (S > INT32_MAX) S = INT32_MAX;
  const int lpr = lanes_per_row(f);
  const int vec = f % 4 == 0 && ldx % 4 == 0 && ldp % 4 == 0 && gcnx_aligned16(x) && gcnx_aligned16(a) && gcnx_aligned16(pooled);
  const int64_t fs = fstride(f);
  if (S == 0) {
#define LAUNCH(LPR, VEC)                                                                                                          \
  hipLaunchKernelGGL((attn_pool_fwd_kernel<LPR, VEC, false>), dim3(b), dim3(256), 0, ctx->stream, graph_ptr, x, ldx, a, b, f, 0, \
                     pooled, ldp, alpha, (float*)nullptr, (float*)nullptr, fs)
    ATTN_POOL_DISPATCH(lpr, vec, LAUNCH);
#undef LAUNCH
    GCNX_LAUNCH_OK(ctx);
    return GCNX_OK;
  }
  const int64_t slots = fwd_slots(n, b, S);
  GCNX_REQUIRE(ctx, slots <= INT32_MAX, "gcnx_attn_pool: too many slices");
  float* ml = scratch;
  float* part = scratch + ((2 * slots + 3) & ~(int64_t)3);
  const int32_t S32 = (int32_t)S;
#define LAUNCH(LPR, VEC)                                                                                                           \
  hipLaunchKernelGGL((attn_pool_fwd_kernel<LPR, VEC, true>), dim3((unsigned)slots), dim3(256), 0, ctx->stream, graph_ptr, x, ldx, \
                     a, b, f, S32, pooled, ldp, alpha, ml, part, fs)
  ATTN_POOL_DISPATCH(lpr, vec, LAUNCH);
#undef LAUNCH
  GCNX_LAUNCH_OK(ctx);
  hipLaunchKernelGGL(attn_pool_combine_kernel, dim3(b), dim3(256), 0, ctx->stream, graph_ptr, f, S32, (const float*)ml,
                     (const float*)part, fs, pooled, ldp, alpha);
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

int gcnx_attn_pool_bwd(gcnx_ctx* ctx, const int32_t* graph_ptr, const float* x, int64_t ldx, const float* a, const float* alpha,
                       const float* pooled, int64_t ldp, const float* dpooled, int64_t lddp, int32_t n, int32_t b, int32_t f,
                       float* dx, int64_t lddx, float* da, float* scratch) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "attention pool bwd");
  GCNX_REQUIRE(ctx, n >= 0 && b >= 0 && f >= 0, "gcnx_attn_pool_bwd: negative size");
  if (n == 0 || b == 0 || f == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, graph_ptr && x && a && alpha && pooled && dpooled, "gcnx_attn_pool_bwd: NULL pointer");
  GCNX_REQUIRE(ctx, f <= 256, "gcnx_attn_pool_bwd: f = %d, at most 256 columns", f);
  GCNX_REQUIRE(ctx, ldx >= f && ldp >= f && lddp >= f && (!dx || lddx >= f), "gcnx_attn_pool_bwd: leading dimension too small");
  GCNX_REQUIRE(ctx, !da || scratch, "gcnx_attn_pool_bwd: da needs scratch");
  GCNX_REQUIRE(ctx, gcnx_aligned16(scratch), "gcnx_attn_pool_bwd: scratch must be 16-byte aligned");
  if (!dx && !da) return GCNX_OK;
  const int lpr = lanes_per_row(f);
  const int vec = f % 4 == 0 && ldx % 4 == 0 && ldp % 4 == 0 && lddp % 4 == 0 && (!dx || lddx % 4 == 0) && gcnx_aligned16(x) &&
                  gcnx_aligned16(a) && gcnx_aligned16(pooled) && gcnx_aligned16(dpooled) && gcnx_aligned16(dx);
  const int64_t fs = fstride(f), rows = bwd_rows(n), nparts = (n + rows - 1) / rows;
  float* part = da ? scratch : nullptr;
#define LAUNCH(LPR, VEC)                                                                                                        \
  hipLaunchKernelGGL((attn_pool_bwd_kernel<LPR, VEC>), dim3((unsigned)nparts), dim3(256), 0, ctx->stream, graph_ptr, b, x, ldx, a, \
                     alpha, pooled, ldp, dpooled, lddp, n, f, rows, dx, lddx, part, fs)
  ATTN_POOL_DISPATCH(lpr, vec, LAUNCH);
#undef LAUNCH
  GCNX_LAUNCH_OK(ctx);
  if (da) {
    hipLaunchKernelGGL(attn_pool_da_kernel, dim3(gcnx_cdiv(f, 16)), dim3(256), 0, ctx->stream, (const float*)part, nparts, f, fs, da);
    GCNX_LAUNCH_OK(ctx);
  }
  return GCNX_OK;
}

}  // extern "C"
