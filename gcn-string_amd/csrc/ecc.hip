// Edge-conditioned convolution (Spektral ECCConv, single / disjoint mode) in its factorised form ("ECCConv"):
//
//   Scat[t, c*F + i] = sum over entries k with destination t of  u^_k[c] * x[src_k, i],   u^_k = [u_k, 1],  C = S' + 1
//   out = act([Scat | x] Wstack + bias)                                    (one weight GEMM: gcnx_gemm)
//
// and its backward gather.  Both kernels are row gathers without atomics: a group of LPR lanes owns one row and walks the
// row's entries in their stored order, so a result is bit-reproducible from run to run.  The chunk's column indices and
// per-entry channels wait in LDS (as spmm_rows_kernel stages its colidx / vals); every lane keeps C accumulators of VEC
// floats (VEC = 4: float4 lanes when F, the leading dimensions and the pointers allow it; VEC = 1: any F >= 1).
#include "common.h"

#include <cstdint>
#include <new>

namespace {

constexpr int kEccMaxC = 17;          // channels + the constant one: C accumulators of VEC floats per lane
constexpr int kEccStageE = 1024;      // entries of a chunk whose column index is staged in LDS
constexpr int kEccStageU = 4096;      // floats of per-entry channels staged in LDS

template <int VEC> struct EccVec;
template <> struct EccVec<4> {
  float4 v;
  __device__ __forceinline__ void zero() { v = make_float4(0.f, 0.f, 0.f, 0.f); }
  __device__ __forceinline__ void load(const float* p) { v = *reinterpret_cast<const float4*>(p); }
  __device__ __forceinline__ void store(float* p) const { *reinterpret_cast<float4*>(p) = v; }
  __device__ __forceinline__ void fma(float s, const EccVec& o) {
    v.x = fmaf(s, o.v.x, v.x); v.y = fmaf(s, o.v.y, v.y); v.z = fmaf(s, o.v.z, v.z); v.w = fmaf(s, o.v.w, v.w);
  }
  __device__ __forceinline__ void add(const EccVec& o) { v.x += o.v.x; v.y += o.v.y; v.z += o.v.z; v.w += o.v.w; }
  __device__ __forceinline__ float dot(const EccVec& o) const {
    return fmaf(v.w, o.v.w, fmaf(v.z, o.v.z, fmaf(v.y, o.v.y, v.x * o.v.x)));
  }
};
template <> struct EccVec<1> {
  float v;
  __device__ __forceinline__ void zero() { v = 0.f; }
  __device__ __forceinline__ void load(const float* p) { v = *p; }
  __device__ __forceinline__ void store(float* p) const { *p = v; }
  __device__ __forceinline__ void fma(float s, const EccVec& o) { v = fmaf(s, o.v, v); }
  __device__ __forceinline__ void add(const EccVec& o) { v += o.v; }
  __device__ __forceinline__ float dot(const EccVec& o) const { return v * o.v; }
};

// Column indices and channel rows of the chunk's first `staged` entries -> LDS.  eperm (may be NULL = identity): row of u
// that belongs to entry e.  SP = C - 1 stored channels per entry.
template <int SP>
__device__ __forceinline__ int ecc_stage(const int32_t* __restrict__ colidx, const int32_t* __restrict__ eperm,
                                         const float* __restrict__ u, int64_t ldu, int e0, int e1, int32_t* s_col, float* s_u) {
  int staged = min(e1 - e0, kEccStageE);
  if (SP > 0) staged = min(staged, kEccStageU / (SP > 0 ? SP : 1));
  for (int i = threadIdx.x; i < staged; i += blockDim.x) {
    s_col[i] = colidx[e0 + i];
    if (SP > 0) {
      const int64_t k = eperm ? (int64_t)eperm[e0 + i] : (int64_t)(e0 + i);
#pragma unroll
      for (int c = 0; c < SP; ++c) s_u[i * SP + c] = u[k * ldu + c];
    }
  }
  __syncthreads();
  return staged;
}

// Forward: one group of (1 << lpr_log2) lanes per destination row, blockIdx.y = column block of LPR * VEC columns.
// root != 0: the row's own x is copied behind the C * F aggregated columns (the operand [Scat | x] of the weight GEMM).
template <int C, int VEC>
__global__ __launch_bounds__(256) void ecc_expand_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                                         const int32_t* __restrict__ eperm, const float* __restrict__ u, int64_t ldu,
                                                         const float* __restrict__ x, int64_t ldx, int32_t f,
                                                         float* __restrict__ scat, int64_t ld, int32_t n, int lpr_log2, int root) {
  constexpr int SP = C - 1;
  __shared__ int32_t s_col[kEccStageE];
  __shared__ float s_u[SP > 0 ? kEccStageU : 1];
  const int lpr = 1 << lpr_log2, rpb = 256 >> lpr_log2;
  const int r0 = blockIdx.x * rpb, r1 = min(n, r0 + rpb);
  const int e0 = rowptr[r0], e1 = rowptr[r1];
  const int staged = ecc_stage<SP>(colidx, eperm, u, ldu, e0, e1, s_col, s_u);

  const int g = threadIdx.x >> lpr_log2, sub = threadIdx.x & (lpr - 1);
  const int r = r0 + g;
  const int col = (blockIdx.y * lpr + sub) * VEC;
  if (r >= r1 || col >= f) return;
  EccVec<VEC> acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c].zero();
  const int b = rowptr[r] - e0, e = rowptr[r + 1] - e0;
#pragma unroll 2
  for (int i = b; i < e; ++i) {               // stored order: the sum of a row is the same bits in every run
    int src;
    float uv[SP > 0 ? SP : 1];
    if (i < staged) {
      src = s_col[i];
#pragma unroll
      for (int c = 0; c < SP; ++c) uv[c] = s_u[i * SP + c];
    } else {
      src = colidx[e0 + i];
      const int64_t k = eperm ? (int64_t)eperm[e0 + i] : (int64_t)(e0 + i);
#pragma unroll
      for (int c = 0; c < SP; ++c) uv[c] = u[k * ldu + c];
    }
    EccVec<VEC> xv;
    xv.load(x + (int64_t)src * ldx + col);
#pragma unroll
    for (int c = 0; c < SP; ++c) acc[c].fma(uv[c], xv);
    acc[SP].add(xv);
  }
  float* o = scat + (int64_t)r * ld + col;
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c].store(o + (int64_t)c * f);
  if (root) {
    EccVec<VEC> xv;
    xv.load(x + (int64_t)r * ldx + col);
    xv.store(o + (int64_t)C * f);
  }
}

// Backward: one group of LPR lanes per SOURCE row s (a row of the original CSR), walking column blocks of LPR * VEC
// columns inside the launch.  Per entry k = (s, t) the lane gathers its C pieces of dScat[t] once and uses them twice:
//   dx[s, i]  = dx_root[s, i] + sum_k sum_c u^_k[c] * dScat[t_k, c*F + i]
//   du[k, c]  = sum_i x[s, i] * dScat[t_k, c*F + i]           (c < S'; lanes of the group combined by a fixed xor tree)
// dx / du may be NULL.  With more than one column block du[k, c] is built up by the same lane block after block.
template <int C, int VEC>
__global__ __launch_bounds__(256) void ecc_bwd_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                                      const float* __restrict__ u, int64_t ldu, const float* __restrict__ x, int64_t ldx,
                                                      const float* __restrict__ dscat, int64_t ldd, const float* dx_root, int64_t lddr,
                                                      int32_t f, float* dx, int64_t lddx, float* __restrict__ du, int64_t lddu,
                                                      int32_t n, int lpr_log2) {
  constexpr int SP = C - 1;
  __shared__ int32_t s_col[kEccStageE];
  __shared__ float s_u[SP > 0 ? kEccStageU : 1];
  const int lpr = 1 << lpr_log2, rpb = 256 >> lpr_log2;
  const int r0 = blockIdx.x * rpb, r1 = min(n, r0 + rpb);
  const int e0 = rowptr[r0], e1 = rowptr[r1];
  const int staged = ecc_stage<SP>(colidx, nullptr, u, ldu, e0, e1, s_col, s_u);

  const int g = threadIdx.x >> lpr_log2, sub = threadIdx.x & (lpr - 1);
  const int r = r0 + g;
  if (r >= r1) return;                        // (whole groups leave: the xor tree below stays inside a group)
  const int b = rowptr[r] - e0, e = rowptr[r + 1] - e0;
  const bool want_du = SP > 0 && du != nullptr;
  for (int cb = 0; cb * lpr * VEC < f; ++cb) {
    const int col = (cb * lpr + sub) * VEC;
    const bool col_ok = col < f;
    EccVec<VEC> acc, xv;
    acc.zero();
    xv.zero();
    if (col_ok) {
      if (dx && dx_root) acc.load(dx_root + (int64_t)r * lddr + col);
      if (want_du) xv.load(x + (int64_t)r * ldx + col);
    }
    for (int i = b; i < e; ++i) {
      int t;
      float uv[SP > 0 ? SP : 1];
      if (i < staged) {
        t = s_col[i];
#pragma unroll
        for (int c = 0; c < SP; ++c) uv[c] = s_u[i * SP + c];
      } else {
        t = colidx[e0 + i];
#pragma unroll
        for (int c = 0; c < SP; ++c) uv[c] = u[(int64_t)(e0 + i) * ldu + c];
      }
      EccVec<VEC> d[C];
#pragma unroll
      for (int c = 0; c < C; ++c) {
        d[c].zero();
        if (col_ok) d[c].load(dscat + (int64_t)t * ldd + (int64_t)c * f + col);
      }
#pragma unroll
      for (int c = 0; c < SP; ++c) acc.fma(uv[c], d[c]);
      acc.add(d[SP]);
      if (want_du) {
#pragma unroll
        for (int c = 0; c < SP; ++c) {
          float p = xv.dot(d[c]);
          for (int off = 1; off < lpr; off <<= 1) p += __shfl_xor(p, off);
          if (sub == 0) {
            float* q = du + (int64_t)(e0 + i) * lddu + c;
            *q = cb == 0 ? p : *q + p;
          }
        }
      }
    }
    if (dx && col_ok) acc.store(dx + (int64_t)r * lddx + col);
  }
}


// lanes per row: the smallest power of two that covers ceil(f / vec) columns, at most one wave
inline int ecc_lpr_log2(int32_t f, int vec) {
  const int lanes = (f + vec - 1) / vec;
  int l = 0;
  while ((1 << l) < lanes && l < 6) ++l;
  return l;
}

}  // namespace

#define GCNX_ECC_CASES(M) \
  M(1) M(2) M(3) M(4) M(5) M(6) M(7) M(8) M(9) M(10) M(11) M(12) M(13) M(14) M(15) M(16) M(17)

extern "C" {

int gcnx_ecc_expand(gcnx_ctx* ctx, const int32_t* rowptr_t, const int32_t* colidx_t, const int32_t* eperm, const float* u,
                    int64_t ldu, int32_t sp, const float* x, int64_t ldx, int32_t f, float* scat, int64_t ld, int32_t n,
                    int32_t nnz, int root) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "ECC expand (edge-conditioned aggregation)");
  GCNX_REQUIRE(ctx, n >= 0 && nnz >= 0 && f >= 0 && sp >= 0, "gcnx_ecc_expand: negative size");
  if (sp + 1 > kEccMaxC)
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_ecc_expand: %d edge channels + the constant one exceed C = %d", sp, kEccMaxC);
  if (n == 0 || f == 0) return GCNX_OK;
  const int c = sp + 1;
  GCNX_REQUIRE(ctx, rowptr_t && x && scat, "gcnx_ecc_expand: NULL pointer");
  GCNX_REQUIRE(ctx, nnz == 0 || (colidx_t && (sp == 0 || u)), "gcnx_ecc_expand: entries without colidx / u");
  GCNX_REQUIRE(ctx, ldx >= f && ld >= (int64_t)(c + (root ? 1 : 0)) * f && (sp == 0 || ldu >= sp),
               "gcnx_ecc_expand: leading dimension too small");
  const int vec = (f % 4 == 0 && ldx % 4 == 0 && ld % 4 == 0 && gcnx_aligned16(x) && gcnx_aligned16(scat)) ? 4 : 1;
  const int l2 = ecc_lpr_log2(f, vec);
  const dim3 grid(gcnx_cdiv(n, 256 >> l2), gcnx_cdiv(f, (1 << l2) * vec));
#define GCNX_ECC_FWD(C_)                                                                                                   \
  case C_:                                                                                                                 \
    if (vec == 4)                                                                                                          \
      hipLaunchKernelGGL((ecc_expand_kernel<C_, 4>), grid, dim3(256), 0, ctx->stream, rowptr_t, colidx_t, eperm, u, ldu, x, \
                         ldx, f, scat, ld, n, l2, root);                                                                   \
    else                                                                                                                   \
      hipLaunchKernelGGL((ecc_expand_kernel<C_, 1>), grid, dim3(256), 0, ctx->stream, rowptr_t, colidx_t, eperm, u, ldu, x, \
                         ldx, f, scat, ld, n, l2, root);                                                                   \
    break;
  switch (c) { GCNX_ECC_CASES(GCNX_ECC_FWD) }
#undef GCNX_ECC_FWD
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

int gcnx_ecc_bwd(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* u, int64_t ldu, int32_t sp,
                 const float* x, int64_t ldx, const float* dscat, int64_t ldd, const float* dx_root, int64_t lddr, int32_t f,
                 float* dx, int64_t lddx, float* du, int64_t lddu, int32_t n, int32_t nnz) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "ECC backward gather (dx, du)");
  GCNX_REQUIRE(ctx, n >= 0 && nnz >= 0 && f >= 0 && sp >= 0, "gcnx_ecc_bwd: negative size");
  if (sp + 1 > kEccMaxC)
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_ecc_bwd: %d edge channels + the constant one exceed C = %d", sp, kEccMaxC);
  if (sp == 0) du = nullptr;
  if (n == 0 || (!dx && !du)) return GCNX_OK;
  if (f == 0) {
    if (du && nnz) GCNX_HIP(ctx, hipMemset2DAsync(du, (size_t)lddu * 4, 0, (size_t)sp * 4, (size_t)nnz, ctx->stream));
    return GCNX_OK;
  }
  const int c = sp + 1;
  GCNX_REQUIRE(ctx, rowptr && dscat, "gcnx_ecc_bwd: NULL pointer");
  GCNX_REQUIRE(ctx, nnz == 0 || (colidx && (sp == 0 || u)), "gcnx_ecc_bwd: entries without colidx / u");
  GCNX_REQUIRE(ctx, !du || x, "gcnx_ecc_bwd: du needs x");
  GCNX_REQUIRE(ctx, ldd >= (int64_t)c * f && (!du || (ldx >= f && lddu >= sp)) && (sp == 0 || ldu >= sp) &&
                        (!dx || (lddx >= f && (!dx_root || lddr >= f))),
               "gcnx_ecc_bwd: leading dimension too small");
  const bool al = f % 4 == 0 && ldd % 4 == 0 && gcnx_aligned16(dscat) && (!du || (ldx % 4 == 0 && gcnx_aligned16(x))) &&
                  (!dx || (lddx % 4 == 0 && gcnx_aligned16(dx) && (!dx_root || (lddr % 4 == 0 && gcnx_aligned16(dx_root)))));
  const int vec = al ? 4 : 1;
  const int l2 = ecc_lpr_log2(f, vec);
  const dim3 grid(gcnx_cdiv(n, 256 >> l2));
#define GCNX_ECC_BWD(C_)                                                                                                  \
  case C_:                                                                                                                \
    if (vec == 4)                                                                                                         \
      hipLaunchKernelGGL((ecc_bwd_kernel<C_, 4>), grid, dim3(256), 0, ctx->stream, rowptr, colidx, u, ldu, x, ldx, dscat,  \
                         ldd, dx_root, lddr, f, dx, lddx, du, lddu, n, l2);                                               \
    else                                                                                                                  \
      hipLaunchKernelGGL((ecc_bwd_kernel<C_, 1>), grid, dim3(256), 0, ctx->stream, rowptr, colidx, u, ldu, x, ldx, dscat,  \
                         ldd, dx_root, lddr, f, dx, lddx, du, lddu, n, l2);                                               \
    break;
  switch (c) { GCNX_ECC_CASES(GCNX_ECC_BWD) }
#undef GCNX_ECC_BWD
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

// gcnx_csr_transpose that also returns where every transposed entry came from: perm_t[p] = index of the entry of the
// original CSR that became entry p of the transpose (the row of the per-entry features that belongs to it).  Integers
// throughout -- a float value array of entry numbers stops being exact at 2^24 entries.  Stable counting sort on the host,
// as gcnx_csr_transpose.
int gcnx_csr_transpose_perm(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, int32_t n, int32_t nnz,
                            int32_t* rowptr_t, int32_t* colidx_t, int32_t* perm_t) {
  GCNX_CHECK_CTX(ctx);
  GCNX_REQUIRE(ctx, n >= 0 && nnz >= 0, "gcnx_csr_transpose_perm: negative size");
  GCNX_REQUIRE(ctx, rowptr && rowptr_t, "gcnx_csr_transpose_perm: NULL rowptr");
  GCNX_REQUIRE(ctx, nnz == 0 || (colidx && colidx_t && perm_t), "gcnx_csr_transpose_perm: NULL colidx / perm");
  GCNX_REQUIRE(ctx, !ctx->capturing, "gcnx_csr_transpose_perm synchronises and cannot be captured");
  try {
    std::vector<int32_t> rp((size_t)n + 1), ci((size_t)nnz), rpt((size_t)n + 1, 0), cit((size_t)nnz), pt((size_t)nnz);
    GCNX_HIP(ctx, hipMemcpyAsync(rp.data(), rowptr, rp.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (nnz) GCNX_HIP(ctx, hipMemcpyAsync(ci.data(), colidx, ci.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    GCNX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (rp[0] != 0 || rp[n] != nnz)
      return gcnx_fail(ctx, GCNX_ERR_DATA, "gcnx_csr_transpose_perm: rowptr[0]=%d, rowptr[n]=%d != nnz=%d", rp[0], rp[n], nnz);
    for (int32_t r = 0; r < n; ++r)
      if (rp[r + 1] < rp[r]) return gcnx_fail(ctx, GCNX_ERR_DATA, "gcnx_csr_transpose_perm: rowptr decreases at row %d", r);
    for (int32_t e = 0; e < nnz; ++e) {
      if (ci[e] < 0 || ci[e] >= n)
        return gcnx_fail(ctx, GCNX_ERR_DATA, "gcnx_csr_transpose_perm: colidx[%d]=%d out of range", e, ci[e]);
      rpt[(size_t)ci[e] + 1]++;
    }
    for (int32_t r = 0; r < n; ++r) rpt[r + 1] += rpt[r];
    std::vector<int32_t> cur(rpt.begin(), rpt.end() - 1);
    for (int32_t r = 0; r < n; ++r)
      for (int32_t e = rp[r]; e < rp[r + 1]; ++e) {
        const int32_t p = cur[ci[e]]++;
        cit[p] = r;
        pt[p] = e;
      }
    GCNX_HIP(ctx, hipMemcpyAsync(rowptr_t, rpt.data(), rpt.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    if (nnz) {
      GCNX_HIP(ctx, hipMemcpyAsync(colidx_t, cit.data(), cit.size() * 4, hipMemcpyHostToDevice, ctx->stream));
      GCNX_HIP(ctx, hipMemcpyAsync(perm_t, pt.data(), pt.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    GCNX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  } catch (const std::bad_alloc&) {
    return gcnx_fail(ctx, GCNX_ERR_NOMEM, "gcnx_csr_transpose_perm: out of host memory");
  }
  return GCNX_OK;
}

}  // extern "C"
