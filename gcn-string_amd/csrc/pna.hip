// PNAConv's neighbourhood statistics (PyG PNAConv, aggregators mean / min / max / std, scalers identity / amplification /
// attenuation, towers = 1): four statistics of the same messages from ONE gather of the neighbour rows, and their backward.
//
//     M_ij = P_i + Q_j        (the pre layer is linear: P = x W_pre[:F] + b_pre, Q = x W_pre[F:], formed per node by the caller)
//     A_i  = [ P_i + mean_j Q_j | P_i + min_j Q_j | P_i + max_j Q_j | sqrt(relu(var_j Q_j) + 1e-5) ]      (a row without entries:
//     C_i  = [ x_i | A_i | s_amp,i A_i | s_att,i A_i ]                                                     A_i = [0 | 0 | 0 | sqrt(1e-5)])
//     s_amp,i = log(max(d_i, 1) + 1) / delta,   s_att,i = delta / log(max(d_i, 1) + 1)
//
// Composed from existing calls this is one gcnx_spmm_csr and two gcnx_spmm_csr_minmax -- three gathers of the same rows -- and
// the std has no kernel.  Here a lane group walks a row's entries once, in CSR order, and keeps per column the shifted sum,
// the shifted sum of squares, the minimum, the maximum and the two tie counts.  The variance is formed on values shifted by
// the row's first gathered entry K (s1 = sum (q - K), s2 = sum (q - K)^2, var = s2 / d - (s1 / d)^2): the plain
// E[q^2] - E[q]^2 loses the std to 1e-3 relative at Q = 100 + N(0, 1).  A row whose entries are all equal has s1 = s2 = 0
// exactly, so its std is sqrt(1e-5) to the bit.  fp32, no atomics: the same bits on every call.
//
// Shape of the launches (gin_aggregate_kernel's, copied -- not shared: that file's tests are yardsticks): 256 threads, a
// power-of-two lane group per row with the column on the lane, float4 lanes when f % 4 == 0 and every operand allows 16-byte
// accesses, scalar lanes otherwise; blockIdx.y walks the column chunks of rows wider than 64 lanes.  Rows of any length
// (hub rows) loop over global memory.  Element offsets are 64-bit.
//
// Backward, two launches:
//   pna_bwd_target_kernel   per target i: folds the 12 blocks of dC with the scalers into (g_mean, g_min, g_max, g_std), writes
//                           dP_i = g_mean + g_min + g_max (0 for an empty row) and the four coefficient rows
//                           [g_mean / d | g_min / cmin | g_max / cmax | g_std [max > min] / (d std)] into scratch [n, 4f]
//   pna_bwd_source_kernel   per source j, over the transposed pattern in its stored order:
//                           dQ_j = sum_i coef_mean + coef_min [Q_j == minQ_i] + coef_max [Q_j == maxQ_i] + coef_std (Q_j - meanQ_i)
// [max > min] is the gate of the relu under the root: the variance of a row is positive exactly when its entries differ.
#include "common.h"

// No contraction of a * b + c beyond the fmaf calls written out below: the float4 and the scalar instantiations then
// perform the same IEEE operations, and an operand's alignment does not change a bit of the result.
#pragma clang fp contract(off)

namespace {

constexpr float kPnaEps = 1e-5f;

template <int VEC> struct PnaVec;
template <> struct PnaVec<4> {
  float v[4];
  __device__ __forceinline__ void load(const float* p) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  }
  __device__ __forceinline__ void store(float* p) const { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};
template <> struct PnaVec<1> {
  float v[1];
  __device__ __forceinline__ void load(const float* p) { v[0] = *p; }
  __device__ __forceinline__ void store(float* p) const { *p = v[0]; }
};

struct PnaFwdArgs {
  const int32_t* rowptr; const int32_t* colidx;
  const float* x; int64_t ldx;           // [n, f]: copied into block 0 of c
  const float* pq; int64_t ldpq;         // [n, 2f] = P | Q
  float delta;                           // avg_deg_log
  float* c; int64_t ldc;                 // [n, 13f]
  float* stats; int64_t lds;             // [n, 6f] = meanQ | minQ | maxQ | std | cmin | cmax (may be NULL)
  int32_t n, f; int lpr_log2;
};

__device__ __forceinline__ void pna_scalers(int d, float delta, float& amp, float& att) {
  const float l = logf((float)(d > 1 ? d : 1) + 1.0f);
  amp = l / delta;
  att = delta / l;
}

template <int VEC>
__global__ __launch_bounds__(256) void pna_aggregate_kernel(PnaFwdArgs p) {
  const int lpr = 1 << p.lpr_log2, rpb = 256 >> p.lpr_log2;
  const int g = threadIdx.x >> p.lpr_log2, sub = threadIdx.x & (lpr - 1);
  const int64_t r = (int64_t)blockIdx.x * rpb + g;
  const int col = (blockIdx.y * lpr + sub) * VEC;
  if (r >= p.n || col >= p.f) return;
  const int64_t f = p.f;
  const int b = p.rowptr[r], e = p.rowptr[r + 1], d = e - b;
  const float* q0 = p.pq + f + col;                    // Q's column piece of row 0
  PnaVec<VEC> own, pi, mean, mn, mx, sd, cmn, cmx;
  own.load(p.x + r * p.ldx + col);
  pi.load(p.pq + r * p.ldpq + col);
  if (d == 0) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      mean.v[k] = 0.f; mn.v[k] = 0.f; mx.v[k] = 0.f; sd.v[k] = sqrtf(kPnaEps); cmn.v[k] = 0.f; cmx.v[k] = 0.f;
      pi.v[k] = 0.f;                                   // an empty row's mean / min / max are 0, not P_i
    }
  } else {
    PnaVec<VEC> kf;                                    // the shift: the row's first gathered entry
    kf.load(q0 + (int64_t)p.colidx[b] * p.ldpq);
    float s1[VEC], s2[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      s1[k] = 0.f; s2[k] = 0.f; mn.v[k] = kf.v[k]; mx.v[k] = kf.v[k]; cmn.v[k] = 1.f; cmx.v[k] = 1.f;
    }
    auto take = [&](const PnaVec<VEC>& h) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const float q = h.v[k], t = q - kf.v[k];
        s1[k] += t;
        s2[k] = fmaf(t, t, s2[k]);
        cmn.v[k] = q < mn.v[k] ? 1.f : (q == mn.v[k] ? cmn.v[k] + 1.f : cmn.v[k]);
        mn.v[k] = fminf(q, mn.v[k]);
        cmx.v[k] = q > mx.v[k] ? 1.f : (q == mx.v[k] ? cmx.v[k] + 1.f : cmx.v[k]);
        mx.v[k] = fmaxf(q, mx.v[k]);
      }
    };
    int i = b + 1;                                     // (entry b is K itself: t = 0, counted in cmn / cmx above)
    for (; i + 4 <= e; i += 4) {                       // stored order: the same bits in every run
      PnaVec<VEC> h[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) h[u].load(q0 + (int64_t)p.colidx[i + u] * p.ldpq);
#pragma unroll
      for (int u = 0; u < 4; ++u) take(h[u]);
    }
    for (; i < e; ++i) {
      PnaVec<VEC> h;
      h.load(q0 + (int64_t)p.colidx[i] * p.ldpq);
      take(h);
    }
    const float inv = 1.0f / (float)d;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const float m1 = s1[k] * inv;
      mean.v[k] = kf.v[k] + m1;
      const float var = mx.v[k] > mn.v[k] ? fmaxf(fmaf(-m1, m1, s2[k] * inv), 0.f) : 0.f;
      sd.v[k] = sqrtf(var + kPnaEps);
    }
  }
  if (p.stats) {
    float* s = p.stats + r * p.lds + col;
    mean.store(s); mn.store(s + f); mx.store(s + 2 * f); sd.store(s + 3 * f); cmn.store(s + 4 * f); cmx.store(s + 5 * f);
  }
  float amp, att;
  pna_scalers(d, p.delta, amp, att);
  PnaVec<VEC> a[4];
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    a[0].v[k] = pi.v[k] + mean.v[k]; a[1].v[k] = pi.v[k] + mn.v[k]; a[2].v[k] = pi.v[k] + mx.v[k]; a[3].v[k] = sd.v[k];
  }
  float* c = p.c + r * p.ldc + col;
  own.store(c);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    PnaVec<VEC> up, dn;
#pragma unroll
    for (int k = 0; k < VEC; ++k) { up.v[k] = amp * a[j].v[k]; dn.v[k] = att * a[j].v[k]; }
    a[j].store(c + (1 + j) * f);
    up.store(c + (5 + j) * f);
    dn.store(c + (9 + j) * f);
  }
}

struct PnaBwdArgs {
  const int32_t* rowptr;                 // the forward pattern: d_i
  const int32_t* rowptr_t; const int32_t* colidx_t;
  const float* pq; int64_t ldpq;
  const float* stats; int64_t lds;
  const float* dc; int64_t lddc;         // [n, 13f]; block 0 is not read
  float delta;
  float* dpq; int64_t lddpq;             // [n, 2f] = dP | dQ
  float* coef;                           // scratch [n, 4f]
  int32_t n, f; int lpr_log2;
};

template <int VEC>
__global__ __launch_bounds__(256) void pna_bwd_target_kernel(PnaBwdArgs p) {
  const int lpr = 1 << p.lpr_log2, rpb = 256 >> p.lpr_log2;
  const int g = threadIdx.x >> p.lpr_log2, sub = threadIdx.x & (lpr - 1);
  const int64_t r = (int64_t)blockIdx.x * rpb + g;
  const int col = (blockIdx.y * lpr + sub) * VEC;
  if (r >= p.n || col >= p.f) return;
  const int64_t f = p.f;
  const int d = p.rowptr[r + 1] - p.rowptr[r];
  float* coef = p.coef + r * 4 * f + col;
  PnaVec<VEC> dp, co[4];
  if (d == 0) {                                        // nothing gathers these rows; zeros keep the scratch defined
#pragma unroll
    for (int k = 0; k < VEC; ++k) dp.v[k] = 0.f;
    dp.store(p.dpq + r * p.lddpq + col);
#pragma unroll
    for (int j = 0; j < 4; ++j) dp.store(coef + j * f);
    return;
  }
  float amp, att;
  pna_scalers(d, p.delta, amp, att);
  const float* dc = p.dc + r * p.lddc + col;
  PnaVec<VEC> gr[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    PnaVec<VEC> gi, ga, gt;
    gi.load(dc + (1 + j) * f); ga.load(dc + (5 + j) * f); gt.load(dc + (9 + j) * f);
#pragma unroll
    for (int k = 0; k < VEC; ++k) gr[j].v[k] = fmaf(att, gt.v[k], fmaf(amp, ga.v[k], gi.v[k]));
  }
  const float* s = p.stats + r * p.lds + col;
  PnaVec<VEC> mn, mx, sd, cmn, cmx;
  mn.load(s + f); mx.load(s + 2 * f); sd.load(s + 3 * f); cmn.load(s + 4 * f); cmx.load(s + 5 * f);
  const float fd = (float)d;
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    dp.v[k] = (gr[0].v[k] + gr[1].v[k]) + gr[2].v[k];
    co[0].v[k] = gr[0].v[k] / fd;
    co[1].v[k] = gr[1].v[k] / cmn.v[k];
    co[2].v[k] = gr[2].v[k] / cmx.v[k];
    co[3].v[k] = mx.v[k] > mn.v[k] ? gr[3].v[k] / (fd * sd.v[k]) : 0.f;
  }
  dp.store(p.dpq + r * p.lddpq + col);
#pragma unroll
  for (int j = 0; j < 4; ++j) co[j].store(coef + j * f);
}

template <int VEC>
__global__ __launch_bounds__(256) void pna_bwd_source_kernel(PnaBwdArgs p) {
  const int lpr = 1 << p.lpr_log2, rpb = 256 >> p.lpr_log2;
  const int g = threadIdx.x >> p.lpr_log2, sub = threadIdx.x & (lpr - 1);
  const int64_t r = (int64_t)blockIdx.x * rpb + g;
  const int col = (blockIdx.y * lpr + sub) * VEC;
  if (r >= p.n || col >= p.f) return;
  const int64_t f = p.f;
  const int b = p.rowptr_t[r], e = p.rowptr_t[r + 1];
  PnaVec<VEC> q, acc;
  q.load(p.pq + r * p.ldpq + f + col);
#pragma unroll
  for (int k = 0; k < VEC; ++k) acc.v[k] = 0.f;
  for (int i = b; i < e; ++i) {                        // the transposed pattern's stored order: the same bits in every run
    const int64_t t = p.colidx_t[i];
    const float* s = p.stats + t * p.lds + col;
    const float* c = p.coef + t * 4 * f + col;
    PnaVec<VEC> mean, mn, mx, c0, c1, c2, c3;
    mean.load(s); mn.load(s + f); mx.load(s + 2 * f);
    c0.load(c); c1.load(c + f); c2.load(c + 2 * f); c3.load(c + 3 * f);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      float v = c0.v[k];
      v += q.v[k] == mn.v[k] ? c1.v[k] : 0.f;
      v += q.v[k] == mx.v[k] ? c2.v[k] : 0.f;
      v = fmaf(c3.v[k], q.v[k] - mean.v[k], v);
      acc.v[k] += v;
    }
  }
  acc.store(p.dpq + r * p.lddpq + f + col);
}

// lanes per row (a power of two up to 64) and the grid for n rows of `units` lanes
bool pna_grid(int32_t n, int units, int& lpr_log2, dim3& grid) {
  lpr_log2 = 0;
  while ((1 << lpr_log2) < units && lpr_log2 < 6) ++lpr_log2;
  const int ny = gcnx_cdiv(units, 1 << lpr_log2);
  grid = dim3(gcnx_cdiv(n, 256 >> lpr_log2), ny);
  return ny <= 65535;
}

bool pna_vec_ok(const void* ptr, int64_t ld) { return gcnx_aligned16(ptr) && ld % 4 == 0; }

}  // namespace

extern "C" {

int gcnx_pna_aggregate(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* x, int64_t ldx, const float* pq,
                       int64_t ldpq, float avg_deg_log, float* c, int64_t ldc, float* stats, int64_t lds, int32_t n, int32_t f) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "PNAConv aggregate");
  GCNX_REQUIRE(ctx, n >= 0 && f >= 1 && ldx >= f && ldpq >= 2 * (int64_t)f && ldc >= 13 * (int64_t)f && (!stats || lds >= 6 * (int64_t)f),
               "gcnx_pna_aggregate: needs n >= 0, f >= 1, ldx >= f, ldpq >= 2f, ldc >= 13f and lds >= 6f");
  GCNX_REQUIRE(ctx, avg_deg_log > 0.f, "gcnx_pna_aggregate: avg_deg_log must be positive");
  if (n == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, rowptr && colidx && x && pq && c, "gcnx_pna_aggregate: NULL pointer");
  GCNX_REQUIRE(ctx, c != x && c != pq && stats != c && (!stats || (stats != x && stats != pq)),
               "gcnx_pna_aggregate: the outputs must not alias the inputs or each other");
  const bool vec = f % 4 == 0 && pna_vec_ok(x, ldx) && pna_vec_ok(pq, ldpq) && pna_vec_ok(c, ldc) && (!stats || pna_vec_ok(stats, lds));
  PnaFwdArgs a{rowptr, colidx, x, ldx, pq, ldpq, avg_deg_log, c, ldc, stats, lds, n, f, 0};
  dim3 grid;
  GCNX_REQUIRE(ctx, pna_grid(n, vec ? f / 4 : f, a.lpr_log2, grid), "gcnx_pna_aggregate: f=%d is too wide", f);
  if (vec) hipLaunchKernelGGL((pna_aggregate_kernel<4>), grid, dim3(256), 0, ctx->stream, a);
  else hipLaunchKernelGGL((pna_aggregate_kernel<1>), grid, dim3(256), 0, ctx->stream, a);
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

int gcnx_pna_bwd_scratch_floats(int64_t n, int32_t f, int64_t* out) {
  if (!out || n < 0 || f < 1) return GCNX_ERR_INVALID;
  *out = 4 * n * (int64_t)f;
  return GCNX_OK;
}

int gcnx_pna_bwd(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const int32_t* rowptr_t, const int32_t* colidx_t,
                 const float* pq, int64_t ldpq, const float* stats, int64_t lds, const float* dc, int64_t lddc, float avg_deg_log,
                 float* dpq, int64_t lddpq, float* scratch, int32_t n, int32_t f) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "PNAConv backward");
  (void)colidx;                                        // the forward pattern gives the degrees; its columns are not read
  GCNX_REQUIRE(ctx, n >= 0 && f >= 1 && ldpq >= 2 * (int64_t)f && lds >= 6 * (int64_t)f && lddc >= 13 * (int64_t)f && lddpq >= 2 * (int64_t)f,
               "gcnx_pna_bwd: needs n >= 0, f >= 1, ldpq >= 2f, lds >= 6f, lddc >= 13f and lddpq >= 2f");
  GCNX_REQUIRE(ctx, avg_deg_log > 0.f, "gcnx_pna_bwd: avg_deg_log must be positive");
  if (n == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, rowptr && rowptr_t && colidx_t && pq && stats && dc && dpq && scratch, "gcnx_pna_bwd: NULL pointer");
  GCNX_REQUIRE(ctx, dpq != pq && dpq != stats && dpq != dc && dpq != scratch && scratch != pq && scratch != stats && scratch != dc,
               "gcnx_pna_bwd: dpq and scratch must not alias the inputs or each other");
  const bool vec = f % 4 == 0 && pna_vec_ok(pq, ldpq) && pna_vec_ok(stats, lds) && pna_vec_ok(dc, lddc) && pna_vec_ok(dpq, lddpq) &&
                   gcnx_aligned16(scratch);
  PnaBwdArgs a{rowptr, rowptr_t, colidx_t, pq, ldpq, stats, lds, dc, lddc, avg_deg_log, dpq, lddpq, scratch, n, f, 0};
  dim3 grid;
  GCNX_REQUIRE(ctx, pna_grid(n, vec ? f / 4 : f, a.lpr_log2, grid), "gcnx_pna_bwd: f=%d is too wide", f);
  if (vec) hipLaunchKernelGGL((pna_bwd_target_kernel<4>), grid, dim3(256), 0, ctx->stream, a);
  else hipLaunchKernelGGL((pna_bwd_target_kernel<1>), grid, dim3(256), 0, ctx->stream, a);
  GCNX_LAUNCH_OK(ctx);
  if (vec) hipLaunchKernelGGL((pna_bwd_source_kernel<4>), grid, dim3(256), 0, ctx->stream, a);
  else hipLaunchKernelGGL((pna_bwd_source_kernel<1>), grid, dim3(256), 0, ctx->stream, a);
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

}  // extern "C"
