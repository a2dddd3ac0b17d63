// What gcnx.Explainer (GNNExplainer over a frozen gcnx.GCN) adds to the library: the gradient with respect to the
// VALUE of every stored entry of the operator, and the soft masks on entries and input features with their regularisers.
//
//     out[e] (+)= scale[e] <L[row(e), :f], R[colidx[e], :f]>                                              gcnx_sddmm_csr
//     v[e] = A^[e] sigma(m[e]) off the diagonal, A^[e] on it;  v_t[p] = v[perm_t[p]]                      gcnx_edge_mask_fwd
//     dm[e] = (dv[e] A^[e] + c_size + c_ent ent'(sigma(m[e]))) sigma'(m[e]) off the diagonal, 0 on it     gcnx_edge_mask_bwd
//     X' = X * sigma(f)   (f: one row for all nodes, or one per node)                                     gcnx_feat_mask_fwd
//     df = (dX' * X (its column sums for the one-row form) + c_size + c_ent ent'(sigma(f))) sigma'(f)     gcnx_feat_mask_bwd
//     ent(p) = -p log(p + 1e-15) - (1 - p) log(1 - p + 1e-15)
//
// The sampled dense-dense product is the hot path.  Shape of a workgroup (gat_bwd_edges'; the device helpers: conv_tile.h): 32
// rows, one lane group of f / 4 lanes per row with one float4 of the target row L[i] each, kept in registers over the row's
// entries; the tile's column indices staged in LDS (1024 of them, the rest read from global memory); the source rows R[j]
// gathered with range-checked 16-byte buffer loads, four entries per trip; dot4, then an xor butterfly over the group (swizzles
// and quad permutations with constant masks: no per-lane address); the group's first lane stores.  Widths 16, 32, 64, 128 with
// 16-byte aligned operands; every other width, alignment and leading dimension runs on sddmm_any_kernel (a wave per row, lane
// groups of the next power of two >= f per entry).  Every out[e] has one writer and one summation order: no atomics, the same
// call leaves the same bits.  The two regulariser sums are folded in a fixed order: per-workgroup partials, then one workgroup
// (as gcnx_grad_sqnorm and its consumer do).
#include <cmath>

#include "common.h"
#include "conv_tile.h"

namespace {

constexpr int kMaskThreads = 256;
constexpr int kMaskMaxParts = 256;        // workgroups (= partial sums) of a mask launch
constexpr int kFeatChunk = 64;            // rows per workgroup of the column-sum stage
constexpr float kEntEps = 1e-15f;

// sum over the LPR (4, 8, 16 or 32) consecutive lanes of a group: every lane ends with the same bits
template <int LPR>
__device__ __forceinline__ float group_sum(float v) {
  if (LPR >= 32) v += swz_xor<16>(v);
  if (LPR >= 16) v += swz_xor<8>(v);
  if (LPR >= 8) v += swz_xor<4>(v);
  v += quad_perm<0x4E>(v);
  v += quad_perm<0xB1>(v);
  return v;
}

struct SddmmArgs {
  const int32_t* rowptr; const int32_t* colidx;
  int32_t n, f;
  const float* l; int64_t ldl;
  const float* r; int64_t ldr;
  const float* scale;
  float* out;
  int accumulate;
};

__device__ __forceinline__ void sddmm_store(const SddmmArgs& p, int64_t e, float d) {
  float v = p.scale ? p.scale[e] * d : d;
  if (p.accumulate) v += p.out[e];
  p.out[e] = v;
}

// ---- widths 16, 32, 64, 128, aligned operands ------------------------------------------------------------------------------
template <int F>
__global__ __launch_bounds__(8 * F) void sddmm_tile_kernel(SddmmArgs p) {
  constexpr int LPR = F / 4, NT = 8 * F;
  __shared__ int32_t s_col[kTileCap];
  __shared__ int32_t s_rp[kTileRows + 1];
  const int tid = threadIdx.x, r = tid / LPR, sub = tid % LPR;
  const ConvTile t = conv_tile(p.rowptr, p.n, s_rp, kTileRows);
  const int staged = min(t.e1 - t.e0, kTileCap);
  for (int i = tid; i < staged; i += NT) s_col[i] = p.colidx[t.e0 + i];
  __syncthreads();
  const bool live = r < t.nr;
  const int ea = live ? s_rp[r] - t.e0 : 0, eb = live ? s_rp[r + 1] - t.e0 : 0;
  const float4 lv = live ? load4(p.l + (int64_t)(t.r0 + r) * p.ldl + 4 * sub) : zero4();
  const unsigned ld4 = (unsigned)p.ldr * 4u, sub16 = (unsigned)sub * 16u;
  const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.r, (short)0, (int)((unsigned)(p.n - 1) * ld4 + (unsigned)F * 4u), 0x00020000);
  const int32_t* __restrict__ gcol = p.colidx + t.e0;
  for (int e = ea; e < eb; e += kTileU) {                   // (the lanes of a row share ea and eb: they exchange together)
    float4 rv[kTileU];
#pragma unroll
    for (int u = 0; u < kTileU; ++u) {
      const bool ok = e + u < eb;
      const int ee = ok ? e + u : e;
      const int col = ee < kTileCap ? s_col[ee] : gcol[ee];
      rv[u] = buf4(rr, ok ? (unsigned)col * ld4 + sub16 : kOffOut);
    }
#pragma unroll
    for (int u = 0; u < kTileU; ++u) {
      const float d = group_sum<LPR>(dot4(lv, rv[u]));
      if (sub == 0 && e + u < eb) sddmm_store(p, (int64_t)t.e0 + e + u, d);
    }
  }
}

// ---- every other width, alignment and leading dimension: a wave per row, a group of g lanes (a power of two) per entry -------
__global__ __launch_bounds__(256) void sddmm_any_kernel(SddmmArgs p, int g) {
  const int lane = threadIdx.x & 63, grp = lane / g, sub = lane % g, epw = 64 / g;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.n) return;                                   // (whole waves leave; the exchanges below stay inside a wave)
  const int ea = p.rowptr[row], eb = p.rowptr[row + 1];
  const float* __restrict__ lrow = p.l + row * p.ldl;
  for (int base = ea; base < eb; base += epw) {
    const int e = base + grp;
    const bool ok = e < eb;
    float d = 0.f;
    if (ok) {
      const float* __restrict__ rrow = p.r + (int64_t)p.colidx[e] * p.ldr;
      for (int k = sub; k < p.f; k += g) d = fmaf(lrow[k], rrow[k], d);
    }
    for (int off = g >> 1; off > 0; off >>= 1) d += __shfl_xor(d, off);
    if (ok && sub == 0) sddmm_store(p, e, d);
  }
}

// ---- masks (row_of: conv_tile.h) ----------------------------------------------------------------------------------------------
// s = sigmoid(a) and q = 1 - s without the cancellation of 1 - s near s = 1: q = exp(-a) s there (exp(-a) <= 1: no overflow)
struct Sig { float s, q; };
__device__ __forceinline__ Sig sig2(float a) {
  const float e = __expf(-a);
  const float s = __builtin_amdgcn_rcpf(1.0f + e);
  return Sig{s, a >= 0.f ? e * s : 1.0f - s};
}
__device__ __forceinline__ float ent1(Sig p) { return -p.s * logf(p.s + kEntEps) - p.q * logf(p.q + kEntEps); }
// d ent / d s
__device__ __forceinline__ float dent1(Sig p) {
  const float a = p.s + kEntEps, b = p.q + kEntEps;
  return -logf(a) - p.s / a + logf(b) + p.q / b;
}

__device__ __forceinline__ float masked_value(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx, int n,
                                              const float* __restrict__ a_vals, const float* __restrict__ logits, int e) {
  const float a = a_vals[e];
  return colidx[e] == row_of(rowptr, n, e) ? a : a * sigmoid1(logits[e]);
}

__global__ __launch_bounds__(kMaskThreads) void edge_mask_fwd_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                                                     int32_t n, int32_t nnz, const float* __restrict__ a_vals,
                                                                     const float* __restrict__ logits, const int32_t* __restrict__ perm_t,
                                                                     float* __restrict__ vals_out, float* __restrict__ vals_t_out) {
  const int e = blockIdx.x * kMaskThreads + threadIdx.x;
  if (e >= nnz) return;
  vals_out[e] = masked_value(rowptr, colidx, n, a_vals, logits, e);
  if (vals_t_out) vals_t_out[e] = masked_value(rowptr, colidx, n, a_vals, logits, perm_t[e]);   // the same expression: the same bits
}

// (x, y) summed over the workgroup's 256 threads in a fixed order: lane += lane + off for off = 32 .. 1, then the four wave sums
// as ((s0 + s1) + s2) + s3; valid in thread 0
__device__ __forceinline__ float2 block_sum2(float x, float y, float2* s_w) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { x += __shfl_down(x, off); y += __shfl_down(y, off); }
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = make_float2(x, y);
  __syncthreads();
  const float2 a = s_w[0], b = s_w[1], c = s_w[2], d = s_w[3];
  return make_float2(((a.x + b.x) + c.x) + d.x, ((a.y + b.y) + c.y) + d.y);
}

__global__ __launch_bounds__(kMaskThreads) void edge_mask_bwd_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                                                     int32_t n, int32_t nnz, const float* __restrict__ a_vals,
                                                                     const float* __restrict__ logits, const float* __restrict__ dv,
                                                                     float c_size, float c_ent, float* __restrict__ dlogits,
                                                                     float* __restrict__ part) {
  __shared__ float2 s_w[4];
  float ssum = 0.f, esum = 0.f;
  for (int e = blockIdx.x * kMaskThreads + threadIdx.x; e < nnz; e += gridDim.x * kMaskThreads) {   // ascending per thread
    float g = 0.f;
    if (colidx[e] != row_of(rowptr, n, e)) {
      const Sig p = sig2(logits[e]);
      g = (dv[e] * a_vals[e] + c_size + c_ent * dent1(p)) * (p.s * p.q);
      ssum += p.s;
      esum += ent1(p);
    }
    dlogits[e] = g;
  }
  const float2 t = block_sum2(ssum, esum, s_w);
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = t.x; part[2 * blockIdx.x + 1] = t.y; }
}

// terms[0 .. 1] = the partial pairs summed: thread j takes pair j (nparts <= 256), then block_sum2's order
__global__ __launch_bounds__(kMaskThreads) void mask_terms_kernel(const float* __restrict__ part, int nparts, float* __restrict__ terms) {
  __shared__ float2 s_w[4];
  const bool ok = (int)threadIdx.x < nparts;
  const float2 t = block_sum2(ok ? part[2 * threadIdx.x] : 0.f, ok ? part[2 * threadIdx.x + 1] : 0.f, s_w);
  if (threadIdx.x == 0) { terms[0] = t.x; terms[1] = t.y; }
}

__global__ __launch_bounds__(kMaskThreads) void feat_mask_fwd_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ logits,
                                                                     int per_row, int64_t n, int32_t f, float* __restrict__ out, int64_t ldo) {
  const int64_t total = n * f;
  for (int64_t i = (int64_t)blockIdx.x * kMaskThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kMaskThreads) {
    const int64_t r = i / f;
    const int k = (int)(i - r * f);
    out[r * ldo + k] = x[r * ldx + k] * sigmoid1(logits[per_row ? i : k]);
  }
}

// one logit per element: the gradient where it stands, the workgroup's share of the two sums
__global__ __launch_bounds__(kMaskThreads) void feat_mask_bwd_rows_kernel(const float* __restrict__ dxm, int64_t ldd, const float* __restrict__ x,
                                                                          int64_t ldx, const float* __restrict__ logits, int64_t n, int32_t f,
                                                                          float c_size, float c_ent, float* __restrict__ dlogits,
                                                                          float* __restrict__ part) {
  __shared__ float2 s_w[4];
  float ssum = 0.f, esum = 0.f;
  const int64_t total = n * f;
  for (int64_t i = (int64_t)blockIdx.x * kMaskThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kMaskThreads) {
    const int64_t r = i / f;
    const int k = (int)(i - r * f);
    const Sig p = sig2(logits[i]);
    dlogits[i] = (dxm[r * ldd + k] * x[r * ldx + k] + c_size + c_ent * dent1(p)) * (p.s * p.q);
    ssum += p.s;
    esum += ent1(p);
  }
  const float2 t = block_sum2(ssum, esum, s_w);
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = t.x; part[2 * blockIdx.x + 1] = t.y; }
}

// One logit per column.  Both stages take fw (a power of two <= 256) columns at a time with 256 / fw lanes per column: lane j adds
// items j, j + 256 / fw, ... in ascending order, then the column's first lane adds the lanes' sums in ascending order (lanes_sum).
// fp64 accumulators: the products are exact and the sum may cancel; one fp32 rounding per part.  (One thread per column left 16 of
// the 256 threads at work at f = 16, on 254 dependent trips in stage 2 at config 2's 20 498 rows: 36 us of a 0.446 ms step.)
__device__ __forceinline__ double lanes_sum(double acc, int fw, double* s_acc) {
  s_acc[threadIdx.x] = acc;
  __syncthreads();
  double t = 0.0;
  if ((int)threadIdx.x < fw)
    for (int j = 0; j < kMaskThreads / fw; ++j) t += s_acc[j * fw + threadIdx.x];
  __syncthreads();
  return t;                                                 // (valid in the first fw threads)
}

// stage 1: part[b][k] = sum over the rows of chunk b of dX'[i, k] x[i, k]
__global__ __launch_bounds__(kMaskThreads) void feat_mask_colpart_kernel(const float* __restrict__ dxm, int64_t ldd, const float* __restrict__ x,
                                                                         int64_t ldx, int64_t n, int32_t f, int64_t rows_per_part,
                                                                         int fw, float* __restrict__ part) {
  __shared__ double s_acc[kMaskThreads];
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_part;
  const int64_t r1 = r0 + rows_per_part < n ? r0 + rows_per_part : n;
  const int lanes = kMaskThreads / fw, lane = threadIdx.x / fw;
  for (int k0 = 0; k0 < f; k0 += fw) {                      // (uniform trip count: the barriers are reached by every thread)
    const int k = k0 + threadIdx.x % fw;
    double acc = 0.0;
    if (k < f)
      for (int64_t r = r0 + lane; r < r1; r += lanes) acc += (double)dxm[r * ldd + k] * (double)x[r * ldx + k];
    const double t = lanes_sum(acc, fw, s_acc);
    if (lane == 0 && k < f) part[(int64_t)blockIdx.x * f + k] = (float)t;
  }
}

// stage 2 (one workgroup): the parts of a column, the gradient of its logit, the two sums
__global__ __launch_bounds__(kMaskThreads) void feat_mask_common_kernel(const float* __restrict__ part, int nparts, const float* __restrict__ logits,
                                                                        int32_t f, int fw, float c_size, float c_ent, float* __restrict__ dlogits,
                                                                        float* __restrict__ terms) {
  __shared__ double s_acc[kMaskThreads];
  __shared__ float2 s_w[4];
  const int lanes = kMaskThreads / fw, lane = threadIdx.x / fw;
  float ssum = 0.f, esum = 0.f;
  for (int k0 = 0; k0 < f; k0 += fw) {
    const int k = k0 + threadIdx.x % fw;
    double acc = 0.0;
    if (k < f)
      for (int b = lane; b < nparts; b += lanes) acc += (double)part[(int64_t)b * f + k];
    const double t = lanes_sum(acc, fw, s_acc);
    if (lane == 0 && k < f) {
      const Sig p = sig2(logits[k]);
      dlogits[k] = ((float)t + c_size + c_ent * dent1(p)) * (p.s * p.q);
      ssum += p.s;
      esum += ent1(p);
    }
  }
  const float2 t = block_sum2(ssum, esum, s_w);
  if (threadIdx.x == 0) { terms[0] = t.x; terms[1] = t.y; }
}

int mask_parts(int64_t elems) {
  const int64_t want = (elems + kMaskThreads - 1) / kMaskThreads;
  return (int)(want < 1 ? 1 : want > kMaskMaxParts ? kMaskMaxParts : want);
}
// rows per column-sum part: kFeatChunk, or what keeps the parts at kMaskMaxParts
int64_t feat_rows_per_part(int64_t n) {
  const int64_t need = (n + kMaskMaxParts - 1) / kMaskMaxParts;
  return need > kFeatChunk ? need : kFeatChunk;
}

}  // namespace

extern "C" {

int gcnx_sddmm_csr(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, int32_t n, int32_t nnz, const float* l, int64_t ldl,
                   const float* r, int64_t ldr, int32_t f, const float* scale, float* out, int accumulate) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "SDDMM on the CSR pattern");
  GCNX_REQUIRE(ctx, n >= 0 && nnz >= 0 && f >= 0, "gcnx_sddmm_csr: negative size");
  if (n == 0 || nnz == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, rowptr && colidx && out && (f == 0 || (l && r)), "gcnx_sddmm_csr: NULL pointer");
  GCNX_REQUIRE(ctx, ldl >= f && ldr >= f, "gcnx_sddmm_csr: ldl and ldr must be >= f");
  GCNX_REQUIRE(ctx, out != l && out != r && out != scale, "gcnx_sddmm_csr: out must not alias an operand");
  SddmmArgs a{};
  a.rowptr = rowptr; a.colidx = colidx; a.n = n; a.f = f; a.l = l; a.ldl = ldl; a.r = r; a.ldr = ldr; a.scale = scale; a.out = out;
  a.accumulate = accumulate ? 1 : 0;
  const bool fast = (f == 16 || f == 32 || f == 64 || f == 128) && gcnx_aligned16(l) && gcnx_aligned16(r) && conv_ld_ok(ldl, f) &&
                    conv_ld_ok(ldr, f) && gcnx_fits_buffer(n, ldr, 4);
  if (fast) {
    const int tiles = gcnx_cdiv(n, kTileRows);
#define GCNX_SDDMM(F_) hipLaunchKernelGGL((sddmm_tile_kernel<F_>), dim3(tiles), dim3(8 * F_), 0, ctx->stream, a)
    if (f == 128) GCNX_SDDMM(128); else if (f == 64) GCNX_SDDMM(64); else if (f == 32) GCNX_SDDMM(32); else GCNX_SDDMM(16);
#undef GCNX_SDDMM
  } else {
    int g = 1;
    while (g < f && g < 64) g <<= 1;
    hipLaunchKernelGGL(sddmm_any_kernel, dim3(gcnx_cdiv(n, 4)), dim3(256), 0, ctx->stream, a, g);
  }
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

int gcnx_edge_mask_fwd(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, int32_t n, int32_t nnz, const float* a_vals,
                       const float* logits, const int32_t* perm_t, float* vals_out, float* vals_t_out) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "edge mask forward");
  GCNX_REQUIRE(ctx, n >= 0 && nnz >= 0, "gcnx_edge_mask_fwd: negative size");
  if (n == 0 || nnz == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, rowptr && colidx && a_vals && logits && vals_out && (perm_t || !vals_t_out), "gcnx_edge_mask_fwd: NULL pointer");
  hipLaunchKernelGGL(edge_mask_fwd_kernel, dim3(gcnx_cdiv(nnz, kMaskThreads)), dim3(kMaskThreads), 0, ctx->stream, rowptr, colidx, n, nnz,
                     a_vals, logits, perm_t, vals_out, vals_t_out);
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

int64_t gcnx_mask_scratch_floats(int64_t n, int32_t f, int per_row) {
  if (n < 0 || f < 0) return 0;
  if (f == 0 || per_row) return 2 * kMaskMaxParts;          // (f == 0: the edge mask)
  const int64_t rpp = feat_rows_per_part(n);
  return ((n + rpp - 1) / rpp) * (int64_t)f + 4;
}

int gcnx_edge_mask_bwd(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, int32_t n, int32_t nnz, const float* a_vals,
                       const float* logits, const float* dv, float c_size, float c_ent, float* dlogits, float* terms, float* scratch) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "edge mask backward");
  GCNX_REQUIRE(ctx, n >= 0 && nnz >= 0, "gcnx_edge_mask_bwd: negative size");
  GCNX_REQUIRE(ctx, terms, "gcnx_edge_mask_bwd: terms is NULL");
  if (n == 0 || nnz == 0) {
    GCNX_HIP(ctx, hipMemsetAsync(terms, 0, 2 * sizeof(float), ctx->stream));
    return GCNX_OK;
  }
  GCNX_REQUIRE(ctx, rowptr && colidx && a_vals && logits && dv && dlogits && scratch, "gcnx_edge_mask_bwd: NULL pointer");
  const int parts = mask_parts(nnz);
  hipLaunchKernelGGL(edge_mask_bwd_kernel, dim3(parts), dim3(kMaskThreads), 0, ctx->stream, rowptr, colidx, n, nnz, a_vals, logits, dv,
                     c_size, c_ent, dlogits, scratch);
  GCNX_LAUNCH_OK(ctx);
  hipLaunchKernelGGL(mask_terms_kernel, dim3(1), dim3(kMaskThreads), 0, ctx->stream, (const float*)scratch, parts, terms);
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

int gcnx_feat_mask_fwd(gcnx_ctx* ctx, const float* x, int64_t ldx, const float* logits, int per_row, int64_t n, int32_t f, float* out,
                       int64_t ldo) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "feature mask forward");
  GCNX_REQUIRE(ctx, n >= 0 && f >= 0, "gcnx_feat_mask_fwd: negative size");
  if (n == 0 || f == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, x && logits && out, "gcnx_feat_mask_fwd: NULL pointer");
  GCNX_REQUIRE(ctx, ldx >= f && ldo >= f, "gcnx_feat_mask_fwd: ldx and ldo must be >= f");
  const int64_t want = (n * f + kMaskThreads - 1) / kMaskThreads;
  hipLaunchKernelGGL(feat_mask_fwd_kernel, dim3((unsigned)(want > 4096 ? 4096 : want)), dim3(kMaskThreads), 0, ctx->stream, x, ldx, logits,
                     per_row ? 1 : 0, n, f, out, ldo);
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

int gcnx_feat_mask_bwd(gcnx_ctx* ctx, const float* dxm, int64_t ldd, const float* x, int64_t ldx, const float* logits, int per_row,
                       int64_t n, int32_t f, float c_size, float c_ent, float* dlogits, float* terms, float* scratch) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "feature mask backward");
  GCNX_REQUIRE(ctx, n >= 0 && f >= 0, "gcnx_feat_mask_bwd: negative size");
  GCNX_REQUIRE(ctx, terms, "gcnx_feat_mask_bwd: terms is NULL");
  if (n == 0 || f == 0) {
    GCNX_HIP(ctx, hipMemsetAsync(terms, 0, 2 * sizeof(float), ctx->stream));
    return GCNX_OK;
  }
  GCNX_REQUIRE(ctx, dxm && x && logits && dlogits && scratch, "gcnx_feat_mask_bwd: NULL pointer");
  GCNX_REQUIRE(ctx, ldd >= f && ldx >= f, "gcnx_feat_mask_bwd: ldd and ldx must be >= f");
  if (per_row) {
    const int parts = mask_parts(n * f);
    hipLaunchKernelGGL(feat_mask_bwd_rows_kernel, dim3(parts), dim3(kMaskThreads), 0, ctx->stream, dxm, ldd, x, ldx, logits, n, f, c_size,
                       c_ent, dlogits, scratch);
    GCNX_LAUNCH_OK(ctx);
    hipLaunchKernelGGL(mask_terms_kernel, dim3(1), dim3(kMaskThreads), 0, ctx->stream, (const float*)scratch, parts, terms);
    GCNX_LAUNCH_OK(ctx);
    return GCNX_OK;
  }
  const int64_t rpp = feat_rows_per_part(n);
  const int parts = (int)((n + rpp - 1) / rpp);
  int fw = 1;
  while (fw < f && fw < kMaskThreads) fw <<= 1;
  hipLaunchKernelGGL(feat_mask_colpart_kernel, dim3(parts), dim3(kMaskThreads), 0, ctx->stream, dxm, ldd, x, ldx, n, f, rpp, fw, scratch);
  GCNX_LAUNCH_OK(ctx);
  hipLaunchKernelGGL(feat_mask_common_kernel, dim3(1), dim3(kMaskThreads), 0, ctx->stream, (const float*)scratch, parts, logits, f, fw,
                     c_size, c_ent, dlogits, terms);
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

}  // extern "C"
