// TopKPool on the device: the one Spektral layer the reference's training script imports that the library could not run
// (`from spektral.layers.pooling import TopKPool`, gcn.py:10), in disjoint mode:
//
//     y = X p / ||p||        k_g = ceil(ratio n_g) rows of every graph g with the largest y        X' = (X * gate(y))[idx]
//     A' = A[idx][:, idx]    (values copied, not renormalised)
//
// Kept rows stay in their original relative order, so old -> new is monotone per graph: A' keeps sorted columns and its
// block-diagonal structure.  Scores compare as IEEE numbers (-0.0 == +0.0); among equal scores the lower row wins.
//
// Launches (none of them uses an atomic: every call leaves the same bits):
//   topk_select_kernel      one workgroup of 1024 threads per graph.  Scores by 16 lanes per row; a 64-bit key per row in LDS
//                           (order-preserving score bits | ~local row), padded to a power of two with key 0, which is below
//                           every real key (a real key's low word is >= 0xFFFFC000); bitonic sort; the k-th largest key is the
//                           threshold.  Keys are distinct, so exactly k rows reach it; they are compacted in row order with
//                           ballots and a running base.  Padding slots only ever exist as LDS keys: nothing indexes x, y, idx
//                           or pos with them.
//   topk_gather_kernel      X'[r] = X[idx[r]] * gate(y[idx[r]])
//   topk_bwd_kernel         128 rows per workgroup over ALL rows by pos: dX (zeros for dropped rows, written here) and the
//                           tile's partial of X^T dy; topk_dp_kernel folds the partials in tile order and projects:
//                           dp = (I - p^ p^T)(X^T dy) / ||p||
//   induce_count_kernel     per kept row the entries whose column survives, scanned inside a block of 256 rows;
//   induce_offsets_kernel   one workgroup scans the block totals (and writes rowptr'[N'] = nnz');
//   induce_fill_kernel      final rowptr', colidx' = pos[col], vals'.
#include "common.h"

namespace {

constexpr int kSelThreads = 1024;
constexpr int kSelMaxRows = 16384;      // 8-byte keys: 128 KiB of the 160 KiB LDS
constexpr int kBwdRows = 128;           // rows per workgroup of topk_bwd_kernel
constexpr int kScanRows = 256;          // rows per workgroup of induce_count_kernel / induce_fill_kernel

__device__ __forceinline__ float gate_of(float y, int sigmoid) { return sigmoid ? 1.0f / (1.0f + expf(-y)) : tanhf(y); }
__device__ __forceinline__ float dgate_of(float g, int sigmoid) { return sigmoid ? g * (1.0f - g) : 1.0f - g * g; }

// sum over the 16 lanes of a row group (xor butterfly: every lane ends with the same bits)
__device__ __forceinline__ float sum16(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// <a[0..f), b[0..f)> by the 16 lanes of a row group, lane `sub`; VEC: f % 4 == 0 and both rows 16-byte aligned
template <bool VEC>
__device__ __forceinline__ float dot16(const float* __restrict__ a, const float* __restrict__ b, int f, int sub) {
  float acc = 0.f;
  if (VEC) {
    for (int c = 4 * sub; c < f; c += 64) {
      const float4 u = *reinterpret_cast<const float4*>(a + c), v = *reinterpret_cast<const float4*>(b + c);
      acc = fmaf(u.x, v.x, acc); acc = fmaf(u.y, v.y, acc); acc = fmaf(u.z, v.z, acc); acc = fmaf(u.w, v.w, acc);
    }
  } else {
    for (int c = sub; c < f; c += 16) acc = fmaf(a[c], b[c], acc);
  }
  return sum16(acc);
}

// 1 / ||p||, the same bits in every workgroup: wave 0 sums p^2 in a fixed order, everyone reads it from *slot.
// (Contains a barrier: call from uniform control flow.)
__device__ __forceinline__ float inv_norm_of(const float* __restrict__ p, int f, float* slot) {
  if (threadIdx.x < 64) {
    float s = 0.f;
    for (int c = threadIdx.x; c < f; c += 64) s = fmaf(p[c], p[c], s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (threadIdx.x == 0) *slot = 1.0f / sqrtf(s);
  }
  __syncthreads();
  return *slot;
}

__device__ __forceinline__ unsigned long long topk_key(float y, int local_row) {
  unsigned u = __float_as_uint(y);
  if ((u << 1) == 0u) u = 0u;                                   // -0.0 compares equal to +0.0
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);               // larger float <=> larger unsigned
  return ((unsigned long long)u << 32) | (unsigned)(~(unsigned)local_row);   // ties: the lower row has the larger key
}

struct SelectArgs {
  const int32_t* graph_ptr; const int32_t* kept_ptr; int32_t cap;   // cap: keys the launch's LDS holds (a power of two)
  const float* x; int64_t ldx; int32_t f; const float* p;
  float* y; int32_t* idx; int32_t* pos;
};

template <bool VEC>
__global__ __launch_bounds__(kSelThreads) void topk_select_kernel(SelectArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long s_key[];
  __shared__ float s_inv;
  __shared__ int s_cnt[kSelThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.x;
  const int r0 = a.graph_ptr[g], ng = a.graph_ptr[g + 1] - r0;
  const int k0 = a.kept_ptr[g];
  const int k = min(max(a.kept_ptr[g + 1] - k0, 0), ng);
  if (ng <= 0 || ng > a.cap) return;                            // (uniform.  ng > cap: refused by the host before the launch)
  const float inv = inv_norm_of(a.p, a.f, &s_inv);
  int m = 2;
  while (m < ng) m <<= 1;
  // ---- scores and keys: 16 lanes per row, 64 rows per pass -------------------------------------------------------------
  const int sub = lane & 15, grp = tid >> 4;
  for (int i0 = 0; i0 < ng; i0 += kSelThreads / 16) {
    const int i = i0 + grp;
    if (i < ng) {
      const float yv = dot16<VEC>(a.x + (int64_t)(r0 + i) * a.ldx, a.p, a.f, sub) * inv;
      if (sub == 0) {
        a.y[r0 + i] = yv;
        s_key[i] = topk_key(yv, i);
      }
    }
  }
  for (int i = ng + tid; i < m; i += kSelThreads) s_key[i] = 0ull;     // padding: below every real key
  __syncthreads();
  // ---- bitonic sort, ascending -----------------------------------------------------------------------------------------
  if (k > 0 && k < ng) {
    for (int kk = 2; kk <= m; kk <<= 1) {
      for (int j = kk >> 1; j > 0; j >>= 1) {
        for (int t = tid; t < (m >> 1); t += kSelThreads) {
          const int lo = 2 * t - (t & (j - 1)), hi = lo + j;
          const unsigned long long u = s_key[lo], v = s_key[hi];
          if ((u > v) == ((lo & kk) == 0)) { s_key[lo] = v; s_key[hi] = u; }
        }
        __syncthreads();
      }
    }
  }
  // k-th largest key (k == ng: every row; k == 0: none -- no key reaches ~0)
  const unsigned long long thr = k <= 0 ? ~0ull : (k >= ng ? 0ull : s_key[m - k]);
  // ---- survivors in row order ------------------------------------------------------------------------------------------
  int base = 0;
  for (int i0 = 0; i0 < ng; i0 += kSelThreads) {
    const int i = i0 + tid;
    const bool keep = i < ng && topk_key(a.y[r0 + min(i, ng - 1)], i) >= thr;
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) s_cnt[wave] = __popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kSelThreads / 64; ++w) {
      const int c = s_cnt[w];
      before += w < wave ? c : 0;
      total += c;
    }
    const int rank = base + before + __popcll(bal & ((1ull << lane) - 1ull));
    if (i < ng) {
      const bool put = keep && rank < k;
      a.pos[r0 + i] = put ? k0 + rank : -1;
      if (put) a.idx[k0 + rank] = r0 + i;
    }
    base += total;
    __syncthreads();                                            // s_cnt is rewritten by the next chunk
  }
}

struct GatherArgs {
  const float* x; int64_t ldx; const float* y; const int32_t* idx; int32_t nk; int32_t f; int sigmoid;
  float* out; int64_t ldo;
};

template <bool VEC>
__global__ __launch_bounds__(256) void topk_gather_kernel(GatherArgs a) {
  const int sub = threadIdx.x & 15;
  const int64_t r = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (r >= a.nk) return;
  const int i = a.idx[r];
  const float gt = gate_of(a.y[i], a.sigmoid);
  const float* __restrict__ src = a.x + (int64_t)i * a.ldx;
  float* __restrict__ dst = a.out + r * a.ldo;
  if (VEC) {
    for (int c = 4 * sub; c < a.f; c += 64) {
      float4 v = *reinterpret_cast<const float4*>(src + c);
      v.x *= gt; v.y *= gt; v.z *= gt; v.w *= gt;
      *reinterpret_cast<float4*>(dst + c) = v;
    }
  } else {
    for (int c = sub; c < a.f; c += 16) dst[c] = src[c] * gt;
  }
}

struct BwdArgs {
  const float* x; int64_t ldx; const float* y; const int32_t* pos; const float* p; int32_t n; int32_t f; int sigmoid;
  const float* dxo; int64_t lddxo;        // dX' [N', f]
  float* dx; int64_t lddx;                // [n, f]: every row written
  float* part;                            // [tiles][f]: the tile's rows of X^T dy
};

template <bool VEC>
__global__ __launch_bounds__(256) void topk_bwd_kernel(BwdArgs a) {
  __shared__ float s_inv;
  __shared__ float s_dy[kBwdRows];
  __shared__ float s_red[4][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sub = tid & 15, grp = tid >> 4;
  const int64_t t0 = (int64_t)blockIdx.x * kBwdRows;
  const float inv = inv_norm_of(a.p, a.f, &s_inv);
  // ---- dX, 16 lanes per row, 16 rows per pass ---------------------------------------------------------------------------
  for (int j0 = 0; j0 < kBwdRows; j0 += 16) {
    const int j = j0 + grp;
    const int64_t i = t0 + j;
    float dy = 0.f;
    if (i < a.n) {
      const int r = a.pos[i];
      float* __restrict__ dst = a.dx + i * a.lddx;
      if (r < 0) {
        if (VEC) for (int c = 4 * sub; c < a.f; c += 64) *reinterpret_cast<float4*>(dst + c) = make_float4(0.f, 0.f, 0.f, 0.f);
        else for (int c = sub; c < a.f; c += 16) dst[c] = 0.f;
      } else {
        const float* __restrict__ xi = a.x + i * a.ldx;
        const float* __restrict__ dr = a.dxo + (int64_t)r * a.lddxo;
        const float gt = gate_of(a.y[i], a.sigmoid);
        dy = dgate_of(gt, a.sigmoid) * dot16<VEC>(dr, xi, a.f, sub);
        const float s = dy * inv;                               // dy p^ = (dy / ||p||) p
        if (VEC) {
          for (int c = 4 * sub; c < a.f; c += 64) {
            const float4 d = *reinterpret_cast<const float4*>(dr + c), pv = *reinterpret_cast<const float4*>(a.p + c);
            *reinterpret_cast<float4*>(dst + c) = make_float4(fmaf(gt, d.x, s * pv.x), fmaf(gt, d.y, s * pv.y),
                                                              fmaf(gt, d.z, s * pv.z), fmaf(gt, d.w, s * pv.w));
          }
        } else {
          for (int c = sub; c < a.f; c += 16) dst[c] = fmaf(gt, dr[c], s * a.p[c]);
        }
      }
    }
    if (sub == 0) s_dy[j] = dy;                                 // rows past the end and dropped rows: 0
  }
  __syncthreads();
  // ---- the tile's part of X^T dy: wave w adds rows w, w + 4, ... of a column in ascending order, wave 0 folds the four ----
  const int nr = (int)min((int64_t)kBwdRows, a.n - t0);
  for (int c0 = 0; c0 < a.f; c0 += 64) {
    const int c = c0 + lane;
    float acc = 0.f;
    if (c < a.f)
      for (int j = wave; j < nr; j += 4) acc = fmaf(a.x[(t0 + j) * a.ldx + c], s_dy[j], acc);
    s_red[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && c < a.f) a.part[(int64_t)blockIdx.x * a.f + c] = ((s_red[0][lane] + s_red[1][lane]) + s_red[2][lane]) + s_red[3][lane];
    __syncthreads();
  }
}

// dp = (I - p^ p^T) v / ||p||, v = the column sums of the tiles' parts in tile order.  One workgroup; dp holds v in between.
__global__ __launch_bounds__(256) void topk_dp_kernel(const float* __restrict__ part, int32_t tiles, const float* __restrict__ p, int32_t f,
                                                      float* __restrict__ dp) {
  __shared__ float s_inv;
  __shared__ float s_sum[256];
  const int tid = threadIdx.x;
  const float inv = inv_norm_of(p, f, &s_inv);
  float pv = 0.f;
  for (int c = tid; c < f; c += 256) {
    float v = 0.f;
    for (int t = 0; t < tiles; ++t) v += part[(int64_t)t * f + c];
    dp[c] = v;
    pv = fmaf(p[c], v, pv);
  }
  s_sum[tid] = pv;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) s_sum[tid] += s_sum[tid + o];
    __syncthreads();
  }
  const float proj = s_sum[0] * inv * inv;                      // <p^, v> / ||p||
  for (int c = tid; c < f; c += 256) dp[c] = (dp[c] - proj * p[c]) * inv;   // (each thread reads back its own stores)
}

// ---- the induced sub-CSR -------------------------------------------------------------------------------------------------
// exclusive prefix of v over the 256 threads of a workgroup; *total = the workgroup's sum
__device__ __forceinline__ int scan256(int v, int* s_w, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  int before = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int c = s_w[w];
    before += w < wave ? c : 0;
    tot += c;
  }
  __syncthreads();                                              // s_w may be rewritten by the caller's next round
  *total = tot;
  return before + inc - v;
}

__global__ __launch_bounds__(kScanRows) void induce_count_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                                                 const int32_t* __restrict__ idx, const int32_t* __restrict__ pos,
                                                                 int32_t nk, int32_t* __restrict__ rowptr_out, int32_t* __restrict__ block_tot) {
  __shared__ int s_w[4];
  const int64_t r = (int64_t)blockIdx.x * kScanRows + threadIdx.x;
  int cnt = 0;
  if (r < nk) {
    const int i = idx[r];
    for (int e = rowptr[i], e1 = rowptr[i + 1]; e < e1; ++e) cnt += pos[colidx[e]] >= 0 ? 1 : 0;
  }
  int total;
  const int ex = scan256(cnt, s_w, &total);
  if (r < nk) rowptr_out[r] = ex;                               // relative to the block: induce_fill_kernel adds the block's offset
  if (threadIdx.x == 0) block_tot[blockIdx.x] = total;
}

// block_tot[nb] -> exclusive offsets in place; rowptr_out[nk] = the grand total (nnz').  One workgroup.
__global__ __launch_bounds__(256) void induce_offsets_kernel(int32_t* __restrict__ block_tot, int32_t nb, int32_t* __restrict__ rowptr_end) {
  __shared__ int s_w[4];
  int base = 0;
  for (int b0 = 0; b0 < nb; b0 += 256) {
    const int b = b0 + threadIdx.x;
    const int v = b < nb ? block_tot[b] : 0;
    int total;
    const int ex = scan256(v, s_w, &total);
    if (b < nb) block_tot[b] = base + ex;
    base += total;
  }
  if (threadIdx.x == 0) *rowptr_end = base;
}

__global__ __launch_bounds__(kScanRows) void induce_fill_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                                                const float* __restrict__ vals, const int32_t* __restrict__ idx,
                                                                const int32_t* __restrict__ pos, int32_t nk, const int32_t* __restrict__ block_off,
                                                                int32_t* __restrict__ rowptr_out, int32_t* __restrict__ colidx_out,
                                                                float* __restrict__ vals_out) {
  const int64_t r = (int64_t)blockIdx.x * kScanRows + threadIdx.x;
  if (r >= nk) return;
  int o = rowptr_out[r] + block_off[blockIdx.x];
  rowptr_out[r] = o;
  const int i = idx[r];
  for (int e = rowptr[i], e1 = rowptr[i + 1]; e < e1; ++e) {
    const int c = pos[colidx[e]];
    if (c >= 0) {
      colidx_out[o] = c;
      if (vals_out) vals_out[o] = vals[e];
      ++o;
    }
  }
}

bool select_shape_ok(int64_t max_graph_rows, int32_t f) { return max_graph_rows >= 0 && max_graph_rows <= kSelMaxRows && f > 0; }

bool rows_vec_ok(int32_t f, const void* a, int64_t lda, const void* b, int64_t ldb) {
  return f % 4 == 0 && gcnx_aligned16(a) && gcnx_aligned16(b) && lda % 4 == 0 && ldb % 4 == 0;
}

}  // namespace

extern "C" {

int gcnx_topk_select_ok(int64_t max_graph_rows, int32_t f) { return select_shape_ok(max_graph_rows, f) ? 1 : 0; }

int gcnx_topk_select(gcnx_ctx* ctx, const int32_t* graph_ptr, const int32_t* kept_ptr, int32_t b, int32_t max_graph_rows,
                     const float* x, int64_t ldx, int32_t f, const float* p, float* y, int32_t* idx, int32_t* pos) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "TopKPool select");
  GCNX_REQUIRE(ctx, b >= 0 && max_graph_rows >= 0, "gcnx_topk_select: negative size");
  if (!select_shape_ok(max_graph_rows, f))
    return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_topk_select: serves graphs of up to %d rows and f > 0 (got max_graph_rows=%d f=%d)",
                     kSelMaxRows, max_graph_rows, f);
  if (b == 0 || max_graph_rows == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, graph_ptr && kept_ptr && x && p && y && idx && pos, "gcnx_topk_select: NULL pointer");
  GCNX_REQUIRE(ctx, ldx >= f, "gcnx_topk_select: ldx < f");
  int cap = 64;
  while (cap < max_graph_rows) cap <<= 1;
  SelectArgs a{graph_ptr, kept_ptr, cap, x, ldx, f, p, y, idx, pos};
  const int lds = cap * (int)sizeof(unsigned long long);
  static bool limit_raised = false;       // the dynamic-LDS limit of both instantiations, once, at the largest size served
  if (!limit_raised) {
    constexpr int kMaxLds = kSelMaxRows * (int)sizeof(unsigned long long);
    GCNX_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(topk_select_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds));
    GCNX_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(topk_select_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds));
    limit_raised = true;
  }
  if (rows_vec_ok(f, x, ldx, p, 4)) hipLaunchKernelGGL(topk_select_kernel<true>, dim3(b), dim3(kSelThreads), lds, ctx->stream, a);
  else hipLaunchKernelGGL(topk_select_kernel<false>, dim3(b), dim3(kSelThreads), lds, ctx->stream, a);
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

int gcnx_topk_gather(gcnx_ctx* ctx, const float* x, int64_t ldx, const float* y, const int32_t* idx, int32_t n_kept, int32_t f,
                     int sigmoid_gating, float* out, int64_t ldo) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "TopKPool gather");
  GCNX_REQUIRE(ctx, n_kept >= 0 && f > 0, "gcnx_topk_gather: bad size");
  if (n_kept == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, x && y && idx && out, "gcnx_topk_gather: NULL pointer");
  GCNX_REQUIRE(ctx, ldx >= f && ldo >= f && x != out, "gcnx_topk_gather: ldx, ldo >= f and out must not alias x");
  GatherArgs a{x, ldx, y, idx, n_kept, f, sigmoid_gating ? 1 : 0, out, ldo};
  const dim3 grid(gcnx_cdiv(n_kept, 16));
  if (rows_vec_ok(f, x, ldx, out, ldo)) hipLaunchKernelGGL(topk_gather_kernel<true>, grid, dim3(256), 0, ctx->stream, a);
  else hipLaunchKernelGGL(topk_gather_kernel<false>, grid, dim3(256), 0, ctx->stream, a);
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

int gcnx_topk_bwd(gcnx_ctx* ctx, const float* x, int64_t ldx, const float* y, const int32_t* pos, const float* p, int32_t n,
                  int32_t f, int sigmoid_gating, const float* dxo, int64_t lddxo, float* dx, int64_t lddx, float* dp) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "TopKPool backward");
  GCNX_REQUIRE(ctx, n >= 0 && f > 0, "gcnx_topk_bwd: bad size");
  GCNX_REQUIRE(ctx, p && dp, "gcnx_topk_bwd: NULL pointer");
  const int tiles = gcnx_cdiv(n, kBwdRows);
  if (tiles > 0) {
    GCNX_REQUIRE(ctx, x && y && pos && dxo && dx, "gcnx_topk_bwd: NULL pointer");
    GCNX_REQUIRE(ctx, ldx >= f && lddxo >= f && lddx >= f && dx != x && dx != dxo, "gcnx_topk_bwd: leading dimensions >= f, dx must not alias x or dxo");
    int rc = gcnx_ws_reserve(ctx, (size_t)tiles * f * sizeof(float));
    if (rc) return rc;
    BwdArgs a{x, ldx, y, pos, p, n, f, sigmoid_gating ? 1 : 0, dxo, lddxo, dx, lddx, (float*)ctx->ws};
    if (rows_vec_ok(f, x, ldx, dxo, lddxo) && rows_vec_ok(f, dx, lddx, p, 4))
      hipLaunchKernelGGL(topk_bwd_kernel<true>, dim3(tiles), dim3(256), 0, ctx->stream, a);
    else
      hipLaunchKernelGGL(topk_bwd_kernel<false>, dim3(tiles), dim3(256), 0, ctx->stream, a);
    GCNX_LAUNCH_OK(ctx);
  }
  hipLaunchKernelGGL(topk_dp_kernel, dim3(1), dim3(256), 0, ctx->stream, (const float*)ctx->ws, tiles, p, f, dp);
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

int gcnx_csr_induce(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* vals, const int32_t* idx,
                    const int32_t* pos, int32_t n_kept, int32_t* rowptr_out, int32_t* colidx_out, float* vals_out) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "induced sub-CSR");
  GCNX_REQUIRE(ctx, n_kept >= 0, "gcnx_csr_induce: negative size");
  GCNX_REQUIRE(ctx, rowptr_out, "gcnx_csr_induce: NULL pointer");
  GCNX_REQUIRE(ctx, (vals == nullptr) == (vals_out == nullptr), "gcnx_csr_induce: vals and vals_out are both given or both NULL");
  const int nb = gcnx_cdiv(n_kept, kScanRows);
  if (nb == 0) {
    GCNX_HIP(ctx, hipMemsetAsync(rowptr_out, 0, sizeof(int32_t), ctx->stream));
    return GCNX_OK;
  }
  GCNX_REQUIRE(ctx, rowptr && colidx && idx && pos && colidx_out, "gcnx_csr_induce: NULL pointer");
  int rc = gcnx_ws_reserve(ctx, (size_t)nb * sizeof(int32_t));
  if (rc) return rc;
  int32_t* block_tot = (int32_t*)ctx->ws;
  hipLaunchKernelGGL(induce_count_kernel, dim3(nb), dim3(kScanRows), 0, ctx->stream, rowptr, colidx, idx, pos, n_kept, rowptr_out, block_tot);
  GCNX_LAUNCH_OK(ctx);
  hipLaunchKernelGGL(induce_offsets_kernel, dim3(1), dim3(256), 0, ctx->stream, block_tot, nb, rowptr_out + n_kept);
  GCNX_LAUNCH_OK(ctx);
  hipLaunchKernelGGL(induce_fill_kernel, dim3(nb), dim3(kScanRows), 0, ctx->stream, rowptr, colidx, vals, idx, pos, n_kept,
                     (const int32_t*)block_tot, rowptr_out, colidx_out, vals_out);
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

}  // extern "C"
