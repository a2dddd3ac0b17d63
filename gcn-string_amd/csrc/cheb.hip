// Chebyshev spectral convolution (PyG's ChebConv(in, out, K, normalization="sym", lambda_max); Spektral's ChebConv(channels, K)
// with K one less): the K-hop layer with one weight matrix per hop distance, for the slot the reference's author left open
// (gcn_utills.py:804-806).  On the operator S of gcnx_cheb_norm, with c_s = -2 / lambda_max and c_d = 2 / lambda_max - 1 rounded
// once to fp32 on the host:
//
//     L^ z = c_s (S z) + c_d z        T_0 z = z      T_1 z = L^ z      T_j z = 2 L^ T_{j-1} z - T_{j-2} z
//
//     basis:  out block j = T_j(L^) x, j = 0 .. k-1                                           (k - 1 gathers)
//     sum:    out = sum_j T_j(L^) H_j + bias, by Clenshaw: b_k = b_{k+1} = 0, b_j = H_j + 2 L^ b_{j+1} - b_{j+2} (j = k-1 .. 1),
//             out = H_0 + L^ b_1 - b_2 + bias                                                 (k - 1 gathers: b_{k-1} = H_{k-1})
//
// One expression per element and step, on both routes: acc = +0, acc = fmaf(vals[e], cur[colidx[e]], acc) entry by entry in
// CSR order, then fmaf(a, acc, fmaf(b, cur[i], d)) with
//     basis step j:  (a, b) = (c_s, c_d) at j = 1, else (2 c_s, 2 c_d);  cur = T_{j-1}, d = -T_{j-2}[i]  (-0 at j = 1)
//     sum step j:    (a, b) = (c_s, c_d) at j = 0, else (2 c_s, 2 c_d);  cur = b_{j+1}, d = H_j[i] - b_{j+2}[i]  (b_k = +0);
//                    step 0 adds bias[col] to the result (no bias: nothing is added)
// Both routes and every column block evaluate exactly that, so they leave the same bits, and which graphs share a batch never
// changes a result.
//
// Resident route (one launch): the workgroup of appnp.hip -- one per (graph, block of cb columns), the graph's row pointers and
// CSR entries staged in LDS, cb / 4 lanes per row -- with the three-term recurrence in TWO buffers of cap x cb floats: the new
// term overwrites the term two steps back, an element that only the lane that owns it reads or writes; gathers read the other
// buffer only; one barrier per step.  basis stores every step's slice to its block of out (16-byte stores); sum loads H_j's
// slice from global memory: the first four rows of a lane group one step ahead (issued before the step they are for, so a whole
// step of gathers hides them), the rows of a taller graph ahead of the row's gather.  Every entry is range-checked when it is
// staged or read, so no LDS address is ever out of range.
//
// Streamed route (k - 1 launches of a one-hop gather with the same epilogue over the whole batch): basis keeps its terms in the
// blocks of out; sum alternates between out and the caller's scratch so that step 0 lands in out, each step overwriting b_{j+2}
// in place (again the owning thread's element only).
//
// No atomics, no host read-back, nothing allocated: capture-safe (gcnx_cheb_norm excepted: it uses the context's workspace).
#include "common.h"
#include "conv_tile.h"
#include "resident_hops.h"

namespace {

constexpr int kChebXR = 4;                   // rows per lane group whose H_j slice is loaded one step ahead
constexpr int kChebMaxK = 16;
// Gathers (k - 1) from which the library's choice is the resident route: APPNP's rule (appnp.hip; DESIGN 4.24 has the readings)
constexpr int kChebMinHops = 3, kChebMinHopsSmall = 2, kChebSmallRows = 256;

// fmaf(a, acc, fmaf(b, cur, d)) with d = inj - prev (SUM) or -prev: the step of both routes
template <bool SUM>
__device__ __forceinline__ float cheb_step1(float a, float acc, float b, float cur, float inj, float prev) {
  return fmaf(a, acc, fmaf(b, cur, SUM ? inj - prev : -prev));
}
template <bool SUM>
__device__ __forceinline__ float4 cheb_step4(float a, float4 acc, float b, float4 cur, float4 inj, float4 prev) {
  return make_float4(cheb_step1<SUM>(a, acc.x, b, cur.x, inj.x, prev.x), cheb_step1<SUM>(a, acc.y, b, cur.y, inj.y, prev.y),
                     cheb_step1<SUM>(a, acc.z, b, cur.z, inj.z, prev.z), cheb_step1<SUM>(a, acc.w, b, cur.w, inj.w, prev.w));
}

struct ResArgs {
  const int32_t* rowptr; const int32_t* colidx; const float* vals;
  const int32_t* graph_ptr;
  int32_t cap;                 // rows of the tallest graph served (max_graph_rows): the LDS layout
  int32_t cb, ncb;             // columns per block, blocks per graph
  int32_t ent_cap;             // CSR entries staged
  const float* in; int64_t ldi;    // basis: x [n, f]; sum: h [n, k f]
  const float* bias;               // sum: [f] or NULL
  int32_t f, k;
  float cs, cd;
  float* out; int64_t ldo;         // basis: [n, k f]; sum: [n, f]
};

// LDS: z0 [cap, cb] | z1 [cap, cb] | s_rp [cap + 1, padded to 4] | s_val [ent_cap] (WEIGHTED only) | s_col [ent_cap] uint16
template <bool WEIGHTED, bool SUM>
__global__ __launch_bounds__(kResThreads) void cheb_resident_kernel(ResArgs p) {
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  const int tid = threadIdx.x, nthr = blockDim.x;           // 256 .. 1024 threads: what the tallest graph's rows fill
  const int id = gcnx_xcd_remap(blockIdx.x, gridDim.x);      // a graph's column blocks are neighbours: they share an L2
  const int g = id / p.ncb, jb = id - g * p.ncb;
  const int r0 = p.graph_ptr[g], ng = p.graph_ptr[g + 1] - r0;
  if (ng <= 0 || ng > p.cap) return;                         // (the whole workgroup: no barrier is left waiting)
  const int cb = p.cb, lpr = cb >> 2;
  float* z0 = s_mem;
  float* z1 = z0 + (size_t)p.cap * cb;
  int32_t* s_rp = reinterpret_cast<int32_t*>(z1 + (size_t)p.cap * cb);
  float* s_val = reinterpret_cast<float*>(s_rp + ((p.cap + 1 + 3) & ~3));
  uint16_t* s_col = reinterpret_cast<uint16_t*>(s_val + (WEIGHTED ? p.ent_cap : 0));

  const int e0 = p.rowptr[r0], e1 = p.rowptr[r0 + ng];
  const int staged = min(max(e1 - e0, 0), p.ent_cap);
  for (int i = tid; i <= ng; i += nthr) s_rp[i] = p.rowptr[r0 + i] - e0;
  for (int i = tid; i < staged; i += nthr) {
    const int c = p.colidx[e0 + i] - r0;                     // (cap < 0xFFFF: a column inside the graph is never the marker)
    s_col[i] = (unsigned)c < (unsigned)ng ? (uint16_t)c : (uint16_t)0xFFFF;
    if (WEIGHTED) s_val[i] = p.vals[e0 + i];
  }
  // the static element-to-thread map of every pass below: lane group rg walks rows rg, rg + ngrp, ...
  const int ngrp = nthr / lpr;
  const int rg = tid / lpr, sub = tid - rg * lpr;
  const int col = jb * cb + 4 * sub;
  const bool active = rg < ngrp && col < p.f;
  const int nstep = p.k - 1;                                 // >= 1: k == 1 never comes here
  // the start term into z0: x (basis; it is block 0 of out as well) or H_{k-1} (sum)
  const float* icol = p.in + (int64_t)r0 * p.ldi + col;      // this lane's columns of block 0 of `in`
  float* ocol = p.out + (int64_t)r0 * p.ldo + col;
  if (active)
    for (int r = rg; r < ng; r += ngrp) {
      const float4 v = load4(icol + (int64_t)r * p.ldi + (SUM ? (int64_t)nstep * p.f : 0));
      *reinterpret_cast<float4*>(z0 + r * cb + 4 * sub) = v;
      if (!SUM) *reinterpret_cast<float4*>(ocol + (int64_t)r * p.ldo) = v;
    }
  // sum: H_j of the first kChebXR rows of this lane group for the first step, in registers; every step loads the next one's
  float4 hn[kChebXR];
#pragma unroll
  for (int q = 0; q < kChebXR; ++q) {
    const int r = rg + q * ngrp;
    hn[q] = zero4();
    if (SUM && active && r < ng) hn[q] = load4(icol + (int64_t)r * p.ldi + (int64_t)(nstep - 1) * p.f);
  }
  float4 bias = zero4();
  if (SUM && p.bias && active) bias = make_float4(p.bias[col], p.bias[col + 1], p.bias[col + 2], p.bias[col + 3]);
  __syncthreads();

  const int rowb = cb * 4, sub16 = sub * 16;                 // bytes per row of the slice, this lane's offset in it
  const int32_t* gcol = p.colidx + e0;
  const float* gval = WEIGHTED ? p.vals + e0 : nullptr;
  for (int s = 1; s <= nstep; ++s) {
    float* curf = (s & 1) ? z0 : z1;
    float* nxt = (s & 1) ? z1 : z0;
    const char* cur = reinterpret_cast<const char*>(curf);
    const bool first = s == 1, last = s == nstep;
    const bool single = SUM ? last : first;                  // the step that applies L^ once: T_1, and the sum's step 0
    const float a = single ? p.cs : 2.0f * p.cs, b = single ? p.cd : 2.0f * p.cd;
    const int64_t blk = (int64_t)(SUM ? nstep - s : s) * p.f;        // sum: H_j read, j = k-1-s; basis: block s of out written
    float4 hc[kChebXR];
#pragma unroll
    for (int q = 0; q < kChebXR; ++q) {
      const int r = rg + q * ngrp;
      hc[q] = hn[q];
      if (SUM && !last && active && r < ng) hn[q] = load4(icol + (int64_t)r * p.ldi + blk - p.f);
    }
    auto row = [&](int r, float4 inj) {
      const int ea = s_rp[r], eb = s_rp[r + 1];
      float4 acc = res_row_staged<WEIGHTED>(s_col, s_val, cur, rowb, sub16, min(ea, staged), min(eb, staged), zero4());
      if (eb > staged) acc = res_row_global<WEIGHTED>(gcol, gval, r0, ng, cur, rowb, sub16, max(ea, staged), eb, acc);
      const float4 own = *reinterpret_cast<const float4*>(curf + r * cb + 4 * sub);
      const float4 prev = first ? zero4() : *reinterpret_cast<const float4*>(nxt + r * cb + 4 * sub);
      const float4 res = cheb_step4<SUM>(a, acc, b, own, inj, prev);
      if (SUM && last) {
        *reinterpret_cast<float4*>(ocol + (int64_t)r * p.ldo) = p.bias ? add4(res, bias) : res;
        return;
      }
      if (!SUM) *reinterpret_cast<float4*>(ocol + (int64_t)r * p.ldo + blk) = res;
      if (!last) *reinterpret_cast<float4*>(nxt + r * cb + 4 * sub) = res;
    };
    if (active) {
#pragma unroll
      for (int q = 0; q < kChebXR; ++q)
        if (rg + q * ngrp < ng) row(rg + q * ngrp, hc[q]);
      for (int r = rg + kChebXR * ngrp; r < ng; r += ngrp) row(r, SUM ? load4(icol + (int64_t)r * p.ldi + blk) : zero4());
    }
    if (!last) __syncthreads();
  }
}

struct HopArgs {
  const int32_t* rowptr; const int32_t* colidx; const float* vals;
  const float* z; int64_t ldz;          // the term gathered (cur)
  const float* prev; int64_t ldp;       // the term two steps back (NULL: +0); may be the very elements out overwrites
  const float* inj; int64_t ldi;        // sum: H_j
  const float* bias;                    // sum's step 0, or NULL
  float* echo; int64_t lde;             // basis step 1: z's own element goes here too (block 0 of out), or NULL
  int32_t n, f;
  float a, b;
  float* out; int64_t ldo;
};

// one step over the whole batch: VEC: f / 4 threads per row (float4 each); otherwise a thread per element
template <bool VEC, bool WEIGHTED, bool SUM>
__global__ __launch_bounds__(kHopThreads) void cheb_hop_kernel(HopArgs p) {
  const int lpr = VEC ? p.f >> 2 : p.f;
  const int64_t idx = (int64_t)blockIdx.x * kHopThreads + threadIdx.x;
  const int64_t row = idx / lpr;
  if (row >= p.n) return;
  const int col = (int)(idx - row * lpr) * (VEC ? 4 : 1);
  const int ea = p.rowptr[row], eb = p.rowptr[row + 1];
  const float* zc = p.z + col;
  if constexpr (VEC) {
    const float4 own = load4(zc + row * p.ldz);
    const float4 inj = SUM ? load4(p.inj + row * p.ldi + col) : zero4();
    const float4 prev = p.prev ? load4(p.prev + row * p.ldp + col) : zero4();
    const float4 acc = hop_row4<WEIGHTED>(p.colidx, p.vals, zc, p.ldz, p.n, row, ea, eb);
    float4 res = cheb_step4<SUM>(p.a, acc, p.b, own, inj, prev);
    if (SUM && p.bias) res = add4(res, make_float4(p.bias[col], p.bias[col + 1], p.bias[col + 2], p.bias[col + 3]));
    *reinterpret_cast<float4*>(p.out + row * p.ldo + col) = res;
    if (!SUM && p.echo) *reinterpret_cast<float4*>(p.echo + row * p.lde + col) = own;
  } else {
    const float own = zc[row * p.ldz];
    const float inj = SUM ? p.inj[row * p.ldi + col] : 0.f;
    const float prev = p.prev ? p.prev[row * p.ldp + col] : 0.f;
    const float acc = hop_row1<WEIGHTED>(p.colidx, p.vals, zc, p.ldz, p.n, ea, eb);
    float res = cheb_step1<SUM>(p.a, acc, p.b, own, inj, prev);
    if (SUM && p.bias) res = res + p.bias[col];
    p.out[row * p.ldo + col] = res;
    if (!SUM && p.echo) p.echo[row * p.lde + col] = own;
  }
}

// k == 1: out = x (basis) or h + bias (sum), element by element (any f, leading dimensions and alignment)
__global__ __launch_bounds__(kHopThreads) void cheb_copy_kernel(const float* __restrict__ x, int64_t ldx, int32_t n, int32_t f,
                                                                const float* __restrict__ bias, float* __restrict__ out, int64_t ldo) {
  const int64_t idx = (int64_t)blockIdx.x * kHopThreads + threadIdx.x;
  const int64_t row = idx / f;
  if (row >= n) return;
  const int col = (int)(idx - row * f);
  const float v = x[row * ldx + col];
  out[row * ldo + col] = bias ? v + bias[col] : v;
}

// r[j] = deg_j^-1/2 of column j of the operator = row j of its transposed CSR, the diagonal left out (0 where deg_j <= 0)
__global__ __launch_bounds__(256) void cheb_degree_kernel(const int32_t* __restrict__ rowptr_t, const int32_t* __restrict__ colidx_t,
                                                          const float* __restrict__ vals_t, int32_t n, float* __restrict__ r) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  double d = 0.0;
  for (int e = rowptr_t[j]; e < rowptr_t[j + 1]; ++e)
    if (colidx_t[e] != j) d += vals_t ? (double)vals_t[e] : 1.0;
  r[j] = d > 0.0 ? (float)(1.0 / sqrt(d)) : 0.f;
}
// S on the stored pattern: (r_i w_ij) r_j off the diagonal, +0 on it (and on an entry whose column lies outside [0, n))
__global__ __launch_bounds__(256) void cheb_scale_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                                         const float* vals, int32_t n, const float* __restrict__ r, float* out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float ri = r[i];
  for (int e = rowptr[i]; e < rowptr[i + 1]; ++e) {
    const int j = colidx[e];
    out[e] = j == i || (unsigned)j >= (unsigned)n ? 0.f : ri * (vals ? vals[e] : 1.0f) * r[j];
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
// What basis and sum share.  in: x [n, f] (basis) or h [n, k f] (sum); out: [n, k f] (basis) or [n, f] (sum).
template <bool SUM>
int cheb_run(gcnx_ctx* ctx, const char* who, const int32_t* rowptr, const int32_t* colidx, const float* vals, const int32_t* graph_ptr,
             int32_t b, int32_t max_graph_rows, const float* in, int64_t ldi, const float* bias, int32_t n, int32_t f, int32_t k,
             float lambda_max, int32_t col_block, float* out, int64_t ldo, float* scratch) {
  GCNX_REQUIRE(ctx, n >= 0 && f >= 0 && b >= 0 && max_graph_rows >= 0, "%s: negative size", who);
  GCNX_REQUIRE(ctx, k >= 1 && k <= kChebMaxK, "%s: k = %d must be in 1 .. %d", who, k, kChebMaxK);
  GCNX_REQUIRE(ctx, lambda_max > 0.f && lambda_max <= 3.0e38f, "%s: lambda_max = %g must be a finite number > 0", who, (double)lambda_max);
  GCNX_REQUIRE(ctx, col_block >= -1, "%s: col_block = %d (0: the library's choice, > 0: resident, -1: streamed)", who, col_block);
  const int64_t wi = SUM ? (int64_t)k * f : f, wo = SUM ? f : (int64_t)k * f;       // widths of in and out
  GCNX_REQUIRE(ctx, ldi >= wi && ldo >= wo, "%s: a leading dimension is below its operand's width", who);
  GCNX_REQUIRE(ctx, wi <= INT32_MAX && wo <= INT32_MAX, "%s: k * f overflows", who);
  const int64_t si = span(n, ldi, (int32_t)wi), so = span(n, ldo, (int32_t)wo);
  const int64_t nscr = SUM && k >= 3 && n > 0 && f > 0 ? (int64_t)n * f : 0;          // what the streamed sum writes
  GCNX_REQUIRE(ctx, !overlap(out, so, in, si), "%s: out overlaps its input", who);
  GCNX_REQUIRE(ctx, !overlap(out, so, scratch, nscr) && !overlap(in, si, scratch, nscr), "%s: scratch overlaps out or the input", who);
  GCNX_REQUIRE(ctx, !overlap(out, so, bias, SUM ? f : 0), "%s: out overlaps bias", who);
  static size_t lds_max = 0;               // (res_lds_max, read once)
  if (lds_max == 0 && res_lds_max(ctx, &lds_max) != GCNX_OK) return GCNX_ERR_HIP;
  const bool vec = f % 4 == 0 && ldi % 4 == 0 && ldo % 4 == 0 && gcnx_aligned16(in) && gcnx_aligned16(out);
  const bool res_ok = graph_ptr && vec && res_shape_ok(max_graph_rows, f, ldi);
  int cb = 0;
  if (col_block > 0) {
    if (!res_ok || col_block % 4 != 0 || col_block > f || !res_fits(max_graph_rows, col_block))
      return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "%s: col_block = %d is not served: the resident route needs graph_ptr, "
                       "max_graph_rows > 0, f, the leading dimensions and col_block in multiples of 4 floats, col_block <= f, 16-byte "
                       "aligned operands, and 2 * max_graph_rows * col_block * 4 bytes + the row pointers within %d bytes of LDS (got "
                       "max_graph_rows=%d f=%d k=%d)", who, col_block, kResLdsMax, max_graph_rows, f, k);
    cb = col_block;
  } else if (col_block == 0 && res_ok && k - 1 >= (max_graph_rows <= kChebSmallRows ? kChebMinHopsSmall : kChebMinHops)) {
    cb = res_choose_cb(ctx, max_graph_rows, f, b, vals != nullptr, lds_max);
  }
  if (n == 0 || f == 0 || (graph_ptr && b == 0)) return GCNX_OK;
  GCNX_REQUIRE(ctx, rowptr && colidx && in && out, "%s: NULL pointer", who);
  GCNX_REQUIRE(ctx, cb > 0 || nscr == 0 || scratch, "%s: the streamed route with k >= 3 needs scratch (gcnx_cheb_scratch_floats)", who);
  GCNX_REQUIRE(ctx, (int64_t)n * k * f < (1ll << 38), "%s: n * k * f = %lld elements are not served", who, (long long)n * k * f);

  if (k == 1) {
    hipLaunchKernelGGL(cheb_copy_kernel, dim3(gcnx_cdiv((int64_t)n * f, kHopThreads)), dim3(kHopThreads), 0, ctx->stream, in, ldi, n, f,
                       SUM ? bias : nullptr, out, ldo);
    GCNX_LAUNCH_OK(ctx);
    return GCNX_OK;
  }
  const float cs = (float)(-2.0 / (double)lambda_max), cd = (float)(2.0 / (double)lambda_max - 1.0);
  if (cb > 0) {
    ResArgs a{};
    a.rowptr = rowptr; a.colidx = colidx; a.vals = vals; a.graph_ptr = graph_ptr; a.cap = max_graph_rows; a.cb = cb;
    a.ncb = gcnx_cdiv(f, cb); a.in = in; a.ldi = ldi; a.bias = SUM ? bias : nullptr; a.f = f; a.k = k; a.cs = cs; a.cd = cd;
    a.out = out; a.ldo = ldo;
    const size_t fixed = 2ull * (size_t)max_graph_rows * cb * 4 + res_rp_bytes(max_graph_rows);
    a.ent_cap = (int32_t)res_ent_cap(max_graph_rows, cb, vals != nullptr, lds_max);
    const int lds = (int)((fixed + (size_t)a.ent_cap * res_ent_bytes(vals != nullptr) + 15) & ~(size_t)15);
    static bool limit_raised = false;       // the dynamic-LDS limit of both instantiations, once, at the largest size served
    if (!limit_raised) {
      GCNX_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(cheb_resident_kernel<true, SUM>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
      GCNX_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(cheb_resident_kernel<false, SUM>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
      limit_raised = true;
    }
    const dim3 grid((unsigned)((int64_t)b * a.ncb)), block(res_threads(max_graph_rows, cb));
    if (vals) hipLaunchKernelGGL((cheb_resident_kernel<true, SUM>), grid, block, lds, ctx->stream, a);
    else hipLaunchKernelGGL((cheb_resident_kernel<false, SUM>), grid, block, lds, ctx->stream, a);
    GCNX_LAUNCH_OK(ctx);
    return GCNX_OK;
  }
  // streamed, step s = 1 .. k-1.  basis: block s of out from blocks s-1 and s-2 (step 1 reads x and copies it into block 0).
  // sum: b_j, j = k-1-s, into out where j is even, else scratch; b_{j+2} sits in the buffer the step writes (step 2: in H_{k-1})
  const bool svec = vec && (nscr == 0 || gcnx_aligned16(scratch));
  const dim3 grid((unsigned)gcnx_cdiv((int64_t)n * (svec ? f / 4 : f), kHopThreads));
  HopArgs h{};
  h.rowptr = rowptr; h.colidx = colidx; h.vals = vals; h.n = n; h.f = f;
  for (int s = 1; s < k; ++s) {
    const bool first = s == 1, last = s == k - 1;
    const bool single = SUM ? last : first;
    h.a = single ? cs : 2.0f * cs;
    h.b = single ? cd : 2.0f * cd;
    if (SUM) {
      const int j = k - 1 - s;
      const bool to_out = (j & 1) == 0;
      h.out = to_out ? out : scratch;
      h.ldo = to_out ? ldo : f;
      h.inj = in + (int64_t)j * f; h.ldi = ldi;
      h.bias = last ? bias : nullptr;
      if (first) { h.z = in + (int64_t)(k - 1) * f; h.ldz = ldi; h.prev = nullptr; h.ldp = 0; }
      else if (s == 2) { h.prev = in + (int64_t)(k - 1) * f; h.ldp = ldi; }
      else { h.prev = h.out; h.ldp = h.ldo; }
    } else {
      h.out = out + (int64_t)s * f; h.ldo = ldo;
      h.z = first ? in : out + (int64_t)(s - 1) * f; h.ldz = first ? ldi : ldo;
      h.prev = s >= 2 ? out + (int64_t)(s - 2) * f : nullptr; h.ldp = ldo;
      h.echo = first ? out : nullptr; h.lde = ldo;
    }
    if (svec) {
      if (vals) hipLaunchKernelGGL((cheb_hop_kernel<true, true, SUM>), grid, dim3(kHopThreads), 0, ctx->stream, h);
      else hipLaunchKernelGGL((cheb_hop_kernel<true, false, SUM>), grid, dim3(kHopThreads), 0, ctx->stream, h);
    } else {
      if (vals) hipLaunchKernelGGL((cheb_hop_kernel<false, true, SUM>), grid, dim3(kHopThreads), 0, ctx->stream, h);
      else hipLaunchKernelGGL((cheb_hop_kernel<false, false, SUM>), grid, dim3(kHopThreads), 0, ctx->stream, h);
    }
    GCNX_LAUNCH_OK(ctx);
    if (SUM) { h.z = h.out; h.ldz = h.ldo; }
  }
  return GCNX_OK;
}

}  // namespace

extern "C" {

int gcnx_cheb_resident_ok(int64_t max_graph_rows, int32_t f, int64_t ld) { return res_shape_ok(max_graph_rows, f, ld) ? 1 : 0; }

int64_t gcnx_cheb_scratch_floats(int64_t n, int32_t f) { return n > 0 && f > 0 ? n * (int64_t)f : 0; }

int gcnx_cheb_norm(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* vals, const int32_t* rowptr_t,
                   const int32_t* colidx_t, const float* vals_t, int32_t n, float* vals_out) {
  GCNX_CHECK_CTX(ctx);
  GCNX_REQUIRE(ctx, n >= 0, "gcnx_cheb_norm: negative n");
  GCNX_REQUIRE(ctx, !ctx->capturing, "gcnx_cheb_norm uses the context's workspace and cannot be captured");
  if (n == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, rowptr && colidx && rowptr_t && colidx_t && vals_out, "gcnx_cheb_norm: NULL pointer");
  GCNX_REQUIRE(ctx, (vals == nullptr) == (vals_t == nullptr), "gcnx_cheb_norm: vals and vals_t must both be given or both be NULL");
  GCNX_REQUIRE(ctx, vals_out != vals_t || rowptr == rowptr_t, "gcnx_cheb_norm: vals_out overwrites the transposed values");
  int rc = gcnx_ws_reserve(ctx, (size_t)n * sizeof(float));
  if (rc) return rc;
  float* r = (float*)ctx->ws;
  const int grid = gcnx_cdiv(n, 256);
  hipLaunchKernelGGL(cheb_degree_kernel, dim3(grid), dim3(256), 0, ctx->stream, rowptr_t, colidx_t, vals_t, n, r);
  GCNX_LAUNCH_OK(ctx);
  hipLaunchKernelGGL(cheb_scale_kernel, dim3(grid), dim3(256), 0, ctx->stream, rowptr, colidx, vals, n, r, vals_out);
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

int gcnx_cheb_basis(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* vals, const int32_t* graph_ptr, int32_t b,
                    int32_t max_graph_rows, const float* x, int64_t ldx, int32_t n, int32_t f, int32_t k, float lambda_max,
                    int32_t col_block, float* out, int64_t ldo, float* scratch) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "Cheb basis");
  return cheb_run<false>(ctx, "gcnx_cheb_basis", rowptr, colidx, vals, graph_ptr, b, max_graph_rows, x, ldx, nullptr, n, f, k, lambda_max,
                         col_block, out, ldo, scratch);
}

int gcnx_cheb_sum(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* vals, const int32_t* graph_ptr, int32_t b,
                  int32_t max_graph_rows, const float* h, int64_t ldh, const float* bias, int32_t n, int32_t f, int32_t k,
                  float lambda_max, int32_t col_block, float* out, int64_t ldo, float* scratch) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "Cheb sum");
  return cheb_run<true>(ctx, "gcnx_cheb_sum", rowptr, colidx, vals, graph_ptr, b, max_graph_rows, h, ldh, bias, n, f, k, lambda_max,
                        col_block, out, ldo, scratch);
}

}  // extern "C"
