// APPNP propagation (Spektral's APPNPConv, PyG's APPNP(K, alpha)): K parameter-free hops of personalised PageRank behind a
// Linear, the long-range counterpart of the one-hop convolutions the reference's author left a slot for (gcn_utills.py:804-806):
//
//     z^0 = x      z^{k+1}[i, :] = (1 - alpha) * sum_{e in row i, CSR order} vals[e] * z^k[colidx[e], :] + alpha * x[i, :]      out = z^K
//
// Two routes, one expression per element: acc = +0, acc = fmaf(vals[e], z^k[colidx[e]], acc) entry by entry, then
// fmaf(alpha, x, (1 - alpha) * acc) with (1 - alpha) rounded once on the host.  Both routes and every column block therefore
// leave the same bits, and which graphs share a batch never changes a result.
//
// Resident route (one launch).  A disjoint batch is block-diagonal: a graph's hops read its own rows only, and a column its
// own column only.  A workgroup (256 .. 1024 threads: one per float4 of the tallest graph's slice) owns one (graph, block of
// cb columns): it loads the graph's n_g x cb slice of
// x into LDS, stages the graph's row pointers and as many of its CSR entries as the rest of its LDS holds (the neighbour's row
// inside the graph as 16 bits, and the weight: 6 bytes per entry, 2 without values; what does not fit is read from global
// memory on every hop), and runs the K hops between two LDS buffers with one workgroup barrier per hop; hop K stores to `out`.
// cb / 4 lanes hold a row (one float4 each, ds_read_b128 gathers); the row groups walk the graph's rows in strides, eight
// entries per trip, all reads of a trip issued before its first fma.  The alpha * x term of a lane group's first four rows
// stays in registers under that static map (a global load per row and hop is a latency the hop then waits for); rows beyond
// them -- a graph of more than 4 * 1024 / (cb / 4) rows -- re-read theirs, issued ahead of the row's gather.  Every entry is
// range-checked against the graph's rows when it is staged or read: one that lies outside contributes nothing, so no LDS
// address is ever out of range.
//
// Streamed route (K launches): a one-hop gather with the same epilogue, cb = f / 4 lanes per row over the whole batch (or a
// thread per element where f % 4 != 0 or an operand is off a 16-byte boundary), ping-ponging between `out` and the caller's
// scratch so that hop K lands in `out`.
//
// No atomics, no host read-back, nothing allocated: capture-safe.
#include "common.h"
#include "conv_tile.h"
#include "resident_hops.h"

namespace {

constexpr int kResXR = 4;                    // rows per lane group whose alpha * x term stays in registers
constexpr int kMaxHops = 64;
// Hops from which the library's choice is the resident route: what its prologue (the slice, the row pointers and the entries into
// LDS) costs is earned back from the second hop on where the graphs are small and from the third where they are tall (measured
// at 64 and at 808 / 1152 rows: DESIGN 4.23); below, the library streams
constexpr int kResMinHops = 3, kResMinHopsSmall = 2, kResSmallRows = 256;

struct ResArgs {
  const int32_t* rowptr; const int32_t* colidx; const float* vals;
  const int32_t* graph_ptr;
  int32_t cap;                 // rows of the tallest graph served (max_graph_rows): the LDS layout
  int32_t cb, ncb;             // columns per block, blocks per graph
  int32_t ent_cap;             // CSR entries staged
  const float* x; int64_t ldx;
  int32_t f, k;
  float alpha, oma;
  float* out; int64_t ldo;
};

// fmaf(alpha, x, (1 - alpha) * acc): the epilogue of both routes
__device__ __forceinline__ float teleport1(float alpha, float x, float oma, float acc) { return fmaf(alpha, x, oma * acc); }
__device__ __forceinline__ float4 teleport4(float alpha, float4 x, float oma, float4 a) {
  return make_float4(teleport1(alpha, x.x, oma, a.x), teleport1(alpha, x.y, oma, a.y), teleport1(alpha, x.z, oma, a.z),
                     teleport1(alpha, x.w, oma, a.w));
}

// LDS: z0 [cap, cb] | z1 [cap, cb] | s_rp [cap + 1, padded to 4] | s_val [ent_cap] (WEIGHTED only) | s_col [ent_cap] uint16
template <bool WEIGHTED>
__global__ __launch_bounds__(kResThreads) void appnp_resident_kernel(ResArgs p) {
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
  // the static element-to-thread map of every pass below: lane group rg walks rows rg, rg + ngrp, ...; the alpha * x term of
  // its first kResXR rows stays in registers, the rows of a taller graph re-read theirs (issued ahead of the row's gather)
  const int ngrp = nthr / lpr;
  const int rg = tid / lpr, sub = tid - rg * lpr;
  const int col = jb * cb + 4 * sub;
  const bool active = rg < ngrp && col < p.f;
  const float* xcol = p.x + (int64_t)r0 * p.ldx + col;
  float4 xr[kResXR];
#pragma unroll
  for (int q = 0; q < kResXR; ++q) {
    const int r = rg + q * ngrp;
    xr[q] = zero4();
    if (active && r < ng) {
      xr[q] = load4(xcol + (int64_t)r * p.ldx);
      *reinterpret_cast<float4*>(z0 + r * cb + 4 * sub) = xr[q];
    }
  }
  if (active)
    for (int r = rg + kResXR * ngrp; r < ng; r += ngrp) *reinterpret_cast<float4*>(z0 + r * cb + 4 * sub) = load4(xcol + (int64_t)r * p.ldx);
  __syncthreads();

  const int rowb = cb * 4, sub16 = sub * 16;                 // bytes per row of the slice, this lane's offset in it
  const int32_t* gcol = p.colidx + e0;
  const float* gval = WEIGHTED ? p.vals + e0 : nullptr;
  for (int k = 0; k < p.k; ++k) {
    const char* cur = reinterpret_cast<const char*>((k & 1) ? z1 : z0);
    float* nxt = (k & 1) ? z0 : z1;
    const bool last = k + 1 == p.k;
    auto row = [&](int r, float4 xv) {
      const int ea = s_rp[r], eb = s_rp[r + 1];
      float4 acc = res_row_staged<WEIGHTED>(s_col, s_val, cur, rowb, sub16, min(ea, staged), min(eb, staged), zero4());
      if (eb > staged) acc = res_row_global<WEIGHTED>(gcol, gval, r0, ng, cur, rowb, sub16, max(ea, staged), eb, acc);
      const float4 res = teleport4(p.alpha, xv, p.oma, acc);
      if (last) *reinterpret_cast<float4*>(p.out + (int64_t)(r0 + r) * p.ldo + col) = res;
      else *reinterpret_cast<float4*>(nxt + r * cb + 4 * sub) = res;
    };
    if (active) {
#pragma unroll
      for (int q = 0; q < kResXR; ++q)
        if (rg + q * ngrp < ng) row(rg + q * ngrp, xr[q]);
      for (int r = rg + kResXR * ngrp; r < ng; r += ngrp) row(r, load4(xcol + (int64_t)r * p.ldx));
    }
    if (!last) __syncthreads();
  }
}

struct HopArgs {
  const int32_t* rowptr; const int32_t* colidx; const float* vals;
  const float* z; int64_t ldz;      // z^k
  const float* x; int64_t ldx;
  int32_t n, f;
  float alpha, oma;
  float* out; int64_t ldo;          // z^{k+1}
};

// one hop over the whole batch: VEC: f / 4 threads per row (float4 each); otherwise a thread per element
template <bool VEC, bool WEIGHTED>
__global__ __launch_bounds__(kHopThreads) void appnp_hop_kernel(HopArgs p) {
  const int lpr = VEC ? p.f >> 2 : p.f;
  const int64_t idx = (int64_t)blockIdx.x * kHopThreads + threadIdx.x;
  const int64_t row = idx / lpr;
  if (row >= p.n) return;
  const int col = (int)(idx - row * lpr) * (VEC ? 4 : 1);
  const int ea = p.rowptr[row], eb = p.rowptr[row + 1];
  const float* zc = p.z + col;
  if constexpr (VEC) {
    const float4 xv = load4(p.x + row * p.ldx + col);
    const float4 acc = hop_row4<WEIGHTED>(p.colidx, p.vals, zc, p.ldz, p.n, row, ea, eb);
    *reinterpret_cast<float4*>(p.out + row * p.ldo + col) = teleport4(p.alpha, xv, p.oma, acc);
  } else {
    const float xv = p.x[row * p.ldx + col];
    const float acc = hop_row1<WEIGHTED>(p.colidx, p.vals, zc, p.ldz, p.n, ea, eb);
    p.out[row * p.ldo + col] = teleport1(p.alpha, xv, p.oma, acc);
  }
}

// k == 0: out = x, element by element (any f, leading dimensions and alignment)
__global__ __launch_bounds__(kHopThreads) void appnp_copy_kernel(const float* __restrict__ x, int64_t ldx, int32_t n, int32_t f,
                                                                 float* __restrict__ out, int64_t ldo) {
  const int64_t idx = (int64_t)blockIdx.x * kHopThreads + threadIdx.x;
  const int64_t row = idx / f;
  if (row < n) out[row * ldo + (idx - row * f)] = x[row * ldx + (idx - row * f)];
}

}  // namespace

extern "C" {

int gcnx_appnp_resident_ok(int64_t max_graph_rows, int32_t f, int64_t ldx) { return res_shape_ok(max_graph_rows, f, ldx) ? 1 : 0; }

int64_t gcnx_appnp_scratch_floats(int64_t n, int32_t f) { return n > 0 && f > 0 ? n * (int64_t)f : 0; }

int gcnx_appnp_propagate(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const float* vals, const int32_t* graph_ptr,
                         int32_t b, int32_t max_graph_rows, const float* x, int64_t ldx, int32_t n, int32_t f, int32_t k, float alpha,
                         int32_t col_block, float* out, int64_t ldo, float* scratch) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "APPNP propagate");
  GCNX_REQUIRE(ctx, n >= 0 && f >= 0 && b >= 0 && max_graph_rows >= 0, "gcnx_appnp_propagate: negative size");
  GCNX_REQUIRE(ctx, k >= 0 && k <= kMaxHops, "gcnx_appnp_propagate: k = %d must be in 0 .. %d", k, kMaxHops);
  GCNX_REQUIRE(ctx, alpha >= 0.f && alpha <= 1.f, "gcnx_appnp_propagate: alpha = %g must be in [0, 1]", (double)alpha);
  GCNX_REQUIRE(ctx, col_block >= -1, "gcnx_appnp_propagate: col_block = %d (0: the library's choice, > 0: resident, -1: streamed)",
               col_block);
  GCNX_REQUIRE(ctx, ldx >= f && ldo >= f, "gcnx_appnp_propagate: ldx, ldo < f");
  const int64_t nscr = gcnx_appnp_scratch_floats(n, f);
  GCNX_REQUIRE(ctx, !overlap(out, span(n, ldo, f), x, span(n, ldx, f)), "gcnx_appnp_propagate: out overlaps x");
  GCNX_REQUIRE(ctx, !overlap(out, span(n, ldo, f), scratch, nscr) && !overlap(x, span(n, ldx, f), scratch, nscr),
               "gcnx_appnp_propagate: scratch overlaps out or x");
  static size_t lds_max = 0;               // (res_lds_max, read once)
  if (lds_max == 0 && res_lds_max(ctx, &lds_max) != GCNX_OK) return GCNX_ERR_HIP;
  const bool vec = f % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && gcnx_aligned16(x) && gcnx_aligned16(out);
  const bool res_ok = graph_ptr && vec && res_shape_ok(max_graph_rows, f, ldx);
  int cb = 0;
  if (col_block > 0) {
    if (!res_ok || col_block % 4 != 0 || col_block > f || !res_fits(max_graph_rows, col_block))
      return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "gcnx_appnp_propagate: col_block = %d is not served: the resident route needs graph_ptr, "
                       "max_graph_rows > 0, f, ldx, ldo and col_block in multiples of 4 floats, col_block <= f, 16-byte aligned x and "
                       "out, and 2 * max_graph_rows * col_block * 4 bytes + the row pointers within %d bytes of LDS (got "
                       "max_graph_rows=%d f=%d)", col_block, kResLdsMax, max_graph_rows, f);
    cb = col_block;
  } else if (col_block == 0 && res_ok && k >= (max_graph_rows <= kResSmallRows ? kResMinHopsSmall : kResMinHops)) {
    cb = res_choose_cb(ctx, max_graph_rows, f, b, vals != nullptr, lds_max);
  }
  if (n == 0 || f == 0 || (graph_ptr && b == 0)) return GCNX_OK;
  GCNX_REQUIRE(ctx, rowptr && colidx && x && out, "gcnx_appnp_propagate: NULL pointer");
  GCNX_REQUIRE(ctx, cb > 0 || k < 2 || scratch, "gcnx_appnp_propagate: the streamed route with k >= 2 needs scratch "
               "(gcnx_appnp_scratch_floats)");
  GCNX_REQUIRE(ctx, (int64_t)n * f < (1ll << 38), "gcnx_appnp_propagate: n * f = %lld elements are not served", (long long)n * f);

  if (k == 0) {
    hipLaunchKernelGGL(appnp_copy_kernel, dim3(gcnx_cdiv((int64_t)n * f, kHopThreads)), dim3(kHopThreads), 0, ctx->stream, x, ldx, n, f,
                       out, ldo);
    GCNX_LAUNCH_OK(ctx);
    return GCNX_OK;
  }
  const float oma = 1.0f - alpha;
  if (cb > 0) {
    ResArgs a{};
    a.rowptr = rowptr; a.colidx = colidx; a.vals = vals; a.graph_ptr = graph_ptr; a.cap = max_graph_rows; a.cb = cb;
    a.ncb = gcnx_cdiv(f, cb); a.x = x; a.ldx = ldx; a.f = f; a.k = k; a.alpha = alpha; a.oma = oma; a.out = out; a.ldo = ldo;
    const size_t fixed = 2ull * (size_t)max_graph_rows * cb * 4 + res_rp_bytes(max_graph_rows);
    a.ent_cap = (int32_t)res_ent_cap(max_graph_rows, cb, vals != nullptr, lds_max);
    const int lds = (int)((fixed + (size_t)a.ent_cap * res_ent_bytes(vals != nullptr) + 15) & ~(size_t)15);
    static bool limit_raised = false;       // the dynamic-LDS limit of both instantiations, once, at the largest size served
    if (!limit_raised) {
      GCNX_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(appnp_resident_kernel<true>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
      GCNX_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(appnp_resident_kernel<false>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
      limit_raised = true;
    }
    const dim3 grid((unsigned)((int64_t)b * a.ncb));
    const dim3 block(res_threads(max_graph_rows, cb));
    if (vals) hipLaunchKernelGGL(appnp_resident_kernel<true>, grid, block, lds, ctx->stream, a);
    else hipLaunchKernelGGL(appnp_resident_kernel<false>, grid, block, lds, ctx->stream, a);
    GCNX_LAUNCH_OK(ctx);
    return GCNX_OK;
  }
  // streamed: hop j (1 .. k) writes `out` where k - j is even, else scratch; hop 1 reads x
  const bool svec = vec && (k < 2 || gcnx_aligned16(scratch));
  const int64_t items = (int64_t)n * (svec ? f / 4 : f);
  const dim3 grid((unsigned)gcnx_cdiv(items, kHopThreads));
  HopArgs h{};
  h.rowptr = rowptr; h.colidx = colidx; h.vals = vals; h.x = x; h.ldx = ldx; h.n = n; h.f = f; h.alpha = alpha; h.oma = oma;
  h.z = x; h.ldz = ldx;
  for (int j = 1; j <= k; ++j) {
    const bool to_out = ((k - j) & 1) == 0;
    h.out = to_out ? out : scratch;
    h.ldo = to_out ? ldo : f;
    if (svec) {
      if (vals) hipLaunchKernelGGL((appnp_hop_kernel<true, true>), grid, dim3(kHopThreads), 0, ctx->stream, h);
      else hipLaunchKernelGGL((appnp_hop_kernel<true, false>), grid, dim3(kHopThreads), 0, ctx->stream, h);
    } else {
      if (vals) hipLaunchKernelGGL((appnp_hop_kernel<false, true>), grid, dim3(kHopThreads), 0, ctx->stream, h);
      else hipLaunchKernelGGL((appnp_hop_kernel<false, false>), grid, dim3(kHopThreads), 0, ctx->stream, h);
    }
    GCNX_LAUNCH_OK(ctx);
    h.z = h.out; h.ldz = h.ldo;
  }
  return GCNX_OK;
}

}  // extern "C"
