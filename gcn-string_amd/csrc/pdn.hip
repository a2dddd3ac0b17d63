// What gcnx.PDN (PyG's PDNConv, Pathfinder Discovery Networks) adds to the library: GCNConv's operator with edge
// weights that a two-layer MLP with a sigmoid learns from the edge features, normalised by the weighted degrees, and the
// gradient of that operator with respect to the MLP.
//
//     z_e = x_e W1 + b1      h_e = relu(z_e)      s_e = <w2, h_e> + b2      w_e = 1 if unit[e] else sigmoid(s_e)
//     deg_i = sum_{e in row i} w_e      r_i = deg_i^-1/2 (0 for an empty row)      v_e = r_i w_e r_j      vt_p = v_{perm_t[p]}
//                                                                                                          gcnx_pdn_operator
//     c_e = G_e w_e      q_i = sum_{e in row i} c_e r_col(e) + sum_{p in row i of the transposed pattern} c_{perm_t[p]} r_{colidx_t[p]}
//     dw_e = G_e r_i r_j - 1/2 r_i^3 q_i      ds_e = dw_e w_e (1 - w_e), 0 where unit[e]
//     dw2 = sum ds_e h_e   db2 = sum ds_e   dz_e = ds_e w2 * [z_e > 0]   dW1 = sum x_e (x) dz_e   db1 = sum dz_e
//                                                                                                          gcnx_pdn_operator_bwd
//
// Launches.  Forward: (1) a group of 16 lanes per row, dealt over the row's entries: the gate of every entry, the row's degree;
// (2) a thread per entry: v and vt from the same expression.  Backward: (1) a lane group per row again: q_i from a walk over the
// row and one over the row of the transposed pattern, then ds_e of the row's entries into scratch; (2) at most 256 workgroups
// over chunks of 64 to 256 entries: z and h recomputed, dz and ds h staged in LDS, every sum's element owned by one thread (or
// by the 256 / fw row lanes of its column where there are fewer than 256 elements); (3) one workgroup of 1024 threads folds the
// parts.
//
// Order and precision of the sums.  Every sum over entries has one fixed order and no atomics.  The degree, q and the four
// parameter gradients are accumulated in fp64: a lane adds its items in ascending order, the lanes are added in ascending
// order.  An item is one fp32 product (relative error 2^-24), a part is rounded to fp32 once, the fold once more: the fold
// adds at most 3 * 2^-24 of the sum of the items' magnitudes, whatever the number of entries.
// The MLP is evaluated by one function (pdn_z, pdn_logit) with explicit fmaf in a fixed order in all kernels: forward and
// backward agree bit for bit on z, and with it on the side of the ReLU, and on s.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "conv_tile.h"

namespace {

constexpr int kPdnThreads = 256;
constexpr int kPdnMaxHe = 64;             // hidden width of the gate MLP served
constexpr int kPdnChunk = 64;             // entries per trip of a workgroup of the parameter-gradient stage at he > 16 (pdn_chunk)
constexpr int kPdnChunkMax = 256;         // ... at he <= 8
constexpr int kPdnFoldThreads = 1024;     // the fold's one workgroup
constexpr int kPdnMaxParts = 256;         // its workgroups (= partial sums)
constexpr int kPdnPasses = 3;             // columns / 256 rounded up: (8 * 64 + 2 * 64 + 1) / 256

struct PdnMlp {
  const float* w1; const float* b1; const float* w2; const float* b2;     // device pointers: [d, he], [he], [he], [1]
  int32_t d, he;
};

// the MLP's parameters in LDS: W1 [d, he] at stride he, b1, w2, b2 (read by every lane at one address: a broadcast)
struct PdnLds {
  float w1[kEdgeMax * kPdnMaxHe];
  float b1[kPdnMaxHe];
  float w2[kPdnMaxHe];
  float b2;
};

__device__ __forceinline__ void pdn_stage(const PdnMlp& m, PdnLds& s) {
  for (int i = threadIdx.x; i < m.d * m.he; i += blockDim.x) s.w1[i] = m.w1[i];
  for (int i = threadIdx.x; i < m.he; i += blockDim.x) { s.b1[i] = m.b1[i]; s.w2[i] = m.w2[i]; }
  if (threadIdx.x == 0) s.b2 = m.b2[0];
  __syncthreads();
}

// one entry's features in registers (constant indices only: rows >= d are zero and never used)
__device__ __forceinline__ EdgeF<kEdgeMax> pdn_load_x(const float* __restrict__ e, int64_t lde, int d, int64_t entry) {
  EdgeF<kEdgeMax> x;
  const float* __restrict__ row = e + entry * lde;
#pragma unroll
  for (int k = 0; k < kEdgeMax; ++k) x.v[k] = k < d ? row[k] : 0.f;
  return x;
}

// z_e[k] = b1[k] + sum_d x_e[d] W1[d, k], d ascending
__device__ __forceinline__ float pdn_z(const EdgeF<kEdgeMax>& x, const PdnLds& s, int d, int he, int k) {
  float z = s.b1[k];
#pragma unroll
  for (int j = 0; j < kEdgeMax; ++j)
    if (j < d) z = fmaf(x.v[j], s.w1[j * he + k], z);
  return z;
}

// s_e = b2 + sum_k w2[k] relu(z_e[k]), k ascending
__device__ __forceinline__ float pdn_logit(const EdgeF<kEdgeMax>& x, const PdnLds& s, int d, int he) {
  float a = s.b2;
  for (int k = 0; k < he; ++k) {
    const float z = pdn_z(x, s, d, he, k);
    a = fmaf(s.w2[k], z > 0.f ? z : 0.f, a);
  }
  return a;
}

// A row belongs to a group of 16 lanes (four rows per wave: the reference's contact graphs average 15 entries per row, and a
// wave per row left three lanes in four idle; the row of 1 100 entries takes 69 trips of its group).  The sum of the group's 16
// values in a fixed order (lane += lane + off for off = 8 .. 1), the same bits in every lane of the group.
constexpr int kPdnRowLanes = 16;
constexpr int kPdnRowsPerWg = kPdnThreads / kPdnRowLanes;
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
  for (int off = kPdnRowLanes / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kPdnRowLanes);
  return __shfl(v, 0, kPdnRowLanes);
}

// ---- forward 1: a lane group per row: the gates of its entries, its degree -------------------------------------------------------
__global__ __launch_bounds__(kPdnThreads) void pdn_gate_kernel(const int32_t* __restrict__ rowptr, int32_t n, const float* __restrict__ e,
                                                               int64_t lde, PdnMlp m, const uint8_t* __restrict__ unit,
                                                               float* __restrict__ w_out, float* __restrict__ r_out) {
  __shared__ PdnLds s;
  pdn_stage(m, s);
  const int lane = threadIdx.x % kPdnRowLanes;
  const int64_t row = (int64_t)blockIdx.x * kPdnRowsPerWg + threadIdx.x / kPdnRowLanes;
  if (row >= n) return;                                     // (whole groups leave, behind the barrier; the exchanges stay inside a group)
  const int ea = rowptr[row], eb = rowptr[row + 1];
  double deg = 0.0;
  for (int en = ea + lane; en < eb; en += kPdnRowLanes) {   // ascending per lane
    float w = 1.0f;
    if (!(unit && unit[en])) w = sigmoid1(pdn_logit(pdn_load_x(e, lde, m.d, en), s, m.d, m.he));
    w_out[en] = w;
    deg += (double)w;
  }
  deg = group_sum(deg);
  const float df = (float)deg;
  if (lane == 0) r_out[row] = df > 0.f ? 1.0f / sqrtf(df) : 0.f;
}

// ---- forward 2: a thread per entry: v, and vt from the same expression ----------------------------------------------------------
__device__ __forceinline__ float pdn_value(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx, int n,
                                           const float* __restrict__ w, const float* __restrict__ r, int en) {
  return (r[row_of(rowptr, n, en)] * w[en]) * r[colidx[en]];
}

__global__ __launch_bounds__(kPdnThreads) void pdn_values_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                                                 int32_t n, int32_t nnz, const float* __restrict__ w,
                                                                 const float* __restrict__ r, const int32_t* __restrict__ perm_t,
                                                                 float* __restrict__ vals_out, float* __restrict__ vals_t_out) {
  const int en = blockIdx.x * kPdnThreads + threadIdx.x;
  if (en >= nnz) return;
  vals_out[en] = pdn_value(rowptr, colidx, n, w, r, en);
  if (vals_t_out) vals_t_out[en] = pdn_value(rowptr, colidx, n, w, r, perm_t[en]);       // the same expression: the same bits
}

// ---- backward 1: a lane group per row: q_i over the row and over the row of the transposed pattern, then ds of the row's entries ------
struct PdnBwdRows {
  const int32_t* rowptr; const int32_t* colidx; const int32_t* rowptr_t; const int32_t* colidx_t; const int32_t* perm_t;
  int32_t n;
  const float* e; int64_t lde;
  const uint8_t* unit;
  const float* w; const float* r; const float* g;
  float* ds;
};

__global__ __launch_bounds__(kPdnThreads) void pdn_bwd_rows_kernel(PdnBwdRows p, PdnMlp m) {
  __shared__ PdnLds s;
  pdn_stage(m, s);
  const int lane = threadIdx.x % kPdnRowLanes;
  const int64_t row = (int64_t)blockIdx.x * kPdnRowsPerWg + threadIdx.x / kPdnRowLanes;
  if (row >= p.n) return;
  const int ea = p.rowptr[row], eb = p.rowptr[row + 1];
  const int ta = p.rowptr_t[row], tb = p.rowptr_t[row + 1];
  double q = 0.0;
  for (int en = ea + lane; en < eb; en += kPdnRowLanes) q += (double)((p.g[en] * p.w[en]) * p.r[p.colidx[en]]);
  for (int t = ta + lane; t < tb; t += kPdnRowLanes) {
    const int en = p.perm_t[t];
    q += (double)((p.g[en] * p.w[en]) * p.r[p.colidx_t[t]]);
  }
  const float ri = p.r[row];
  const float ddeg = -0.5f * (ri * ri * ri) * (float)group_sum(q);
  for (int en = ea + lane; en < eb; en += kPdnRowLanes) {
    float d = 0.f;
    if (!(p.unit && p.unit[en])) {
      const float a = pdn_logit(pdn_load_x(p.e, p.lde, m.d, en), s, m.d, m.he);
      const float w = p.w[en];
      const float om = a >= 0.f ? __expf(-a) * w : 1.0f - w;             // 1 - w without the cancellation near w = 1
      d = fmaf(p.g[en] * ri, p.r[p.colidx[en]], ddeg) * (w * om);
    }
    p.ds[en] = d;
  }
}

// ---- backward 2 and 3: the sums over entries ------------------------------------------------------------------------------------
// The sums are the columns of one virtual [entries, ncols] matrix: column dd he + k: x_e[dd] dz_e[k] (dW1), d he + k: dz_e[k]
// (db1), d he + he + k: ds_e h_e[k] (dw2), d he + 2 he: ds_e (db2) -- the layout of a part.  fw columns at a time (a power of
// two <= 256) with 256 / fw row lanes per column: row lane j adds rows j, j + 256 / fw, ... in ascending order.
__device__ __forceinline__ int pdn_ncols(int d, int he) { return d * he + 2 * he + 1; }

// the row lanes' sums of one pass added in ascending order; valid in the first fw threads
template <int NT>
__device__ __forceinline__ double pdn_lanes_sum(double acc, int fw, double* s_acc) {
  s_acc[threadIdx.x] = acc;
  __syncthreads();
  double t = 0.0;
  if ((int)threadIdx.x < fw)
    for (int j = 0; j < NT / fw; ++j) t += s_acc[j * fw + threadIdx.x];
  __syncthreads();
  return t;
}

struct PdnBwdSums {
  int32_t nnz;
  const float* e; int64_t lde;
  const uint8_t* unit;
  const float* ds;
  float* part;
  int fw, chunk;
};

__global__ __launch_bounds__(kPdnThreads) void pdn_bwd_parts_kernel(PdnBwdSums p, PdnMlp m) {
  // chunk rows of stride hp = he | 1 (odd: the stores of a wave's entries hit different banks) in room for 64 rows of 65: a
  // barrier waits for every load in flight, so a trip pays the latency of its loads in full, and a narrow MLP takes more
  // entries per trip (pdn_chunk): 128 at he = 16 halves the trips of the 64 the widest MLP leaves room for
  __shared__ PdnLds s;
  __shared__ float s_dz[kPdnChunk * (kPdnMaxHe + 1)];
  __shared__ float s_hs[kPdnChunk * (kPdnMaxHe + 1)];
  __shared__ float s_x[kPdnChunkMax * kEdgeMax];
  __shared__ float s_ds[kPdnChunkMax];
  __shared__ double s_acc[kPdnThreads];
  pdn_stage(m, s);
  const int d = m.d, he = m.he, ncols = pdn_ncols(d, he);
  const int fw = p.fw, lanes = kPdnThreads / fw, lane = threadIdx.x / fw;
  const int chunk = p.chunk, tpe = kPdnThreads / chunk, HP = he | 1;
  const int el = threadIdx.x / tpe, sub = threadIdx.x % tpe;   // stage: tpe = 4, 2 or 1 threads per entry, k dealt among them
  double acc[kPdnPasses] = {0.0, 0.0, 0.0};
  const int chunks = (p.nnz + chunk - 1) / chunk;
  for (int c = blockIdx.x; c < chunks; c += gridDim.x) {    // ascending per workgroup; uniform: every thread meets the barriers
    const int en = c * chunk + el;
    const bool live = en < p.nnz && !(p.unit && p.unit[en]);
    const float dse = live ? p.ds[en] : 0.f;
    EdgeF<kEdgeMax> x;
#pragma unroll
    for (int k = 0; k < kEdgeMax; ++k) x.v[k] = 0.f;
    if (live) x = pdn_load_x(p.e, p.lde, d, en);
    for (int k = sub; k < he; k += tpe) {
      const float z = live ? pdn_z(x, s, d, he, k) : 0.f;
      s_hs[el * HP + k] = z > 0.f ? dse * z : 0.f;
      s_dz[el * HP + k] = z > 0.f ? dse * s.w2[k] : 0.f;
    }
    if (sub == 0) {
      s_ds[el] = dse;
#pragma unroll
      for (int k = 0; k < kEdgeMax; ++k) s_x[el * kEdgeMax + k] = x.v[k];
    }
    __syncthreads();
#pragma unroll
    for (int ps = 0; ps < kPdnPasses; ++ps) {
      const int col = ps * fw + (int)threadIdx.x % fw;
      if (col < ncols) {                                    // (unrolled: eight rows' LDS reads in flight per add chain)
        const int k = col < d * he ? col % he : col < d * he + he ? col - d * he : col < d * he + 2 * he ? col - d * he - he : 0;
        if (col < d * he) {
          const int dd = col / he;
#pragma unroll 8
          for (int r = lane; r < chunk; r += lanes) acc[ps] += (double)(s_x[r * kEdgeMax + dd] * s_dz[r * HP + k]);
        } else if (col < d * he + he) {
#pragma unroll 8
          for (int r = lane; r < chunk; r += lanes) acc[ps] += (double)s_dz[r * HP + k];
        } else if (col < d * he + 2 * he) {
#pragma unroll 8
          for (int r = lane; r < chunk; r += lanes) acc[ps] += (double)s_hs[r * HP + k];
        } else {
#pragma unroll 8
          for (int r = lane; r < chunk; r += lanes) acc[ps] += (double)s_ds[r];
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int ps = 0; ps < kPdnPasses; ++ps) {
    if (ps * fw >= ncols) break;                            // (uniform)
    const double t = pdn_lanes_sum<kPdnThreads>(acc[ps], fw, s_acc);
    const int col = ps * fw + (int)threadIdx.x;
    if ((int)threadIdx.x < fw && col < ncols) p.part[(int64_t)blockIdx.x * ncols + col] = (float)t;
  }
}

// one workgroup: the parts of a column dealt to its row lanes, then the lanes; the four gradients written where they belong
__global__ __launch_bounds__(kPdnFoldThreads) void pdn_bwd_fold_kernel(const float* __restrict__ part, int nparts, int d, int he, int fw,
                                                                   float* __restrict__ dw1, float* __restrict__ db1,
                                                                   float* __restrict__ dw2, float* __restrict__ db2) {
  __shared__ double s_acc[kPdnFoldThreads];
  const int ncols = pdn_ncols(d, he), lanes = kPdnFoldThreads / fw, lane = threadIdx.x / fw;
  for (int c0 = 0; c0 < ncols; c0 += fw) {                  // (uniform trip count)
    const int col = c0 + (int)threadIdx.x % fw;
    double acc = 0.0;
    if (col < ncols) {
      for (int b = lane; b < nparts; b += 8 * lanes) {      // eight loads in flight, added in ascending order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = b + u * lanes < nparts ? part[(int64_t)(b + u * lanes) * ncols + col] : 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += (double)v[u];
      }
    }
    const double t = pdn_lanes_sum<kPdnFoldThreads>(acc, fw, s_acc);
    if (lane == 0 && col < ncols) {
      const float v = (float)t;
      if (col < d * he) dw1[col] = v;
      else if (col < d * he + he) db1[col - d * he] = v;
      else if (col < d * he + 2 * he) dw2[col - d * he - he] = v;
      else db2[0] = v;
    }
  }
}

int pdn_parts(int64_t nnz) {
  const int64_t want = (nnz + kPdnChunk - 1) / kPdnChunk;
  return (int)(want < 1 ? 1 : want > kPdnMaxParts ? kPdnMaxParts : want);
}
// entries per trip of the parts kernel: what fits its LDS rows (64 rows of 65 floats) at stride he | 1, a divisor of 256
int pdn_chunk(int he) { return he <= 8 ? kPdnChunkMax : he <= 16 ? 128 : kPdnChunk; }
int pdn_fw(int d, int he) {
  const int ncols = d * he + 2 * he + 1;
  int fw = 1;
  while (fw < ncols && fw < kPdnThreads) fw <<= 1;
  return fw;
}
// the ds [nnz] of backward 1 in front (rounded up to 4 floats), the parts behind it
int64_t pdn_ds_floats(int64_t nnz) { return (nnz + 3) / 4 * 4; }

}  // namespace

extern "C" {

int gcnx_pdn_ok(int32_t d, int32_t he) { return d >= 1 && d <= kEdgeMax && he >= 1 && he <= kPdnMaxHe ? 1 : 0; }

int gcnx_pdn_operator(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, int32_t n, int32_t nnz, const float* e, int64_t lde,
                      int32_t d, const float* w1, const float* b1, const float* w2, const float* b2, int32_t he, const uint8_t* unit,
                      const int32_t* perm_t, float* w_out, float* r_out, float* vals_out, float* vals_t_out) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "PDN operator");
  GCNX_REQUIRE(ctx, n >= 0 && nnz >= 0, "gcnx_pdn_operator: negative size");
  GCNX_REQUIRE(ctx, gcnx_pdn_ok(d, he), "gcnx_pdn_operator: d = %d must be 1 .. 8 and he = %d must be 1 .. 64", d, he);
  if (n == 0 || nnz == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, rowptr && colidx && e && w1 && b1 && w2 && b2 && w_out && r_out && vals_out, "gcnx_pdn_operator: NULL pointer");
  GCNX_REQUIRE(ctx, (perm_t != nullptr) == (vals_t_out != nullptr), "gcnx_pdn_operator: perm_t and vals_t_out go together");
  GCNX_REQUIRE(ctx, lde >= d, "gcnx_pdn_operator: lde must be >= d");
  const PdnMlp m{w1, b1, w2, b2, d, he};
  hipLaunchKernelGGL(pdn_gate_kernel, dim3(gcnx_cdiv(n, kPdnRowsPerWg)), dim3(kPdnThreads), 0, ctx->stream, rowptr, n, e, lde, m, unit, w_out,
                     r_out);
  GCNX_LAUNCH_OK(ctx);
  hipLaunchKernelGGL(pdn_values_kernel, dim3(gcnx_cdiv(nnz, kPdnThreads)), dim3(kPdnThreads), 0, ctx->stream, rowptr, colidx, n, nnz,
                     (const float*)w_out, (const float*)r_out, perm_t, vals_out, vals_t_out);
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

int64_t gcnx_pdn_bwd_scratch_floats(int64_t n, int64_t nnz, int32_t d, int32_t he) {
  if (n < 0 || nnz < 0 || !gcnx_pdn_ok(d, he)) return 0;
  return pdn_ds_floats(nnz) + (int64_t)pdn_parts(nnz) * (d * he + 2 * he + 1);
}

int gcnx_pdn_operator_bwd(gcnx_ctx* ctx, const int32_t* rowptr, const int32_t* colidx, const int32_t* rowptr_t, const int32_t* colidx_t,
                          const int32_t* perm_t, int32_t n, int32_t nnz, const float* e, int64_t lde, int32_t d, const float* w1,
                          const float* b1, const float* w2, const float* b2, int32_t he, const uint8_t* unit, const float* w,
                          const float* r, const float* g, float* dw1, float* db1, float* dw2, float* db2, float* scratch) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "PDN operator backward");
  GCNX_REQUIRE(ctx, n >= 0 && nnz >= 0, "gcnx_pdn_operator_bwd: negative size");
  GCNX_REQUIRE(ctx, gcnx_pdn_ok(d, he), "gcnx_pdn_operator_bwd: d = %d must be 1 .. 8 and he = %d must be 1 .. 64", d, he);
  GCNX_REQUIRE(ctx, dw1 && db1 && dw2 && db2, "gcnx_pdn_operator_bwd: NULL gradient");
  if (n == 0 || nnz == 0) {                                 // written, not accumulated: the sums over no entries
    GCNX_HIP(ctx, hipMemsetAsync(dw1, 0, sizeof(float) * d * he, ctx->stream));
    GCNX_HIP(ctx, hipMemsetAsync(db1, 0, sizeof(float) * he, ctx->stream));
    GCNX_HIP(ctx, hipMemsetAsync(dw2, 0, sizeof(float) * he, ctx->stream));
    GCNX_HIP(ctx, hipMemsetAsync(db2, 0, sizeof(float), ctx->stream));
    return GCNX_OK;
  }
  GCNX_REQUIRE(ctx, rowptr && colidx && rowptr_t && colidx_t && perm_t && e && w1 && b1 && w2 && b2 && w && r && g && scratch,
               "gcnx_pdn_operator_bwd: NULL pointer");
  GCNX_REQUIRE(ctx, lde >= d, "gcnx_pdn_operator_bwd: lde must be >= d");
  const PdnMlp m{w1, b1, w2, b2, d, he};
  float* ds = scratch;
  float* part = scratch + pdn_ds_floats(nnz);
  PdnBwdRows a{};
  a.rowptr = rowptr; a.colidx = colidx; a.rowptr_t = rowptr_t; a.colidx_t = colidx_t; a.perm_t = perm_t; a.n = n; a.e = e; a.lde = lde;
  a.unit = unit; a.w = w; a.r = r; a.g = g; a.ds = ds;
  hipLaunchKernelGGL(pdn_bwd_rows_kernel, dim3(gcnx_cdiv(n, kPdnRowsPerWg)), dim3(kPdnThreads), 0, ctx->stream, a, m);
  GCNX_LAUNCH_OK(ctx);
  const int chunk = pdn_chunk(he), fw = pdn_fw(d, he);
  const int parts = std::min(pdn_parts(nnz), gcnx_cdiv(nnz, chunk));       // (never more than the scratch holds)
  PdnBwdSums b{};
  b.nnz = nnz; b.e = e; b.lde = lde; b.unit = unit; b.ds = ds; b.part = part; b.fw = fw; b.chunk = chunk;
  hipLaunchKernelGGL(pdn_bwd_parts_kernel, dim3(parts), dim3(kPdnThreads), 0, ctx->stream, b, m);
  GCNX_LAUNCH_OK(ctx);
  hipLaunchKernelGGL(pdn_bwd_fold_kernel, dim3(1), dim3(kPdnFoldThreads), 0, ctx->stream, (const float*)part, parts, d, he, fw, dw1, db1, dw2,
                     db2);
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

}  // extern "C"
