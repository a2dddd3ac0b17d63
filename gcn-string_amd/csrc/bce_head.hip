// The post-pool half of the reference's torch GCN (gcn_utills.py:846-853) with its loss and backward in ONE launch:
//   z3 = P W3^T + b3,  y3 = PReLU_a3(BN3(z3))         [b, h]
//   z4 = y3 W4^T + b4, out = PReLU_a4(BN4(z4))        [b, 1]   (the logits torch's forward returns)
//   loss = BCEWithLogits(out, t) (mean over the graphs), accuracy = #(out > 0 == t)   (binary_acc, gcn.py:42-57)
// and, for a training step, dP and the gradients of the ten parameters.  BatchNorm1d(track_running_stats=False): batch
// mean, biased variance, eps -- every BN needs all b rows, so one workgroup owns the whole head.  At the reference's sizes
// (b = 50, h = 64) the head is a few hundred thousand flops: as separate launches it would be ~20 launches of latency.
//
// One workgroup of 256 threads; thread j owns column j of layer 3 (h <= 256).  Intermediates live in the caller's
// scratch: z3 [b, h], y3 [b, h] (dZ3 in the backward), W3^T [h, h], z4 [b], dz4 [b].  Every reduction has a fixed order.
#include "common.h"

namespace {

constexpr int kT = 256;   // threads = the widest h served
constexpr int kRB = 8;    // rows staged in LDS per pass of the row-times-matrix products

__device__ __forceinline__ float zb_of(float z, float mu, float sc, float be) { return __builtin_fmaf(z - mu, sc, be); }
__device__ __forceinline__ float prelu1(float x, float a) { return x > 0.f ? x : a * x; }

__device__ __forceinline__ float block_sum(float v, float* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = kT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

// out[r, c] = bias[c] + sum_k a[r, k] m[k, c] for r < rows, c < h (m row-major [h, h]); rows of `a` staged in LDS kRB at a
// time, thread c reads column c of m (coalesced across the workgroup).  Ends with a barrier.
__device__ void rows_times(const float* a, int64_t lda, int rows, int h, const float* m, const float* bias, float* out,
                           int64_t ldo, float (*sa)[kT]) {
  const int c = threadIdx.x;
  for (int r0 = 0; r0 < rows; r0 += kRB) {
    const int nr = min(kRB, rows - r0);
    for (int i = threadIdx.x; i < kRB * h; i += kT) {
      const int r = i / h, k = i - r * h;
      sa[r][k] = r < nr ? a[(int64_t)(r0 + r) * lda + k] : 0.f;
    }
    __syncthreads();
    if (c < h) {
      float acc[kRB];
      const float b0 = bias ? bias[c] : 0.f;
#pragma unroll
      for (int r = 0; r < kRB; ++r) acc[r] = 0.f;
#pragma unroll 8
      for (int k = 0; k < h; ++k) {
        const float w = m[(int64_t)k * h + c];
#pragma unroll
        for (int r = 0; r < kRB; ++r) acc[r] = __builtin_fmaf(sa[r][k], w, acc[r]);
      }
      for (int r = 0; r < nr; ++r) out[(int64_t)(r0 + r) * ldo + c] = acc[r] + b0;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kT) void bce_head_kernel(gcnx_bce_head_args a) {
  __shared__ float sa[kRB][kT];
  __shared__ float sb[kRB][kT];
  __shared__ float red[kT];
  const int tid = threadIdx.x, B = a.b, H = a.h;
  float* z3 = a.scratch;
  float* y3 = z3 + (int64_t)B * H;
  float* w3t = y3 + (int64_t)B * H;
  float* z4 = w3t + (int64_t)H * H;
  float* dz4 = z4 + B;
  const float inv_b = 1.0f / (float)B;

  // ---- forward: z3 = P W3^T + b3 (W3^T staged once: coalesced operand reads) ----
  for (int i = tid; i < H * H; i += kT) {
    const int k = i / H, j = i - k * H;
    w3t[i] = a.w3[(int64_t)j * H + k];
  }
  __syncthreads();
  rows_times(a.pooled, a.ldp, B, H, w3t, a.b3, z3, H, sa);

  // BN3 (two-pass moments) + PReLU3, column j per thread
  const int j = tid;
  float mu3 = 0.f, iv3 = 0.f, ga3 = 0.f, be3 = 0.f;
  const float al3 = a.alpha3[0];
  if (j < H) {
    float s = 0.f;
#pragma unroll 8
    for (int r = 0; r < B; ++r) s += z3[(int64_t)r * H + j];
    mu3 = s * inv_b;
    float v = 0.f;
#pragma unroll 8
    for (int r = 0; r < B; ++r) { const float d = z3[(int64_t)r * H + j] - mu3; v = __builtin_fmaf(d, d, v); }
    iv3 = 1.0f / sqrtf(v * inv_b + a.eps);
    ga3 = a.gamma3[j];
    be3 = a.beta3[j];
    const float sc = ga3 * iv3;
#pragma unroll 8
    for (int r = 0; r < B; ++r) y3[(int64_t)r * H + j] = prelu1(zb_of(z3[(int64_t)r * H + j], mu3, sc, be3), al3);
  }
  __syncthreads();

  // z4 = y3 W4^T + b4, then BN4 over the b values
  float s4 = 0.f;
  for (int r = tid; r < B; r += kT) {
    float acc = 0.f;
#pragma unroll 8
    for (int k = 0; k < H; ++k) acc = __builtin_fmaf(y3[(int64_t)r * H + k], a.w4[k], acc);
    z4[r] = acc + a.b4[0];
    s4 += z4[r];
  }
  const float mu4 = block_sum(s4, red) * inv_b;
  float v4 = 0.f;
  for (int r = tid; r < B; r += kT) { const float d = z4[r] - mu4; v4 = __builtin_fmaf(d, d, v4); }
  const float iv4 = 1.0f / sqrtf(block_sum(v4, red) * inv_b + a.eps);
  const float ga4 = a.gamma4[0], be4 = a.beta4[0], al4 = a.alpha4[0], sc4 = ga4 * iv4;

  // out, probabilities, loss, hits; the output layer's backward terms on the way
  const bool grads = a.grads && a.y;
  float loss = 0.f, hits = 0.f, t0 = 0.f, t1 = 0.f, t2 = 0.f;
  for (int r = tid; r < B; r += kT) {
    const float zb = zb_of(z4[r], mu4, sc4, be4);
    const float o = prelu1(zb, al4);
    const float p = 1.0f / (1.0f + expf(-o));
    if (a.out) a.out[r] = o;
    if (a.probs) a.probs[r] = p;
    if (a.y) {
      const float t = a.y[(int64_t)r * a.y_stride + a.y_col];
      loss += fmaxf(o, 0.f) - o * t + log1pf(expf(-fabsf(o)));
      hits += ((o > 0.f) == (t > 0.5f)) ? 1.f : 0.f;
      if (grads) {
        const float d = (p - t) / a.denom;
        const float dzb = zb > 0.f ? d : al4 * d;
        const float xh = (z4[r] - mu4) * iv4;
        dz4[r] = dzb;                                    // dzb for now; dz4 below
        t0 += dzb;
        t1 += dzb * xh;
        t2 += d * fminf(zb, 0.f);
      }
    }
  }
  if (a.y) {
    const float l = block_sum(loss, red), hsum = block_sum(hits, red);
    if (tid == 0 && a.loss_acc) { a.loss_acc[0] = l / a.denom; a.loss_acc[1] = hsum; }
  }
  if (!grads) return;

  // ---- backward: output layer (BN4 training-mode backward, Linear4) ----
  const float sdb4 = block_sum(t0, red), sdg4 = block_sum(t1, red), sda4 = block_sum(t2, red);
  float sdz = 0.f;
  for (int r = tid; r < B; r += kT) {
    const float xh = (z4[r] - mu4) * iv4;
    dz4[r] = ga4 * iv4 * (dz4[r] - sdb4 * inv_b - xh * sdg4 * inv_b);
    sdz += dz4[r];
  }
  const float db4 = block_sum(sdz, red);              // (its barriers publish dz4)
  if (tid == 0) {
    a.dbeta4[0] = sdb4; a.dgamma4[0] = sdg4; a.dalpha4[0] = sda4; a.db4[0] = db4;
  }
  // dW4[k] = sum_r dz4[r] y3[r, k]; PReLU3 / BN3 backward with dy3[r, j] = dz4[r] w4[j]
  float da3 = 0.f;
  if (j < H) {
    float acc = 0.f;
#pragma unroll 8
    for (int r = 0; r < B; ++r) acc = __builtin_fmaf(dz4[r], y3[(int64_t)r * H + j], acc);
    a.dw4[j] = acc;
    const float w4j = a.w4[j], sc = ga3 * iv3;
    float s0 = 0.f, s1 = 0.f;
#pragma unroll 4
    for (int r = 0; r < B; ++r) {
      const float z = z3[(int64_t)r * H + j];
      const float zb = zb_of(z, mu3, sc, be3);
      const float dy = dz4[r] * w4j;
      const float dzb = zb > 0.f ? dy : al3 * dy;
      s0 += dzb;
      s1 += dzb * ((z - mu3) * iv3);
      da3 += dy * fminf(zb, 0.f);
    }
    a.dbeta3[j] = s0;
    a.dgamma3[j] = s1;
    // dZ3 (over y3, which nobody reads any more) and db3
    float sd = 0.f;
#pragma unroll 4
    for (int r = 0; r < B; ++r) {
      const float z = z3[(int64_t)r * H + j];
      const float zb = zb_of(z, mu3, sc, be3);
      const float dy = dz4[r] * w4j;
      const float dzb = zb > 0.f ? dy : al3 * dy;
      const float d = ga3 * iv3 * (dzb - s0 * inv_b - ((z - mu3) * iv3) * s1 * inv_b);
      y3[(int64_t)r * H + j] = d;
      sd += d;
    }
    a.db3[j] = sd;
  }
  const float da3_sum = block_sum(da3, red);         // (its barriers publish dZ3)
  if (tid == 0) a.dalpha3[0] = da3_sum;
  const float* dz3 = y3;

  // dP = dZ3 W3 (W3 [out, in] is the [h, h] operand of rows_times as it stands)
  if (a.dpooled) rows_times(dz3, H, B, H, a.w3, nullptr, a.dpooled, a.lddp, sa);

  // dW3[j, k] = sum_r dZ3[r, j] P[r, k]: outputs dealt 16 per thread per pass, rows staged in LDS kRB at a time
  constexpr int kPer = 16;
  const int total = H * H;
  for (int o0 = 0; o0 < total; o0 += kT * kPer) {
    float acc[kPer];
#pragma unroll
    for (int m = 0; m < kPer; ++m) acc[m] = 0.f;
    for (int r0 = 0; r0 < B; r0 += kRB) {
      const int nr = min(kRB, B - r0);
      for (int i = tid; i < kRB * H; i += kT) {
        const int r = i / H, k = i - r * H;
        sa[r][k] = r < nr ? a.pooled[(int64_t)(r0 + r) * a.ldp + k] : 0.f;
        sb[r][k] = r < nr ? dz3[(int64_t)(r0 + r) * H + k] : 0.f;
      }
      __syncthreads();
#pragma unroll
      for (int m = 0; m < kPer; ++m) {
        const int o = o0 + m * kT + tid;
        if (o < total) {
          const int jj = o / H, kk = o - jj * H;
          for (int r = 0; r < nr; ++r) acc[m] = __builtin_fmaf(sb[r][jj], sa[r][kk], acc[m]);
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int m = 0; m < kPer; ++m) {
      const int o = o0 + m * kT + tid;
      if (o < total) a.dw3[o] = acc[m];
    }
  }
}

// ---- the same head in seven phases, for a batch sharded by graph over ranks (sync-BN) ----------------------------------
// Phase k works on the local rows, writes its local partial sums to its slice of `red` (PhaseRed below), the caller
// all-reduces that slice, and phase k + 1 reads the global sums back.  The arithmetic and every reduction order are those
// of bce_head_kernel, with the local row loops and the global count in place of b.  Scratch: bce_head_kernel's
// z3 | y3 (dZ3) | W3^T | z4 | dz4, then the moments mu3 [h] | iv3 [h] | mu4 | iv4, kept between the phases.
struct PhaseRed {                                     // offsets into red[4h + 4]
  int z3s, z3v, z4s, z4v, t4, t3;
  __host__ __device__ explicit PhaseRed(int h) : z3s(0), z3v(h), z4s(2 * h), z4v(2 * h + 1), t4(2 * h + 2), t3(2 * h + 4) {}
};

__global__ __launch_bounds__(kT) void bce_head_phase_kernel(gcnx_bce_head_args a, int phase, float count, float* red) {
  __shared__ float sa[kRB][kT];
  __shared__ float sb[kRB][kT];
  __shared__ float rsum[kT];
  const int tid = threadIdx.x, B = a.b, H = a.h, j = tid;
  float* z3 = a.scratch;
  float* y3 = z3 + (int64_t)B * H;
  float* w3t = y3 + (int64_t)B * H;
  float* z4 = w3t + (int64_t)H * H;
  float* dz4 = z4 + B;
  float* mu3 = dz4 + B;
  float* iv3 = mu3 + H;
  float* m4 = iv3 + H;                                // m4[0] = mu4, m4[1] = iv4
  const PhaseRed R(H);
  const float ic = 1.0f / count;

  if (phase == 0) {                                   // z3 = P W3^T + b3; sum z3
    for (int i = tid; i < H * H; i += kT) {
      const int k = i / H, jj = i - k * H;
      w3t[i] = a.w3[(int64_t)jj * H + k];
    }
    __syncthreads();
    rows_times(a.pooled, a.ldp, B, H, w3t, a.b3, z3, H, sa);
    if (j < H) {
      float s = 0.f;
#pragma unroll 8
      for (int r = 0; r < B; ++r) s += z3[(int64_t)r * H + j];
      red[R.z3s + j] = s;
    }
    return;
  }
  if (phase == 1) {                                   // mean3; sum (z3 - mean3)^2
    if (j < H) {
      const float mu = red[R.z3s + j] * ic;
      mu3[j] = mu;
      float v = 0.f;
#pragma unroll 8
      for (int r = 0; r < B; ++r) { const float d = z3[(int64_t)r * H + j] - mu; v = __builtin_fmaf(d, d, v); }
      red[R.z3v + j] = v;
    }
    return;
  }
  if (phase == 2) {                                   // inv3, y3 = PReLU3(BN3(z3)), z4 = y3 W4^T + b4; sum z4
    const float al3 = a.alpha3[0];
    if (j < H) {
      const float mu = mu3[j], iv = 1.0f / sqrtf(red[R.z3v + j] * ic + a.eps);
      iv3[j] = iv;
      const float sc = a.gamma3[j] * iv, be = a.beta3[j];
#pragma unroll 8
      for (int r = 0; r < B; ++r) y3[(int64_t)r * H + j] = prelu1(zb_of(z3[(int64_t)r * H + j], mu, sc, be), al3);
    }
    __syncthreads();
    float s4 = 0.f;
    for (int r = tid; r < B; r += kT) {
      float acc = 0.f;
#pragma unroll 8
      for (int k = 0; k < H; ++k) acc = __builtin_fmaf(y3[(int64_t)r * H + k], a.w4[k], acc);
      z4[r] = acc + a.b4[0];
      s4 += z4[r];
    }
    const float t = block_sum(s4, rsum);
    if (tid == 0) red[R.z4s] = t;
    return;
  }
  if (phase == 3) {                                   // mean4; sum (z4 - mean4)^2
    const float mu = red[R.z4s] * ic;
    float v4 = 0.f;
    for (int r = tid; r < B; r += kT) { const float d = z4[r] - mu; v4 = __builtin_fmaf(d, d, v4); }
    const float t = block_sum(v4, rsum);
    if (tid == 0) { m4[0] = mu; red[R.z4v] = t; }
    return;
  }
  const float mu4 = m4[0];
  const float ga4 = a.gamma4[0], be4 = a.beta4[0], al4 = a.alpha4[0];
  if (phase == 4) {                                   // inv4, out, probs, loss part, hits; the output layer's sums
    const float iv4 = 1.0f / sqrtf(red[R.z4v] * ic + a.eps), sc4 = ga4 * iv4;
    if (tid == 0) m4[1] = iv4;
    const bool grads = a.grads && a.y;
    float loss = 0.f, hits = 0.f, t0 = 0.f, t1 = 0.f, t2 = 0.f;
    for (int r = tid; r < B; r += kT) {
      const float zb = zb_of(z4[r], mu4, sc4, be4);
      const float o = prelu1(zb, al4);
      const float p = 1.0f / (1.0f + expf(-o));
      if (a.out) a.out[r] = o;
      if (a.probs) a.probs[r] = p;
      if (a.y) {
        const float t = a.y[(int64_t)r * a.y_stride + a.y_col];
        loss += fmaxf(o, 0.f) - o * t + log1pf(expf(-fabsf(o)));
        hits += ((o > 0.f) == (t > 0.5f)) ? 1.f : 0.f;
        if (grads) {
          const float d = (p - t) / a.denom;
          const float dzb = zb > 0.f ? d : al4 * d;
          const float xh = (z4[r] - mu4) * iv4;
          dz4[r] = dzb;                                  // dzb for now; dz4 in phase 5
          t0 += dzb;
          t1 += dzb * xh;
          t2 += d * fminf(zb, 0.f);
        }
      }
    }
    if (a.y) {
      const float l = block_sum(loss, rsum), hsum = block_sum(hits, rsum);
      if (tid == 0 && a.loss_acc) { a.loss_acc[0] = l / a.denom; a.loss_acc[1] = hsum; }
    }
    if (!grads) return;
    const float sdb4 = block_sum(t0, rsum), sdg4 = block_sum(t1, rsum), sda4 = block_sum(t2, rsum);
    if (tid == 0) {
      red[R.t4] = sdb4; red[R.t4 + 1] = sdg4;
      a.dbeta4[0] = sdb4; a.dgamma4[0] = sdg4; a.dalpha4[0] = sda4;
    }
    return;
  }
  const float iv4 = m4[1];
  const float al3 = a.alpha3[0];
  const float mu = j < H ? mu3[j] : 0.f, iv = j < H ? iv3[j] : 0.f;
  const float ga3 = j < H ? a.gamma3[j] : 0.f, be3 = j < H ? a.beta3[j] : 0.f, w4j = j < H ? a.w4[j] : 0.f;
  const float sc = ga3 * iv;
  if (phase == 5) {                                   // dz4 (global sums), db4, dW4; BN3 / PReLU3 backward sums
    const float sdb4 = red[R.t4], sdg4 = red[R.t4 + 1];
    float sdz = 0.f;
    for (int r = tid; r < B; r += kT) {
      const float xh = (z4[r] - mu4) * iv4;
      dz4[r] = ga4 * iv4 * (dz4[r] - sdb4 * ic - xh * sdg4 * ic);
      sdz += dz4[r];
    }
    const float db4 = block_sum(sdz, rsum);           // (its barriers publish dz4)
    if (tid == 0) a.db4[0] = db4;
    float da3 = 0.f;
    if (j < H) {
      float acc = 0.f;
#pragma unroll 8
      for (int r = 0; r < B; ++r) acc = __builtin_fmaf(dz4[r], y3[(int64_t)r * H + j], acc);
      a.dw4[j] = acc;
      float s0 = 0.f, s1 = 0.f;
#pragma unroll 4
      for (int r = 0; r < B; ++r) {
        const float z = z3[(int64_t)r * H + j];
        const float zb = zb_of(z, mu, sc, be3);
        const float dy = dz4[r] * w4j;
        const float dzb = zb > 0.f ? dy : al3 * dy;
        s0 += dzb;
        s1 += dzb * ((z - mu) * iv);
        da3 += dy * fminf(zb, 0.f);
      }
      red[R.t3 + j] = s0;
      red[R.t3 + H + j] = s1;
      a.dbeta3[j] = s0;
      a.dgamma3[j] = s1;
    }
    const float da3_sum = block_sum(da3, rsum);
    if (tid == 0) a.dalpha3[0] = da3_sum;
    return;
  }
  // phase 6: dZ3 (over y3) with the global sums, db3, dP = dZ3 W3, dW3 = dZ3^T P
  if (j < H) {
    const float s0 = red[R.t3 + j], s1 = red[R.t3 + H + j];
    float sd = 0.f;
#pragma unroll 4
    for (int r = 0; r < B; ++r) {
      const float z = z3[(int64_t)r * H + j];
      const float zb = zb_of(z, mu, sc, be3);
      const float dy = dz4[r] * w4j;
      const float dzb = zb > 0.f ? dy : al3 * dy;
      const float d = ga3 * iv * (dzb - s0 * ic - ((z - mu) * iv) * s1 * ic);
      y3[(int64_t)r * H + j] = d;
      sd += d;
    }
    a.db3[j] = sd;
  }
  __syncthreads();                                    // publish dZ3
  const float* dz3 = y3;
  if (a.dpooled) rows_times(dz3, H, B, H, a.w3, nullptr, a.dpooled, a.lddp, sa);
  constexpr int kPer = 16;
  const int total = H * H;
  for (int o0 = 0; o0 < total; o0 += kT * kPer) {
    float acc[kPer];
#pragma unroll
    for (int m = 0; m < kPer; ++m) acc[m] = 0.f;
    for (int r0 = 0; r0 < B; r0 += kRB) {
      const int nr = min(kRB, B - r0);
      for (int i = tid; i < kRB * H; i += kT) {
        const int r = i / H, k = i - r * H;
        sa[r][k] = r < nr ? a.pooled[(int64_t)(r0 + r) * a.ldp + k] : 0.f;
        sb[r][k] = r < nr ? dz3[(int64_t)(r0 + r) * H + k] : 0.f;
      }
      __syncthreads();
#pragma unroll
      for (int m = 0; m < kPer; ++m) {
        const int o = o0 + m * kT + tid;
        if (o < total) {
          const int jj = o / H, kk = o - jj * H;
          for (int r = 0; r < nr; ++r) acc[m] = __builtin_fmaf(sb[r][jj], sa[r][kk], acc[m]);
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int m = 0; m < kPer; ++m) {
      const int o = o0 + m * kT + tid;
      if (o < total) a.dw3[o] = acc[m];
    }
  }
}

// The head's argument checks, shared by the one-launch head and its phases (min_b: 2 for the one launch, 1 for a shard).
int check_head_args(gcnx_ctx* ctx, const gcnx_bce_head_args& a, int min_b, int64_t scratch_need, const char* fn) {
  GCNX_REQUIRE(ctx, a.b >= min_b, "%s: BatchNorm needs at least %d rows (b = %d)", fn, min_b, a.b);
  GCNX_REQUIRE(ctx, a.h >= 1, "%s: h = %d", fn, a.h);
  if (a.h > kT) return gcnx_fail(ctx, GCNX_ERR_UNSUPPORTED, "%s: h = %d > 256 is not served", fn, a.h);
  GCNX_REQUIRE(ctx, a.pooled && a.ldp >= a.h && a.w3 && a.b3 && a.gamma3 && a.beta3 && a.alpha3 && a.w4 && a.b4 && a.gamma4 &&
                        a.beta4 && a.alpha4, "%s: NULL input", fn);
  GCNX_REQUIRE(ctx, a.eps > 0.f && (!a.y || a.denom > 0.f), "%s: eps and denom must be positive", fn);
  GCNX_REQUIRE(ctx, !a.y || (a.y_stride >= 1 && a.y_col >= 0 && a.y_col < a.y_stride && a.loss_acc),
               "%s: bad label layout or no loss_acc", fn);
  GCNX_REQUIRE(ctx, !a.grads || a.y, "%s: gradients need labels", fn);
  GCNX_REQUIRE(ctx, !a.grads || (a.dw3 && a.db3 && a.dgamma3 && a.dbeta3 && a.dalpha3 && a.dw4 && a.db4 && a.dgamma4 && a.dbeta4 &&
                                 a.dalpha4 && (!a.dpooled || a.lddp >= a.h)), "%s: NULL gradient output", fn);
  GCNX_REQUIRE(ctx, a.scratch && a.scratch_floats >= scratch_need, "%s: scratch of %lld floats, %lld needed", fn,
               (long long)a.scratch_floats, (long long)scratch_need);
  return GCNX_OK;
}

}  // namespace

extern "C" {

int64_t gcnx_bce_head_scratch_floats(int32_t b, int32_t h) {
  if (b < 0 || h < 0) return 0;
  return 2 * (int64_t)b * h + (int64_t)h * h + 2 * (int64_t)b;
}

int64_t gcnx_bce_head_phase_scratch_floats(int32_t b, int32_t h) {
  if (b < 0 || h < 0) return 0;
  return gcnx_bce_head_scratch_floats(b, h) + 2 * (int64_t)h + 2;
}

int64_t gcnx_bce_head_phase_red_floats(int32_t h) {
  if (h < 0) return 0;
  return 4 * (int64_t)h + 4;
}

int gcnx_bce_head_phase(gcnx_ctx* ctx, const gcnx_bce_head_args* args, int32_t phase, float count, float* red) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "BN-PReLU-BCE head (phase)");
  GCNX_REQUIRE(ctx, args != nullptr, "gcnx_bce_head_phase: args is NULL");
  const gcnx_bce_head_args& a = *args;
  GCNX_REQUIRE(ctx, phase >= 0 && phase <= 6, "gcnx_bce_head_phase: phase %d is not in 0..6", phase);
  GCNX_REQUIRE(ctx, count >= 2.f, "gcnx_bce_head_phase: BatchNorm needs at least 2 rows in the whole batch (count = %g)",
               (double)count);
  GCNX_REQUIRE(ctx, red != nullptr, "gcnx_bce_head_phase: red is NULL");
  int rc = check_head_args(ctx, a, 1, gcnx_bce_head_phase_scratch_floats(a.b, a.h), "gcnx_bce_head_phase");
  if (rc) return rc;
  GCNX_REQUIRE(ctx, a.b <= count, "gcnx_bce_head_phase: %d local rows > count %g", a.b, (double)count);
  GCNX_REQUIRE(ctx, phase < 5 || a.grads, "gcnx_bce_head_phase: phases 5 and 6 are the backward (grads = 0)");
  hipLaunchKernelGGL(bce_head_phase_kernel, dim3(1), dim3(kT), 0, ctx->stream, a, (int)phase, count, red);
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

int gcnx_bn_prelu_bce_head(gcnx_ctx* ctx, const gcnx_bce_head_args* args) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "BN-PReLU-BCE head");
  GCNX_REQUIRE(ctx, args != nullptr, "gcnx_bn_prelu_bce_head: args is NULL");
  const gcnx_bce_head_args& a = *args;
  int rc = check_head_args(ctx, a, 2, gcnx_bce_head_scratch_floats(a.b, a.h), "gcnx_bn_prelu_bce_head");
  if (rc) return rc;
  hipLaunchKernelGGL(bce_head_kernel, dim3(1), dim3(kT), 0, ctx->stream, a);
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

}  // extern "C"
