// Optimizers with state over the flat parameter / gradient buffers of a model: Adam / AdamW in torch's
// form, Keras SGD with momentum (the reference's optimizer class, gcn.py:325), both with torch's clip_grad_norm_ in front.
//
// A step is   gcnx_counter_add(t)  ->  [gcnx_grad_sqnorm]  ->  gcnx_adam | gcnx_sgd_momentum   on one stream: the step count
// t and the clip factor never leave the device, so a captured step replays as it is.
//
// The norm, in a FIXED order (no atomics: an eager call and a replay give the same bits).  gcnx_grad_sqnorm launches
// n_partials workgroups of 256 threads.  Thread j of workgroup b adds the fp32 squares g[i] * g[i] (rounded, no fma) of
// i = 256 b + j, + 256 n_partials, ... in ascending order from +0.f; the 64 lanes of a wave fold with lane += lane + off,
// off = 32, 16, 8, 4, 2, 1; wave 0's lane 0 adds the four wave sums as ((s0 + s1) + s2) + s3: partials[b].  The update launch
// folds the partials the same way in EVERY workgroup: thread j holds partials[j] (+0.f past n_partials), then the same six
// lane steps and the same three additions -- no third launch, no host read.  Longest addition chain:
// ceil(n / (256 n_partials)) + 9 + 9.
#include <cstdint>

#include "common.h"

namespace {

constexpr int kOptimMaxPartials = GCNX_OPTIM_MAX_PARTIALS;   // one per thread of the update launch's workgroups
constexpr int kOptimMaxBlocks = 512;                         // grid cap of the update launches (threads loop past it)

// Sum over the 256 threads of a workgroup in the order given above; every thread returns the total.
__device__ __forceinline__ float block_sum_256(float x, float* s4) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = __fadd_rn(x, __shfl_down(x, off));
  if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = x;
  __syncthreads();
  return __fadd_rn(__fadd_rn(__fadd_rn(s4[0], s4[1]), s4[2]), s4[3]);
}

__global__ __launch_bounds__(256) void grad_sqnorm_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ partials) {
  __shared__ float s4[4];
  float acc = 0.f;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const float x = g[i];
    acc = __fadd_rn(acc, __fmul_rn(x, x));
  }
  const float tot = block_sum_256(acc, s4);
  if (threadIdx.x == 0) partials[blockIdx.x] = tot;
}

// sqrt(sum of the partials), in every workgroup alike; block 0 leaves it in norm_out.  Returns the clip factor
// min(1, clipnorm / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_), formed once per thread in fp64 from the fp32 norm.
__device__ __forceinline__ double clip_factor(const float* __restrict__ partials, int n_partials, float clipnorm,
                                             float* __restrict__ norm_out, float* s4) {
  if (partials == nullptr) return 1.0;                       // (uniform: a kernel argument)
  const float mine = (int)threadIdx.x < n_partials ? partials[threadIdx.x] : 0.f;
  const float norm = sqrtf(block_sum_256(mine, s4));
  if (norm_out != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *norm_out = norm;
  if (!(clipnorm > 0.f)) return 1.0;
  const double s = (double)clipnorm / ((double)norm + 1e-6);
  return s < 1.0 ? s : 1.0;
}

__device__ __forceinline__ double pow_u32(double b, uint32_t t) {   // b^t by squaring, fp64
  double r = 1.0;
  for (; t; t >>= 1, b *= b)
    if (t & 1u) r *= b;
  return r;
}

struct AdamCoef {
  float s, s_lo, decay, b1, omb1, omb1_lo, b2, omb2, step, rs2, eps;   // decay = lr * weight_decay; step = lr / (1 - b1^t); rs2 = sqrt(1 - b2^t)
};

// One element, fp32.  m = b1 m + (1 - b1) g' cancels where the gradient turns against the running mean, and the update
// divides by sqrt(v): a rounding of either product would then show in p at many times 2^-24 of the update.  So the
// second product is carried as a pair hi + lo (lo = the fma residual; s and 1 - b1 carry the fp32 remainder of their fp64
// value too), the first is exact inside the fma, and m ends within 2 * 2^-24 of ITSELF.  v sums non-negative terms (one fma);
// the parameter takes ONE rounding of its own: p - (decay p + update).
__device__ __forceinline__ void adam_elem(const AdamCoef& c, float& p, float g, float& m, float& v) {
  const float gs = c.s * g;
  const float gs_lo = fmaf(c.s, g, -gs) + c.s_lo * g;
  const float w = c.omb1 * gs;
  const float w_lo = fmaf(c.omb1, gs, -w) + (c.omb1 * gs_lo + c.omb1_lo * gs);
  m = fmaf(c.b1, m, w) + w_lo;
  v = fmaf(c.omb2, gs * gs, c.b2 * v);
  const float upd = c.step * (m / (sqrtf(v) / c.rs2 + c.eps));
  p = p - fmaf(c.decay, p, upd);                       // (decay == 0: p - upd, bit for bit)
}

template <bool VEC>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, int64_t n, const uint32_t* __restrict__ t_dev, float lr_arg,
                                                   const float* __restrict__ lr_dev, float beta1, float beta2, float eps,
                                                   float weight_decay, const float* __restrict__ partials, int n_partials,
                                                   float clipnorm, float* __restrict__ norm_out) {
  __shared__ float s4[4];
  const float lr = lr_dev ? *lr_dev : lr_arg;            // (gcnx_set_lr_source)
  uint32_t t = *t_dev;                                   // advanced for this step by an earlier launch (gcnx_counter_add)
  if (t == 0u) t = 1u;
  AdamCoef c;
  const double s = clip_factor(partials, n_partials, clipnorm, norm_out, s4);
  c.s = (float)s; c.s_lo = (float)(s - (double)c.s);
  // the bias corrections in fp64 from the fp32 betas (1 - 0.999f^1 in fp32 has already lost five digits), once per thread
  const double bc1 = 1.0 - pow_u32((double)beta1, t), bc2 = 1.0 - pow_u32((double)beta2, t);
  c.decay = lr * weight_decay;
  c.b1 = beta1; c.omb1 = 1.f - beta1; c.b2 = beta2; c.omb2 = 1.f - beta2;
  c.omb1_lo = (float)((1.0 - (double)beta1) - (double)c.omb1);   // (0 for beta1 >= 0.5: the fp32 difference is exact)
  c.step = lr / (float)bc1;
  c.rs2 = (float)sqrt(bc2);
  c.eps = eps;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
  if (VEC) {
    const int64_t n4 = n >> 2;
    for (int64_t i = tid; i < n4; i += stride) {
      float4 pp = reinterpret_cast<float4*>(p)[i], mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
      const float4 gg = reinterpret_cast<const float4*>(g)[i];
      adam_elem(c, pp.x, gg.x, mm.x, vv.x); adam_elem(c, pp.y, gg.y, mm.y, vv.y);
      adam_elem(c, pp.z, gg.z, mm.z, vv.z); adam_elem(c, pp.w, gg.w, mm.w, vv.w);
      reinterpret_cast<float4*>(p)[i] = pp; reinterpret_cast<float4*>(m)[i] = mm; reinterpret_cast<float4*>(v)[i] = vv;
    }
    const int64_t i = (n4 << 2) + tid;                   // the tail of at most 3 elements
    if (i < n) adam_elem(c, p[i], g[i], m[i], v[i]);
  } else {
    for (int64_t i = tid; i < n; i += stride) adam_elem(c, p[i], g[i], m[i], v[i]);
  }
}

// Keras SGD(momentum, nesterov): vel = momentum vel - lr g'; p += vel, or with Nesterov p += momentum vel - lr g'.
// An element is formed in fp64 from the fp32 operands and rounded ONCE per stored value: vel, and with Nesterov p (which
// reads the stored vel, as Keras does).  With the products rounded in fp32 the Nesterov form collects (1 + momentum) roundings
// of lr g' twice over and misses 3 * 2^-24 (|p| + |vel| + |lr g'|); the kernel is bound by its 20 B per element either way.
__device__ __forceinline__ void momentum_elem(double s, double lr, double mom, bool nesterov, float& p, float g, float& vel) {
  const double step = lr * (s * (double)g);
  vel = (float)(mom * (double)vel - step);
  p = nesterov ? (float)((double)p + (mom * (double)vel - step)) : p + vel;
}

template <bool VEC>
__global__ __launch_bounds__(256) void sgd_momentum_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ vel,
                                                           int64_t n, float lr_arg, const float* __restrict__ lr_dev, float mom,
                                                           int nesterov, const float* __restrict__ partials, int n_partials,
                                                           float clipnorm, float* __restrict__ norm_out) {
  __shared__ float s4[4];
  const float lr = lr_dev ? *lr_dev : lr_arg;            // (gcnx_set_lr_source)
  const double s = clip_factor(partials, n_partials, clipnorm, norm_out, s4);
  const bool nes = nesterov != 0;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
  if (VEC) {
    const int64_t n4 = n >> 2;
    for (int64_t i = tid; i < n4; i += stride) {
      float4 pp = reinterpret_cast<float4*>(p)[i], vv = reinterpret_cast<float4*>(vel)[i];
      const float4 gg = reinterpret_cast<const float4*>(g)[i];
      momentum_elem(s, lr, mom, nes, pp.x, gg.x, vv.x); momentum_elem(s, lr, mom, nes, pp.y, gg.y, vv.y);
      momentum_elem(s, lr, mom, nes, pp.z, gg.z, vv.z); momentum_elem(s, lr, mom, nes, pp.w, gg.w, vv.w);
      reinterpret_cast<float4*>(p)[i] = pp; reinterpret_cast<float4*>(vel)[i] = vv;
    }
    const int64_t i = (n4 << 2) + tid;
    if (i < n) momentum_elem(s, lr, mom, nes, p[i], g[i], vel[i]);
  } else {
    for (int64_t i = tid; i < n; i += stride) momentum_elem(s, lr, mom, nes, p[i], g[i], vel[i]);
  }
}

int update_grid(int64_t n, bool vec) {
  const int64_t work = vec ? (n >> 2) + 3 : n;           // (+ 3: the tail's threads)
  const int64_t g = (work + 255) / 256;
  return (int)(g > kOptimMaxBlocks ? kOptimMaxBlocks : g);
}

}  // namespace

extern "C" {

int gcnx_grad_sqnorm(gcnx_ctx* ctx, const float* g, int64_t n, float* partials, int32_t n_partials) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "gradient norm (partials)");
  GCNX_REQUIRE(ctx, n >= 0, "gcnx_grad_sqnorm: negative size");
  GCNX_REQUIRE(ctx, n_partials >= 1 && n_partials <= kOptimMaxPartials, "gcnx_grad_sqnorm: n_partials %d outside [1, %d]",
               (int)n_partials, kOptimMaxPartials);
  if (n == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, g && partials, "gcnx_grad_sqnorm: NULL pointer");
  hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(n_partials), dim3(256), 0, ctx->stream, g, n, partials);
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

// the clip arguments of both update launches
static int check_clip(gcnx_ctx* ctx, const char* who, const float* partials, int32_t n_partials, float clipnorm) {
  GCNX_REQUIRE(ctx, n_partials >= 0 && n_partials <= kOptimMaxPartials, "%s: n_partials %d outside [0, %d]", who, (int)n_partials,
               kOptimMaxPartials);
  GCNX_REQUIRE(ctx, !(clipnorm > 0.f) || (partials && n_partials >= 1), "%s: clipnorm needs the partials of gcnx_grad_sqnorm", who);
  GCNX_REQUIRE(ctx, !partials || n_partials >= 1, "%s: partials without a count", who);
  return GCNX_OK;
}

int gcnx_adam(gcnx_ctx* ctx, float* p, const float* g, float* m, float* v, int64_t n, const uint32_t* t_dev, float lr, float beta1,
              float beta2, float eps, float weight_decay, const float* partials, int32_t n_partials, float clipnorm, float* norm_out) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "Adam update");
  GCNX_REQUIRE(ctx, n >= 0, "gcnx_adam: negative size");
  GCNX_REQUIRE(ctx, beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "gcnx_adam: betas (%g, %g) outside [0, 1)", (double)beta1,
               (double)beta2);
  if (int rc = check_clip(ctx, "gcnx_adam", partials, n_partials, clipnorm)) return rc;
  if (n == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, p && g && m && v && t_dev, "gcnx_adam: NULL pointer");
  const bool vec = gcnx_aligned16(p) && gcnx_aligned16(g) && gcnx_aligned16(m) && gcnx_aligned16(v);
  const dim3 grid(update_grid(n, vec));
  if (vec)
    hipLaunchKernelGGL((adam_kernel<true>), grid, dim3(256), 0, ctx->stream, p, g, m, v, n, t_dev, lr, ctx->lr_dev, beta1, beta2, eps,
                       weight_decay, partials, (int)n_partials, clipnorm, norm_out);
  else
    hipLaunchKernelGGL((adam_kernel<false>), grid, dim3(256), 0, ctx->stream, p, g, m, v, n, t_dev, lr, ctx->lr_dev, beta1, beta2, eps,
                       weight_decay, partials, (int)n_partials, clipnorm, norm_out);
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

int gcnx_sgd_momentum(gcnx_ctx* ctx, float* p, const float* g, float* vel, int64_t n, float lr, float momentum, int nesterov,
                      const float* partials, int32_t n_partials, float clipnorm, float* norm_out) {
  GCNX_CHECK_CTX(ctx);
  GCNX_RANGE(ctx, "SGD momentum update");
  GCNX_REQUIRE(ctx, n >= 0, "gcnx_sgd_momentum: negative size");
  GCNX_REQUIRE(ctx, momentum >= 0.f && momentum < 1.f, "gcnx_sgd_momentum: momentum %g outside [0, 1)", (double)momentum);
  if (int rc = check_clip(ctx, "gcnx_sgd_momentum", partials, n_partials, clipnorm)) return rc;
  if (n == 0) return GCNX_OK;
  GCNX_REQUIRE(ctx, p && g && vel, "gcnx_sgd_momentum: NULL pointer");
  const bool vec = gcnx_aligned16(p) && gcnx_aligned16(g) && gcnx_aligned16(vel);
  const dim3 grid(update_grid(n, vec));
  if (vec)
    hipLaunchKernelGGL((sgd_momentum_kernel<true>), grid, dim3(256), 0, ctx->stream, p, g, vel, n, lr, ctx->lr_dev, momentum, nesterov,
                       partials, (int)n_partials, clipnorm, norm_out);
  else
    hipLaunchKernelGGL((sgd_momentum_kernel<false>), grid, dim3(256), 0, ctx->stream, p, g, vel, n, lr, ctx->lr_dev, momentum, nesterov,
                       partials, (int)n_partials, clipnorm, norm_out);
  GCNX_LAUNCH_OK(ctx);
  return GCNX_OK;
}

}  // extern "C"
