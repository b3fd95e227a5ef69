// The learned discount of `pred_discount: True` (gfx950): the binary head's log-likelihood, the imagined discounts with their
// cumulative weights, and the lambda-return scan on a discount per step and column.  The reference's head is Bernoulli(logits = z)
// with z = sigmoid(x) (DistLayer 'binary', agent/dreamer_utils.py:820-823, hands the sigmoid to BernoulliDist's first parameter,
// `logits`, :199-201): its mean is sigmoid(sigmoid(x)).  That arithmetic is restated here, not mended.  Elementwise / one thread per
// column, coalesced over N, fp32, every output element written.
#include "common.h"
#include <math.h>

namespace {

// sigmoid(x) and 1 - sigmoid(x), each from the one exponential that cannot overflow: both keep their relative accuracy at either end
__device__ __forceinline__ void sigmoid_pair(float x, float& s, float& oms) {
  const float e = expf(-fabsf(x));
  const float big = 1.0f / (1.0f + e), small = e / (1.0f + e);
  s = x >= 0.f ? big : small;
  oms = x >= 0.f ? small : big;
}

// like = t z - softplus(z), z = sigmoid(x)   (Independent(Bernoulli(logits = z), 1).log_prob on a one-wide event)
__global__ void binary_like_fwd_kernel(const float* __restrict__ x, const float* __restrict__ target, float* __restrict__ like, long R) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= R) return;
  float z, omz;
  sigmoid_pair(x[i], z, omz);
  like[i] = target[i] * z - log1pf(expf(z));          // (z lies in [0, 1]: no overflow)
}
// dx = glike (t - sigmoid(z)) z (1 - z)
__global__ void binary_like_bwd_kernel(const float* __restrict__ x, const float* __restrict__ target, const float* __restrict__ glike,
                                       float* __restrict__ dx, long R) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= R) return;
  float z, omz, p, omp;
  sigmoid_pair(x[i], z, omz);
  sigmoid_pair(z, p, omp);
  dx[i] = glike[i] * (target[i] - p) * (z * omz);
}

// WorldModel.imagine, agent/dreamer.py:274-286: p[t] = the head's mean, row 0 replaced by 1 - is_terminal of the start states;
// disc = gamma p; weight = cumprod(cat(1, p[:-1])), multiplied in time order.  One thread walks its column.
__global__ void imag_discount_fwd_kernel(const float* __restrict__ x, const float* __restrict__ term, int H1, long N, float gamma,
                                         float* __restrict__ disc, float* __restrict__ weight) {
  const long n = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float w = 1.0f;
  for (int t = 0; t < H1; ++t) {
    float p;
    if (t == 0 && term) {
      p = 1.0f - term[n];
    } else {
      float z, omz, omp;
      sigmoid_pair(x[(long)t * N + n], z, omz);
      sigmoid_pair(z, p, omp);
    }
    disc[(long)t * N + n] = gamma * p;
    weight[(long)t * N + n] = w;
    w = w * p;
  }
}
// dx = gdisc gamma p (1 - p) z (1 - z); row 0 is the replay buffer's flag when `term` was given: exactly zero
__global__ void imag_discount_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gdisc, int term_given, long N, long total,
                                         float gamma, float* __restrict__ dx) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  if (term_given && i < N) {
    dx[i] = 0.f;
    return;
  }
  float z, omz, p, omp;
  sigmoid_pair(x[i], z, omz);
  sigmoid_pair(z, p, omp);
  dx[i] = gdisc[i] * gamma * (p * omp) * (z * omz);
}

// lambda_return with a tensor pcont (agent/dreamer_utils.py:228-253): R_t = r_t + d_t ((1 - lam) v_{t+1} + lam R_{t+1}), R_H = v_H.
// Expression for expression the scalar kernel of dist.hip with its `disc` read per element: equal discounts give equal bits.
__global__ void lambda_return_disc_fwd_kernel(const float* __restrict__ reward, const float* __restrict__ value,
                                              const float* __restrict__ disc, float* __restrict__ ret, int H, long N, float lam) {
  const long n = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float agg = value[(long)H * N + n];
  for (int t = H - 1; t >= 0; --t) {
    const float d = disc[(long)t * N + n];
    const float inp = reward[(long)t * N + n] + d * value[(long)(t + 1) * N + n] * (1.0f - lam);
    agg = inp + d * lam * agg;
    ret[(long)t * N + n] = agg;
  }
}
// a_t = g_t + d_{t-1} lam a_{t-1}; dr_t = a_t; dd_t = a_t ((1 - lam) v_{t+1} + lam R_{t+1}); dv_{t+1} = d_t (1 - lam) a_t, the bootstrap
// row d_{H-1} a_{H-1}; dv_0 = 0
__global__ void lambda_return_disc_bwd_kernel(const float* __restrict__ gret, const float* __restrict__ value, const float* __restrict__ disc,
                                              const float* __restrict__ ret, float* __restrict__ dreward, float* __restrict__ dvalue,
                                              float* __restrict__ ddisc, int H, long N, float lam, int zero_tail) {
  const long n = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float a = 0.f, dprev = 0.f;
  dvalue[n] = 0.f;
  if (zero_tail) {                 // reward and disc carry an (unread) row H: its gradient is zero
    dreward[(long)H * N + n] = 0.f;
    ddisc[(long)H * N + n] = 0.f;
  }
  for (int t = 0; t < H; ++t) {
    const float d = disc[(long)t * N + n];
    a = gret[(long)t * N + n] + dprev * lam * a;
    dreward[(long)t * N + n] = a;
    const float vn = value[(long)(t + 1) * N + n];
    const float rn = (t == H - 1) ? vn : ret[(long)(t + 1) * N + n];
    ddisc[(long)t * N + n] = a * ((1.0f - lam) * vn + lam * rn);
    dvalue[(long)(t + 1) * N + n] = (t == H - 1) ? d * a : d * (1.0f - lam) * a;
    dprev = d;
  }
}

}  // namespace

extern "C" {

int genrl_binary_like_fwd(const float* x, const float* target, float* like, long R, void* stream) {
  GENRL_ENTER();
  if (R < 1 || !x || !target || !like) return GENRL_EINVAL;
  hipLaunchKernelGGL(binary_like_fwd_kernel, dim3(cdiv(R, 256)), dim3(256), 0, (hipStream_t)stream, x, target, like, R);
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

int genrl_binary_like_bwd(const float* x, const float* target, const float* glike, float* dx, long R, void* stream) {
  GENRL_ENTER();
  if (R < 1 || !x || !target || !glike || !dx) return GENRL_EINVAL;
  hipLaunchKernelGGL(binary_like_bwd_kernel, dim3(cdiv(R, 256)), dim3(256), 0, (hipStream_t)stream, x, target, glike, dx, R);
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

int genrl_imag_discount_fwd(const float* x, const float* term, int H1, long N, float gamma, float* disc, float* weight, void* stream) {
  GENRL_ENTER();
  if (H1 < 1 || N < 1 || !x || !disc || !weight) return GENRL_EINVAL;
  hipLaunchKernelGGL(imag_discount_fwd_kernel, dim3(cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, x, term, H1, N, gamma, disc,
                     weight);
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

int genrl_imag_discount_bwd(const float* x, const float* gdisc, int term_given, int H1, long N, float gamma, float* dx, void* stream) {
  GENRL_ENTER();
  if (H1 < 1 || N < 1 || !x || !gdisc || !dx) return GENRL_EINVAL;
  const long total = (long)H1 * N;
  hipLaunchKernelGGL(imag_discount_bwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, x, gdisc, term_given, N, total,
                     gamma, dx);
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

int genrl_lambda_return_disc_fwd(const float* reward, const float* value, const float* disc, float* ret, int H, long N, float lam,
                                 void* stream) {
  GENRL_ENTER();
  if (H < 1 || N < 1 || !reward || !value || !disc || !ret) return GENRL_EINVAL;
  hipLaunchKernelGGL(lambda_return_disc_fwd_kernel, dim3(cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, reward, value, disc, ret, H,
                     N, lam);
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

int genrl_lambda_return_disc_bwd(const float* gret, const float* value, const float* disc, const float* ret, float* dreward,
                                 float* dvalue, float* ddisc, int H, long N, float lam, int zero_tail, void* stream) {
  GENRL_ENTER();
  if (H < 1 || N < 1 || !gret || !value || !disc || !ret || !dreward || !dvalue || !ddisc) return GENRL_EINVAL;
  hipLaunchKernelGGL(lambda_return_disc_bwd_kernel, dim3(cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, gret, value, disc, ret,
                     dreward, dvalue, ddisc, H, N, lam, zero_tail);
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

}  // extern "C"
