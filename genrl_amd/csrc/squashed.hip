// The squashed-Gaussian policy head (gfx950): DistLayer 'tanh_normal' (agent/dreamer_utils.py:824-829), SquashedNormal (tools/utils.py:126-170)
// wrapped in SampleDist (agent/dreamer_utils.py:28-60) on raw [R, 2A] = [out | std_raw]:
//   mean = 5 tanh(out / 5), std = softplus(std_raw + init_std) + min_std (torch's softplus: the identity above 20),
//   x = mean + std eps, action = tanh(x).
// The head pair is elementwise, one thread per element, like the truncated-normal head of normfree.hip.  The Monte-Carlo pair (SampleDist's
// mean and entropy over K samples, and the entropy's backward) is a row kernel in the style of discrete.hip: one row on an aligned group of
// W lanes, lane a holding action dimension a and walking the K samples of eps [K, R, A], so that for one k the lanes of a wave read
// consecutive addresses.  eps is the only stream that matters (K R A floats); it is read once per launch and nothing is kept between the
// forward and the backward but raw.  Per-sample terms are summed in double per lane, in the order of k, and the lanes of a row are combined
// by shuffles in a fixed order: results are bit-reproducible.  No allocation, no synchronisation with the host, no atomics.
#include "common.h"
#include "genrl_hip.h"
#include <math.h>
#include <type_traits>

namespace {

constexpr int MAX_A = 64;                                  // one action dimension per lane of a wave
constexpr double LOG_2 = 0.6931471805599453, HALF_LOG_2PI = 0.9189385332046727;

// torch.nn.functional.softplus (beta 1, threshold 20) and its derivative
__device__ __forceinline__ float softplusf_(float z) { return z > 20.0f ? z : log1pf(expf(z)); }
__device__ __forceinline__ float dsoftplusf_(float z) { return z > 20.0f ? 1.0f : sigmoidf_(z); }

struct Row {              // one element of the head from raw
  float th, mean, z, std;         // th = tanh(out / 5), mean = 5 th, z = std_raw + init_std, std = softplus(z) + min_std
  __device__ __forceinline__ Row(const float* __restrict__ raw, long r, int a, int A, float min_std, float init_std) {
    th = tanhf(raw[r * 2 * A + a] / 5.0f);
    mean = 5.0f * th;
    z = raw[r * 2 * A + A + a] + init_std;
    std = softplusf_(z) + min_std;
  }
  // d mean / d out and d std / d std_raw
  __device__ __forceinline__ float dmean() const { return 1.0f - th * th; }
  __device__ __forceinline__ float dstd() const { return dsoftplusf_(z); }
};

// log |d tanh(x) / dx| = 2 (log 2 - x - softplus(-2x)) (TanhTransform.log_abs_det_jacobian).  x < -10: softplus(-2x) = -2x, the value is
// 2 (log 2 + x); large x: exp(-2x) = 0, the value is 2 (log 2 - x).  Never inf for a finite x
__device__ __forceinline__ double ladj(float x) { return 2.0 * (LOG_2 - (double)x - (double)softplusf_(-2.0f * x)); }

template <int W>
__device__ __forceinline__ double group_sum_d(double v) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// eps == NULL: the mean form, action = tanh(mean)
__global__ void sq_head_fwd_kernel(const float* __restrict__ raw, const float* __restrict__ eps, float* __restrict__ action,
                                   float* __restrict__ mean_out, float* __restrict__ std_out, long n, int A, float min_std,
                                   float init_std, long ld_action) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long r = i / A;
  const int a = (int)(i % A);
  const Row h(raw, r, a, A, min_std, init_std);
  if (action) action[r * ld_action + a] = tanhf(eps ? h.mean + h.std * eps[i] : h.mean);
  if (mean_out) mean_out[i] = h.mean;
  if (std_out) std_out[i] = h.std;
}

// dx = daction (1 - action^2); d mean = dx, d std = dx eps; then through 5 tanh(. / 5) and the softplus
__global__ void sq_head_bwd_kernel(const float* __restrict__ daction, const float* __restrict__ raw, const float* __restrict__ eps,
                                   float* __restrict__ draw, long n, int A, float min_std, float init_std, long ld_action) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long r = i / A;
  const int a = (int)(i % A);
  const Row h(raw, r, a, A, min_std, init_std);
  const float e = eps[i];
  const float t = tanhf(h.mean + h.std * e);
  const float dx = daction[r * ld_action + a] * (1.0f - t * t);
  draw[r * 2 * A + a] = dx * h.dmean();
  draw[r * 2 * A + A + a] = dx * e * h.dstd();
}

// ent[r] = sum_a ( mean_k(eps^2 / 2 + ladj(x_ka)) + log std_a + log(2 pi) / 2 ) = -mean_k log_prob(sample_k): with x = mean + std eps the
// quadratic term of the Normal's log-density is eps^2 / 2.  mean_action[r, a] = mean_k tanh(x_ka).  Either output may be null
template <int W>
__global__ __launch_bounds__(256) void sq_mc_fwd_kernel(const float* __restrict__ raw, const float* __restrict__ eps,
                                                        float* __restrict__ ent, float* __restrict__ mean_action, long R, int A, int K,
                                                        float min_std, float init_std) {
  const long r = ((long)blockIdx.x * 256 + threadIdx.x) / W;
  const int a = threadIdx.x % W;
  const bool valid = (r < R) && (a < A);
  double term = 0.0;
  if (valid) {
    const Row h(raw, r, a, A, min_std, init_std);
    const float* e = eps + r * A + a;
    const long step = R * A;
    double st = 0.0, se = 0.0;
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
      const float ev = e[k * step];
      const float x = h.mean + h.std * ev;
      if (mean_action) st += (double)tanhf(x);
      if (ent) se += 0.5 * (double)ev * (double)ev + ladj(x);
    }
    if (mean_action) mean_action[r * A + a] = (float)(st / K);
    term = se / K + (double)logf(h.std) + HALF_LOG_2PI;
  }
  if (!ent) return;
  const double s = group_sum_d<W>(term);
  if (valid && a == 0) ent[r] = (float)s;
}

// d ent / d mean_a = mean_k(-2 tanh x_ka), d ent / d std_a = 1 / std_a + mean_k(-2 tanh(x_ka) eps_ka) (the quadratic term cancels), then
// through the head; draw (+)= gent[r] times that.  No reduction across lanes
template <int W>
__global__ __launch_bounds__(256) void sq_ent_bwd_kernel(const float* __restrict__ gent, const float* __restrict__ raw,
                                                         const float* __restrict__ eps, float* __restrict__ draw, long R, int A, int K,
                                                         float min_std, float init_std, int accumulate) {
  const long r = ((long)blockIdx.x * 256 + threadIdx.x) / W;
  const int a = threadIdx.x % W;
  if (r >= R || a >= A) return;
  const Row h(raw, r, a, A, min_std, init_std);
  const float* e = eps + r * A + a;
  const long step = R * A;
  double st = 0.0, se = 0.0;
#pragma unroll 4
  for (int k = 0; k < K; ++k) {
    const float ev = e[k * step];
    const double t = (double)tanhf(h.mean + h.std * ev);
    st += t;
    se += t * (double)ev;
  }
  const double g = (double)gent[r];
  const float dm = (float)(g * (-2.0 * st / K) * (double)h.dmean());
  const float ds = (float)(g * (1.0 / (double)h.std - 2.0 * se / K) * (double)h.dstd());
  float* d = draw + r * 2 * A;
  d[a] = accumulate ? d[a] + dm : dm;
  d[A + a] = accumulate ? d[A + a] + ds : ds;
}

template <typename F>
int dispatch_w(int A, F&& f) {
  if (A <= 4) return f(std::integral_constant<int, 4>{});
  if (A <= 8) return f(std::integral_constant<int, 8>{});
  if (A <= 16) return f(std::integral_constant<int, 16>{});
  if (A <= 32) return f(std::integral_constant<int, 32>{});
  return f(std::integral_constant<int, 64>{});
}

inline bool bad_width(int A) { return A < 1 || A > MAX_A; }

}  // namespace

extern "C" {

int genrl_tanh_normal_head_fwd(const float* raw, const float* eps, float* action, float* mean, float* std, long R, int A,
                               float min_std, float init_std, long ld_action, void* stream) {
  GENRL_ENTER();
  if (bad_width(A) || R < 0 || !raw || (!action && !mean && !std)) return GENRL_EINVAL;
  if (ld_action == 0) ld_action = A;
  if (ld_action < A) return GENRL_EINVAL;
  if (R == 0) return GENRL_OK;
  const long n = R * A;
  sq_head_fwd_kernel<<<cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(raw, eps, action, mean, std, n, A, min_std, init_std, ld_action);
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

int genrl_tanh_normal_head_bwd(const float* daction, const float* raw, const float* eps, float* draw, long R, int A, float min_std,
                               float init_std, long ld_action, void* stream) {
  GENRL_ENTER();
  if (bad_width(A) || R < 0 || !daction || !raw || !eps || !draw) return GENRL_EINVAL;
  if (ld_action == 0) ld_action = A;
  if (ld_action < A) return GENRL_EINVAL;
  if (R == 0) return GENRL_OK;
  const long n = R * A;
  sq_head_bwd_kernel<<<cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(daction, raw, eps, draw, n, A, min_std, init_std, ld_action);
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

int genrl_tanh_normal_mc_fwd(const float* raw, const float* eps, float* ent, float* mean_action, long R, int A, int K, float min_std,
                             float init_std, void* stream) {
  GENRL_ENTER();
  if (bad_width(A) || K < 1 || R < 0 || !raw || !eps || (!ent && !mean_action)) return GENRL_EINVAL;
  if (R == 0) return GENRL_OK;
  return dispatch_w(A, [&](auto w) {
    constexpr int W = decltype(w)::value;
    hipLaunchKernelGGL((sq_mc_fwd_kernel<W>), dim3(cdiv(R * W, 256)), dim3(256), 0, (hipStream_t)stream, raw, eps, ent, mean_action, R,
                       A, K, min_std, init_std);
    GENRL_CHECK_LAUNCH();
    return GENRL_OK;
  });
}

int genrl_tanh_normal_ent_bwd(const float* gent, const float* raw, const float* eps, float* draw, long R, int A, int K, float min_std,
                              float init_std, int accumulate, void* stream) {
  GENRL_ENTER();
  if (bad_width(A) || K < 1 || R < 0 || !gent || !raw || !eps || !draw) return GENRL_EINVAL;
  if (R == 0) return GENRL_OK;
  return dispatch_w(A, [&](auto w) {
    constexpr int W = decltype(w)::value;
    hipLaunchKernelGGL((sq_ent_bwd_kernel<W>), dim3(cdiv(R * W, 256)), dim3(256), 0, (hipStream_t)stream, gent, raw, eps, draw, R, A,
                       K, min_std, init_std, accumulate);
    GENRL_CHECK_LAUNCH();
    return GENRL_OK;
  });
}

}  // extern "C"
