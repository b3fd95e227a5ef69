// The continuous actor heads as kernels of their own (gfx950), on raw [R, 2A] = [out | std_raw]; the arithmetic of each head is in
// actor_heads.h.  One flat forward and one flat backward, elementwise with one thread per element, serve all three heads; the Normal head
// also has a forward that emits the h2 planes of its action rows.  (The Normal head fused with the policy's output layer is in rowops.hip.)
//
// The Monte-Carlo pair of the squashed head (SampleDist's mean and entropy over K samples, agent/dreamer_utils.py:28-60, and the entropy's
// backward) is a row kernel in the style of discrete.hip: one row on an aligned group of W lanes, lane a holding action dimension a and
// walking the K samples of eps [K, R, A], so that for one k the lanes of a wave read consecutive addresses.  eps is the only stream that
// matters (K R A floats); it is read once per launch and nothing is kept between the forward and the backward but raw.  Per-sample terms
// are summed in double per lane, in the order of k, and the lanes of a row are combined by shuffles in a fixed order: results are
// bit-reproducible.  No allocation, no synchronisation with the host, no atomics.
#include "actor_heads.h"
#include "genrl_hip.h"
#include <math.h>

namespace {

constexpr int MAX_A = 64;                                  // the Monte-Carlo kernels: one action dimension per lane of a wave
constexpr double LOG_2 = 0.6931471805599453, HALF_LOG_2PI = 0.9189385332046727;

// action [R, ld_action], mean / std [R, A] (any may be null); eps [R, A], null: the mode
template <typename Head>
__global__ void head_fwd_kernel(const float* __restrict__ raw, const float* __restrict__ eps, float* __restrict__ action,
                                float* __restrict__ mean_out, float* __restrict__ std_out, long n, int A, float p0, float p1,
                                long ld_action) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long r = i / A;
  const int a = (int)(i % A);
  const Head h(raw[r * 2 * A + a], raw[r * 2 * A + A + a], p0, p1);
  if (action) action[r * ld_action + a] = h.action(eps ? eps[i] : 0.f, eps != nullptr);
  if (mean_out) mean_out[i] = h.mean;
  if (std_out) std_out[i] = h.std;
}

template <typename Head>
__global__ void head_bwd_kernel(const float* __restrict__ daction, const float* __restrict__ raw, const float* __restrict__ eps,
                                float* __restrict__ draw, long n, int A, float p0, float p1, long ld_action) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long r = i / A;
  const int a = (int)(i % A);
  const Head h(raw[r * 2 * A + a], raw[r * 2 * A + A + a], p0, p1);
  h.backward(daction[r * ld_action + a], eps[i], draw[r * 2 * A + a], draw[r * 2 * A + A + a]);
}

// the Normal head with an h2-plane copy of the action rows: one thread per row (A ~ 10: the row maximum is a loop)
__global__ void actor_head_fwd_rows_kernel(const float* __restrict__ raw, const float* __restrict__ eps,
                                           float* __restrict__ action, float* __restrict__ mean_out,
                                           float* __restrict__ std_out, long R, int A, float min_std,
                                           float max_std, long ld_action, PlaneOut xo) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  float amax = 0.f;
  for (int a = 0; a < A; ++a) {
    const NormalHead h(raw[r * 2 * A + a], raw[r * 2 * A + A + a], min_std, max_std);
    const float act = h.action(eps ? eps[r * A + a] : 0.f, eps != nullptr);
    amax = fmaxf(amax, fabsf(act));
    action[r * ld_action + a] = act;
    if (mean_out) mean_out[r * A + a] = h.mean;
    if (std_out) std_out[r * A + a] = h.std;
  }
  const float inv = h2_inv_of(amax), sc = h2_scale_of(inv);
  xo.inv[r] = inv;
  for (int a = 0; a < A; ++a) h2_store1(xo, r * xo.ld + a, action[r * ld_action + a], sc);
}

// log |d tanh(x) / dx| = 2 (log 2 - x - softplus(-2x)) (TanhTransform.log_abs_det_jacobian).  x < -10: softplus(-2x) = -2x, the value is
// 2 (log 2 + x); large x: exp(-2x) = 0, the value is 2 (log 2 - x).  Never inf for a finite x
__device__ __forceinline__ double ladj(float x) { return 2.0 * (LOG_2 - (double)x - (double)softplusf_(-2.0f * x)); }

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
    const TanhNormalHead h(raw[r * 2 * A + a], raw[r * 2 * A + A + a], min_std, init_std);
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
  const TanhNormalHead h(raw[r * 2 * A + a], raw[r * 2 * A + A + a], min_std, init_std);
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

inline bool bad_width(int A) { return A < 1 || A > MAX_A; }

// the flat launches (ld_action already resolved); R A > 0
template <typename Head>
int head_fwd(const float* raw, const float* eps, float* action, float* mean, float* std, long n, int A, float p0, float p1,
             long ld_action, void* stream) {
  head_fwd_kernel<Head><<<cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(raw, eps, action, mean, std, n, A, p0, p1, ld_action);
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}
template <typename Head>
int head_bwd(const float* daction, const float* raw, const float* eps, float* draw, long n, int A, float p0, float p1, long ld_action,
             void* stream) {
  head_bwd_kernel<Head><<<cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(daction, raw, eps, draw, n, A, p0, p1, ld_action);
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

int actor_head_fwd_impl(const float* raw, const float* eps, float* action, float* mean, float* std, long R, int A, float min_std,
                        float max_std, long ld_action, PlaneOut xo, void* stream) {
  GENRL_ENTER();
  const long n = R * A;
  if (n <= 0) return GENRL_OK;
  if (xo.p && (xo.ld < A || !xo.inv || !action)) return GENRL_EINVAL;
  if (ld_action <= 0) ld_action = A;
  if (!xo.p) return head_fwd<NormalHead>(raw, eps, action, mean, std, n, A, min_std, max_std, ld_action, stream);
  hipLaunchKernelGGL(actor_head_fwd_rows_kernel, dim3(cdiv(R, 64)), dim3(64), 0, (hipStream_t)stream, raw, eps, action, mean, std, R, A,
                     min_std, max_std, ld_action, xo);
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

}  // namespace

extern "C" {

int genrl_actor_head_fwd(const float* raw, const float* eps, float* action, float* mean, float* std, long R, int A,
                         float min_std, float max_std, long ld_action, void* stream) {
  return actor_head_fwd_impl(raw, eps, action, mean, std, R, A, min_std, max_std, ld_action, PlaneOut{nullptr, 0, 0, nullptr}, stream);
}
/* + the action as x3 planes (rows ldp wide; the columns >= A must have been zeroed by the caller once) */
int genrl_actor_head_fwd_h2(const float* raw, const float* eps, float* action, float* mean, float* std, long R, int A,
                            float min_std, float max_std, long ld_action, uint16_t* ap, long ldp, long plane, float* inv, void* stream) {
  return actor_head_fwd_impl(raw, eps, action, mean, std, R, A, min_std, max_std, ld_action, PlaneOut{ap, ldp, plane, inv}, stream);
}

int genrl_actor_head_bwd(const float* daction, const float* raw, const float* eps, float* draw, long R, int A,
                         float min_std, float max_std, long ld_action, void* stream) {
  GENRL_ENTER();
  const long n = R * A;
  if (n <= 0) return GENRL_OK;
  return head_bwd<NormalHead>(daction, raw, eps, draw, n, A, min_std, max_std, ld_action > 0 ? ld_action : (long)A, stream);
}

int genrl_trunc_normal_head_fwd(const float* raw, const float* eps, float* action, float* mean, float* std, long R, int A,
                                float min_std, float init_std, long ld_action, void* stream) {
  GENRL_ENTER();
  if (R <= 0) return GENRL_OK;
  if (A <= 0 || !raw || (!action && !mean && !std)) return GENRL_EINVAL;
  if (ld_action == 0) ld_action = A;
  if (ld_action < A) return GENRL_EINVAL;
  return head_fwd<TruncNormalHead>(raw, eps, action, mean, std, R * A, A, min_std, init_std, ld_action, stream);
}

int genrl_trunc_normal_head_bwd(const float* daction, const float* raw, const float* eps, float* draw, long R, int A, float init_std,
                                long ld_action, void* stream) {
  GENRL_ENTER();
  if (R <= 0) return GENRL_OK;
  if (A <= 0 || !daction || !raw || !eps || !draw) return GENRL_EINVAL;
  if (ld_action == 0) ld_action = A;
  if (ld_action < A) return GENRL_EINVAL;
  return head_bwd<TruncNormalHead>(daction, raw, eps, draw, R * A, A, 0.f, init_std, ld_action, stream);      // (min_std: not in the gradient)
}

int genrl_tanh_normal_head_fwd(const float* raw, const float* eps, float* action, float* mean, float* std, long R, int A,
                               float min_std, float init_std, long ld_action, void* stream) {
  GENRL_ENTER();
  if (bad_width(A) || R < 0 || !raw || (!action && !mean && !std)) return GENRL_EINVAL;
  if (ld_action == 0) ld_action = A;
  if (ld_action < A) return GENRL_EINVAL;
  if (R == 0) return GENRL_OK;
  return head_fwd<TanhNormalHead>(raw, eps, action, mean, std, R * A, A, min_std, init_std, ld_action, stream);
}

int genrl_tanh_normal_head_bwd(const float* daction, const float* raw, const float* eps, float* draw, long R, int A, float min_std,
                               float init_std, long ld_action, void* stream) {
  GENRL_ENTER();
  if (bad_width(A) || R < 0 || !daction || !raw || !eps || !draw) return GENRL_EINVAL;
  if (ld_action == 0) ld_action = A;
  if (ld_action < A) return GENRL_EINVAL;
  if (R == 0) return GENRL_OK;
  return head_bwd<TanhNormalHead>(daction, raw, eps, draw, R * A, A, min_std, init_std, ld_action, stream);
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
