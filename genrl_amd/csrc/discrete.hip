// Discrete-action policy kernels (gfx950): the log-probability and entropy of the actor's unimix one-hot head
// (DistLayer 'onehot' -> OneHotDist, agent/dreamer_utils.py:177-197, :835-836) and the REINFORCE actor objective
// (agent/dreamer.py:392-429, actor_grad 'reinforce').  Bandwidth-bound row kernels in the style of dist.hip / stats.hip: one
// categorical of K classes per aligned group of W lanes reduced with shuffles; the objective is one workgroup with a fixed
// summation order and double accumulation.  No allocation, no synchronisation with the host, no atomics.
#include "common.h"
#include <math.h>

namespace {

// ---- one categorical of K classes held by an aligned group of W lanes ----
// p = softmax(l); u = (1 - mix) p + mix / K; pn = u / sum(u) (torch's Categorical(probs=) renormalises; sum(u) is 1 up to rounding);
// lg = log(clamp(pn, eps, 1 - eps)) (probs_to_logits), what OneHotCategorical.log_prob gathers and .entropy multiplies with pn
template <int W>
struct MixCat {
  float p, pn, s, lg;
  bool inside;            // pn strictly inside the clamp: d lg / d pn = 1 / pn there, 0 on the clamp
  __device__ __forceinline__ void init(float logit, bool valid, int K, float mix) {
    const float eps = 1.1920928955078125e-07f;            // torch.finfo(float32).eps
    const float l = valid ? logit : -INFINITY;
    const float m = group_max<W>(l);
    const float e = valid ? expf(l - m) : 0.f;
    const float z = group_sum<W>(e);
    p = e / z;
    const float u = valid ? (1.0f - mix) * p + mix / K : 0.f;
    s = group_sum<W>(u);
    pn = u / s;
    inside = valid && pn > eps && pn < 1.0f - eps;
    lg = valid ? logf(fminf(fmaxf(pn, eps), 1.0f - eps)) : 0.f;
  }
  // g = dL/dpn (per class) -> dL/dlogit, through the renormalisation, the mix and the softmax
  __device__ __forceinline__ float backward(float g, bool valid, float mix) const {
    const float gi = valid ? g : 0.f;
    const float dot = group_sum<W>(gi * pn);
    const float dp = (1.0f - mix) * ((gi - dot) / s);
    const float dot2 = group_sum<W>(valid ? dp * p : 0.f);
    return valid ? p * (dp - dot2) : 0.f;
  }
};

// logp[g] = sum_k action[g,k] lg[g,k];  ent[g] = -sum_k pn[g,k] lg[g,k]   (either output may be null)
template <int W>
__global__ __launch_bounds__(256) void logp_ent_fwd_kernel(const float* __restrict__ logits, const float* __restrict__ action,
                                                           float* __restrict__ logp, float* __restrict__ ent, long G, int K,
                                                           float mix) {
  const long g = ((long)blockIdx.x * 256 + threadIdx.x) / W;
  const int k = threadIdx.x % W;
  const bool valid = (g < G) && (k < K);
  const long gi = g < G ? g : G - 1;
  MixCat<W> c;
  c.init(valid ? logits[gi * K + k] : 0.f, valid, K, mix);
  const float a = (valid && logp) ? action[gi * K + k] : 0.f;
  const float lp = group_sum<W>(valid ? a * c.lg : 0.f);
  const float en = group_sum<W>(valid ? c.pn * c.lg : 0.f);
  if (g < G && k == 0) {
    if (logp) logp[g] = lp;
    if (ent) ent[g] = -en;
  }
}

// dlogits (+)= glogp[g] d logp / d logits + gent[g] d ent / d logits   (glogp or gent may be null)
template <int W>
__global__ __launch_bounds__(256) void logp_ent_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ action,
                                                           const float* __restrict__ glogp, const float* __restrict__ gent,
                                                           float* __restrict__ dlogits, long G, int K, float mix, int accumulate) {
  const long g = ((long)blockIdx.x * 256 + threadIdx.x) / W;
  const int k = threadIdx.x % W;
  const bool valid = (g < G) && (k < K);
  const long gi = g < G ? g : G - 1;
  MixCat<W> c;
  c.init(valid ? logits[gi * K + k] : 0.f, valid, K, mix);
  float gp = 0.f;
  if (valid) {
    const float dlg = c.inside ? 1.0f / c.pn : 0.f;
    if (glogp) gp += glogp[gi] * action[gi * K + k] * dlg;
    if (gent) gp -= gent[gi] * (c.lg + c.pn * dlg);
  }
  const float d = c.backward(gp, valid, mix);
  if (valid) dlogits[gi * K + k] = accumulate ? dlogits[gi * K + k] + d : d;
}

// ---- REINFORCE objective on lambda-returns (agent/dreamer.py:400-429, actor_grad 'reinforce') ----
//   nt = (target - offset) / scale, nb = (baseline - offset) / scale   [H, N]  (os == null: offset 0, scale 1);
//   loss = -mean_{h >= 1}( weight[h-1] (logp[h-1] (nt[h] - nb[h]) + ent_scale ent[h-1]) )
// out[0], out[1] = mean, unbiased std of nt over all H*N (the 'normed_target_*' metrics; written only with os).
constexpr int NT = 1024;

__device__ __forceinline__ float advantage(float t, float b, const float* os) {
  return os ? (t - os[0]) / os[1] - (b - os[0]) / os[1] : t - b;
}

__global__ __launch_bounds__(NT) void reinforce_obj_fwd_kernel(const float* __restrict__ target, const float* __restrict__ baseline,
                                                                const float* __restrict__ logp, const float* __restrict__ ent,
                                                                const float* __restrict__ weight, const float* __restrict__ os,
                                                                float ent_scale, int H, long N, float* __restrict__ loss,
                                                                float* __restrict__ out) {
  __shared__ double red[16];
  double l = 0.0, s = 0.0, q = 0.0;
  const long n = (long)H * N;
  for (long i = threadIdx.x; i < n; i += NT) {
    if (os) {
      const float v = (target[i] - os[0]) / os[1];
      s += v; q += (double)v * v;
    }
    if (i >= N) {
      const long j = i - N;
      float obj = logp[j] * advantage(target[i], baseline[i], os);
      if (ent) obj += ent_scale * ent[j];
      l += (double)(weight ? weight[j] : 1.0f) * obj;
    }
  }
  l = block_sum_d(l, red);
  if (os) { s = block_sum_d(s, red); q = block_sum_d(q, red); }
  if (threadIdx.x == 0) {
    loss[0] = (float)(-l / ((double)(H - 1) * N));
    if (os && out) {
      const double mean = s / n;
      out[0] = (float)mean;
      out[1] = (float)sqrt(fmax((q - n * mean * mean) / (n - 1), 0.0));
    }
  }
}

// from the scalar gradient g: dlogp, dent [H-1, N]; dtarget, dbaseline [H, N] with row 0 zero (any output may be null)
__global__ __launch_bounds__(256) void reinforce_obj_bwd_kernel(const float* __restrict__ g, const float* __restrict__ target,
                                                                const float* __restrict__ baseline, const float* __restrict__ logp,
                                                                const float* __restrict__ weight, const float* __restrict__ os,
                                                                float ent_scale, int H, long N, float* __restrict__ dlogp,
                                                                float* __restrict__ dtarget, float* __restrict__ dbaseline,
                                                                float* __restrict__ dent) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)H * N) return;
  if (i < N) {
    if (dtarget) dtarget[i] = 0.f;
    if (dbaseline) dbaseline[i] = 0.f;
    return;
  }
  const long j = i - N;
  const float c = -g[0] * (weight ? weight[j] : 1.0f) / (float)((double)(H - 1) * N);
  if (dlogp) dlogp[j] = c * advantage(target[i], baseline[i], os);
  if (dent) dent[j] = c * ent_scale;
  const float dt = os ? c * logp[j] / os[1] : c * logp[j];
  if (dtarget) dtarget[i] = dt;
  if (dbaseline) dbaseline[i] = -dt;
}

}  // namespace

extern "C" {

int genrl_onehot_logp_ent_fwd(const float* logits, const float* action, float* logp, float* ent, long G, int K, float unimix,
                              void* stream) {
  GENRL_ENTER();
  if (K < 2 || K > 64 || G < 0 || !logits || (logp && !action) || (!logp && !ent)) return GENRL_EINVAL;
  if (G == 0) return GENRL_OK;
  return dispatch_w(K, [&](auto w) {
    constexpr int W = decltype(w)::value;
    hipLaunchKernelGGL((logp_ent_fwd_kernel<W>), dim3(cdiv(G * W, 256)), dim3(256), 0, (hipStream_t)stream, logits, action, logp,
                       ent, G, K, unimix);
    GENRL_CHECK_LAUNCH();
    return GENRL_OK;
  });
}

int genrl_onehot_logp_ent_bwd(const float* logits, const float* action, const float* glogp, const float* gent, float* dlogits,
                              long G, int K, float unimix, int accumulate, void* stream) {
  GENRL_ENTER();
  if (K < 2 || K > 64 || G < 0 || !logits || !dlogits || (glogp && !action) || (!glogp && !gent)) return GENRL_EINVAL;
  if (G == 0) return GENRL_OK;
  return dispatch_w(K, [&](auto w) {
    constexpr int W = decltype(w)::value;
    hipLaunchKernelGGL((logp_ent_bwd_kernel<W>), dim3(cdiv(G * W, 256)), dim3(256), 0, (hipStream_t)stream, logits, action, glogp,
                       gent, dlogits, G, K, unimix, accumulate);
    GENRL_CHECK_LAUNCH();
    return GENRL_OK;
  });
}

int genrl_reinforce_obj_fwd(const float* target, const float* baseline, const float* logp, const float* ent, const float* weight,
                            const float* offset_scale, float ent_scale, int H, long N, float* loss, float* out, void* stream) {
  GENRL_ENTER();
  if (H < 2 || N <= 0 || !target || !baseline || !logp || !loss || (!ent && ent_scale != 0.f) || (offset_scale && !out))
    return GENRL_EINVAL;
  hipLaunchKernelGGL(reinforce_obj_fwd_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, target, baseline, logp, ent, weight,
                     offset_scale, ent_scale, H, N, loss, out);
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

int genrl_reinforce_obj_bwd(const float* g, const float* target, const float* baseline, const float* logp, const float* weight,
                            const float* offset_scale, float ent_scale, int H, long N, float* dlogp, float* dtarget,
                            float* dbaseline, float* dent, void* stream) {
  GENRL_ENTER();
  if (H < 2 || N <= 0 || !g || !target || !baseline || !logp) return GENRL_EINVAL;
  hipLaunchKernelGGL(reinforce_obj_bwd_kernel, dim3(cdiv((long)H * N, 256)), dim3(256), 0, (hipStream_t)stream, g, target, baseline,
                     logp, weight, offset_scale, ent_scale, H, N, dlogp, dtarget, dbaseline, dent);
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

}  // extern "C"
