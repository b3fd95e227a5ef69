// Continuous (Gaussian) RSSM latents (gfx950): the sufficient-statistics head of EnsembleRSSM._suff_stats_layer with `discrete: False`
// (agent/dreamer_utils.py:513-521) fused with the reparameterised sample of get_dist (:416-419), and the Normal-Normal KL of
// EnsembleRSSM.kl_loss (:534-555; torch's kl_normal_normal under Independent(., 1)) with the entropies of both sides, each with its
// backward.  Bandwidth-bound row kernels: the head pair walks rows grid-strided with one 256-thread workgroup per row, as the activations of
// rowact.hip do, with 16-byte accesses where pointers, S and pitches allow and scalar ones otherwise (the std half of a row starts
// at column S: 8-byte aligned only for S = 30); the KL puts a row on an aligned group of W lanes that stride over S and combine with
// shuffles in a fixed order, as the categorical kernels of dist.hip / discrete.hip do.  No allocation, no synchronisation with the host,
// no atomics.
#include "common.h"
#include "genrl_hip.h"
#include <math.h>

namespace {

constexpr int GS_GRID = 2048;          // workgroups at most: rows are grid-strided
enum { ACT_SOFTPLUS = 0, ACT_SIGMOID = 1, ACT_SIGMOID2 = 2 };

// the std activation before `+ min_std`
template <int ACT>
__device__ __forceinline__ float std_act(float x) {
  if (ACT == ACT_SOFTPLUS) return softplusf_(x);
  if (ACT == ACT_SIGMOID) return sigmoidf_(x);
  return 2.0f * sigmoidf_(0.5f * x);
}
// sigmoid'(x) = e / (1 + e)^2 with e = exp(-|x|): no 1 - sigmoid(x) cancellation in the saturated tails
__device__ __forceinline__ float dsigmoidf_(float x) {
  const float e = expf(-fabsf(x)), d = 1.0f + e;
  return e / (d * d);
}
template <int ACT>
__device__ __forceinline__ float dstd_act(float x) {
  if (ACT == ACT_SOFTPLUS) {
    if (x > 20.0f) return 1.0f;
    const float e = expf(-fabsf(x));            // sigmoid(x) from the small exponential on either side
    return (x >= 0.f ? 1.0f : e) / (1.0f + e);
  }
  if (ACT == ACT_SIGMOID) return dsigmoidf_(x);
  return dsigmoidf_(0.5f * x);                  // d/dx 2 sigmoid(x / 2)
}

template <int ACT>
__device__ __forceinline__ void head_elem(float m, float x, float e, bool has_eps, float min_std, float& sd, float& st) {
  sd = std_act<ACT>(x) + min_std;
  st = has_eps ? m + sd * e : m;
}

// raw[R, ldr] = [mean | std_raw]: mean, std = act(std_raw) + min_std, stoch = mean + std eps (eps null: stoch = mean); outputs [R, S]
template <int ACT, bool VEC>
__global__ __launch_bounds__(256) void gauss_head_fwd_kernel(const float* __restrict__ raw, long ldr, const float* __restrict__ eps,
                                                             float* __restrict__ mean, float* __restrict__ std,
                                                             float* __restrict__ stoch, long R, int S, float min_std) {
  for (long row = blockIdx.x; row < R; row += gridDim.x) {
    const float* rr = raw + row * ldr;
    const long o = row * S;
    if (VEC) {
      for (int j = 4 * threadIdx.x; j < S; j += 4 * 256) {
        const float4 m = ld4(rr + j), x = ld4(rr + S + j);
        const float4 e = eps ? ld4(eps + o + j) : float4{0.f, 0.f, 0.f, 0.f};
        float4 sd, st;
        head_elem<ACT>(m.x, x.x, e.x, eps != nullptr, min_std, sd.x, st.x);
        head_elem<ACT>(m.y, x.y, e.y, eps != nullptr, min_std, sd.y, st.y);
        head_elem<ACT>(m.z, x.z, e.z, eps != nullptr, min_std, sd.z, st.z);
        head_elem<ACT>(m.w, x.w, e.w, eps != nullptr, min_std, sd.w, st.w);
        if (mean) st4(mean + o + j, m);
        if (std) st4(std + o + j, sd);
        if (stoch) st4(stoch + o + j, st);
      }
    } else {
      for (int j = threadIdx.x; j < S; j += 256) {
        const float m = rr[j];
        float sd, st;
        head_elem<ACT>(m, rr[S + j], eps ? eps[o + j] : 0.f, eps != nullptr, min_std, sd, st);
        if (mean) mean[o + j] = m;
        if (std) std[o + j] = sd;
        if (stoch) stoch[o + j] = st;
      }
    }
  }
}

// draw[:, :S] (+)= dstoch + dmean; draw[:, S:2S] (+)= (dstoch eps + dstd) act'(std_raw)   (an absent gradient is zero)
template <int ACT, bool VEC>
__global__ __launch_bounds__(256) void gauss_head_bwd_kernel(const float* __restrict__ dstoch, const float* __restrict__ dmean,
                                                             const float* __restrict__ dstd, const float* __restrict__ raw, long ldr,
                                                             const float* __restrict__ eps, float* __restrict__ draw, long lddr, long R,
                                                             int S, int accumulate) {
  const bool se = dstoch && eps;
  for (long row = blockIdx.x; row < R; row += gridDim.x) {
    const float* xr = raw + row * ldr + S;
    float* dr = draw + row * lddr;
    const long o = row * S;
    if (VEC) {
      const float4 z = {0.f, 0.f, 0.f, 0.f};
      for (int j = 4 * threadIdx.x; j < S; j += 4 * 256) {
        const float4 gs = dstoch ? ld4(dstoch + o + j) : z, gm = dmean ? ld4(dmean + o + j) : z;
        const float4 gd = dstd ? ld4(dstd + o + j) : z, e = se ? ld4(eps + o + j) : z, x = ld4(xr + j);
        float4 a = {gs.x + gm.x, gs.y + gm.y, gs.z + gm.z, gs.w + gm.w};
        float4 b = {(gs.x * e.x + gd.x) * dstd_act<ACT>(x.x), (gs.y * e.y + gd.y) * dstd_act<ACT>(x.y),
                    (gs.z * e.z + gd.z) * dstd_act<ACT>(x.z), (gs.w * e.w + gd.w) * dstd_act<ACT>(x.w)};
        if (accumulate) {
          const float4 pa = ld4(dr + j), pb = ld4(dr + S + j);
          a.x += pa.x; a.y += pa.y; a.z += pa.z; a.w += pa.w;
          b.x += pb.x; b.y += pb.y; b.z += pb.z; b.w += pb.w;
        }
        st4(dr + j, a);
        st4(dr + S + j, b);
      }
    } else {
      for (int j = threadIdx.x; j < S; j += 256) {
        const float gs = dstoch ? dstoch[o + j] : 0.f;
        float a = gs + (dmean ? dmean[o + j] : 0.f);
        float b = ((se ? gs * eps[o + j] : 0.f) + (dstd ? dstd[o + j] : 0.f)) * dstd_act<ACT>(xr[j]);
        if (accumulate) { a += dr[j]; b += dr[S + j]; }
        dr[j] = a;
        dr[S + j] = b;
      }
    }
  }
}

// ---- Normal-Normal KL: one row per aligned group of W lanes; double arithmetic and accumulation, fixed order
// kl[m] = sum_s 0.5 (v + t - 1 - log v), v = (std_l / std_r)^2, t = ((mean_l - mean_r) / std_r)^2;
// ent_x[m] = sum_s (0.5 + 0.5 log 2 pi + log std_x)   (any output may be null)
template <int W>
__global__ __launch_bounds__(256) void gauss_kl_fwd_kernel(const float* __restrict__ ml, const float* __restrict__ sl,
                                                           const float* __restrict__ mr, const float* __restrict__ sr,
                                                           float* __restrict__ kl, float* __restrict__ ent_l, float* __restrict__ ent_r,
                                                           long R, int S) {
  const long g = ((long)blockIdx.x * 256 + threadIdx.x) / W;
  const int lane = threadIdx.x % W;
  const long base = (g < R ? g : R - 1) * S;        // (a group past the end re-reads the last row and stores nothing)
  double k = 0.0, el = 0.0, er = 0.0;
  for (int s = lane; s < S; s += W) {
    const long i = base + s;
    // (double throughout: a row of an entropy can cancel to far below its terms, and a KL row of equal distributions to zero; the
    // kernel moves 16 bytes per element and has the arithmetic to spare)
    if (kl) {
      const double b = sr[i], r = sl[i] / b, d = ((double)ml[i] - mr[i]) / b;
      const double v = r * r;
      k += 0.5 * (v + d * d - 1.0 - log(v));
    }
    if (ent_l) el += log((double)sl[i]);
    if (ent_r) er += log((double)sr[i]);
  }
  k = group_sum_d<W>(k);
  if (ent_l) el = group_sum_d<W>(el);
  if (ent_r) er = group_sum_d<W>(er);
  if (g < R && lane == 0) {
    const double c = 0.5 + 0.5 * 1.8378770664093454835606594728112;      // 0.5 + 0.5 log(2 pi)
    if (kl) kl[g] = (float)k;
    if (ent_l) ent_l[g] = (float)(S * c + el);
    if (ent_r) ent_r[g] = (float)(S * c + er);
  }
}

// elementwise: d kl / d (mean_l, std_l) scaled by gp[row], d kl / d (mean_r, std_r) by gq[row]
__global__ __launch_bounds__(256) void gauss_kl_bwd_kernel(const float* __restrict__ ml, const float* __restrict__ sl,
                                                           const float* __restrict__ mr, const float* __restrict__ sr,
                                                           const float* __restrict__ gp, const float* __restrict__ gq,
                                                           float* __restrict__ dml, float* __restrict__ dsl, float* __restrict__ dmr,
                                                           float* __restrict__ dsr, long n, int S) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long row = i / S;
  const double a = sl[i], b = sr[i], d = (double)ml[i] - mr[i];         // (double, as the forward: one rounding per result)
  const double ib = 1.0 / b, ib2 = ib * ib;
  if (dml || dsl) {
    const double g = gp[row];
    if (dml) dml[i] = (float)(g * (d * ib2));
    if (dsl) dsl[i] = (float)(g * (a * ib2 - 1.0 / a));
  }
  if (dmr || dsr) {
    const double g = gq[row];
    if (dmr) dmr[i] = (float)(-g * (d * ib2));
    if (dsr) dsr[i] = (float)(g * (ib - (a * a + d * d) * (ib2 * ib)));
  }
}

template <typename F>
int dispatch_act(int act, F&& f) {
  if (act == ACT_SOFTPLUS) return f(std::integral_constant<int, ACT_SOFTPLUS>{});
  if (act == ACT_SIGMOID) return f(std::integral_constant<int, ACT_SIGMOID>{});
  return f(std::integral_constant<int, ACT_SIGMOID2>{});
}

inline bool bad_act(int act) { return act != ACT_SOFTPLUS && act != ACT_SIGMOID && act != ACT_SIGMOID2; }
inline bool vec_ok(const void* p) { return !p || aligned16(p); }
constexpr int GS_MAX_S = 1 << 20;

}  // namespace

extern "C" {

int genrl_gauss_head_fwd(const float* raw, long ldr, const float* eps, float* mean, float* std, float* stoch, long R, int S,
                         int std_act, float min_std, void* stream) {
  GENRL_ENTER();
  if (R < 0 || S <= 0 || S > GS_MAX_S || ldr < 2L * S || !raw || (!mean && !std && !stoch) || bad_act(std_act)) return GENRL_EINVAL;
  if (R == 0) return GENRL_OK;
  const bool vec = (S & 3) == 0 && (ldr & 3) == 0 && aligned16(raw) && vec_ok(eps) && vec_ok(mean) && vec_ok(std) && vec_ok(stoch);
  return dispatch_act(std_act, [&](auto a) {
    constexpr int ACT = decltype(a)::value;
    if (vec)
      hipLaunchKernelGGL((gauss_head_fwd_kernel<ACT, true>), dim3(row_grid(R, GS_GRID)), dim3(256), 0, (hipStream_t)stream, raw, ldr, eps, mean,
                         std, stoch, R, S, min_std);
    else
      hipLaunchKernelGGL((gauss_head_fwd_kernel<ACT, false>), dim3(row_grid(R, GS_GRID)), dim3(256), 0, (hipStream_t)stream, raw, ldr, eps, mean,
                         std, stoch, R, S, min_std);
    GENRL_CHECK_LAUNCH();
    return GENRL_OK;
  });
}

int genrl_gauss_head_bwd(const float* dstoch, const float* dmean, const float* dstd, const float* raw, long ldr, const float* eps,
                         float* draw, long lddr, long R, int S, int std_act, int accumulate, void* stream) {
  GENRL_ENTER();
  if (R < 0 || S <= 0 || S > GS_MAX_S || ldr < 2L * S || lddr < 2L * S || !raw || !draw || (!dstoch && !dmean && !dstd) ||
      bad_act(std_act))
    return GENRL_EINVAL;
  if (R == 0) return GENRL_OK;
  const bool vec = (S & 3) == 0 && (ldr & 3) == 0 && (lddr & 3) == 0 && aligned16(raw) && aligned16(draw) && vec_ok(eps) &&
                   vec_ok(dstoch) && vec_ok(dmean) && vec_ok(dstd);
  return dispatch_act(std_act, [&](auto a) {
    constexpr int ACT = decltype(a)::value;
    if (vec)
      hipLaunchKernelGGL((gauss_head_bwd_kernel<ACT, true>), dim3(row_grid(R, GS_GRID)), dim3(256), 0, (hipStream_t)stream, dstoch, dmean, dstd,
                         raw, ldr, eps, draw, lddr, R, S, accumulate);
    else
      hipLaunchKernelGGL((gauss_head_bwd_kernel<ACT, false>), dim3(row_grid(R, GS_GRID)), dim3(256), 0, (hipStream_t)stream, dstoch, dmean, dstd,
                         raw, ldr, eps, draw, lddr, R, S, accumulate);
    GENRL_CHECK_LAUNCH();
    return GENRL_OK;
  });
}

int genrl_gauss_kl_fwd(const float* mean_l, const float* std_l, const float* mean_r, const float* std_r, float* kl, float* ent_l,
                       float* ent_r, long R, int S, void* stream) {
  GENRL_ENTER();
  if (R < 0 || S <= 0 || S > GS_MAX_S || (!kl && !ent_l && !ent_r) || (kl && (!mean_l || !std_l || !mean_r || !std_r)) ||
      (ent_l && !std_l) || (ent_r && !std_r))
    return GENRL_EINVAL;
  if (R == 0) return GENRL_OK;
  return dispatch_w(S, [&](auto w) {
    constexpr int W = decltype(w)::value;
    hipLaunchKernelGGL((gauss_kl_fwd_kernel<W>), dim3(cdiv(R * W, 256)), dim3(256), 0, (hipStream_t)stream, mean_l, std_l, mean_r,
                       std_r, kl, ent_l, ent_r, R, S);
    GENRL_CHECK_LAUNCH();
    return GENRL_OK;
  });
}

int genrl_gauss_kl_bwd(const float* mean_l, const float* std_l, const float* mean_r, const float* std_r, const float* gp,
                       const float* gq, float* dmean_l, float* dstd_l, float* dmean_r, float* dstd_r, long R, int S, void* stream) {
  GENRL_ENTER();
  const bool left = dmean_l || dstd_l, right = dmean_r || dstd_r;
  if (R < 0 || S <= 0 || S > GS_MAX_S || !mean_l || !std_l || !mean_r || !std_r || (!left && !right) || (left && !gp) || (right && !gq))
    return GENRL_EINVAL;
  if (R == 0) return GENRL_OK;
  const long n = R * S;
  hipLaunchKernelGGL(gauss_kl_bwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, mean_l, std_l, mean_r, std_r, gp, gq,
                     dmean_l, dstd_l, dmean_r, dstd_r, n, S);
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

}  // extern "C"
