// Small statistics of the actor-critic update (gfx950): the pieces the reference gets from a dozen torch reductions and a
// sort each -- StreamNorm's moments (agent/dreamer_utils.py:934-1001), RewardEMA's quantile EMA (:1014-1029), the
// return-normalised actor objective (agent/dreamer.py:392-429), weighted means of per-row losses (:431-438, :229-243)
// and the policy-entropy metric -- as one launch each.  All are reductions over <= a few 10^5 floats (H x N returns):
// one workgroup of 1024 threads, fixed summation order (deterministic), double accumulation.
#include "actor_heads.h"
#include <algorithm>
#include <math.h>

namespace {

constexpr int NT = 1024;

// out[0..3] = mean, unbiased std, mean |x|, mean x^2
__global__ __launch_bounds__(NT) void moments_kernel(const float* __restrict__ x, long n, float* __restrict__ out) {
  __shared__ double red[16];
  double s = 0.0, q = 0.0, a = 0.0;
  for (long i = threadIdx.x; i < n; i += NT) {
    const double v = x[i];
    s += v; q += v * v; a += fabs(v);
  }
  s = block_sum_d(s, red); q = block_sum_d(q, red); a = block_sum_d(a, red);
  if (threadIdx.x == 0) {
    const double mean = s / n;
    const double var = n > 1 ? fmax((q - n * mean * mean) / (n - 1), 0.0) : NAN;      // torch.std: correction 1
    out[0] = (float)mean; out[1] = (float)sqrt(var); out[2] = (float)(a / n); out[3] = (float)(q / n);
  }
}

// order-preserving map float -> uint32
__device__ __forceinline__ unsigned key_of(float f) {
  const unsigned u = __builtin_bit_cast(unsigned, f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float val_of(unsigned k) {
  const unsigned u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
  return __builtin_bit_cast(float, u);
}

// torch.quantile(x, [q0, q1]) (linear interpolation) by MSB-first radix select of the four order statistics it reads,
// then ema = alpha * quantile + (1 - alpha) * ema in place and (offset, scale) = (ema[0], max(ema[1] - ema[0], 1)).
// One workgroup; four rounds of 8 bits, each one pass over x with a 256-bin histogram per wanted rank.
__global__ __launch_bounds__(NT) void quantile_ema_kernel(const float* __restrict__ x, long n, float q0, float q1,
                                                           float alpha, float* __restrict__ ema,
                                                           float* __restrict__ out /* offset, scale, quantile0, quantile1 */) {
  __shared__ unsigned hist[4][256];
  __shared__ unsigned prefix[4];
  __shared__ long rank[4];
  __shared__ float wgt[2];
  __shared__ int slot[4], nslot;          // ranks whose prefixes coincide (floor / ceil of one quantile, all four in round 0) share a histogram
  if (threadIdx.x == 0) {
    // torch: ranks = q * (n - 1) in float32; below = floor, above = ceil, weight = ranks - below
    const float r0 = q0 * (float)(n - 1), r1 = q1 * (float)(n - 1);
    rank[0] = (long)floorf(r0); rank[1] = (long)ceilf(r0); rank[2] = (long)floorf(r1); rank[3] = (long)ceilf(r1);
    wgt[0] = r0 - floorf(r0); wgt[1] = r1 - floorf(r1);
    for (int s = 0; s < 4; ++s) prefix[s] = 0u;
  }
  // the keys stay in registers when they fit (n <= 16 per thread: the 16 x 1024 lambda-returns of the headline size): x is read once
  constexpr int KPT = 16;
  const bool inreg = n <= (long)KPT * NT;
  unsigned keys[KPT];
  if (inreg) {
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
      const long i = (long)j * NT + threadIdx.x;
      keys[j] = i < n ? key_of(x[i]) : 0u;
    }
  }
  for (int round = 0; round < 4; ++round) {
    const int shift = 24 - 8 * round;
    for (int i = threadIdx.x; i < 4 * 256; i += NT) (&hist[0][0])[i] = 0u;
    if (threadIdx.x == 0) {
      int ns = 0;
      for (int s2 = 0; s2 < 4; ++s2) {
        int found = -1;
        for (int t = 0; t < s2; ++t)
          if (prefix[t] == prefix[s2]) { found = slot[t]; break; }
        slot[s2] = found >= 0 ? found : ns++;
      }
      nslot = ns;
    }
    __syncthreads();
    const unsigned mask = round == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
    unsigned pf[4];               // prefix of histogram h (first rank that uses it)
    const int ns = nslot;
#pragma unroll
    for (int h = 0; h < 4; ++h) pf[h] = 0xFFFFFFFFu;
#pragma unroll
    for (int s2 = 3; s2 >= 0; --s2) pf[slot[s2]] = prefix[s2];
    auto count = [&](unsigned k) {
#pragma unroll
      for (int h = 0; h < 4; ++h)
        if (h < ns && (k & mask) == pf[h]) atomicAdd(&hist[h][(k >> shift) & 255u], 1u);     // (integer counts: order-free)
    };
    if (inreg) {
#pragma unroll
      for (int j = 0; j < KPT; ++j)
        if ((long)j * NT + threadIdx.x < n) count(keys[j]);
    } else {
      for (long i = threadIdx.x; i < n; i += NT) count(key_of(x[i]));
    }
    __syncthreads();
    if (threadIdx.x < 4) {
      const int s2 = threadIdx.x, h = slot[s2];
      long r = rank[s2];
      int b = 0;
      for (; b < 255; ++b) {
        const unsigned c = hist[h][b];
        if (r < (long)c) break;
        r -= c;
      }
      rank[s2] = r;                                  // rank inside the chosen bin
      prefix[s2] |= ((unsigned)b) << shift;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float v[4] = {val_of(prefix[0]), val_of(prefix[1]), val_of(prefix[2]), val_of(prefix[3])};
    float qv[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {        // torch lerp
      const float a = v[2 * j], b = v[2 * j + 1], w = wgt[j];
      qv[j] = w < 0.5f ? a + w * (b - a) : b - (b - a) * (1.0f - w);
    }
    const float e0 = alpha * qv[0] + (1.0f - alpha) * ema[0], e1 = alpha * qv[1] + (1.0f - alpha) * ema[1];
    ema[0] = e0; ema[1] = e1;
    out[0] = e0; out[1] = fmaxf(e1 - e0, 1.0f); out[2] = qv[0]; out[3] = qv[1];
  }
}

// out = scale * mean(x[i] * (w ? w[i] : 1)) over n elements
__global__ __launch_bounds__(NT) void wmean_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, long n,
                                                        float scale, float* __restrict__ out, float add = 0.f) {
  __shared__ double red[16];
  double s = 0.0;
  for (long i = threadIdx.x; i < n; i += NT) s += (double)x[i] * (w ? (double)w[i] : 1.0);
  s = block_sum_d(s, red);
  if (threadIdx.x == 0) out[0] = add + (float)(scale * s / n);
}
__global__ void wmean_bwd_kernel(const float* __restrict__ g, const float* __restrict__ w, long n, float scale,
                                 float* __restrict__ dx) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dx[i] = g[0] * scale / n * (w ? w[i] : 1.0f);
}

// Actor objective on lambda-returns (agent/dreamer.py:392-429, actor_grad 'dynamics', no entropy term):
//   normed = (target - offset) / scale   [H, N];   loss = -mean_{h >= 1}( weight[h-1] * normed[h] )
// offset / scale = os[0], os[1] (device scalars from quantile_ema_kernel).  loss[0]; out[0] = mean(normed),
// out[1] = std(normed) over all H*N (the 'normed_target_*' metrics).
__global__ __launch_bounds__(NT) void actor_obj_fwd_kernel(const float* __restrict__ target, const float* __restrict__ weight,
                                                            const float* __restrict__ os, int H, long N,
                                                            float* __restrict__ loss, float* __restrict__ out) {
  __shared__ double red[16];
  const float off = os[0], sc = os[1];
  double l = 0.0, s = 0.0, q = 0.0;
  const long n = (long)H * N;
  for (long i = threadIdx.x; i < n; i += NT) {
    const float v = (target[i] - off) / sc;
    s += v; q += (double)v * v;
    if (i >= N) l += (double)(weight ? weight[i - N] : 1.0f) * v;
  }
  l = block_sum_d(l, red); s = block_sum_d(s, red); q = block_sum_d(q, red);
  if (threadIdx.x == 0) {
    const double mean = s / n;
    loss[0] = (float)(-l / ((double)(H - 1) * N));
    out[0] = (float)mean;
    out[1] = (float)sqrt(fmax((q - n * mean * mean) / (n - 1), 0.0));
  }
}
__global__ void actor_obj_bwd_kernel(const float* __restrict__ g, const float* __restrict__ weight,
                                     const float* __restrict__ os, int H, long N, float* __restrict__ dtarget) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)H * N) return;
  dtarget[i] = i < N ? 0.f : -g[0] * (weight ? weight[i - N] : 1.0f) / (os[1] * (float)((double)(H - 1) * N));
}

// mean over rows of the entropy of Independent(Normal(., std)), std the Normal head's (actor_heads.h).  Two stages with a
// fixed order: one thread per row, one partial per workgroup (double), then one workgroup sums the partials.
__global__ __launch_bounds__(256) void normal_entropy_part_kernel(const float* __restrict__ raw, long R, int A, float min_std,
                                                                  float max_std, double* __restrict__ part) {
  __shared__ double red[4];
  double s = 0.0;
  for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < R; r += (long)gridDim.x * 256) {
    float t = 0.f;
    for (int a = 0; a < A; ++a) t += logf(NormalHead(0.f, raw[r * 2 * A + A + a], min_std, max_std).std);      // (out: not in the entropy)
    s += A * (0.5 + 0.5 * log(2.0 * M_PI)) + (double)t;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ void normal_entropy_final_kernel(const double* __restrict__ part, int nparts, long R, float* __restrict__ out) {
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < nparts; ++i) s += part[i];
    out[0] = (float)(s / R);
  }
}

// ---- connector inputs (VideoSSM.update, agent/video_utils.py:127-161): one workgroup per (b, t) row of E floats
//   clean[b,t]  = video[b, (t / nf) * nf + nf - 1]              (the embedding of the aligned nf-frame chunk)
//   noisy[b,t]  = unit((1 - lam) * clean + lam * unit(eps))     ('lafite' noise; the aligner's input)
//   act_tm[t,b] = [clean * cscale | slots]                      (the SSM's 'action', time-major)
// slots: nf zeros, or with `temporal` one_hot(t % nf) (`connector.temporal_embeds`, get_action :121).
// F.normalize: x / max(||x||, 1e-12).
__global__ __launch_bounds__(256) void connector_prep_kernel(const float* __restrict__ video, const float* __restrict__ eps,
                                                             float* __restrict__ clean, float* __restrict__ noisy,
                                                             float* __restrict__ act_tm, int B, int T, int E, int nf,
                                                             float lam, float cscale, int temporal) {
  __shared__ float red[8];
  const int b = blockIdx.x / T, t = blockIdx.x % T;
  const float* src = video + ((long)b * T + (t / nf) * nf + nf - 1) * E;
  const float* ep = eps + ((long)b * T + t) * E;
  float* cl = clean + ((long)b * T + t) * E;
  float* no = noisy + ((long)b * T + t) * E;
  float* ac = act_tm + ((long)t * B + b) * (E + nf);
  float se = 0.f;
  for (int i = threadIdx.x; i < E; i += 256) se += ep[i] * ep[i];
  se = block_sum_256(se, red);
  const float inv_e = 1.0f / fmaxf(sqrtf(se), 1e-12f);
  float sm = 0.f;
  for (int i = threadIdx.x; i < E; i += 256) {
    const float c = src[i];
    const float m = (1.0f - lam) * c + lam * (ep[i] * inv_e);
    cl[i] = c;
    no[i] = m;                       // (normalised below)
    ac[i] = c * cscale;
    sm += m * m;
  }
  const int slot = temporal ? t % nf : -1;
  for (int i = threadIdx.x; i < nf; i += 256) ac[E + i] = i == slot ? 1.f : 0.f;
  sm = block_sum_256(sm, red);
  const float inv_m = 1.0f / fmaxf(sqrtf(sm), 1e-12f);
  for (int i = threadIdx.x; i < E; i += 256) no[i] *= inv_m;
}

// ---- aligner loss (agent/video_utils.py:146-150): 1 - mean_rows cos(unit(x), c), gradient to x.
// cos[row] = (r . c) / (max(||r||, 1e-8) max(||c||, 1e-8)), r = x / max(||x||, 1e-12)   (F.normalize + F.cosine_similarity)
__global__ __launch_bounds__(256) void cosdist_rows_kernel(const float* __restrict__ x, const float* __restrict__ c,
                                                           float* __restrict__ cosv, float* __restrict__ xnorm, int E) {
  __shared__ float red[8];
  const long row = blockIdx.x;
  const float* xr = x + row * E;
  const float* cr = c + row * E;
  float sx = 0.f, sc = 0.f, dot = 0.f;
  for (int i = threadIdx.x; i < E; i += 256) {
    const float a = xr[i], b = cr[i];
    sx += a * a; sc += b * b; dot += a * b;
  }
  sx = block_sum_256(sx, red); sc = block_sum_256(sc, red); dot = block_sum_256(dot, red);
  if (threadIdx.x == 0) {
    const float nx = fmaxf(sqrtf(sx), 1e-12f);
    const float rn = sqrtf(sx) / nx;                                   // ||r|| (1 unless x is ~0)
    cosv[row] = (dot / nx) / (fmaxf(rn, 1e-8f) * fmaxf(sqrtf(sc), 1e-8f));
    xnorm[row] = nx;
  }
}
// dx[row] = -(g / R) * (c_hat / max(||r||, 1e-8) - cos * r / ||r||^2) / max(||x||, 1e-12)   with c_hat = c / max(||c||, 1e-8),
// r = x / max(||x||, 1e-12): the derivative of both clamps as torch takes it.  For every x with ||x|| >= 1e-12, ||r|| is exactly 1
// and this is (c_hat - cos * r) / ||x||; on an all-zero x row the forward's 1e-8 clamp of ||r|| scales c_hat by 1e8 and the
// projection term (d||r|| = 0 inside the clamp) drops out.
__global__ __launch_bounds__(256) void cosdist_bwd_kernel(const float* __restrict__ x, const float* __restrict__ c,
                                                          const float* __restrict__ cosv, const float* __restrict__ xnorm,
                                                          const float* __restrict__ g, float* __restrict__ dx, long R, int E) {
  __shared__ float red[8];
  const long row = blockIdx.x;
  const float* xr = x + row * E;
  const float* cr = c + row * E;
  float sc = 0.f, sx = 0.f;
  for (int i = threadIdx.x; i < E; i += 256) { sc += cr[i] * cr[i]; sx += xr[i] * xr[i]; }
  sc = block_sum_256(sc, red);
  sx = block_sum_256(sx, red);
  const float nx = xnorm[row], cs = cosv[row];
  const float rn = nx > 1e-12f ? 1.0f : sqrtf(sx) / nx;                  // ||r||: 1 unless the 1e-12 clamp of ||x|| acted
  const float inv_c = 1.0f / fmaxf(sqrtf(sc), 1e-8f) / fmaxf(rn, 1e-8f);
  const float proj = rn >= 1e-8f ? cs / (rn * rn) : 0.f;
  const float k = -g[0] / (float)R / nx;
  for (int i = threadIdx.x; i < E; i += 256) dx[row * E + i] = k * (cr[i] * inv_c - proj * (xr[i] / nx));
}

// ---- teacher-forcing inputs under `connector.token_dropout` (VideoSSM.update, agent/video_utils.py:171-179): one workgroup per
// time-major output row r = t * B + b of W floats.
//   keep[t,b] = e[t,b] < thresh          (e ~ Exp(1): exp(-e) is uniform, so this is `rand > p` with thresh = -log p)
//   x[t,b]    = keep * (t == 0 ? first[b] : post[b, t-1])      (post batch-major (B,T,W))
// Values are copied or zeroed, never scaled: keep is exactly 0 or 1.  VEC: rows of float4 (W % 4 == 0 and aligned bases).
template <bool VEC>
__global__ __launch_bounds__(256) void tf_inputs_fwd_kernel(const float* __restrict__ first, const float* __restrict__ post,
                                                            const float* __restrict__ e, float thresh, int B, int T, int W,
                                                            float* __restrict__ x, float* __restrict__ keep) {
  const long r = blockIdx.x;
  const int t = (int)(r / B), b = (int)(r % B);
  const bool k = e[r] < thresh;
  if (threadIdx.x == 0) keep[r] = k ? 1.f : 0.f;
  const float* src = t == 0 ? first + (long)b * W : post + ((long)b * T + (t - 1)) * W;
  float* dst = x + r * W;
  if (VEC) {
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = threadIdx.x; i < W / 4; i += 256)
      reinterpret_cast<float4*>(dst)[i] = k ? reinterpret_cast<const float4*>(src)[i] : z;
  } else {
    for (int i = threadIdx.x; i < W; i += 256) dst[i] = k ? src[i] : 0.f;
  }
}
// one workgroup per row r = t * B + b of g (T*B, W):  row (0, b) -> dfirst[b];  row (t >= 1, b) -> dpost[b, t-1] (when asked for);
// the rows (T, b) past the end of g zero dpost[b, T-1] (grid: (T + 1) * B rows when dpost is written, B otherwise).
template <bool VEC>
__global__ __launch_bounds__(256) void tf_inputs_bwd_kernel(const float* __restrict__ g, const float* __restrict__ keep, int B,
                                                            int T, int W, float* __restrict__ dfirst, float* __restrict__ dpost) {
  const long r = blockIdx.x;
  const int t = (int)(r / B), b = (int)(r % B);
  float* dst = t == 0 ? dfirst + (long)b * W : dpost + ((long)b * T + (t - 1)) * W;
  const bool k = t < T && keep[r] != 0.f;
  const float* src = g + (t < T ? r : 0) * W;               // (not read when !k)
  if (VEC) {
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = threadIdx.x; i < W / 4; i += 256)
      reinterpret_cast<float4*>(dst)[i] = k ? reinterpret_cast<const float4*>(src)[i] : z;
  } else {
    for (int i = threadIdx.x; i < W; i += 256) dst[i] = k ? src[i] : 0.f;
  }
}

// rows of W floats at these bases can go as float4: W % 4 == 0 and every (non-null) base 16-byte aligned
bool rows_of_float4(int W, const void* a, const void* b, const void* c) {
  return W % 4 == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0;
}

}  // namespace

extern "C" {

int genrl_moments(const float* x, long n, float* out, void* stream) {
  GENRL_ENTER();
  if (n <= 0) return GENRL_EINVAL;
  hipLaunchKernelGGL(moments_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, x, n, out);
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

int genrl_quantile_ema(const float* x, long n, float q0, float q1, float alpha, float* ema, float* out, void* stream) {
  GENRL_ENTER();
  if (n <= 0) return GENRL_EINVAL;
  hipLaunchKernelGGL(quantile_ema_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, x, n, q0, q1, alpha, ema, out);
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

int genrl_wmean_fwd(const float* x, const float* w, long n, float scale, float* out, void* stream) {
  GENRL_ENTER();
  if (n <= 0) return GENRL_EINVAL;
  hipLaunchKernelGGL(wmean_fwd_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, x, w, n, scale, out);
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

int genrl_wmean_bwd(const float* g, const float* w, long n, float scale, float* dx, void* stream) {
  GENRL_ENTER();
  if (n <= 0) return GENRL_EINVAL;
  hipLaunchKernelGGL(wmean_bwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, g, w, n, scale, dx);
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

int genrl_actor_obj_fwd(const float* target, const float* weight, const float* offset_scale, int H, long N, float* loss,
                        float* out, void* stream) {
  GENRL_ENTER();
  if (H < 2 || N <= 0) return GENRL_EINVAL;
  hipLaunchKernelGGL(actor_obj_fwd_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, target, weight, offset_scale, H, N, loss,
                     out);
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

int genrl_actor_obj_bwd(const float* g, const float* weight, const float* offset_scale, int H, long N, float* dtarget,
                        void* stream) {
  GENRL_ENTER();
  if (H < 2 || N <= 0) return GENRL_EINVAL;
  hipLaunchKernelGGL(actor_obj_bwd_kernel, dim3(cdiv((long)H * N, 256)), dim3(256), 0, (hipStream_t)stream, g, weight,
                     offset_scale, H, N, dtarget);
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

int genrl_normal_entropy_mean(const float* raw, long R, int A, float min_std, float max_std, float* out, float* ws, void* stream) {
  GENRL_ENTER();
  if (R <= 0 || A <= 0 || !ws || (reinterpret_cast<uintptr_t>(ws) & 7)) return GENRL_EINVAL;
  const int nb = (int)std::min<long>(cdiv(R, 256), 64);
  double* part = reinterpret_cast<double*>(ws);
  hipLaunchKernelGGL(normal_entropy_part_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, raw, R, A, min_std, max_std, part);
  hipLaunchKernelGGL(normal_entropy_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, part, nb, R, out);
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

int genrl_connector_prep(const float* video, const float* eps, float* clean, float* noisy, float* act_tm, int B, int T,
                         int E, int nf, float lam, float cscale, void* stream) {
  return genrl_connector_prep_slots(video, eps, clean, noisy, act_tm, B, T, E, nf, lam, cscale, 0, stream);
}

int genrl_connector_prep_slots(const float* video, const float* eps, float* clean, float* noisy, float* act_tm, int B, int T,
                               int E, int nf, float lam, float cscale, int temporal, void* stream) {
  GENRL_ENTER();
  if (B <= 0 || T <= 0 || E <= 0 || nf <= 0 || T % nf) return GENRL_EINVAL;
  hipLaunchKernelGGL(connector_prep_kernel, dim3(B * T), dim3(256), 0, (hipStream_t)stream, video, eps, clean, noisy, act_tm,
                     B, T, E, nf, lam, cscale, temporal != 0);
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

int genrl_tf_inputs_fwd(const float* first, const float* post, const float* e, float thresh, int B, int T, int W, float* x,
                        float* keep, void* stream) {
  GENRL_ENTER();
  if (B <= 0 || T <= 0 || W <= 0 || !first || !post || !e || !x || !keep) return GENRL_EINVAL;
  auto kern = rows_of_float4(W, first, post, x) ? tf_inputs_fwd_kernel<true> : tf_inputs_fwd_kernel<false>;
  hipLaunchKernelGGL(kern, dim3((unsigned)((long)T * B)), dim3(256), 0, (hipStream_t)stream, first, post, e, thresh, B, T, W, x,
                     keep);
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

int genrl_tf_inputs_bwd(const float* g, const float* keep, int B, int T, int W, float* dfirst, float* dpost, void* stream) {
  GENRL_ENTER();
  if (B <= 0 || T <= 0 || W <= 0 || !g || !keep || !dfirst) return GENRL_EINVAL;
  auto kern = rows_of_float4(W, g, dfirst, dpost) ? tf_inputs_bwd_kernel<true> : tf_inputs_bwd_kernel<false>;
  const long rows = dpost ? (long)(T + 1) * B : B;
  hipLaunchKernelGGL(kern, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, g, keep, B, T, W, dfirst, dpost);
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

/* out[0] = 1 - mean(cos); cosv / xnorm: R floats each, kept for the backward */
int genrl_cosdist_fwd(const float* x, const float* c, float* cosv, float* xnorm, float* out, long R, int E, void* stream) {
  GENRL_ENTER();
  if (R <= 0 || E <= 0) return GENRL_EINVAL;
  hipLaunchKernelGGL(cosdist_rows_kernel, dim3(R), dim3(256), 0, (hipStream_t)stream, x, c, cosv, xnorm, E);
  hipLaunchKernelGGL(wmean_fwd_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, cosv, (const float*)nullptr, R, -1.0f, out, 1.0f);
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

int genrl_cosdist_bwd(const float* x, const float* c, const float* cosv, const float* xnorm, const float* g, float* dx,
                      long R, int E, void* stream) {
  GENRL_ENTER();
  if (R <= 0 || E <= 0) return GENRL_EINVAL;
  hipLaunchKernelGGL(cosdist_bwd_kernel, dim3(R), dim3(256), 0, (hipStream_t)stream, x, c, cosv, xnorm, g, dx, R, E);
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

}  // extern "C"
