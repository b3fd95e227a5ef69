// The continuous actor heads (DistLayer, agent/dreamer_utils.py:814-834), each defined once on ONE element of raw [R, 2A] = [out | std_raw].
// A head is constructed from (out, std_raw, p0, p1) -- its two parameters in the order of its entry points -- and has
//   mean, std                          the distribution's parameters,
//   action(e, has_eps)                 the sample with noise e, or the mode without (has_eps false: e is not looked at),
//   backward(g, e, d_out, d_std_raw)   d raw from g = d loss / d action.
// Every kernel that runs a head (heads.hip; the linear-fused pair of rowops.hip) takes it from here, so a kernel that is to run another
// head takes it as a template argument.  Each struct keeps its own order of floating-point operations: results are bits that tests and
// recorded runs compare, and a product taken in another order is another number.
#pragma once
#include "common.h"

// 'normal' (:814-819): mean = tanh(out), std = (max_std - min_std) sigmoid(std_raw + 2) + min_std, action = mean + std eps
struct NormalHead {
  float mean, std, sg, span;         // sg = sigmoid(std_raw + 2), span = max_std - min_std
  __device__ __forceinline__ NormalHead(float out, float std_raw, float min_std, float max_std) {
    mean = tanhf(out);
    sg = sigmoidf_(std_raw + 2.0f);
    span = max_std - min_std;
    std = span * sg + min_std;
  }
  __device__ __forceinline__ float action(float e, bool has_eps) const { return mean + std * (has_eps ? e : 0.f); }
  __device__ __forceinline__ void backward(float g, float e, float& d_out, float& d_std_raw) const {
    d_out = g * (1.0f - mean * mean);
    d_std_raw = g * e * span * sg * (1.0f - sg);
  }
};

// 'trunc_normal' (:830-834 with tools/utils.py:102-123): mean = tanh(out), std = 2 sigmoid((std_raw + init_std) / 2) + min_std,
// action = clamp(mean + eps std).  The clamp is straight-through (x - sg(x) + sg(clamp(x))): the gradient is that of x = mean + eps std
// whether or not the element clamped
struct TruncNormalHead {
  float mean, std, sg;               // sg = sigmoid((std_raw + init_std) / 2)
  __device__ __forceinline__ TruncNormalHead(float out, float std_raw, float min_std, float init_std) {
    mean = tanhf(out);
    sg = sigmoidf_((std_raw + init_std) * 0.5f);
    std = 2.0f * sg + min_std;
  }
  // TruncatedNormal._clamp: low + eps, high - eps with low, high = -1, 1 and eps = 1e-6, rounded to fp32 as torch.clamp does
  static __device__ __forceinline__ float clamp(float x) {
    const float lo = (float)(-1.0 + 1e-6), hi = (float)(1.0 - 1e-6);
    return x < lo ? lo : (x > hi ? hi : x);           // (a NaN stays NaN)
  }
  __device__ __forceinline__ float action(float e, bool has_eps) const { return clamp(has_eps ? mean + e * std : mean); }
  __device__ __forceinline__ void backward(float g, float e, float& d_out, float& d_std_raw) const {
    d_out = g * (1.0f - mean * mean);
    d_std_raw = g * e * (sg * (1.0f - sg));
  }
};

// 'tanh_normal' (:824-829; SquashedNormal, tools/utils.py:126-170): mean = 5 tanh(out / 5), std = softplus(std_raw + init_std) + min_std,
// x = mean + std eps, action = tanh(x)
struct TanhNormalHead {
  float th, mean, z, std;            // th = tanh(out / 5), z = std_raw + init_std
  __device__ __forceinline__ TanhNormalHead(float out, float std_raw, float min_std, float init_std) {
    th = tanhf(out / 5.0f);
    mean = 5.0f * th;
    z = std_raw + init_std;
    std = softplusf_(z) + min_std;
  }
  // d mean / d out and d std / d std_raw (what the Monte-Carlo kernels of heads.hip chain through)
  __device__ __forceinline__ float dmean() const { return 1.0f - th * th; }
  __device__ __forceinline__ float dstd() const { return dsoftplusf_(z); }
  __device__ __forceinline__ float action(float e, bool has_eps) const { return tanhf(has_eps ? mean + std * e : mean); }
  // dx = g (1 - action^2); d mean = dx, d std = dx eps
  __device__ __forceinline__ void backward(float g, float e, float& d_out, float& d_std_raw) const {
    const float t = tanhf(mean + std * e);
    const float dx = g * (1.0f - t * t);
    d_out = dx * dmean();
    d_std_raw = dx * e * dstd();
  }
};
