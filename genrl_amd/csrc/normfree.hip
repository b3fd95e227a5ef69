// Kernels of the DreamerV2 defaults (conf/defaults/dreamer_v2.yaml): the SiLU behind a norm-free Linear (`norm: none`,
// agent/dreamer_utils.py:739-747), the truncated-normal actor head (DistLayer 'trunc_normal', :830-834 with tools/utils.py:102-123) and the
// squared-error log-likelihood of the one-wide `mse` heads (:62-83), each with its backward.
//
// The SiLU pair has the shape of the ReLU pair of ensemble.hip: one 256-thread workgroup walks rows grid-strided with 16-byte accesses; a
// call that also emits h2 planes makes two sweeps over the row (store fp32 + row maximum, then re-read what THIS thread stored and split),
// so the planes are those of the stored fp32 values.  The head and the squared error are elementwise: one thread per element.
// No reductions other than the row maximum (fixed order), no atomics, no allocation.
#include "common.h"
#include "genrl_hip.h"

namespace {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
constexpr int NF_GRID = 2048;          // workgroups at most: rows are grid-strided

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// second sweep: planes of the row this thread has just written
__device__ __forceinline__ void planes_of_row(const float* yr, int nv, const PlaneOut& xo, long row, float amax, float* red) {
  const float inv = h2_inv_of(block_max_256(amax, red)), sc = h2_scale_of(inv);
  for (int j = threadIdx.x; j < nv; j += 256) h2_store4(xo, row, 4 * j, ld4(yr + 4 * j), sc);
  if (threadIdx.x == 0) xo.inv[row] = inv;
}

// y = x sigmoid(x) (y may be x).  x = -100: exp(100) = inf, sigmoid = 0, y = -0; a NaN stays NaN
__global__ __launch_bounds__(256) void silu_fwd_kernel(const float* x, long ldx, float* y, long ldy, int M, int N, PlaneOut xo) {
  __shared__ float red[8];
  const int nv = N >> 2;
  for (long row = blockIdx.x; row < M; row += gridDim.x) {
    const float* xr = x + row * ldx;
    float* yr = y + row * ldy;
    float am = 0.f;
    for (int j = threadIdx.x; j < nv; j += 256) {
      float4 v = ld4(xr + 4 * j);
      v.x = siluf_(v.x); v.y = siluf_(v.y); v.z = siluf_(v.z); v.w = siluf_(v.w);
      st4(yr + 4 * j, v);
      am = fmaxf(am, h2_amax4(v));
    }
    if (xo.p) planes_of_row(yr, nv, xo, row, am, red);
  }
}

// dx = dy sigmoid(x) (1 + x (1 - sigmoid(x))) from the saved pre-activation x (dx may be dy)
__global__ __launch_bounds__(256) void silu_bwd_kernel(const float* dy, long lddy, const float* x, long ldx, float* dx, long lddx,
                                                       int M, int N, PlaneOut xo) {
  __shared__ float red[8];
  const int nv = N >> 2;
  for (long row = blockIdx.x; row < M; row += gridDim.x) {
    const float* gr = dy + row * lddy;
    const float* xr = x + row * ldx;
    float* dr = dx + row * lddx;
    float am = 0.f;
    for (int j = threadIdx.x; j < nv; j += 256) {
      const float4 g = ld4(gr + 4 * j), a = ld4(xr + 4 * j);
      float4 v;
      v.x = g.x * dsiluf_(a.x); v.y = g.y * dsiluf_(a.y); v.z = g.z * dsiluf_(a.z); v.w = g.w * dsiluf_(a.w);
      st4(dr + 4 * j, v);
      am = fmaxf(am, h2_amax4(v));
    }
    if (xo.p) planes_of_row(dr, nv, xo, row, am, red);
  }
}

// the clamp of TruncatedNormal._clamp (low + eps, high - eps with low, high = -1, 1 and eps = 1e-6, rounded to fp32 as torch.clamp does)
__device__ __forceinline__ float tn_clamp(float x) {
  const float lo = (float)(-1.0 + 1e-6), hi = (float)(1.0 - 1e-6);
  return x < lo ? lo : (x > hi ? hi : x);           // (a NaN stays NaN)
}

// raw[R, 2A] = [out | std_raw]; mean = tanh(out); std = 2 sigmoid((std_raw + init_std) / 2) + min_std; action = clamp(mean + eps std).
// eps == NULL: the mean-only form (action, if asked for, = clamp(mean))
__global__ void tn_head_fwd_kernel(const float* __restrict__ raw, const float* __restrict__ eps, float* __restrict__ action,
                                   float* __restrict__ mean_out, float* __restrict__ std_out, long n, int A, float min_std,
                                   float init_std, long ld_action) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long r = i / A;
  const int a = (int)(i % A);
  const float mean = tanhf(raw[r * 2 * A + a]);
  const float sd = 2.0f * sigmoidf_((raw[r * 2 * A + A + a] + init_std) * 0.5f) + min_std;
  if (action) action[r * ld_action + a] = tn_clamp(eps ? mean + eps[i] * sd : mean);
  if (mean_out) mean_out[i] = mean;
  if (std_out) std_out[i] = sd;
}

// straight-through clamp (x - sg(x) + sg(clamp(x))): the gradient is that of x = mean + eps std whether or not the element clamped
__global__ void tn_head_bwd_kernel(const float* __restrict__ daction, const float* __restrict__ raw, const float* __restrict__ eps,
                                   float* __restrict__ draw, long n, int A, float init_std, long ld_action) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long r = i / A;
  const int a = (int)(i % A);
  const float mean = tanhf(raw[r * 2 * A + a]);
  const float sg = sigmoidf_((raw[r * 2 * A + A + a] + init_std) * 0.5f);
  const float g = daction[r * ld_action + a];
  draw[r * 2 * A + a] = g * (1.0f - mean * mean);
  draw[r * 2 * A + A + a] = g * eps[i] * (sg * (1.0f - sg));
}

// like = -(out - x)^2
__global__ void sqerr_fwd_kernel(const float* __restrict__ out, const float* __restrict__ x, float* __restrict__ like, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float d = out[i] - x[i];
  like[i] = -(d * d);
}

// dout = -2 (out - x) g
__global__ void sqerr_bwd_kernel(const float* __restrict__ out, const float* __restrict__ x, const float* __restrict__ g,
                                 float* __restrict__ dout, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  dout[i] = -2.0f * (out[i] - x[i]) * g[i];
}

inline int row_grid(int M) { return M < NF_GRID ? M : NF_GRID; }
inline bool bad_planes(const uint16_t* yp, long ldp, const float* inv, int N) { return yp && (!inv || (ldp & 3) || ldp < N); }

}  // namespace

extern "C" {

int genrl_silu_fwd_h2(const float* x, long ldx, float* y, long ldy, int M, int N, uint16_t* yp, long ldp, long plane, float* inv,
                      void* stream) {
  GENRL_ENTER();
  if (M <= 0) return GENRL_OK;
  if (N <= 0 || (N & 3) || (ldx & 3) || (ldy & 3) || ldx < N || ldy < N || !x || !y || !aligned16(x) || !aligned16(y) ||
      bad_planes(yp, ldp, inv, N))
    return GENRL_EINVAL;
  silu_fwd_kernel<<<row_grid(M), 256, 0, (hipStream_t)stream>>>(x, ldx, y, ldy, M, N, PlaneOut{yp, ldp, plane, inv});
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

int genrl_silu_bwd_h2(const float* dy, long lddy, const float* x, long ldx, float* dx, long lddx, int M, int N, uint16_t* dxp, long ldp,
                      long plane, float* inv, void* stream) {
  GENRL_ENTER();
  if (M <= 0) return GENRL_OK;
  if (N <= 0 || (N & 3) || (lddy & 3) || (ldx & 3) || (lddx & 3) || lddy < N || ldx < N || lddx < N || !dy || !x || !dx ||
      !aligned16(dy) || !aligned16(x) || !aligned16(dx) || bad_planes(dxp, ldp, inv, N))
    return GENRL_EINVAL;
  silu_bwd_kernel<<<row_grid(M), 256, 0, (hipStream_t)stream>>>(dy, lddy, x, ldx, dx, lddx, M, N, PlaneOut{dxp, ldp, plane, inv});
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

int genrl_trunc_normal_head_fwd(const float* raw, const float* eps, float* action, float* mean, float* std, long R, int A,
                                float min_std, float init_std, long ld_action, void* stream) {
  GENRL_ENTER();
  if (R <= 0) return GENRL_OK;
  if (A <= 0 || !raw || (!action && !mean && !std)) return GENRL_EINVAL;
  if (ld_action == 0) ld_action = A;
  if (ld_action < A) return GENRL_EINVAL;
  const long n = R * A;
  tn_head_fwd_kernel<<<cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(raw, eps, action, mean, std, n, A, min_std, init_std, ld_action);
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

int genrl_trunc_normal_head_bwd(const float* daction, const float* raw, const float* eps, float* draw, long R, int A, float init_std,
                                long ld_action, void* stream) {
  GENRL_ENTER();
  if (R <= 0) return GENRL_OK;
  if (A <= 0 || !daction || !raw || !eps || !draw) return GENRL_EINVAL;
  if (ld_action == 0) ld_action = A;
  if (ld_action < A) return GENRL_EINVAL;
  const long n = R * A;
  tn_head_bwd_kernel<<<cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(daction, raw, eps, draw, n, A, init_std, ld_action);
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

int genrl_sqerr_fwd(const float* out, const float* x, float* like, long n, void* stream) {
  GENRL_ENTER();
  if (n <= 0) return GENRL_OK;
  if (!out || !x || !like) return GENRL_EINVAL;
  sqerr_fwd_kernel<<<cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(out, x, like, n);
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

int genrl_sqerr_bwd(const float* out, const float* x, const float* g, float* dout, long n, void* stream) {
  GENRL_ENTER();
  if (n <= 0) return GENRL_OK;
  if (!out || !x || !g || !dout) return GENRL_EINVAL;
  sqerr_bwd_kernel<<<cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(out, x, g, dout, n);
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

}  // extern "C"
