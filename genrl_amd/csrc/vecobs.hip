// Vector (1-D) observations (gfx950): the symlog of the encoder's MLP inputs (agent/dreamer_utils.py:623-628, `symlog_inputs`) written
// straight into a column slice of the first layer's input, so that the concatenation of several keys is one launch per key and no copy;
// and the log-likelihood of the decoder's vector heads with its gradient -- MSEDist on a D-wide head (:62-83), with the elementwise
// squared error of the one-wide `mse` heads (reward, critic) as a pair of its own, and SymlogDist 'mse' with agg 'sum' (:85-118,
// `mlp_dist: symlog_mse`).  Bandwidth-bound row kernels: the symlog walks the elements flat, with 16-byte accesses where pointers, D and
// pitches allow and scalar ones otherwise (widths such as 7 and 9 are the normal case); the likelihood puts a row on an aligned group of W
// lanes that stride over D and combine with shuffles in a fixed order, as gauss_kl_fwd_kernel of gaussian.hip does; its gradient is
// elementwise.  No allocation, no synchronisation with the host, no atomics.
#include "common.h"
#include "genrl_hip.h"
#include <math.h>

namespace {

constexpr int VO_GRID = 1 << 16;       // workgroups at most: elements are grid-strided
constexpr int VO_MAX_D = 1 << 20;

template <bool SYMLOG>
__device__ __forceinline__ float maybe_symlog(float x) { return SYMLOG ? symlogf_(x) : x; }

// y[r, :D] = symlog(x[r, :D]) (or x); VEC: one float4 per thread and sweep, D % 4 == 0
template <bool SYMLOG, bool VEC>
__global__ __launch_bounds__(256) void symlog_rows_kernel(const float* __restrict__ x, long ldx, float* __restrict__ y, long ldy, long R,
                                                          int D) {
  const int per = VEC ? D / 4 : D;              // work items of a row
  const long n = R * per;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long row = i / per;
    const int c = (int)(i - row * per);
    if (VEC) {
      const float4 v = ld4(x + row * ldx + 4 * c);
      st4(y + row * ldy + 4 * c,
          float4{maybe_symlog<SYMLOG>(v.x), maybe_symlog<SYMLOG>(v.y), maybe_symlog<SYMLOG>(v.z), maybe_symlog<SYMLOG>(v.w)});
    } else {
      y[row * ldy + c] = maybe_symlog<SYMLOG>(x[row * ldx + c]);
    }
  }
}

// one element's distance: (mode - t)^2 in double from the fp32 operands, t = x or symlog(x) -- the logarithm in double as well: the target
// then carries no rounding of its own and a row's error is the one rounding of its result (the kernel moves 8 bytes per element and has the
// arithmetic to spare); KIND 1: 0 below tol.  The forward and the backward kernel decide `below tol` with this one expression.
template <int KIND>
__device__ __forceinline__ double vec_dist(float m, float x, double tol, double& diff) {
  const double t = KIND == 1 ? copysign(log(fabs((double)x) + 1.0), (double)x) : (double)x;
  diff = (double)m - t;
  const double d = diff * diff;
  return (KIND == 1 && d < tol) ? 0.0 : d;
}

// like[r] = -sum_d dist(mode[r, d], x[r, d]): one row per aligned group of W lanes, double accumulation, fixed order
template <int W, int KIND>
__global__ __launch_bounds__(256) void vec_like_fwd_kernel(const float* __restrict__ mode, long ldm, const float* __restrict__ x, long ldx,
                                                           float* __restrict__ like, long R, int D, float tol) {
  const long g = ((long)blockIdx.x * 256 + threadIdx.x) / W;
  const int lane = threadIdx.x % W;
  const long row = g < R ? g : R - 1;            // (a group past the end re-reads the last row and stores nothing)
  const float* mr = mode + row * ldm;
  const float* xr = x + row * ldx;
  double s = 0.0, diff;
  for (int d = lane; d < D; d += W) s += vec_dist<KIND>(mr[d], xr[d], (double)tol, diff);
  s = group_sum_d<W>(s);
  if (g < R && lane == 0) like[g] = (float)(-s);
}

// dmode[r, d] (+)= -2 (mode - t) g[r]; KIND 1: exactly 0 where (mode - t)^2 < tol
template <int KIND>
__global__ __launch_bounds__(256) void vec_like_bwd_kernel(const float* __restrict__ mode, long ldm, const float* __restrict__ x, long ldx,
                                                           const float* __restrict__ g, float* __restrict__ dmode, long lddm, long R, int D,
                                                           float tol, int accumulate) {
  const long n = R * D;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long row = i / D;
    const int c = (int)(i - row * D);
    double diff;
    const double d = vec_dist<KIND>(mode[row * ldm + c], x[row * ldx + c], (double)tol, diff);
    float v = d == 0.0 ? 0.0f : (float)(-2.0 * diff * (double)g[row]);
    float* o = dmode + row * lddm + c;
    if (accumulate) v += *o;
    *o = v;
  }
}

// the one-wide heads, on contiguous operands and in fp32: like = -(out - x)^2 per element
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

inline int flat_grid(long n) {
  const long b = (n + 255) / 256;
  return b < VO_GRID ? (int)b : VO_GRID;
}

}  // namespace

extern "C" {

int genrl_symlog_rows(const float* x, long ldx, float* y, long ldy, long R, int D, int symlog, void* stream) {
  GENRL_ENTER();
  if (R < 0 || D <= 0 || D > VO_MAX_D || ldx < D || ldy < D || !x || !y) return GENRL_EINVAL;
  if (R == 0) return GENRL_OK;
  const bool vec = (D & 3) == 0 && (ldx & 3) == 0 && (ldy & 3) == 0 && aligned16(x) && aligned16(y);
  const dim3 grid(flat_grid(R * (vec ? D / 4 : D))), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (symlog) {
    if (vec) hipLaunchKernelGGL((symlog_rows_kernel<true, true>), grid, block, 0, st, x, ldx, y, ldy, R, D);
    else hipLaunchKernelGGL((symlog_rows_kernel<true, false>), grid, block, 0, st, x, ldx, y, ldy, R, D);
  } else {
    if (vec) hipLaunchKernelGGL((symlog_rows_kernel<false, true>), grid, block, 0, st, x, ldx, y, ldy, R, D);
    else hipLaunchKernelGGL((symlog_rows_kernel<false, false>), grid, block, 0, st, x, ldx, y, ldy, R, D);
  }
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

int genrl_vec_like_fwd(const float* mode, long ldm, const float* x, long ldx, float* like, long R, int D, int kind, float tol,
                       void* stream) {
  GENRL_ENTER();
  if (R < 0 || R > (1L << 32) || D <= 0 || D > VO_MAX_D || ldm < D || ldx < D || !mode || !x || !like || (kind != 0 && kind != 1) ||
      !(tol >= 0.f))
    return GENRL_EINVAL;
  if (R == 0) return GENRL_OK;
  return dispatch_w(D, [&](auto w) {
    constexpr int W = decltype(w)::value;
    const dim3 grid(cdiv(R * W, 256)), block(256);
    if (kind == 0)
      hipLaunchKernelGGL((vec_like_fwd_kernel<W, 0>), grid, block, 0, (hipStream_t)stream, mode, ldm, x, ldx, like, R, D, tol);
    else
      hipLaunchKernelGGL((vec_like_fwd_kernel<W, 1>), grid, block, 0, (hipStream_t)stream, mode, ldm, x, ldx, like, R, D, tol);
    GENRL_CHECK_LAUNCH();
    return GENRL_OK;
  });
}

int genrl_vec_like_bwd(const float* mode, long ldm, const float* x, long ldx, const float* g, float* dmode, long lddm, long R, int D,
                       int kind, float tol, int accumulate, void* stream) {
  GENRL_ENTER();
  if (R < 0 || D <= 0 || D > VO_MAX_D || ldm < D || ldx < D || lddm < D || !mode || !x || !g || !dmode || (kind != 0 && kind != 1) ||
      !(tol >= 0.f))
    return GENRL_EINVAL;
  if (R == 0) return GENRL_OK;
  const dim3 grid(flat_grid(R * D)), block(256);
  if (kind == 0)
    hipLaunchKernelGGL((vec_like_bwd_kernel<0>), grid, block, 0, (hipStream_t)stream, mode, ldm, x, ldx, g, dmode, lddm, R, D, tol,
                       accumulate);
  else
    hipLaunchKernelGGL((vec_like_bwd_kernel<1>), grid, block, 0, (hipStream_t)stream, mode, ldm, x, ldx, g, dmode, lddm, R, D, tol,
                       accumulate);
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
