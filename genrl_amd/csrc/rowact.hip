// Activations that stand alone between two products (gfx950), each with its backward: the ReLU between the two layers of a Plan2Explore
// ensemble member (agent/plan2explore.py:8-41) and the SiLU or ELU behind a norm-free Linear (`norm: none`, agent/dreamer_utils.py:739-747).
//
// HBM-bound streams over rows of any multiple of 4 floats: one 256-thread workgroup walks rows grid-strided with 16-byte accesses.  A call
// that also emits h2 planes needs the row maximum before it can split, so it makes two sweeps over the row: the first computes and stores
// the fp32 result and takes the maximum, the second re-reads what THIS thread has just stored (the same addresses in program order: served
// by the L2) and writes the planes, so the planes are those of the stored fp32 values.  HBM bytes per element: 4 read + 4 written + 4 for
// the two fp16 planes.  The activation is a policy: fwd(x), and bwd(g, saved) with `saved` what its backward keeps from the forward.
// No reductions other than the row maximum (fixed order), no atomics, no allocation.
#include "common.h"
#include "genrl_hip.h"

namespace {

constexpr int ACT_GRID = 2048;          // workgroups at most: rows are grid-strided

struct Relu {          // saved: the output y.  (a NaN stays NaN, as in torch.relu: fmaxf would drop it)
  static __device__ __forceinline__ float fwd(float x) { return x > 0.f ? x : (x != x ? x : 0.f); }
  static __device__ __forceinline__ float bwd(float g, float y) { return y > 0.f ? g : 0.f; }
};
struct Silu {          // saved: the pre-activation x.  x = -100: exp(100) = inf, sigmoid = 0, y = -0; a NaN stays NaN
  static __device__ __forceinline__ float fwd(float x) { return siluf_(x); }
  static __device__ __forceinline__ float bwd(float g, float x) { return g * dsiluf_(x); }
};
struct Elu {           // saved: the pre-activation x.  x = -100: y = -1, dy/dx = 0; a NaN stays NaN (common.h)
  static __device__ __forceinline__ float fwd(float x) { return eluf_(x); }
  static __device__ __forceinline__ float bwd(float g, float x) { return g * deluf_(x); }
};

// y = act(x) (y may be x itself)
template <typename Act>
__global__ __launch_bounds__(256) void act_fwd_kernel(const float* x, long ldx, float* y, long ldy, int M, int N, PlaneOut xo) {
  __shared__ float red[8];
  const int nv = N >> 2;
  for (long row = blockIdx.x; row < M; row += gridDim.x) {
    const float* xr = x + row * ldx;
    float* yr = y + row * ldy;
    float am = 0.f;
    for (int j = threadIdx.x; j < nv; j += 256) {
      float4 v = ld4(xr + 4 * j);
      v.x = Act::fwd(v.x); v.y = Act::fwd(v.y); v.z = Act::fwd(v.z); v.w = Act::fwd(v.w);
      st4(yr + 4 * j, v);
      am = fmaxf(am, h2_amax4(v));
    }
    if (xo.p) planes_of_row(yr, nv, xo, row, am, red);
  }
}

// dx = act'(dy; saved) (dx may be dy itself)
template <typename Act>
__global__ __launch_bounds__(256) void act_bwd_kernel(const float* dy, long lddy, const float* saved, long lds_, float* dx, long lddx,
                                                      int M, int N, PlaneOut xo) {
  __shared__ float red[8];
  const int nv = N >> 2;
  for (long row = blockIdx.x; row < M; row += gridDim.x) {
    const float* gr = dy + row * lddy;
    const float* sr = saved + row * lds_;
    float* dr = dx + row * lddx;
    float am = 0.f;
    for (int j = threadIdx.x; j < nv; j += 256) {
      const float4 g = ld4(gr + 4 * j), a = ld4(sr + 4 * j);
      float4 v;
      v.x = Act::bwd(g.x, a.x); v.y = Act::bwd(g.y, a.y); v.z = Act::bwd(g.z, a.z); v.w = Act::bwd(g.w, a.w);
      st4(dr + 4 * j, v);
      am = fmaxf(am, h2_amax4(v));
    }
    if (xo.p) planes_of_row(dr, nv, xo, row, am, red);
  }
}

template <typename Act>
int act_fwd(const float* x, long ldx, float* y, long ldy, int M, int N, uint16_t* yp, long ldp, long plane, float* inv, void* stream) {
  GENRL_ENTER();
  if (M <= 0) return GENRL_OK;
  if (N <= 0 || (N & 3) || (ldx & 3) || (ldy & 3) || ldx < N || ldy < N || !x || !y || !aligned16(x) || !aligned16(y) ||
      bad_planes(yp, ldp, inv, N))
    return GENRL_EINVAL;
  act_fwd_kernel<Act><<<row_grid(M, ACT_GRID), 256, 0, (hipStream_t)stream>>>(x, ldx, y, ldy, M, N, PlaneOut{yp, ldp, plane, inv});
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

template <typename Act>
int act_bwd(const float* dy, long lddy, const float* saved, long lds_, float* dx, long lddx, int M, int N, uint16_t* dxp, long ldp,
            long plane, float* inv, void* stream) {
  GENRL_ENTER();
  if (M <= 0) return GENRL_OK;
  if (N <= 0 || (N & 3) || (lddy & 3) || (lds_ & 3) || (lddx & 3) || lddy < N || lds_ < N || lddx < N || !dy || !saved || !dx ||
      !aligned16(dy) || !aligned16(saved) || !aligned16(dx) || bad_planes(dxp, ldp, inv, N))
    return GENRL_EINVAL;
  act_bwd_kernel<Act><<<row_grid(M, ACT_GRID), 256, 0, (hipStream_t)stream>>>(dy, lddy, saved, lds_, dx, lddx, M, N,
                                                                              PlaneOut{dxp, ldp, plane, inv});
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

}  // namespace

extern "C" {

int genrl_relu_fwd_h2(const float* x, long ldx, float* y, long ldy, int M, int N, uint16_t* yp, long ldp, long plane, float* inv,
                      void* stream) {
  return act_fwd<Relu>(x, ldx, y, ldy, M, N, yp, ldp, plane, inv, stream);
}

int genrl_relu_bwd_h2(const float* dy, long lddy, const float* y, long ldy, float* dx, long lddx, int M, int N, uint16_t* dxp, long ldp,
                      long plane, float* inv, void* stream) {
  return act_bwd<Relu>(dy, lddy, y, ldy, dx, lddx, M, N, dxp, ldp, plane, inv, stream);
}

int genrl_silu_fwd_h2(const float* x, long ldx, float* y, long ldy, int M, int N, uint16_t* yp, long ldp, long plane, float* inv,
                      void* stream) {
  return act_fwd<Silu>(x, ldx, y, ldy, M, N, yp, ldp, plane, inv, stream);
}

int genrl_silu_bwd_h2(const float* dy, long lddy, const float* x, long ldx, float* dx, long lddx, int M, int N, uint16_t* dxp, long ldp,
                      long plane, float* inv, void* stream) {
  return act_bwd<Silu>(dy, lddy, x, ldx, dx, lddx, M, N, dxp, ldp, plane, inv, stream);
}

int genrl_elu_fwd_h2(const float* x, long ldx, float* y, long ldy, int M, int N, uint16_t* yp, long ldp, long plane, float* inv,
                     void* stream) {
  return act_fwd<Elu>(x, ldx, y, ldy, M, N, yp, ldp, plane, inv, stream);
}

int genrl_elu_bwd_h2(const float* dy, long lddy, const float* x, long ldx, float* dx, long lddx, int M, int N, uint16_t* dxp, long ldp,
                     long plane, float* inv, void* stream) {
  return act_bwd<Elu>(dy, lddy, x, ldx, dx, lddx, M, N, dxp, ldp, plane, inv, stream);
}

}  // extern "C"
