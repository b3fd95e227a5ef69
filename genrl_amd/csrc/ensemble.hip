// Row kernels of the Plan2Explore ensemble (agent/plan2explore.py:8-41): the row-wise L2 prediction error of the training loss and the
// across-member variance of the intrinsic reward, each with its backward.  (The ReLU between a member's two products is in rowact.hip.)
//
// All four are HBM-bound streams over rows of up to 12 288 floats (any multiple of 4): one 256-thread workgroup walks rows
// grid-strided with 16-byte accesses.  A kernel that also emits h2 planes needs the row maximum before it can split, so it makes two
// sweeps over the row: the first computes and stores the fp32 result and takes the maximum, the second re-reads what THIS thread has
// just stored (the same addresses in program order: served by the L2, the row is <= 48 KiB per member) and writes the planes.  HBM
// bytes per element: 4 read + 4 written + 4 for the two fp16 planes.
//
// Reductions have a fixed order (per thread in column order, 64-lane butterfly, four waves summed in order): same input, same bits.
// No atomics, no allocation, no synchronisation.
#include "common.h"
#include "genrl_hip.h"

namespace {

constexpr int ENS_GRID = 2048;          // workgroups at most: rows are grid-strided
constexpr int ENS_MAXK = 8;

// err[m] = || t[m] - p[m] ||
__global__ __launch_bounds__(256) void l2err_fwd_kernel(const float* __restrict__ t, long ldt, const float* __restrict__ p, long ldp,
                                                        float* __restrict__ err, int M, int N) {
  __shared__ float red[8];
  const int nv = N >> 2;
  for (long row = blockIdx.x; row < M; row += gridDim.x) {
    const float* tr = t + row * ldt;
    const float* pr = p + row * ldp;
    float s = 0.f;
    for (int j = threadIdx.x; j < nv; j += 256) {
      const float4 a = ld4(tr + 4 * j), b = ld4(pr + 4 * j);
      const float d0 = a.x - b.x, d1 = a.y - b.y, d2 = a.z - b.z, d3 = a.w - b.w;
      s += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
    }
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) err[row] = sqrtf(s);
  }
}

// dp[m] = -(t[m] - p[m]) (g[m] / err[m]); a row with err = 0 gets zeros (torch's norm backward masks it the same way)
__global__ __launch_bounds__(256) void l2err_bwd_kernel(const float* __restrict__ g, const float* __restrict__ err,
                                                        const float* __restrict__ t, long ldt, const float* __restrict__ p, long ldp,
                                                        float* __restrict__ dp, long lddp, int M, int N, PlaneOut xo) {
  __shared__ float red[8];
  const int nv = N >> 2;
  for (long row = blockIdx.x; row < M; row += gridDim.x) {
    const float* tr = t + row * ldt;
    const float* pr = p + row * ldp;
    float* dr = dp + row * lddp;
    const float e = err[row];
    const bool zero = e == 0.f;
    const float c = zero ? 0.f : g[row] / e;
    float am = 0.f;
    for (int j = threadIdx.x; j < nv; j += 256) {
      const float4 a = ld4(tr + 4 * j), b = ld4(pr + 4 * j);
      float4 v;
      v.x = zero ? 0.f : -((a.x - b.x) * c); v.y = zero ? 0.f : -((a.y - b.y) * c);
      v.z = zero ? 0.f : -((a.z - b.z) * c); v.w = zero ? 0.f : -((a.w - b.w) * c);
      st4(dr + 4 * j, v);
      am = fmaxf(am, h2_amax4(v));
    }
    if (xo.p) planes_of_row(dr, nv, xo, row, am, red);
  }
}

// v[k] <- p_k - mean over the members, formed on the differences d_k = v_k - v_0: dev_k = d_k - mean(d).  Members that agree to a few
// ulps -- where v_0 + mean(d) would round the mean to fp32 of the VALUES and leave deviations wrong by up to half an ulp of them, i.e. by
// their own size -- keep deviations accurate to an ulp of the DIFFERENCES (d_k is exact for neighbours); identical members give exactly 0
template <int K>
__device__ __forceinline__ void member_deviations(float4* v) {
  const float4 v0 = v[0];
  float4 md = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    v[k] = make_float4(v[k].x - v0.x, v[k].y - v0.y, v[k].z - v0.z, v[k].w - v0.w);
    md.x += v[k].x; md.y += v[k].y; md.z += v[k].z; md.w += v[k].w;
  }
  md.x *= 1.f / K; md.y *= 1.f / K; md.z *= 1.f / K; md.w *= 1.f / K;
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = make_float4(v[k].x - md.x, v[k].y - md.y, v[k].z - md.z, v[k].w - md.w);
}

// r[m] = mean_e var_k p[k][m][e] (unbiased over the K members): per element two passes over the K values held in registers
// (deviations from the mean, then their squares)
template <int K>
__global__ __launch_bounds__(256) void ens_var_fwd_kernel(const float* __restrict__ p, long member, long ld, float* __restrict__ r,
                                                          int M, int N) {
  __shared__ float red[8];
  const int nv = N >> 2;
  for (long row = blockIdx.x; row < M; row += gridDim.x) {
    const float* pr = p + row * ld;
    float s = 0.f;
    for (int j = threadIdx.x; j < nv; j += 256) {
      float4 v[K];
#pragma unroll
      for (int k = 0; k < K; ++k) v[k] = ld4(pr + k * member + 4 * j);
      member_deviations<K>(v);
      float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int k = 0; k < K; ++k) { q.x += v[k].x * v[k].x; q.y += v[k].y * v[k].y; q.z += v[k].z * v[k].z; q.w += v[k].w * v[k].w; }
      s += (q.x + q.y) + (q.z + q.w);
    }
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) r[row] = s / (float)(K - 1) / (float)N;
  }
}

// dp[k][m][e] = g[m] 2 (p_k - mean_k) / ((K - 1) E) (g == NULL: 1).  dp may be NULL when planes are asked for (planes only): the second
// sweep recomputes the values from p (L2) either way, so the fp32 copy is pure output.
template <int K>
__global__ __launch_bounds__(256) void ens_var_bwd_kernel(const float* __restrict__ g, const float* __restrict__ p, long member, long ld,
                                                          float* __restrict__ dp, long dmember, long lddp, int M, int N, PlaneOut xo,
                                                          long pmember, long imember) {
  __shared__ float red[8];
  const int nv = N >> 2;
  for (long row = blockIdx.x; row < M; row += gridDim.x) {
    const float* pr = p + row * ld;
    const float c = (g ? g[row] : 1.f) * (2.f / ((float)(K - 1) * (float)N));
    float am[K];
#pragma unroll
    for (int k = 0; k < K; ++k) am[k] = 0.f;
    for (int sweep = 0; sweep < (xo.p ? 2 : 1); ++sweep) {
      float sc[K];
      if (sweep == 1) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float inv = h2_inv_of(block_max_256(am[k], red));
          sc[k] = h2_scale_of(inv);
          if (threadIdx.x == 0) xo.inv[k * imember + row] = inv;
        }
      }
      for (int j = threadIdx.x; j < nv; j += 256) {
        float4 v[K];
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = ld4(pr + k * member + 4 * j);
        member_deviations<K>(v);
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float4 d = make_float4(v[k].x * c, v[k].y * c, v[k].z * c, v[k].w * c);
          if (sweep == 0) {
            if (dp) st4(dp + k * dmember + row * lddp + 4 * j, d);
            am[k] = fmaxf(am[k], h2_amax4(d));
          } else {
            h2_store4(PlaneOut{xo.p + k * pmember, xo.ld, xo.plane, nullptr}, row, 4 * j, d, sc[k]);
          }
        }
      }
    }
  }
}

}  // namespace

extern "C" {

int genrl_l2err_fwd(const float* t, long ldt, const float* p, long ldp, float* err, int M, int N, void* stream) {
  GENRL_ENTER();
  if (M <= 0) return GENRL_OK;
  if (N <= 0 || (N & 3) || (ldt & 3) || (ldp & 3) || ldt < N || ldp < N || !t || !p || !err || !aligned16(t) || !aligned16(p))
    return GENRL_EINVAL;
  l2err_fwd_kernel<<<row_grid(M, ENS_GRID), 256, 0, (hipStream_t)stream>>>(t, ldt, p, ldp, err, M, N);
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

int genrl_l2err_bwd(const float* g, const float* err, const float* t, long ldt, const float* p, long ldp, float* dp, long lddp, int M,
                    int N, uint16_t* dpp, long ldpl, long plane, float* inv, void* stream) {
  GENRL_ENTER();
  if (M <= 0) return GENRL_OK;
  if (N <= 0 || (N & 3) || (ldt & 3) || (ldp & 3) || (lddp & 3) || ldt < N || ldp < N || lddp < N || !g || !err || !t || !p || !dp ||
      !aligned16(t) || !aligned16(p) || !aligned16(dp) || bad_planes(dpp, ldpl, inv, N))
    return GENRL_EINVAL;
  l2err_bwd_kernel<<<row_grid(M, ENS_GRID), 256, 0, (hipStream_t)stream>>>(g, err, t, ldt, p, ldp, dp, lddp, M, N, PlaneOut{dpp, ldpl, plane, inv});
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

#define ENS_DISPATCH(KERNEL, ...)                                                                                     \
  switch (K) {                                                                                                        \
    case 2: KERNEL<2><<<row_grid(M, ENS_GRID), 256, 0, (hipStream_t)stream>>>(__VA_ARGS__); break;                    \
    case 3: KERNEL<3><<<row_grid(M, ENS_GRID), 256, 0, (hipStream_t)stream>>>(__VA_ARGS__); break;                    \
    case 4: KERNEL<4><<<row_grid(M, ENS_GRID), 256, 0, (hipStream_t)stream>>>(__VA_ARGS__); break;                    \
    case 5: KERNEL<5><<<row_grid(M, ENS_GRID), 256, 0, (hipStream_t)stream>>>(__VA_ARGS__); break;                    \
    case 6: KERNEL<6><<<row_grid(M, ENS_GRID), 256, 0, (hipStream_t)stream>>>(__VA_ARGS__); break;                    \
    case 7: KERNEL<7><<<row_grid(M, ENS_GRID), 256, 0, (hipStream_t)stream>>>(__VA_ARGS__); break;                    \
    default: KERNEL<8><<<row_grid(M, ENS_GRID), 256, 0, (hipStream_t)stream>>>(__VA_ARGS__); break;                   \
  }

int genrl_ens_var_fwd(const float* p, long member, long ld, int K, float* r, int M, int N, void* stream) {
  GENRL_ENTER();
  if (M <= 0) return GENRL_OK;
  if (K < 2 || K > ENS_MAXK || N <= 0 || (N & 3) || (ld & 3) || (member & 3) || ld < N || !p || !r || !aligned16(p)) return GENRL_EINVAL;
  ENS_DISPATCH(ens_var_fwd_kernel, p, member, ld, r, M, N)
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

int genrl_ens_var_bwd(const float* g, const float* p, long member, long ld, int K, float* dp, long dmember, long lddp, int M, int N,
                      uint16_t* dpp, long pmember, long ldpl, long plane, float* inv, long imember, void* stream) {
  GENRL_ENTER();
  if (M <= 0) return GENRL_OK;
  if (K < 2 || K > ENS_MAXK || N <= 0 || (N & 3) || (ld & 3) || (member & 3) || ld < N || !p || !aligned16(p) || (!dp && !dpp) ||
      (dp && ((lddp & 3) || (dmember & 3) || lddp < N || !aligned16(dp))) || bad_planes(dpp, ldpl, inv, N) || (dpp && (pmember & 3)))
    return GENRL_EINVAL;
  ENS_DISPATCH(ens_var_bwd_kernel, g, p, member, ld, dp, dmember, lddp, M, N, PlaneOut{dpp, ldpl, plane, inv}, pmember, imember)
  GENRL_CHECK_LAUNCH();
  return GENRL_OK;
}

}  // extern "C"
