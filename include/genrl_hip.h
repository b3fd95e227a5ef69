/* genrl_hip.h — C-ABI of libgenrl_hip.so: the MI355X (gfx950) kernels under the GenRL
 * world-model + imagination hot path.
 *
 * The reference (mazpie/genrl) has no FFI of its own: its hot path is Python calling
 * torch.nn / torch.distributions.  This header is the boundary a maintainer binds
 * instead (ctypes stub in INTEGRATION.md; genrl_amd/_lib.py is that stub).  Conventions:
 *   - plain pointers (device memory, fp32 unless stated) and sizes; no torch types;
 *   - `stream` is a hipStream_t passed as void*; entry points only enqueue work on it, never
 *     synchronise and never allocate (workspaces `ws` are caller-provided, sizes from *_ws_floats);
 *   - return 0 on success, 1 invalid argument, 2 launch failure; no exceptions cross the ABI.
 * Each entry cites the reference code (file:line under /root/reference) whose arithmetic it
 * replaces.
 */
#ifndef GENRL_HIP_H
#define GENRL_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- dense products: nn.Linear fwd/dgrad/wgrad (agent/dreamer_utils.py:339-346,734,760,798)
 * C[m,n] = sum_k A[m*a_rs+k*a_ks] * B[n*b_rs+k*b_ks] (+bias[n]) (+C if accumulate);
 * one stride of each operand must be 1.  Matrix pipe per genrl_set_gemm_precision below (fp32: v_mfma_f32_16x16x4_f32 on the 64x64 tiles and the skinny kernel,
 * six v_mfma_f32_32x32x16_bf16 on exactly split operands on the 128x128 tiles).
 * Shapes with few output tiles and a long reduction (the M=N=1024 GEMMs, the conv weight
 * gradients) are split over K into `ws` (>= genrl_sgemm_ws_floats(M,N,K) floats; pass NULL/0 to
 * disable) and reduced deterministically.
 * Padded lines: an operand whose lines (rows of a k-contiguous operand, k-lines of a row-contiguous one) are a
 * multiple of 4 floats apart, 16-byte aligned and at least roundup4(extent) long is read with 16-byte loads
 * up to the end of the padded line (extent = 255 in rows of 256: element 255 of every line is read and
 * ignored), so the padding must be addressable; every other layout takes the scalar-load kernel. */
long genrl_sgemm_ws_floats(int M, int N, int K);
/* Arithmetic of the MFMA GEMMs (process-wide; returns the previous setting; initial value from GENRL_GEMM_MODE, default 2):
 *   0  fp32 MFMAs everywhere.
 *   2  fp32 (default): as 0, except that the 128x128-tile kernels split every fp32 operand element exactly into three
 *      bf16 terms and sum the six largest bf16-MFMA cross products in fp32 -- error of the size of fp32 rounding.
 *   3  the same split on every tile (slower on the 64x64 tile; for experiments).
 *   1  precision 16: the operands are rounded to bf16 (nearest even) on their way into the matrix cores, products
 *      accumulate in fp32 and every tensor stays fp32 in memory -- the reference's `precision: 16` autocast mode
 *      (agent/dreamer_utils.py:889-932) without a gradient scaler, which bf16's fp32 exponent range makes unnecessary. */
int genrl_set_gemm_precision(int mode);
/* matrix pipe the most recent genrl_sgemm / genrl_sgemm_conv launch ran on (measurement: bench.py prices each pipe against
 * its own peak): 0 fp32 MFMA, 1 bf16-rounded operands, 3 fp32 operands split into three bf16 terms (six bf16 MFMAs) */
int genrl_sgemm_last_pipe(void);
/* the mode genrl_set_gemm_precision last selected (the fused row kernels that contain a small matrix product -- the policy's
 * output layer inside the Normal-head kernels -- round their operands to bf16 in mode 1 as well) */
int genrl_gemm_precision(void);
int genrl_sgemm(const float* A, long a_rs, long a_ks, const float* B, long b_rs, long b_ks, float* C, long ldc,
                const float* bias, int M, int N, int K, int accumulate, float* ws, long ws_floats, void* stream);

/* The same product with ONE operand read as the implicit patch matrix of a stride-2 k x k convolution
 * over an NHWC image (N, img_h, img_w, img_c) -- replaces F.unfold-style patch materialisation for
 * nn.Conv2d forward / weight gradient (agent/dreamer_utils.py:604-621) and the nn.ConvTranspose2d
 * input / weight gradients (:686-706).  which = 1: A (k-contiguous, a_ks = 1) is the (pixels x k*k*C)
 * patch matrix of the image at `A`, B k-contiguous;  which = 2: A and B row-contiguous, B is the patch
 * matrix (K = pixels, N = k*k*C) of the image at `B`.  Patch column order (kh, kw, c).  Requires
 * img_c % 4 == 0 and 16-byte aligned operands (returns 1 otherwise). */
int genrl_sgemm_conv(const float* A, long a_rs, long a_ks, const float* B, long b_rs, long b_ks, float* C, long ldc,
                     const float* bias, int M, int N, int K, int accumulate, float* ws, long ws_floats, int which,
                     int img_h, int img_w, int img_c, int ksize, void* stream);

/* ---- the same products on PRE-SPLIT operands (genrl_amd/csrc/gemm_planes.hip): no conversion work in the K loop, the operand
 * planes go global -> LDS by DMA and LDS -> matrix cores.
 *
 * "h2 planes" (the product path: the imagination rollout and the policy's batched backward): a row of an fp32 operand is
 * scaled by a power of two s (its largest magnitude lands in [2^14, 2^15)), every element a s is held as two fp16 numbers
 * h + l / 2^11 (h = fp16(a s), l = fp16((a s - h) 2^11), round to nearest even: 22 + 2 implicit mantissa bits, representation
 * error <= 2^-22 |a| and ~2^-24 |a| typical for elements within 2^-28 of the row maximum), inv[row] = 1 / s undoes the
 * scaling.  Operand = two planes of fp16 [rows][ld] (`plane` elements apart, k-contiguous, ld % 64 == 0, zero padded along
 * k) + inv[rows].  The product sums h_a h_b + (h_a l_b + l_a h_b) / 2^11 (three v_mfma_f32_32x32x16_f16 per block and k-step,
 * the magnitude classes in separate fp32 accumulators) and multiplies by ainv[m] binv[n]: the error of an fp32-MFMA product
 * (tests/test_gpu_planes.py) at 3/16 of its matrix-core cycles.  An Inf operand gives NaN (Inf - Inf in the residual).
 * genrl_split_h2: fp32 (R x Cn, row stride ldx) -> planes [R][ld_out] + inv[R], or those of the TRANSPOSE ([Cn][ld_out],
 * inv[Cn]: weights for the dgrad products), zero padded up to ld_out columns.
 * genrl_gemm_h2: C (M x N fp32, row stride ldc) (+)= A0 B0^T + A1 B1^T (+ bias); k0, k1 multiples of 64 (k1 may be 0):
 * two operand segments = Linear over a concatenated input (agent/dreamer_utils.py:461-462,777) in one launch; the
 * accumulators are rescaled by an exact power of two per element where the segments' row scales differ.
 *
 * "x3 planes" (kept as the exactly-representing variant, scripts/h2_bench.py compares the two): three bf16 planes h + m + l = a
 * (exact), six v_mfma_f32_32x32x16_bf16 per block and k-step, no row scaling. */
int genrl_split_h2(const float* x, long ldx, int R, int Cn, uint16_t* out, long ld_out, long plane, float* inv, int transpose,
                   void* stream);
int genrl_gemm_h2(const uint16_t* a0, long a0_ld, long a0_plane, const float* a0_inv, const uint16_t* b0, long b0_ld, long b0_plane,
                  const float* b0_inv, int k0, const uint16_t* a1, long a1_ld, long a1_plane, const float* a1_inv,
                  const uint16_t* b1, long b1_ld, long b1_plane, const float* b1_inv, int k1,
                  float* C, long ldc, const float* bias, int M, int N, int accumulate, void* stream);
/* Two one-segment products on ONE A operand in one launch: C0 (+)= A B0^T (M x N0) and C1 (+)= A B1^T (M x N1), no bias (the two dgrads of
 * one gradient: the imagination rollout's GRU backward).  Column tile t < N0 / 64 of the launch belongs to product 0, the rest to product 1;
 * each tile runs genrl_gemm_h2's 64x64 tile body on its own product's (B, C, ldc, accumulate): each C is bitwise what its own genrl_gemm_h2
 * launch gives.  The tile order places both products' tiles of a row panel on the same XCDs, so that A is fetched once per XCD.
 * GENRL_EINVAL -- the caller launches the two products itself -- unless N0 % 64 == 0 and genrl_gemm_h2 would run both products on the
 * three-stage 64x64 instantiation (fewer than 2048 tiles each; not 257+ tiles with k <= 1536).  A launch of more than 256 such tiles that
 * 128x64 tiles cover in 225 .. 256 workgroups runs on those (the same tile -> product map and the same bits; GENRL_PLANES_RECT=0: never). */
int genrl_gemm_h2_pair(const uint16_t* a, long a_ld, long a_plane, const float* a_inv, int k,
                       const uint16_t* b0, long b0_ld, long b0_plane, const float* b0_inv, float* C0, long ldc0, int N0, int accumulate0,
                       const uint16_t* b1, long b1_ld, long b1_plane, const float* b1_inv, float* C1, long ldc1, int N1, int accumulate1,
                       int M, void* stream);
/* genrl_gemm_h2 (one segment) whose output rows are the logits of N / 32 categorical latents of 32 classes (the RSSM prior head
 * inside the imagination rollout, agent/dreamer_utils.py:466-470,177-197): the same launch also takes the unimix softmax +
 * exponential-race sample of every latent (argmax_k pn_k / q_k, first maximum wins) from the logits it has just formed and
 * writes the one-hot rows `sample` and, if sp != NULL, their h2 planes (scale 2^14, sinv[row] = 2^-14).  N % 32 == 0;
 * ldc, ldq, lds % 4 == 0; C, bias, q, sample 16-byte aligned. */
int genrl_gemm_h2_sample(const uint16_t* a0, long a0_ld, long a0_plane, const float* a0_inv, const uint16_t* b0, long b0_ld,
                         long b0_plane, const float* b0_inv, int k0, float* C, long ldc, const float* bias, int M, int N,
                         const float* q, long ldq, float unimix, float* sample, long lds, uint16_t* sp, long sld, long splane,
                         float* sinv, void* stream);
/* Dense -> LayerNorm (-> act: GENRL_ACT_*, SiLU or ELU) in ONE launch (round 6; replaces genrl_gemm_h2 + genrl_ln_act_fwd_h2 for the MLP / img_step layers of
 * agent/dreamer_utils.py:718-747, :459-473 at <= 1024 columns): C = A0 B0^T (+ A1 B1^T) + bias as genrl_gemm_h2 (C keeps the pre-activation the
 * LayerNorm backward reads), then y = act(LayerNorm(C) gamma + beta) as fp32 rows (y may be NULL) and as h2 planes with ONE scale for the
 * whole tensor (the bound max|gamma| sqrt(N) + max|beta|; yinv[row] holds the same value in every row), mean / rstd [M].  A LayerNorm row spans
 * the N / 64 column tiles of its 64-row block: the launch places those workgroups on ONE XCD (the dispatcher deals workgroups round-robin; the kernel reads its XCD id) and they exchange
 * partial row statistics through that XCD's L2 -- no fence, no cache write-back or invalidate, no atomic: every tile stores its rows' records
 * {mean, tag, M2, tag} (one 16-byte store each) and reads its peers' with L2-served loads until all carry this launch's tag (the tag counts the
 * slot's launches; profiles/r06_xcd_barrier.txt: a counter barrier of 16 workgroups inside one XCD costs 0.7 us, a chip-wide one 3.9).
 * genrl_gemm_h2_ln_ok(M, N): N % 64 == 0, N <= 1024 and all cdiv(M, 64) N / 64 workgroups resident at once, at most 32 per XCD (1024 rows at
 * N = 1024).  gamma / beta / C / y / part 16-byte aligned; ldc / ldy / yld % 4 == 0.  part: genrl_gemm_h2_ln_part_floats(M, N) floats, ZEROED
 * ONCE by the caller and then owned by the launches of one stream (the record tags live there).  sync: genrl_gemm_h2_ln_sync_words() uint32
 * words, zeroed once; sync[0] != 0 after a launch: the exchange timed out (bounded spin, no hang) -- the results are invalid and part / sync must
 * be zeroed again.  Two such launches must not run concurrently (each would wait for workgroups the other keeps off the CUs): the caller
 * uses it on one stream at a time. */
int genrl_gemm_h2_ln_ok(int M, int N);
long genrl_gemm_h2_ln_part_floats(int M, int N);
long genrl_gemm_h2_ln_sync_words(void);
int genrl_gemm_h2_ln(const uint16_t* a0, long a0_ld, long a0_plane, const float* a0_inv, const uint16_t* b0, long b0_ld, long b0_plane,
                     const float* b0_inv, int k0, const uint16_t* a1, long a1_ld, long a1_plane, const float* a1_inv,
                     const uint16_t* b1, long b1_ld, long b1_plane, const float* b1_inv, int k1,
                     float* C, long ldc, const float* bias, int M, int N, const float* gamma, const float* beta, float eps, int act,
                     float* y, long ldy, float* mean, float* rstd, uint16_t* yp, long yld, long yplane, float* yinv,
                     float* part, unsigned* sync, void* stream);
/* UNIFORM-scale h2 planes (one power-of-two scale for the whole tensor, inv[row] the same in every row): what the convolution
 * products need -- a patch row gathers from several pixel rows, a weight gradient sums over them (csrc/gemm_planes*.hip).
 * genrl_split_h2u: from an fp32 matrix, exact tensor maximum (two launches; ws >= 1024 floats).  genrl_ln_act_fwd_h2u: the channel
 * LayerNorm (+SiLU / ELU, rows of <= 256 floats, agent/dreamer_utils.py:1031-1040) emits them itself with the scale its parameters
 * guarantee (|gamma x^ + beta| <= max|gamma| sqrt(N) + max|beta|); y == NULL: planes only (an inner layer's fp32 activation has no reader
 * when the next convolution gathers from the planes forward and backward).  genrl_ln_act_bwd_h2u: its backward leaves one partial maximum
 * of dx per workgroup in amax_ws (>= 2048 floats), a second launch splits dx with the tensor's scale. */
int genrl_split_h2u(const float* x, long ldx, int R, int Cn, uint16_t* out, long ld_out, long plane, float* inv, float* ws,
                    void* stream);
int genrl_ln_act_fwd_h2u(const float* x, long ldx, const float* gamma, const float* beta, float* y, long ldy, float* mean,
                         float* rstd, int M, int N, float eps, int act, uint16_t* yp, long ldp, long plane, float* inv,
                         void* stream);
int genrl_ln_act_bwd_h2u(const float* dy, long lddy, const float* x, long ldx, const float* gamma, const float* beta,
                         const float* mean, const float* rstd, float* dx, long lddx, float* dgamma, float* dbeta, float* dcolsum,
                         float* ws, int M, int N, int act, int accumulate_params, uint16_t* dxp, long ldp, long plane, float* inv,
                         float* amax_ws, void* stream);
/* A conv layer WITHOUT a channel-LayerNorm (`encoder.norm: none` / `decoder.norm: none`: Conv2d + bias, NormLayer('none'), act;
 * agent/dreamer_utils.py:587, :669): the activation alone over M pixel rows of N channels, rows ld* floats apart.
 * genrl_chan_act_fwd_h2u: y = act(x), act = GENRL_ACT_SILU or GENRL_ACT_ELU (any other code, 0 included: 1 before any launch).  With
 * yp != NULL also UNIFORM planes of y: the launch leaves one partial maximum of |y| per workgroup in amax_ws (>= 2048 floats), a second
 * launch reduces them and splits the stored y -- bit for bit what genrl_split_h2u makes of y; padding columns are written as zeros.
 * genrl_chan_act_bwd_h2u: dx = dy act'(x) and, with db != NULL, db[n] (+)= sum_m dx[m][n] (the conv bias gradient; accumulate 1 adds
 * into db) from per-workgroup partial rows in ws (>= genrl_chan_act_bwd_ws_floats(M, N) floats, 16-byte aligned) summed in a fixed order,
 * no atomics; dxp != NULL: uniform planes of dx as in the forward.
 * Rows of N <= 1024 floats with N % 4 == 0, ld* % 4 == 0 and 16-byte aligned pointers take the lane-group kernels (16 / 32 / 64 lanes per
 * row for N <= 64 / 128 / wider); everything else takes a scalar arm, which has no planes (asking for them returns 1).  M <= 0 returns 0
 * without a launch.  x and y (dy / x and dx) must not overlap. */
int genrl_chan_act_fwd_h2u(const float* x, long ldx, float* y, long ldy, int M, int N, int act, uint16_t* yp, long ldp, long plane,
                           float* inv, float* amax_ws, void* stream);
long genrl_chan_act_bwd_ws_floats(int M, int N);
int genrl_chan_act_bwd_h2u(const float* dy, long lddy, const float* x, long ldx, float* dx, long lddx, float* db, float* ws,
                           int accumulate, int M, int N, int act, uint16_t* dxp, long ldp, long plane, float* inv, float* amax_ws,
                           void* stream);
/* The stride-2 convolution product on planes: C[m, n] (+)= sum_kk patch(m, kk) B[n, kk] (+ bias), the patch matrix of an NHWC image
 * (agent/dreamer_utils.py:604-621 forward; :686-706 input gradient of the transposed convolutions) gathered by the operand DMA
 * itself -- m = (image, oy, ox), kk = (kh k + kw) Cc + c, 16-byte chunks = 8 channels of one pixel.  img: UNIFORM-scale planes
 * [Nimg H W][ld_img] with img_inv the same in every row (genrl_ln_act_fwd_h2u / genrl_split_h2u); Cc % 8 == 0, Cc >= 48;
 * B: planes [N][b_ld] of the (N, k k Cc) weight matrix, b_ld = k k Cc rounded up to 64 (zero padded). */
int genrl_gemm_h2_conv(const uint16_t* img, long ld_img, long plane_img, const float* img_inv, int Nimg, int H, int W, int Cc, int k,
                       const uint16_t* b, long b_ld, long b_plane, const float* b_inv, float* C, long ldc, const float* bias, int N,
                       int accumulate, void* stream);
/* Gather ("sub-pixel") form of a stride-2 transposed convolution with an even kernel k = 2T -- nn.ConvTranspose2d(k, 2) forward
 * (agent/dreamer_utils.py:686-706) and, with the channel roles swapped, the input gradient of nn.Conv2d(k, 2) (:590-612): all four
 * output parity classes (a, b) read the SAME T x T patch of the zero-padded input, so ONE product with rows (image, py, px) and
 * columns (a, b, co) does the layer and the epilogue writes straight to out[n][2 py + a][2 px + b][co] (no cols matrix, no col2im):
 *   out[n][2 py + a][2 px + b][co] = bias[(a, b, co)] + sum_{u, v, c} img[n][py + u][px + v][c] * B[(a, b, co)][(u, v, c)]
 * img: UNIFORM-scale planes of the input zero-padded by T - 1 pixels on every side, [Nimg][Hp][Wp][ld_img] (genrl_pad_planes);
 * B: planes [4 Co][b_ld] of the rearranged weight (genrl_subpixel_weight), b_ld = T T Cc rounded up to 64; bias: 4 Co floats or NULL.
 * out: fp32 NHWC [Nimg][Ho][Wo][Co]; positions beyond Ho / Wo are dropped, positions no patch reaches are not written.
 * Cc % 8 == 0, Cc >= 48, Co % 4 == 0, out and bias 16-byte aligned. */
int genrl_gemm_h2_subpixel(const uint16_t* img, long ld_img, long plane_img, const float* img_inv, int Nimg, int Hp, int Wp, int Cc, int T,
                           const uint16_t* b, long b_ld, long b_plane, const float* b_inv, float* out, int Ho, int Wo, int Co,
                           const float* bias, void* stream);
/* Zero-padded copy of NHWC planes: dst[p][n][y + pad][x + pad][:ld] = src[p][n][y][x][:ld], the border pixels zero (both planes);
 * dinv[0 .. Nimg (H + 2 pad)(W + 2 pad)) = sinv[0] (uniform scale).  ld % 8 == 0. */
int genrl_pad_planes(const uint16_t* src, long splane, const float* sinv, uint16_t* dst, long dplane, float* dinv, int Nimg, int H, int W,
                     long ld, int pad, void* stream);
/* fp32 values of h2 planes: y[r][c] = (h + l / 2^11) inv[r], rows x cols (cols % 4 == 0, y 16-byte aligned, ldy % 4 == 0).  Used when an
 * inner convolution layer's channel-LayerNorm (agent/dreamer_utils.py:590-612, 686-706) wrote ONLY the planes of its output and a consumer
 * off the plane path reads fp32 after all. */
int genrl_planes_to_f32(const uint16_t* p, long ld, long plane, const float* inv, float* y, long ldy, long rows, int cols, void* stream);
/* The rearranged weight of genrl_gemm_h2_subpixel as an fp32 matrix [4 Co][T T Ci] (+ the bias repeated per class, 4 Co floats, if
 * bias4 != NULL):  Wsub[(a, b, co)][(u, v, ci)] = w(ci, co, a + 2 (T - 1 - u), b + 2 (T - 1 - v)), zero where a tap index reaches k
 * (odd k: the kernel is treated as k + 1 with a zero last tap).  w(ci, co, kh, kw) = W[ci s_ci + co s_co + (kh k + kw) s_tap]:
 * nn.ConvTranspose2d's (Ci, Co, k, k) layout has (s_ci, s_co, s_tap) = (Co k k, k k, 1), its channel-last permutation (ci, kh, kw, co)
 * (k k Co, 1, Co); for the input gradient of nn.Conv2d -- summed channel = Cout, produced channel = Cin -- pass Ci := Cout, Co := Cin
 * and the strides of (cout, cin) in the weight's storage. */
int genrl_subpixel_weight(const float* W, long s_ci, long s_co, long s_tap, int Ci, int Co, int k, int T, float* Wsub, const float* bias,
                          float* bias4, void* stream);
/* The first encoder layer straight from the u8 frames (agent/dreamer_utils.py:604-621 with WorldModel.preprocess :139-151 fused): nn.Conv2d(3 -> Co,
 * k = 4, stride 2) on x / 255 - 0.5; in u8 NCHW [Nimg][3][Hi][Wi], Wp = the weight permuted to (co, kh, kw, c), y fp32 [Nimg Ho Wo][Co] (+ bias).  The
 * MFMA operands are read from the frames themselves (no patch matrix); exact fp32 arithmetic, the same per element as genrl_im2col_s2 mode 2 + genrl_sgemm.
 * genrl_conv1_u8_wgrad: dWp[co][(kh, kw, c)] = sum over the pixels of dy[m][co] patch(m)[..] (ws: genrl_conv1_u8_wgrad_ws_floats(Co) floats; summed in a
 * fixed order).  Supported: Co = 48, k = 4, Wi even, frames 2-byte / y, dy 16-byte aligned; GENRL_EINVAL otherwise. */
int genrl_conv1_u8_fwd(const uint8_t* in, const float* Wp, const float* bias, float* y, int Nimg, int Hi, int Wi, int Co, int k, void* stream);
long genrl_conv1_u8_wgrad_ws_floats(int Co);
int genrl_conv1_u8_wgrad(const uint8_t* in, const float* dy, float* dWp, float* ws, int Nimg, int Hi, int Wi, int Co, int k, void* stream);
/* nn.ConvTranspose2d(Ci -> Co, k, stride 2) forward for Co <= 4 output channels -- the decoder's last layer
 * (agent/dreamer_utils.py:686-706) -- in gather form on the fp32 matrix cores (csrc/conv.hip): every wave owns 16 consecutive patch
 * positions, all four output parity classes x Co channels are the 16 MFMA columns, the weights live in registers; exact fp32, no cols
 * matrix, no col2im.  x fp32 NHWC [Nimg][Hi][Wi][Ci], Wp = the weight permuted to (ci, kh, kw, co), bias[Co] or NULL; out fp32
 * [Nimg][Co][Ho][Wo] (out_nchw != 0) or [Nimg][Ho][Wo][Co], Ho = 2 (Hi - 1) + k.  Supported: k = 6, Ci = 48; GENRL_EINVAL otherwise. */
int genrl_convt_small_co_fwd(const float* x, const float* Wp, const float* bias, float* out, int Nimg, int Hi, int Wi, int Ci, int Co,
                             int k, int out_nchw, void* stream);
/* Backward of genrl_convt_small_co_fwd for an NCHW output gradient dy [Nimg][Co][Ho][Wo] (the decoder's frames): the input gradient dx
 * (fp32 NHWC [Nimg][Hi][Wi][Ci]; NULL: skipped) and the weight gradient dWp ([Ci][k k Co], the permuted weight's own layout; NULL: skipped)
 * with the patch operands gathered from dy itself on the fp32 matrix cores -- no im2col matrix.  ws: genrl_convt_small_co_bwd_ws_floats
 * floats (per-workgroup partial weight gradients, summed in workgroup order: deterministic).  Supported: k = 6, Ci = 48, Co = 3. */
long genrl_convt_small_co_bwd_ws_floats(int Ci, int Co);
int genrl_convt_small_co_bwd(const float* x, const float* Wp, const float* dy, float* dx, float* dWp, float* ws, int Nimg, int Hi, int Wi,
                             int Ci, int Co, int k, void* stream);
/* ---- sequence-level entry points (csrc/seq.hip; SURVEY 8b rssm_observe_seq): the per-step launch loops of the RSSM scans
 * (EnsembleRSSM.observe, agent/dreamer_utils.py:362-371, 425-457; VideoSSM.update, agent/video_utils.py:150-187) run from ONE call --
 * the same launches in the same order as the per-step entry points above (bit-identical), without ~20 us of host work per launch.
 * forward: pre (T, B, 3D) holds x_t W_x^T on entry, the full pre-activations on return; Wh = the recurrent block of the (3D, I + D)
 * weight (row stride ldw); mask (T, B) or NULL with hm (T, B, D) = masked previous states (hm[0] prepared by the caller).
 * backward: dha / dhb ping-pong d(hm_t); pa / pb (S, B, D) K-split slabs (S = 0: none); *final_dh / *final_parts (host ints) name the
 * buffers that hold d(hm_0)'s direct part / remaining slabs.  ws: genrl_gru_seq_ws_floats(B, D); gws: genrl_gru_ws_floats(B, D). */
long genrl_gru_seq_ws_floats(int B, int D);
int genrl_gru_seq_fwd(float* pre, const float* Wh, long ldw, const float* gamma, const float* beta, const float* h0, const float* mask,
                      float* out, float* hm, float* mean, float* rstd, float* ws, long ws_floats, int T, int B, int D, float eps,
                      void* stream);
int genrl_gru_seq_bwd(const float* dout, const float* pre, const float* Wh, long ldw, const float* gamma, const float* beta, const float* h0,
                      const float* mask, const float* out, const float* hm, const float* mean, const float* rstd, float* dpre, float* dha,
                      float* dhb, float* pa, float* pb, int S, float* dgamma, float* dbeta, int direct, float* gws, float* ws,
                      long ws_floats, int T, int B, int D, int* final_dh, int* final_parts, void* stream);
/* The imagination rollout's H-step launch loop in C (csrc/seq.hip; SURVEY 8b imagine_seq; WorldModel.imagine, agent/dreamer.py:254-287,
 * with the policy of ActorCritic, :323-350): per step the policy's L Dense + LayerNorm + SiLU layers and its output layer + Normal head,
 * then img_step -- [stoch | action] -> hidden, [hidden | deter] -> GRU gates, deter -> hidden -> prior logits + categorical sample -- on
 * plane operands: 16 launches per step (10 with r->ln_sync, below), exactly those of genrl_amd/ops_planes.py::_RolloutPlanes.forward in the same order (bit-identical),
 * from ONE host call.  All buffers are the caller's (genrl_rollout names them); time-major rows h N + n; planes rows likewise. */
/* BINDING GRAMMAR.  genrl_amd/_lib.py builds the ctypes classes of every argument struct from this text (there is no second definition),
 * and refuses -- it never skips -- a declaration outside this grammar:
 *   typedef struct { DECL ... } genrl_NAME;            no tag, no nesting of anonymous structs / unions, defined before its first use
 *   DECL    = [const] BASE NAME[, NAME ...];           scalars and earlier genrl_* structs by value; each NAME may carry one [N], N a literal
 *           | [const] BASE* NAME; | [const] BASE* NAME[N];     ONE declarator per pointer declaration, the star written against the type
 *   BASE    = int | unsigned | long | float | uint16_t | an earlier genrl_NAME  (pointers also: void)
 * No bit-fields, function pointers, pointers to pointers, enums, macros or preprocessor conditionals inside a struct; comments anywhere.
 * A function parameter `const genrl_NAME*` binds as a pointer to that class: a call with another struct is a Python TypeError. */
typedef struct { const uint16_t* p; long ld, plane; const float* inv; } genrl_planes_ref;    /* h2 planes [2][rows][ld] + inverse row scales */
typedef struct {
  int H, N, S, K, D, A, AP, U, L;                 /* horizon, rows, latents, classes, deter, action dim (AP: padded to 4), hidden, policy layers (<= 8) */
  float unimix, min_std, max_std;
  float* stoch; float* deter; float* logit; float* action; float* raws;      /* (H+1,N,S K) (H+1,N,D) (H+1,N,S K) (H+1,N,AP) (H,N,2A) */
  const float* eps; const float* q;                                           /* policy noise (H,N,A), sampling noise (H,N,S K) */
  genrl_planes_ref stoch_p, deter_p, act_p, x_p, o_p;                          /* (H+1) N rows each for the states / actions; N rows for x, o */
  float* x_pre; float* x; float* g_pre; float* o_pre; float* o;                /* (H,N,U) (N,U) (H,N,3D) (H,N,U) (N,U) */
  float* xm; float* xr; float* gm; float* gr; float* om; float* orr;           /* LayerNorm statistics, (H,N) each */
  genrl_planes_ref w_in_s, w_in_a, w_g_x, w_g_h, w_out, w_dist;               /* frozen world-model weights as planes */
  const float* in_b; const float* in_g; const float* in_be; float in_eps;
  const float* gru_g; const float* gru_be;
  const float* out_b; const float* out_g; const float* out_be; float out_eps;
  const float* dist_b;
  genrl_planes_ref pw0s, pw0d;                                                /* policy layer 0: the stoch / deter column blocks of its weight */
  genrl_planes_ref pw[8]; const float* pb[8]; const float* pg[8]; const float* pbe[8]; float peps[8]; int pU[8];
  float* ppre[8]; float* py[8]; float* pmean[8]; float* prstd[8]; genrl_planes_ref pyp[8];    /* py[l], l < L - 1, may be NULL: planes only */
  const float* head_w; const float* head_b;
  /* round 6: Dense -> LayerNorm in ONE launch (genrl_gemm_h2_ln) for the policy layers, img_in and img_out where genrl_gemm_h2_ln_ok(N, width):
   * 10 launches per step instead of 16.  ln_sync == NULL: the 16-launch form.  ln_part / ln_sync: genrl_gemm_h2_ln's workspaces. */
  float* ln_part; unsigned* ln_sync;
} genrl_rollout;
int genrl_imagine_seq_fwd(const genrl_rollout* r, void* stream);
/* ... and its backward through the frozen dynamics (the dgrad chain of _RolloutPlanes.backward, same order; 8 launches per step + 1: the two
 * GRU dgrads are one genrl_gemm_h2_pair launch, and with dx_pre_all the head's backward runs once behind the loop): ds / dd
 * (H+1,N,S K) / (H+1,N,D) hold the upstream state gradients on entry and the complete ones on return; dl_in: upstream logit gradients
 * (H+1,N,S K) or NULL; dact_all: upstream action gradients in padded rows (H+1,N,AP) or NULL; d_raw (H,N,2A): the policy output's
 * gradient per step (handed to the policy's batched backward).  Scratch: dlg, dov, do_pre, dx, dx_pre + their planes, dha / dhb.  What only plane
 * products read is written as planes only: dg_pre is never written (may be NULL), dlg only with dl_in (the accumulating form) or where the
 * one-hot backward cannot write planes itself, do_pre may be NULL (genrl_ln_act_bwd_h2).  dx_pre_all (H,N,U) or NULL: a slab per step for
 * d x_pre -- genrl_actor_head_linear_bwd then runs ONCE over all H N rows behind the loop instead of once per step on dx_pre (N,U). */
typedef struct {
  int H, N, S, K, D, A, AP, U;
  float unimix, min_std, max_std;
  const float* logit; const float* deter; const float* raws; const float* eps; const float* x_pre; const float* g_pre; const float* o_pre;
  const float* xm; const float* xr; const float* gm; const float* gr; const float* om; const float* orr;
  float* ds; float* dd; const float* dl_in; const float* dact_all; float* d_raw;
  float* dlg; float* dov; float* do_pre; float* dg_pre; float* dx; float* dx_pre; float* dha; float* dhb;
  genrl_planes_ref dlg_p, dop_p, dg_p, dxp_p;
  genrl_planes_ref wt_dist, wt_out, wt_g_x, wt_g_h, wt_in_s;
  const float* waT;
  const float* out_g; const float* out_be; const float* gru_g; const float* gru_be; const float* in_g; const float* in_be;
  float* dx_pre_all;
} genrl_rollout_bwd;
int genrl_imagine_seq_bwd(const genrl_rollout_bwd* r, void* stream);
/* The same two loops for the fp32-OPERAND rollout (genrl_amd/ops.py::_Rollout: fewer than GENRL_PLANES_MIN_ROWS rows -- the per-GPU sizes
 * under data parallelism): 20 launches per step forward, 14 backward, launch for launch what the Python loops issue (bit-identical).
 * Weights are fp32 matrices here: ws_in (U, S K) / wa (U, AP) = the stoch / padded-action column blocks of img_in's weight, gru_w (3D, U + D),
 * out_w (U, D), dist_w (S K, U), policy layers pw[l] (pU[l], K_l; layer 0: (U, S K + D)), waT (A, U).  ws / ws_floats: workspace for the
 * split-K products (>= the largest genrl_sgemm_ws_floats of the loop's shapes; checked).  Backward fields as in genrl_rollout_bwd. */
typedef struct {
  int H, N, S, K, D, A, AP, U, L;
  float unimix, min_std, max_std;
  float* stoch; float* deter; float* logit; float* action; float* raws; const float* eps; const float* q;
  float* x_pre; float* x; float* g_pre; float* o_pre; float* o;                        /* (H,N,U) (H,N,U) (H,N,3D) (H,N,U) (H,N,U) */
  float* xm; float* xr; float* gm; float* gr; float* om; float* orr;
  const float* ws_in; const float* wa; const float* gru_w; const float* out_w; const float* dist_w;
  const float* in_b; const float* in_g; const float* in_be; float in_eps; const float* gru_g; const float* gru_be;
  const float* out_b; const float* out_g; const float* out_be; float out_eps; const float* dist_b;
  const float* pw[8]; const float* pb[8]; const float* pg[8]; const float* pbe[8]; float peps[8]; int pU[8];
  float* ppre[8]; float* py[8]; float* pmean[8]; float* prstd[8];
  const float* head_w; const float* head_b;
  float* ws; long ws_floats;
  /* backward only */
  float* ds; float* dd; const float* dl_in; const float* dact_all; float* d_raw;
  float* dlg; float* dov; float* do_pre; float* dg_pre; float* dx; float* dx_pre; float* dha; float* dhb; const float* waT;
} genrl_rollout_f32;
int genrl_imagine_seq_f32_fwd(const genrl_rollout_f32* r, void* stream);
int genrl_imagine_seq_f32_bwd(const genrl_rollout_f32* r, void* stream);

/* EnsembleRSSM.observe WITHOUT single_obs_posterior (conf/defaults/dreamer_v3.yaml:5; agent/dreamer_utils.py:362-371 static_scan over
 * obs_step :432-441 = img_step :459-473 + get_post_stoch :443-457): the posterior reads [deter_t, embed_t], so the sampled latent is part
 * of the recurrence.  The caller batches over T what does not feed it (the action half of _img_in + bias: already in xpre; the embed half
 * of _obs_out + bias: already in opre; the prior head: on all deter afterwards); these entries run the remaining chain, eight dependent
 * launches per step each way (csrc/seq.hip says which), from ONE host call.  Time-major buffers:
 *   sm (T, B, SK) masked previous latent of every step (sm_0 = mask_0 stoch_0 is the caller's); xpre / opre / o (T, B, U);
 *   xh (T, B, U + D) = [x_t | hm_t] (right half of row block 0 = mask_0 deter_0 is the caller's); gpre (T, B, 3D); deter (T, B, D);
 *   plog / pst (T, B, SK); q (T, B * S, K) Exp(1) noise; mask (T, B) = 1 - is_first; xm .. orr (T, B) LayerNorm statistics.
 * Weights: w_in_s = the latent block (U x SK, rows ld_in_s apart) of _img_in; w_g (3D x (U + D), ld_g) GRUCell._layer; w_o = the deter
 * block (U x D, rows ld_o apart) of _obs_out; w_d (SK x U) _obs_dist with bias dist_b.  ws: max genrl_sgemm_ws_floats over the step products.
 * Backward (see csrc/seq.hip): dlg (T, B, SK) / dd (T, B, D) hold the direct logit / deter gradients on entry; d_pst may be NULL; all
 * per-step gradients stay in dlg, dov, dopre, dgpre, dxh, dxpre for the caller's batched weight-gradient passes; dgamma / dbeta / gws /
 * direct as genrl_gru_seq_bwd's. */
typedef struct {
  int T, B, S, K, D, U;
  float unimix, in_eps, out_eps;
  const float* w_in_s; long ld_in_s; const float* w_g; long ld_g; const float* w_o; long ld_o; const float* w_d;
  const float* in_g; const float* in_be; const float* gru_g; const float* gru_be; const float* out_g; const float* out_be;
  const float* dist_b; const float* mask; const float* q;
  const float* out_b; int opre_acc;   /* opre_acc 1: opre holds the batched half on entry (observe); 0: opre_t = deter_t w_o^T + out_b (imagine) */
  /* fused forward launches (both NULL / 0: the eight-launch form): idx (T, B, S) int32 scratch + w_in_sT = the latent block of _img_in
   * TRANSPOSED ([S K][U], rows U apart): from step 1 on the latent half of _img_in is a gather fused with its LayerNorm
   * (genrl_onehot_gather_ln_fwd); fuse_sample 1 (K == 32): head product + sample in one launch (genrl_linear_sample32): 6 launches per step */
  int* idx; const float* w_in_sT; int fuse_sample;
  float* sm; float* xpre; float* xh; float* gpre; float* deter; float* opre; float* o; float* plog; float* pst;
  float* xm; float* xr; float* gm; float* gr; float* om; float* orr;
  float* ws; long ws_floats;
  /* backward only */
  const float* d_pst; float* dlg; float* dd; float* dov; float* dopre; float* dgpre; float* dxh; float* dxpre;
  float* dsa; float* dsb; float* dhd_a; float* dhd_b; float* dgamma; float* dbeta; float* gws; int direct;
} genrl_observe;
int genrl_observe_seq_fwd(const genrl_observe* r, void* stream);
int genrl_observe_seq_bwd(const genrl_observe* r, int* final_buf, void* stream);
/* EnsembleRSSM.imagine (agent/dreamer_utils.py:373-381: static_scan over img_step :459-473 for GIVEN actions -- the data-free block's
 * warm-up rollouts, train.py:283-340, report / video_imagine) is the same loop with the prior head in the posterior's place: call
 * genrl_observe_seq_fwd with mask = NULL (no resets), opre_acc = 0, w_o / out_b / out_g / out_be = _ensemble_img_out, w_d / dist_b =
 * _ensemble_img_dist, q = NULL for mode() instead of sample().  Forward only. */
/* Weight-gradient product on the SAME planes (csrc/gemm_planes_tn.hip):  C[i, j] (+)= sum_m A(m, i) B(m, j) for h2 planes
 * A [2][M][a_ld] (columns i < NI) and B [2][M][b_ld] (columns j < NJ) with per-row inverse scales a_inv[M], b_inv[M] -- dW = dY^T X
 * (agent/dreamer_utils.py:739-747 backward) read against the planes' storage order through the transposing LDS read
 * ds_read_b64_tr_b16, the row scales (which sit inside the sum) folded into one operand's fragments as exact powers of two;
 * deterministic split-K over m.  M % 64 == 0; a_ld, b_ld % 64 == 0; with more than one split NJ % 4 == ldc % 4 == 0.
 * ws: genrl_gemm_h2_tn_ws_bytes(NI, NJ, M) bytes of device workspace, 256-byte aligned. */
long genrl_gemm_h2_tn_ws_bytes(int NI, int NJ, int M);
int genrl_gemm_h2_tn(const uint16_t* a, long a_ld, long a_plane, const float* a_inv, const uint16_t* b, long b_ld, long b_plane,
                     const float* b_inv, float* C, long ldc, int NI, int NJ, int M, int accumulate, void* ws, long ws_bytes,
                     void* stream);
/* The convolution weight gradient on planes: genrl_gemm_h2_tn with B(m, j) = the stride-2 patch matrix of an NHWC image held as
 * uniform-scale planes [pixel][ld_img], gathered by the operand DMA: j = (kh k + kw) Cc + c (NJ = k k Cc columns), m = (image, oy, ox).
 * rowoff (uint32, M + 256 entries, the tail repeating the last value): ((n H + 2 oy) W + 2 ox) * ld_img * 2 -- the byte offset of the
 * patch's first pixel row; img_inv: the image's uniform inverse scale per pixel row (>= M entries).  ws as genrl_gemm_h2_tn's for
 * (NI, k k Cc, M).  (agent/dreamer_utils.py:604-621 weight gradient; with A = the input planes and the image = dY: :686-706.) */
int genrl_gemm_h2_tn_conv(const uint16_t* a, long a_ld, long a_plane, const float* a_inv, const uint16_t* img, long ld_img,
                          long plane_img, const float* img_inv, const unsigned* rowoff, int W, int Cc, int k, float* C, long ldc,
                          int NI, int M, int accumulate, void* ws, long ws_bytes, void* stream);
/* the same for n matrices in one launch set (row splits: one launch; transposed splits: two) -- all weights of an optimiser group
 * after its step.  Descriptors are read on the host at call time. */
typedef struct {
  const float* src; long ldx; int R, Cn;         /* fp32 source (R x Cn, row stride ldx) */
  uint16_t* out; long ld_out, plane; float* inv; /* planes [R][ld_out] (or [Cn][ld_out] when transpose) + inverse row scales */
  int transpose;
} genrl_split_desc;
int genrl_split_h2_batch(const genrl_split_desc* descs, int n, void* stream);
int genrl_split_x3(const float* x, long ldx, int R, int Cn, uint16_t* out, long ld_out, long plane, int transpose,
                   void* stream);
int genrl_gemm_x3(const uint16_t* a0, long a0_ld, long a0_plane, const uint16_t* b0, long b0_ld, long b0_plane, int k0,
                  const uint16_t* a1, long a1_ld, long a1_plane, const uint16_t* b1, long b1_ld, long b1_plane, int k1,
                  float* C, long ldc, const float* bias, int M, int N, int accumulate, void* stream);
int genrl_planes_force_tile(int t);      /* experiments: 0 auto, 1 64x64 tiles, 2 128x128 tiles (both formats), 3 64x192, 4 128x64 tiles (h2) */
/* kernel instantiations the most recent plane product entry call (genrl_gemm_h2, _sample, _ln, _conv, _subpixel, _tn, _tn_conv,
 * genrl_gemm_x3) launched, reset by each such call (a refused call reports none): the GENRL_ROUTE_* bits OR-ed in the low 32 bits
 * -- a row-split product or a two-segment 128-tile product reports both of its launches -- and the split-K count of a TN product
 * in the high bits (tests: which route a product took; the launch-log families do not tell the kernels of a family apart) */
long genrl_planes_last_route(void);
#define GENRL_ROUTE_64_NS3        0x1u      /* 64x64 tile, three-stage ring */
#define GENRL_ROUTE_64_NS2        0x2u      /* 64x64 tile, two-stage ring, two workgroups per CU */
#define GENRL_ROUTE_64_SAMPLE     0x4u      /* 64x64 tile with the categorical-sample epilogue */
#define GENRL_ROUTE_64_LN         0x8u      /* 64x64 tile with the LayerNorm epilogue */
#define GENRL_ROUTE_128_PLAIN     0x10u     /* 128x128 tile, two whole stages (GENRL_PLANES_HL=0) */
#define GENRL_ROUTE_128_HL        0x20u     /* 128x128 tile, plane-alternating half stages */
#define GENRL_ROUTE_128_HLW       0x40u     /* 128x192 tile, half stages */
#define GENRL_ROUTE_CONV_PLAIN    0x80u
#define GENRL_ROUTE_CONV_HL       0x100u
#define GENRL_ROUTE_CONV_HLW      0x200u
#define GENRL_ROUTE_CONV_TALL96   0x400u    /* 256x96 tile */
#define GENRL_ROUTE_SUBPIXEL_HL   0x800u
#define GENRL_ROUTE_SUBPIXEL_HLW  0x1000u
#define GENRL_ROUTE_X3_64         0x2000u
#define GENRL_ROUTE_X3_128        0x4000u
#define GENRL_ROUTE_TN            0x8000u
#define GENRL_ROUTE_TN_CONV       0x10000u
#define GENRL_ROUTE_64X192        0x20000u  /* 64x192 tile, four plane-alternating half stages: one round of 225 .. 256 workgroups */
#define GENRL_ROUTE_128X64        0x40000u  /* 128x64 tile, three-stage ring (also the pair of products): one round of 225 .. 256 workgroups */

/* Row kernels with an additional h2-plane output (the operand of the next genrl_gemm_h2): same arithmetic and fp32
 * outputs as the entry points without the suffix (documented below), plus planes [.][ldp] `plane` elements apart and
 * inv[row] (the row maximum is taken over the kernel's output row).  ldp % 4 == 0, ldp >= row length; columns beyond the
 * row length are left untouched (callers zero them once).  genrl_ln_act_fwd_h2 with 256 < N <= 4096 (16-byte aligned operands) accepts
 * y == NULL: planes only (the fp32 copy has no reader when every consumer takes the planes: 5.9 -> 5.4 us at 1 024 x 1 024, 34.8 -> 28.0 at
 * 16 384 rows).  genrl_ln_act_bwd_h2 with 256 < N <= 4096 accepts dx == NULL: planes
 * only (the fp32 copy has no reader when dgrad AND weight gradient run on planes). */
int genrl_ln_act_fwd_h2(const float* x, long ldx, const float* gamma, const float* beta, float* y, long ldy, float* mean,
                        float* rstd, int M, int N, float eps, int act, uint16_t* yp, long ldp, long plane, float* inv,
                        void* stream);
/* Deferred parameter-gradient reductions of the LayerNorm backward: with accumulate_params & 4 genrl_ln_act_bwd / _h2 / _h2u leave
 * their per-workgroup partial rows in ws (genrl_ln_bwd_parts(M, N) rows of np * N floats, np = 3 with dcolsum else 2; 0 = this shape
 * has no such kernel and the flag is refused) and the caller sums MANY of them in one launch per 24 at the end of the backward pass
 * (same arithmetic and order as the immediate reduction; ws must stay untouched until then). */
typedef struct {
  const float* part; float* out0; float* out1; float* out2;   /* out2 NULL unless np == 3 */
  int nchunk, N, np, accumulate;
} genrl_reduce_desc;
int genrl_ln_bwd_parts(int M, int N);
int genrl_reduce_params_batch(const genrl_reduce_desc* descs, int n, void* stream);
int genrl_ln_act_bwd_h2(const float* dy, long lddy, const float* x, long ldx, const float* gamma, const float* beta,
                        const float* mean, const float* rstd, float* dx, long lddx, float* dgamma, float* dbeta,
                        float* dcolsum, float* ws, int M, int N, int act, int accumulate_params, uint16_t* dxp, long ldp,
                        long plane, float* inv, void* stream);
int genrl_gru_gates_fwd_h2(const float* pre, const float* h, long ldh, const float* gamma, const float* beta,
                           float* hout, long ldo, float* hout2, const float* hout2_scale, float* mean, float* rstd,
                           int R, int D, float eps, uint16_t* hp, long ldp, long plane, float* inv, void* stream);
/* (dpre may be NULL when dprep is given: the pre-activation gradient as planes only; NULL without planes: GENRL_EINVAL) */
int genrl_gru_gates_bwd_h2(const float* dhout, long lddo, const float* dhout2, const float* dhout2_scale,
                           const float* pre, const float* h, long ldh, const float* gamma, const float* beta,
                           const float* mean, const float* rstd, float* dpre, float* dh, long lddh, float* dgamma,
                           float* dbeta, float* ws, int R, int D, int accumulate_params, const float* dhout2_parts,
                           int nparts, long part_stride, uint16_t* dprep, long ldp, long plane, float* inv, void* stream);
int genrl_actor_head_fwd_h2(const float* raw, const float* eps, float* action, float* mean, float* std, long R, int A,
                            float min_std, float max_std, long ld_action, uint16_t* ap, long ldp, long plane, float* inv,
                            void* stream);
/* planes of the sample / of d logits: rows of `rowlen` = S*K elements (the sample's scale is the constant 2^14) */
int genrl_onehot_fwd_h2(const float* logits, const float* q, float* sample, float* probs, long G, int K, float unimix,
                        uint16_t* sp, int rowlen, long ldp, long plane, float* inv, void* stream);
/* dlogits may be NULL (planes only) when accumulate == 0 and the kernel writes the planes itself -- genrl_onehot_bwd_planes_only_ok(K, rowlen):
 * K in {4, 8, 16, 32, 64}, rowlen % 64 == 0, rowlen <= 1024; GENRL_EINVAL otherwise */
int genrl_onehot_bwd_planes_only_ok(int K, int rowlen);
int genrl_onehot_bwd_h2(const float* logits, const float* gsample, float* dlogits, long G, int K, float unimix,
                        int accumulate, uint16_t* dp, int rowlen, long ldp, long plane, float* inv, void* stream);

/* M <= 32 rows, A k-contiguous: the product as `nparts` K-split partial slabs (P + s*part_stride, leading dimension
 * ldp) that the consumer sums -- the recurrent dgrad d h_{t-1} += dpre_t W_h of the RSSM scans' backward
 * (GRUCell, agent/dreamer_utils.py:771-785), consumed by genrl_gru_gates_bwd(dhout2_parts). */
int genrl_sgemm_skinny_parts(const float* A, long a_rs, const float* B, long b_rs, long b_ks, float* P, long ldp,
                             long part_stride, int M, int N, int K, int nparts, void* stream);

/* ---- LayerNorm(+SiLU): NormLayer + act (agent/dreamer_utils.py:844-859,462-463,745) and, on NHWC
 * activations, ImgChLayerNorm (:1031-1040).  act: 0 none, 1 SiLU, 2 ELU (torch.nn.ELU, alpha 1: z above 0, expm1(z) below; the `act:`
 * of a block's configuration, get_act :862-868) -- the GENRL_ACT_* below.  The same codes are taken by genrl_ln_act_{fwd,bwd}, _h2, _h2u and
 * genrl_gemm_h2_ln, in every instantiation their dispatchers select; any other value returns 1 before a launch.  The plane scales need
 * no reasoning of their own for ELU: |ELU(z)| <= |z| as |SiLU(z)| <= |z|, so the uniform bound max|gamma| sqrt(N) + max|beta| and the
 * row-maximum planes hold as they do for SiLU.  The sequence entries (seq.hip), the policy tape, the fused rollout and
 * genrl_onehot_gather_ln_fwd take no code: they have SiLU built in. */
#define GENRL_ACT_NONE 0
#define GENRL_ACT_SILU 1
#define GENRL_ACT_ELU 2
int genrl_ln_act_fwd(const float* x, long ldx, const float* gamma, const float* beta, float* y, long ldy, float* mean,
                     float* rstd, int M, int N, float eps, int act, void* stream);
long genrl_ln_ws_floats(int M, int N);
int genrl_ln_act_bwd(const float* dy, long lddy, const float* x, long ldx, const float* gamma, const float* beta,
                     const float* mean, const float* rstd, float* dx, long lddx, float* dgamma, float* dbeta,
                     float* dcolsum, float* ws, int M, int N, int act, int accumulate_params, void* stream);
/* column sums (bias gradients) */
long genrl_colsum_ws_floats(int M, int N);
int genrl_colsum(const float* x, long ldx, float* out, float* ws, int M, int N, int accumulate, void* stream);

/* ---- GRU gate block: GRUCell.forward after the projection (agent/dreamer_utils.py:778-785), with the
 * is_first reset of the next step's previous state (:433-434) fused as a scaled second output; the
 * backward includes the LayerNorm backward and the recurrent-gradient add of a sequence scan.
 * genrl_gru_gates_bwd's accumulate_params is a bit set: 1 = add to dgamma/dbeta; 2 = add this call's per-workgroup
 * partial sums to those a previous call (same R, D) left in ws; 4 = leave the partials in ws, no reduction.  A T-step
 * scan passes 4, 2|4, ..., 2|4, 2: one parameter-gradient reduction per scan instead of one per step. */
int genrl_gru_gates_fwd(const float* pre, const float* h, long ldh, const float* gamma, const float* beta,
                        float* hout, long ldo, float* hout2, const float* hout2_scale, float* mean, float* rstd,
                        int R, int D, float eps, void* stream);
/* the same with hout2's rows ldo2 floats apart (the state half of a concatenated [x | h] operand of the next step's product) */
int genrl_gru_gates_fwd_ld2(const float* pre, const float* h, long ldh, const float* gamma, const float* beta,
                            float* hout, long ldo, float* hout2, long ldo2, const float* hout2_scale, float* mean, float* rstd,
                            int R, int D, float eps, void* stream);
long genrl_gru_ws_floats(int R, int D);
int genrl_gru_gates_bwd(const float* dhout, long lddo, const float* dhout2, const float* dhout2_scale,
                        const float* pre, const float* h, long ldh, const float* gamma, const float* beta,
                        const float* mean, const float* rstd, float* dpre, float* dh, long lddh, float* dgamma,
                        float* dbeta, float* ws, int R, int D, int accumulate_params, const float* dhout2_parts,
                        int nparts, long part_stride, void* stream);
/* the same with the slabs' rows ldpart floats apart (a slab that is a column block of a wider product's output) */
int genrl_gru_gates_bwd_ldp(const float* dhout, long lddo, const float* dhout2, const float* dhout2_scale,
                            const float* pre, const float* h, long ldh, const float* gamma, const float* beta,
                            const float* mean, const float* rstd, float* dpre, float* dh, long lddh, float* dgamma,
                            float* dbeta, float* ws, int R, int D, int accumulate_params, const float* dhout2_parts,
                            int nparts, long part_stride, long ldpart, void* stream);

/* ---- actor Normal head: DistLayer 'normal' + rsample (agent/dreamer_utils.py:814-819) */
int genrl_actor_head_fwd(const float* raw, const float* eps, float* action, float* mean, float* std, long R, int A,
                         float min_std, float max_std, long ld_action /* 0 = A */, void* stream);
/* the policy's output layer fused with the head: raw = y W^T + b (W: 2A x U; agent/dreamer_utils.py:798), then the head above on
 * raw; writes raw (R x 2A) and action (R x ld_action), optionally the action's h2 planes (ap != NULL).  One workgroup per row; U % 4 == 0,
 * A <= 32, y rows and W 16-byte aligned. */
int genrl_actor_head_linear_fwd(const float* y, long ldy, const float* W, const float* b, const float* eps, float* raw,
                                float* action, long R, int U, int A, float min_std, float max_std, long ld_action, uint16_t* ap,
                                long ldp, long plane, float* inv, void* stream);
/* backward twin inside the rollout: d raw = head_bwd(dx WaT^T (+ daction_up)), WaT = the action columns of the img_in weight,
 * transposed (A x U row-major); one workgroup per row */
int genrl_actor_head_linear_bwd(const float* dx, long lddx, const float* WaT, const float* daction_up, long ld_action,
                                const float* raw, const float* eps, float* draw, long R, int U, int A, float min_std, float max_std,
                                void* stream);
int genrl_actor_head_bwd(const float* daction, const float* raw, const float* eps, float* draw, long R, int A,
                         float min_std, float max_std, long ld_action /* 0 = A */, void* stream);

/* strided 2-D copy with optional per-row scale (is_first reset mask, agent/dreamer_utils.py:433-435;
 * torch.cat of [stoch, action] / [x, deter], :461,:777) */
int genrl_copy2d(const float* src, long lds, float* dst, long ldd, long rows, int cols, const float* rowscale,
                 int accumulate, void* stream);

/* ---- categorical latents: OneHotDist (agent/dreamer_utils.py:177-197), sample with injected
 * exponential noise q (argmax p/q == torch.multinomial), mode when q == NULL; straight-through bwd */
int genrl_onehot_fwd(const float* logits, const float* q, float* sample, float* probs, long G, int K, float unimix,
                     void* stream);
int genrl_onehot_bwd(const float* logits, const float* gsample, float* dlogits, long G, int K, float unimix,
                     int accumulate, void* stream);
/* the scan forms (EnsembleRSSM.observe without single_obs_posterior, genrl_observe_seq_*): G = rows * S groups; the forward also writes
 * sample2 = scale2[g / S] * sample (the next step's is_first-reset previous latent, agent/dreamer_utils.py:433-434; sample2 may be NULL);
 * the backward's upstream is gsample (may be NULL) + scale2[g / S] * g2 (g2 may be NULL; scale2 NULL = 1) */
int genrl_onehot_fwd_masked(const float* logits, const float* q, float* sample, float* sample2, int* idx2, const float* scale2, int S,
                            long G, int K, float unimix, void* stream);
/* (idx2, int32 [G], may be NULL: the sampled class of every group, -1 where scale2 is 0 -- what genrl_onehot_gather_ln_fwd reads)
 * The head product AND the sample in one launch, for few rows (M <= 64 is what it is meant for) and 32-class latents: logits C (M x S*32,
 * rows ldc apart) = A (M x Kred, rows a_ld apart) W^T + bias (W: S*32 x Kred, rows b_ld apart; agent/dreamer_utils.py:443-457, 475-490),
 * outputs as genrl_onehot_fwd_masked's.  Kred % 16 == 0, a_ld / b_ld % 4 == 0, 16-byte aligned operands; returns 1 otherwise. */
int genrl_linear_sample32(const float* A, long a_ld, const float* W, long b_ld, const float* bias, float* C, long ldc, const float* q,
                          float* sample, float* sample2, int* idx2, const float* scale2, int M, int S, int Kred, float unimix,
                          void* stream);
/* x = SiLU(LayerNorm(xpre)) after xpre (M x N, rows ldx apart) += sum over the S latents of wT[(s K + idx[m][s])][:] (idx -1: nothing):
 * the latent block of _img_in applied to a ONE-HOT previous latent as a gather of rows of the transposed weight wT [S K][N] (rows ldw
 * apart) -- no product -- with the LayerNorm + SiLU that follows (agent/dreamer_utils.py:461-463) in the same launch.  xpre holds the
 * batched half (action columns + bias) on entry and the full pre-activation on return.  N % 4 == 0, N <= 1024, S <= 64. */
int genrl_onehot_gather_ln_fwd(const int* idx, int S, int K, const float* wT, long ldw, float* xpre, long ldx, const float* gamma,
                               const float* beta, float* y, long ldy, float* mean, float* rstd, int M, int N, float eps, void* stream);
int genrl_onehot_bwd_masked(const float* logits, const float* gsample, const float* g2, const float* scale2, int S, float* dlogits,
                            long G, int K, float unimix, int accumulate, void* stream);
/* KL(Independent(OneHotDist(lp)) || Independent(OneHotDist(lq))) per row + entropies
 * (EnsembleRSSM.kl_loss, agent/dreamer_utils.py:534-555; agent/dreamer.py:249-250) */
int genrl_cat_kl_fwd(const float* lp, const float* lq, float* kl, float* ent_p, float* ent_q, long R, int S, int K,
                     float unimix, void* stream);
int genrl_cat_kl_bwd(const float* lp, const float* lq, const float* gp, const float* gq, float* dlp, float* dlq, long R,
                     int S, int K, float unimix, void* stream);

/* The balanced free-nats loss on top of the per-row KL (EnsembleRSSM.kl_loss, agent/dreamer_utils.py:534-555, balance != 0.5,
 * free_avg False): loss = mix*mean(max(kl,free)) + (1-mix)*mean(max(kl,free)) as one device scalar, and the per-row
 * upstream gradients of the two sides (gp -> genrl_cat_kl_bwd's gp: the side scaled by mix; gq: by 1-mix) from the
 * scalar gradient gloss[0]; rows with kl < free get zero. */
int genrl_kl_balance_fwd(const float* kl, long R, float mix, float free_nats, float* loss, void* stream);
int genrl_kl_balance_bwd(const float* kl, const float* gloss, long R, float mix, float free_nats, float* gp, float* gq,
                         void* stream);
/* The same loss in every mode of the reference's kl_loss (:542-554) -- the GENRL_KL_* below, picked from `kl.balance` / `kl.free_avg`:
 *   BALANCED    the pair above, bit for bit;
 *   UNBALANCED  (balance == 0.5) loss = mean(max(kl,free)): one KL with its full gradient into both sides, gp = gq = the row's
 *               gradient; mix is not read;
 *   FREE_AVG    (free_avg) loss = mix*max(mean(kl),free) + (1-mix)*max(mean(kl),free): the clamp acts on the mean; every row gets
 *               mix*gloss/R (gp) and (1-mix)*gloss/R (gq) when the mean lies above free, exact zeros when below.
 * torch.maximum's tie rule holds in all of them: half the gradient at kl == free (FREE_AVG: at mean == free).  fwd is one workgroup
 * with a fixed summation order and also writes mean(kl) to the device scalar `mean` (NULL: not written; FREE_AVG needs it), which
 * bwd reads in FREE_AVG (there `kl` may be NULL) -- no mode is decided on the host.  bwd writes every element of gp and gq.  An
 * unknown mode, R < 1 or a NULL the mode needs returns 1 before any launch. */
#define GENRL_KL_BALANCED 0
#define GENRL_KL_UNBALANCED 1
#define GENRL_KL_FREE_AVG 2
int genrl_kl_loss_fwd(const float* kl, long R, int mode, float mix, float free_nats, float* loss, float* mean, void* stream);
int genrl_kl_loss_bwd(const float* kl, const float* mean, const float* gloss, long R, int mode, float mix, float free_nats,
                      float* gp, float* gq, void* stream);

/* ---- TwoHotDist (agent/dreamer_utils.py:120-171): mode 0 log_prob(x), mode 1 mean.  logits rows are `ld` floats
 * apart (255, or 256 for the padded rows the head's GEMMs prefer), dlogits rows `ldd`; with ldd > 255 the
 * backward also writes a zero into column 255. */
int genrl_twohot_fwd(const float* logits, long ld, const float* x, const float* buckets, float* out, long R, int mode,
                     void* stream);
int genrl_twohot_bwd(const float* logits, long ld, const float* x, const float* buckets, const float* gout,
                     float* dlogits, long ldd, long R, int mode, void* stream);

/* ---- lambda_return (agent/dreamer_utils.py:228-253): reward [H,N], value [H+1,N] */
int genrl_lambda_return_fwd(const float* reward, const float* value, float* ret, int H, long N, float disc, float lam,
                            void* stream);
/* zero_tail != 0: dreward has H+1 rows (the caller's reward tensor carries an unused row H); row H is zeroed */
int genrl_lambda_return_bwd(const float* gret, float* dreward, float* dvalue, int H, long N, float disc, float lam,
                            int zero_tail, void* stream);

/* ---- the learned discount of `pred_discount: True` (csrc/discount.hip).  The head is DistLayer 'binary' (agent/dreamer_utils.py:
 * 820-823): Independent(Bernoulli(logits = z), 1) with z = sigmoid(x) -- the reference hands the sigmoid to BernoulliDist's first
 * parameter, `logits` (:199-201) --, restated as it computes: log_prob(t) = t z - softplus(z), mean = sigmoid(z).  Every entry: fp32,
 * one thread per element or column, every output element written; a NULL among the required pointers or a count below 1 returns 1
 * before any launch.
 * like[i] = target[i] z - softplus(z);  dx[i] = glike[i] (target[i] - sigmoid(z)) z (1 - z).  Finite for every finite x. */
int genrl_binary_like_fwd(const float* x, const float* target, float* like, long R, void* stream);
int genrl_binary_like_bwd(const float* x, const float* target, const float* glike, float* dx, long R, void* stream);
/* WorldModel.imagine's discounts (agent/dreamer.py:274-286) from the head's raw output x [H1,N] at the H1 rollout states:
 * p[t] = sigmoid(sigmoid(x[t])), with p[0] = 1 - term where term [N] (is_terminal of the start states, as floats) is not NULL;
 * disc[t] = gamma p[t]; weight[0] = 1, weight[t] = weight[t-1] p[t-1], multiplied in that order.  One launch.
 * bwd: dx[t] = gdisc[t] gamma p (1 - p) z (1 - z); row 0 is exactly zero when term_given != 0.  The weight has no backward. */
int genrl_imag_discount_fwd(const float* x, const float* term, int H1, long N, float gamma, float* disc, float* weight, void* stream);
int genrl_imag_discount_bwd(const float* x, const float* gdisc, int term_given, int H1, long N, float gamma, float* dx, void* stream);
/* lambda_return with a discount per step and column (a tensor `pcont`): R_t = r_t + d_t ((1-lam) v_{t+1} + lam R_{t+1}), R_H = v_H;
 * reward [H,N], value [H+1,N], disc [H,N]; reward and disc may carry an unread row H.  With every d_t equal to `disc` of
 * genrl_lambda_return_fwd / _bwd, ret, dreward and dvalue equal theirs bit for bit.
 * bwd: a_t = g_t + d_{t-1} lam a_{t-1}; dreward_t = a_t; ddisc_t = a_t ((1-lam) v_{t+1} + lam R_{t+1}); dvalue_{t+1} = d_t (1-lam) a_t
 * (t < H-1), d_{H-1} a_{H-1} (bootstrap); dvalue_0 = 0.  zero_tail != 0: dreward and ddisc have H+1 rows, row H is zeroed. */
int genrl_lambda_return_disc_fwd(const float* reward, const float* value, const float* disc, float* ret, int H, long N, float lam,
                                 void* stream);
int genrl_lambda_return_disc_bwd(const float* gret, const float* value, const float* disc, const float* ret, float* dreward,
                                 float* dvalue, float* ddisc, int H, long N, float lam, int zero_tail, void* stream);

/* ---- MSEDist.log_prob against uint8 frames (agent/dreamer_utils.py:74-83; agent/dreamer.py:294-295) */
int genrl_mse_fwd(const float* mean, const uint8_t* obs, float* like, long Nimg, int E, void* stream);
int genrl_mse_bwd(const float* mean, const uint8_t* obs, const float* glike, float* dmean, long Nimg, int E,
                  void* stream);

/* ---- imagination reward: max_cosine_similarity + align_sequence index (tools/genrl_utils.py:240-242,344-366) */
int genrl_maxcos_fwd(const float* u, const float* v, const long* urow, float* out, long R, int E, void* stream);
int genrl_maxcos_bwd(const float* u, const float* v, const long* urow, const float* gout, float* dv, long R, int E,
                     void* stream);
int genrl_align_index(const float* ct, const float* ca, long* urow, int T, long N, int E, int nf, void* stream);

/* ---- stride-2 conv data movement (Encoder/Decoder, agent/dreamer_utils.py:578-589,654-671) */
int genrl_im2col_s2(const void* in, float* cols, int Nimg, int Hi, int Wi, int C, int k, int in_mode, void* stream);
int genrl_col2im_s2(const float* cols, const float* bias, float* out, int Nimg, int Ha, int Wa, int C, int k,
                    int Ho_override, int Wo_override, int out_nchw, void* stream);
/* out[b,c,p] (+)= in[b,p,c] */
int genrl_transpose_last2(const float* in, float* out, long B, int P, int C, int accumulate, void* stream);

/* ---- replay window gather: ReplayBuffer.__iter__'s np.stack of (episode, t0..t0+T) slices + host-to-device
 * copy (tools/replay.py:223-236) on a device-resident ring of ring_rows steps:
 * dst[b,t,:] = src[(start[b]+t) % ring_rows,:] */
int genrl_gather_windows(const void* src, long row_bytes, long ring_rows, const long* start, int B, int T, void* dst,
                         void* stream);

/* ---- small statistics of the actor-critic update, one launch each (genrl_amd/csrc/stats.hip)
 * genrl_moments: StreamNorm's running statistics and metrics (agent/dreamer_utils.py:934-1001): out[0..3] = mean,
 *   unbiased std, mean |x|, mean x^2.
 * genrl_quantile_ema: RewardEMA (agent/dreamer_utils.py:1014-1029): torch.quantile(x, [q0, q1]) (linear interpolation)
 *   by radix select, ema <- alpha * quantile + (1 - alpha) * ema in place, out = (ema[0], max(ema[1] - ema[0], 1),
 *   quantile0, quantile1).
 * genrl_wmean_{fwd,bwd}: out = scale * mean(x * w) (w may be NULL): -like.mean() of the ELBO terms
 *   (agent/dreamer.py:229-243), the critic's weighted two-hot loss (:431-438).
 * genrl_actor_obj_{fwd,bwd}: the return-normalised actor objective (agent/dreamer.py:392-429, actor_grad 'dynamics',
 *   actor_ent 0): target [H, N] lambda-returns, offset_scale = genrl_quantile_ema's out; loss[0]; out = (mean, std of the
 *   normalised returns).
 * genrl_normal_entropy_mean: mean entropy of the policy's Independent(Normal) (the 'actor_ent' metric, :425-427). */
int genrl_moments(const float* x, long n, float* out, void* stream);
int genrl_quantile_ema(const float* x, long n, float q0, float q1, float alpha, float* ema, float* out, void* stream);
int genrl_wmean_fwd(const float* x, const float* w, long n, float scale, float* out, void* stream);
int genrl_wmean_bwd(const float* g, const float* w, long n, float scale, float* dx, void* stream);
int genrl_actor_obj_fwd(const float* target, const float* weight, const float* offset_scale, int H, long N, float* loss,
                        float* out, void* stream);
int genrl_actor_obj_bwd(const float* g, const float* weight, const float* offset_scale, int H, long N, float* dtarget,
                        void* stream);
int genrl_normal_entropy_mean(const float* raw, long R, int A, float min_std, float max_std, float* out,
                              float* ws /* >= 128 floats, 8-byte aligned */, void* stream);

/* ---- connector (VideoSSM.update, agent/video_utils.py:127-161)
 * genrl_connector_prep: from the batch's clip embeddings video (B,T,E) and Gaussian noise eps (B,T,E): clean (B,T,E) = the
 *   embedding of each aligned nf-frame chunk held over the chunk (:134-136), noisy (B,T,E) = unit((1-lam) clean + lam unit(eps))
 *   (lafite noise, :141-145), act_tm (T,B,E+nf) = [clean * cscale | zeros] time-major (get_action, :114-125).
 * genrl_connector_prep_slots: the same launch with the slot columns chosen: temporal 0 = zeros (what genrl_connector_prep passes),
 *   non-zero = one_hot(t % nf) (`connector.temporal_embeds`, :121).
 * genrl_tf_inputs_{fwd,bwd}: the teacher-forced input of the connector's prior pass under `connector.token_dropout` (:171-179).
 *   fwd: first (B,W), post (B,T,W) batch-major, e (T,B) Exp(1) noise: keep (T,B) = e < thresh as 0/1 floats and
 *   x (T*B,W) time-major, x[t*B+b] = keep[t,b] * (t == 0 ? first[b] : post[b,t-1]).
 *   bwd: g (T*B,W): dfirst[b] = keep[0,b] g[0,b]; dpost (NULL: not written) [b,t] = keep[t+1,b] g[t+1,b], zero at t = T-1.
 *   Any W; rows go as float4 where W % 4 == 0 and the bases are 16-byte aligned.
 * genrl_cosdist_{fwd,bwd}: the aligner's loss 1 - mean(cosine_similarity(normalize(x), c)) (:146-150), gradient to x;
 *   cosv, xnorm: R floats each, kept for the backward. */
int genrl_connector_prep(const float* video, const float* eps, float* clean, float* noisy, float* act_tm, int B, int T,
                         int E, int nf, float lam, float cscale, void* stream);
int genrl_connector_prep_slots(const float* video, const float* eps, float* clean, float* noisy, float* act_tm, int B, int T,
                               int E, int nf, float lam, float cscale, int temporal, void* stream);
int genrl_tf_inputs_fwd(const float* first, const float* post, const float* e, float thresh, int B, int T, int W, float* x,
                        float* keep, void* stream);
int genrl_tf_inputs_bwd(const float* g, const float* keep, int B, int T, int W, float* dfirst, float* dpost, void* stream);
int genrl_cosdist_fwd(const float* x, const float* c, float* cosv, float* xnorm, float* out, long R, int E, void* stream);
int genrl_cosdist_bwd(const float* x, const float* c, const float* cosv, const float* xnorm, const float* g, float* dx,
                      long R, int E, void* stream);

/* ---- Optimizer.__call__ (agent/dreamer_utils.py:892-932) on flat buffers */
long genrl_sqnorm_ws_floats(long n);
/* step_inc (may be NULL): a device-side Adam step counter incremented by one (before genrl_adam_step reads it) */
int genrl_grad_norm(const float* g, long n, float* norm_out, float* ws, float scale, int* step_inc, void* stream);
/* zero_grad != 0: g is cleared in the same pass (the optimiser's zero_grad()) */
int genrl_adam_step(float* p, float* g, float* m, float* v, long n, const float* norm, float gscale, float clip,
                    float lr, float b1, float b2, float eps, float wd, int step, const int* step_dev, int zero_grad,
                    void* stream);
int genrl_scale(float* p, long n, float s, void* stream);

/* ---- Plan2Explore ensemble (agent/plan2explore.py:8-41; genrl_amd/csrc/ensemble.hip, the ReLU in rowact.hip): the row kernels around a member's two products.
 * Rows of N floats, N % 4 == 0 (tested to 12 288), any row pitch that is a multiple of 4 floats, 16-byte aligned bases; returns 1 otherwise.
 * Plane outputs (yp / dxp / dpp; NULL: none) follow the contract of genrl_ln_act_fwd_h2: planes [.][ldp] `plane` elements apart, inv[row],
 * the row maximum taken over the kernel's output row, columns beyond N untouched -- bit-identical to genrl_split_h2 of the fp32 output.
 * genrl_relu_fwd_h2: y = max(x, 0) (y may be x).  genrl_relu_bwd_h2: dx = dy [y > 0] (dx may be dy).
 * genrl_l2err_fwd: err[m] = || t[m, :] - p[m, :] ||_2.  genrl_l2err_bwd: dp[m, :] = -g[m] (t - p) / err[m]; a row with err = 0 gets zeros.
 * genrl_ens_var_fwd: K member predictions p[k] = p + k * member (2 <= K <= 8), r[m] = mean_e of the unbiased variance over k (two passes per
 * element over the K values in registers).  genrl_ens_var_bwd: dp[k][m][e] = g[m] 2 (p_k - mean_k) / ((K - 1) N) (g NULL: 1) into dp + k * dmember
 * (dp NULL with dpp given: planes only) and, with dpp, the planes of every dp_k: member k at dpp + k * pmember, inv + k * imember. */
int genrl_relu_fwd_h2(const float* x, long ldx, float* y, long ldy, int M, int N, uint16_t* yp, long ldp, long plane, float* inv,
                      void* stream);
int genrl_relu_bwd_h2(const float* dy, long lddy, const float* y, long ldy, float* dx, long lddx, int M, int N, uint16_t* dxp, long ldp,
                      long plane, float* inv, void* stream);
int genrl_l2err_fwd(const float* t, long ldt, const float* p, long ldp, float* err, int M, int N, void* stream);
int genrl_l2err_bwd(const float* g, const float* err, const float* t, long ldt, const float* p, long ldp, float* dp, long lddp, int M,
                    int N, uint16_t* dpp, long ldpl, long plane, float* inv, void* stream);
int genrl_ens_var_fwd(const float* p, long member, long ld, int K, float* r, int M, int N, void* stream);
int genrl_ens_var_bwd(const float* g, const float* p, long member, long ld, int K, float* dp, long dmember, long lddp, int M, int N,
                      uint16_t* dpp, long pmember, long ldpl, long plane, float* inv, long imember, void* stream);

/* ---- the DreamerV2 defaults (conf/defaults/dreamer_v2.yaml; genrl_amd/csrc/rowact.hip, heads.hip, vecobs.hip)
 * genrl_silu_{fwd,bwd}_h2: the activation behind a Linear without LayerNorm (`norm: none`, agent/dreamer_utils.py:739-747).  Rows, pitches,
 *   alignment and the optional plane output as genrl_relu_*_h2 above (planes bit-identical to genrl_split_h2 of the fp32 output).
 *   fwd: y = x sigmoid(x) (y may be x).  bwd: dx = dy sigmoid(x) (1 + x (1 - sigmoid(x))) from the saved pre-activation x (dx may be dy).
 *   Large |x| gives no NaN (x = -100: y = -0, dx = -0 dy); a NaN input stays NaN.
 * genrl_elu_{fwd,bwd}_h2: the same contract for `act: ELU`.  fwd: y = x above 0, expm1(x) below (y may be x).  bwd: dx = dy above 0,
 *   dy exp(x) below, from the saved pre-activation x (dx may be dy).  x = -100: y = -1, dx = 0; x = 100: y = 100; a NaN input stays NaN.
 * genrl_trunc_normal_head_{fwd,bwd}: DistLayer 'trunc_normal' (:830-834) + TruncatedNormal.sample (tools/utils.py:102-123) on
 *   raw [R, 2A] = [out | std_raw]: mean = tanh(out), std = 2 sigmoid((std_raw + init_std) / 2) + min_std, action = clamp(mean + eps std,
 *   -1 + 1e-6, 1 - 1e-6) (rows ld_action apart, 0 = A).  eps NULL: the mean-only form (action, if given, = clamp(mean)); any of action / mean /
 *   std may be NULL.  bwd: the clamp is straight-through -- d raw is that of mean + eps std for every element, clamped or not.
 * genrl_sqerr_{fwd,bwd}: MSEDist.log_prob of a one-wide head (:62-83): like = -(out - x)^2 elementwise; dout = -2 (out - x) g. */
int genrl_silu_fwd_h2(const float* x, long ldx, float* y, long ldy, int M, int N, uint16_t* yp, long ldp, long plane, float* inv,
                      void* stream);
int genrl_silu_bwd_h2(const float* dy, long lddy, const float* x, long ldx, float* dx, long lddx, int M, int N, uint16_t* dxp, long ldp,
                      long plane, float* inv, void* stream);
int genrl_elu_fwd_h2(const float* x, long ldx, float* y, long ldy, int M, int N, uint16_t* yp, long ldp, long plane, float* inv,
                     void* stream);
int genrl_elu_bwd_h2(const float* dy, long lddy, const float* x, long ldx, float* dx, long lddx, int M, int N, uint16_t* dxp, long ldp,
                     long plane, float* inv, void* stream);
int genrl_trunc_normal_head_fwd(const float* raw, const float* eps, float* action, float* mean, float* std, long R, int A,
                                float min_std, float init_std, long ld_action, void* stream);
int genrl_trunc_normal_head_bwd(const float* daction, const float* raw, const float* eps, float* draw, long R, int A, float init_std,
                                long ld_action, void* stream);
int genrl_sqerr_fwd(const float* out, const float* x, float* like, long n, void* stream);
int genrl_sqerr_bwd(const float* out, const float* x, const float* g, float* dout, long n, void* stream);

/* ---- the squashed-Gaussian actor head (DistLayer 'tanh_normal', agent/dreamer_utils.py:824-829: SquashedNormal, tools/utils.py:126-170, in
 * SampleDist, agent/dreamer_utils.py:28-60; genrl_amd/csrc/heads.hip).  raw [R, 2A] = [out | std_raw], 1 <= A <= 64:
 *   mean = 5 tanh(out / 5), std = softplus(std_raw + init_std) + min_std (torch's softplus: the identity above 20), x = mean + std eps,
 *   action = tanh(x).  Every entry returns 1 before any launch, and writes nothing, for A out of range, K < 1, a missing required pointer
 *   or no output at all; R = 0 is a no-op.  No NaN or inf for any finite input (out = +-50, std_raw = 25 or -30, eps = +-6, x < -10).
 * genrl_tanh_normal_head_{fwd,bwd}: the shape of genrl_trunc_normal_head_* above: eps [R, A], action rows ld_action apart (0 = A); any of
 *   action / mean / std may be NULL.  eps NULL: the mean form (action, if given, = tanh(mean)).  bwd: draw [R, 2A] from daction (rows
 *   ld_action apart): dx = daction (1 - action^2), d mean = dx, d std = dx eps, then through 5 tanh(. / 5) and the softplus.
 * genrl_tanh_normal_mc_fwd: SampleDist over K samples, eps [K, R, A]: mean_action[R, A] = mean_k tanh(x_k) (SampleDist.mean) and
 *   ent[R] = -mean_k log_prob(sample_k) (SampleDist.entropy), log_prob = sum_a(-(x - mean)^2 / (2 std^2) - log std - log(2 pi) / 2 - ladj(x))
 *   with ladj(x) = 2 (log 2 - x - softplus(-2x)), on the pre-tanh x (no atanh).  ent or mean_action may be NULL.  One row per aligned
 *   group of 4 ... 64 lanes, one action dimension per lane; per-sample terms are summed in double in the order of k and across the row by
 *   shuffles in a fixed order: two launches on the same inputs agree bit for bit.
 * genrl_tanh_normal_ent_bwd: draw [R, 2A] (+)= gent[r] d ent[r] / d raw, recomputed from raw and eps (nothing else is saved):
 *   d ent / d mean_a = mean_k(-2 tanh x_ka), d ent / d std_a = 1 / std_a + mean_k(-2 tanh(x_ka) eps_ka), then through the head.
 *   accumulate != 0 adds into draw, as genrl_onehot_logp_ent_bwd does. */
int genrl_tanh_normal_head_fwd(const float* raw, const float* eps, float* action, float* mean, float* std, long R, int A,
                               float min_std, float init_std, long ld_action, void* stream);
int genrl_tanh_normal_head_bwd(const float* daction, const float* raw, const float* eps, float* draw, long R, int A, float min_std,
                               float init_std, long ld_action, void* stream);
int genrl_tanh_normal_mc_fwd(const float* raw, const float* eps, float* ent, float* mean_action, long R, int A, int K, float min_std,
                             float init_std, void* stream);
int genrl_tanh_normal_ent_bwd(const float* gent, const float* raw, const float* eps, float* draw, long R, int A, int K, float min_std,
                              float init_std, int accumulate, void* stream);

/* ---- discrete actions (`discrete_actions`, agent/dreamer.py:332-333; `actor_grad: reinforce`, :413-419; genrl_amd/csrc/discrete.hip)
 * genrl_onehot_logp_ent_{fwd,bwd}: the actor's OneHotDist (agent/dreamer_utils.py:177-197) on logits [G, K], 2 <= K <= 64 (returns 1
 *   otherwise and writes nothing): p = (1 - unimix) softmax(logits) + unimix / K, renormalised as torch's Categorical(probs=) does.  Here
 *   `unimix` is the weight of the UNIFORM part (0.01), not the 0.99 that genrl_onehot_fwd takes.  logp[g] = sum_k action[g, k] log p[g, k]
 *   (action: one-hot rows [G, K]), ent[g] = -sum_k p log p, with log p = log(clamp(p, eps, 1 - eps)) (probs_to_logits); logp or ent may
 *   be NULL.  bwd: dlogits = glogp[g] d logp + gent[g] d ent through the mix and the softmax (glogp or gent may be NULL; accumulate != 0
 *   adds into dlogits, as genrl_onehot_bwd does).  No gradient to action.
 * genrl_reinforce_obj_{fwd,bwd}: the REINFORCE actor objective with the shapes and conventions of genrl_actor_obj_*: target, baseline
 *   [H, N] (row 0 unused), logp, ent, weight [H-1, N] (weight may be NULL = 1; ent may be NULL when ent_scale == 0), offset_scale =
 *   genrl_quantile_ema's out (NULL: `reward_ema: False`, offset 0, scale 1):
 *     loss[0] = -mean(weight (logp ((target[1:] - offset) / scale - (baseline[1:] - offset) / scale) + ent_scale ent));
 *   with offset_scale, out = (mean, unbiased std of (target - offset) / scale over all H N).  bwd, from the scalar gradient g: dlogp, dent
 *   [H-1, N], dtarget, dbaseline [H, N] with row 0 zero (any of them may be NULL).  The advantage is NOT detached (:416-417). */
int genrl_onehot_logp_ent_fwd(const float* logits, const float* action, float* logp, float* ent, long G, int K, float unimix,
                              void* stream);
int genrl_onehot_logp_ent_bwd(const float* logits, const float* action, const float* glogp, const float* gent, float* dlogits,
                              long G, int K, float unimix, int accumulate, void* stream);
int genrl_reinforce_obj_fwd(const float* target, const float* baseline, const float* logp, const float* ent, const float* weight,
                            const float* offset_scale, float ent_scale, int H, long N, float* loss, float* out, void* stream);
int genrl_reinforce_obj_bwd(const float* g, const float* target, const float* baseline, const float* logp, const float* weight,
                            const float* offset_scale, float ent_scale, int H, long N, float* dlogp, float* dtarget,
                            float* dbaseline, float* dent, void* stream);

/* ---- continuous (Gaussian) RSSM latents (`rssm.discrete: False`, agent/dreamer_utils.py:333-335, :416-419, :513-521; genrl_amd/csrc/gaussian.hip)
 * std_act: 0 softplus (torch's: x above the threshold 20, log1p(exp(x)) below), 1 sigmoid, 2 sigmoid2 = 2 sigmoid(x / 2).  Every entry
 * returns 1 before any launch for S < 1, a pitch below 2 S, an unknown std_act, a missing required pointer or no output at all.
 * genrl_gauss_head_fwd: raw [R, 2S] with row pitch ldr = [mean | std_raw]: mean = raw[:, :S], std = act(raw[:, S:]) + min_std,
 *   stoch = mean + std eps (eps [R, S]; NULL: the mean form, stoch = mean).  mean, std, stoch are [R, S], contiguous; any of them may be
 *   NULL.  No alignment is required of raw, S or ldr: 16-byte accesses are used when every pointer, S and ldr allow them.
 * genrl_gauss_head_bwd: draw [R, 2S] with row pitch lddr: draw[:, :S] = dstoch + dmean, draw[:, S:] = (dstoch eps + dstd) act'(raw[:, S:]);
 *   each of dstoch, dmean, dstd [R, S] may be NULL (zero; at least one is given), eps NULL: the mean form.  accumulate != 0 adds into
 *   draw.  Columns of draw past 2S are not written.
 * genrl_gauss_kl_fwd: kl[m] = sum_s 0.5 (v + t - 1 - log v), v = (std_l / std_r)^2, t = ((mean_l - mean_r) / std_r)^2 (torch's
 *   kl_normal_normal summed by Independent(., 1)); ent_x[m] = sum_s (0.5 + 0.5 log 2 pi + log std_x).  Inputs [R, S] contiguous, any S >= 1;
 *   kl, ent_l, ent_r may be NULL (not all); without kl only the std of the requested entropies is read.  Sums are accumulated in double
 *   in a fixed order.
 * genrl_gauss_kl_bwd: elementwise; gp[m] scales the gradient into (mean_l, std_l), gq[m] into (mean_r, std_r) -- the two per-row vectors
 *   of genrl_kl_balance_bwd.  Any of the four outputs may be NULL (not all); gp / gq is read only for a side with an output. */
int genrl_gauss_head_fwd(const float* raw, long ldr, const float* eps, float* mean, float* std, float* stoch, long R, int S,
                         int std_act, float min_std, void* stream);
int genrl_gauss_head_bwd(const float* dstoch, const float* dmean, const float* dstd, const float* raw, long ldr, const float* eps,
                         float* draw, long lddr, long R, int S, int std_act, int accumulate, void* stream);
int genrl_gauss_kl_fwd(const float* mean_l, const float* std_l, const float* mean_r, const float* std_r, float* kl, float* ent_l,
                       float* ent_r, long R, int S, void* stream);
int genrl_gauss_kl_bwd(const float* mean_l, const float* std_l, const float* mean_r, const float* std_r, const float* gp,
                       const float* gq, float* dmean_l, float* dstd_l, float* dmean_r, float* dstd_r, long R, int S, void* stream);

/* ---- vector (1-D) observations (encoder `mlp_keys` / `symlog_inputs`, decoder `mlp_keys` / `mlp_dist: mse | symlog_mse`,
 * agent/dreamer_utils.py:558-715, :62-118; genrl_amd/csrc/vecobs.hip).  Rows of D >= 1 floats with independent row pitches (in floats,
 * each >= D), so that an operand may be a column slice of a wider buffer; columns past D are neither read nor written.  No alignment is
 * required of any pointer, D or pitch.  Every entry returns 1 before any launch for D < 1, R < 0, a pitch below D, a missing pointer, a kind
 * other than 0 / 1 or a tol that is negative or NaN; R == 0 returns 0 without a launch.  Inputs and outputs must not overlap.
 * genrl_symlog_rows: y[r, :D] = symlog ? sign(x) log(|x| + 1) : x, with |x| + 1 rounded to fp32 before the logarithm (the arithmetic of
 *   the two-hot kernels' symlog; not log1p).  NaN stays NaN.  16-byte accesses are used when x, y, D and both pitches allow them.
 * genrl_vec_like_fwd: like[r] = -sum_d dist(mode[r, d], x[r, d]).  kind 0: MSEDist on a D-wide head, dist = (mode - x)^2.  kind 1:
 *   SymlogDist 'mse' with agg 'sum', dist = (mode - symlog(x))^2 replaced by 0 where it is below tol (the reference's 1e-8).  Target
 *   and difference are taken in double from the fp32 operands and the sum is accumulated in double in a fixed order: results are
 *   bit-reproducible, and a row with mode == target gives exactly 0 (kind 1: a mode that is the fp32 symlog of x lies below tol).
 *   R <= 2^32.
 * genrl_vec_like_bwd: dmode[r, d] = -2 (mode - t) g[r], t = x or symlog(x); for kind 1 exactly 0 where (mode - t)^2 < tol (decided by
 *   the forward's expression).  Elementwise; accumulate != 0 adds into dmode, as genrl_onehot_logp_ent_bwd does.  No gradient to x. */
int genrl_symlog_rows(const float* x, long ldx, float* y, long ldy, long R, int D, int symlog, void* stream);
int genrl_vec_like_fwd(const float* mode, long ldm, const float* x, long ldx, float* like, long R, int D, int kind, float tol,
                       void* stream);
int genrl_vec_like_bwd(const float* mode, long ldm, const float* x, long ldx, const float* g, float* dmode, long lddm, long R, int D,
                       int kind, float tol, int accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif
