/*
 * laplace_hip.h — C ABI of the MI355X (gfx950) curvature kernels behind
 * `laplace_amd.HipGGN`, the drop-in `laplace.curvature.CurvatureInterface` backend.
 *
 * Conventions (all entry points):
 *   - every tensor is a raw DEVICE pointer to fp32 (labels: int64) + explicit sizes; the caller
 *     (torch) owns every buffer; kernels never allocate.  Scratch comes from a caller-provided
 *     workspace sized by the matching lk_*_workspace_bytes().
 *   - `stream` is a hipStream_t passed as void*; work is enqueued asynchronously on it.  No
 *     entry point synchronises with the host.
 *   - return 0 on success, negative LK_E* on error; lk_last_error() returns a thread-local
 *     message for the last failure on the calling thread.
 *   - matrices are row-major and dense (leading dimension = number of columns) unless stated.
 *
 * Each function cites the reference code (relative to aleximmer/Laplace @ 0.2.3) it replaces.
 */
#ifndef LAPLACE_HIP_H
#define LAPLACE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LK_OK 0
#define LK_EINVAL (-1)    /* bad argument */
#define LK_EWORKSPACE (-2) /* workspace too small */
#define LK_ELAUNCH (-3)    /* HIP launch/runtime failure */
#define LK_ENOTCONV (-4)   /* eigensolver did not converge (reported through `info`) */

/* flags for the Gram (factor accumulation) family */
#define LK_GRAM_UPPER_ONLY 1u /* update only the upper block triangle; caller runs lk_symmetrize_f32 later */
#define LK_GRAM_SLABS_PERSIST 2u /* the workspace is a zero-initialised, caller-owned accumulator of split-K partial
                                    tiles that persists across launches: `slab += partial`, C is not touched; reduce
                                    once with lk_gram_slabs_reduce_f32 (a sum over minibatches is linear) */

int lk_version(void);
const char* lk_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Likelihood: square root of the softmax-CE Hessian + loss.
 * Replaces GGNInterface._get_functional_hessian (laplace/curvature/curvature.py:366-373) and the
 * `factor * lossfunc(f, y)` evaluations (curvature.py:408,417; curvlinops.py:106).
 *   S[c][n][j] = delta_jc*sqrt(p_nc) - p_nj*sqrt(p_nc)   (column c of a root of diag(p)-pp^T)
 *   loss_accum[0] += sum_n -log p_n[y_n]                  (skipped when y or loss_accum is NULL)
 * f: [B][C] logits; S: [C][B][C] (one backward seed per class, `is_grads_batched` layout).
 *
 * The loss is reduced in a FIXED order (per-workgroup partials in `ws`, then one wave sums them in index order):
 * run-to-run deterministic, no floating-point atomics.  `ws`: lk_loss_workspace_bytes(B) bytes, needed whenever the
 * loss is requested.  Labels outside [0, C) contribute nothing to the loss (CrossEntropyLoss's ignore_index).
 * ------------------------------------------------------------------------------------------- */
size_t lk_loss_workspace_bytes(int64_t B);
int lk_softmax_hess_sqrt_f32(const float* f, const int64_t* y, int64_t B, int64_t C, float* S,
                             float* loss_accum, float* ws, void* stream);

/* Same contract with the rank-revealing root: the softmax Hessian has rank C-1, and its closed-form Cholesky
 * factor  L[j][j] = sqrt(p_j s_{j+1}/s_j),  L[i][j] = -p_i sqrt(p_j/(s_j s_{j+1})) (i > j),  s_j = sum_{k>=j} p_k
 * has only C-1 non-zero columns: S is [C-1][B][C] and the fit needs one reverse pass fewer.
 * 2 <= C <= LK_SOFTMAX_CHOL_MAX_C (4 waves x (2C+1) floats of LDS per workgroup). */
#define LK_SOFTMAX_CHOL_MAX_C 2000
int lk_softmax_hess_chol_f32(const float* f, const int64_t* y, int64_t B, int64_t C, float* S,
                             float* loss_accum, float* ws, void* stream);

/* loss_accum[0] += scale * sum (f - y)^2 over `numel` elements (MSELoss(sum) * factor); fixed-order reduction
 * through `ws` (>= 4 KiB). */
int lk_sq_err_sum_f32(const float* f, const float* y, int64_t numel, float scale, float* loss_accum,
                      float* ws, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Gram / factor accumulation:  C += alpha * X^T X   (fp32 MFMA, split-K, deterministic).
 * Replaces the A^T A / G^T G accumulations inside curvlinops' KFACLinearOperator._compute_kfac
 * as consumed by CurvlinopsInterface.kron (laplace/curvature/curvlinops.py:55-108), and the
 * dense einsums of GGNInterface.full / EFInterface.full (curvature.py:406,409,491).
 *
 *  _tn  : X is [K][n] row-major with leading dimension ldx      (nn.Linear inputs / output grads)
 *  _nt  : X is [nb][n][L] row-major; C += alpha * sum_b X_b X_b^T (NCHW conv output grads).  With L % 4 == 0 and
 *         16-byte aligned X the products run on the bf16 matrix cores at fp32 accuracy: every operand is split once
 *         into three bf16 pieces (x = h + m + l exactly) and six v_mfma_f32_32x32x16_bf16 form hh' + hm' + mh' + mm' +
 *         hl' + lh' (dropped terms <= 3 * 2^-24 |x y|, accumulation in fp32); otherwise v_mfma_f32_32x32x2_f32.
 *  _conv: x is an NHWC activation [B][H][W][Cin]; the Gram matrix of the *unfolded* patch matrix
 *         (rows = (b,oh,ow), columns = (kh,kw,ci)) is accumulated WITHOUT materialising it.
 *         Column order of C is (kh,kw,ci) ("native"); lk_permute_sym_f32 converts to the
 *         reference's F.unfold order (ci,kh,kw).
 * C is [n][n] (ldc = n).  Workspace: lk_gram_workspace_bytes(n, K) for _tn (K rows) and _conv (K = B*OH*OW);
 * lk_gram_nt_workspace_bytes(nb_total, n, L) for _nt / _nt_seg (nb_total = nseg * nb images of L positions).
 * ------------------------------------------------------------------------------------------- */
size_t lk_gram_workspace_bytes(int64_t n, int64_t K);
size_t lk_gram_nt_workspace_bytes(int64_t nb_total, int64_t n, int64_t L);
/* Which instantiation of the Gram engine, which split of K and which reduction a launch takes (pure host function, no device:
 * the launchers decide with the same helpers of csrc/lk_gram.hip).  `entry`: LK_GRAM_*; (n, K, L) per entry:
 *   LK_GRAM_TN            n, K of lk_gram_tn_f32
 *   LK_GRAM_NT            n, K = nseg * nb images, L positions of lk_gram_nt_f32 / lk_gram_nt_seg_f32
 *   LK_GRAM_CONV          n = Cin * kh * kw, K = B * OH * OW of lk_gram_conv_nhwc_f32
 *   LK_GRAM_XCORR_FULL    n = Cin, K = B * H * W: the full-grid launch of lk_conv3x3_shiftcorr_f32 (13 shifts)
 *   LK_GRAM_XCORR_STRIPS  n = Cin, K = B * max(H, W): its launch of the four boundary strips and four corners (25 shifts)
 * `vec4_ok`: what of the 16-byte-load rule the arguments do not show — every operand pointer 16-byte aligned, for _TN
 * ldx % 4 == 0, for _CONV Cin % 4 == 0 (n % 4 for _TN, L % 4 for _NT and Cin % 4 for _XCORR_* are applied here).  `flags`: as
 * for the launch.  Fills out[12]:
 *   [0] loader: 0 TN, 1 NT, 2 CONV, 3 XCORR, 5 NTB (NT on split-bf16 products)   [1] VEC: 4 or 1 floats per load
 *   [2] tile configuration: 0 SMALL (64), 1 BIG (128), 2 WIDE (192)   [3] T   [4] BK rows per chunk
 *   [5] tile pairs (workgroups per split)   [6] chunks   [7] splits of K   [8] chunks per split
 *   [9] epilogue: 0 slabs + reduce, 1 direct into C, 2 persistent slabs   [10] two-level slab reduction   [11] rows per
 *   workgroup of the reduction (4 or 64)
 * and returns 0, or a negative value for what the entry point refuses or launches nothing for (n < 1, K < 0; _XCORR_*: K < 1).
 * The pixel-pair form reports its tile through lk_conv3x3_pixpair_plan (64: the 64-tile with 16-row chunks, 128: BIG). */
#define LK_GRAM_TN 0
#define LK_GRAM_NT 1
#define LK_GRAM_CONV 2
#define LK_GRAM_XCORR_FULL 3
#define LK_GRAM_XCORR_STRIPS 4
int lk_gram_launch_variant(int entry, int64_t n, int64_t K, int64_t L, int vec4_ok, unsigned flags, int* out);
/* C += alpha * sum of the persistent slabs (LK_GRAM_SLABS_PERSIST) of an n x n product; L_nt = L of the _nt launches
 * that filled them (0 for _tn / _conv); `slabs` is modified.  flags: LK_GRAM_UPPER_ONLY as for the launches. */
int lk_gram_slabs_reduce_f32(float* slabs, size_t slabs_bytes, int64_t n, int64_t L_nt, float alpha, float* C,
                             unsigned flags, void* stream);
int lk_gram_tn_f32(const float* X, int64_t K, int64_t n, int64_t ldx, float alpha, float* C,
                   unsigned flags, void* ws, size_t ws_bytes, void* stream);
int lk_gram_nt_f32(const float* X, int64_t nb, int64_t n, int64_t L, float alpha, float* C,
                   unsigned flags, void* ws, size_t ws_bytes, void* stream);
/* Same, with X given as `nseg` (<= 16) separate [nb][n][L] tensors (HOST array of device pointers):
 * the per-seed output gradients of the C backward passes are consumed where autograd left them,
 * without stacking them into one buffer. */
int lk_gram_nt_seg_f32(const float* const* segs, int64_t nseg, int64_t nb, int64_t n, int64_t L, float alpha,
                       float* C, unsigned flags, void* ws, size_t ws_bytes, void* stream);
int lk_gram_conv_nhwc_f32(const float* x, int64_t B, int64_t H, int64_t W, int64_t Cin, int kh, int kw,
                          int sh, int sw, int ph, int pw, int dh, int dw, float alpha, float* C,
                          unsigned flags, void* ws, size_t ws_bytes, void* stream);

/* Pixel-pair form of the same factor for SMALL maps (4x4 and below): the caller accumulates the pixel-pair Gram
 *   Cp[(q,ci),(q',cj)] += sum_b x[b,q,ci] x[b,q',cj]     (lk_gram_tn_f32 on the NHWC images flattened to rows, then
 * lk_symmetrize_f32) over ALL minibatches of a fit -- it is linear in the data -- and this call assembles the patch
 * Gram from it once:  A[(d,ci),(e,cj)] += alpha * sum_{p: p+d, p+e in the grid} Cp[(p+d,ci),(p+e,cj)], native
 * (kh,kw,ci) order.  Cp: [H*W*Cin][H*W*Cin], both triangles valid.  A: [9*Cin][9*Cin]. */
int lk_conv3x3_pixgram_assemble_f32(const float* Cp, int64_t H, int64_t W, int64_t Cin, float alpha, float* A,
                                    void* stream);

/* Banded pixel-pair form for ANY map size (Cin % 64 == 0): only the pixel pairs (q, q + D) a 3x3 window can see are
 * kept, D in the half plane {(0,0),(0,1),(0,2),(1,-2..2),(2,-2..2)}: `n_blocks` blocks Blk[q,D] = [Cin][Cin], stored
 * back to back, accumulated over all minibatches of a fit and assembled once:
 *   _plan      : tile edge (64 / 128), number of T x T launch tiles and of blocks for a geometry
 *   _tables    : fills HOST tables  tiles[n_tiles][3] = (column of the A panel, column of the B panel, output offset)
 *                and  slots[H*W][13] = block index of (q, D) or -1; the caller uploads them once per geometry
 *   _accumulate: Blk[q,D] += alpha * sum_b x[b,q,:]^T x[b,q+D,:]   (x: NHWC [B][H][W][Cin]; tiles_dev on the device)
 *   _assemble  : A[(d,ci),(e,cj)] += alpha * sum_{p: p+d, p+e in the map} Blk[p+d, e-d][ci][cj]  (native order)
 * Replaces, like lk_conv3x3_shiftcorr_f32, the per-minibatch A^T A of curvlinops' KFAC for such layers. */
int lk_conv3x3_pixpair_plan(int64_t H, int64_t W, int64_t Cin, int64_t* tile, int64_t* n_tiles, int64_t* n_blocks);
int lk_conv3x3_pixpair_tables(int64_t H, int64_t W, int64_t Cin, int32_t* tiles, int32_t* slots);
int lk_conv3x3_pixpair_accumulate_f32(const float* x, int64_t B, int64_t H, int64_t W, int64_t Cin, float alpha,
                                      float* blocks, const int32_t* tiles_dev, int64_t n_tiles, void* stream);
int lk_conv3x3_pixpair_assemble_f32(const float* blocks, const int32_t* slots_dev, int64_t H, int64_t W, int64_t Cin,
                                    float alpha, float* A, void* stream);
/* _assemble of blocks + blocks2 (blocks2 optional): the accumulators of the two lanes of a fit with two minibatches in
 * flight are summed on the fly, element by element, in the same order as a separate addition would.  upper_only != 0:
 * only the (d, e) blocks with e >= d are written — the upper triangle of A, which is all lk_finalize_factors_f32 and
 * lk_pack_upper_f32 read; the mirrored blocks are one 4-byte access per element and were half of the launch. */
int lk_conv3x3_pixpair_assemble2_f32(const float* blocks, const float* blocks2, const int32_t* slots_dev, int64_t H, int64_t W,
                                     int64_t Cin, float alpha, float* A, int upper_only, void* stream);
/* _accumulate on a split tensor (csrc/lk_sweep16.hip): x as two fp16 planes with one power-of-two scale (lk_split_f16x2 of
 * the NHWC images), three fp16 MFMAs per fp32 product block instead of the exact-fp32 MFMA; same tables, same blocks. */
int lk_conv3x3_pixpair_accumulate_f16x2(const void* x_h, const void* x_l, const int* sexp, int64_t B, int64_t H, int64_t W,
                                        int64_t Cin, float alpha, float* blocks, const int32_t* tiles_dev, int64_t n_tiles,
                                        const void* zero16, void* stream);
/* The same for Cin == 64 with one workgroup per pixel: the pixel's panel is staged once for its (up to) 13 shifts instead of
 * once per (pixel, shift) block — the launch was bound by what a CU ingests, not by the matrix pipe.  slots_dev: the
 * [H W][13] slot table of lk_conv3x3_pixpair_tables (-1: the shifted pixel is outside the map). */
int lk_conv3x3_pixpair_accumulate13_f16x2(const void* x_h, const void* x_l, const int* sexp, int64_t B, int64_t H, int64_t W,
                                          int64_t Cin, float alpha, float* blocks, const int32_t* slots_dev, const void* zero16,
                                          void* stream);

/* Same result as lk_gram_conv_nhwc_f32 for a 3x3 / stride 1 / padding 1 / dilation 1 convolution, through the
 * shift-correlation identity (the input grid equals the output grid, so the 81 (offset, offset) blocks of the
 * patch Gram matrix depend only on the 25 offset differences plus boundary-strip corrections):
 *   C[(d,ci),(e,cj)] += alpha * ( R[e-d] - Row_d[e-d] - Col_d[e-d] + Pix_d[e-d] )[ci][cj]
 * 13 full-grid channel correlations (R[-D] = R[D]^T) instead of the 40.5 block products of the symmetric half.
 * C is written in the native (kh,kw,ci) order, both triangles.  H, W >= 2. */
size_t lk_conv3x3_shiftcorr_workspace_bytes(int64_t B, int64_t H, int64_t W, int64_t Cin);
int lk_conv3x3_shiftcorr_f32(const float* x, int64_t B, int64_t H, int64_t W, int64_t Cin, float alpha, float* C,
                             void* ws, size_t ws_bytes, void* stream);

/* dst[b][h][w][c] = src[b][c][h][w]  (NCHW -> NHWC staging for lk_gram_conv_nhwc_f32). */
int lk_nchw_to_nhwc_f32(const float* src, int64_t B, int64_t C, int64_t HW, float* dst, void* stream);

/* Mirror the upper block triangle written under LK_GRAM_UPPER_ONLY into the lower one. */
int lk_symmetrize_f32(float* C, int64_t n, void* stream);

/* dst[(ci*KK+d), (cj*KK+e)] (+)= src[(d*Cin+ci), (e*Cin+cj)]  — native (kh,kw,ci) -> unfold (ci,kh,kw)
 * order.  accumulate != 0 adds into dst. */
int lk_permute_sym_f32(const float* src, int64_t Cin, int64_t KK, float* dst, int accumulate, void* stream);

/* The once-per-fit layout pass of `count` factors in ONE launch (what CurvlinopsInterface.kron does per minibatch with
 * torch ops on the library's factors, laplace/curvature/curvlinops.py:55-75; here once, on the accumulated sums).
 * Host arrays of length count.  Factor i is n[i] x n[i], upper triangle valid:
 *   kk[i] <= 1: mirrored (in place if dst[i] == NULL), with C[r][c] *= scale[i][r] * scale[i][c] first when scale[i] is
 *               given (the deferred BatchNorm scale of a G factor: diag(s) G diag(s));
 *   kk[i]  > 1: dst[i] = the full matrix in F.unfold's (ci, kh, kw) order from src[i] in the kernels' (kh, kw, ci) order
 *               (n = cin * kk, dst != src, no scale) -- lk_symmetrize_f32 + lk_permute_sym_f32 in one pass. */
int lk_finalize_factors_f32(int64_t count, const float* const* src, float* const* dst, const float* const* scale,
                            const int64_t* n, const int64_t* cin, const int64_t* kk, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Convolution of the seed-batched reverse sweep (csrc/lk_conv.hip): implicit GEMM on NHWC tensors, fp32-level
 * products from two-piece fp16 operands (three v_mfma_f32_32x32x16_f16 per fp32 product block).
 * Replaces the backward-data convolutions inside the C reverse passes of curvlinops' KFACLinearOperator._compute_kfac
 * as driven by CurvlinopsInterface.kron (laplace/curvature/curvlinops.py:87-100); the same GEMM is the forward conv.
 *
 * A "split tensor" is a pair of fp16 planes (h, l) of the tensor's layout plus device ints `sexp`:
 *     x * 2^sexp = h + l (+ e, |e| <= max(2^-22 |x 2^sexp|, 2^-25)),   max|x| * 2^sexp < 2^15,
 * ONE scale for the tensor (the reverse sweep's cotangents: what consumes them are sums over samples) or ONE PER IMAGE of
 * the leading dimension, sexp[n] (the forward's activations: lk_split_images_f16x2, lk_bn_act_fwd_nhwc_f16x2) — the
 * reference computes every sample in fp32 whatever else is in its minibatch (laplace/curvature/curvature.py:375-433), and
 * a ReLU mask decided on an activation resolved only relative to the LARGEST image of the minibatch is not that.
 * ------------------------------------------------------------------------------------------- */
/* out[0] = bit pattern of max_i |x[i] * cscale[(i / inner) % C]| (cscale may be NULL); deterministic. */
int lk_absmax_f32(const float* x, int64_t n, const float* cscale, int64_t inner, int64_t C, unsigned* out, void* stream);
/* fp32 -> split tensor; the scale comes from the DEVICE value amax[0] * bound_mul (any upper bound of max|x|).
 * n % 8 == 0. */
int lk_split_f16x2(const float* x, int64_t n, const float* amax, float bound_mul, void* planes_h, void* planes_l,
                   int* sexp, void* stream);
/* x [N][per] fp32 -> split tensor with one scale per image: sexp[n] from the image's own max|x_n|, which is also left in
 * amax[n] (bit pattern of a float: the measured maximum the next producer derives its bound from).  per % 8 == 0. */
int lk_split_images_f16x2(const float* x, int64_t N, int64_t per, void* planes_h, void* planes_l, int* sexp, unsigned* amax,
                          void* stream);

/* Patch matrix of a convolution (the rows F.unfold produces, laplace/curvature/curvlinops.py:55-75: the A factor of a Conv2d is the
 * Gram of its unfolded inputs) as split planes with ONE scale: x [B][H][W][C] fp32 NHWC -> planes [B * Ho * Wo][Kp], column
 * k = (kh * KW + kw) * C + c (the kernels' native order), zero outside the image and for k >= KH * KW * C (Kp: 64 or a multiple of 128,
 * what lk_gram_tn_f16x2 takes), scale from amax[0] = max|x|.  lk_gram_tn_f16x2 on the result is the A factor of a strided or stem
 * convolution on the fp16 matrix cores at fp32 level (2.6 x faster than lk_gram_conv_nhwc_f32's exact-fp32 MFMA on the c4 layers). */
int lk_im2col_split_f16x2(const float* x, int64_t B, int64_t H, int64_t W, int64_t C, int64_t KH, int64_t KW, int64_t stride,
                          int64_t pad, int64_t Ho, int64_t Wo, int64_t Kp, const float* amax, void* planes_h, void* planes_l,
                          int* sexp, void* stream);
/* W[Co][Ci][taps] (* cscale[co], e.g. a folded BatchNorm scale) -> planes[2][taps][N][K] fp16 + sexp;
 * transpose = 1 (backward-data): n = ci, k = co; 0 (forward): n = co, k = ci.  amax_ws: one device word. */
int lk_conv_prep_weights_f16x2(const float* W, int64_t Co, int64_t Ci, int64_t taps, int transpose, const float* cscale,
                               unsigned* amax_ws, void* planes, int* sexp, void* stream);
/* One launch of the implicit GEMM
 *     out[n][i*out_step + oh0][j*out_step + ow0][co] (+)= sum_t sum_c in[n][i*in_mul + dh_t][j*in_mul + dw_t][c] * Wt[wt_t][co][c]
 * for i < Hc, j < Wc (taps outside the [Hi][Wi] image contribute zero).  in: split tensor [N][Hi][Wi][Ci], Ci % 32 == 0,
 * with in_nsexp = 1 scale or in_nsexp = N scales (one per image: GEMM rows never mix images, the epilogue un-scales row by row);
 * w: split planes [.][Co][Ci]; taps: T x {dh, dw, wt} (T <= 9, host array); zero16: >= 16 zero bytes on the device;
 * out: fp32 [N][Ho][Wo][Co]; accumulate != 0 adds into out; amax_out (may be NULL): atomicMax of the bit patterns of
 * |out| (zero it first).  Stride-1 backward-data and forward convs are one launch, a stride-s backward-data is one
 * launch per output-pixel residue class.  config bit 0: 64-deep K chunks; bit 1: never use the form that keeps
 * the input patch of a tile resident in LDS across the taps (used when the output grid is the input grid);
 * bit 4: write the output position-contiguous, out[n][co][pixel] (dense grids, Ho*Wo % 4 == 0, no accumulate);
 * bits 12..14: tile shape of the generic form — 0: chosen from the shapes by occupancy (a pure function of the arguments),
 * 1: 64x64, 2: 128x64, 3: 64x128, 4: 128x128, 5: 256x64, 6: the big tile by output width only; the remaining bits select
 * development variants of the K pipeline (csrc/lk_conv.hip).  Every choice computes the same sums in the same order. */
int lk_conv_nhwc_f16x2(const void* in_h, const void* in_l, const int* in_sexp, int64_t in_nsexp, int64_t N, int64_t Hi,
                       int64_t Wi, int64_t Ci, const void* w_h, const void* w_l, const int* w_sexp, int64_t Co, int64_t Hc,
                       int64_t Wc, int64_t in_mul, int64_t Ho, int64_t Wo, int64_t out_step, int64_t oh0, int64_t ow0,
                       int64_t T, const int* taps, const void* zero16, float* out, int accumulate, unsigned* amax_out,
                       int config, void* stream);

/* lk_conv_nhwc_f16x2 with a dense, POSITION-contiguous output emitted as a split tensor: out_h / out_l [N][Co][Ho * Wo] fp16,
 * scaled per entry of in_sexp (the whole tensor, or image by image) from the guaranteed bound
 *     max|out_n| <= in_amax[n] * w_l1[0]        (in_amax: in_nsexp words, bit patterns, or NULL = 2^(15 - in_sexp[n]); w_l1:
 *                                                max_co sum_{t,c} |Wt[t][co][c]|, device word)
 * with the scale left in out_sexp[n].  (Ho * Wo) % 4 == 0; in_mul = the convolution's stride.  This is how the Kron predictive's
 * eigenbasis rotations (laplace/utils/matrix.py:406-456: Q1^T over the output cotangents as a 1x1 convolution, the unfolded
 * inputs times Q2 as a convolution whose filters are the eigenvectors) hand their results to
 * lk_kron_quadform_shared_planes_f16x2: no fp32 round trip, nothing left to split inside the quadratic-form kernel. */
int lk_conv_nhwc_f16x2_planes(const void* in_h, const void* in_l, const int* in_sexp, int64_t in_nsexp, const void* in_amax,
                              int64_t N, int64_t Hi, int64_t Wi, int64_t Ci, const void* w_h, const void* w_l,
                              const int* w_sexp, const float* w_l1, int64_t Co, int64_t Ho, int64_t Wo, int64_t in_mul, int64_t T,
                              const int* taps, const void* zero16, void* out_h, void* out_l, int* out_sexp, int config,
                              void* stream);

/* lk_conv_nhwc_f16x2 (dense output grid; in_mul = the convolution's stride) with the forward's eval-mode BatchNorm, residual
 * add and ReLU in its epilogue — the model's forward pass inside GGNInterface / CurvlinopsInterface
 * (laplace/curvature/curvature.py:309-311 `self.model(x)`; torchvision-style conv -> bn -> (+ identity) -> relu blocks):
 *     y[n][i][j][c] = act(conv[n][i][j][c] * scale[c] + shift[c] + addend[n][i][j][c])        act: 0 none, 1 ReLU
 * To the bit what lk_conv_nhwc_f16x2 followed by lk_bn_act_fwd_nhwc_f16x2 (x_mul = w_l1, no x_add) computes — the same fp32
 * operations in the same order — in one launch and without the fp32 round trip of the convolution's output.  in_amax:
 * in_namax (1 or N) words with the measured max|in_n|; w_l1: max_co sum |W[co]| (device word).  Outputs: y fp32 NHWC, mask
 * (NHWC bytes y > 0, may be NULL), y_h / y_l (both or none: the split planes of y with one scale per image, y_sexp[N], from the
 * guaranteed bound y_bound[N] = in_amax[n] w_l1 max|scale| + max|shift| + addend_bound[n]), y_amax[N] (measured max|y_n| as bit
 * patterns; zeroed by the caller).  Co % 8 == 0; addend_bound: 1 or N floats. */
int lk_conv_bn_act_nhwc_f16x2(const void* in_h, const void* in_l, const int* in_sexp, int64_t in_nsexp, const void* in_amax,
                              int64_t in_namax, int64_t N, int64_t Hi, int64_t Wi, int64_t Ci, const void* w_h, const void* w_l,
                              const int* w_sexp, const float* w_l1, int64_t Co, int64_t Ho, int64_t Wo, int64_t in_mul,
                              int64_t T, const int* taps, const void* zero16, const float* scale, const float* shift,
                              const void* scale_amax, const void* shift_amax, const float* addend, const float* addend_bound,
                              int64_t addend_nbound, int act, float* y, void* mask, void* y_h, void* y_l, int* y_sexp,
                              float* y_bound, void* y_amax, int config, void* stream);

/* lk_conv_nhwc_f16x2 with the element-wise VJP of the sweep fused into its epilogue (one dense launch: forward / stride-1
 * backward-data; Co % 8 == 0):
 *     o[n][i][j][c] = (conv[n][i][j][c] + add[n][i][j][c]) * M[(n,i,j) mod mask_rows][c] * scale[c]
 * emitted as a split tensor out_h / out_l / out_sexp — what lk_vjp_nhwc_split_f16x2 would make of the fp32 output, without
 * that tensor's round trip through HBM (the backward passes of laplace/curvature/curvlinops.py:87-100 through an
 * activation / folded BatchNorm / residual join).  The result's scale is derived before the launch from a guaranteed
 * bound: max|in| (in_amax: measured, device word, or NULL = 2^(15 - in_sexp)) * w_l1 (device word: max_n sum_{t,k}
 * |Wt[t][n][k]| of the prepared weights) + 2^(15 - add_sexp), times max|M| (mult_amax, fp32 multipliers only) and
 * max|scale|; out_amax (zeroed by the caller) receives the MEASURED max|o|, which the next launch takes as its in_amax.
 * add / mask / scale may be NULL.  mask: uint8 (mask_is_float = 0) or fp32 [mask_rows][Co]. */
int lk_conv_nhwc_f16x2_vjp(const void* in_h, const void* in_l, const int* in_sexp, const void* in_amax, int64_t N, int64_t Hi,
                           int64_t Wi, int64_t Ci, const void* w_h, const void* w_l, const int* w_sexp, const float* w_l1,
                           int64_t Co, int64_t Ho, int64_t Wo, int64_t T, const int* taps, const void* zero16,
                           const void* add_h, const void* add_l, const int* add_sexp, const void* mask, int mask_is_float,
                           const void* mult_amax, int64_t mask_rows, const float* scale, const void* scale_amax, void* out_h,
                           void* out_l, int* out_sexp, void* out_amax, int config, void* stream);
/* lk_conv_nhwc_f16x2_vjp with the weights ALSO handed over chunk-major (wc_h / wc_l: [tap][Ci / 16][Co][16] fp16 per plane,
 * same scale w_sexp): 3 x 3 / stride-1 launches with 64 output channels on maps of more than 64 pixels and Ci <= 4064
 * (lk_conv_winp_eligible; the chunk count Ci / 16 travels in an 8-bit field of the kernel's tile descriptor) then run the PERSISTENT window form — two workgroups per CU walk through the pixel tiles, the
 * input window of a tile resident in LDS, the next tile's operands requested under the epilogue; the chunk-major order
 * makes every weight staging instruction one contiguous kilobyte.  Other shapes ignore the extra planes. */
int lk_conv_winp_eligible(int64_t N, int64_t Hi, int64_t Wi, int64_t Ci, int64_t Co, int64_t T, int mask_is_float);
int lk_conv_nhwc_f16x2_vjp_wc(const void* in_h, const void* in_l, const int* in_sexp, const void* in_amax, int64_t N, int64_t Hi,
                              int64_t Wi, int64_t Ci, const void* w_h, const void* w_l, const int* w_sexp, const float* w_l1,
                              const void* wc_h, const void* wc_l, int64_t Co, int64_t Ho, int64_t Wo, int64_t T, const int* taps,
                              const void* zero16, const void* add_h, const void* add_l, const int* add_sexp, const void* mask,
                              int mask_is_float, const void* mult_amax, int64_t mask_rows, const float* scale,
                              const void* scale_amax, void* out_h, void* out_l, int* out_sexp, void* out_amax, int config,
                              void* stream);

/* The backward-data of a STRIDED convolution (stride `os` = 2; reference: the torch.func Jacobians of curvature.py:94-147
 * run it once per output class through autograd) with every residue class of the input-gradient pixels in ONE launch —
 * class (oh0, ow0): dX[i*os + oh0, j*os + ow0] = sum over that class's taps of g[i + dh, j + dw] W[slice] — optionally
 * together with a SECOND convolution that reads the same input (in2_* / w2_*, NULL without one: the 1 x 1 shortcut of a
 * residual down-sampling block, with its own cotangent and weights), and with the element-wise VJP fused as in
 * lk_conv_nhwc_f16x2_vjp: out = (dX + dX2 + add) * M * scale[channel] as a split tensor with its measured max|.|.
 * taps: T <= 12 rows {dh, dw, weight slice, source (0 / 1), oh0, ow0}; every one of the os*os classes needs a tap;
 * both cotangents are [N][Hi][Wi][Ci] with Hi = Ho / os, Wi = Wo / os; weights [slice][Co][Ci] per plane. */
int lk_conv_nhwc_f16x2_vjp_strided(const void* in_h, const void* in_l, const int* in_sexp, const void* in_amax, const void* w_h,
                                   const void* w_l, const int* w_sexp, const float* w_l1, const void* in2_h, const void* in2_l,
                                   const int* in2_sexp, const void* in2_amax, const void* w2_h, const void* w2_l,
                                   const int* w2_sexp, const float* w2_l1, int64_t N, int64_t Hi, int64_t Wi, int64_t Ci,
                                   int64_t Co, int64_t Ho, int64_t Wo, int64_t os, int64_t T, const int* taps,
                                   const void* zero16, const void* add_h, const void* add_l, const int* add_sexp,
                                   const void* mask, int mask_is_float, const void* mult_amax, int64_t mask_rows,
                                   const float* scale, const void* scale_amax, void* out_h, void* out_l, int* out_sexp,
                                   void* out_amax, int config, void* stream);


/* Element-wise VJP of the NHWC sweep with a split result (csrc/lk_sweep16.hip):
 *     out[s][e] = (g[s][e] + g2[s][e]) * M[e] * scale[e % C]      e < per = B*H*W*C,  s < S
 * g: fp32 addend with the bit pattern of max|g| in g_amax (both may be NULL); g2: split addend (may be NULL);
 * M: per-sample multiplier, uint8 mask or fp32 (m_amax: bit pattern of max|M| for fp32, NULL = 1), may be NULL;
 * scale: per-channel (scale_amax: bit pattern of max|scale|), may be NULL.  The output scale is derived on the device
 * from the guaranteed bound (max|g| + max|g2|) max|M| max|scale| — no pass over the data to find it. */
int lk_vjp_nhwc_split_f16x2(const float* g, const unsigned* g_amax, const void* g2_h, const void* g2_l, const int* g2_sexp,
                            const void* m, int m_is_float, const unsigned* m_amax, const float* scale,
                            const unsigned* scale_amax, int64_t C, int64_t S, int64_t per, void* out_h, void* out_l,
                            int* out_sexp, void* stream);
/* Forward of the NHWC sweep: y = act(x * scale[c] + shift[c] + addend) on fp32 NHWC tensors x [N][per], act 0 none /
 * 1 ReLU / 2 tanh (replaces BatchNorm2d-eval + add + activation, three library launches per layer), producing in the same
 * pass the ReLU mask as NHWC bytes and the split planes of y for the next convolution with ONE SCALE PER IMAGE, image n
 * scaled from the guaranteed bound
 *     y_bound[n] = bx_n max|scale| + max|shift| + addend_bound[n],   bx_n = x_amax[n] * x_mul[0] + x_add[0] >= max|x_n|   (tanh: 1)
 * x_amax: x_namax = 1 or N words (bit patterns; for a convolution's output: the measured maxima of its INPUT images, with
 * x_mul = the l1 norm of its weights and x_add = max|bias|; x_mul / x_add may be NULL = 1 / 0); addend_bound: 1 or N floats.
 * y_amax (N words, zeroed by the caller; may be NULL) receives the MEASURED max|y_n| — the next layer's x_amax, so the
 * slack of the bound does not compound.  scale_amax / shift_amax: device words with bit patterns of the maxima; addend,
 * mask, y_h / y_l may be NULL.  C % 8 == 0, per % C == 0, N <= 65535. */
int lk_bn_act_fwd_nhwc_f16x2(const float* x, const unsigned* x_amax, int64_t x_namax, const float* x_mul, const float* x_add,
                             const float* scale, const float* shift, const unsigned* scale_amax, const unsigned* shift_amax,
                             const float* addend, const float* addend_bound, int64_t addend_nbound, int act, int64_t C,
                             int64_t N, int64_t per, float* y, void* mask, void* y_h, void* y_l, int* y_sexp, float* y_bound,
                             unsigned* y_amax, void* stream);
/* y[0..n) = x[0..n) and *amax = max(*amax, max|x|) (bit pattern of a non-negative float; NOT reset: the word runs over the
 * minibatches stacked for one pixel-pair launch, which are then split with it instead of being measured in a pass of
 * their own).  16-byte aligned buffers, n % 4 == 0. */
int lk_copy_absmax_f32(const float* x, float* y, int64_t n, unsigned* amax, void* stream);

/* Row-major packed upper triangle of a symmetric n x n factor (what the ranks of a data-parallel fit exchange: half the
 * bytes of the square): packed[i n - i (i - 1) / 2 + (j - i)] = A[i][j], j >= i.  Unpacking writes the upper triangle only. */
int lk_pack_upper_f32(const float* A, int64_t n, float* packed, void* stream);
int lk_unpack_upper_f32(const float* packed, int64_t n, float* A, void* stream);

/* Eigenbasis algebra of KronDecomposed (laplace/utils/matrix.py:406-461: `_bmm` at exponents -1 / -1/2, i.e. the
 * materialised-Jacobian GLM predictive `inv_square_form` and the posterior samples of baselaplace.py:1845-1858).
 * lk_gemm_f32: batched  C[b] = alpha (op(A[b]) . op(B[b])) (.) E  (+ C[b] if accumulate) on the exact-fp32 MFMA; matrices
 * row-major with leading dimensions, batch strides (0 = shared operand), op = transpose if trans_x != 0 (A stored K x M,
 * B stored N x K), E optional M x N weight (lde = 0: one row broadcast).
 * lk_kron_pow_f32: lam[i][j] = (l1[i] l2[j] + delta)^e (damping: ((l1[i] + sqrt delta)(l2[j] + sqrt delta))^e;
 * l2 == NULL: (l1[i] + delta)^e); delta is a device scalar. */
int lk_gemm_f32(const float* A, const float* B, const float* E, float* C, int64_t batch, int64_t M, int64_t N, int64_t K,
                int64_t lda, int64_t ldb, int64_t ldc, int64_t lde, int64_t stride_a, int64_t stride_b, int64_t stride_c,
                int trans_a, int trans_b, float alpha, int accumulate, void* stream);
int lk_kron_pow_f32(const float* l1, int64_t n1, const float* l2, int64_t n2, const float* delta, float exponent,
                    int damping, float* lam, void* stream);
/* Split NHWC cotangent x [S*B][L][C] (seed-major batch) -> fp32 out[b][s][c][l]: position-contiguous and sample-major,
 * the `u` operand of lk_kron_quadform_shared_f32 / lk_diag_quadform_shared_f32. */
int lk_unsplit_transpose_f32(const void* x_h, const void* x_l, const int* sexp, int64_t S, int64_t B, int64_t L, int64_t C,
                             float* out, void* stream);
/* G[C][C] += alpha * X^T X for a split tensor X [R][C] (rows = (seed, sample, position) of an NHWC cotangent): the
 * G factor of a convolution layer (curvlinops.py:87-100).  Only the 32x32 tiles on or above the diagonal are written
 * (lk_symmetrize_f32 mirrors).  C = 64 or a multiple of 128.  Deterministic (workspace partials, fixed-order sum). */
size_t lk_gram_tn_f16x2_workspace_bytes(int64_t R, int64_t C);
int lk_gram_tn_f16x2(const void* x_h, const void* x_l, const int* sexp, int64_t R, int64_t C, float alpha, float* G,
                     const void* zero16, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Diagonal GGN / EF.  Replaces GGNInterface.diag / EFInterface.diag (curvature.py:413-433,494-505)
 * for nn.Linear layers:  h_w[o][i] += alpha * sum_n (sum_c g[c][n][o]^2) a[n][i]^2,
 *                        h_b[o]    += alpha * sum_n  sum_c g[c][n][o]^2          (h_b may be NULL)
 * a: [B][Di], g: [Cc][B][Do].
 * ------------------------------------------------------------------------------------------- */
int lk_diag_ggn_linear_f32(const float* a, const float* g, int64_t B, int64_t Cc, int64_t Di, int64_t Do,
                           float alpha, float* h_w, float* h_b, void* stream);

/* Per-sample weight Jacobians of one layer written into Js[B][C][P] at column `col0`
 * (replaces the jacrev materialisation of CurvatureInterface.jacobians, curvature.py:88-129):
 *   linear: Js[n][c][col0 + o*Di + i] = g[c][n][o] * a[n][i];  bias: Js[n][c][bcol0 + o] = g[c][n][o]
 *   conv  : Js[n][c][col0 + o*Dk + k] = sum_l g[c][n][o][l] * patches[n][l][k]   (patches NHWC-native
 *           order is converted to unfold order on the fly) */
int lk_jac_linear_f32(const float* a, const float* g, int64_t B, int64_t Cc, int64_t Di, int64_t Do,
                      float* Js, int64_t P, int64_t col0, int64_t bcol0, void* stream);
int lk_jac_conv_f32(const float* x_nchw, const float* g, int64_t B, int64_t Cc, int64_t Cin, int64_t H, int64_t W,
                    int64_t Do, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                    float* Js, int64_t P, int64_t col0, int64_t bcol0, void* stream);

/* Per-sample Jacobian of an affine normalisation layer y = w * xhat + b (eval-mode BatchNorm1d/2d, LayerNorm,
 * GroupNorm) w.r.t. w and b, written into Js[B][S][P] (replaces the norm-parameter columns of the jacrev materialisation
 * of CurvatureInterface.jacobians, laplace/curvature/curvature.py:88-129, and - with lk_sq_colsum_f32 on the block - of
 * GGNInterface.diag / EFInterface.diag, curvature.py:413-433, 494-505):
 *   Js[n][s][wcol0 + ch] = sum_l g * xhat      (skipped when wcol0 < 0)
 *   Js[n][s][bcol0 + ch] = sum_l g             (skipped when bcol0 < 0)
 * g:    [S][B][Ch][L] (layout 0, channels first: NCHW cotangents, GroupNorm, BatchNorm1d on [B, C, L])
 *    or [S][B][L][Ch] (layout 1, channels last: LayerNorm over the last dim(s), NHWC cotangents), fp32 in both;
 * xhat: [B][..] in the same layout, ONE copy shared by all S seeds (xhat does not depend on w, b).
 * Every other column of Js is left untouched.  Deterministic (no atomics; one owner per output, fixed reduction tree). */
int lk_jac_norm_affine_f32(const float* g, const float* xhat, int64_t S, int64_t B, int64_t L, int64_t Ch, int layout,
                           float* Js, int64_t P, int64_t wcol0, int64_t bcol0, void* stream);

/* The same Jacobian for a norm layer tapped on the NHWC split-fp16 reverse sweep, read where that sweep leaves the cotangent
 * of the layer's output (replaces the same norm-parameter columns of CurvatureInterface.jacobians,
 * laplace/curvature/curvature.py:88-129, and of GGNInterface.diag / EFInterface.diag, curvature.py:413-433, 494-505):
 *   g:  [S][B][L][Ch] as the two fp16 planes g_h, g_l of a ONE-scale split tensor, g = (float(h) + float(l)) * 2^-sexp[0]
 *       (sexp: one device int);
 *   x:  [B][L][Ch] fp32, ONE copy for all seeds; mu, rstd: [Ch], given together or both null;
 *   xhat = (x - mu[ch]) * rstd[ch], formed in registers (no activation-sized xhat tensor exists); x itself when both are null;
 *   Js[n][s][wcol0 + ch] = sum_l g * xhat      (skipped when wcol0 < 0)
 *   Js[n][s][bcol0 + ch] = sum_l g             (skipped when bcol0 < 0)
 * fp32 accumulation, the power-of-two scale applied once at the store.  Every other column of Js is left untouched.
 * Deterministic: no atomics, one owner per output, a fixed reduction tree (xor-shuffles inside a wave, then LDS), plain stores.
 * Few (sample, channel tile) pairs: the seeds are split over grid.y; L is never split.
 * Minimal traffic: 4 S B L Ch + 4 B L Ch + 8 B S Ch bytes.
 * Contract: g_h, g_l, sexp, x, Js non-null; 1 <= S, 0 <= B, S * B < 2^31; 1 <= L < 2^30; 1 <= Ch < 2^30; S * B * L * Ch < 2^40;
 * B * (channel tiles per sample) < 2^31; column ranges inside P and not overlapping.  B == 0, or both offsets negative, returns
 * LK_OK.
 * lk_normtap_variant (host only): the path a shape takes; `affine`: mu and rstd are given; `aligned`: g_h, g_l, x, mu and rstd
 * are 16-byte aligned.  Returns
 *   vector class | seed-split << 2 | affine << 3 | seeds per pass << 4 | log2(lane rows per workgroup) << 8 |
 *   seeds per grid.y slice (capped at 255) << 12 | channel tiles per sample (capped at 2047) << 20
 *   vector class: 0 one channel per lane, 1 four (8-byte plane loads; Ch % 4 == 0 and aligned), 2 eight (16-byte plane loads;
 *   Ch % 8 == 0 and aligned); seeds per pass: how many seeds' plane loads a lane has in flight
 * or a negative value for a shape the entry point refuses. */
int lk_jac_norm_affine_nhwc_f16x2(const void* g_h, const void* g_l, const int* sexp, const float* x, const float* mu,
                                  const float* rstd, int64_t S, int64_t B, int64_t L, int64_t Ch, float* Js, int64_t P,
                                  int64_t wcol0, int64_t bcol0, void* stream);
int lk_normtap_variant(int64_t S, int64_t B, int64_t L, int64_t Ch, int affine, int aligned);

/* Forward and input VJP of the per-sample normalisation layers (nn.GroupNorm, nn.LayerNorm) for the seed-batched reverse
 * sweep; they replace the reverse passes through these layers of laplace/curvature/curvlinops.py:87-100 (the KFAC backward)
 * and of the jacrev materialisation of CurvatureInterface.jacobians, laplace/curvature/curvature.py:88-129 (one stock
 * autograd pass per seed).  Geometry as lk_jac_norm_affine_f32: layout 0 is [B][Ch][L], layout 1 is [B][L][Ch]; a statistics
 * row is (n, group) with N = (Ch / G) * L elements.  nn.GroupNorm(G, Ch) is either layout with that G; nn.LayerNorm is
 * layout 1 with B = product of the leading dims, L = 1, Ch = prod(normalized_shape), G = 1.
 *
 * lk_norm_fwd_f32: biased variance by the mean-shifted two-pass form, rstd = 1 / sqrt(var + eps), xhat = (x - mu) * rstd,
 *   y = w[ch] * xhat + b[ch]; w and b may be null (no affine).  rstd is [B * G].  Always a lane group per statistics row: in
 *   layout 1 with L > 1 and Ch / G not a multiple of 4 it reads 4 bytes per lane (DESIGN.md has the measured cost).
 * lk_norm_vjp_f32: g is [S][B].. in the layout of xhat (ONE xhat and rstd per sample for all seeds):
 *   t = w * g;  m1 = mean_row(t);  m2 = mean_row(t * xhat);  dx = rstd * (t - m1 - xhat * m2)
 *   w may be null.  amax, when given, receives max|dx| as the bit pattern of a non-negative float through atomicMax (as
 *   amax_out of lk_conv_nhwc_f16x2); the caller zeroes it.  dx must not overlap g.  Deterministic: one owner per element,
 *   fixed reduction trees, plain stores.
 * Contract of both: layout 0 or 1; G >= 1 divides Ch; 1 <= S < 2^31, 0 <= B < 2^31, 1 <= L, Ch < 2^30, N < 2^31; B == 0
 * returns LK_OK.
 * lk_norm_sweep_variant (host only): the kernel and path lk_norm_vjp_f32 takes for a shape; `aligned`: g, xhat and dx are
 * 16-byte aligned.  Returns
 *   kernel | vec << 1 | two-pass << 2 | seed-split << 3 | lanes << 4 | groups << 16
 *   kernel: LK_NORMVJP_ROW (a lane group per statistics row) or LK_NORMVJP_TILE (layout 1 with narrow groups: a workgroup owns
 *   `groups` adjacent groups of a sample); vec: 16-byte loads; two-pass: the row does not stay on chip, g is read twice;
 *   seed-split: the seeds are split over grid.y; lanes: per row (ROW) or across the channel vectors (TILE)
 * or a negative value for a shape the entry point refuses. */
#define LK_NORMVJP_ROW 0
#define LK_NORMVJP_TILE 1
int lk_norm_fwd_f32(const float* x, const float* w, const float* b, int64_t B, int64_t L, int64_t Ch, int64_t G, int layout,
                    float eps, float* y, float* xhat, float* rstd, void* stream);
int lk_norm_vjp_f32(const float* g, const float* xhat, const float* rstd, const float* w, int64_t S, int64_t B, int64_t L,
                    int64_t Ch, int64_t G, int layout, float* dx, unsigned* amax, void* stream);
int lk_norm_sweep_variant(int64_t S, int64_t B, int64_t L, int64_t Ch, int64_t G, int layout, int aligned);

/* Forward and input VJP of nn.RMSNorm (the pre-norm of LLaMA / Mistral / Gemma / T5 blocks) for the seed-batched reverse
 * sweep; they replace the reverse passes through this layer of laplace/curvature/curvlinops.py:87-100 (the KFAC backward)
 * and of the jacrev materialisation of CurvatureInterface.jacobians, laplace/curvature/curvature.py:88-129 (one stock
 * autograd pass per seed).  x is [rows][D]: rows = product of the leading dims, D = prod(normalized_shape).
 *
 * lk_rmsnorm_fwd_f32: r = 1 / sqrt(mean_row(x^2) + eps) with the mean of squares in fp32 and no subtraction anywhere;
 *   y = w[d] * (x * r); w may be null.  Writes y and rstd [rows] only: xhat = x * rstd is one multiply away from the input, so
 *   no activation-sized xhat is stored.
 * lk_rmsnorm_vjp_f32: g is [S][rows][D] (ONE x and rstd per row for all seeds):
 *   t = w * g;  xh = x * rstd;  m2 = mean_row(t * xh);  dx = rstd * (t - xh * m2)          (there is no mean_row(t) term)
 *   w may be null.  amax, when given, receives max|dx| as the bit pattern of a non-negative float through atomicMax (as
 *   lk_norm_vjp_f32); the caller zeroes it.  dx must not overlap g.  Deterministic: one owner per element, a fixed xor-shuffle
 *   tree per row, plain vector stores, no atomics on data.  Minimal traffic: 4 (2 S + 1) rows D bytes.
 * Contract of both: x, y / g, dx and rstd non-null; 1 <= S < 2^31, 0 <= rows < 2^31, 1 <= D < 2^30, S * rows * D < 2^40 (the
 *   forward has S = 1); rows == 0 returns LK_OK.
 * lk_rmsnorm_variant (host only): the path lk_rmsnorm_vjp_f32 takes for a shape; `aligned`: g, x, dx and w are 16-byte
 * aligned.  Returns
 *   vec | two-pass << 1 | seed-split << 2 | log2(lanes) << 3 | min(seeds per slice, 2^24 - 1) << 6
 *   vec: 16-byte loads and stores (D % 4 == 0 and aligned), else 4-byte ones; two-pass: the row does not stay in registers
 *   (more than 8 vectors per lane), g is read twice; seed-split: the seeds are split over grid.y; lanes: a group of 1 .. 64
 *   lanes owns a row; seeds per slice: how many seeds one workgroup loops over
 * or a negative value for a shape the entry points refuse. */
int lk_rmsnorm_fwd_f32(const float* x, const float* w, int64_t rows, int64_t D, float eps, float* y, float* rstd,
                       void* stream);
int lk_rmsnorm_vjp_f32(const float* g, const float* x, const float* rstd, const float* w, int64_t S, int64_t rows, int64_t D,
                       float* dx, unsigned* amax, void* stream);
int lk_rmsnorm_variant(int64_t S, int64_t rows, int64_t D, int aligned);

/* Scaled dot-product self-attention (F.scaled_dot_product_attention without mask tensor or dropout, Tq == Tk) for the
 * seed-batched reverse sweep; they replace the reverse passes through an attention core of
 * laplace/curvature/curvlinops.py:87-100 (the KFAC backward) and of the jacrev materialisation of
 * CurvatureInterface.jacobians, laplace/curvature/curvature.py:88-129 (one stock autograd pass per seed).  fp32 throughout,
 * products on the exact fp32 matrix instructions.  Layout 0 is [B][H][T][D], layout 1 is [B][T][H][D]; go, dq, dk, dv carry a
 * leading [S] in the same layout; lse is always [B][H][T].  Causal: key j <= query i.
 *
 * lk_attn_fwd_f32: P = softmax(scale * q k^T (+ causal mask)) by the running-maximum form (the row maximum is always
 *   subtracted before exp), o = P v, lse = row maximum + log(row sum) of the scaled, masked scores.
 * lk_attn_vjp_f32: ALL S seeds from ONE q, k, v, o, lse per sample; P is rebuilt on chip, P = exp(scale * q k^T - lse):
 *   dv = P^T go,  dP = go v^T,  delta = rowsum(go o o),  dS = P o (dP - delta),  dq = scale dS k,  dk = scale dS^T q.
 *   Two owner passes: 64 query rows own dq and delta [S][B][H][T] (in ws), 64 key rows own dk and dv.  One owner per
 *   element, fixed reduction order, plain stores, no atomics: two equal calls are bit-equal.  T == 1 gives dq = dk = 0 and
 *   dv = go exactly.  ws: lk_attn_vjp_workspace_bytes(S, B, H, T, D) bytes (0 for a refused shape), 16-byte aligned.
 *   Minimal traffic: 4 S B H T D * (2 reads of go + 3 writes) + 8 S B H T (delta, written and read) + the per-sample
 *   operands (q, k, v twice, o, lse: 24 B H T D + 8 B H T) bytes.
 * Contract: pointers non-null and 16-byte aligned; layout 0 or 1; D % 4 == 0, 4 <= D <= 128; 1 <= T < 2^15; 1 <= S, 0 <= B,
 * S * B < 2^31; 1 <= H < 2^16; S * B * H * T * D < 2^40; B * H * ceil(T / 64) < 2^31; scale finite; no output (ws included)
 * overlaps an input; ws_bytes at least the workspace size.  B == 0 returns LK_OK.
 * lk_attn_variant (host only): the path lk_attn_vjp_f32 takes for a shape.  Returns
 *   resident | seed-split << 1 | log2(DP / 16) << 2 | causal << 4 | layout << 5 | seeds per grid.y slice (capped at 255) << 8 |
 *   owner blocks per (b, h) (capped at 4095) << 16
 *   resident: T <= LK_ATTN_RESIDENT_MAX_T, an owner's [64][T] block of P is built once into LDS and the seeds loop over it
 *   (else it is rebuilt per seed); seed-split: the seeds are split over grid.y (each slice builds P once); DP: D padded to
 *   16, 32, 64 or 128 (the kernel instantiation); owner blocks: ceil(T / 64), the rows of a workgroup (streamed side: stages
 *   of 32 rows)
 * or a negative value for a shape the entry points refuse. */
#define LK_ATTN_RESIDENT_MAX_T 256
int lk_attn_fwd_f32(const float* q, const float* k, const float* v, int64_t B, int64_t H, int64_t T, int64_t D, int layout,
                    float scale, int causal, float* o, float* lse, void* stream);
size_t lk_attn_vjp_workspace_bytes(int64_t S, int64_t B, int64_t H, int64_t T, int64_t D);
int lk_attn_vjp_f32(const float* go, const float* q, const float* k, const float* v, const float* o, const float* lse, int64_t S,
                    int64_t B, int64_t H, int64_t T, int64_t D, int layout, float scale, int causal, float* dq, float* dk,
                    float* dv, void* ws, size_t ws_bytes, void* stream);
int lk_attn_variant(int64_t S, int64_t B, int64_t H, int64_t T, int64_t D, int layout, int causal);

/* The same attention with STRIDED operands, for a packed projection (nn.MultiheadAttention's in_proj, a fused qkv Linear): the
 * operands are read where the projection left them and the cotangent is written where the projection's VJP reads it, so
 * neither the three slice copies nor the concatenation of dq, dk, dv exist.
 *   q, k, v: [B][T][H][D] with a row stride of ldq floats; for one [B][T][3 H D] projection q = qkv, k = qkv + H D,
 *     v = qkv + 2 H D, ldq = 3 H D.
 *   dq, dk, dv: [S][B][T][H][D] with a row stride of ldd floats; the three may interleave in one [S][B][T][3 H D] buffer.
 *     Every element of all three is written (no zero fill needed); what lies between the rows is not touched.
 *   o, go: layout 1 ([B][T][H][D], go with a leading [S]); lse [B][H][T].
 * The same kernels and the same arithmetic in the same order as layout 1: with ldq = ldd = H D the results are bit-equal to
 * lk_attn_fwd_f32 / lk_attn_vjp_f32 with layout = 1.  One owner per element, no atomics, two equal calls are bit-equal.  The
 * workspace is that of lk_attn_vjp_workspace_bytes, the path what lk_attn_variant(S, B, H, T, D, 1, causal) names.
 * Contract: that of the layout-1 entry points, and: ldq >= H D, ldd >= H D, both multiples of 4; B T ldq < 2^40,
 * S B T ldd < 2^40; no output overlaps an input (extents from the first to the last element); dq, dk, dv may interleave but
 * share no element.  The forward has no ldd. */
int lk_attn_fwd_strided_f32(const float* q, const float* k, const float* v, int64_t ldq, int64_t B, int64_t H, int64_t T, int64_t D,
                            float scale, int causal, float* o, float* lse, void* stream);
int lk_attn_vjp_strided_f32(const float* go, const float* q, const float* k, const float* v, int64_t ldq, const float* o,
                            const float* lse, int64_t S, int64_t B, int64_t H, int64_t T, int64_t D, float scale, int causal,
                            float* dq, float* dk, float* dv, int64_t ldd, void* ws, size_t ws_bytes, void* stream);

/* Max and average pooling (nn.MaxPool2d / nn.AvgPool2d, ceil_mode false, no dilation) on fp32 NHWC feature maps for the NHWC
 * reverse sweep; they replace, there, max_pool2d(return_indices=True) / avg_pool2d and the seed-expanded scatter_add_ of the
 * NCHW sweep (the reverse passes of laplace/curvature/curvlinops.py:87-100 and curvature.py:88-129 through a pooling layer).
 * OH = (H + 2 ph - kh) / sh + 1, OW likewise; the window of (oh, ow) starts at (oh * sh - ph, ow * sw - pw).
 *
 * lk_pool_fwd_nhwc_f32: x [B][H][W][C] -> y [B][OH][OW][C].
 *   LK_POOL_MAX: the maximum over the window's in-image taps (padding takes no part); arg [B][OH][OW][C], one byte each, is
 *     the window-local tap code dy * kw + dx of the FIRST maximum in row-major scan order (strict >, torch's tie rule).
 *   LK_POOL_AVG: (sum of the in-image taps) / div with div = divisor_override when it is > 0, else kh * kw when
 *     count_include_pad is set, else the number of in-image taps; arg must be null.
 * lk_pool_vjp_nhwc_f32: g [S][B][OH][OW][C] -> dx [S][B][H][W][C], ONE arg for all seeds.  Gather form: the owner of a dx
 *   element walks the windows that cover its pixel in fixed (oh, ow) order and adds g where the window's code names the pixel
 *   (max) or g / div(window) (average).  Plain stores, no atomics on data: deterministic.  amax, when given, receives max|dx|
 *   as the bit pattern of a non-negative float through atomicMax (as lk_norm_vjp_f32); the caller zeroes it.  dx must not
 *   overlap g.  Minimal traffic: 4 S B C (OH OW + H W) + B C OH OW bytes.
 * Contract of both: kind 0 or 1; 1 <= kh, kw <= 8; 1 <= sh, sw < 32768; 0 <= ph <= kh / 2, 0 <= pw <= kw / 2; OH, OW >= 1;
 * 1 <= H, W < 32768; 1 <= C < 2^30; 1 <= S, 0 <= B, S * B < 2^31; S * B * C * max(H * W, OH * OW) < 2^40; arg non-null exactly
 * for LK_POOL_MAX.  B == 0 returns LK_OK.
 * lk_pool_variant (host only): the path lk_pool_vjp_nhwc_f32 takes for a shape; `aligned`: g and dx are 16-byte and arg is
 * 4-byte aligned.  Returns
 *   vec | summing << 1 | seed-split << 2 | seeds per pass << 4 | seeds per grid.y slice (capped at 65535) << 12
 *   vec: 16-byte loads of g, 4-byte loads of arg (C % 4 == 0 and aligned); summing: two windows may share a pixel (otherwise
 *   SELECTION: kh <= sh and kw <= sw, dx is a copy or a zero); seed-split: the seeds are split over grid.y; seeds per pass:
 *   how many seeds' loads a lane has in flight
 * or a negative value for a shape the entry point refuses. */
#define LK_POOL_MAX 0
#define LK_POOL_AVG 1
int lk_pool_fwd_nhwc_f32(int kind, const float* x, int64_t B, int64_t H, int64_t W, int64_t C, int kh, int kw, int sh, int sw,
                         int ph, int pw, int count_include_pad, int divisor_override, float* y, uint8_t* arg, void* stream);
int lk_pool_vjp_nhwc_f32(int kind, const float* g, const uint8_t* arg, int64_t S, int64_t B, int64_t H, int64_t W, int64_t C,
                         int kh, int kw, int sh, int sw, int ph, int pw, int count_include_pad, int divisor_override, float* dx,
                         unsigned* amax, void* stream);
int lk_pool_variant(int kind, int64_t S, int64_t B, int64_t H, int64_t W, int64_t C, int kh, int kw, int sh, int sw, int ph,
                    int pw, int aligned);

/* Depthwise convolution (nn.Conv2d with groups == in_channels == out_channels, no dilation, zero padding) on NHWC feature
 * maps for the NHWC reverse sweep; they replace, there, the module's own forward and convolution_backward with `groups` of the
 * NCHW sweep (the reverse pass through a depthwise layer of laplace/curvature/curvlinops.py:87-100 and curvature.py:88-129).
 * OH = (H + 2 ph - kh) / sh + 1, OW likewise.  Weights are tap-major fp32: w_tap[kh kw][C], w_tap[dy kw + dx][c] =
 * weight[c, 0, dy, dx].
 *
 * lk_dwconv_fwd_nhwc_f32: x [B][H][W][C] -> y [B][OH][OW][C],
 *   y = bias[c] + sum over the in-image taps, in fixed (dy, dx) order, of w_tap[dy kw + dx][c] * x[n, oh sh - ph + dy, ow sw - pw + dx, c];
 *   bias may be null.
 * lk_dwconv_bwd_nhwc_f16x2: the cotangent g [S][B][OH][OW][C] as the two fp16 planes g_h, g_l of a ONE-scale split tensor,
 *   g = (float(h) + float(l)) * 2^-sexp[0] (sexp: one device int) -> dx [S][B][H][W][C] fp32,
 *   dx[s,n,h,w,c] = sum over (dy, dx) in fixed row-major order with (h + ph - dy) % sh == 0, (w + pw - dx) % sw == 0 and
 *   oh = (h + ph - dy) / sh in [0, OH), ow likewise, of w_tap[dy kw + dx][c] * g[s,n,oh,ow,c].
 *   Gather form: every dx element has one owner, plain stores, deterministic; a pixel no window reaches receives 0.  amax, when
 *   given, receives max|dx| as the bit pattern of a non-negative float through atomicMax (as lk_pool_vjp_nhwc_f32); the caller
 *   zeroes it.  dx must not overlap g.  Minimal traffic: 4 S B C (OH OW + H W) + 4 kh kw C bytes.
 * Contract of both: 1 <= kh, kw and kh * kw <= 25; 1 <= sh, sw <= 8; 0 <= ph < kh, 0 <= pw < kw; OH, OW >= 1; 1 <= H, W < 32768;
 * 1 <= C < 2^30; 1 <= S, 0 <= B, S * B < 2^31; S * B * C * max(H * W, OH * OW) < 2^40.  B == 0 returns LK_OK.
 * lk_dwconv_variant (host only): the path lk_dwconv_bwd_nhwc_f16x2 takes for a shape; `aligned`: g_h and g_l are 8-byte, w_tap
 * and dx 16-byte aligned.  Returns
 *   vec | strided << 1 | seed-split << 2 | tap class << 3 | seeds per pass << 4 | seeds per grid.y slice (capped at 65535) << 12
 *   vec: 8-byte loads of the planes, 16-byte loads of w_tap and stores of dx (C % 4 == 0 and aligned); strided: sh > 1 or
 *   sw > 1, the divisibility test is live; seed-split: the seeds are split over grid.y; tap class: 0 for <= 9 taps, 1 for
 *   <= 25; seeds per pass: how many seeds' loads a lane has in flight
 * or a negative value for a shape the entry point refuses. */
int lk_dwconv_fwd_nhwc_f32(const float* x, const float* w_tap, const float* bias, int64_t B, int64_t H, int64_t W, int64_t C,
                           int kh, int kw, int sh, int sw, int ph, int pw, float* y, void* stream);
int lk_dwconv_bwd_nhwc_f16x2(const void* g_h, const void* g_l, const int* sexp, const float* w_tap, int64_t S, int64_t B,
                             int64_t H, int64_t W, int64_t C, int kh, int kw, int sh, int sw, int ph, int pw, float* dx,
                             unsigned* amax, void* stream);
int lk_dwconv_variant(int64_t S, int64_t B, int64_t H, int64_t W, int64_t C, int kh, int kw, int sh, int sw, int ph, int pw,
                      int aligned);

/* Channel concatenation (torch.cat along dim 1 of [B, C, H, W] maps) on NHWC feature maps for the NHWC reverse sweep; they
 * replace, there, torch.cat and - in the reverse pass - a .float() per split part, a sum over the whole map, a strided
 * narrow().contiguous() per source and a pass for max|.| (the reverse passes of laplace/curvature/curvlinops.py:87-100 and
 * curvature.py:88-129 through a concatenation).  Rows are the R = N H W pixels of a map; a slice is channels [c0, c0 + Cs) of
 * a map with Ct channels.
 *
 * lk_cat_fwd_nhwc_f32: dst[r Ct + c0 + c] = src[r Cs + c]; src [R][Cs] contiguous, dst [R][Ct]; one launch per source.
 *   (replaces torch.cat in the forward of curvlinops.py:87-100.)  Minimal traffic 8 R Cs bytes.
 * lk_cat_vjp_nhwc_f32: dst[r Cs + c] = sum_p value_p[r Ct + c0 + c] over nparts parts (1 <= nparts <= LK_CAT_MAX_PARTS); f32,
 *   hi, lo and sexp are HOST arrays of nparts device pointers (read before the call returns, passed to the kernel by value).
 *   Part p is the fp32 map f32[p] [R][Ct] when that pointer is non-null; otherwise a ONE-scale split tensor: fp16 planes hi[p]
 *   and lo[p] [R][Ct] and the device word sexp[p][0], value = (float(hi) + float(lo)) * 2^-sexp.  The sum runs in fp32, left to
 *   right in the listed order; dst is a contiguous [R][Cs] map; one owner per dst element, plain stores, no atomics on data:
 *   deterministic.  amax, when given, receives max|dst| as the bit pattern of a non-negative float through atomicMax (as
 *   lk_pool_vjp_nhwc_f32); the caller zeroes it.  dst must not overlap a part.  (replaces the reverse pass of curvature.py:88-129
 *   through a concatenation.)  Minimal traffic: R Cs (4 + 4 n_f32 + 4 n_split) bytes - only the slice of every part is read.
 * Contract of both: pointers non-null where used; 1 <= Cs, 0 <= c0, c0 + Cs <= Ct < 2^30; 0 <= R, R * Ct < 2^40; dst does not
 * overlap src / a part.  R == 0 returns LK_OK.
 * lk_cat_variant (host only): the path lk_cat_vjp_nhwc_f32 takes for a shape; split_mask: bit p set when part p is a split
 * tensor; `aligned`: the fp32 maps and dst are 16-byte, the planes 8-byte aligned.  Returns
 *   vec | nparts << 1 | split_mask << 4 | 64-bit lane index << 8 | workgroups of the grid << 12
 *   vec: 16-byte fp32 loads and stores, 8-byte loads of four halves (Ct, c0 and Cs multiples of 4, and aligned), else one
 *   element per lane; nparts and split_mask select the kernel instance and the loads of each part; 64-bit lane index: R * Cs
 *   (/ 4 with vec) >= 2^31; the grid strides over the lanes with at most 2048 workgroups of 256 threads
 * or a negative value for a shape the entry point refuses. */
#define LK_CAT_MAX_PARTS 4
int lk_cat_fwd_nhwc_f32(const float* src, int64_t R, int64_t Cs, float* dst, int64_t Ct, int64_t c0, void* stream);
int lk_cat_vjp_nhwc_f32(int nparts, const float* const* f32, const void* const* hi, const void* const* lo,
                        const int* const* sexp, int64_t R, int64_t Ct, int64_t c0, int64_t Cs, float* dst, unsigned* amax,
                        void* stream);
int lk_cat_variant(int nparts, int split_mask, int64_t R, int64_t Ct, int64_t c0, int64_t Cs, int aligned);

/* Static slicing (Tensor.chunk / split / narrow, x[:, a:b], x[:, 0]) for the seed-batched reverse sweeps: the transpose of the
 * concatenation above.  A slice along dim d of a contiguous [N, ...] tensor is a column range of the row matrix
 * [R = N prod(dims before d)][Ct = prod(dims from d)]; a piece is columns [c0, c0 + cs) of it.  They replace, in the reverse
 * pass of laplace/curvature/curvlinops.py:87-100 and curvature.py:88-129 through a slice, a zero fill of the whole tensor and a
 * strided read-modify-write per slice, a sum of the full-width tensors and a pass for max|.|.
 *
 * lk_slice_fwd_f32: dst[r Cs + c] = src[r Ct + c0 + c]; src [R][Ct], dst a contiguous [R][Cs].  Minimal traffic 8 R Cs bytes.
 * lk_slice_vjp_f32: dst[r Ct + c] = the value of the first listed piece p with c0[p] <= c < c0[p] + cs[p], plus the later
 *   covering pieces in the listed order, in fp32; +0.0f where no piece covers c.  f32, hi, lo, sexp, c0 and cs are HOST arrays of
 *   npieces entries (read before the call returns; the metadata reaches the kernel by value).  Piece p is a contiguous
 *   [R][cs[p]]: the fp32 map f32[p] when that pointer is non-null, otherwise a ONE-scale split tensor as in lk_cat_vjp_nhwc_f32:
 *   fp16 planes hi[p], lo[p] and the device word sexp[p][0], value = (float(hi) + float(lo)) * 2^-sexp.  A full-width cotangent
 *   is the piece (0, Ct); pieces may overlap or repeat.  One owner per dst element, plain stores, no atomics on data:
 *   deterministic.  amax, when given, receives max|dst| as the bit pattern of a non-negative float through atomicMax (as
 *   lk_cat_vjp_nhwc_f32); the caller zeroes it.  Minimal traffic: 4 R Ct bytes written plus every piece read once.
 * Contract of both: pointers non-null where used; 1 <= npieces <= LK_SLICE_MAX_PIECES; 1 <= cs, 0 <= c0, c0 + cs <= Ct < 2^30;
 * 0 <= R, R * Ct < 2^40; dst does not overlap src / a piece.  R == 0 returns LK_OK.
 * lk_slice_variant (host only): the path lk_slice_vjp_f32 takes for a shape; split_mask: bit p set when piece p is a split
 * tensor; `aligned`: the fp32 maps and dst are 16-byte, the planes 8-byte aligned.  Returns
 *   vec | npieces << 1 | split_mask << 5 | 64-bit lane index << 13 | workgroups of the grid << 14
 *   bit 0 vec: 16-byte fp32 loads and stores, 8-byte loads of four halves (Ct and every c0 and cs multiples of 4, and aligned),
 *   else one element per lane; bits 1-4 npieces and bits 5-12 split_mask select the kernel instance and the loads of each
 *   piece; bit 13: R * Ct (/ 4 with vec) >= 2^31 lanes; bits 14 and up: the grid, at most 2048 workgroups of 256 threads that
 *   stride over the lanes
 * or a negative value for a shape the entry point refuses. */
#define LK_SLICE_MAX_PIECES 8
int lk_slice_fwd_f32(const float* src, int64_t R, int64_t Ct, int64_t c0, int64_t Cs, float* dst, void* stream);
int lk_slice_vjp_f32(int npieces, const float* const* f32, const void* const* hi, const void* const* lo,
                     const int* const* sexp, const int64_t* c0, const int64_t* cs, int64_t R, int64_t Ct, float* dst,
                     unsigned* amax, void* stream);
int lk_slice_variant(int npieces, int split_mask, const int64_t* c0, const int64_t* cs, int64_t R, int64_t Ct, int aligned);

/* Maximum over positions (x.amax(2), x.max(2)[0], AdaptiveMaxPool1d(1): what 1-D ResNets, text CNNs and PointNets end in) for
 * the seed-batched reverse sweep.  The operand is a contiguous fp32 [outer][L][inner], L the product of the reduced dims.  They
 * replace, in the reverse pass of laplace/curvature/curvlinops.py:87-100 and curvature.py:88-129 through such a reduction, a
 * zero fill of the whole [S][outer][L][inner] tensor and a scatter per seed.
 *
 * lk_maxred_fwd_f32: y[o][i] = max_l x[o][l][i]; idx[o][i] (int32) = the first l that holds it; cnt[o][i] (int32) = how many l
 *   compare equal to it (0.0 == -0.0, as torch compares).  A row with a NaN gives NaN in y; its idx and cnt are unspecified.
 *   inner == 1: a group of 1 .. 64 lanes per row and a fixed xor-shuffle tree on (value, index, count) items ordered "larger
 *   value, then smaller index" (the result does not depend on the tree); inner > 1: a lane per (outer, inner vector) that walks
 *   l.  A reduction is never split over workgroups.
 * lk_maxred_vjp_f32: g is [S][outer][inner], dx [S][outer][L][inner], all seeds in one launch.  With idx alone (x, y, cnt null)
 *   dx = (l == idx) ? g : +0.0f (max(dim), the adaptive max pools: the first maximum); with x, y and cnt (idx is ignored)
 *   dx = (x == y) ? g / cnt : +0.0f (amax: an even split over the maxima; one fp32 division).  Every element of dx is written:
 *   the caller fills nothing.  One owner per element, plain stores, no atomics: deterministic.  idx / x, y, cnt of an element
 *   are read once for all seeds.  Minimal traffic: 4 S (outer inner)(L + 1) bytes.
 * Contract of both: pointers non-null where used; 1 <= S < 2^31 (the forward has S = 1), 0 <= outer, 1 <= L < 2^30,
 *   1 <= inner < 2^30, outer * inner < 2^31, S * outer * L * inner < 2^40; the outputs overlap no operand (nor, in the forward,
 *   each other).  outer == 0 returns LK_OK.  Errors: "<entry>: bad arguments (...)".
 * lk_reduce_variant (host only): the path a shape takes in the forward (vjp == 0) or the VJP (vjp != 0; `even`: x, y, cnt are
 * given); `aligned`: every pointer is 16-byte aligned.  Returns
 *   row | vec << 1 | even << 2 | 64-bit lane index << 3 | log2(lanes per row) << 4 | seed-split << 7 | workgroups << 8
 *   row: inner == 1; vec: 16-byte accesses (forward: inner % 4 == 0; VJP: inner % 4 == 0, or L % 4 == 0 where inner == 1; and
 *   aligned); seed-split: the seeds are split over grid.y; workgroups: at most 2048 of 256 threads stride over the work
 * or a negative value for a shape the entry points refuse. */
int lk_maxred_fwd_f32(const float* x, int64_t outer, int64_t L, int64_t inner, float* y, int* idx, int* cnt, void* stream);
int lk_maxred_vjp_f32(const float* g, const int* idx, const float* x, const float* y, const int* cnt, int64_t S, int64_t outer,
                      int64_t L, int64_t inner, float* dx, void* stream);
int lk_reduce_variant(int vjp, int64_t S, int64_t outer, int64_t L, int64_t inner, int even, int aligned);

/* Static, separable, linear resampling of the last two dims (nn.Upsample / F.interpolate: nearest, nearest-exact, linear,
 * bilinear, bicubic, area, with or without antialias; F.pad and the padding modules: constant, reflect, replicate, circular,
 * cropping pads included) for the seed-batched reverse sweep.  Per plane the operation is y = Mh x Mw^T + const with static sparse
 * axis matrices Mh [OH][H], Mw [OW][W].  It replaces, in the reverse pass of laplace/curvature/curvlinops.py:87-100 and
 * curvature.py:88-129 through such an operation as stock torch runs it once per seed, upsample_*_backward,
 * reflection_pad*_backward and replication_pad*_backward, which accumulate with atomics (the bits change from run to run), or
 * the zero fill and strided copy of a constant pad.
 *
 * lk_resample_vjp_f32: g is [P][OH][OW], dx [P][H][W], contiguous fp32, all seeds in one launch (P = S B C planes).
 *   dx[p][h][w] = sum_{j in [ptr_h[h], ptr_h[h + 1])} sum_{i in [ptr_w[w], ptr_w[w + 1])} w_h[j] * w_w[i] * g[p][idx_h[j]][idx_w[i]]
 *   in fp32, j ascending, then i, formed as acc += w_h[j] * (sum_i w_w[i] * g).  (ptr, idx, w) of an axis is the TRANSPOSE of
 *   its matrix in CSR form: ptr [L + 1] int32, idx int32 ascending per entry, w float32, all on the device.  Every element of dx
 *   is written: an input that no output reads (a cropped border) receives +0.0f; the caller fills nothing.  One owner per
 *   element, plain stores, no atomics, a fixed tap order: deterministic.  A lane reads the taps of its pixels once for all
 *   planes of its slice.  Minimal traffic: 4 P (OH OW + H W) bytes; the reuse of g among neighbouring lanes is left to the caches.
 * Contract: pointers non-null; 1 <= P; 1 <= OH, OW, H, W < 2^30; P * max(OH * OW, H * W) < 2^40; ptr monotone from 0 with
 *   ptr[L] = nnz; 0 <= idx_h < OH, 0 <= idx_w < OW; at most LK_RESAMPLE_MAX_TAPS taps per entry; dx overlaps no operand.  The
 *   tables live on the device and are NOT validated by the entry point (the caller validates them when it builds them); what is
 *   free is done there: a longer list is cut at LK_RESAMPLE_MAX_TAPS and an index is clamped into the plane, so that no table
 *   content makes the kernel write outside dx.  The scalars, the pointers and the overlap (g and the ptr arrays in full, the tap
 *   arrays by their first entry) are checked.  Errors: "lk_resample_vjp_f32: bad arguments (...)".
 * lk_resample_variant (host only): the path a shape takes; taps_h / taps_w: the longest tap list of each axis; `aligned`: dx is
 * 16-byte aligned.  Returns
 *   vec | taps-in-registers << 1 | 64-bit lane index << 2 | plane-split << 3 | grid-stride << 4 | packed slices << 5 |
 *   workgroups of grid.x << 8
 *   vec: 16-byte stores (W % 4 == 0 and aligned), else one pixel per lane; taps-in-registers: both lists hold at most 4 taps
 *   (decided per lane on the device: this is the answer for the longest lists); 64-bit lane index: H * W (/ 4 with vec) >= 2^31;
 *   plane-split: the planes are split into slices over grid.y (one plane leaves the device short of waves); grid-stride: one
 *   plane has more lanes than the at most 2048 workgroups of 256 threads of grid.x; packed slices: a plane has at most 128
 *   lanes and a workgroup takes 256 / lanes slices side by side
 * or a negative value for a shape the entry point refuses or a tap count outside 0 .. LK_RESAMPLE_MAX_TAPS. */
#define LK_RESAMPLE_MAX_TAPS 16
int lk_resample_vjp_f32(const float* g, int64_t P, int64_t OH, int64_t OW, int64_t H, int64_t W, const int* ptr_h, const int* idx_h,
                        const float* w_h, const int* ptr_w, const int* idx_w, const float* w_w, float* dx, void* stream);
int lk_resample_variant(int64_t P, int64_t OH, int64_t OW, int64_t H, int64_t W, int taps_h, int taps_w, int aligned);

/* Element-wise product of two traced tensors (squeeze-and-excitation gates, GLU / SwiGLU / GeGLU, self-gating) for the
 * seed-batched reverse sweep.  It replaces, in the reverse pass of laplace/curvature/curvlinops.py:87-100 and
 * curvature.py:88-129 through out = a * b as stock torch runs it once per seed, g * b, g * a and - for a gate - a sum over the
 * trailing dims: five passes over [S*B, ...] tensors.
 *
 * lk_mul_vjp_f32: g [S][R][L] is the cotangent of a * b for all S seeds; a [R][L]; b [R][L] (b_row == 0, full form) or [R]
 *   (b_row == 1, row gate: R = B * prod(dims before the gate's trailing ones), L the product of the remaining dims).
 *     da[s][r][l] = g[s][r][l] * b[r][l] (b[r] for a row gate)                               da [S][R][L]
 *     db[s][r][l] = g[s][r][l] * a[r][l]  /  db[s][r] = sum_l g[s][r][l] * a[r][l]           db [S][R][L] / [S][R]
 *   da or db may be NULL (that output is not computed), not both.  One launch for all seeds: g is read once for both outputs,
 *   a and b once per sample row.  Plain fp32, one rounding per product; the row sum adds in a fixed order (lane-strided partial
 *   sums, then a xor-shuffle tree); one owner per output element, plain stores, no atomics, deterministic.
 *   Minimal traffic: 4 S R L bytes of g, a and b once, and the outputs asked for.
 * Contract: g, a, b and at least one output non-null; b_row 0 or 1; 1 <= S, 0 <= R, 1 <= L < 2^30, S * R * L < 2^40; no output
 *   overlaps an input or the other output.  R == 0 returns LK_OK.
 * lk_mul_variant (host only): the path lk_mul_vjp_f32 takes for a shape; want_da / want_db: which outputs are asked for;
 * `aligned`: every pointer is 16-byte aligned.  Returns
 *   form | vec << 1 | log2(lanes per row) << 2 | resident << 5 | seed-split << 6 | wide << 7 | da << 8 | db << 9 |
 *   workgroups of grid.x << 10
 *   bit 0 form: 1 row gate, 0 full form; bit 1 vec: 16-byte loads and stores (L % 4 == 0 and aligned), else 4-byte ones;
 *   bits 2-4: a group of 1 .. 64 lanes owns a row (0 in the full form: a lane owns one vector of the flattened [R * L]);
 *   bit 5 resident: a of a row stays in registers across the seed loop (at most 8 vectors per lane; always in the full form),
 *   else it is re-read per seed; bit 6: the seeds are split over grid.y; bit 7 wide: S * R * L >= 2^31, an element offset
 *   passes 31 bits (the kernel indexes with 64 bits throughout); bits 8 and 9: the outputs; bits 10 and up: at most 2048
 *   workgroups of 256 threads that stride over the rows / vectors
 * or a negative value for a shape the entry point refuses. */
int lk_mul_vjp_f32(const float* g, const float* a, const float* b, int64_t S, int64_t R, int64_t L, int b_row, float* da,
                   float* db, void* stream);
int lk_mul_variant(int64_t S, int64_t R, int64_t L, int b_row, int want_da, int want_db, int aligned);

/* Squeeze-and-excitation gate out = x * gate[B, C, 1, 1] on NHWC feature maps for the NHWC reverse sweep.  They replace, there,
 * the reverse pass of laplace/curvature/curvlinops.py:87-100 through such a block as the NCHW route runs it: the product rule on
 * an NCHW copy of the cotangent, the pooling cotangent expanded to the whole map, and the add of the two.
 * N = S B maps, seed-major; P = H W positions; C channels innermost.  The cotangent g [N][P][C] is EITHER the fp32 map g (g_h,
 * g_l and sexp null) OR - g null - a ONE-scale split tensor read as it lies: fp16 planes g_h and g_l [N][P][C] and the device
 * word sexp[0], value = (float(g_h) + float(g_l)) * 2^-sexp, exactly as lk_cat_vjp_nhwc_f32 forms it.
 *
 * lk_gate_reduce_nhwc_f32: ds[s][b][c] = sum_p g[s B + b][p][c] * x[b][p][c]; x [B][P][C] fp32, one copy per sample shared by
 *   all seeds; ds [S B][C] fp32.  One launch for all seeds; fp32 accumulation; lanes across the channels, the sum over the
 *   positions in a fixed order (per thread every (256 / lanes)-th position in ascending order, then a fixed tree over the
 *   position groups); one owner per ds element, no atomics: bit-reproducible.  x stays in registers across the seed loop while
 *   a thread owns at most 16 positions, else it is re-read per seed; few (sample, channel tile) units: the seeds go over grid.y.
 *   Minimal traffic: g once, x once, 4 S B C bytes of ds.
 * lk_gate_vjp_nhwc_f32: dx[s B + b][p][c] = g[s B + b][p][c] * gate[b][c] + r[s B + b][c]; gate [B][C] fp32; r [S B][C] fp32 or
 *   NULL (the cotangent of the pooled tensor, already divided by P); dx [N][P][C] fp32.  One launch for all seeds, g read
 *   once; gate of the sample and r of the map stay in registers along the positions; one owner per element, plain stores, no
 *   atomics on data.  With r NULL dx is the fp32 product (one rounding).  amax, when given, receives max|dx| as the bit pattern
 *   of a non-negative float through atomicMax (as lk_cat_vjp_nhwc_f32); the caller zeroes it.
 * Contract of both: pointers non-null where used; exactly one form of g; 1 <= S, 0 <= B, 1 <= P < 2^30, 1 <= C < 2^30,
 *   S * B * P * C < 2^40; no output overlaps an input.  B == 0 returns LK_OK before any device call.
 * lk_gate_variant (host only): the path a shape takes; vjp: 0 the reduce, 1 the VJP; `aligned`: the fp32 bases are 16-byte, the
 * planes 8-byte aligned.  Returns
 *   vec | resident << 1 | seed-split << 2 | wide << 3 | log2(lanes across the channel vectors) << 4 | workgroups of grid.x << 8
 *   bit 0 vec: 16-byte fp32 accesses, 8-byte loads of four halves (C % 4 == 0 and aligned), else one element per lane; bit 1
 *   resident (reduce): x stays in registers across the seed loop; bit 2 (reduce): the seeds are split over grid.y; bit 3 wide:
 *   S * B * P * C >= 2^31, an element offset passes 31 bits (the kernels index with 64 bits throughout); bits 4-6: 1 .. 64 lanes
 *   across the channel vectors of a position (256 / lanes position groups); bits 8 and up: at most 2048 workgroups of 256 threads
 * or a negative value for a shape the entry points refuse. */
int lk_gate_reduce_nhwc_f32(const float* g, const void* g_h, const void* g_l, const int* sexp, const float* x, int64_t S,
                            int64_t B, int64_t P, int64_t C, float* ds, void* stream);
int lk_gate_vjp_nhwc_f32(const float* g, const void* g_h, const void* g_l, const int* sexp, const float* gate, const float* r,
                         int64_t S, int64_t B, int64_t P, int64_t C, float* dx, unsigned* amax, void* stream);
int lk_gate_variant(int vjp, int64_t S, int64_t B, int64_t P, int64_t C, int aligned);

/* Softmax / log-softmax along the last, contiguous dim (hand-written attention, attention pooling, soft mixture gates,
 * log-softmax head features) for the seed-batched reverse sweep.  It replaces, in the reverse pass of
 * laplace/curvature/curvlinops.py:87-100 and curvature.py:88-129 through y = softmax(x) as stock torch runs it once per seed,
 * S calls of the softmax backward that each read y again.
 *
 * lk_softmax_vjp_f32: g [S][R][L] is the cotangent of y for all S seeds; y [R][L] is the forward's OUTPUT (probabilities, or
 *   log-probabilities with is_log == 1), one per sample row for all seeds.
 *     is_log == 0:  dx[s][r][l] = y[r][l] * (g[s][r][l] - sum_j g[s][r][j] y[r][j])
 *     is_log == 1:  dx[s][r][l] = g[s][r][l] - exp(y[r][l]) * sum_j g[s][r][j]
 *   One launch for all seeds; y (exp(y), computed once) of a row stays in registers across the seeds while the row fits.  Plain
 *   fp32; the row sum adds in a fixed order (lane-strided partial sums, then a xor-shuffle tree); one owner per output element,
 *   plain stores, no atomics, deterministic.  y[r][l] == 0 gives dx == 0 exactly (for finite g).
 *   Minimal traffic: 8 S R L bytes (g read, dx written) plus y once.
 * Contract: g, y, dx non-null; is_log 0 or 1; 1 <= S, 0 <= R, 1 <= L < 2^30, S * R * L < 2^40; dx overlaps neither input.
 *   R == 0 returns LK_OK.
 * lk_softmax_vjp_variant (host only): the path lk_softmax_vjp_f32 takes for a shape; `aligned`: every pointer is 16-byte
 * aligned.  Returns
 *   vec | log2(lanes per row) << 1 | resident << 4 | seed-split << 5 | wide << 6 | is_log << 7 | workgroups of grid.x << 8
 *   bit 0 vec: 16-byte loads and stores (L % 4 == 0 and aligned), else 4-byte ones; bits 1-3: a group of 1 .. 64 lanes owns a
 *   row; bit 4 resident: y and the seed's g of a row stay in registers (at most 8 vectors per lane), else both are re-read per
 *   seed; bit 5: the seeds are split over grid.y; bit 6 wide: S * R * L >= 2^31 (the kernel indexes with 64 bits throughout);
 *   bits 8 and up: at most 2048 workgroups of 256 threads that stride over the rows
 * or a negative value for a shape the entry point refuses. */
int lk_softmax_vjp_f32(const float* g, const float* y, int64_t S, int64_t R, int64_t L, int is_log, float* dx, void* stream);
int lk_softmax_vjp_variant(int64_t S, int64_t R, int64_t L, int is_log, int aligned);

/* Batched matrix product of two traced tensors (hand-written attention q @ k^T and p @ v, bilinear heads) for the
 * seed-batched reverse sweep.  It replaces, in the reverse pass of laplace/curvature/curvlinops.py:87-100 and
 * curvature.py:88-129 through out = a @ b as stock torch runs it once per seed, two batched products per seed.
 *
 * lk_matmul_vjp_f32: g [S][NB][M][N] is the cotangent of a @ b for all S seeds (seed-major, as the sweep leaves it);
 *   a [NB][M][K] and b [NB][K][N] are the per-sample operands, shared by all seeds.
 *     da[s][n] = g[s][n] b[n]^T     da [S][NB][M][K]   (reduction over N)
 *     db[s][n] = a[n]^T g[s][n]     db [S][NB][K][N]   (reduction over M)
 *   da or db may be NULL (that output is not computed), not both.  One launch per requested output; a workgroup owns a
 *   64 x 64 output tile of one sample matrix and loops over the seeds inside: the operand panel of the tile is staged into LDS
 *   once for all seeds of the slice while the reduction depth (N for da, M for db) is at most 128, and restaged per seed
 *   beyond that.  Exact fp32 matrix instruction, the reduction index ascends in a fixed order, one owner per output element,
 *   plain stores, no atomics: deterministic.  No copy of g, a or b is made; sizes need not be multiples of anything.
 *   Minimal traffic: g once per requested output, a and b once, the outputs once.
 * Contract: g, a, b and at least one output non-null; 1 <= S, 0 <= NB, 1 <= M, K, N < 2^24; S * NB * M * N, S * NB * M * K
 *   and S * NB * K * N < 2^40; NB * ceil(M / 64) * ceil(K / 64) and NB * ceil(K / 64) * ceil(N / 64) < 2^31; no output
 *   overlaps an input or the other output.  NB == 0 returns LK_OK.
 * lk_matmul_vjp_variant (host only): the path lk_matmul_vjp_f32 takes for a shape.  Returns
 *   da | db << 1 | resident(da) << 2 | resident(db) << 3 | seed-split << 4 | wide << 5 | workgroups << 6
 *   bits 0 and 1: the outputs asked for; bits 2 and 3: that output's operand panel stays in LDS across the seeds (4-byte
 *   accesses throughout: there is no vector-width bit); bit 4: the seeds are split over grid.y; bit 5 wide: an element offset
 *   passes 31 bits (64-bit offsets throughout); bits 6 and up: the workgroups of grid.x summed over the requested outputs
 *   (saturating at 2^24 - 1)
 * or a negative value for a shape the entry point refuses. */
int lk_matmul_vjp_f32(const float* g, const float* a, const float* b, int64_t S, int64_t NB, int64_t M, int64_t K, int64_t N,
                      float* da, float* db, void* stream);
int lk_matmul_vjp_variant(int64_t S, int64_t NB, int64_t M, int64_t K, int64_t N, int want_da, int want_db);

/* Per-sample weight Jacobian of a GROUPED convolution (nn.Conv2d(groups > 1): depthwise, channel multipliers, narrow
 * groups), written into Js[B][C][P] (replaces the grouped-convolution columns of the jacrev materialisation of
 * CurvatureInterface.jacobians, laplace/curvature/curvature.py:88-129):
 *   Js[n][c][col0 + o*Dkg + k] = sum_l g[c][n][o][l] * patch[n][l][grp(o)*Cig + ci][dy][dx]
 *   Js[n][c][bcol0 + o]        = sum_l g[c][n][o][l]                                  (skipped when bcol0 < 0)
 * Cig = Cin / groups, Dkg = Cig*kh*kw, k = (ci, dy, dx) as weight[o].flatten(), grp(o) = o / (Do / groups); groups must
 * divide Cin and Do.  x_nchw: [B][Cin][H][W], g: [Cc][B][Do][OH*OW].  With groups = 1 this is lk_jac_conv_f32's contract.
 * Depthwise layers (Cig = 1, kh*kw <= 49) run a streaming reduction with any B*Cc; every other shape runs the 16 x 16 tile
 * scheme and needs B*Cc <= 65535 and groups * ceil(Do/groups/16) <= 65535.  Every other column of Js is left untouched.
 * Deterministic (no atomics; one owner per output, fixed reduction tree). */
int lk_jac_gconv_f32(const float* x_nchw, const float* g, int64_t B, int64_t Cc, int64_t Cin, int64_t H, int64_t W,
                     int64_t Do, int64_t groups, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                     float* Js, int64_t P, int64_t col0, int64_t bcol0, void* stream);

/* nn.Embedding weight W[V][D] with token ids ids[B][T]: the per-sample Jacobian is a segmented sum of the cotangent
 * g[S][B][T][D] of the module's output (replaces the embedding columns of the jacrev materialisation of
 * CurvatureInterface.jacobians, laplace/curvature/curvature.py:88-129, and of GGNInterface.diag / EFInterface.diag,
 * curvature.py:413-433, 494-505):
 *   lk_jac_embed_f32:            Js[b][s][col0 + v*D + d]  = sum over {t : ids[b][t] == v} of g[s][b][t][d]
 *   lk_diag_embed_f32:           h[v*D + d]               += alpha * sum_(s, b) (that sum)^2        (never forms [B][S][V*D])
 *   lk_diag_quadform_embed_f32:  fvar[b][c][k]            += sum_v sum_d r_c[d] * r_k[d] * var[v*D + d],  r_c the sum of class c
 * The ids arrive SORTED (int64, torch's stable sort; the host never reads them): `order` / `sorted_ids` are the argsort and the
 * sorted values of ids.reshape(-1) (b-major, so one id's positions are ordered by (b, t)); `order_row` / `sorted_ids_row`, both
 * [B][T], those of ids.sort(dim=1, stable=True).  The thread group at the first sorted position of a run of equal keys owns
 * the run's outputs and walks it in ascending order; every other group exits: one owner per output element, no atomics, the same
 * bits on every launch.  A run whose id is padding_idx (-1: the module has none) or lies outside [0, V) writes nothing;
 * lk_jac_embed_f32 leaves every element of Js that is no such sum untouched (the caller has zeroed it).
 * 1 <= S (or C) < 2^31, 0 <= B, 1 <= T, 1 <= D, 1 <= V, B*T < 2^31, V*D < 2^31, 0 <= col0, col0 + V*D <= P; B == 0 is LK_OK.
 * 16-byte accesses where D % 4 == 0 and the pointers (and P, col0) are 16-byte aligned, 4-byte otherwise.
 *
 * lk_embed_variant (host only): vec | slots << 1 | lanes << 12 | chunks << 20 for a shape, `aligned` as above.  vec: 16-byte
 * accesses; lanes (<= 16): across the d vectors of lk_diag_embed_f32's workgroup; slots = 1024 / lanes: the row slots a long run
 * of one id is cut into (the long-run path, reduced through LDS in ascending order); chunks: its grid.y (saturating at 2047).  Negative for
 * a shape the entry points refuse. */
int lk_jac_embed_f32(const float* g, const int64_t* order, const int64_t* sorted_ids, int64_t S, int64_t B, int64_t T, int64_t D,
                     int64_t V, int64_t padding_idx, float* Js, int64_t P, int64_t col0, void* stream);
int lk_diag_embed_f32(const float* g, const int64_t* order, const int64_t* sorted_ids, int64_t S, int64_t B, int64_t T, int64_t D,
                      int64_t V, int64_t padding_idx, float alpha, float* h, void* stream);
int lk_diag_quadform_embed_f32(const float* g, const int64_t* order_row, const int64_t* sorted_ids_row, int64_t C, int64_t B,
                               int64_t T, int64_t D, int64_t V, int64_t padding_idx, const float* var, float* fvar,
                               void* stream);
int lk_embed_variant(int64_t S, int64_t B, int64_t T, int64_t D, int aligned);

/* h[p] += alpha * sum_r Js[r][col0 + p]^2 for p < width (rows r = (sample, class)); the conv-layer
 * diagonal GGN / EF is the squared per-sample weight Jacobian summed over samples. */
int lk_sq_colsum_f32(const float* Js, int64_t rows, int64_t P, int64_t col0, int64_t width, float alpha,
                     float* h, void* stream);

/* Element-wise VJP of the seed-batched reverse sweep: all S seeds of an `activation(BatchNorm_eval(.))` backward
 * in one pass (the reference gets these from stock autograd, one backward kernel per seed and layer —
 * laplace/curvature/curvlinops.py:87-106 through curvlinops' hooks):
 *   out[s][e] = (g[s][e] + g2[s][e]) * M[e] * scale[(e / HW) % C],   e < per_sample = B*C*HW
 * g2: second branch of a residual connection, summed on the fly (NULL = none; may not alias out).
 * M: per-sample multiplier (NULL = 1): bytes that are zero / non-zero (a ReLU mask, m_is_float = 0) or floats
 * (f'(y), m_is_float = 1).  scale: per-channel factor gamma/sqrt(var+eps) (NULL = 1; then C, HW are ignored). */
/* Forward counterpart in the sweep's own interpretation of the model: eval-mode BatchNorm (a per-channel affine map)
 * with an optional ReLU and the mask its VJP needs, in one pass:
 *   y[e] = act(x[e] * scale[c(e)] + shift[c(e)] + addend[e]),  mask[e] = y[e] > 0
 *   (addend: the other branch of a residual connection, NULL = none; mask may be NULL; relu = 0: no activation),
 *   scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale, e < total = B*C*HW. */
int lk_bn_act_fwd_f32(const float* x, const float* scale, const float* shift, const float* addend, int64_t total,
                      int64_t C, int64_t HW, int relu, float* y, unsigned char* mask, void* stream);
int lk_vjp_scale_mask_f32(const float* g, const float* g2, const void* m, int m_is_float, const float* scale, int64_t S,
                          int64_t per_sample, int64_t C, int64_t HW, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Dense last-layer GGN.  Replaces last_layer_jacobians + GGNInterface.full for a Linear head
 * (curvature.py:131-167,375-411) without materialising Js, using J_n = I_C (x) [phi_n, 1]:
 *   H[(j,a),(k,b)] += alpha * sum_n (delta_jk p_nj - p_nj p_nk) pt_na pt_nb      pt = [phi, 1]
 *                   = alpha * ( blockdiag_j Gram(sqrt(p_j s_j).Pt) - offdiag_jk Gram(Y) ),
 *                     s_nj = sum_{k != j} p_nk,  Y[n][(j,a)] = p_nj pt_na
 * No class-diagonal block is formed as a difference, so rows with p_j within an ulp of 0 or 1 keep their
 * digits and H stays positive semi-definite to rounding.
 * phi: [B][D]; probs: [B][C] softmax probabilities (NULL = regression, Lambda = I);
 * H: [P][P] in the reference's parameter order (weight [C][D] row-major, then bias [C]),
 * P = C*D (+C if has_bias).
 * ------------------------------------------------------------------------------------------- */
size_t lk_ll_ggn_workspace_bytes(int64_t B, int64_t C, int64_t D);
int lk_ll_ggn_full_f32(const float* phi, const float* probs, int64_t B, int64_t C, int64_t D, int has_bias,
                       float alpha, float* H, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Symmetric eigendecomposition (two-sided block-Jacobi, exact-fp32 MFMA tile updates).
 * Replaces utils.symeig -> torch.linalg.eigh(M, UPLO="U") as used by Kron.decompose
 * (laplace/utils/utils.py:193-228, laplace/utils/matrix.py:123-150):
 *   reads the UPPER triangle of A[n][n]; writes ascending eigenvalues w[n] clamped at >= 0 (when
 *   clamp != 0) and eigenvectors as the COLUMNS of Q[n][n] (row-major), NaNs zeroed.
 *   info (device int32[2]): info[0] = 0 converged / 1 sweeps ran out, or A is outside the supported range (below);
 *   info[1] = sweeps executed.
 * Supported magnitudes: every symmetric fp32 matrix whose spectrum fp32 can hold.  The solve runs on A * 2^-e (e = the
 *   binary exponent of max |a_ij|, exact) and scales the eigenvalues back, so its thresholds and its split-fp16 products
 *   see the same numbers at every scale: the accuracy relative to lambda_max that holds for an O(1) matrix holds for
 *   max |a_ij| from 2^-126 (the smallest normal float) up to max_i sum_j |a_ij| < 3e38 (the row sum bounds lambda_max);
 *   tests/test_gpu_eigensolver.py holds it to 5e-6 from 2^-100 to 2^100.  Outside of that -- a max row sum of 3e38 or
 *   more, or a non-zero matrix with only denormal entries -- the call sets info[0] = 1 and writes w = 0: it reports,
 *   it does not guess.  NaN and +-inf entries (|a_ij| > 3e38) are read as 0.  Eigenvalues below 2^-126 come out as
 *   denormals (absolute accuracy kept, relative accuracy lost).
 * A is not modified.  Fully asynchronous on `stream`.
 * ------------------------------------------------------------------------------------------- */
size_t lk_syevj_workspace_bytes(int64_t n);
int lk_syevj_f32(const float* A, int64_t n, float* w, float* Q, int clamp, int max_sweeps, int32_t* info,
                 void* ws, size_t ws_bytes, void* stream);

/* All factors of one Kron.decompose (laplace/utils/matrix.py:123-150 loops over them one by one) in one call.
 * Matrix i (arguments as lk_syevj_f32, given as HOST arrays of `count` entries; ws[i] >=
 * lk_syevj_workspace_bytes(n[i]), private to matrix i) runs on streams[i % nstreams], matrices sharing a stream in
 * index order (pass the largest first).  A host-side scheduler keeps every stream two sweeps ahead of the device,
 * reads each solve's `converged` flag back asynchronously and finalises a matrix as soon as it has converged, so
 * no stream starves behind another one's launch queue and no empty sweeps are enqueued.
 * EXCEPTION to the no-host-synchronisation rule: the call returns when the last sweep of every matrix has
 * executed (the refinement / sort / gather of the last matrices may still be in flight on their streams). */
int lk_syevj_batched_f32(int64_t count, const float* const* A, const int64_t* n, float* const* w, float* const* Q,
                         int32_t* const* info, void* const* ws, const size_t* ws_bytes, int clamp, int max_sweeps,
                         void* const* streams, int64_t nstreams);

/* ---------------------------------------------------------------------------------------------
 * KronDecomposed.logdet (laplace/utils/matrix.py:381-404) for one two-factor block, with the
 * derivatives autograd needs for the marginal-likelihood sweep (baselaplace.py:466-485):
 *   out[0] += sum_ij log(l1_i l2_j + delta);  d_delta[0] += sum_ij 1/(l1_i l2_j + delta)
 *   d_l1[i] += sum_j l2_j/(.) ;  d_l2[j] += sum_i l1_i/(.)      (d_* may be NULL)
 * n2 == 0 means a single-factor block: sum_i log(l1_i + delta).
 * damping != 0 uses (l1+sqrt(delta)) (x) (l2+sqrt(delta)) (matrix.py:397-399; no derivatives).
 * delta is read from DEVICE memory (delta[0]).
 * ------------------------------------------------------------------------------------------- */
size_t lk_kron_logdet_workspace_bytes(int64_t n1);
int lk_kron_logdet_f32(const float* l1, int64_t n1, const float* l2, int64_t n2, const float* delta,
                       int damping, float* out, float* d_l1, float* d_l2, float* d_delta, void* ws,
                       size_t ws_bytes, void* stream);

/* The whole posterior precision in one pass: every block of a KronDecomposed (matrix.py:381-404 loops over the blocks;
 * the marginal-likelihood sweep, baselaplace.py:466-485 and marglik_training.py:303-314, calls it once per step):
 *   out[0]      += sum_b sum_ij log(s * l1[b]_i l2[b]_j + delta[b])      (n2[b] == 0: sum_i log(s * l1[b]_i + delta[b]))
 *   d_delta[b]  += sum_ij 1 / (.)                                         (may be NULL)
 *   d_scale[0]  += sum_b sum_ij l1[b]_i l2[b]_j / (.)                     (may be NULL)
 * s = scale[0] is the scalar H_factor = 1/(sigma^2 T) of `H * H_factor + delta` (baselaplace.py:1820), applied to the
 * eigenvalue PRODUCT (matrix.py:366-376 splits it as s^(1/2) per factor); scale == NULL means 1.
 * l1, n1, l2, n2 are HOST arrays of nblocks entries (device pointers / lengths); delta, scale, out, d_* are DEVICE
 * memory (delta has nblocks entries).  Three launches per 32 blocks, fixed-order fp64 reduction: deterministic. */
size_t lk_kron_logdet_blocks_workspace_bytes(int64_t total_rows /* sum_b n1[b] */, int64_t nblocks);
int lk_kron_logdet_blocks_f32(int64_t nblocks, const float* const* l1, const int64_t* n1, const float* const* l2,
                              const int64_t* n2, const float* delta, const float* scale, float* out, float* d_delta,
                              float* d_scale, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * GLM predictive variances  f_var[n] = J_n Sigma J_n^T  without materialising J (V1-V3).
 * ------------------------------------------------------------------------------------------- */
/* Kron posterior, one nn.Linear layer (KronDecomposed.inv_square_form, matrix.py:406-461, called from
 * KronLaplace.functional_variance, baselaplace.py:1834-1835).  u = g Q1 [Cc][B][Do], v = a Q2 [B][Di]
 * are the eigenbasis projections (plain GEMMs done by the caller);
 *   fvar[n][c][k] += sum_o u[c][n][o] u[k][n][o] * ( sum_i v[n][i]^2 / (l1_o l2_i + delta) )
 *                  + (bias block, if lb != NULL: ub = g Qb, sum_o ub[c][n][o] ub[k][n][o]/(lb_o + delta_b)) */
int lk_kron_quadform_linear_f32(const float* u, const float* v, const float* l1, const float* l2,
                                const float* delta, int64_t B, int64_t Cc, int64_t Do, int64_t Di,
                                const float* ub, const float* lb, const float* delta_b,
                                float* fvar, void* stream);

/* Diagonal posterior, one nn.Linear layer (DiagLaplace.functional_variance, baselaplace.py:2113-2115):
 *   fvar[n][c][k] += sum_{o,i} g[c][n][o] g[k][n][o] a[n][i]^2 var_w[o][i] + sum_o g[c][n][o] g[k][n][o] var_b[o] */
int lk_diag_quadform_linear_f32(const float* a, const float* g, const float* var_w, const float* var_b,
                                int64_t B, int64_t Cc, int64_t Do, int64_t Di, float* fvar, void* stream);

/* Weight-sharing layers (nn.Conv2d; nn.Linear applied along a sequence): the per-sample Jacobian of output c is
 * J_c = sum_l u[n][c][:][l] v[n][:][l]^T  (Do x Dk, L shared positions), and KronLaplace / DiagLaplace
 * .functional_variance (baselaplace.py:1834-1835 via matrix.py:406-461; baselaplace.py:2113-2115) contract the
 * materialised [B, C, Do*Dk] block.  These two never form it:
 *   fvar[n][c][k] += sum_{o,i} J_c[o,i] J_k[o,i] w[o,i]
 *   Kronecker posterior: u = Q1^T (grad w.r.t. the layer output), v = Q2^T (unfolded input), w = 1/(l1[o] l2[i] + delta[0])
 *   diagonal posterior:  u, v raw,                                                          w = var_w[o][i]
 * u [B][C][Do][L], v [B][Dk][L] (both position-contiguous: the NCHW layout of a convolution's output gradient and of
 * F.unfold), C <= 10 (LK_EINVAL beyond: use the generic Jacobian form).  Per sample one MFMA GEMM
 * [(C*Do) x L].[L x Dk] whose 32x32 tiles stay in accumulators for all C outputs and are folded into the C(C+1)/2 pair
 * sums in registers; workgroup partials are reduced in fixed order.  With L % 4 == 0 and 16-byte aligned u, v the
 * product runs on the bf16 matrix cores at fp32 accuracy (operands split into three bf16 pieces, six
 * v_mfma_f32_32x32x16_bf16 per fp32 product; dropped terms <= 3 * 2^-24), otherwise on v_mfma_f32_32x32x2_f32.
 * Requires C*L*Do < 2^29 and L*Dk < 2^29. */
size_t lk_quadform_shared_workspace_bytes(int64_t B, int64_t C, int64_t Do, int64_t Dk);
int lk_kron_quadform_shared_f32(const float* u, const float* v, const float* l1, const float* l2, const float* delta,
                                int64_t B, int64_t C, int64_t Do, int64_t Dk, int64_t L, float* fvar, void* ws,
                                size_t ws_bytes, void* stream);
/* lk_kron_quadform_shared_f32 for u stored seed-major, [C][B][Do][L]: what a seed-batched reverse sweep (and the rotation
 * convolution over its cotangent) leaves in memory — no transposed copy. */
int lk_kron_quadform_shared_seedmajor_f32(const float* u, const float* v, const float* l1, const float* l2, const float* delta,
                                          int64_t B, int64_t C, int64_t Do, int64_t Dk, int64_t L, float* fvar, void* ws,
                                          size_t ws_bytes, void* stream);
/* The same quadratic form on operands that ARRIVE split (round 5): u_h / u_l [C][B][Do][L] fp16 planes with the scale
 * u_sexp[0] (seed-major), v_h / v_l [B][Dk][L] with one scale per sample (v_nsexp = B) or one for the tensor (v_nsexp = 1),
 * as lk_conv_nhwc_f16x2_planes leaves them.  A chunk of 16 positions is then 8-byte copies into LDS, two 16-byte loads and
 * C x three v_mfma_f32_32x32x16_f16 — the fp32-operand forms above spend as many vector-pipe cycles splitting in flight as
 * their matrix pipe spends on the products; the operands are staged by LDS-DMA into a ring of four stages, requested three
 * chunks ahead (one wave per SIMD: nothing else hides a load).  L % 16 == 0, Do % 32 == 0, C <= 10; zero16: >= 16 zero bytes
 * on the device; same workspace. */
int lk_kron_quadform_shared_planes_f16x2(const void* u_h, const void* u_l, const int* u_sexp, const void* v_h, const void* v_l,
                                         const int* v_sexp, int64_t v_nsexp, const float* l1, const float* l2,
                                         const float* delta, int64_t B, int64_t C, int64_t Do, int64_t Dk, int64_t L,
                                         const void* zero16, float* fvar, void* ws, size_t ws_bytes, void* stream);
int lk_diag_quadform_shared_f32(const float* u, const float* v, const float* var_w, int64_t B, int64_t C, int64_t Do,
                                int64_t Dk, int64_t L, float* fvar, void* ws, size_t ws_bytes, void* stream);

/* Exact GGN / Fisher diagonal of a weight-sharing layer (GGNInterface.diag, laplace/curvature/curvature.py:413-433,
 * restricted to the layer's weight): h[o][i] += alpha * sum_{n,s} (sum_l u[n][s][o][l] v[n][i][l])^2 with
 * u [B][S][Do][L] the seed cotangents at the layer output and v [B][Dk][L] the unfolded input, S <= 10 seeds per call.
 * Same tile GEMM as lk_*_quadform_shared_f32; the squares are summed over (sample, seed) in registers, so the
 * [B, S, Do*Dk] per-sample Jacobian the as-written einsum contracts is never formed. */
size_t lk_diag_ggn_shared_workspace_bytes(int64_t B, int64_t Do, int64_t Dk);
int lk_diag_ggn_shared_f32(const float* u, const float* v, int64_t B, int64_t S, int64_t Do, int64_t Dk, int64_t L,
                           float alpha, float* h, void* ws, size_t ws_bytes, void* stream);

/* Generic streaming form over a materialised Jacobian (any layer type):
 *   fvar[n][c][k] = sum_p Js[n][c][p] var[p] Js[n][k][p] */
int lk_diag_quadform_js_f32(const float* Js, const float* var, int64_t B, int64_t C, int64_t P, float* fvar,
                            void* stream);

/* Last-layer Jacobians (CurvatureInterface.last_layer_jacobians, laplace/curvature/curvature.py:131-167, for a Linear head):
 *   Js[n][c][:] = e_c (x) [phi_n, 1]  — [B][C][P], P = C*D (+ C with a bias), parameter order weight [C][D] row-major then bias.
 * The fused consumers (lk_ll_ggn_full_f32, lk_dense_quadform_ll_f32) never form it; this is for callers of the drop-in seam that
 * ask for the Jacobian itself (la(x) of the reference's last-layer flavours). */
int lk_jac_last_layer_f32(const float* phi, int64_t B, int64_t C, int64_t D, int has_bias, float* Js, void* stream);

/* Dense last-layer posterior (FullLaplace.functional_variance with J = I (x) [phi,1],
 * baselaplace.py:1683-1684, lllaplace.py:212-237):
 *   fvar[n][c][k] = phit_n^T Sigma[(c,:),(k,:)] phit_n,   Sigma: [P][P] in the reference's parameter
 *   order (weight [C][D] row-major, then bias [C]). */
size_t lk_dense_quadform_ll_workspace_bytes(int64_t B, int64_t C, int64_t D);
int lk_dense_quadform_ll_f32(const float* phi, const float* Sigma, int64_t B, int64_t C, int64_t D, int has_bias,
                             float* fvar, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Prior-precision grid search (BaseLaplace.optimize_prior_precision(method="gridsearch"), baselaplace.py:487-561) in one
 * pass: only the diagonal of the output covariance, var [G][B][C] (+=), at all G prior precisions deltas[G].  Weight of
 * parameter (o, i) at grid point g, by `mode`:
 *   0  Kron           1 / (l1_o l2_i + delta_g)                 w0 = l1 [Do], w1 = l2 [Di / Dk]
 *   1  damped Kron    1 / ((l1_o + sqrt delta_g)(l2_i + sqrt delta_g))   (matrix.py:397-399, 441-444)
 *   2  diagonal       1 / (h_oi + delta_g)                        w0 = h [Do][Di / Dk] (prior-free precision), w1 unused
 * Every sum runs in a fixed order (no float atomics): repeated calls give the same bits.
 * ------------------------------------------------------------------------------------------- */
/* nn.Linear layer: var[g][n][c] += sum_o u[c][n][o]^2 sum_i v[n][i]^2 W_g(o,i)  (+ sum_o ub[c][n][o]^2 / (wb_o + delta_g) if
 * ub != NULL).  u [C][B][Do], v [B][Di] as for lk_kron_quadform_linear_f32 (eigenbasis projections; raw gradients /
 * activations for mode 2). */
int lk_quadform_linear_grid_f32(const float* u, const float* v, const float* w0, const float* w1, const float* deltas,
                                int64_t G, int mode, int64_t B, int64_t C, int64_t Do, int64_t Di, const float* ub,
                                const float* wb, float* var, void* stream);
/* Weight-sharing layer: var[g][n][c] += sum_{o,i} (sum_l u[n][c][o][l] v[n][i][l])^2 W_g(o,i).  u [B][C][Do][L] (seed_major:
 * [C][B][Do][L]), v [B][Dk][L]; any C.  The tile products of lk_kron_quadform_shared_f32 (fp32 accuracy) are formed once;
 * only the weighted reduction runs per grid point. */
size_t lk_quadform_shared_grid_workspace_bytes(int64_t B, int64_t C, int64_t Do, int64_t Dk, int64_t G);
int lk_quadform_shared_grid_f32(const float* u, const float* v, const float* w0, const float* w1, const float* deltas,
                                int64_t G, int mode, int64_t B, int64_t C, int64_t Do, int64_t Dk, int64_t L,
                                int seed_major, float* var, void* ws, size_t ws_bytes, void* stream);
/* Which instantiation of the weight-sharing kernels a shape launches (pure host function, no device call: the launchers
 * above decide with the same helpers).  `form`: LK_QF_*; `C`: outputs (seeds S for LK_QF_DIAG_GGN); `aligned16`: u and v
 * are 16-byte aligned (ignored by LK_QF_PLANES, which requires it; for LK_QF_GRID the answer is that of one block of
 * outputs — every block launches the same CT, the alignment is that of the block's first output).  Returns
 *   CT | flags << 4 | split << 8      CT: outputs held in accumulators, split: workgroups per sample (LK_QF_DIAG_GGN: nsplit,
 *                                     workgroups per tile)
 *   flags, LK_QF_PLANES: 1 = two workgroups per CU (OCC = 2), 2 = SUB (one-chunk tiles), 4 = eigenvalues in LDS
 *   flags, other forms:  1 = ARITH 1 (three-piece bf16 products; 0: v_mfma_f32_32x32x2_f32)
 * or a negative value for a shape the form does not serve (B, C, Do, Dk or L < 1, more than 10 outputs outside LK_QF_GRID,
 * LK_QF_PLANES with L % 16 or Do % 32, an unknown form). */
#define LK_QF_KRON 0           /* lk_kron_quadform_shared_f32 */
#define LK_QF_KRON_SEEDMAJOR 1 /* lk_kron_quadform_shared_seedmajor_f32 */
#define LK_QF_DIAG 2           /* lk_diag_quadform_shared_f32 */
#define LK_QF_PLANES 3         /* lk_kron_quadform_shared_planes_f16x2 */
#define LK_QF_DIAG_GGN 4       /* lk_diag_ggn_shared_f32 */
#define LK_QF_GRID 5           /* lk_quadform_shared_grid_f32, all three modes, either layout of u */
int lk_quadform_shared_variant(int form, int64_t B, int64_t C, int64_t Do, int64_t Dk, int64_t L, int aligned16);
/* Which kernel, tile, epilogue and grid a launch of the split-fp16 convolution takes (pure host function except for the
 * device's CU count, 256 without a device: conv_dispatch and the launchers decide with the same helpers of csrc/lk_conv.hip).
 * `entry`: LK_CONV_*; the arguments are those of the entry point (the three dense entry points ignore Hc, Wc, out_step, oh0, ow0,
 * LK_CONV_VJP also in_mul); `have_wc`: chunk-major weights are handed over (lk_conv_nhwc_f16x2_vjp_wc); `mask_is_float`: the
 * multiplier is fp32.  Fills out[16]:
 *   [0] kernel: 0 generic (conv_f16x2_kernel), 1 / 2 persistent window form on 256 / 512 pixels, 3 strided
 *   [1] BM  [2] BN  [3] epilogue: 0 plain, 1 split planes, 2 VJP, 3 forward (BatchNorm / add / ReLU)
 *   [4] position-major rows  [5] dense grid  [6] workgroups  [7] pixel tiles nb_m  [8] column tiles nb_n
 *   [9] co-located columns  [10] split_S (1: no split tail)  [11] split_L  [12] workgroups per CU (window form)
 *   [13] tiles walked  [14] position-contiguous output  [15] residue classes (strided form)
 * and returns 0, or a negative value for a shape the entry point refuses or launches nothing for. */
#define LK_CONV_PLAIN 0  /* lk_conv_nhwc_f16x2 */
#define LK_CONV_PLANES 1 /* lk_conv_nhwc_f16x2_planes */
#define LK_CONV_BN_ACT 2 /* lk_conv_bn_act_nhwc_f16x2 */
#define LK_CONV_VJP 3    /* lk_conv_nhwc_f16x2_vjp, lk_conv_nhwc_f16x2_vjp_wc */
int lk_conv_launch_variant(int entry, int64_t N, int64_t Hi, int64_t Wi, int64_t Ci, int64_t Co, int64_t Hc, int64_t Wc,
                           int64_t in_mul, int64_t Ho, int64_t Wo, int64_t out_step, int64_t oh0, int64_t ow0, int64_t T,
                           const int* taps, int64_t in_nsexp, int have_wc, int mask_is_float, int config, int* out);
/* the same for lk_conv_nhwc_f16x2_vjp_strided (`taps`: T x 6 ints as there) */
int lk_conv_strided_launch_variant(int64_t N, int64_t Hi, int64_t Wi, int64_t Ci, int64_t Co, int64_t Ho, int64_t Wo, int64_t os,
                                   int64_t T, const int* taps, int two_sources, int* out);
/* Probit link + NLL: loss_sum[g] += sum_n -log(max(softmax(kappa f_mu[n])[labels[n]], 1e-30)),
 * kappa_c = 1 / sqrt(1 + pi/8 var[g][n][c]) (baselaplace.py:649-651); f_mu [B][C], labels int64 [B], loss_sum double [G]. */
int lk_probit_nll_grid_f32(const float* f_mu, const float* var, const int64_t* labels, int64_t G, int64_t B, int64_t C,
                           double* loss_sum, void* stream);

/* ---- the fit's one collective (replaces nothing in the reference, which has no multi-GPU fit: the loop of
 * laplace/baselaplace.py:969-985 sharded over ranks needs ONE sum of the accumulated factors at epoch end) -------------------
 * Thin wrappers over RCCL (ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy / ncclAllReduce(ncclFloat, ncclSum, in place)),
 * bound by dlopen at the first call, for hosts that are not PyTorch; the Python host of this repository uses
 * torch.distributed's "nccl" backend (the same RCCL) and the packed upper-triangle buffer of `KronAccumulator.tensors()`.
 * `id128`: 128 bytes (ncclUniqueId) made on rank 0 and handed to the other ranks by the host's own means. */
int lk_comm_unique_id(void* id128);
int lk_comm_init_rank(void** comm, int nranks, const void* id128, int rank);
int lk_comm_destroy(void* comm);
int lk_allreduce_sum_f32(void* comm, float* buf, int64_t count, void* stream);

/* ---- dense Laplace in the eigenbasis of the curvature (csrc/lk_spectral.hip) ----------------------------------------------------
 * H = Q diag(lam) Q^T once (lk_syevj_f32); for a SCALAR prior precision delta the posterior precision is Q diag(mu) Q^T with
 * mu_j = hfac lam_j + delta, and with R = J Q (which does not depend on delta)
 *   COV   fvar[n][c][k]  = sum_j R[n][c][j] R[n][k][j] / (hfac lam_j + delta)     (FullLaplace.functional_variance,
 *                                                                                  laplace/baselaplace.py:1683-1684, without the
 *                                                                                  Cholesky + inverse per prior of utils.py:118-129)
 *   GRID  var[g][n][c]  += sum_j R[n][c][j]^2 / (hfac lam_j + deltas[g])          (the diagonal at G priors in one pass: the grid
 *                                                                                  search of baselaplace.py:487-561; the caller zeroes var)
 * lk_spectral_quadform_ll_f32 / lk_spectral_grid_ll_f32: last layer, J = I (x) [phi, 1]: R[n][c][j] = sum_d phi[n][d] Q[c D + d][j]
 *   (+ Q[C D + c][j] with a bias) is formed per tile on the exact-fp32 matrix instruction and never stored; phi [B][D], Q [P][P]
 *   row-major with the eigenvectors in its columns, rows in the reference's parameter order (weight [C][D], then bias),
 *   P = C D (+ C); lam [P]; delta / deltas on the device; fvar [B][C][C], var [G][B][C].
 * lk_spectral_quadform_f32 / lk_spectral_grid_f32: R [N][C][P] is given (Js Q by one lk_gemm_f32).
 * Tiles of LK_SP_TILE_N samples x LK_SP_TILE_J eigen-columns; a workgroup owns a sample tile and a contiguous range of column
 * tiles, the ranges' partial sums go to the workspace and are added in ascending order: one owner per output element, no float
 * atomics, fixed order, repeated calls give the same bits; fvar is written in both triangles from one value.  COV holds up to 10
 * outputs (1, 2, 5 or 10 accumulators); more run in pairs of blocks of 5.  GRID serves any C in blocks of 1, 2, 5 or 10 outputs
 * and walks the grid in chunks of 64 / CT (5 for ten outputs) points, 128 points per launch.  Pointers need no alignment.
 * Contract: pointers non-null; 0 <= B, N < 2^24; 1 <= C < 2^15; 1 <= G < 2^20; LL: 1 <= D <= 896 and P <= 32768; R: 1 <= P <=
 *   32768; hfac positive and finite; the output overlaps neither an input nor the workspace; ws_bytes >=
 *   lk_spectral_workspace_bytes (else LK_EWORKSPACE).  B, N == 0 returns LK_OK before any device call.
 * `form`: LK_SP_* (| LK_SP_BIAS for the LL forms with a bias row); D_or_P: D for the LL forms, P for the others; G is ignored
 * by the COV forms (pass 1).
 * lk_spectral_variant (host only; `aligned` is ignored, every form reads single dwords) returns
 *   CT | grid << 4 | pairs << 5 | LL << 6 | (split > 1) << 7 | split << 8 | GC << 20
 *   CT: outputs held in accumulators; grid: the GRID epilogue; pairs: COV in pairs of blocks of 5 (C > 10); LL: the last-layer
 *   loader; split: workgroups per sample tile (column ranges); GC: grid points per epilogue chunk
 * or a negative value for a shape the entry points refuse. */
#define LK_SP_TILE_N 32
#define LK_SP_TILE_J 128
#define LK_SP_QUAD_LL 0 /* lk_spectral_quadform_ll_f32 */
#define LK_SP_GRID_LL 1 /* lk_spectral_grid_ll_f32 */
#define LK_SP_QUAD_R 2  /* lk_spectral_quadform_f32 */
#define LK_SP_GRID_R 3  /* lk_spectral_grid_f32 */
#define LK_SP_BIAS 4
size_t lk_spectral_workspace_bytes(int form, int64_t N, int64_t C, int64_t D_or_P, int64_t G);
int lk_spectral_quadform_ll_f32(const float* phi, const float* Q, const float* lam, float hfac, const float* delta, int64_t B,
                                int64_t C, int64_t D, int has_bias, float* fvar, void* ws, size_t ws_bytes, void* stream);
int lk_spectral_grid_ll_f32(const float* phi, const float* Q, const float* lam, float hfac, const float* deltas, int64_t G,
                            int64_t B, int64_t C, int64_t D, int has_bias, float* var, void* ws, size_t ws_bytes, void* stream);
int lk_spectral_quadform_f32(const float* R, const float* lam, float hfac, const float* delta, int64_t N, int64_t C, int64_t P,
                             float* fvar, void* ws, size_t ws_bytes, void* stream);
int lk_spectral_grid_f32(const float* R, const float* lam, float hfac, const float* deltas, int64_t G, int64_t N, int64_t C,
                         int64_t P, float* var, void* ws, size_t ws_bytes, void* stream);
int lk_spectral_variant(int form, int64_t N, int64_t C, int64_t D_or_P, int64_t G, int aligned);

#ifdef __cplusplus
}
#endif
#endif /* LAPLACE_HIP_H */
