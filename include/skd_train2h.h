/*
 * skd_train2h.h -- the training student's wide 3x3 convolutions on TWO FP16 PIECES per operand with a scaled residual (three
 * products, include/skd_split2h.h) and a POWER-OF-TWO SCALE PER GRADIENT TENSOR, found on the device: the scale word
 * (csrc/scale_word.hip), the fp16 two-plane pack pair and the scaled data gradient (csrc/conv3x3.hip), the weight gradient
 * (csrc/conv3x3_wgrad.hip).  The forward is skd_conv3x3_split2h_nhwc (skd_split2h.h) without batch norm and with SKD_ACT_NONE; x
 * and the weights are NOT scaled, so the forward and the weight gradient keep that header's loud contract for them: |x| or |w|
 * above 65504 gives NaN.  A mode for training (networks.pspnet_combine.route_training_convs's ``piece_format``), opt-in and off by
 * default: fp32 in, fp32 out, fp32 accumulation, 22 significant bits per operand -- the three-piece accuracy at three products.
 * Like the entries of skd_train2.h they are outside the frozen core ABI (skd.h): the plain-C oracle implements the core ABI only,
 * so a back-end may lack them (the student then stays on three bf16 pieces).  Same conventions as skd.h: int return, 1 =
 * success, 0 = refused with nothing launched; raw DEVICE pointers; outputs pre-sized by the caller; asynchronous on `stream`.
 *
 * Numerics: pieces, products, join, range and subnormal behaviour are those of skd_split2h.h -- a0 = fp16(a),
 * a1 = fp16((a - a0) 2^11); lo += a0 b1, a1 b0; hi += a0 b0; out = fma(lo, 2^-11, hi).  New here is the SCALE WORD of a gradient
 * tensor g (gradients of mean-reduced losses lie far below fp16's range; an unscaled fp16 split loses them):
 *     word = max over all elements of (bits(g) & 0x7fffffff), as uint32
 * -- independent of the order of evaluation, so the same word on every run; an infinity or a NaN makes it >= 0x7f800000.  The
 * scale s(word):  s = 1 if word == 0 or word >= 0x7f800000 (a non-finite g stays loud and is never masked); otherwise
 *     e = (word >> 23) - 127 (an fp32-subnormal amax counts as e = -127),  k = clamp(14 - e, -126, 126),  s = 2^k,  1 / s = 2^-k,
 * both normal fp32, so every finite amax >= 2^-112 lands in [2^14, 2^15), below 65504.  The scaled operand g s is computed in
 * fp32 in the staging, in front of the split (exact); the product is unscaled by ONE multiplication by 1 / s behind the join and
 * in front of anything else in the epilogue (exact while nothing leaves fp32's normal range).
 * SCALE INVARIANCE: out(g 2^j) == 2^j out(g) bit for bit while nothing leaves fp32's normal range.
 * EXACT: skd_split2h.h's classes on g s -- one operand at most 11 significant bits, the other at most 22.
 * ERROR, per output element of either gradient product, b the unscaled operand:
 *     |out - exact| <= 2^-21 sum |a| |b| + 2^-49 amax(g) sum |b| + (the fp32 accumulation's own error)
 * the first term for 22-bit operands and the dropped a1 b1, the second for pieces of g s below fp16's subnormal resolution.
 *
 * Out of scope, on three pieces or the library as before: the 64-column forms, the 1x1 shortcut convolutions, the statistics
 * form, piece planes, stride 2; scaling x or the weights; per-row or per-channel scales.
 */
#ifndef SKD_TRAIN2H_H_
#define SKD_TRAIN2H_H_

#include "skd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * The scale word of a dense fp32 tensor of n elements, written to ONE device uint32: two launches (per-workgroup maxima into
 * `workspace`, a finishing workgroup), one where a single workgroup covers n; integer maxima only, no atomics, no host
 * synchronisation, capturable in a graph, the same word on every run.  g is read with 16-byte loads (a ragged tail with 4-byte
 * ones); nothing but the word and the workspace is written.  workspace_bytes(n): the bytes the call needs (0 for n < 1); the
 * workspace may be uninitialised.
 * Refused (returns 0, nothing launched): g, workspace or word NULL, n < 1, g not 16-byte aligned, workspace or word not 4-byte
 * aligned, a workspace shorter than the query's answer.
 * ---------------------------------------------------------------------------------- */
int64_t skd_fp16_scale_word_workspace_bytes(int64_t n);
int skd_fp16_scale_word(int64_t n, const float *g, void *workspace, int64_t workspace_bytes, uint32_t *word, skd_stream_t stream);

/* ------------------------------------------------------------------------------------
 * skd_conv3x3_split2_pack_pair (skd_train2.h: argument list, refusals) for the fp16 two-plane image: ONE launch writes
 *   pack_fwd  byte for byte what skd_conv3x3_split2h_pack_weights(Cin, Cout, w, ...) writes;
 *   pack_bwd  byte for byte what skd_conv3x3_split2h_pack_weights(Cout, Cin, Wd, ...) writes for the contiguous
 *             Wd[c][n][ty][tx] = w[n][c][2 - ty][2 - tx]  (Cin, Cout, 3, 3), never materialised.
 * Sizes: skd_conv3x3_split2h_pack_bytes(Cin, Cout) and (Cout, Cin).
 * ---------------------------------------------------------------------------------- */
int skd_conv3x3_split2h_pack_pair(int Cin, int Cout, const float *w, int64_t stride_n, int64_t stride_c, int64_t stride_y,
                                  int64_t stride_x, void *pack_fwd, int64_t fwd_bytes, void *pack_bwd, int64_t bwd_bytes,
                                  skd_stream_t stream);

/* ------------------------------------------------------------------------------------
 * The raw convolution skd_conv3x3_split2h_nhwc(..., no conv bias, no statistics, SKD_ACT_NONE, ...) whose activation operand is
 * scaled by s(*word) in front of the split and whose result is multiplied by 1 / s behind the join: with x = g and wpack =
 * pack_bwd, the data gradient.  Every workgroup reads the word once.  With a word whose scale is 1 the output equals that entry's
 * bit for bit.  Refused: what skd_conv3x3_split2h_nhwc refuses, and word NULL (the caller wants that entry then) or not 4-byte
 * aligned.
 * ---------------------------------------------------------------------------------- */
int skd_conv3x3_split2h_scaled_nhwc(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const void *wpack,
                                    float *out, const uint32_t *word, int geometry, skd_stream_t stream);

/* ------------------------------------------------------------------------------------
 * skd_conv3x3_split2_wgrad_plan (skd_train2.h), unchanged: tiles, workgroups per compute unit and workspace layout are those of
 * the bf16 forms, so the plan is the same arithmetic with the same refusals.
 * ---------------------------------------------------------------------------------- */
int skd_conv3x3_split2h_wgrad_plan(int B, int H, int W, int Cin, int Cout, int slices, int cus, int64_t *plan);

/* ------------------------------------------------------------------------------------
 * skd_conv3x3_split2_wgrad_nhwc (skd_train2.h: formula, layouts, strides of dw, workspace, refusals) on two fp16 pieces per
 * operand: g's rows are multiplied by s(*word) and both operands cut into two fp16 pieces in the staging, x's rows unscaled; the
 * slice's block is fma(lo, 2^-11, hi) (1 / s).  The slice sum is the three-piece entry's launch.  word NULL means scale 1; a word
 * that is not 4-byte aligned is refused.
 * ---------------------------------------------------------------------------------- */
int skd_conv3x3_split2h_wgrad_nhwc(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const float *g, float *dw,
                                   int64_t sn, int64_t sc, int64_t sy, int64_t sx, void *workspace, int64_t workspace_bytes,
                                   const uint32_t *word, int slices, skd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SKD_TRAIN2H_H_ */
