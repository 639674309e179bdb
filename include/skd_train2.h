/*
 * skd_train2.h -- the TWO-PIECE (three-product) forms of the training student's wide 3x3 convolutions on the split core: the
 * two-plane pack pair (csrc/conv3x3.hip) and the weight gradient with PIECES = 2 (csrc/conv3x3_wgrad.hip).  Forward and data
 * gradient are skd_conv3x3_split2_nhwc (skd_split2.h) in both directions, without batch norm and with SKD_ACT_NONE; the conv
 * bias goes in the epilogue.  A reduced-precision mode for training (networks.pspnet_combine.route_training_convs's ``pieces``),
 * opt-in and off by default: fp32 in, fp32 out, fp32 accumulation, 16 significant bits per operand.  bf16 pieces only -- they keep
 * fp32's exponent, so small gradients need no scaling; the fp16 form, which finds a power-of-two scale per gradient tensor on the
 * device and keeps 22 bits, is skd_train2h.h.  Like the entries of skd_train.h and skd_wgrad.h
 * they are outside the frozen core ABI (skd.h): the plain-C oracle implements the core ABI only, so a back-end may lack them (the
 * student then stays on three pieces).  Same conventions as skd.h: int return, 1 = success, 0 = refused with nothing launched;
 * raw DEVICE pointers; NULL = optional tensor absent; outputs pre-sized by the caller; asynchronous on `stream`.
 *
 * Numerics: those of skd_split2.h.  Each fp32 operand a is a0 + a1 + r with a0 = bf16(a), a1 = bf16(a - a0); r (|r| <= 2^-17 |a|)
 * is dropped, and of the four piece products a0 b1, a1 b0, a0 b0 are kept, a1 b1 (below 2^-16 |a b|) dropped.  So every output
 * element is within 2^-15 sum |a| |b| of the exact sum, beside the fp32 accumulation's own error.  EXACT on integer data when one
 * operand has at most 8 significant bits, the other at most 16 and all partial sums stay below 2^24; with 16-bit values on both
 * sides the result equals the three-product model (tests/split2_ref.py) bit for bit, not the exact product.
 *
 * Out of scope, on three pieces or the library as before: the 64-column forms (skd_narrow.h, skd_narrow_wgrad.h), the 1x1
 * shortcut convolutions (skd_shortcut.h), the statistics form (skd_bnstats.h), stride 2.
 */
#ifndef SKD_TRAIN2_H_
#define SKD_TRAIN2_H_

#include "skd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * skd_conv3x3_split_pack_pair (skd_train.h) for the two-plane image: ONE launch writes
 *   pack_fwd  byte for byte what skd_conv3x3_split2_pack_weights(Cin, Cout, w, ...) writes;
 *   pack_bwd  byte for byte what skd_conv3x3_split2_pack_weights(Cout, Cin, Wd, ...) writes for the contiguous
 *             Wd[c][n][ty][tx] = w[n][c][2 - ty][2 - tx]  (Cin, Cout, 3, 3), never materialised,
 * so that skd_conv3x3_split2_nhwc(B, H, W, Cout, Cin, dilation, g, pack_bwd, dx, NULL..., SKD_ACT_NONE, ...) is the data gradient.
 * Either pack pointer may be NULL: only the other image is written.  fwd_bytes / bwd_bytes: at least
 * skd_conv3x3_split2_pack_bytes(Cin, Cout) and skd_conv3x3_split2_pack_bytes(Cout, Cin).
 * Refused (returns 0, nothing launched): w NULL, both packs NULL, a pack that is not 16-byte aligned or too short, a negative
 * stride, channel counts the requested direction does not take.
 * ---------------------------------------------------------------------------------- */
int skd_conv3x3_split2_pack_pair(int Cin, int Cout, const float *w, int64_t stride_n, int64_t stride_c, int64_t stride_y,
                                 int64_t stride_x, void *pack_fwd, int64_t fwd_bytes, void *pack_bwd, int64_t bwd_bytes,
                                 skd_stream_t stream);

/* ------------------------------------------------------------------------------------
 * skd_conv3x3_split_wgrad_plan (skd_wgrad.h), unchanged: the two-piece kernel keeps the tiles, the workgroups per compute unit
 * and the workspace layout of the three-piece one, so the plan -- slices, K-tiles per slice, workspace bytes -- is the same
 * arithmetic with the same refusals.  The predicate is skd_conv3x3_split_wgrad_supported.
 * ---------------------------------------------------------------------------------- */
int skd_conv3x3_split2_wgrad_plan(int B, int H, int W, int Cin, int Cout, int slices, int cus, int64_t *plan);

/* ------------------------------------------------------------------------------------
 * skd_conv3x3_split_wgrad_nhwc (skd_wgrad.h: formula, layouts, strides of dw, workspace, refusals) with both operands cut into
 * two pieces in the staging and three products per K-tile: a0 b1 and a1 b0 into one fp32 accumulator set, a0 b0 into a second
 * one, added in the epilogue.  The slice sum is the three-piece entry's launch: the same bits on every call.
 * ---------------------------------------------------------------------------------- */
int skd_conv3x3_split2_wgrad_nhwc(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const float *g, float *dw,
                                  int64_t sn, int64_t sc, int64_t sy, int64_t sx, void *workspace, int64_t workspace_bytes,
                                  int slices, skd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SKD_TRAIN2_H_ */
