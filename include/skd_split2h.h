/*
 * skd_split2h.h -- the frozen network's split-core convolutions on TWO FP16 PIECES per operand with a SCALED RESIDUAL (three
 * products): a third numeric form beside the three bf16 pieces of skd_eval.h / skd.h and the two bf16 pieces of skd_split2.h.  It
 * covers exactly what skd_split2.h covers -- csrc/conv3x3.hip's 128-column forward family and csrc/conv1x1.hip's GEMM, with
 * PIECES = 2 and the piece format kFp16 of csrc/conv_split_dev.hpp -- entry for entry, with the same argument lists and the same
 * host-side refusals.  Opt-in and off by default (networks.pspnet_combine.set_teacher_pieces(model, 2, piece_format="fp16")).
 * Like every extension entry these are outside the frozen core ABI
 * (skd.h): the plain-C oracle implements the core ABI only, so a back-end may lack them (the teacher then stays on three bf16
 * pieces).  Conventions of skd.h: int return, 1 = success, 0 = refused with nothing launched; raw DEVICE pointers; NULL =
 * optional tensor absent; outputs pre-sized by the caller; asynchronous on `stream`.
 *
 * Numerics.  An fp16 piece carries 11 significant bits, two carry 22 -- within two bits of fp32, where two bf16 pieces carry 16.
 * fp16's exponent is narrow, though: the residual a - fp16(a), about 2^-11 |a|, would be an fp16 subnormal for every |a| < 0.125.
 * So the residual is multiplied by 2^11 (exact) before it is converted.  Every fp32 operand a (behind the prologue, where there is
 * one) and b is cut, round to nearest even (v_cvt_pk_f16_f32), into
 *     a0 = fp16(a),   a1 = fp16((a - a0) * 2^11)        likewise b0, b1;      a ~ a0 + 2^-11 a1,
 * the residual a - a0 being exact in fp32.  What a0 + 2^-11 a1 leaves of a (below 2^-22 |a|) is DROPPED.  Of the four products of
 * the pieces THREE are kept, in this order per 16 k of a 32 x 32 block, each one v_mfma_f32_32x32x16_f16 with fp32 accumulation:
 *     lo += a0 b1,   lo += a1 b0,   hi += a0 b0;        out = fma(lo, 2^-11, hi)
 * a1 b1 (2^-22 of the product) is dropped as well.  `lo` and `hi` are two fp32 accumulator sets in BOTH kernels (their scales
 * differ by 2^11, so the 1x1 kernel cannot share one set as its bf16 forms do); the one fma joins them in front of the epilogue's
 * BatchNorm, residual and activation terms, which are those of the other forms.  tests/split2h_ref.py is the model.
 * EXACT: the result equals the exact product bit for bit when every value of one operand has at most 11 significant bits (it is
 * one piece: its second piece is 0), every value of the other at most 22 (two pieces, nothing dropped), every value's first piece
 * is finite (|v| <= 65504) and no piece falls below fp16's range (see below), and all partial sums stay below 2^24 of their unit.
 * TWO PIECES ON BOTH SIDES: the result equals the three-product model bit for bit and differs from the exact product by a1 b1.
 * RANGE.  This is the loud contract skd_split2.h states for bf16 overflow (about 3.39e38), at a REACHABLE magnitude: a finite |a|
 * above 65504 (from 65520 on) rounds a0 to infinity and makes its residual the opposite infinity, so every output that reads it
 * is NaN -- never a finite wrong value, and not the +-inf or finite value an fp32 chain would have given.  A NaN input gives NaN
 * outputs.  A frozen ResNet's post-ReLU activations and weights are orders of magnitude below it; a caller who cannot say that
 * of its data stays on the bf16 forms.  At the other end an fp16 piece below 2^-14 is a SUBNORMAL and is used as it is: the fp16
 * MFMA does not flush its A / B operands (measured: tests/test_split2h_gpu.py pins it), so a0 keeps absolute resolution 2^-24 and
 * a1 resolution 2^-35; what lies below that is lost, an absolute error below 2^-36 |b| per product.
 *
 * Shapes: the predicates are those of the three-piece entries, skd_conv3x3_split_supported() (skd_eval.h) and
 * skd_conv1x1_abn_supported() (skd.h).  Launch geometry -- grid, tile heights, tile order -- is exactly the three-piece one
 * (skd_conv1x1_abn_geometry / _tile_of describe these launches too); the 1x1 kernel holds 64 accumulator registers more than its
 * bf16 twins and is compiled for two workgroups per CU instead of three.
 */
#ifndef SKD_SPLIT2H_H_
#define SKD_SPLIT2H_H_

#include "skd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * The two-plane fp16 weight image of a (Cout, Cin, 3, 3) weight: the layout of skd_conv3x3_split2_pack_weights' image (per column
 * tile of 128 output channels and K-tile of 16 k, 2 * 2 * 128 chunks of 16 bytes) holding the planes (b0, b1 scaled) -- 4 bytes
 * per weight: pack_bytes = 4 * Cout * Cin * 9, or 0 where skd_conv3x3_split_supported would refuse the channel counts.
 * pack_weights: the parameter list and the refusals of skd_conv3x3_split_pack_weights (w or pack NULL, a negative stride, a
 * pack shorter than pack_bytes or not 16-byte aligned, unsupported channel counts).
 * ---------------------------------------------------------------------------------- */
int64_t skd_conv3x3_split2h_pack_bytes(int Cin, int Cout);
int skd_conv3x3_split2h_pack_weights(int Cin, int Cout, const float *w, int64_t stride_n, int64_t stride_c, int64_t stride_y,
                                     int64_t stride_x, void *pack, int64_t pack_bytes, skd_stream_t stream);

/* ------------------------------------------------------------------------------------
 * skd_conv3x3_split_nhwc (skd_eval.h: formula, layouts, epilogue terms, `geometry`) on the fp16 two-piece core; wpack is the
 * image of skd_conv3x3_split2h_pack_weights.  Refused on the host, in front of any launch: x, wpack or out NULL, x or wpack not
 * 16-byte aligned, one of mean / var without the other, a size < 1, channel counts or a dilation the predicate refuses, an
 * activation outside SKD_ACT_NONE / _RELU / _LEAKY_RELU, a geometry outside 0 .. 3.
 * ---------------------------------------------------------------------------------- */
int skd_conv3x3_split2h_nhwc(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const void *wpack, float *out,
                             const float *conv_bias, const float *mean, const float *var, const float *weight, const float *bias,
                             float eps, int activation, float slope, int geometry, skd_stream_t stream);

/* ------------------------------------------------------------------------------------
 * skd_conv1x1_abn_nhwc / skd_conv1x1_abn_pro_nhwc (skd.h: formula, layouts, residual, prologue) on the fp16 two-piece core.  The
 * prologue's BatchNorm + ReLU is applied in fp32 first; its result is what is split.  Refused on the host, in front of any
 * launch: x, w, out, mean or var NULL (pro: ppack NULL or K > 512), x, w or ppack not 16-byte aligned, M, K or N < 1, K not a
 * multiple of 16 or N of 128, an unknown activation.
 * ---------------------------------------------------------------------------------- */
int skd_conv1x1_abn2h_nhwc(int64_t M, int K, int N, const float *x, const float *w, const float *residual, float *out,
                           const float *mean, const float *var, const float *weight, const float *bias, float eps,
                           int activation, float slope, skd_stream_t stream);
int skd_conv1x1_abn2h_pro_nhwc(int64_t M, int K, int N, const float *x, const float *w, const float *residual, float *out,
                               const float *mean, const float *var, const float *weight, const float *bias, float eps,
                               const float *ppack, int activation, float slope, skd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SKD_SPLIT2H_H_ */
