/*
 * skd_split2.h -- the TWO-PIECE (three-product) forms of the frozen network's split-core convolutions: csrc/conv3x3.hip's
 * 128-column forward family and csrc/conv1x1.hip's GEMM with PIECES = 2 of csrc/conv_split_dev.hpp.  A reduced-precision mode
 * for a frozen teacher (networks.pspnet_combine.set_teacher_pieces), opt-in and off by default.  Like the entries of skd_eval.h,
 * skd_eval_ms.h, skd_ohem.h, skd_infer.h, skd_train.h, skd_wgrad.h, skd_narrow.h, skd_narrow_wgrad.h and skd_shortcut.h they are
 * outside the frozen core ABI (skd.h): the plain-C oracle implements the core ABI only, so a back-end may lack them (the teacher
 * then stays on three pieces).  Same conventions as skd.h: int return, 1 = success, 0 = refused with nothing launched; raw
 * DEVICE pointers; NULL = optional tensor absent; outputs pre-sized by the caller; asynchronous on `stream`.
 *
 * Numerics.  Every fp32 operand a (behind the prologue, where there is one) is written as a0 + a1 + r with
 *     a0 = bf16(a),  a1 = bf16(a - a0)        round to nearest even; the residual a - a0 is exact in fp32,
 * and the second residual r = a - a0 - a1 (|r| <= 2^-17 |a|, the third piece of the three-piece core) is DROPPED.  Of the four
 * products of the pieces THREE are kept, in this order per 16 k of a 32 x 32 block:
 *     a0 b1,  a1 b0,  a0 b0        each one v_mfma_f32_32x32x16_bf16 with fp32 accumulation;
 * a1 b1 (below 2^-16 |a b|) is dropped as well.  The 3x3 entry sums a0 b1 and a1 b0 into one fp32 accumulator set and a0 b0
 * into a second one, added in the epilogue (the two-set rule of csrc/conv3x3.hip); the 1x1 entries use one set.  The result is
 * therefore that of a product of operands with 16 significant bits, less a1 b1: about 4e-6 of the output's largest magnitude
 * for one product on post-ReLU data, 13 x the fp32 chain and 600 x below plain bf16 (profiles/r25_split2_accuracy.md).  The
 * truncation is by design; tests/split2_ref.py is the model.
 * EXACT on integer data when every value of one operand has at most 8 significant bits (it is one piece: its a1 is 0, so
 * a1 b1 = 0), every value of the other at most 16 (two pieces, r = 0), and all partial sums stay below 2^24 in magnitude: the
 * result then equals the exact product bit for bit.  With two-piece values on both sides it equals the three-product model
 * bit for bit, not the exact product.
 * Outside the normal range the pieces behave as in the three-piece core: a finite |a| above the largest bf16 (about 3.39e38)
 * rounds a0 to infinity and an infinite a has an undefined residual, so the affected outputs are NaN where an fp32 chain would
 * have given +-inf or a finite value; a NaN input gives NaN outputs; pieces below the fp32 normal range may be flushed.
 *
 * Shapes: the predicates are those of the three-piece entries, skd_conv3x3_split_supported() (skd_eval.h) and
 * skd_conv1x1_abn_supported() (skd.h).  Launch geometry -- grid, tile heights, tile order -- is exactly the three-piece one
 * (skd_conv1x1_abn_geometry / _tile_of describe these launches too).
 */
#ifndef SKD_SPLIT2_H_
#define SKD_SPLIT2_H_

#include "skd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * The two-plane weight image of a (Cout, Cin, 3, 3) weight: per column tile of 128 output channels and K-tile of 16 k the
 * first two planes (a0, a1) of skd_conv3x3_split_pack_weights' image, 2 * 2 * 128 chunks of 16 bytes -- 4 bytes per weight:
 * pack_bytes = 4 * Cout * Cin * 9, or 0 where skd_conv3x3_split_supported would refuse the channel counts.
 * pack_weights: the parameter list and the refusals of skd_conv3x3_split_pack_weights (w or pack NULL, a negative stride, a
 * pack shorter than pack_bytes or not 16-byte aligned, unsupported channel counts).
 * ---------------------------------------------------------------------------------- */
int64_t skd_conv3x3_split2_pack_bytes(int Cin, int Cout);
int skd_conv3x3_split2_pack_weights(int Cin, int Cout, const float *w, int64_t stride_n, int64_t stride_c, int64_t stride_y,
                                    int64_t stride_x, void *pack, int64_t pack_bytes, skd_stream_t stream);

/* ------------------------------------------------------------------------------------
 * skd_conv3x3_split_nhwc (skd_eval.h: formula, layouts, epilogue terms, `geometry`) on the two-piece core; wpack is the image
 * of skd_conv3x3_split2_pack_weights.  Refused on the host, in front of any launch: x, wpack or out NULL, x or wpack not
 * 16-byte aligned, one of mean / var without the other, a size < 1, channel counts or a dilation the predicate refuses, an
 * activation outside SKD_ACT_NONE / _RELU / _LEAKY_RELU, a geometry outside 0 .. 3.
 * ---------------------------------------------------------------------------------- */
int skd_conv3x3_split2_nhwc(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const void *wpack, float *out,
                            const float *conv_bias, const float *mean, const float *var, const float *weight, const float *bias,
                            float eps, int activation, float slope, int geometry, skd_stream_t stream);

/* ------------------------------------------------------------------------------------
 * skd_conv1x1_abn_nhwc / skd_conv1x1_abn_pro_nhwc (skd.h: formula, layouts, residual, prologue) on the two-piece core.  The
 * prologue's BatchNorm + ReLU is applied in fp32 first; its result is what is split.  Refused on the host, in front of any
 * launch: x, w, out, mean or var NULL (pro: ppack NULL or K > 512), x, w or ppack not 16-byte aligned, M, K or N < 1, K not a
 * multiple of 16 or N of 128, an unknown activation.
 * ---------------------------------------------------------------------------------- */
int skd_conv1x1_abn2_nhwc(int64_t M, int K, int N, const float *x, const float *w, const float *residual, float *out,
                          const float *mean, const float *var, const float *weight, const float *bias, float eps,
                          int activation, float slope, skd_stream_t stream);
int skd_conv1x1_abn2_pro_nhwc(int64_t M, int K, int N, const float *x, const float *w, const float *residual, float *out,
                              const float *mean, const float *var, const float *weight, const float *bias, float eps,
                              const float *ppack, int activation, float slope, skd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SKD_SPLIT2_H_ */
