/*
 * skd_infer2h.h -- the student's fused inference form on TWO FP16 PIECES per operand with a scaled residual (three products
 * instead of six): the residual-epilogue, 64-column and stride-2 forms of csrc/conv3x3.hip with PIECES = 2 and the piece format
 * kFp16 of csrc/conv_split_dev.hpp -- the three forms skd_split2h.h left without an fp16 twin.  Every entry is the twin of a
 * three-piece entry, argument for argument and host refusal for host refusal; only the piece format, and with it the weight
 * image, differs.  Opt-in and off by default (networks.pspnet_combine.fuse_for_inference(model, piece_format="fp16")).  Like
 * every extension entry these are outside the frozen core ABI (skd.h): the plain-C oracle implements the core ABI only, so a
 * back-end may lack them (the student then stays on three bf16 pieces).  Conventions of skd.h: int return, 1 = success, 0 =
 * refused with nothing launched; raw DEVICE pointers; NULL = optional tensor absent; outputs pre-sized by the caller;
 * asynchronous on `stream`.
 *
 * Numerics: those of skd_split2h.h, which states them in full and whose model is tests/split2h_ref.py.  In short: every fp32
 * operand a is cut into a0 = fp16(a), a1 = fp16((a - a0) * 2^11); lo += a0 b1, lo += a1 b0, hi += a0 b0 per 16 k, out =
 * fma(lo, 2^-11, hi) in front of the epilogue.  EXACT where one operand has at most 11 significant bits and the other at most
 * 22; two pieces on both sides give the three-product model bit for bit (the exact product less a1 b1).  LOUD: a finite
 * |a| > 65504 makes every output that reads it non-finite, never a finite wrong value.  An fp16 piece below 2^-14 is a
 * subnormal and is used as it is.  The residual of the epilogue is never split: it is added in fp32 behind the BatchNorm
 * expression, as in skd_infer.h.
 *
 * Launch geometry -- grid, tile heights, tile order, LDS and register budget per residency -- is that of the three-piece twin.
 */
#ifndef SKD_INFER2H_H_
#define SKD_INFER2H_H_

#include "skd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * skd_conv3x3_split_res_nhwc (skd_infer.h: formula, layouts, `geometry` 0 .. 3) on the fp16 two-piece core:
 *   out = act( ABN_eval(conv3x3(x) + conv_bias) + residual )
 * wpack is the image of skd_conv3x3_split2h_pack_weights (skd_split2h.h).  The result equals act(z + residual) of the fp32 z that
 * skd_conv3x3_split2h_nhwc writes with activation none.  residual NULL: skd_conv3x3_split2h_nhwc itself, bit for bit.  A residual
 * that overlaps `out` is refused.  The other refusals are those of skd_conv3x3_split2h_nhwc.
 * Rows at or beyond B * H * W neither read `residual` nor write `out`.
 * ---------------------------------------------------------------------------------- */
int skd_conv3x3_split2h_res_nhwc(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const void *wpack, float *out,
                                 const float *residual, const float *conv_bias, const float *mean, const float *var,
                                 const float *weight, const float *bias, float eps, int activation, float slope, int geometry,
                                 skd_stream_t stream);

/* ------------------------------------------------------------------------------------
 * The two-plane fp16 weight image of the 64-column form: the layout of skd_conv3x3_narrow_pack_pair's forward image (skd_narrow.h:
 * per column tile of 64 output channels and K-tile of 16 k, chunk(h, row) = h * 64 + (row ^ 4 h)) holding the two planes (b0, b1
 * scaled) instead of three bf16 planes: 256 chunks of 16 bytes per tile, 4 bytes per weight.
 * pack_bytes = 4 * Cout * Cin * 9, or 0 where skd_conv3x3_narrow_supported refuses the channel counts.
 * pack_weights: the forward image alone, with the parameter list and refusals of skd_conv3x3_split2h_pack_weights (w or pack
 * NULL, a negative stride, a pack shorter than pack_bytes or not 16-byte aligned, unsupported channel counts).
 * ---------------------------------------------------------------------------------- */
int64_t skd_conv3x3_narrow2h_pack_bytes(int Cin, int Cout);
int skd_conv3x3_narrow2h_pack_weights(int Cin, int Cout, const float *w, int64_t stride_n, int64_t stride_c, int64_t stride_y,
                                      int64_t stride_x, void *pack, int64_t pack_bytes, skd_stream_t stream);

/* ------------------------------------------------------------------------------------
 * skd_conv3x3_narrow_nhwc (skd_narrow.h: formula, layouts, the residual pointer, `geometry` 0 / 1) on the fp16 two-piece core;
 * wpack is the image of skd_conv3x3_narrow2h_pack_weights.  At a Cout that is a multiple of 128 it gives the bits of
 * skd_conv3x3_split2h_nhwc / skd_conv3x3_split2h_res_nhwc.  The refusals are those of skd_conv3x3_narrow_nhwc.
 * ---------------------------------------------------------------------------------- */
int skd_conv3x3_narrow2h_nhwc(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const void *wpack, float *out,
                              const float *residual, const float *conv_bias, const float *mean, const float *var,
                              const float *weight, const float *bias, float eps, int activation, float slope, int geometry,
                              skd_stream_t stream);

/* ------------------------------------------------------------------------------------
 * skd_conv3x3_split_s2_nhwc (skd_stride2.h: the row map, layouts, `geometry`, SKD_ACT_NONE / _RELU only) on the fp16 two-piece
 * core, without its `pieces` argument: wpack is the image of skd_conv3x3_split2h_pack_weights, which does not depend on the
 * stride.  The result is bit for bit skd_conv3x3_split2h_nhwc's output at the even pixels.  The predicate is
 * skd_conv3x3_split_s2_supported; the refusals are those of skd_conv3x3_split_s2_nhwc.
 * ---------------------------------------------------------------------------------- */
int skd_conv3x3_split2h_s2_nhwc(int B, int H, int W, int Cin, int Cout, const float *x, const void *wpack, float *out,
                                const float *conv_bias, const float *mean, const float *var, const float *weight, const float *bias,
                                float eps, int activation, float slope, int geometry, skd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SKD_INFER2H_H_ */
