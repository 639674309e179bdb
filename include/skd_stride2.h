/*
 * skd_stride2.h -- entry points of the stride-2 forward form of the split-core 3x3 convolution (csrc/conv3x3.hip with
 * STRIDE = 2): the frozen teacher's layer2.0 conv2 (128 -> 128, 129^2 -> 65^2) and the student's layer2.0 conv1 in its inference
 * form (64 -> 128).  The 128-column family only, padding 1, dilation 1, forward only: the stride-2 gradients stay with the
 * library.  Like the entries of skd_eval.h, skd_eval_ms.h, skd_ohem.h, skd_infer.h, skd_train.h, skd_wgrad.h, skd_narrow.h,
 * skd_narrow_wgrad.h, skd_shortcut.h, skd_split2.h and skd_bnstats.h they are outside the frozen core ABI (skd.h): the plain-C
 * oracle implements the core ABI only, so a back-end may lack them (those convolutions then run what they ran before).  Same
 * conventions as skd.h: int return, 1 = success, 0 = refused with nothing launched; raw DEVICE pointers unless stated; NULL =
 * optional tensor absent; outputs pre-sized by the caller; asynchronous on `stream`.
 *
 * The form differs from skd_conv3x3_split_nhwc in ONE thing, the row map: output row m = (b * Ho + oy) * Wo + ox,
 * Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, reads the 3 x 3 window centred on input pixel (2 oy, 2 ox).  Taps, K loop, product
 * order, packed weights and epilogue are the stride-1 kernel's, so the result is BIT FOR BIT the stride-1 output at the even
 * pixels: s2(x) == skd_conv3x3_split_nhwc(x)[:, ::2, ::2, :] (tests/test_conv3x3_stride2_gpu.py, no tolerance).
 */
#ifndef SKD_STRIDE2_H_
#define SKD_STRIDE2_H_

#include "skd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * 1 when the kernel takes a (Cout, Cin, 3, 3) convolution: Cin a multiple of 16, Cout a multiple of 128, stride 2, padding 1,
 * dilation 1, groups 1.
 * ---------------------------------------------------------------------------------- */
int skd_conv3x3_split_s2_supported(int Cin, int Cout, int stride, int padding, int dilation, int groups);

/* ------------------------------------------------------------------------------------
 * HOST ONLY, no device is touched: the kernel's row map (the one function the kernel calls) for output row m of an input of
 * H x W pixels per image.  *pixel: the flattened input pixel index of the row's centre tap, (b * H + 2 oy) * W + 2 ox; *mask:
 * bit 3 ty + tx set iff tap (ty, tx) lies inside the image, 0 <= 2 oy + ty - 1 < H and 0 <= 2 ox + tx - 1 < W (the centre,
 * bit 4, always does).  pixel and mask are HOST pointers.  m may be any row >= 0: the image index b = m / (Ho * Wo) is not bounded.
 * Refused: H or W < 1, H * W >= 2^31, m < 0, pixel or mask NULL.
 * ---------------------------------------------------------------------------------- */
int skd_conv3x3_split_s2_taps(int H, int W, int64_t m, int64_t *pixel, unsigned *mask);

/* ------------------------------------------------------------------------------------
 *   out = act( ABN_eval(conv3x3(x, stride 2, padding 1) + conv_bias) )
 * with the epilogue arguments and their meaning of skd_conv3x3_split_nhwc (skd_eval.h): x (B, H, W, Cin) and out
 * (B, Ho, Wo, Cout) channels-last fp32, every epilogue term optional.
 *   wpack     the image of skd_conv3x3_split_pack_weights (skd_eval.h) for pieces = 3, of skd_conv3x3_split2_pack_weights
 *             (skd_split2.h) for pieces = 2: the image does not depend on the stride.
 *   pieces    3 = the three-piece split (six products), 2 = the reduced-precision form of skd_split2.h (three products).
 *   activation  SKD_ACT_NONE or SKD_ACT_RELU (the two epilogues the networks use at stride 2).
 *   geometry  as skd_conv3x3_split_nhwc: 0 = the shipped choice, 1 / 3 = the tall forms, 2 = 64-row tiles; the choice is made
 *             on the OUTPUT's row count M = B * Ho * Wo.
 * Refused: channel counts the predicate refuses; a size < 1; x, wpack or out NULL; x or wpack not 16-byte aligned; mean without
 * var or var without mean; any other activation (SKD_ACT_LEAKY_RELU included); a geometry outside 0..3; H * W >= 2^31; pieces
 * not 2 or 3.
 * Rows at or beyond M write nothing; no byte outside x, wpack and the epilogue vectors is read.
 * ---------------------------------------------------------------------------------- */
int skd_conv3x3_split_s2_nhwc(int B, int H, int W, int Cin, int Cout, const float *x, const void *wpack, float *out,
                              const float *conv_bias, const float *mean, const float *var, const float *weight, const float *bias,
                              float eps, int activation, float slope, int pieces, int geometry, skd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SKD_STRIDE2_H_ */
