/*
 * skd_narrow.h -- entry points of the 64-column form of the split-core 3x3 convolution (csrc/conv3x3_narrow.hip): the
 * convolutions of skd_conv3x3_split_nhwc / skd_conv3x3_split_res_nhwc (skd_eval.h, skd_infer.h) for output channel counts that
 * are multiples of 64, not 128 -- the student's stem and layer1.  Like the entries of skd_eval.h, skd_eval_ms.h, skd_ohem.h,
 * skd_infer.h, skd_train.h and skd_wgrad.h they are outside the frozen core ABI (skd.h): the plain-C oracle implements the core
 * ABI only, so a back-end may lack them (those convolutions then run what they ran before).  Same conventions as skd.h: int
 * return, 1 = success, 0 = refused with nothing launched; raw DEVICE pointers; NULL = optional tensor absent; outputs pre-sized
 * by the caller; asynchronous on `stream`.
 */
#ifndef SKD_NARROW_H_
#define SKD_NARROW_H_

#include "skd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * 1 when the kernel takes a (Cout, Cin, 3, 3) convolution: Cin a multiple of 16, Cout a multiple of 64, stride 1,
 * padding == dilation >= 1, groups 1.  A multiple of 128 is a multiple of 64: such a convolution runs as twice as many column
 * tiles and gives the bits of skd_conv3x3_split_nhwc.
 * ---------------------------------------------------------------------------------- */
int skd_conv3x3_narrow_supported(int Cin, int Cout, int stride, int padding, int dilation, int groups);

/* ------------------------------------------------------------------------------------
 * Bytes of the weight image of a (Cout, Cin, 3, 3) weight: (Cout / 64) * (9 * Cin / 16) tiles of 384 chunks of 16 bytes -- per
 * column tile of 64 output channels and K-tile of 16 k (k = tap * Cin + c), three bf16 planes of 64 rows,
 * chunk(h, row) = h * 64 + (row ^ 4 h), h = k / 8.  6 bytes per weight; 0 for channel counts the predicate refuses.
 * ---------------------------------------------------------------------------------- */
int64_t skd_conv3x3_narrow_pack_bytes(int Cin, int Cout);

/* ------------------------------------------------------------------------------------
 * The three-piece split of the weight w (Cout, Cin, 3, 3), read through its strides in elements, written as two images by ONE
 * launch -- skd_conv3x3_split_pack_pair (skd_train.h) for 64-row tiles:
 *   pack_fwd  the image of w for skd_conv3x3_narrow_nhwc(B, H, W, Cin, Cout, ...): needs Cout % 64 == 0, Cin % 16 == 0;
 *   pack_bwd  the image of Wd[c][n][ty][tx] = w[n][c][2 - ty][2 - tx] (Cin, Cout, 3, 3), never materialised, for the data
 *             gradient skd_conv3x3_narrow_nhwc(B, H, W, Cout, Cin, ...): needs Cin % 64 == 0, Cout % 16 == 0.
 * Either pack pointer may be NULL: only the other image is written.  fwd_bytes / bwd_bytes: the sizes of the buffers, at least
 * skd_conv3x3_narrow_pack_bytes(Cin, Cout) and skd_conv3x3_narrow_pack_bytes(Cout, Cin).
 * Refused (returns 0, nothing launched): w NULL, both packs NULL, a pack that is not 16-byte aligned or too short, a negative
 * stride, channel counts the requested direction does not take.
 * ---------------------------------------------------------------------------------- */
int skd_conv3x3_narrow_pack_pair(int Cin, int Cout, const float *w, int64_t stride_n, int64_t stride_c, int64_t stride_y,
                                 int64_t stride_x, void *pack_fwd, int64_t fwd_bytes, void *pack_bwd, int64_t bwd_bytes,
                                 skd_stream_t stream);

/* ------------------------------------------------------------------------------------
 *   out = act( ABN_eval(conv3x3(x) + conv_bias) + residual )
 * with the argument list and the meaning of skd_conv3x3_split_res_nhwc (skd_infer.h): x (B, H, W, Cin) and out (B, H, W, Cout)
 * channels-last fp32, wpack the forward image of skd_conv3x3_narrow_pack_pair, every epilogue term optional, residual NULL or
 * the output's shape (it may not overlap `out`: refused).  Output tiles are 128 pixels x 64 channels.
 *   geometry  0 = the shipped choice, 1 = 128 x 64 tiles (the one form there is); anything else is refused.
 * Refused: channel counts the predicate refuses; a size < 1; x, wpack or out NULL; x or wpack not 16-byte aligned; mean without
 * var or var without mean; an activation that is not SKD_ACT_NONE / _RELU / _LEAKY_RELU; H * W >= 2^31.
 * Rows at or beyond B * H * W neither read `residual` nor write `out`.
 * ---------------------------------------------------------------------------------- */
int skd_conv3x3_narrow_nhwc(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const void *wpack, float *out,
                            const float *residual, const float *conv_bias, const float *mean, const float *var,
                            const float *weight, const float *bias, float eps, int activation, float slope, int geometry,
                            skd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SKD_NARROW_H_ */
