/*
 * skd_train.h -- entry points of the training student's 3x3 convolutions on the split core (csrc/conv3x3.hip): the per-step
 * weight split that writes the image of the forward convolution and the image of its data gradient in one launch.  The
 * convolutions themselves are skd_conv3x3_split_nhwc (skd_eval.h) in both directions.  Like the entries of skd_eval.h,
 * skd_eval_ms.h, skd_ohem.h and skd_infer.h they are outside the frozen core ABI (skd.h): the plain-C oracle implements the core
 * ABI only, so a back-end may lack them (the student's convolutions then run what they ran before).  Same conventions as skd.h:
 * int return, 1 = success, 0 = failure; raw DEVICE pointers; NULL = optional tensor absent; outputs pre-sized by the caller;
 * asynchronous on `stream`.
 */
#ifndef SKD_TRAIN_H_
#define SKD_TRAIN_H_

#include "skd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * 1 when BOTH directions of a (Cout, Cin, 3, 3) convolution fit the core: the conditions of skd_conv3x3_split_supported
 * (stride 1, padding == dilation >= 1, groups 1, Cout a multiple of 128) and Cin a multiple of 128 too -- each channel count is
 * the N of one direction and the K of the other.
 * ---------------------------------------------------------------------------------- */
int skd_conv3x3_split_train_supported(int Cin, int Cout, int stride, int padding, int dilation, int groups);

/* ------------------------------------------------------------------------------------
 * The three-piece split of the weight w (Cout, Cin, 3, 3), read through its strides in elements (contiguous, channels-last or
 * a channel slice of a wider weight), written as two images by ONE launch:
 *   pack_fwd  byte for byte what skd_conv3x3_split_pack_weights(Cin, Cout, w, ...) writes;
 *   pack_bwd  byte for byte what skd_conv3x3_split_pack_weights(Cout, Cin, Wd, ...) writes for the contiguous
 *             Wd[c][n][ty][tx] = w[n][c][2 - ty][2 - tx]  (Cin, Cout, 3, 3),
 * so that skd_conv3x3_split_nhwc(B, H, W, Cout, Cin, dilation, g, pack_bwd, dx, NULL..., SKD_ACT_NONE, ...) is the data
 * gradient dx (B, H, W, Cin) of the same-size convolution for the output gradient g (B, H, W, Cout).  Wd is never materialised.
 * Either pack pointer may be NULL: only the other image is written (its direction alone has to fit the core: the image's N a
 * multiple of 128, its K of 16).  fwd_bytes / bwd_bytes: the sizes of the buffers, at least
 * skd_conv3x3_split_pack_bytes(Cin, Cout) and skd_conv3x3_split_pack_bytes(Cout, Cin) (equal when both exist).
 * Refused (returns 0, nothing launched): w NULL, both packs NULL, a pack that is not 16-byte aligned or too short, a negative
 * stride, channel counts the requested direction does not take.
 * ---------------------------------------------------------------------------------- */
int skd_conv3x3_split_pack_pair(int Cin, int Cout, const float *w, int64_t stride_n, int64_t stride_c, int64_t stride_y,
                                int64_t stride_x, void *pack_fwd, int64_t fwd_bytes, void *pack_bwd, int64_t bwd_bytes,
                                skd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SKD_TRAIN_H_ */
