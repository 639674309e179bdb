/*
 * skd_infer.h -- entry points of the student's fused inference path (csrc/conv3x3.hip): the split-core 3x3 convolution with a
 * residual in its epilogue, the second convolution of a BasicBlock.  Like the entries of skd_eval.h, skd_eval_ms.h and
 * skd_ohem.h they are outside the frozen core ABI (skd.h): the plain-C oracle implements the core ABI only, so a back-end may
 * lack them (the BasicBlocks then run the op sequence they ran before).  Same conventions as skd.h: int return, 1 = success,
 * 0 = failure; raw DEVICE pointers; NULL = optional tensor absent; outputs pre-sized by the caller; asynchronous on `stream`.
 */
#ifndef SKD_INFER_H_
#define SKD_INFER_H_

#include "skd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * skd_conv3x3_split_nhwc (skd_eval.h) with a residual behind the normalisation:
 *   out = act( ABN_eval(conv3x3(x) + conv_bias) + residual )
 * = relu(bn2(conv2(.)) + residual) of a BasicBlock in one launch.  Every argument but `residual` is that of
 * skd_conv3x3_split_nhwc: the same preconditions (skd_conv3x3_split_supported), the same packed weights
 * (skd_conv3x3_split_pack_weights), the same geometry rules (0 = the shipped choice, 1-3 forced) and the same result for
 * every geometry.
 *   residual (B, H, W, Cout) channels-last fp32, the output's shape: read once, at the output's offsets; added in fp32 to the
 *   rounded value of the BN expression, so the result equals act(z + residual) of the fp32 z that skd_conv3x3_split_nhwc
 *   writes with activation none.  It may not overlap `out` (refused: returns 0).
 *   residual NULL: skd_conv3x3_split_nhwc itself, bit for bit.
 * Rows at or beyond B * H * W neither read `residual` nor write `out`.
 * ---------------------------------------------------------------------------------- */
int skd_conv3x3_split_res_nhwc(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const void *wpack, float *out,
                               const float *residual, const float *conv_bias, const float *mean, const float *var,
                               const float *weight, const float *bias, float eps, int activation, float slope, int geometry,
                               skd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SKD_INFER_H_ */
