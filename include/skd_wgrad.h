/*
 * skd_wgrad.h -- entry points of the WEIGHT GRADIENT of the training student's 3x3 convolutions on the split core
 * (csrc/conv3x3_wgrad.hip): the third product of the convolutions whose forward and data gradient are skd_conv3x3_split_nhwc
 * (skd_eval.h, skd_train.h).  Like the entries of skd_eval.h, skd_eval_ms.h, skd_ohem.h, skd_infer.h and skd_train.h they are
 * outside the frozen core ABI (skd.h): the plain-C oracle implements the core ABI only, so a back-end may lack them (the weight
 * gradients then come from the library, as before).  Same conventions as skd.h: int return, 1 = success, 0 = refused with
 * nothing launched; raw DEVICE pointers; outputs pre-sized by the caller; asynchronous on `stream`.
 */
#ifndef SKD_WGRAD_H_
#define SKD_WGRAD_H_

#include "skd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * 1 when the weight gradient of a (Cout, Cin, 3, 3) convolution fits the core: stride 1, padding == dilation >= 1, groups 1,
 * Cin and Cout multiples of 128 (each is the row count of one operand's tile).
 * ---------------------------------------------------------------------------------- */
int skd_conv3x3_split_wgrad_supported(int Cin, int Cout, int stride, int padding, int dilation, int groups);

/* ------------------------------------------------------------------------------------
 * The split-K geometry of one weight gradient: pure host arithmetic, no device call.  The reduction runs over the
 * P = B * H * W pixels in nk = ceil(P / 16) K-tiles, cut into slices that one workgroup each (per tap and 128 x 128 tile) sums.
 *   slices >= 1  that many, clamped to nk;
 *   slices == 0  the shipped choice for a device of `cus` compute units (0: 256): with tiles = 9 * (Cin / 128) * (Cout / 128)
 *                and slots = 2 * cus, the count S in 1 .. max(1, 2 * slots / tiles) that minimises
 *                ceil(tiles * S / slots) * ceil(nk / S) -- rounds of the device times the length of a slice -- the smaller
 *                count on a tie.
 * Either way the count is then made an exact cover: T = ceil(nk / slices) K-tiles per slice and ceil(nk / T) slices, so no
 * slice is empty.
 *   plan[0] = slices used, plan[1] = K-tiles per slice, plan[2] = workspace bytes = slices * 9 * Cin * Cout * 4.
 * Refused: plan NULL, a size < 1, slices < 0, cus < 0, channel counts the predicate refuses, P >= 2^30.
 * ---------------------------------------------------------------------------------- */
int skd_conv3x3_split_wgrad_plan(int B, int H, int W, int Cin, int Cout, int slices, int cus, int64_t *plan);

/* ------------------------------------------------------------------------------------
 * dw[n][c][ty][tx] = sum over the pixels m = (b, y, x) of g[m][n] * x[b, y + (ty - 1) d, x + (tx - 1) d, c] (0 outside the
 * image) for channels-last x (B, H, W, Cin) and g (B, H, W, Cout), d = dilation: the weight gradient of the same-size
 * convolution.  Two launches on `stream`: the partial sums of every slice into workspace[slice][n][tap][c] (every element
 * written: the workspace need not be initialised), then their sum in slice order -- the same bits on every call -- written to
 * dw through its four strides in elements (sn, sc, sy, sx: contiguous, channels-last, or a channel slice of a wider weight).
 * `slices` is plan[0] of skd_conv3x3_split_wgrad_plan for these sizes (the launch never chooses: geometry is decided in one
 * place), workspace_bytes at least its plan[2].
 * Refused: a NULL pointer; x, g or the workspace not 16-byte aligned; a short workspace; a negative stride; slices < 1 or
 * > nk or not a count the plan returns; dilation < 1; a size < 1; channel counts the predicate refuses.
 * ---------------------------------------------------------------------------------- */
int skd_conv3x3_split_wgrad_nhwc(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const float *g, float *dw,
                                 int64_t sn, int64_t sc, int64_t sy, int64_t sx, void *workspace, int64_t workspace_bytes,
                                 int slices, skd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SKD_WGRAD_H_ */
