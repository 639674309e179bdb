/*
 * skd_narrow_wgrad.h -- entry points of the WEIGHT GRADIENT of the training student's 64-channel 3x3 convolutions on the split
 * core (csrc/conv3x3_wgrad.hip, the 128 x 64 tile form of its one kernel): the third product of the convolutions whose forward
 * and data gradient are skd_conv3x3_narrow_nhwc / skd_conv3x3_split_nhwc (skd_narrow.h, skd_train.h).  Like the entries of
 * skd_eval.h, skd_eval_ms.h, skd_ohem.h, skd_infer.h, skd_train.h, skd_wgrad.h and skd_narrow.h they are outside the frozen core
 * ABI (skd.h): the plain-C oracle implements the core ABI only, so a back-end may lack them (these weight gradients then come
 * from the library, as before).  Same conventions as skd.h: int return, 1 = success, 0 = refused with nothing launched; raw
 * DEVICE pointers; outputs pre-sized by the caller; asynchronous on `stream`.
 */
#ifndef SKD_NARROW_WGRAD_H_
#define SKD_NARROW_WGRAD_H_

#include "skd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * 1 when the weight gradient of a (Cout, Cin, 3, 3) convolution fits the 128 x 64 form: stride 1, padding == dilation >= 1,
 * groups 1, Cin and Cout multiples of 64 (Cin in units of 64 rows of the shifted x, two to a tile; Cout in column tiles of 64).
 * A pair of multiples of 128 is taken too, and gives the bits of skd_conv3x3_split_wgrad_nhwc for the same slice count.
 * ---------------------------------------------------------------------------------- */
int skd_conv3x3_narrow_wgrad_supported(int Cin, int Cout, int stride, int padding, int dilation, int groups);

/* ------------------------------------------------------------------------------------
 * The split-K geometry of one weight gradient: pure host arithmetic, no device call; the arguments and plan[0..2] of
 * skd_conv3x3_split_wgrad_plan.  The reduction runs over the P = B * H * W pixels in nk = ceil(P / 16) K-tiles, cut into slices
 * that one workgroup each (per 128 x 64 tile) sums.
 *   slices >= 1  that many, clamped to nk;
 *   slices == 0  the shipped choice for a device of `cus` compute units (0: 256): with tiles = ceil(9 * (Cin / 64) / 2) *
 *                (Cout / 64) and slots = 3 * cus (three workgroups share a compute unit), the count S in
 *                1 .. max(1, slots / tiles) -- at most ONE round of the device -- that minimises
 *                ceil(tiles * S / slots) * ceil(nk / S) -- rounds of the device times the length of a slice -- the smaller
 *                count on a tie.  (The wide plan allows two rounds.  Here a second round buys nothing: the stem's 32,768 K-tiles
 *                over 5 tiles give 153 slices of 215 K-tiles in one round against 307 of 107 in two -- a cost of 215 against
 *                214 for twice the workspace and twice the reduce launch.)
 * Either way the count is then made an exact cover: T = ceil(nk / slices) K-tiles per slice and ceil(nk / T) slices, so no
 * slice is empty.
 *   plan[0] = slices used, plan[1] = K-tiles per slice, plan[2] = workspace bytes = slices * 9 * Cin * Cout * 4.
 * Refused: plan NULL, a size < 1, slices < 0, cus < 0, channel counts the predicate refuses, P >= 2^30.
 * ---------------------------------------------------------------------------------- */
int skd_conv3x3_narrow_wgrad_plan(int B, int H, int W, int Cin, int Cout, int slices, int cus, int64_t *plan);

/* ------------------------------------------------------------------------------------
 * dw[n][c][ty][tx] = sum over the pixels m = (b, y, x) of g[m][n] * x[b, y + (ty - 1) d, x + (tx - 1) d, c] (0 outside the
 * image) for channels-last x (B, H, W, Cin) and g (B, H, W, Cout), d = dilation; the arguments of skd_conv3x3_split_wgrad_nhwc.
 * Two launches on `stream`: the partial sums of every slice into workspace[slice][tap * Cin + c][n] (every element written: the
 * workspace need not be initialised), then their sum in slice order -- the same bits on every call -- written to dw through its
 * four strides in elements (sn, sc, sy, sx), four consecutive c as one 16-byte store where the destination allows it (sc == 1,
 * the other strides multiples of four, dw 16-byte aligned: a dense channels-last weight).
 * `slices` is plan[0] of skd_conv3x3_narrow_wgrad_plan for these sizes, workspace_bytes at least its plan[2].
 * Refused, on the host and in front of the first launch: a NULL pointer; x, g or the workspace not 16-byte aligned; a short
 * workspace; a negative stride; slices < 1 or > nk or not a count the plan returns; dilation < 1; a size < 1; P >= 2^30; channel
 * counts the predicate refuses.
 * ---------------------------------------------------------------------------------- */
int skd_conv3x3_narrow_wgrad_nhwc(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const float *g, float *dw,
                                  int64_t sn, int64_t sc, int64_t sy, int64_t sx, void *workspace, int64_t workspace_bytes,
                                  int slices, skd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SKD_NARROW_WGRAD_H_ */
