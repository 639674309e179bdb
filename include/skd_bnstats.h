/*
 * skd_bnstats.h -- entry points of the training student's 3x3 convolutions that emit the batch-norm statistics of their own
 * output from the epilogue (csrc/conv3x3.hip, the STATS form of its one kernel), and of the small kernel that finishes them
 * (csrc/abn_nhwc.hip).  With them the InPlace-ABN forward behind such a convolution is a finalize launch of a few workgroups and
 * the pure streaming pass skd_abn_apply_nhwc_to: the conv output is not read a second time for its statistics and no partial sum
 * is handed across the grid.  Like the entries of skd_eval.h, skd_eval_ms.h, skd_ohem.h, skd_infer.h, skd_train.h, skd_wgrad.h,
 * skd_narrow.h, skd_narrow_wgrad.h, skd_shortcut.h and skd_split2.h they are outside the frozen core ABI (skd.h): the plain-C
 * oracle implements the core ABI only, so a back-end may lack them (the convolutions and the ABN forward then run what they ran
 * before).  Same conventions as skd.h: int return, 1 = success, 0 = refused with nothing launched; raw DEVICE pointers; NULL =
 * optional tensor absent; outputs pre-sized by the caller; asynchronous on `stream`.
 *
 * The statistics workspace of an output of M = B * H * W pixels and Cout channels (channels-last) holds one record per 32-row
 * block of M and channel:
 *     stats[(block * Cout + channel) * 2 + 0] = mean of the block's rows of that channel
 *     stats[(block * Cout + channel) * 2 + 1] = M2, the sum of their squared deviations about THAT mean
 * for block = 0 .. ceil(M / 32) - 1, over the rows 32 * block .. min(M, 32 * block + 32) - 1.  The count of a block,
 * min(32, M - 32 * block), follows from (M, block) and is not stored.  Both numbers are computed in fp32 from the fp32 values the
 * convolution stores (after the conv bias), in two passes about the block's own mean: there is no pivot and no sum of squares,
 * so a channel whose offset is large against its spread keeps its variance.  The layout and the bits of a record depend on the
 * output alone: not on the tile geometry and not on the column width of the kernel that wrote it.  Every record is written by
 * every call (plain vector stores, no atomics): the workspace need not be initialised.
 */
#ifndef SKD_BNSTATS_H_
#define SKD_BNSTATS_H_

#include "skd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * Floats of the statistics workspace for M output pixels and Cout channels: ceil(M / 32) * Cout * 2.  0 for sizes no entry
 * below takes: M < 1, Cout < 1 or not a multiple of 64.
 * ---------------------------------------------------------------------------------- */
int64_t skd_conv3x3_bnstats_floats(int64_t M, int Cout);

/* ------------------------------------------------------------------------------------
 * out = conv3x3(x) + conv_bias exactly as skd_conv3x3_split_nhwc(B, H, W, Cin, Cout, dilation, x, wpack, out, conv_bias, NULL,
 * NULL, NULL, NULL, 0, SKD_ACT_NONE, 0, geometry, stream) writes it -- the same bits -- plus the statistics records of `out` in
 * `stats`.  conv_bias may be NULL.  geometry 0 .. 3 as in skd_eval.h; the records do not depend on it.
 * Refused (returns 0, nothing launched): everything the plain entry refuses (a NULL x, wpack or out; x or wpack not 16-byte
 * aligned; a size < 1; geometry outside 0 .. 3; channel counts or a dilation skd_conv3x3_split_supported refuses); stats NULL
 * or not 8-byte aligned; stats_floats < skd_conv3x3_bnstats_floats(B * H * W, Cout).
 * ---------------------------------------------------------------------------------- */
int skd_conv3x3_split_stats_nhwc(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const void *wpack, float *out,
                                 const float *conv_bias, int geometry, float *stats, int64_t stats_floats, skd_stream_t stream);

/* ------------------------------------------------------------------------------------
 * The same on the 64-column form (skd_narrow.h: wpack of skd_conv3x3_narrow_pack_pair, Cout a multiple of 64, geometry 0 or 1):
 * the bits of skd_conv3x3_narrow_nhwc without residual, BN terms and activation, and -- at a Cout both forms take -- the records
 * of skd_conv3x3_split_stats_nhwc bit for bit.  Refusals as above, with skd_conv3x3_narrow_supported and geometry 0 .. 1.
 * ---------------------------------------------------------------------------------- */
int skd_conv3x3_narrow_stats_nhwc(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const void *wpack,
                                  float *out, const float *conv_bias, int geometry, float *stats, int64_t stats_floats,
                                  skd_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Finalize: mean[c] and the biased var[c] of a (rows, C) channels-last tensor from its ceil(rows / 32) records per channel, and
 * -- when the running pointers are not NULL -- the running-statistics update of skd_abn_forward_train_nhwc:
 *     running_mean = running_mean * (1 - momentum) + momentum * mean
 *     running_var  = running_var  * (1 - momentum) + momentum * var * rows / (rows - 1)        (rows == 1: var itself)
 * One launch.  The records of a channel are combined in double precision in a fixed order: as sums shifted by the mean of the
 * channel's block 0 -- S1 = sum n_b (mean_b - K), S2 = sum M2_b + n_b (mean_b - K)^2, the form the other statistics kernels
 * finish with -- over 128 interleaved runs of blocks, the runs added in a fixed order; mean = K + S1 / rows, var = (S2 - S1^2 /
 * rows) / rows.  No atomics: the same bits on every call.
 * Refused (returns 0, nothing launched): rows < 1; C < 16 or not a multiple of 16; stats, mean or var NULL; stats not 8-byte
 * aligned; stats_floats < ceil(rows / 32) * C * 2.
 * ---------------------------------------------------------------------------------- */
int skd_abn_stats_from_partials_nhwc(int64_t rows, int C, const float *stats, int64_t stats_floats, float *mean, float *var,
                                     float *running_mean, float *running_var, float momentum, skd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SKD_BNSTATS_H_ */
