/*
 * skd_eval.h -- evaluation entry points of libskd_hip.so that are not part of the frozen core ABI (skd.h): the
 * plain-C oracle implements the core ABI only, so a back-end may lack these (the Python side then raises
 * NotImplementedError naming the missing entry).  Same conventions as skd.h: int return, 1 = success, 0 = failure;
 * raw DEVICE pointers; NULL = optional tensor absent; outputs pre-sized by the caller; asynchronous on `stream`.
 */
#ifndef SKD_EVAL_H_
#define SKD_EVAL_H_

#include "skd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * Sliding-window evaluation tail, networks/evaluate.py:70-104, 187-198:
 *   for every tile t (row-major order of the table) the logits (C, h, w) are up-sampled to (tile_h, tile_w), bilinear,
 *   align_corners=True, fp32 (the four-term expression of the whole-image entry, individually rounded), cropped to
 *   [0 : y2 - y1, 0 : x2 - x1] and added in float64 to the window [y1 : y2, x1 : x2] of the (H, W) image;
 *   probs = sum / cover count (float64);  pred = argmax_c probs (first maximum, uint8).
 * One lane per image pixel gathers from every tile that covers it, in table order, so the float64 sums equal the
 * tile-after-tile accumulation bit for bit and nothing of size H x W x C exists unless `probs` is asked for.
 *   logits (T, C, h, w) fp32;  tiles (T, 4) int32 rows (y1, x1, y2, x2) in DEVICE memory (T is unbounded and every lane
 *   reads the same row, which the scalar unit serves from its cache; a by-value table would cap T), 0 <= y1 < y2 <= H,
 *   y2 - y1 <= tile_h, same for x; a pixel no tile covers gets NaN probabilities and prediction 0;
 *   target (H, W) int64 or NULL;  remap: 256 uint8 applied to the WRITTEN prediction only (trainId -> id), or NULL;
 *   pred (H, W) uint8 or NULL;  probs (H, W, C) float64 or NULL;  confusion (C, C) int64, ACCUMULATED into with the
 *   un-remapped prediction over the pixels with target != ignore_index and 0 <= target < C (required with target).
 * 1 <= C <= 32; anything else returns 0.
 * ---------------------------------------------------------------------------------- */
int skd_seg_sliding(int T, int C, int h, int w, int tile_h, int tile_w, int H, int W, const float *logits,
                    const int *tiles, const int64_t *target, int ignore_index, const uint8_t *remap, uint8_t *pred,
                    double *probs, int64_t *confusion, skd_stream_t stream);

/* ------------------------------------------------------------------------------------
 * 3x3 stride-1 "same" convolution of a FROZEN network as an implicit GEMM on the split-operand bf16-MFMA core
 * (csrc/conv3x3.hip; the core and its numerics: csrc/conv1x1.hip), inference only:
 *   out[b][h][w][n] = act( ((sum_{ty,tx,c} x[b][h + (ty-1) d][w + (tx-1) d][c] * w[n][c][ty][tx] + conv_bias[n] - mean[n])
 *                           * invstd[n]) * (|weight[n]| + eps) + bias[n] ),     taps outside the image are exact zeros;
 *   x (B, H, W, Cin) and out (B, H, W, Cout) channels-last fp32, x 16-byte aligned; any H, W >= 1 and dilation d >= 1.
 *   conv_bias NULL: none.  mean / var NULL (both): no normalisation (weight / bias ignored); with them, weight / bias may be
 *   NULL (gamma 1, beta 0) -- the eval-mode InPlace-ABN formula of skd_conv1x1_abn_nhwc.  activation: SKD_ACT_*.
 * skd_conv3x3_split_supported(): Cin % 16 == 0, Cout % 128 == 0, stride 1, padding == dilation >= 1, groups 1.
 * The weight is split ONCE into three bf16 planes laid out as the kernel's LDS image: skd_conv3x3_split_pack_bytes() bytes
 * (6 per weight), 16-byte aligned, written by skd_conv3x3_split_pack_weights() from a (Cout, Cin, 3, 3) fp32 tensor of ANY
 * memory format -- stride_* are its strides in elements.  A frozen network packs once; re-pack when the weight changes.
 * geometry: 0 = the shipped choice per problem size; for measurements 1 = 128-pixel x 128-channel tiles, 2 = 64-pixel tiles,
 * 3 = 128-pixel tiles for the launch's whole rounds and 64 for the rest.  Same result for every geometry.
 * ---------------------------------------------------------------------------------- */
int skd_conv3x3_split_supported(int Cin, int Cout, int stride, int padding, int dilation, int groups);
int64_t skd_conv3x3_split_pack_bytes(int Cin, int Cout);
int skd_conv3x3_split_pack_weights(int Cin, int Cout, const float *w, int64_t stride_n, int64_t stride_c, int64_t stride_y,
                                   int64_t stride_x, void *pack, int64_t pack_bytes, skd_stream_t stream);
int skd_conv3x3_split_nhwc(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const void *wpack, float *out,
                           const float *conv_bias, const float *mean, const float *var, const float *weight, const float *bias,
                           float eps, int activation, float slope, int geometry, skd_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Launch geometry of skd_conv1x1_abn_nhwc / skd_conv1x1_abn_pro_nhwc (csrc/conv1x1.hip) for an (M, K, N) problem on a device of
 * `cus` compute units: HOST arithmetic only, no device is touched, so a test can check on any machine that the workgroups of
 * a launch cover the M x N output exactly once.  Both return 0 for a problem skd_conv1x1_abn_supported() refuses, cus < 0 or
 * a grid beyond 2^31 - 1 workgroups.
 *   geometry: out[7] = tiles_n (column tiles of 128), ct (column tiles per weight chunk), pm (row panels per panel group),
 *     p_full (row panels of 128 rows; the panels behind them are 64 rows high), panels (all row panels), grid (workgroups),
 *     nt (1: wide output -- super-tile order and non-temporal stores; 0: panel-major order).
 *   tile_of: out[3 i ...] = m0, rows, n0 of workgroup block + i for 0 <= i < count (all inside [0, grid), else 0 is returned):
 *     the workgroup writes rows [m0, min(m0 + rows, M)) x columns [n0, n0 + 128); rows = 128 or 64, or 0 for a padding
 *     workgroup that exits.  The same inline function decodes blockIdx.x in the kernel.
 * ---------------------------------------------------------------------------------- */
int skd_conv1x1_abn_geometry(int64_t M, int K, int N, int cus, int64_t *out);
int skd_conv1x1_abn_tile_of(int64_t M, int K, int N, int cus, int64_t block, int64_t count, int64_t *out);

#ifdef __cplusplus
}
#endif

#endif /* SKD_EVAL_H_ */
