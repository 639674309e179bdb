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

#ifdef __cplusplus
}
#endif

#endif /* SKD_EVAL_H_ */
