/*
 * skd_eval_ms.h -- multi-scale / flip evaluation entry points of libskd_hip.so (csrc/evaluate_multiscale.hip).  Like the entries
 * of skd_eval.h they are outside the frozen core ABI (skd.h): the plain-C oracle implements the core ABI only, so a back-end
 * may lack these (the Python side then raises NotImplementedError naming the missing entry).  Same conventions as skd.h: int
 * return, 1 = success, 0 = failure; raw DEVICE pointers; NULL = optional tensor absent; outputs pre-sized by the caller;
 * asynchronous on `stream`.
 */
#ifndef SKD_EVAL_MS_H_
#define SKD_EVAL_MS_H_

#include "skd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * Image resize of networks/evaluate.py:127, scipy.ndimage.zoom(image, (1, 1, s, s), order=1, prefilter=False):
 *   output index k of an axis sits at cc = k * ((n_in - 1) / (n_out - 1)), formed in float64; a coordinate ABOVE n_in - 1 is
 *   outside the input (scipy's default mode 'constant') and the output element is 0 -- for some sizes the last coordinate
 *   rounds up and the WHOLE last row / column is zero (1024 rows to 768 is one); this is reproduced on purpose;
 *   t = cc - floor(cc), weights (1 - t, t);  out = (float)(p00*wy0*wx0 + p01*wy0*wx1 + p10*wy1*wx0 + p11*wy1*wx1), float64,
 *   summed in that order, each product formed left to right, no contraction, one cast.
 *   image (C, H, W) fp32;  out (F, C, Ho, Wo) fp32 with F = 1 + (mirror != 0); with channels_last != 0 its memory is
 *   (F, Ho, Wo, C).  Element 1 is element 0 mirrored in X (scale_image[:, :, :, ::-1]), written by the same launch.
 *   The caller passes Ho, Wo: scipy's are Python's round(n * s), which rounds half to even.
 * Returns 0 for non-positive sizes, Ho < 2 or Wo < 2, NULL pointers.
 * ---------------------------------------------------------------------------------- */
int skd_zoom_linear(int C, int H, int W, int Ho, int Wo, const float *image, float *out, int mirror, int channels_last,
                    skd_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Multi-scale / flip evaluation tail, networks/evaluate.py:115-134, 187-198.  For every scale s in table order:
 *   a = map 0 of the scale, up-sampled to (H, W), bilinear, align_corners=True, fp32 (the four-term expression of
 *       skd_seg_confusion, individually rounded; scale factors (h_s - 1) / (H - 1) and (w_s - 1) / (W - 1) as fp32 quotients,
 *       0 where the output axis is 1);
 *   F = 2: b = map 1 (the forward of the X-mirrored image) up-sampled the same way and read at (Y, W - 1 - X);
 *          v = 0.5f * (a + b) in fp32;      F = 1: v = a;
 *   sum += (double)v.
 *   probs = sum / (double)S;  pred = argmax_c probs (first maximum, uint8).
 * One lane per output pixel walks the scales, so the float64 sums equal the scale-after-scale accumulation bit for bit and
 * nothing of size H x W x C exists unless `probs` is asked for.
 *   logits: one packed fp32 buffer;  table (S, 3) int64 rows (offset in floats, h_s, w_s) in DEVICE memory (every lane reads
 *   the same row): the maps of scale s are (F, C, h_s, w_s), contiguous at logits + offset.  Source indices are clamped to
 *   [0, h_s - 1] x [0, w_s - 1] and plane offsets are 64-bit, so no table content makes a lane read outside the map the row
 *   describes; the caller keeps a map at 2^31 - 1 floats or fewer (the Python side refuses more).
 *   target (H, W) int64 or NULL;  remap: 256 uint8 applied to the WRITTEN prediction only (trainId -> id), or NULL;
 *   pred (H, W) uint8 or NULL;  probs (H, W, C) float64 or NULL;  confusion (C, C) int64, ACCUMULATED into with the
 *   un-remapped prediction over the pixels with target != ignore_index and 0 <= target < C (required with target).
 * Returns 0 for S <= 0, F outside {1, 2}, C outside 1 .. 32, non-positive H or W, NULL logits or table, target without
 * confusion.
 * ---------------------------------------------------------------------------------- */
int skd_seg_multiscale(int S, int F, int C, int H, int W, const float *logits, const int64_t *table, const int64_t *target,
                       int ignore_index, const uint8_t *remap, uint8_t *pred, double *probs, int64_t *confusion,
                       skd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SKD_EVAL_MS_H_ */
