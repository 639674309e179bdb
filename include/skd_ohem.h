/*
 * skd_ohem.h -- online hard-example mining for the fused cross-entropy criterion (csrc/ce_ohem.hip): the entry points behind
 * OhemCrossEntropy2d / CriterionOhemDSN (reference utils/criterion.py:11-90, 190-209).  Like the entries of skd_eval.h and
 * skd_eval_ms.h they are outside the frozen core ABI (skd.h): the plain-C oracle implements the core ABI only, so a back-end
 * may lack these (the Python side then raises NotImplementedError naming the missing entry).  Same conventions as skd.h: int
 * return, 1 = success, 0 = failure; raw DEVICE pointers; NULL = optional tensor absent; outputs pre-sized by the caller;
 * asynchronous on `stream`.  Nothing here reads a device value back to the host.
 *
 * Common arguments: logits (B, C, h, w) fp32, target (B, H, W) int64, 1 <= C <= 64 as in skd_ce_dsn_forward; the logits are
 * up-sampled to (H, W), bilinear, align_corners=True, inside the kernels and never exist at that size.
 */
#ifndef SKD_OHEM_H_
#define SKD_OHEM_H_

#include "skd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Floats of workspace that skd_ohem_threshold and skd_ce_ohem_dsn_forward need (one buffer serves both, one call after the
 * other on a stream).  The contents on entry do not matter.  8 for non-positive sizes. */
int64_t skd_ce_ohem_workspace_floats(int B, int C, int h, int w, int H, int W, int factor);

/* ------------------------------------------------------------------------------------
 * The OHEM threshold, OhemCrossEntropy2d.find_threshold (criterion.py:20-48), at 1 / factor resolution.
 *   Hd = round(H * (1.0 / factor)), Wd likewise (half to even, as scipy.ndimage.zoom sizes its output).  Down-sampled index k of
 *   an axis sits at cc = k * ((n_in - 1) / (n_out - 1)) in float64; a coordinate ABOVE n_in - 1 is outside the input (mode
 *   'constant'): there the label is 0 and the probability is 0 (256 -> 32 zeroes the whole last row and column).
 *   label_ds = target[b, min(floor(ccy + 0.5), H - 1), min(floor(ccx + 0.5), W - 1)]            (zoom order 0)
 *   pred_ds  = (float)(p00*wy0*wx0 + p01*wy0*wx1 + p10*wy1*wx0 + p11*wy1*wx1), float64, in that order (zoom order 1, the
 *              arithmetic of skd_zoom_linear), p.. = the fp32 softmax probability of class label_ds at the four full-resolution
 *              pixels around (ccy, ccx), each the softmax of the C bilinearly up-sampled logits of that pixel.
 *   num_valid = number of down-sampled pixels with label_ds != ignore_index;  mk = min_kept / (factor * factor) (integer).
 *   threshold = 1.0f when mk >= num_valid; otherwise thresh, or the mk-th smallest pred_ds over the valid pixels when mk > 0
 *   and that value is greater than thresh (fp32 comparisons).  The selection is an exact radix select on the bit patterns:
 *   bit-reproducible.  A label outside [0, C) that is not ignore_index counts as valid with probability 0 (the loss entry
 *   turns the whole result into NaN for such a target).
 *   threshold [1] fp32, num_valid [1] int32: device memory.  pred_ds (B, Hd, Wd) fp32 or NULL: the keys, -1 where ignored.
 * Returns 0 for non-positive sizes, C > 64, factor < 1, min_kept < 0, NULL logits / target / threshold / num_valid /
 * workspace, a down-sampled size of 0, or a down-sampled size of 1 along an axis whose input is longer than 1.
 * ---------------------------------------------------------------------------------- */
int skd_ohem_threshold(int B, int C, int h, int w, int H, int W, const float *logits_main, const int64_t *target,
                       int ignore_index, float thresh, int min_kept, int factor, float *threshold, int32_t *num_valid,
                       float *pred_ds, float *workspace, skd_stream_t stream);

/* ------------------------------------------------------------------------------------
 * CriterionOhemDSN.forward (criterion.py:200-209) given the threshold (DEVICE memory, [1]):
 *   a main-head pixel is kept iff target != ignore_index and p_label <= threshold[0], p_label the fp32 softmax probability of
 *   its label (the same device function as in skd_ohem_threshold);
 *   loss = mean over the kept pixels of -log p (main) + aux_weight * mean over the valid pixels of -log p (dsn);
 *   grad_main = (softmax - onehot) / n_kept over the kept pixels, grad_dsn = aux_weight * (softmax - onehot) / n_valid, both
 *   pulled back through the bilinear weights.  No kept pixel: NaN, like CrossEntropyLoss.  A label outside [0, C) that is not
 *   ignore_index: NaN loss, NaN n_kept and NaN gradients, as in skd_ce_dsn_forward.
 *   logits_dsn NULL: the single-head form (OhemCrossEntropy2d; grad_dsn must be NULL).  grad_main / grad_dsn (B, C, h, w) or
 *   NULL.  loss [1];  n_kept [1] fp32 or NULL;  kept (B, H, W) uint8 or NULL: 1 where the main head kept the pixel.
 *   workspace: skd_ce_ohem_workspace_floats floats.
 * Returns 0 on the conditions of skd_ce_dsn_forward and for a NULL threshold.
 * ---------------------------------------------------------------------------------- */
int skd_ce_ohem_dsn_forward(int B, int C, int h, int w, int H, int W, const float *logits_main, const float *logits_dsn,
                            const int64_t *target, int ignore_index, float aux_weight, const float *threshold, float *loss,
                            float *n_kept, uint8_t *kept, float *grad_main, float *grad_dsn, float *workspace,
                            skd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SKD_OHEM_H_ */
