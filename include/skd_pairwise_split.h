/*
 * skd_pairwise_split.h -- the two matrix products of the pair-wise similarity loss on the split-operand bf16-MFMA core
 * (csrc/pairwise_split.hip): the twins of skd_pairwise_gram_loss and skd_pairwise_backward of skd.h, which run on the fp32 MFMA.
 * Like the entries of skd_eval.h, skd_eval_ms.h, skd_ohem.h, skd_infer.h, skd_train.h, skd_wgrad.h, skd_narrow.h,
 * skd_narrow_wgrad.h, skd_shortcut.h, skd_split2.h, skd_bnstats.h and skd_stride2.h they are outside the frozen core ABI (skd.h):
 * the plain-C oracle implements the core ABI only, so a back-end may lack them (the loss then stays on the fp32 kernels, as
 * before).  Same conventions as skd.h: int return, 1 = success, 0 = refused with nothing launched; raw DEVICE pointers; outputs
 * pre-sized by the caller; asynchronous on `stream`.
 *
 * Every fp32 operand is split into three bf16 pieces on its way into LDS and the six products a_i b_j with i + j <= 2 are
 * accumulated in fp32, a0 b0 in an accumulator set of its own (csrc/conv1x1.hip documents the core, csrc/conv3x3.hip the two
 * sets).  The argument lists are those of the fp32 twins: a caller can hand both the same buffers.  Only the workspaces differ.
 */
#ifndef SKD_PAIRWISE_SPLIT_H_
#define SKD_PAIRWISE_SPLIT_H_

#include "skd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * Floats of workspace for skd_pairwise_split_gram_loss: a node-major copy of both normalised panels, (B, ldm, Kp) with
 * Kp = roundup(Ct, 16) + roundup(Cs, 16) and ldm = skd_pairwise_ldm(M), followed by one loss partial per workgroup.
 * Pure host arithmetic, no device call; 1 for a size < 1.
 * ---------------------------------------------------------------------------------- */
int64_t skd_pairwise_split_workspace_floats(int B, int Cs, int Ct, int M);

/* ------------------------------------------------------------------------------------
 * G[b] = Fh_T[b]^T Fh_T[b] - Fh_S[b]^T Fh_S[b] and loss[0] = sum(G[:, :M, :M]^2) / M^2 / B.
 * fhat_s (B, Cs, ldm) and fhat_t (B, Ct, ldm): the channel-major, zero-padded buffers skd_channel_l2_normalise writes, 16-byte
 * aligned; any Cs, Ct >= 1.  G (B, ldm, ldm), 16-byte aligned, or NULL for the loss alone; every element of G is written, rows
 * and columns >= M with +0.0.  Only the tiles of the upper triangle are computed and each element above the diagonal is stored a
 * second time in its mirror position: G equals its transpose bit for bit.  The loss is the fixed-order sum of one partial per
 * workgroup: no atomics, the same bits on every call.  Three launches on `stream` (node-major copy, Gram, final sum); the
 * workspace need not be initialised.
 * Refused on the host: a NULL pointer other than G; a size < 1; ldm != skd_pairwise_ldm(M); B > 65535; Cs + Ct > 2^20;
 * fhat_s, fhat_t, G or the workspace not 16-byte aligned.
 * ---------------------------------------------------------------------------------- */
int skd_pairwise_split_gram_loss(int B, int Cs, int Ct, int M, int ldm, const float *fhat_s, const float *fhat_t, float *G,
                                 float *loss, float *workspace, skd_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Floats of workspace for skd_pairwise_split_backward: when the contraction over the nodes is cut into S > 1 slices, S raw
 * 64 x 128 partial tiles per output tile; 1 otherwise.  Pure host arithmetic, no device call; 1 for a size < 1.
 * ---------------------------------------------------------------------------------- */
int64_t skd_pairwise_split_backward_workspace_floats(int B, int Cs, int M);

/* ------------------------------------------------------------------------------------
 * dpooled[b][c][m] = coef * grad_loss[0] * (sum_n fhat_s[b][c][n] * G[b][m][n]) / norm_s[b][m],  coef = -4 / (M^2 B).
 * G (B, ldm, ldm) must be symmetric (it is read along its rows), norm_s (B, M), dpooled (B, Cs, ldm): columns >= M are written
 * with +0.0, nothing else is.  fhat_s, G, dpooled and the workspace 16-byte aligned.  One launch, or -- when the node range is
 * cut into slices -- two: the slices' partial tiles into the workspace, then their sum in slice order (no atomics, the same bits
 * on every call; every element the second launch reads is written by the first).
 * Refused on the host: a NULL pointer; a size < 1; ldm != skd_pairwise_ldm(M); B > 65535; a misaligned buffer.
 * ---------------------------------------------------------------------------------- */
int skd_pairwise_split_backward(int B, int Cs, int M, int ldm, const float *fhat_s, const float *G, const float *norm_s,
                                const float *grad_loss, float *dpooled, float *workspace, skd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SKD_PAIRWISE_SPLIT_H_ */
