/*
 * skd_planes.h -- PIECE PLANES: an activation map handed from one split-core kernel to the next as the three bf16 pieces the
 * consumer's MFMAs read, instead of as fp32 that the consumer cuts up again for every tap and every column tile.  The frozen
 * teacher's Bottleneck link conv1 -> bn1 -> relu -> conv2: the split reduce GEMM (csrc/conv1x1.hip) writes the pieces of its
 * epilogue's value, the wide stride-1 3x3 convolution (csrc/conv3x3.hip with PLANES) loads them straight into its LDS image.
 * Opt-in (pspnet_combine.route_teacher_planes; kd_model's switch ``teacher_planes`` / SKD_TEACHER_PLANES=1).
 *
 * EQUALITY CONTRACT.  The pieces are exactly those the consumer's own split (split4, csrc/conv_split_dev.hpp) makes of the fp32
 * value: p0 = bf16(v), p1 = bf16(v - p0), p2 = bf16(v - p0 - p1), round to nearest even, both residuals exact in fp32.  The
 * split is a pure function of v, so the consumer sees the same bf16 operands in the same order and its output is BIT FOR BIT
 * that of skd_conv3x3_split_nhwc on the fp32 map; the producer's fp32 value is that of skd_conv1x1_abn_nhwc (the same
 * expression in the epilogue).  A speed feature, not an accuracy trade (tests/test_conv_planes_gpu.py, no tolerance anywhere).
 * Three pieces only: the two-piece mode of skd_split2.h has no planes form.
 *
 * LAYOUT.  One allocation of skd_planes_bytes(M, C) = 6 M C bytes, 16-byte aligned, for a map of M = B H W rows and C channels,
 * C a multiple of 16.  Interleaved per quad of four channels: the 4 channels x 3 pieces of one row and quad are 24 contiguous
 * bytes (piece 0 | piece 1 | piece 2, 8 bytes each), a row's quads follow each other, rows follow each other; there is no
 * padding.  Why: a thread of the consumer's K loop owns four consecutive k of a row, i.e. exactly one such 24-byte run (a 16-byte
 * and an 8-byte load), the row's four threads cover the K-tile's 96 bytes completely, and a tap shift moves whole rows, as in the
 * fp32 map; a planar layout would put a thread's three loads M C * 2 bytes apart.  The layout is DEFINED by one address function (planes_offset,
 * csrc/conv_split_dev.hpp) that every kernel calls and that skd_planes_offset exports: callers and tests build and decode planes
 * through it and never hard-code the above.
 *
 * An extension header: like the entries of skd_eval.h ... skd_pairwise_split.h these are outside the
 * frozen core ABI (skd.h) -- the plain-C oracle implements the core ABI only, so a back-end may lack them (the teacher then keeps
 * its fp32 link; kd_model warns once when the switch asks for them).  Same conventions as skd.h: int return, 1 = success, 0 =
 * refused with nothing launched; raw DEVICE pointers unless stated; NULL = optional tensor absent; outputs pre-sized by the
 * caller; asynchronous on `stream`.
 *
 * Memory contract of the four device entries: rows at or beyond M are neither read nor written; no byte outside the stated
 * buffers is touched; planes are written at exactly the offsets of the map for rows < M (all 6 M C bytes, the layout has no
 * padding bytes).
 */
#ifndef SKD_PLANES_H_
#define SKD_PLANES_H_

#include "skd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * HOST ONLY.  1 when the kernels take a map of C channels: C >= 1 and a multiple of 16.
 * ---------------------------------------------------------------------------------- */
int skd_planes_supported(int C);

/* ------------------------------------------------------------------------------------
 * HOST ONLY.  *bytes = the size of the planes of an (M, C) map.  bytes is a HOST pointer.
 * Refused: M < 1, C the predicate refuses, M > 2^40, bytes NULL.
 * ---------------------------------------------------------------------------------- */
int skd_planes_bytes(int64_t M, int C, int64_t *bytes);

/* ------------------------------------------------------------------------------------
 * HOST ONLY, no device is touched: THE layout -- *byte_offset = offset of the bf16 that is piece `piece` (0, 1, 2) of element
 * (row, channel) inside the planes of an (M, C) map.  The function the kernels call.  byte_offset is a HOST pointer.
 * Refused: sizes skd_planes_bytes refuses; row outside 0 .. M - 1, channel outside 0 .. C - 1, piece outside 0 .. 2; NULL.
 * ---------------------------------------------------------------------------------- */
int skd_planes_offset(int64_t M, int C, int64_t row, int channel, int piece, int64_t *byte_offset);

/* ------------------------------------------------------------------------------------
 * planes = the pieces of x (M, C) fp32 channels-last: a stand-alone streaming kernel, for a map no producer wrote.
 * Refused: sizes skd_planes_bytes refuses; x or planes NULL or not 16-byte aligned.
 * ---------------------------------------------------------------------------------- */
int skd_planes_split_nhwc(int64_t M, int C, const float *x, void *planes, skd_stream_t stream);

/* ------------------------------------------------------------------------------------
 * x (M, C) fp32 = (p0 + p1) + p2 of the planes, a zero sum with p0's sign (so -0.0 comes back as -0.0): the inverse of the split
 * for every fp32 value three bf16 pieces can carry -- all of magnitude 2^-109 and above below the bf16 overflow threshold, +-0, and
 * the smaller ones whose low bits are clear (a bf16 piece has no bit below 2^-133).  A debugging and test aid; no routed path
 * calls it.  Refusals as skd_planes_split_nhwc.
 * ---------------------------------------------------------------------------------- */
int skd_planes_join_nhwc(int64_t M, int C, const void *planes, float *x, skd_stream_t stream);

/* ------------------------------------------------------------------------------------
 *   planes_out = pieces( act( ((x . w^T - mean) * invstd) * (|weight| + eps) + bias ) )
 * the split GEMM of skd_conv1x1_abn_nhwc (skd.h) without residual, three pieces per operand, its epilogue's fp32 value cut into
 * its pieces and written to the planes of the (M, N) output; no fp32 output exists.  x (M, K) and w (N, K) fp32, mean / var
 * required, weight / bias optional, as there.  The predicate is skd_conv1x1_abn_supported(M, K, N) (N a multiple of 128, so the
 * planes' channel count is always supported).
 * Refused: what the predicate refuses; x, w, planes_out, mean or var NULL; x, w or planes_out not 16-byte aligned; an
 * activation skd_conv1x1_abn_nhwc refuses.
 * ---------------------------------------------------------------------------------- */
int skd_conv1x1_abn_planes_nhwc(int64_t M, int K, int N, const float *x, const float *w, void *planes_out, const float *mean,
                                const float *var, const float *weight, const float *bias, float eps, int activation, float slope,
                                skd_stream_t stream);

/* ------------------------------------------------------------------------------------
 *   out = act( ABN_eval(conv3x3(join(planes_in), padding = dilation) + conv_bias) )
 * skd_conv3x3_split_nhwc (skd_eval.h) -- the wide stride-1 form, three pieces, no residual -- with the planes of the
 * (B, H, W, Cin) input in x's place: the same wpack (skd_conv3x3_split_pack_weights), geometries and epilogue arguments; out
 * (B, H, W, Cout) fp32 channels-last, bit for bit that entry's output on the fp32 map whose pieces the planes hold.  A tap
 * outside the image is not loaded and contributes exact zeros in all three pieces.
 * Refused: channel counts skd_conv3x3_split_supported refuses (Cin a multiple of 16, Cout of 128); a size < 1; dilation < 1;
 * planes_in, wpack or out NULL; planes_in or wpack not 16-byte aligned; mean without var or var without mean; an unknown
 * activation; a geometry outside 0..3; H * W >= 2^31.
 * ---------------------------------------------------------------------------------- */
int skd_conv3x3_split_planes_nhwc(int B, int H, int W, int Cin, int Cout, const void *planes_in, const void *wpack, float *out,
                                  const float *conv_bias, const float *mean, const float *var, const float *weight,
                                  const float *bias, float eps, int activation, float slope, int dilation, int geometry,
                                  skd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SKD_PLANES_H_ */
