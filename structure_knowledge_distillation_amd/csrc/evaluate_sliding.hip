// evaluate_sliding.hip -- sliding-window evaluation tail for gfx950: per-tile bilinear upsample (align_corners) of the
// class logits, float64 accumulation over the overlapping tiles, mean, argmax, optional id remap, confusion matrix --
// one fused gather kernel.
//
// Reference: networks/evaluate.py:70-104 (predict_sliding: every tile's logits are up-sampled to the tile size, copied
// to the host, cropped and added into float64 full_probs / count_predictions arrays of H x W x C, tile after tile, then
// divided), :187-198 (argmax -> uint8, id remap for the test split, confusion matrix over the non-ignored pixels).
// Here one lane owns one pixel (Y, X) of the full image and walks the tile table in order.  For every tile that covers
// the pixel it rebuilds its C up-sampled logits from the 4 neighbouring source pixels of that tile's logit map (all
// maps together are a few MB: L2 resident) with the four-term expression of evaluate.hip, promotes to double and adds
// into C register accumulators.  The additions happen in tile order, exactly the order of the reference's `+=`, so the
// float64 sums carry the same bits and no H x W x C array is needed: per pixel the kernel reads 8 B of label and writes
// 1 B of prediction (plus 8 C bytes when the probabilities are asked for).
// The accumulators are indexed by fully unrolled loops over a compile-time bound CT >= C (8, 16, 19, 21, 32), so they
// stay in registers (2 CT VGPRs); a class count above 32 is refused by the entry point rather than spilled.
// The tile table lives in device memory: every lane reads the same row, so the loads are scalar and cached, and the
// number of tiles is not capped by the kernel-argument size.
// Floating-point contraction is OFF in this file, as in evaluate.hip: individually rounded mul / add.  The interpolation and the
// epilogue are shared with evaluate_multiscale.hip and live in eval_dev.hpp (contraction is off there too).
#include "eval_dev.hpp"
#include "skd_eval.h"

#pragma clang fp contract(off)

namespace skd {
namespace {

template <int CT>
__global__ __launch_bounds__(kThreads) void seg_sliding_kernel(
    const float *__restrict__ logits, const int *__restrict__ tiles, const int64_t *__restrict__ target,
    const unsigned char *__restrict__ remap, unsigned char *__restrict__ pred, double *__restrict__ probs,
    unsigned long long *__restrict__ confusion, int T, int C, int h, int w, int H, int W, int ignore_index, float sy,
    float sx) {
  extern __shared__ unsigned int hist[];  // C * C
  hist_clear(hist, C);
  const int64_t total = (int64_t)H * W;
  const int hw = h * w;
  const int64_t chw = (int64_t)C * hw;
  for (int64_t pix = (int64_t)blockIdx.x * kThreads + threadIdx.x; pix < total; pix += (int64_t)gridDim.x * kThreads) {
    const int X = (int)(pix % W);
    const int Y = (int)(pix / W);
    double acc[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[c] = 0.0;
    int cover = 0;
    for (int t = 0; t < T; ++t) {
      const int ty1 = tiles[4 * t + 0], tx1 = tiles[4 * t + 1], ty2 = tiles[4 * t + 2], tx2 = tiles[4 * t + 3];
      if (Y < ty1 || Y >= ty2 || X < tx1 || X >= tx2) continue;
      const Bilinear b = bilinear_at(sy, sx, Y - ty1, X - tx1, h, w);  // at (Y - y1, X - x1) of the tile
      const float *p = logits + (int64_t)t * chw;
#pragma unroll
      for (int c = 0; c < CT; ++c)
        if (c < C) acc[c] += (double)bilinear_value(b, p + c * hw);
      ++cover;
    }
    // 0 / 0 = NaN for a pixel outside every tile
    finish_pixel<CT>(acc, (double)cover, C, pix, target, ignore_index, remap, pred, probs, hist);
  }
  hist_flush(hist, C, confusion);
}

}  // namespace
}  // namespace skd

using namespace skd;

extern "C" {

int skd_seg_sliding(int T, int C, int h, int w, int tile_h, int tile_w, int H, int W, const float *logits,
                    const int *tiles, const int64_t *target, int ignore_index, const uint8_t *remap, uint8_t *pred,
                    double *probs, int64_t *confusion, skd_stream_t stream) {
  if (T <= 0 || C <= 0 || C > kMaxAccumClasses || h <= 0 || w <= 0 || tile_h <= 0 || tile_w <= 0 || H <= 0 || W <= 0) return 0;
  if (!logits || !tiles) return 0;
  if (target != nullptr && confusion == nullptr) return 0;
  if ((int64_t)C * h * w > (int64_t)INT32_MAX) return 0;  // per-tile offsets are 32-bit
  const float sy = tile_h > 1 ? (float)(h - 1) / (float)(tile_h - 1) : 0.f;
  const float sx = tile_w > 1 ? (float)(w - 1) / (float)(tile_w - 1) : 0.f;
  const dim3 grid(accum_grid((int64_t)H * W)), block(kThreads);
  const size_t lds = sizeof(unsigned int) * C * C;
  unsigned long long *cm = reinterpret_cast<unsigned long long *>(confusion);
  hipStream_t st = as_stream(stream);
  with_class_bound(C, [&](auto ct) {
    seg_sliding_kernel<decltype(ct)::value><<<grid, block, lds, st>>>(logits, tiles, target, remap, pred, probs, cm, T, C, h, w,
                                                                      H, W, ignore_index, sy, sx);
  });
  return ok();
}

}  // extern "C"
