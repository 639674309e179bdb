// evaluate_multiscale.hip -- multi-scale / flip evaluation for gfx950: the image resize of scipy.ndimage.zoom(order=1,
// prefilter=False) as one small kernel, and the whole tail -- align-corners upsample of every scale's logits, fp32 flip
// average, float64 sum in scale order, mean, argmax, optional id remap, confusion matrix -- as one fused gather kernel.
//
// Reference: networks/evaluate.py:115-134 (predict_multiscale: per scale ndimage.zoom on the host, one or two forwards, each
// up-sampled to H x W x C on the GPU and copied to the host, `0.5 * (a + b[:, ::-1, :])` in fp32, `full_probs += ...` and
// `/= len(scales)` in float64), :187-198 (argmax -> uint8, id remap for the test split, confusion matrix).
//
// zoom_linear_kernel: one lane per output pixel, all C channels.  scipy sizes nothing here (the host passes Ho, Wo); it places
// output index k at k * ((n_in - 1) / (n_out - 1)) in float64 and, in its default mode 'constant', treats a coordinate ABOVE
// n_in - 1 as outside: for some sizes the product of the last index rounds up, and the whole last row / column is zero
// (1024 rows at scale 0.75 is one).  That is reproduced, not repaired.  Weights t = cc - floor(cc), (1 - t, t); the float64 sum
// p00*wy0*wx0 + p01*wy0*wx1 + p10*wy1*wx0 + p11*wy1*wx1 in that order, each product left to right, one cast to fp32.  The
// mirrored copy (scale_image[:, :, :, ::-1]) is written by the same lane.
//
// seg_multiscale_kernel: one lane owns one pixel (Y, X) of the (H, W) output and walks the scale table in order.  Per scale it
// rebuilds the C up-sampled logits at (Y, X) of map 0 with the four-term expression of evaluate.hip (eval_dev.hpp) and, with a
// flipped forward, at (Y, W - 1 - X) of map 1; v = 0.5f * (a + b) in fp32; acc[c] += (double)v.  Same operations in the same
// order as the reference, so the float64 sums carry its bits, and no H x W x C array exists unless the probabilities are asked
// for.  Accumulators, class bounds, epilogue and histogram are those of evaluate_sliding.hip (eval_dev.hpp).
// The scale table lives in device memory: every lane reads the same row (scalar, cached loads).
// Floating-point contraction is OFF in this file, as in evaluate.hip and evaluate_sliding.hip.
#include "eval_dev.hpp"
#include "skd_eval_ms.h"

#pragma clang fp contract(off)

namespace skd {
namespace {

// one axis of the resize: source indices, weights, and whether the coordinate lies inside the input
struct ZoomAxis {
  int i0, i1;
  double w0, w1;
  bool inside;
};

__device__ __forceinline__ ZoomAxis zoom_axis(int k, int n_in, double step) {
  const double cc = (double)k * step;
  const double fl = floor(cc);
  ZoomAxis a;
  a.inside = cc <= (double)(n_in - 1);
  a.w1 = cc - fl;
  a.w0 = 1.0 - a.w1;
  int i = (int)fl;
  if (i > n_in - 1) i = n_in - 1;
  if (i < 0) i = 0;
  a.i0 = i;
  a.i1 = i < n_in - 1 ? i + 1 : i;
  return a;
}

__global__ __launch_bounds__(kThreads) void zoom_linear_kernel(const float *__restrict__ image, float *__restrict__ out, int C,
                                                              int H, int W, int Ho, int Wo, int mirror, int channels_last,
                                                              double step_y, double step_x) {
  const int64_t total = (int64_t)Ho * Wo;
  const int64_t hw = (int64_t)H * W;
  for (int64_t pix = (int64_t)blockIdx.x * kThreads + threadIdx.x; pix < total; pix += (int64_t)gridDim.x * kThreads) {
    const int xo = (int)(pix % Wo);
    const int yo = (int)(pix / Wo);
    const ZoomAxis ay = zoom_axis(yo, H, step_y), ax = zoom_axis(xo, W, step_x);
    const bool inside = ay.inside && ax.inside;
    const int64_t o00 = (int64_t)ay.i0 * W + ax.i0, o01 = (int64_t)ay.i0 * W + ax.i1;
    const int64_t o10 = (int64_t)ay.i1 * W + ax.i0, o11 = (int64_t)ay.i1 * W + ax.i1;
    const int64_t pix_m = (int64_t)yo * Wo + (Wo - 1 - xo);
    for (int c = 0; c < C; ++c) {
      const float *q = image + c * hw;
      float v = 0.f;
      if (inside)
        v = (float)((double)q[o00] * ay.w0 * ax.w0 + (double)q[o01] * ay.w0 * ax.w1 + (double)q[o10] * ay.w1 * ax.w0 +
                    (double)q[o11] * ay.w1 * ax.w1);
      if (channels_last) {
        out[pix * C + c] = v;
        if (mirror) out[(total + pix_m) * C + c] = v;
      } else {
        out[c * total + pix] = v;
        if (mirror) out[(C + c) * total + pix_m] = v;
      }
    }
  }
}

template <int CT>
__global__ __launch_bounds__(kThreads) void seg_multiscale_kernel(
    const float *__restrict__ logits, const int64_t *__restrict__ table, const int64_t *__restrict__ target,
    const unsigned char *__restrict__ remap, unsigned char *__restrict__ pred, double *__restrict__ probs,
    unsigned long long *__restrict__ confusion, int S, int F, int C, int H, int W, int ignore_index) {
  extern __shared__ unsigned int hist[];  // C * C
  hist_clear(hist, C);
  const int64_t total = (int64_t)H * W;
  const float dy = (float)(H - 1), dx = (float)(W - 1);
  for (int64_t pix = (int64_t)blockIdx.x * kThreads + threadIdx.x; pix < total; pix += (int64_t)gridDim.x * kThreads) {
    const int X = (int)(pix % W);
    const int Y = (int)(pix / W);
    double acc[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[c] = 0.0;
    for (int s = 0; s < S; ++s) {
      const int64_t off = table[3 * s + 0];
      // a map has at least one pixel and at most 2^31 - 1 per plane: the clamps of bilinear_at then keep every read inside it
      const int64_t h64 = table[3 * s + 1], w64 = table[3 * s + 2];
      const int h = h64 < 1 ? 1 : (h64 > INT32_MAX ? INT32_MAX : (int)h64);
      const int w = w64 < 1 ? 1 : ((int64_t)h * w64 > INT32_MAX ? INT32_MAX / h : (int)w64);
      const float sy = H > 1 ? (float)(h - 1) / dy : 0.f;
      const float sx = W > 1 ? (float)(w - 1) / dx : 0.f;
      const int64_t hw = (int64_t)h * w;
      const float *p = logits + off;
      const Bilinear a = bilinear_at(sy, sx, Y, X, h, w);
      if (F == 2) {
        const Bilinear b = bilinear_at(sy, sx, Y, W - 1 - X, h, w);  // the forward of the mirrored image, mirrored back
        const float *pm = p + (int64_t)C * hw;
#pragma unroll
        for (int c = 0; c < CT; ++c) {
          if (c < C) {
            const float v = 0.5f * (bilinear_value(a, p + c * hw) + bilinear_value(b, pm + c * hw));
            acc[c] += (double)v;
          }
        }
      } else {
#pragma unroll
        for (int c = 0; c < CT; ++c)
          if (c < C) acc[c] += (double)bilinear_value(a, p + c * hw);
      }
    }
    finish_pixel<CT>(acc, (double)S, C, pix, target, ignore_index, remap, pred, probs, hist);
  }
  hist_flush(hist, C, confusion);
}

}  // namespace
}  // namespace skd

using namespace skd;

extern "C" {

int skd_zoom_linear(int C, int H, int W, int Ho, int Wo, const float *image, float *out, int mirror, int channels_last,
                    skd_stream_t stream) {
  if (C <= 0 || H <= 0 || W <= 0 || Ho < 2 || Wo < 2 || !image || !out) return 0;
  const double step_y = (double)(H - 1) / (double)(Ho - 1), step_x = (double)(W - 1) / (double)(Wo - 1);
  int64_t wgs = cdiv((int64_t)Ho * Wo, (int64_t)kThreads);
  if (wgs > 8192) wgs = 8192;
  zoom_linear_kernel<<<dim3((unsigned)wgs), dim3(kThreads), 0, as_stream(stream)>>>(image, out, C, H, W, Ho, Wo, mirror ? 1 : 0,
                                                                                    channels_last ? 1 : 0, step_y, step_x);
  return ok();
}

int skd_seg_multiscale(int S, int F, int C, int H, int W, const float *logits, const int64_t *table, const int64_t *target,
                       int ignore_index, const uint8_t *remap, uint8_t *pred, double *probs, int64_t *confusion,
                       skd_stream_t stream) {
  if (S <= 0 || (F != 1 && F != 2) || C <= 0 || C > kMaxAccumClasses || H <= 0 || W <= 0) return 0;
  if (!logits || !table) return 0;
  if (target != nullptr && confusion == nullptr) return 0;
  const dim3 grid(accum_grid((int64_t)H * W)), block(kThreads);
  const size_t lds = sizeof(unsigned int) * C * C;
  unsigned long long *cm = reinterpret_cast<unsigned long long *>(confusion);
  hipStream_t st = as_stream(stream);
  with_class_bound(C, [&](auto ct) {
    seg_multiscale_kernel<decltype(ct)::value><<<grid, block, lds, st>>>(logits, table, target, remap, pred, probs, cm, S, F, C, H,
                                                                         W, ignore_index);
  });
  return ok();
}

}  // extern "C"
