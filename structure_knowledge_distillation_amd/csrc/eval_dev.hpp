// eval_dev.hpp -- device code shared by the accumulating evaluation tails (evaluate_sliding.hip, evaluate_multiscale.hip):
// the fp32 align-corners interpolation of evaluate.hip as a (setup, value) pair, the per-pixel epilogue (float64 divide,
// first-maximum argmax, optional probabilities, optional id remap, per-workgroup LDS histogram) and the dispatch over the
// compile-time class bounds.  One definition, so that both kernels produce the same bits from the same inputs.
// Floating-point contraction is OFF from here to the end of the including file: individually rounded mul / add.
#pragma once
#include <type_traits>

#include "skd_common.hpp"

#pragma clang fp contract(off)

namespace skd {

constexpr int kMaxAccumClasses = 32;  // 2 VGPRs per class accumulator; the entry points refuse more

// upsample_bilinear2d, align_corners=True, at (y, x) of an (out_h, out_w) image over an (h, w) map: src = scale * dst;
// i0 = (int)src; i1 = i0 + (i0 < in - 1).  The clamps keep every offset inside the map whatever the caller's tables hold
// (h, w >= 1 is the caller's part).
struct Bilinear {
  int o00, o01, o10, o11;
  float ly0, ly1, lx0, lx1;
};

__device__ __forceinline__ Bilinear bilinear_at(float sy, float sx, int y, int x, int h, int w) {
  const float fy = sy * (float)y, fx = sx * (float)x;
  int y0 = (int)fy, x0 = (int)fx;
  if (y0 > h - 1) y0 = h - 1;
  if (x0 > w - 1) x0 = w - 1;
  const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
  Bilinear b;
  b.ly1 = fy - (float)y0;
  b.lx1 = fx - (float)x0;
  b.ly0 = 1.f - b.ly1;
  b.lx0 = 1.f - b.lx1;
  b.o00 = y0 * w + x0;
  b.o01 = y0 * w + x1;
  b.o10 = y1 * w + x0;
  b.o11 = y1 * w + x1;
  return b;
}

// the four-term expression on one class plane q
__device__ __forceinline__ float bilinear_value(const Bilinear &b, const float *__restrict__ q) {
  return b.ly0 * (b.lx0 * q[b.o00] + b.lx1 * q[b.o01]) + b.ly1 * (b.lx0 * q[b.o10] + b.lx1 * q[b.o11]);
}

__device__ __forceinline__ void hist_clear(unsigned int *hist, int C) {
  for (int i = threadIdx.x; i < C * C; i += kThreads) hist[i] = 0u;
  __syncthreads();
}

__device__ __forceinline__ void hist_flush(const unsigned int *hist, int C, unsigned long long *__restrict__ confusion) {
  __syncthreads();
  if (confusion != nullptr)
    for (int i = threadIdx.x; i < C * C; i += kThreads)
      if (hist[i] != 0u) atomicAdd(&confusion[i], (unsigned long long)hist[i]);
}

// acc[c] / n -> probabilities; first maximum wins (numpy argmax; a NaN never replaces the running maximum); `remap` goes on the
// WRITTEN prediction only, the histogram takes the un-remapped one over target != ignore_index && 0 <= target < C.
template <int CT>
__device__ __forceinline__ void finish_pixel(double (&acc)[CT], double n, int C, int64_t pix, const int64_t *__restrict__ target,
                                             int ignore_index, const unsigned char *__restrict__ remap,
                                             unsigned char *__restrict__ pred, double *__restrict__ probs, unsigned int *hist) {
  double best = 0.0;
  int arg = 0;
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    if (c < C) {
      acc[c] = acc[c] / n;
      if (c == 0 || acc[c] > best) {
        best = acc[c];
        arg = c;
      }
    }
  }
  if (probs != nullptr) {
    double *o = probs + pix * C;
#pragma unroll
    for (int c = 0; c < CT; ++c)
      if (c < C) o[c] = acc[c];
  }
  if (pred != nullptr) pred[pix] = remap != nullptr ? remap[arg] : (unsigned char)arg;
  if (target != nullptr) {
    const int64_t g = target[pix];
    if (g != (int64_t)ignore_index && g >= 0 && g < C) atomicAdd(&hist[(int)g * C + arg], 1u);
  }
}

// f(std::integral_constant<int, CT>) with the smallest compile-time bound CT >= C of (8, 16, 19, 21, 32); 1 <= C <= 32
template <class F>
static inline void with_class_bound(int C, F f) {
  if (C <= 8)
    f(std::integral_constant<int, 8>());
  else if (C <= 16)
    f(std::integral_constant<int, 16>());
  else if (C <= 19)
    f(std::integral_constant<int, 19>());
  else if (C <= 21)
    f(std::integral_constant<int, 21>());
  else
    f(std::integral_constant<int, 32>());
}

// ~4 pixels per lane: one histogram flush per 1024 pixels
static inline unsigned accum_grid(int64_t total) {
  int64_t wgs = cdiv(total, (int64_t)kThreads * 4);
  if (wgs < 1) wgs = 1;
  if (wgs > 8192) wgs = 8192;
  return (unsigned)wgs;
}

}  // namespace skd
