// scale_word.hip -- the scale word of a gradient tensor (include/skd_train2h.h): word = max over all elements of
// bits(g) & 0x7fffffff as uint32, from which the fp16 two-piece training kernels (conv3x3.hip's SCALED form, conv3x3_wgrad.hip's
// FMT = kFp16) derive the power of two that puts g's largest magnitude into [2^14, 2^15) (scale_of, conv_split_dev.hpp).
// An integer maximum: independent of the order of evaluation, so two stages of plain maxima give the same word on every run --
// no atomics, no float compare (a NaN would lose every one), nothing to zero first.  Stage 1: each workgroup takes a contiguous
// slab of whole 16-byte quads (the last one the ragged tail too) and writes one partial; stage 2: one workgroup takes the
// partials.  A tensor one workgroup covers is one launch, straight into the word.
#include "skd_common.hpp"
#include "skd_train2h.h"

namespace skd {
namespace {

constexpr int kSlabQuads = 4 * kThreads;               // 16-byte loads per workgroup and trip: four in flight per lane
constexpr int64_t kMaxPartials = 1024;                 // stage 2 is one workgroup: four partials a lane

__device__ __forceinline__ uint32_t mag(uint32_t bits) { return bits & 0x7fffffffu; }
__device__ __forceinline__ uint32_t mag4(uint4 v) { return max(max(mag(v.x), mag(v.y)), max(mag(v.z), mag(v.w))); }

// The workgroup's maximum, valid in thread 0.
__device__ __forceinline__ uint32_t block_max(uint32_t m, uint32_t *red) {
#pragma unroll
  for (int s = kWave / 2; s > 0; s >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, s, kWave));
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = m;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kWavesPerWG; ++w) m = max(m, red[w]);
  return m;
}

// Elements [blockIdx.x * per_wg, + per_wg) of g, clipped to n; per_wg is a multiple of 4 and g 16-byte aligned, so every slab
// starts on a quad.  out[blockIdx.x] = the slab's maximum.
__global__ __launch_bounds__(kThreads) void scale_word_slab_kernel(const uint32_t *__restrict__ g, int64_t n, int64_t per_wg,
                                                                   uint32_t *__restrict__ out) {
  __shared__ uint32_t red[kWavesPerWG];
  const int64_t lo = (int64_t)blockIdx.x * per_wg;
  const int64_t hi = lo + per_wg < n ? lo + per_wg : n;
  const int64_t quads = (hi - lo) >> 2;
  const uint4 *q = reinterpret_cast<const uint4 *>(g + lo);
  uint32_t m = 0u;
  int64_t i = threadIdx.x;
  for (; i + 3 * kThreads < quads; i += kSlabQuads) {
    const uint4 a = q[i], b = q[i + kThreads], c = q[i + 2 * kThreads], d = q[i + 3 * kThreads];
    m = max(max(m, mag4(a)), max(max(mag4(b), mag4(c)), mag4(d)));
  }
  for (; i < quads; i += kThreads) m = max(m, mag4(q[i]));
  const int64_t tail = lo + 4 * quads + threadIdx.x;       // at most three elements, in the last slab alone
  if (tail < hi) m = max(m, mag(g[tail]));
  m = block_max(m, red);
  if (threadIdx.x == 0) out[blockIdx.x] = m;
}

__global__ __launch_bounds__(kThreads) void scale_word_final_kernel(const uint32_t *__restrict__ part, int count,
                                                                    uint32_t *__restrict__ word) {
  __shared__ uint32_t red[kWavesPerWG];
  uint32_t m = 0u;
  for (int i = threadIdx.x; i < count; i += kThreads) m = max(m, part[i]);
  m = block_max(m, red);
  if (threadIdx.x == 0) *word = m;
}

// Workgroups of stage 1 and the elements of a slab: slabs of at least 16 trips' worth, at most kMaxPartials of them.
void slabs(int64_t n, int64_t &wgs, int64_t &per_wg) {
  wgs = cdiv(n, (int64_t)16 * 4 * kSlabQuads);
  if (wgs > kMaxPartials) wgs = kMaxPartials;
  per_wg = cdiv(cdiv(n, wgs), 4) * 4;
  wgs = cdiv(n, per_wg);
}

}  // namespace
}  // namespace skd

using namespace skd;

extern "C" {

int64_t skd_fp16_scale_word_workspace_bytes(int64_t n) {
  if (n < 1) return 0;
  int64_t wgs, per_wg;
  slabs(n, wgs, per_wg);
  return wgs * (int64_t)sizeof(uint32_t);
}

int skd_fp16_scale_word(int64_t n, const float *g, void *workspace, int64_t workspace_bytes, uint32_t *word, skd_stream_t stream) {
  if (n < 1 || !g || !workspace || !word) return 0;
  if ((reinterpret_cast<uintptr_t>(g) & 15) || ((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(word)) & 3)) return 0;
  int64_t wgs, per_wg;
  slabs(n, wgs, per_wg);
  if (workspace_bytes < wgs * (int64_t)sizeof(uint32_t)) return 0;
  hipStream_t st = as_stream(stream);
  const uint32_t *bits = reinterpret_cast<const uint32_t *>(g);
  uint32_t *part = static_cast<uint32_t *>(workspace);
  if (wgs == 1) {
    scale_word_slab_kernel<<<dim3(1), dim3(kThreads), 0, st>>>(bits, n, per_wg, word);
    return ok();
  }
  scale_word_slab_kernel<<<dim3((unsigned)wgs), dim3(kThreads), 0, st>>>(bits, n, per_wg, part);
  if (!ok()) return 0;
  scale_word_final_kernel<<<dim3(1), dim3(kThreads), 0, st>>>(part, (int)wgs, word);
  return ok();
}

}  // extern "C"
