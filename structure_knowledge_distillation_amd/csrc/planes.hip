// planes.hip -- piece planes (include/skd_planes.h): an (M, C) fp32 channels-last activation map stored as the three bf16
// pieces of the split core, p0 = bf16(v), p1 = bf16(v - p0), p2 = bf16(v - p0 - p1) (split4, conv_split_dev.hpp), in the layout of
// planes_offset (the same header: one function for these kernels, the producer's epilogue in conv1x1.hip, the consumer's loader
// in conv3x3.hip and the host entry below).
//
// Here: the three host-only entries (predicate, size, offset map) and the two streaming kernels -- fp32 -> planes for a map no
// producer wrote (and for the tests, which feed the consumer without the producer), planes -> fp32 as a test and debugging aid.
// One thread per quad of four consecutive channels of one row: a 16-byte load and three 8-byte stores (or the reverse), 24
// contiguous bytes in the committed layout.  HBM-bound: 4 + 6 bytes per element.
#include "conv_split_dev.hpp"
#include "skd_planes.h"

namespace skd {
namespace {

constexpr int64_t kMaxQuads = (int64_t)2147483647 * kThreads;      // the grid is one thread per quad

__global__ __launch_bounds__(kThreads) void planes_split_kernel(const float *__restrict__ X, unsigned char *__restrict__ P, int64_t M,
                                                                int C) {
  const int64_t quad = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int qpr = C >> 2;                                            // quads per row
  const int64_t row = quad / qpr;
  if (row >= M) return;
  const int c = (int)(quad - row * qpr) * 4;
  uint2 p[3];
  split4(*reinterpret_cast<const float4 *>(X + quad * 4), p[0], p[1], p[2]);
#pragma unroll
  for (int i = 0; i < 3; ++i) *reinterpret_cast<uint2 *>(P + planes_offset(M, C, row, c, i)) = p[i];
}

// (p0 + p1) + p2, exact for the pieces of a value they can carry.  A zero sum takes p0's sign: the pieces of -0.0 are -0, +0, +0
// (v - p0 is +0) and their sum +0, so without this the one value that would not come back bit for bit is -0.0.
__device__ __forceinline__ float join3(float p0, float p1, float p2) {
  const float r = (p0 + p1) + p2;
  return r == 0.f ? p0 : r;
}

__global__ __launch_bounds__(kThreads) void planes_join_kernel(const unsigned char *__restrict__ P, float *__restrict__ X, int64_t M,
                                                               int C) {
  const int64_t quad = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int qpr = C >> 2;
  const int64_t row = quad / qpr;
  if (row >= M) return;
  const int c = (int)(quad - row * qpr) * 4;
  uint2 p[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) p[i] = *reinterpret_cast<const uint2 *>(P + planes_offset(M, C, row, c, i));
  float4 v;
  v.x = join3(bf16_lo(p[0].x), bf16_lo(p[1].x), bf16_lo(p[2].x));
  v.y = join3(bf16_hi(p[0].x), bf16_hi(p[1].x), bf16_hi(p[2].x));
  v.z = join3(bf16_lo(p[0].y), bf16_lo(p[1].y), bf16_lo(p[2].y));
  v.w = join3(bf16_hi(p[0].y), bf16_hi(p[1].y), bf16_hi(p[2].y));
  *reinterpret_cast<float4 *>(X + quad * 4) = v;
}

static bool sizes_ok(int64_t M, int C) { return M >= 1 && C >= 1 && C % kBK == 0 && M <= ((int64_t)1 << 40) && M * (C / 4) <= kMaxQuads; }

}  // namespace
}  // namespace skd

using namespace skd;

extern "C" {

int skd_planes_supported(int C) { return C >= 1 && C % kBK == 0; }

int skd_planes_bytes(int64_t M, int C, int64_t *bytes) {
  if (!sizes_ok(M, C) || !bytes) return 0;
  *bytes = planes_bytes(M, C);
  return 1;
}

int skd_planes_offset(int64_t M, int C, int64_t row, int channel, int piece, int64_t *byte_offset) {
  if (!sizes_ok(M, C) || !byte_offset || row < 0 || row >= M || channel < 0 || channel >= C || piece < 0 || piece > 2) return 0;
  *byte_offset = planes_offset(M, C, row, channel, piece);
  return 1;
}

int skd_planes_split_nhwc(int64_t M, int C, const float *x, void *planes, skd_stream_t stream) {
  if (!sizes_ok(M, C) || !x || !planes) return 0;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(planes)) & 15) return 0;
  planes_split_kernel<<<dim3((unsigned)cdiv(M * (C / 4), kThreads)), dim3(kThreads), 0, as_stream(stream)>>>(
      x, static_cast<unsigned char *>(planes), M, C);
  return ok();
}

int skd_planes_join_nhwc(int64_t M, int C, const void *planes, float *x, skd_stream_t stream) {
  if (!sizes_ok(M, C) || !x || !planes) return 0;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(planes)) & 15) return 0;
  planes_join_kernel<<<dim3((unsigned)cdiv(M * (C / 4), kThreads)), dim3(kThreads), 0, as_stream(stream)>>>(
      static_cast<const unsigned char *>(planes), x, M, C);
  return ok();
}

}  // extern "C"
