// conv3x3_narrow.hip -- the 64-column form of the split-core 3x3 convolution of conv3x3.hip: the same implicit GEMM
//     Y[m][n] = epi( sum_{tap, c} X[pixel(m) + shift(tap)][c] * W[n][c][tap] ),   k = tap * Cin + c,
// for output tiles 128 pixels x 64 channels, so that Cout (and, for the data gradient, Cin) need only be a multiple of 64: the
// student's stem conv2 (64 -> 64), the data gradient of its conv3 (64 -> 128) and the four convolutions of layer1.
//
// The core is conv_split_dev.hpp's, unchanged: split4 / split_store, the kPlaneChunks image of the activations with its XOR
// swizzle, k_loop<2>, store_block.  What differs from conv3x3_tile is the assignment of output elements to waves -- waves 4 x 1,
// each owning 32 pixels x 64 channels = 1 x 2 blocks of 32 x 32, the wave tile of conv3x3.hip's 64-row form -- and the B image,
// which has 64 rows per plane.  narrow_mma keeps tile_mma's arithmetic: v_mfma_f32_32x32x16_bf16, the six products in the order
// kPA / kPB, five into `low` and a0 b0 into `acc`, added in the epilogue, K-tiles in the order k = tap * Cin + c.  Every output
// element therefore sees the operations of the wide kernel in the same order, and at a Cout that both kernels take the two give
// the same bits (tests/test_conv3x3_narrow_gpu.py).
//
// Weight image: per column tile of 64 output channels and K-tile of 16 k, three bf16 planes of 64 rows,
//   chunk(h, row) = h * 64 + (row ^ 4 h),   h = k / 8,
// 384 chunks of 16 bytes = 6,144 bytes, still 6 bytes per weight.  256 threads copy 384 chunks: every thread one, the first two
// waves a second one (uniform per wave).
//
// LDS: a stage is the 768 chunks of the A operand and the 384 of B; k_loop places its second stage kStageChunks behind the
// first, so the launch asks for (kStageChunks + 1152) * 16 = 43,008 bytes.  The register budget (two accumulator sets of 32 each,
// two staging sets) admits three workgroups per CU, which 43 KB each allow as well.
#include "conv_split_dev.hpp"
#include "skd_narrow.h"

namespace skd {
namespace {

constexpr int kNarrowTN = 64;                                       // output channels per tile
constexpr int kNarrowPlane = 2 * kNarrowTN;                         // chunks of one piece of the B operand
constexpr int kNarrowTile = 3 * kNarrowPlane;                       // one (column tile, K-tile) of packed weights: 384 chunks
constexpr int kNarrowRA = kTM / kRPP;                               // float4 of the A panel per thread and K-tile (2)
constexpr size_t kNarrowLds = sizeof(uint4) * (kStageChunks + kOperandChunks + kNarrowTile);
static_assert(kNarrowTile > kThreads && kNarrowTile <= 2 * kThreads, "one chunk per thread, a second for the first threads");

struct NarrowStaging {
  float4 a[kNarrowRA];
  uint4 b[2];
};

__device__ __forceinline__ int64_t narrow_tap_shift(int tap, int W, int dil, int Cin) {
  const int ty = tap / 3, tx = tap - 3 * ty;
  return ((int64_t)(ty - 1) * W + (tx - 1)) * dil * Cin;
}

// One K-tile out of LDS: tile_mma (conv_split_dev.hpp) for waves 4 x 1 and a B image of 64 rows.
__device__ __forceinline__ void narrow_mma(const uint4 *stage, f32x16 (&lo)[2], f32x16 (&hi)[2]) {
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  const int half = lane >> 5, r = lane & 31;
  const uint4 *pa = stage + half * 128 + ((wid * 32 + r) ^ (half * 4));
  const uint4 *pb = stage + kOperandChunks + half * kNarrowTN + (r ^ (half * 4));
  bf16x8 a[3], b[2][3];
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    a[p] = __builtin_bit_cast(bf16x8, pa[p * kPlaneChunks]);
#pragma unroll
    for (int j = 0; j < 2; ++j) b[j][p] = __builtin_bit_cast(bf16x8, pb[p * kNarrowPlane + 32 * j]);
  }
  constexpr int kPA[6] = {0, 1, 2, 0, 1, 0}, kPB[6] = {2, 1, 0, 1, 0, 0};
#pragma unroll
  for (int t = 0; t < 6; ++t)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      f32x16 &dst = t < 5 ? lo[j] : hi[j];
      dst = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[kPA[t]], b[j][kPB[t]], dst, 0, 0, 0);
    }
}

// What k_loop needs of a tile (see Tile3 of conv3x3.hip): the cursor is stepped behind every load.
struct NarrowTile {
  typedef NarrowStaging Stg;
  const float *__restrict__ X;
  const uint4 *__restrict__ bsrc;
  int srow, W, dil, Cin;
  int tap, c0;
  int64_t shift;
  int64_t abase[kNarrowRA];
  unsigned mask[kNarrowRA];
  f32x16 (&low)[2], (&acc)[2];
  __device__ __forceinline__ void load(Stg &s, int kt) {
    // the activations: a lane whose tap is outside the image issues no load and stages an exact zero
#pragma unroll
    for (int h = 0; h < kNarrowRA; ++h) {
      s.a[h] = make_float4(0.f, 0.f, 0.f, 0.f);
      if ((mask[h] >> tap) & 1u) s.a[h] = *reinterpret_cast<const float4 *>(X + abase[h] + shift + c0);
    }
    // the packed weights: chunk t, and chunk 256 + t for the first 128 threads
    const uint4 *src = bsrc + (int64_t)kt * kNarrowTile;
    s.b[0] = src[0];
    s.b[1] = make_uint4(0u, 0u, 0u, 0u);
    if (threadIdx.x < kNarrowTile - kThreads) s.b[1] = src[kThreads];
    c0 += kBK;
    if (c0 == Cin) {
      c0 = 0;
      ++tap;
      shift = narrow_tap_shift(tap, W, dil, Cin);
    }
  }
  __device__ __forceinline__ void store(const Stg &s, uint4 *stage, int) const {
    uint2 *sa = reinterpret_cast<uint2 *>(stage) + srow;
#pragma unroll
    for (int h = 0; h < kNarrowRA; ++h) split_store(s.a[h], sa + 2 * kRPP * h);
    uint4 *sb = stage + kOperandChunks + threadIdx.x;
    sb[0] = s.b[0];
    if (threadIdx.x < kNarrowTile - kThreads) sb[kThreads] = s.b[1];
  }
  __device__ __forceinline__ void mma(const uint4 *stage) const { narrow_mma(stage, low, acc); }
};

// One output tile of 128 pixels x 64 channels per workgroup; three workgroups per CU.
template <int ACT, bool HAS_RES>
__global__ __launch_bounds__(kThreads, kMinWG) __attribute__((amdgpu_waves_per_eu(kMinWG, kMinWG)))
void conv3x3_narrow_kernel(
    const float *__restrict__ X, const uint4 *__restrict__ Bp, float *__restrict__ Y, const float *__restrict__ cbias,
    const float *__restrict__ mean, const float *__restrict__ var, const float *__restrict__ weight,
    const float *__restrict__ bias, float eps, float slope, int64_t M, int H, int W, int Cin, int N, int dil, int tiles_n,
    const float *__restrict__ R) {
  extern __shared__ __attribute__((aligned(16))) uint4 lds[];
  // XCD-aware panel-major order (conv3x3.hip): row panel p lives on XCD p % 8, its column tiles run back to back
  const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
  const int pl = j / tiles_n, tn = j - pl * tiles_n;
  const int64_t m0 = ((int64_t)pl * 8 + xcd) * kTM;
  if (m0 >= M) return;
  f32x16 acc[2], low[2];
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[b][q] = low[b][q] = 0.f;
  const int nk = 9 * (Cin / kBK);
  const int gt = threadIdx.x, grow = gt / kQK, gkq = (gt % kQK) * 4;
  NarrowTile tile = {X, Bp + (int64_t)tn * nk * kNarrowTile + gt, plane_slot(grow, gkq), W, dil, Cin, 0, 0,
                     narrow_tap_shift(0, W, dil, Cin), {}, {}, low, acc};
  // this thread's panel rows: address of (pixel, channel quad) and the taps that stay inside the image; a row beyond M has none
  const int64_t hw = (int64_t)H * W;
#pragma unroll
  for (int h = 0; h < kNarrowRA; ++h) {
    const int64_t m = m0 + grow + kRPP * h;
    const bool live = m < M;
    const int64_t mm = live ? m : 0;
    const int pix = (int)(mm % hw);
    const int py = pix / W, px = pix - py * W;
    unsigned bits = 0;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int64_t y = py + (int64_t)(tap / 3 - 1) * dil, x = px + (int64_t)(tap % 3 - 1) * dil;
      if (live && y >= 0 && y < H && x >= 0 && x < W) bits |= 1u << tap;
    }
    tile.mask[h] = bits;
    tile.abase[h] = mm * Cin + gkq;
  }
  k_loop<2>(tile, nk, lds);
  // ---- epilogue: (+ conv bias) -> eval-mode InPlace-ABN formula (when there are statistics) -> (+ residual) -> activation ----
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  const int64_t row0 = m0 + wid * 32;
  const bool full = m0 + kTM <= M;
#pragma unroll
  for (int bj = 0; bj < 2; ++bj) {
    const int col = tn * kNarrowTN + bj * 32 + (lane & 31);
    const bool bn = mean != nullptr;
    const float mu = bn ? mean[col] : 0.f, is = bn ? inv_std_of(var[col], eps) : 1.f;
    const float ga = bn && weight != nullptr ? fabsf(weight[col]) + eps : 1.f;
    const float be = bn && bias != nullptr ? bias[col] : 0.f;
    const float cb = cbias != nullptr ? cbias[col] : 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[bj][q] += low[bj][q];
    if (cbias != nullptr) {
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[bj][q] += cb;
    }
    if (full)
      store_block<ACT, HAS_RES, true, false>(acc[bj], R, Y, row0, col, M, N, mu, is, ga, be, slope);
    else
      store_block<ACT, HAS_RES, false, false>(acc[bj], R, Y, row0, col, M, N, mu, is, ga, be, slope);
  }
}

// The weight split for 64-row tiles: conv3x3_pack_pair_kernel (conv3x3.hip) with kNarrowPlane threads per (column tile, K-tile),
// one per 16-byte chunk.  The first `fwd_tiles` workgroups write the image of W (Cout, Cin, 3, 3), the others the image of
// Wd[c][n][ty][tx] = W[n][c][2 - ty][2 - tx]; both read W through its strides in elements.
__global__ __launch_bounds__(kNarrowPlane) void conv3x3_narrow_pack_pair_kernel(
    const float *__restrict__ Wt, int64_t sn, int64_t sc, int64_t sy, int64_t sx, int Cin, int Cout, int64_t fwd_tiles,
    uint4 *__restrict__ pack_fwd, uint4 *__restrict__ pack_bwd) {
  const int chunk = threadIdx.x;
  const int kh = chunk / kNarrowTN, row = (chunk % kNarrowTN) ^ (kh * 4);
  const bool fwd = (int64_t)blockIdx.x < fwd_tiles;
  const int64_t tile = fwd ? (int64_t)blockIdx.x : (int64_t)blockIdx.x - fwd_tiles;      // = column tile * nk + kt
  const int K9 = fwd ? Cin : Cout;                                                      // channels per tap of this image's K
  const int nk = 9 * (K9 / kBK);
  const int kt = (int)(tile % nk), tn = (int)(tile / nk);
  const int k0 = kt * kBK + kh * 8, tap = k0 / K9, e0 = k0 - tap * K9;
  const int ty = fwd ? tap / 3 : 2 - tap / 3, tx = fwd ? tap % 3 : 2 - tap % 3;         // backward: the flipped tap
  const int64_t srow = fwd ? sn : sc, sk = fwd ? sc : sn;                               // backward: rows are c, k runs over n
  const float *src = Wt + (int64_t)(tn * kNarrowTN + row) * srow + ty * sy + tx * sx;
  float v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = src[(e0 + i) * sk];
  uint2 lo[3], hi[3];
  split4(make_float4(v[0], v[1], v[2], v[3]), lo[0], lo[1], lo[2]);
  split4(make_float4(v[4], v[5], v[6], v[7]), hi[0], hi[1], hi[2]);
  uint4 *pack = fwd ? pack_fwd : pack_bwd;
#pragma unroll
  for (int p = 0; p < 3; ++p) pack[(tile * 3 + p) * kNarrowPlane + chunk] = make_uint4(lo[p].x, lo[p].y, hi[p].x, hi[p].y);
}

template <int ACT, bool HAS_RES>
static int launch_narrow(const float *X, const uint4 *Bp, float *Y, const float *R, const float *cbias, const float *mean,
                         const float *var, const float *weight, const float *bias, float eps, float slope, int64_t M, int H, int W,
                         int Cin, int N, int dil, hipStream_t st) {
  static PerDeviceFlag ready;          // per instantiation AND per device
  bool *rdy = ready.get();
  if (rdy == nullptr) return 0;
  if (!*rdy) {
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(conv3x3_narrow_kernel<ACT, HAS_RES>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)kNarrowLds) != hipSuccess) return 0;
    *rdy = true;
  }
  const int tiles_n = N / kNarrowTN;
  const int64_t grid = cdiv(cdiv(M, kTM), 8) * 8 * tiles_n;
  if (grid > 2147483647) return 0;
  conv3x3_narrow_kernel<ACT, HAS_RES><<<dim3((unsigned)grid), dim3(kThreads), kNarrowLds, st>>>(
      X, Bp, Y, cbias, mean, var, weight, bias, eps, slope, M, H, W, Cin, N, dil, tiles_n, R);
  return ok();
}

// The (column tile, K-tile) count of the image of an (N, K / 9, 3, 3) weight in `pack`, 0 for no image (pack == nullptr), -1
// for an image that is refused: a direction the kernel does not take, a buffer too small or not 16-byte aligned.
static int64_t narrow_image_tiles(int K9, int N, const void *pack, int64_t pack_bytes) {
  if (!pack) return 0;
  const int64_t need = skd_conv3x3_narrow_pack_bytes(K9, N);
  if (need == 0 || pack_bytes < need || (reinterpret_cast<uintptr_t>(pack) & 15)) return -1;
  return (int64_t)(N / kNarrowTN) * (9 * (K9 / kBK));
}

}  // namespace
}  // namespace skd

using namespace skd;

extern "C" {

int skd_conv3x3_narrow_supported(int Cin, int Cout, int stride, int padding, int dilation, int groups) {
  return Cin > 0 && Cout > 0 && Cin % kBK == 0 && Cout % kNarrowTN == 0 && stride == 1 && dilation >= 1 && padding == dilation &&
         groups == 1;
}

int64_t skd_conv3x3_narrow_pack_bytes(int Cin, int Cout) {
  if (!skd_conv3x3_narrow_supported(Cin, Cout, 1, 1, 1, 1)) return 0;
  return (int64_t)(Cout / kNarrowTN) * (9 * (Cin / kBK)) * kNarrowTile * (int64_t)sizeof(uint4);
}

// Either image or both in one launch; every refusal is decided here, in front of the launch.
int skd_conv3x3_narrow_pack_pair(int Cin, int Cout, const float *w, int64_t stride_n, int64_t stride_c, int64_t stride_y,
                                 int64_t stride_x, void *pack_fwd, int64_t fwd_bytes, void *pack_bwd, int64_t bwd_bytes,
                                 skd_stream_t stream) {
  if (!w || (!pack_fwd && !pack_bwd)) return 0;
  if (stride_n < 0 || stride_c < 0 || stride_y < 0 || stride_x < 0) return 0;
  const int64_t fwd_tiles = narrow_image_tiles(Cin, Cout, pack_fwd, fwd_bytes);
  const int64_t bwd_tiles = narrow_image_tiles(Cout, Cin, pack_bwd, bwd_bytes);
  if (fwd_tiles < 0 || bwd_tiles < 0 || fwd_tiles + bwd_tiles > 2147483647) return 0;
  conv3x3_narrow_pack_pair_kernel<<<dim3((unsigned)(fwd_tiles + bwd_tiles)), dim3(kNarrowPlane), 0, as_stream(stream)>>>(
      w, stride_n, stride_c, stride_y, stride_x, Cin, Cout, fwd_tiles, static_cast<uint4 *>(pack_fwd),
      static_cast<uint4 *>(pack_bwd));
  return ok();
}

// out = act(ABN_eval(conv3x3(x) + conv_bias) [+ residual]).  The kernel reads the residual through a __restrict__ pointer at
// the offsets it writes, so a residual that overlaps the output is refused, not defined.
int skd_conv3x3_narrow_nhwc(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const void *wpack, float *out,
                            const float *residual, const float *conv_bias, const float *mean, const float *var,
                            const float *weight, const float *bias, float eps, int activation, float slope, int geometry,
                            skd_stream_t stream) {
  if (!skd_conv3x3_narrow_supported(Cin, Cout, 1, dilation, dilation, 1) || B < 1 || H < 1 || W < 1) return 0;
  if (!x || !wpack || !out || (mean == nullptr) != (var == nullptr) || geometry < 0 || geometry > 1) return 0;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(wpack)) & 15) return 0;
  if ((int64_t)H * W > 2147483647 || dilation > (1 << 24)) return 0;
  const int64_t M = (int64_t)B * H * W;
  if (residual != nullptr) {
    const uintptr_t bytes = (uintptr_t)M * Cout * sizeof(float);
    const uintptr_t r = reinterpret_cast<uintptr_t>(residual), o = reinterpret_cast<uintptr_t>(out);
    if (r < o + bytes && o < r + bytes) return 0;
  }
  hipStream_t st = as_stream(stream);
  const uint4 *bp = static_cast<const uint4 *>(wpack);
#define SKD_CONV3X3_NARROW_CASE(ACT)                                                                                          \
  case ACT:                                                                                                                   \
    return (residual != nullptr ? launch_narrow<ACT, true> : launch_narrow<ACT, false>)(                                     \
        x, bp, out, residual, conv_bias, mean, var, weight, bias, eps, slope, M, H, W, Cin, Cout, dilation, st)
  switch (activation) {
    SKD_CONV3X3_NARROW_CASE(SKD_ACT_NONE);
    SKD_CONV3X3_NARROW_CASE(SKD_ACT_RELU);
    SKD_CONV3X3_NARROW_CASE(SKD_ACT_LEAKY_RELU);
    default: return 0;
  }
#undef SKD_CONV3X3_NARROW_CASE
}

}  // extern "C"
