// conv3x3.hip -- 3x3, stride-1 (frozen forwards: stride-2 too, STRIDE below), "same" (padding = dilation) convolution as an IMPLICIT GEMM on the split-operand bf16-MFMA core
// of conv_split_dev.hpp (see conv1x1.hip for the core): fp32 in, fp32 out.
//
//     Y[m][n] = epi( sum_{tap, c} X[pixel(m) + shift(tap)][c] * W[n][c][tap] ),   M = B*H*W output pixels (channels-last),
//     N = Cout, K = 9 * Cin with k = tap * Cin + c, tap = 3 ty + tx, shift = ((ty - 1) * W + (tx - 1)) * dilation pixels.
// A tap that falls outside the image contributes an exact zero: the load is not issued, the staging register is set to 0.
// M is the flattened pixel index, so a tile's rows cross image rows and images freely; every thread works out (h, w) of the
// one or two panel rows it owns once per tile and keeps a 9-bit validity mask per row.
//
// Why: the teacher's 3x3 convolutions were MIOpen implicit-GEMM kernels on v_mfma_f32_32x32x2_f32 at 0.79-0.87 of that pipe's
// peak (profiles/r06w_conv_shapes.md); the pipe is the limit, and six bf16 MFMAs per 16 k take 2.67 x less matrix-pipe time than
// eight fp32 ones (conv1x1.hip).
//
// ONE kernel family with the column-tile width TN as a template parameter: TN = 128 output channels per tile (include/skd_eval.h,
// skd_infer.h, skd_train.h: the frozen teacher, the student's wide layers) and TN = 64 (include/skd_narrow.h: the student's stem
// conv2, layer1 and the data gradient of conv3, whose N is a multiple of 64 only).  TN sets the wave map and the B image
// (tile_mma) and nothing else: taps, masks, K loop, product order and epilogue are the same code, so every output element sees
// the same operations in the same order and at a Cout both forms take they give the same bits (tests/test_conv3x3_narrow_gpu.py).
//
// Weights are split ONCE per weight version (once for a frozen network): conv3x3_pack_pair_kernel writes, per column tile of TN
// output channels and per K-tile of 16 k, the three bf16 planes in exactly the LDS image of the core -- chunk(h, row) = h * TN +
// (row ^ 4 h), 6 TN chunks of 16 bytes (768 or 384).  The main loop's B stage is then three (TN = 64: one, and a second for the
// first two waves) 16-byte global loads and ds_write_b128 per thread: no VALU work.  The split is a pure function of the fp32
// value, so the result equals splitting in the loop bit for bit.  Activations are split on their way into LDS as in the 1x1
// kernel (each element nine times, once per tap).
//
// Epilogue (store_block): out = act( ((acc + conv_bias - mean) * invstd) * (|weight| + eps) + bias [+ residual] ), every term
// optional: the identity (raw convolution output: the PSP bottleneck's `feats` half, the bottleneck blocks' conv2), conv bias +
// eval-mode InPlace-ABN + leaky ReLU (the deep-supervision head), eval-mode BN + ReLU, BN + residual + ReLU (a BasicBlock's tail).
// STATS (include/skd_bnstats.h; the raw epilogue of the training forward alone): behind its stores a block also writes the
// batch-norm statistics record of what it stored (block_stats); STATS = false is the code without it.
//
// Grid: XCD-aware panel-major order as in conv1x1.hip -- row panel p lives on XCD p % 8, its column tiles run back to back --
// so the workgroups resident on an XCD together started together and walk the same K-tiles of the same (at most Cout / TN)
// weight panels at about the same time: a weight slice is fetched into that L2 once per wave of workgroups, not once per tile.
// Two accumulator sets (tile_mma).  TN = 128 has two kernels, chosen per launch by launch3g: the TALL one runs 128 x 128 output
// tiles for the launch's whole rounds and 64 x 128 tiles for the last, partial round, all at two workgroups per CU (one kernel, one
// register budget); the other runs 64 x 128 tiles throughout at three workgroups per CU and takes the problems that do not fill
// the chip's two-per-CU slots once.  48 KB of LDS either way.  TN = 64 runs 128 x 64 tiles throughout: two accumulator sets of 32
// registers each and 42 KB of LDS (a stage is the 768 chunks of A and the 384 of B; k_loop places its second stage kStageChunks
// behind the first) admit three workgroups per CU.
#include "conv_split_dev.hpp"
#include "skd_bnstats.h"
#include "skd_infer.h"
#include "skd_infer2h.h"
#include "skd_narrow.h"
#include "skd_planes.h"
#include "skd_split2.h"
#include "skd_split2h.h"
#include "skd_stride2.h"
#include "skd_train.h"
#include "skd_train2.h"
#include "skd_train2h.h"

namespace skd {
namespace {

constexpr int kDepth3x3 = 2;                          // K-tiles of load look-ahead (k_loop, conv_split_dev.hpp)
constexpr int kNarrowTN = 64;                         // the column tile of include/skd_narrow.h; kTN = 128 is the others'
// One (column tile, K-tile) of packed weights, in chunks: 768 = 12,288 bytes, or 384.  Thread t copies chunks t + i * kThreads.
// PIECES (conv_split_dev.hpp) = 2: the two-plane image of include/skd_split2.h, 512 chunks = 8,192 bytes at TN = 128 -- two
// copies per thread.
constexpr int tile_chunks(int TN, int PIECES = 3) { return PIECES * 2 * TN; }
constexpr int b_copies(int TN, int PIECES = 3) { return (tile_chunks(TN, PIECES) + kThreads - 1) / kThreads; }
// Whether thread t's copy i exists: a constant for every copy but the last of TN = 64 (t < 128: uniform per wave).
template <int TN, int PIECES = 3>
__device__ __forceinline__ bool b_copy_live(int i) {
  return (i + 1) * kThreads <= tile_chunks(TN, PIECES) || (int)threadIdx.x < tile_chunks(TN, PIECES) - i * kThreads;
}
constexpr size_t conv3x3_lds(int TN, int PIECES = 3) {
  return sizeof(uint4) * (stage_chunks(PIECES) + operand_chunks(PIECES) + tile_chunks(TN, PIECES));
}
static_assert(conv3x3_lds(kTN) == kConvLds, "the 128-column form fills both stages");
static_assert(conv3x3_lds(kTN, 2) == conv_lds(2) && tile_chunks(kTN, 2) == 2 * kThreads, "... of two pieces too: 32 KB, two copies");

// One panel row's four k of a K-tile in the staging registers: the fp32 quad that stage_store3 splits, or -- PLANES
// (include/skd_planes.h): the activation is the piece planes of the map -- its three 8-byte piece quads, ready to store: two
// registers more per panel row and staging set, four per 64 rows of the tile over k_loop's two sets.
// (Native vector types, one array per piece: with HIP's uint2 / uint4 structs in this set the copies of the first weight chunk
// stayed memcpys and the set in scratch, 56 bytes per lane.)
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
template <int TM, int TN, int PIECES = 3, bool PLANES = false>
struct Staging3 {
  float4 a[TM / kRPP];
  uint4 b[b_copies(TN, PIECES)];
};
template <int TM, int TN, int PIECES>
struct Staging3<TM, TN, PIECES, true> {
  u32x2 a0[TM / kRPP], a1[TM / kRPP], a2[TM / kRPP];
  u32x4 b[b_copies(TN, PIECES)];
};

struct TapCursor {      // the K-tile being staged: tap 0..8, first channel c0, and the tap's address shift in floats
  int tap, c0;
  int64_t shift;
};

__device__ __forceinline__ int64_t tap_shift(int tap, int W, int dil, int Cin) {
  const int ty = tap / 3, tx = tap - 3 * ty;
  return ((int64_t)(ty - 1) * W + (tx - 1)) * dil * Cin;
}

// The packed weights: every lane loads its chunks (a copy that does not exist stages zeros, which nothing stores).
template <int TM, int TN, int PIECES, bool PLANES>
__device__ __forceinline__ void stage_load3_b(Staging3<TM, TN, PIECES, PLANES> &s, const uint4 *__restrict__ bsrc) {
#pragma unroll
  for (int i = 0; i < b_copies(TN, PIECES); ++i) {
    if constexpr (PLANES) {
      s.b[i] = u32x4{0u, 0u, 0u, 0u};
      if (b_copy_live<TN, PIECES>(i)) s.b[i] = reinterpret_cast<const u32x4 *>(bsrc)[i * kThreads];
    } else {
      s.b[i] = make_uint4(0u, 0u, 0u, 0u);
      if (b_copy_live<TN, PIECES>(i)) s.b[i] = bsrc[i * kThreads];
    }
  }
}
// The activations: a lane whose tap is outside the image issues no load and stages an exact zero.
template <int TM, int TN, int PIECES>
__device__ __forceinline__ void stage_load3_a(Staging3<TM, TN, PIECES, false> &s, const float *__restrict__ X, const TapCursor &cur,
                                              const int64_t (&abase)[TM / kRPP], const unsigned (&mask)[TM / kRPP], int) {
#pragma unroll
  for (int h = 0; h < TM / kRPP; ++h) {
    s.a[h] = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((mask[h] >> cur.tap) & 1u) s.a[h] = *reinterpret_cast<const float4 *>(X + abase[h] + cur.shift + cur.c0);
  }
}
// PLANES: X is the piece planes, abase[h] the BYTE offset of (the row's pixel, the thread's k quad, piece 0) and the cursor's
// shift + c0 -- a multiple of 16 channels, negative for the upper taps -- goes through planes_offset as the channel: the map is
// affine in it (conv_split_dev.hpp).  Three 8-byte loads in the source, adjacent in the committed layout (the compiler issues a
// 16-byte and an 8-byte one); a masked tap stages zeros in all three pieces, which is what split4 makes of the fp32 zero the other
// form stages.
template <int TM, int TN, int PIECES>
__device__ __forceinline__ void stage_load3_a(Staging3<TM, TN, PIECES, true> &s, const float *__restrict__ X, const TapCursor &cur,
                                              const int64_t (&abase)[TM / kRPP], const unsigned (&mask)[TM / kRPP], int Cin) {
  static_assert(PIECES == 3, "piece planes hold three pieces");
  const unsigned char *P = reinterpret_cast<const unsigned char *>(X);
#pragma unroll
  for (int h = 0; h < TM / kRPP; ++h) {
    s.a0[h] = s.a1[h] = s.a2[h] = u32x2{0u, 0u};
    if ((mask[h] >> cur.tap) & 1u) {
      const unsigned char *src = P + abase[h];
      s.a0[h] = *reinterpret_cast<const u32x2 *>(src + planes_offset(0, Cin, 0, cur.shift + cur.c0, 0));
      s.a1[h] = *reinterpret_cast<const u32x2 *>(src + planes_offset(0, Cin, 0, cur.shift + cur.c0, 1));
      s.a2[h] = *reinterpret_cast<const u32x2 *>(src + planes_offset(0, Cin, 0, cur.shift + cur.c0, 2));
    }
  }
}

// SCALED (include/skd_train2h.h): the fp32 quad is multiplied by `scale`, a power of two, in front of the split.
template <int TM, int TN, int PIECES, bool PLANES, int FMT = kBf16, bool SCALED = false>
__device__ __forceinline__ void stage_store3(const Staging3<TM, TN, PIECES, PLANES> &s, uint4 *stage, int srow, float scale = 1.f) {
  uint2 *sa = reinterpret_cast<uint2 *>(stage) + srow;
#pragma unroll
  for (int h = 0; h < TM / kRPP; ++h) {
    if constexpr (PLANES) {          // the three piece quads into split_store's slots, no split4
      u32x2 *dst = reinterpret_cast<u32x2 *>(sa + 2 * kRPP * h);
      dst[0] = s.a0[h];
      dst[2 * kPlaneChunks] = s.a1[h];
      dst[4 * kPlaneChunks] = s.a2[h];
    } else if constexpr (SCALED) {
      split_store<PIECES, FMT>(scaled(s.a[h], scale), sa + 2 * kRPP * h);
    } else {
      split_store<PIECES, FMT>(s.a[h], sa + 2 * kRPP * h);
    }
  }
  uint4 *sb = stage + operand_chunks(PIECES) + threadIdx.x;
#pragma unroll
  for (int i = 0; i < b_copies(TN, PIECES); ++i)
    if (b_copy_live<TN, PIECES>(i)) {
      if constexpr (PLANES) reinterpret_cast<u32x4 *>(sb)[i * kThreads] = s.b[i];
      else sb[i * kThreads] = s.b[i];
    }
}

// What k_loop (conv_split_dev.hpp) needs of a tile of this kernel.  k_loop calls load for kt = 0, 1, 2, ... in order, so the
// cursor is simply stepped behind every one: it runs as far ahead of the MFMAs as the loads do and crosses a tap boundary
// wherever that falls.  (Behind the last tile it stands at tap 9, which nothing reads.)
template <int TM, int TN, int PIECES = 3, bool PLANES = false, int FMT = kBf16, bool SCALED = false>
struct Tile3 {
  typedef Staging3<TM, TN, PIECES, PLANES> Stg;
  static constexpr int WM = wave_blocks_m(TM, TN);
  const float *__restrict__ X;
  const uint4 *__restrict__ bsrc;
  int srow, W, dil, Cin;
  TapCursor cur;
  int64_t abase[TM / kRPP];
  unsigned mask[TM / kRPP];
  float scale;                        // SCALED: the power of two of the activation operand (scale_of); otherwise unused
  f32x16 (&low)[WM][2], (&acc)[WM][2];
  __device__ __forceinline__ void load(Stg &s, int kt) {
    stage_load3_a<TM, TN, PIECES>(s, X, cur, abase, mask, Cin);
    stage_load3_b<TM, TN, PIECES, PLANES>(s, bsrc + (int64_t)kt * tile_chunks(TN, PIECES));
    cur.c0 += kBK;
    if (cur.c0 == Cin) {
      cur.c0 = 0;
      ++cur.tap;
      cur.shift = tap_shift(cur.tap, W, dil, Cin);
    }
  }
  __device__ __forceinline__ void store(const Stg &s, uint4 *stage, int) const { stage_store3<TM, TN, PIECES, PLANES, FMT, SCALED>(s, stage, srow, scale); }
  __device__ __forceinline__ void mma(const uint4 *stage) const { tile_mma<TM, TN, false, PIECES, FMT>(stage, low, acc); }
};

// STRIDE = 2 (include/skd_stride2.h; padding 1, dilation 1): THE row map of that form -- output row m = (b * Ho + oy) * Wo + ox of
// the (B, Ho, Wo) output, Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, reads the 3 x 3 window centred on input pixel (2 oy, 2 ox).
// *pixel: the flattened index of that centre, (b * H + 2 oy) * W + 2 ox, which is always inside the image; *mask: bit 3 ty + tx
// set iff tap (ty, tx) is, 0 <= 2 oy + ty - 1 < H and 0 <= 2 ox + tx - 1 < W.  Nothing else of the kernel knows the stride: the
// tap shifts are those of the input's W, the rows of the output are m.  The kernel calls it per panel row, the host entry
// skd_conv3x3_split_s2_taps per m (tests/test_conv3x3_stride2_cpu.py sweeps it).
__host__ __device__ inline void s2_row_map(int H, int W, int64_t m, int64_t *pixel, unsigned *mask) {
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const int64_t howo = (int64_t)Ho * Wo, b = m / howo;
  const int r = (int)(m - b * howo);
  const int oy = r / Wo, ox = r - oy * Wo;
  unsigned bits = 0;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int y = 2 * oy + tap / 3 - 1, x = 2 * ox + tap % 3 - 1;
    if (y >= 0 && y < H && x >= 0 && x < W) bits |= 1u << tap;
  }
  *mask = bits;
  *pixel = (b * H + 2 * oy) * W + 2 * ox;
}

// STATS (include/skd_bnstats.h): the batch-norm statistics record of one 32 x 32 accumulator block, from the fp32 values
// store_block has just stored (ACT = none, no BN terms: the stored value IS acc[q]).  Column `col` of the block lives in lanes l and
// l ^ 32, sixteen rows each (store_block's row map), so a record is an in-lane sum, one exchange with the other half, the
// block's own mean, the in-lane sum of the squared deviations about it and a second exchange: two passes, no pivot, no LDS, no
// barrier, no atomics.  Rows >= M are left out; the count min(32, M - row0) is implied by (M, block) and never stored.  The
// additions are written as one chain per lane and a + b of the two halves (commutative: both halves hold the same bits), the
// multiply-adds as explicit fmaf, so every tile form runs the same operations on the same values in the same order: the record
// of (block, channel) is a function of Y alone.  Record (mean, M2) at stats[(block * N + col) * 2], block = row0 / 32 -- row0 is a
// multiple of 32 in every tile form (m0 of 64, the wave offset of 32) -- written by the lower half as 32 consecutive float2.
__device__ __forceinline__ void block_stats(const f32x16 &acc, float *__restrict__ stats, int64_t row0, int col, int64_t M, int N) {
  if (row0 >= M) return;                                   // a block beyond the last row has no record (wave-uniform)
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t left = M - row0;                           // rows of this block that exist, if < 32
  const float cnt = left < 32 ? (float)left : 32.f;
  bool live[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) live[q] = (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5) < left;
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < 16; ++q) s += live[q] ? acc[q] : 0.f;
  const float mean = (s + __shfl_xor(s, 32, kWave)) / cnt;
  float m2 = 0.f;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const float d = live[q] ? acc[q] - mean : 0.f;
    m2 = __builtin_fmaf(d, d, m2);
  }
  m2 += __shfl_xor(m2, 32, kWave);
  if (lane < 32) *reinterpret_cast<float2 *>(stats + ((row0 >> 5) * N + col) * 2) = make_float2(mean, m2);
}

// One output tile of TM x TN pixels x channels.  HAS_RES: the residual R (the output's shape) is added behind the BN expression,
// in front of the activation (store_block): the second convolution of a BasicBlock.  STRIDE = 2: M counts the rows of the
// (B, Ho, Wo) output, H and W stay the input's, and the rows' addresses and masks come from s2_row_map; STRIDE = 1 is the code
// without it.  PLANES (include/skd_planes.h): X is the piece planes of the (M, Cin) input map; the rows' addresses are byte
// offsets of that layout and the staging set holds piece quads (stage_load3_a, stage_store3); masks, tap cursor, K loop, product order
// and epilogue are the code without it.  SCALED (include/skd_train2h.h; the data gradient on two fp16 pieces): the workgroup reads
// the scale word of X once, the staging multiplies X's quads by s in front of the split and the epilogue multiplies the joined
// sets by 1 / s in front of everything else; SCALED = false is the code without it.
template <int TM, int TN, int ACT, bool HAS_RES, int PIECES = 3, bool STATS = false, int STRIDE = 1, bool PLANES = false, int FMT = kBf16,
          bool SCALED = false>
__device__ __forceinline__ void conv3x3_tile(const float *__restrict__ X, const uint4 *__restrict__ Bp, float *__restrict__ Y,
                                             const float *__restrict__ R, float *__restrict__ stats,
                                             const float *__restrict__ cbias, const float *__restrict__ mean,
                                             const float *__restrict__ var, const float *__restrict__ weight,
                                             const float *__restrict__ bias, float eps, float slope, int64_t M, int H, int W,
                                             int Cin, int N, int dil, int64_t m0, int tn, uint4 *lds) {
  constexpr int WM = wave_blocks_m(TM, TN), kRA = TM / kRPP;
  float scale = 1.f, unscale = 1.f;
  if constexpr (SCALED) scale_of(__float_as_uint(*R), scale, unscale);      // R: the scale word's address (the kernel's note)
  f32x16 acc[WM][2], low[WM][2];      // a0 b0 | the five (PIECES = 2: two) smaller products (tile_mma): added in the epilogue
#pragma unroll
  for (int i = 0; i < WM; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][j][q] = low[i][j][q] = 0.f;
  const int nk = 9 * (Cin / kBK);
  const int gt = threadIdx.x, grow = gt / kQK, gkq = (gt % kQK) * 4;
  const int srow = plane_slot(grow, gkq);
  // this thread's panel rows: address of (pixel, channel quad) and the taps that stay inside the image; a row beyond M has none
  int64_t abase[kRA];
  unsigned mask[kRA];
  const int64_t hw = (int64_t)H * W;
#pragma unroll
  for (int h = 0; h < kRA; ++h) {
    const int64_t m = m0 + grow + kRPP * h;
    const bool live = m < M;
    if constexpr (STRIDE == 2) {
      int64_t pixel = 0;
      unsigned bits = 0;
      if (live) s2_row_map(H, W, m, &pixel, &bits);
      mask[h] = bits;
      abase[h] = pixel * Cin + gkq;
      continue;
    }
    const int64_t mm = live ? m : 0;
    const int pix = (int)(mm % hw);
    const int py = pix / W, px = pix - py * W;
    unsigned bits = 0;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int64_t y = py + (int64_t)(tap / 3 - 1) * dil, x = px + (int64_t)(tap % 3 - 1) * dil;
      if (live && y >= 0 && y < H && x >= 0 && x < W) bits |= 1u << tap;
    }
    mask[h] = bits;
    abase[h] = PLANES ? planes_offset(M, Cin, mm, gkq, 0) : mm * Cin + gkq;
  }
  const uint4 *bsrc = Bp + (int64_t)tn * nk * tile_chunks(TN, PIECES) + gt;
  Tile3<TM, TN, PIECES, PLANES, FMT, SCALED> tile = {X, bsrc, srow, W, dil, Cin, {0, 0, tap_shift(0, W, dil, Cin)}, {}, {}, scale, low, acc};
#pragma unroll
  for (int h = 0; h < kRA; ++h) {
    tile.abase[h] = abase[h];
    tile.mask[h] = mask[h];
  }
  k_loop<kDepth3x3, PIECES>(tile, nk, lds);
  // ---- epilogue: (+ conv bias) -> eval-mode InPlace-ABN formula (when there are statistics) -> (+ residual) -> activation ----
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  const int wi = (wid / (TN / 64)) * (TM / waves_m(TN)), wj = (wid % (TN / 64)) * 64;      // tile_mma's wave map
  const bool full = m0 + TM <= M;
#pragma unroll
  for (int bj = 0; bj < 2; ++bj) {
    const int col = tn * TN + wj + bj * 32 + (lane & 31);
    const bool bn = mean != nullptr;
    const float mu = bn ? mean[col] : 0.f, is = bn ? inv_std_of(var[col], eps) : 1.f;
    const float ga = bn && weight != nullptr ? fabsf(weight[col]) + eps : 1.f;     // bn.cu:153
    const float be = bn && bias != nullptr ? bias[col] : 0.f;
    const float cb = cbias != nullptr ? cbias[col] : 0.f;
#pragma unroll
    for (int bi = 0; bi < WM; ++bi) {
      join_sets<FMT>(acc[bi][bj], low[bi][bj]);
      if constexpr (SCALED) {
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[bi][bj][q] *= unscale;
      }
      if (cbias != nullptr) {
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[bi][bj][q] += cb;
      }
      const int64_t row0 = m0 + wi + bi * 32;
      if (full)
        store_block<ACT, HAS_RES, true, false>(acc[bi][bj], R, Y, row0, col, M, N, mu, is, ga, be, slope);
      else
        store_block<ACT, HAS_RES, false, false>(acc[bi][bj], R, Y, row0, col, M, N, mu, is, ga, be, slope);
      if constexpr (STATS) block_stats(acc[bi][bj], stats, row0, col, M, N);
    }
  }
}

// TALL: row panels p < p_full are 128 pixels high, the panels behind them 64 (conv1x1.hip, round 6: the half-height mechanism);
// the two accumulator sets of a 128 x 128 tile take 128 VGPRs and the kernel 238 (two staging sets: k_loop), so that form runs two workgroups per CU -- its
// 64-row panels too: they are the same kernel.  !TALL: every panel is 64 pixels high (p_full = 0), 64 accumulator registers,
// 148 VGPRs; three workgroups per CU, which is what 48 KB of LDS per workgroup and 168 registers admit.
// TN = 64 is TALL with every panel 128 pixels high (a 64 x 64 tile would leave a wave 16 rows): 64 accumulator registers again,
// so three workgroups per CU.
// The waves-per-SIMD range states those residencies (2, 3) so that the register budget follows from them and not from the
// launch bound alone (profiles/r15_kernel_resources.md).
constexpr int conv3x3_wgs(int TN, bool TALL) { return TALL && TN == kTN ? 2 : kMinWG; }

// PIECES = 2 keeps the residencies, the grid and the tile heights of its three-piece twin (include/skd_split2.h); so does
// STRIDE = 2 (include/skd_stride2.h), whose M is that of the smaller output.
// FMT = kFp16 (two fp16 pieces, include/skd_split2h.h) also has the residual-epilogue, 64-column and stride-2 forms
// (include/skd_infer2h.h: the student's inference form); two bf16 pieces have the wide forms without residual alone.  The 64-column
// two-piece form takes 28 KB of LDS: a stage is 512 chunks of A and 256 of B -- one copy per thread -- the second stage
// stage_chunks(2) = 1024 chunks behind the first.
// SCALED (include/skd_train2h.h): the raw 128-column stride-1 fp16 form alone, both tile heights.  It has no residual, and the scale
// word of X (one 32-bit word on the device) arrives in the residual pointer's place, so the kernel's argument list is one for every
// instantiation and the old ones are what they were.
template <int TN, int ACT, bool TALL, bool HAS_RES, int PIECES = 3, bool STATS = false, int STRIDE = 1, bool PLANES = false, int FMT = kBf16,
          bool SCALED = false>
__global__ __launch_bounds__(kThreads, conv3x3_wgs(TN, TALL))
__attribute__((amdgpu_waves_per_eu(conv3x3_wgs(TN, TALL), conv3x3_wgs(TN, TALL))))
void conv3x3_split_kernel(
    const float *__restrict__ X, const uint4 *__restrict__ Bp, float *__restrict__ Y, const float *__restrict__ cbias,
    const float *__restrict__ mean, const float *__restrict__ var, const float *__restrict__ weight,
    const float *__restrict__ bias, float eps, float slope, int64_t M, int H, int W, int Cin, int N, int dil, int tiles_n,
    int p_full, const float *__restrict__ R, float *__restrict__ stats) {
  static_assert(TALL || TN == kTN, "64-row panels exist for the 128-column form only");
  static_assert(!STATS || (ACT == SKD_ACT_NONE && !HAS_RES && PIECES == 3), "statistics: the training forward's raw epilogue alone");
  static_assert(PIECES == 3 || FMT == kFp16 || (TN == kTN && !HAS_RES), "two bf16 pieces: the 128-column forward family without the residual");
  static_assert(STRIDE == 1 || (STRIDE == 2 && TN == kTN && !HAS_RES && !STATS), "stride 2: the 128-column frozen forward alone");
  static_assert(!PLANES || (TN == kTN && PIECES == 3 && !HAS_RES && !STATS && STRIDE == 1), "piece planes in: the wide stride-1 frozen forward alone");
  static_assert(FMT == kBf16 || (PIECES == 2 && !STATS && !PLANES), "fp16 pieces: two of them, the frozen forward families alone (include/skd_infer2h.h)");
  static_assert(!SCALED || (FMT == kFp16 && PIECES == 2 && TN == kTN && ACT == SKD_ACT_NONE && !HAS_RES && !STATS && STRIDE == 1 && !PLANES),
                "a scaled operand: the raw wide stride-1 form on two fp16 pieces alone (include/skd_train2h.h)");
  extern __shared__ __attribute__((aligned(16))) uint4 lds[];
  const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
  const int pl = j / tiles_n, tn = j - pl * tiles_n;
  const int64_t tm = (int64_t)pl * 8 + xcd;
  if (TALL && (TN < kTN || tm < p_full)) {
    const int64_t m0 = tm * kTM;
    if (m0 >= M) return;
    conv3x3_tile<kTM, TN, ACT, HAS_RES, PIECES, STATS, STRIDE, PLANES, FMT, SCALED>(X, Bp, Y, R, stats, cbias, mean, var, weight, bias, eps, slope, M, H, W, Cin, N, dil, m0, tn, lds);
  } else if constexpr (TN == kTN) {
    const int64_t m0 = (int64_t)p_full * kTM + (tm - p_full) * (kTM / 2);
    if (m0 >= M) return;
    conv3x3_tile<kTM / 2, TN, ACT, HAS_RES, PIECES, STATS, STRIDE, PLANES, FMT, SCALED>(X, Bp, Y, R, stats, cbias, mean, var, weight, bias, eps, slope, M, H, W, Cin, N, dil, m0, tn, lds);
  }
}

// The weight split, of a frozen network (once) and of the training form (per step, include/skd_train.h): ONE launch writes the
// image of W (Cout, Cin, 3, 3) for the forward convolution and / or the image of Wd[c][n][ty][tx] = W[n][c][2 - ty][2 - tx]
// (Cin, Cout, 3, 3) for the data gradient, both read from W through its strides (elements) -- contiguous and channels-last
// tensors give the same pack, and Wd is index arithmetic, never a tensor.  One workgroup of 2 TN threads per (column tile,
// K-tile) of one image, one thread per 16-byte chunk (the 8 consecutive k of one row, three pieces), so the direction is uniform
// per workgroup: the first `fwd_tiles` workgroups write the forward image (8 k = one tap, 8 channels of one output channel), the
// others the backward image.  There the rows of a tile are TN input channels c and the 8 consecutive k of a chunk are 8 output channels n at stride sn:
// a wave's 64 lanes are 64 consecutive c, so each of its eight loads reads a run of 64 elements at stride sc -- 256 contiguous
// bytes of a channels-last weight (sc = 1: the training student's, and the PSP bottleneck's channel slice).
// PIECES = 2 (include/skd_split2.h): the first two planes alone, 4 TN chunks per (column tile, K-tile).
// FMT = kFp16 (include/skd_split2h.h): the two fp16 planes p0 and the scaled p1 of split4_f16, the same 4 TN chunks.
template <int TN, int PIECES = 3, int FMT = kBf16>
__global__ __launch_bounds__(2 * TN) void conv3x3_pack_pair_kernel(
    const float *__restrict__ Wt, int64_t sn, int64_t sc, int64_t sy, int64_t sx, int Cin, int Cout, int64_t fwd_tiles,
    uint4 *__restrict__ pack_fwd, uint4 *__restrict__ pack_bwd) {
  const int chunk = threadIdx.x;
  const int kh = chunk / TN, row = (chunk % TN) ^ (kh * 4);
  const bool fwd = (int64_t)blockIdx.x < fwd_tiles;
  const int64_t tile = fwd ? (int64_t)blockIdx.x : (int64_t)blockIdx.x - fwd_tiles;      // = column tile * nk + kt
  const int K9 = fwd ? Cin : Cout;                                                      // channels per tap of this image's K
  const int nk = 9 * (K9 / kBK);
  const int kt = (int)(tile % nk), tn = (int)(tile / nk);
  const int k0 = kt * kBK + kh * 8, tap = k0 / K9, e0 = k0 - tap * K9;
  const int ty = fwd ? tap / 3 : 2 - tap / 3, tx = fwd ? tap % 3 : 2 - tap % 3;         // backward: the flipped tap
  const int64_t srow = fwd ? sn : sc, sk = fwd ? sc : sn;                               // backward: rows are c, k runs over n
  const float *src = Wt + (int64_t)(tn * TN + row) * srow + ty * sy + tx * sx;
  float v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = src[(e0 + i) * sk];
  // the three-piece split for either PIECES: its first two pieces ARE the two-piece split (the third is dropped unused), so the
  // two-plane image is planes 0 and 1 of the other bit for bit; the two-piece split4 overload serves split_store<2> alone
  uint2 lo[3], hi[3];
  if constexpr (FMT == kFp16) {
    static_assert(PIECES == 2, "fp16 pieces: two of them");
    split4_f16(make_float4(v[0], v[1], v[2], v[3]), lo[0], lo[1]);
    split4_f16(make_float4(v[4], v[5], v[6], v[7]), hi[0], hi[1]);
  } else {
    split4(make_float4(v[0], v[1], v[2], v[3]), lo[0], lo[1], lo[2]);
    split4(make_float4(v[4], v[5], v[6], v[7]), hi[0], hi[1], hi[2]);
  }
  uint4 *pack = fwd ? pack_fwd : pack_bwd;
#pragma unroll
  for (int p = 0; p < PIECES; ++p) pack[(tile * PIECES + p) * (2 * TN) + chunk] = make_uint4(lo[p].x, lo[p].y, hi[p].x, hi[p].y);
}

template <int TN, int ACT, bool TALL, bool HAS_RES, int PIECES = 3, bool STATS = false, int STRIDE = 1, bool PLANES = false, int FMT = kBf16,
          bool SCALED = false>
static int launch3(const float *X, const uint4 *Bp, float *Y, const float *R, const float *cbias, const float *mean, const float *var,
                   const float *weight, const float *bias, float eps, float slope, int64_t M, int H, int W, int Cin, int N, int dil,
                   int geometry, hipStream_t st, float *stats = nullptr, const uint32_t *word = nullptr) {
  static PerDeviceFlag ready;          // per instantiation AND per device
  bool *rdy = ready.get();
  if (rdy == nullptr) return 0;
  if (!*rdy) {
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(conv3x3_split_kernel<TN, ACT, TALL, HAS_RES, PIECES, STATS, STRIDE, PLANES, FMT, SCALED>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)conv3x3_lds(TN, PIECES)) != hipSuccess) return 0;
    *rdy = true;
  }
  const int tiles_n = N / TN;
  const int64_t tiles_m = cdiv(M, kTM);
  // TALL: 128-row panels p < p_full, 64-row panels behind them.  geometry 1: all 128; geometry 3: 128 for the launch's whole
  // rounds (two workgroups per CU) and 64 for the rest
  int64_t p_full = TALL ? tiles_m : 0;
  if (TALL && geometry == 3) {
    const int64_t slots = 2 * (int64_t)cu_count(st), tiles = tiles_m * tiles_n;
    if (slots > 0 && tiles % slots != 0) p_full = (tiles / slots) * slots / tiles_n / 8 * 8;
  }
  const int64_t panels = p_full < tiles_m ? p_full + cdiv(M - p_full * kTM, kTM / 2) : tiles_m;
  const int64_t grid = cdiv(panels, 8) * 8 * tiles_n;
  if (grid > 2147483647) return 0;
  conv3x3_split_kernel<TN, ACT, TALL, HAS_RES, PIECES, STATS, STRIDE, PLANES, FMT, SCALED><<<dim3((unsigned)grid), dim3(kThreads), conv3x3_lds(TN, PIECES), st>>>(
      X, Bp, Y, cbias, mean, var, weight, bias, eps, slope, M, H, W, Cin, N, dil, tiles_n, (int)p_full,
      SCALED ? reinterpret_cast<const float *>(word) : R, stats);
  return ok();
}

// geometry (see skd_eval.h): 1 and 3 = the TALL forms, 2 = 64-row tiles; 0 = the shipped choice: 3 once the 128-row tiles fill the
// chip's two-per-CU slots at least once (every routed shape of the teacher at batch 8), 64-row tiles below that.
// profiles/r12_conv3x3_isolated.md (tools/conv3x3_bench.py) has every geometry per shape: on the four routed shapes 3 is 6-14 %
// ahead of the 64-row tiles and 10-19 % ahead of 1 (all tiles 128 rows: its partial last round leaves CUs idle); below one full
// round the 64-row tiles win (128 -> 128 at 65 x 65: 85 against 95 us).  1 is kept for measurements only.
// TN = 64 has the one geometry, 1 (skd_narrow.h: 0 and 1 are accepted and mean it).
template <int TN, int ACT, bool HAS_RES, int PIECES = 3, bool STATS = false, int STRIDE = 1, bool PLANES = false, int FMT = kBf16,
          bool SCALED = false>
static int launch3g(const float *X, const uint4 *Bp, float *Y, const float *R, const float *cbias, const float *mean, const float *var,
                    const float *weight, const float *bias, float eps, float slope, int64_t M, int H, int W, int Cin, int N, int dil,
                    int geometry, hipStream_t st, float *stats = nullptr, const uint32_t *word = nullptr) {
  if constexpr (TN < kTN) {
    static_assert(STRIDE == 1 && !PLANES && !SCALED, "the 64-column form: stride 1 on an unscaled fp32 map");
    return launch3<TN, ACT, true, HAS_RES, PIECES, STATS, 1, false, FMT>(X, Bp, Y, R, cbias, mean, var, weight, bias, eps, slope, M, H, W, Cin, N, dil, 1, st, stats);
  } else {
    if (geometry == 0) geometry = cdiv(M, kTM) * (N / kTN) > 2 * (int64_t)cu_count(st) ? 3 : 2;
    if (geometry == 1 || geometry == 3)
      return launch3<TN, ACT, true, HAS_RES, PIECES, STATS, STRIDE, PLANES, FMT, SCALED>(X, Bp, Y, R, cbias, mean, var, weight, bias, eps, slope, M, H, W, Cin, N, dil, geometry, st, stats, word);
    return launch3<TN, ACT, false, HAS_RES, PIECES, STATS, STRIDE, PLANES, FMT, SCALED>(X, Bp, Y, R, cbias, mean, var, weight, bias, eps, slope, M, H, W, Cin, N, dil, geometry, st, stats, word);
  }
}

// ---- the host bodies of the two entry families (TN = 128: skd_conv3x3_split_*, TN = 64: skd_conv3x3_narrow_*) ----

template <int TN>
static int supported3(int Cin, int Cout, int stride, int padding, int dilation, int groups) {
  return Cin > 0 && Cout > 0 && Cin % kBK == 0 && Cout % TN == 0 && stride == 1 && dilation >= 1 && padding == dilation && groups == 1;
}

template <int TN, int PIECES = 3>
static int64_t pack_bytes3(int Cin, int Cout) {
  if (!supported3<TN>(Cin, Cout, 1, 1, 1, 1)) return 0;
  return (int64_t)(Cout / TN) * (9 * (Cin / kBK)) * tile_chunks(TN, PIECES) * (int64_t)sizeof(uint4);
}

// The (column tile, K-tile) count of the image of an (N, K / 9, 3, 3) weight in `pack`, 0 for no image (pack == nullptr), -1
// for an image that is refused: a direction the core does not take, a buffer too small or not 16-byte aligned.
template <int TN, int PIECES = 3>
static int64_t pack_image_tiles(int K9, int N, const void *pack, int64_t pack_bytes) {
  if (!pack) return 0;
  const int64_t need = pack_bytes3<TN, PIECES>(K9, N);
  if (need == 0 || pack_bytes < need || (reinterpret_cast<uintptr_t>(pack) & 15)) return -1;
  return (int64_t)(N / TN) * (9 * (K9 / kBK));
}

// Either image or both in one launch (include/skd_train.h); every refusal is decided here, in front of the launch.
template <int TN, int PIECES = 3, int FMT = kBf16>
static int pack_pair3(int Cin, int Cout, const float *w, int64_t stride_n, int64_t stride_c, int64_t stride_y, int64_t stride_x,
                      void *pack_fwd, int64_t fwd_bytes, void *pack_bwd, int64_t bwd_bytes, skd_stream_t stream) {
  if (!w || (!pack_fwd && !pack_bwd)) return 0;
  if (stride_n < 0 || stride_c < 0 || stride_y < 0 || stride_x < 0) return 0;
  const int64_t fwd_tiles = pack_image_tiles<TN, PIECES>(Cin, Cout, pack_fwd, fwd_bytes);
  const int64_t bwd_tiles = pack_image_tiles<TN, PIECES>(Cout, Cin, pack_bwd, bwd_bytes);
  if (fwd_tiles < 0 || bwd_tiles < 0 || fwd_tiles + bwd_tiles > 2147483647) return 0;
  conv3x3_pack_pair_kernel<TN, PIECES, FMT><<<dim3((unsigned)(fwd_tiles + bwd_tiles)), dim3(2 * TN), 0, as_stream(stream)>>>(
      w, stride_n, stride_c, stride_y, stride_x, Cin, Cout, fwd_tiles, static_cast<uint4 *>(pack_fwd),
      static_cast<uint4 *>(pack_bwd));
  return ok();
}

// out = act(ABN_eval(conv3x3(x) + conv_bias) [+ residual]); residual == nullptr takes the instantiations without the residual
// read.  The kernel reads the residual through a __restrict__ pointer at the offsets it writes, so a residual that overlaps the
// output is refused, not defined.
template <int TN, int PIECES = 3, int FMT = kBf16>
static int run3(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const void *wpack, float *out,
                const float *residual, const float *conv_bias, const float *mean, const float *var, const float *weight,
                const float *bias, float eps, int activation, float slope, int geometry, int max_geometry, skd_stream_t stream) {
  if (!supported3<TN>(Cin, Cout, 1, dilation, dilation, 1) || B < 1 || H < 1 || W < 1) return 0;
  if (!x || !wpack || !out || (mean == nullptr) != (var == nullptr) || geometry < 0 || geometry > max_geometry) return 0;
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
#define SKD_CONV3X3_CASE(ACT)                                                                                                 \
  case ACT:                                                                                                                   \
    if constexpr (PIECES == 3)                                                                                                \
      return (residual != nullptr ? launch3g<TN, ACT, true> : launch3g<TN, ACT, false>)(                                     \
          x, bp, out, residual, conv_bias, mean, var, weight, bias, eps, slope, M, H, W, Cin, Cout, dilation, geometry, st,    \
          nullptr, nullptr);                                                                                                  \
    else if constexpr (FMT == kFp16) /* include/skd_infer2h.h: the fp16 form has the residual epilogue */                     \
      return (residual != nullptr ? launch3g<TN, ACT, true, PIECES, false, 1, false, FMT>                                     \
                                  : launch3g<TN, ACT, false, PIECES, false, 1, false, FMT>)(                                  \
          x, bp, out, residual, conv_bias, mean, var, weight, bias, eps, slope, M, H, W, Cin, Cout, dilation, geometry, st,    \
          nullptr, nullptr);                                                                                                  \
    else                                                                                                                      \
      return residual != nullptr ? 0 : launch3g<TN, ACT, false, PIECES, false, 1, false, FMT>(                                \
          x, bp, out, residual, conv_bias, mean, var, weight, bias, eps, slope, M, H, W, Cin, Cout, dilation, geometry, st)
  switch (activation) {
    SKD_CONV3X3_CASE(SKD_ACT_NONE);
    SKD_CONV3X3_CASE(SKD_ACT_RELU);
    SKD_CONV3X3_CASE(SKD_ACT_LEAKY_RELU);
    default: return 0;
  }
#undef SKD_CONV3X3_CASE
}

// include/skd_planes.h: run3<kTN> without residual whose activation operand is the piece planes of the (B, H, W, Cin) map --
// run3's refusals, the planes pointer in x's place (16-byte aligned, as x).
static int run3_planes(int B, int H, int W, int Cin, int Cout, int dilation, const void *planes, const void *wpack, float *out,
                       const float *conv_bias, const float *mean, const float *var, const float *weight, const float *bias,
                       float eps, int activation, float slope, int geometry, skd_stream_t stream) {
  if (!supported3<kTN>(Cin, Cout, 1, dilation, dilation, 1) || B < 1 || H < 1 || W < 1) return 0;
  if (!planes || !wpack || !out || (mean == nullptr) != (var == nullptr) || geometry < 0 || geometry > 3) return 0;
  if ((reinterpret_cast<uintptr_t>(planes) | reinterpret_cast<uintptr_t>(wpack)) & 15) return 0;
  if ((int64_t)H * W > 2147483647 || dilation > (1 << 24)) return 0;
  const int64_t M = (int64_t)B * H * W;
  hipStream_t st = as_stream(stream);
  const float *x = static_cast<const float *>(planes);
  const uint4 *bp = static_cast<const uint4 *>(wpack);
#define SKD_CONV3X3_PLANES_CASE(ACT)                                                                                          \
  case ACT:                                                                                                                   \
    return launch3g<kTN, ACT, false, 3, false, 1, true>(x, bp, out, nullptr, conv_bias, mean, var, weight, bias, eps, slope, M, H, W, \
                                                        Cin, Cout, dilation, geometry, st)
  switch (activation) {
    SKD_CONV3X3_PLANES_CASE(SKD_ACT_NONE);
    SKD_CONV3X3_PLANES_CASE(SKD_ACT_RELU);
    SKD_CONV3X3_PLANES_CASE(SKD_ACT_LEAKY_RELU);
    default: return 0;
  }
#undef SKD_CONV3X3_PLANES_CASE
}

// include/skd_train2h.h: the raw convolution on two fp16 pieces whose activation operand is scaled by its word -- run3's refusals
// (no residual, no epilogue terms), and a NULL or misaligned word.
static int run3_scaled(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const void *wpack, float *out,
                       const uint32_t *word, int geometry, skd_stream_t stream) {
  if (!supported3<kTN>(Cin, Cout, 1, dilation, dilation, 1) || B < 1 || H < 1 || W < 1) return 0;
  if (!x || !wpack || !out || !word || geometry < 0 || geometry > 3) return 0;
  if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(wpack)) & 15) || (reinterpret_cast<uintptr_t>(word) & 3)) return 0;
  if ((int64_t)H * W > 2147483647 || dilation > (1 << 24)) return 0;
  const int64_t M = (int64_t)B * H * W;
  return launch3g<kTN, SKD_ACT_NONE, false, 2, false, 1, false, kFp16, true>(x, static_cast<const uint4 *>(wpack), out, nullptr, nullptr,
                                                                             nullptr, nullptr, nullptr, nullptr, 0.f, 0.f, M, H, W, Cin,
                                                                             Cout, dilation, geometry, as_stream(stream), nullptr, word);
}

// include/skd_bnstats.h: floats of the statistics workspace of an (M, Cout) output -- one (mean, M2) per 32-row block and
// channel -- or 0 for sizes no entry takes.
static int64_t bnstats_floats(int64_t M, int Cout) {
  if (M < 1 || Cout < 1 || Cout % kNarrowTN != 0 || M > (int64_t)1 << 40) return 0;
  return cdiv(M, (int64_t)32) * Cout * 2;
}

// out = conv3x3(x) + conv_bias, raw (the training forward: no BN terms, no activation, no residual), and the statistics records
// of `out`.  Everything run3 refuses is refused; so are a NULL or misaligned (8 bytes: the records are float2) or short `stats`.
template <int TN>
static int run3_stats(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const void *wpack, float *out,
                      const float *conv_bias, int geometry, int max_geometry, float *stats, int64_t stats_floats,
                      skd_stream_t stream) {
  if (!supported3<TN>(Cin, Cout, 1, dilation, dilation, 1) || B < 1 || H < 1 || W < 1) return 0;
  if (!x || !wpack || !out || geometry < 0 || geometry > max_geometry) return 0;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(wpack)) & 15) return 0;
  if ((int64_t)H * W > 2147483647 || dilation > (1 << 24)) return 0;
  const int64_t M = (int64_t)B * H * W, need = bnstats_floats(M, Cout);
  if (!stats || (reinterpret_cast<uintptr_t>(stats) & 7) || need == 0 || stats_floats < need) return 0;
  return launch3g<TN, SKD_ACT_NONE, false, 3, true>(x, static_cast<const uint4 *>(wpack), out, nullptr, conv_bias, nullptr, nullptr,
                                                    nullptr, nullptr, 0.f, 0.f, M, H, W, Cin, Cout, dilation, geometry,
                                                    as_stream(stream), stats);
}

// include/skd_stride2.h: the predicate, the host evaluation of the row map and the frozen forward of the stride-2 form.
static int supported3_s2(int Cin, int Cout, int stride, int padding, int dilation, int groups) {
  return Cin > 0 && Cout > 0 && Cin % kBK == 0 && Cout % kTN == 0 && stride == 2 && padding == 1 && dilation == 1 && groups == 1;
}

static int taps_s2(int H, int W, int64_t m, int64_t *pixel, unsigned *mask) {
  if (H < 1 || W < 1 || m < 0 || !pixel || !mask || (int64_t)H * W > 2147483647) return 0;
  s2_row_map(H, W, m, pixel, mask);
  return 1;
}

// out (B, Ho, Wo, Cout) = act(ABN_eval(conv3x3_stride2(x) + conv_bias)): run3's refusals (no residual), on the packs of either
// piece count -- the image does not depend on the stride.  Raw and ReLU epilogues are instantiated; leaky ReLU is refused.
// FMT = kFp16 (include/skd_infer2h.h): on the two-plane fp16 image of skd_conv3x3_split2h_pack_weights.
template <int PIECES, int FMT = kBf16>
static int run3_s2(int B, int H, int W, int Cin, int Cout, const float *x, const void *wpack, float *out, const float *conv_bias,
                   const float *mean, const float *var, const float *weight, const float *bias, float eps, int activation,
                   float slope, int geometry, skd_stream_t stream) {
  if (!supported3_s2(Cin, Cout, 2, 1, 1, 1) || B < 1 || H < 1 || W < 1) return 0;
  if (!x || !wpack || !out || (mean == nullptr) != (var == nullptr) || geometry < 0 || geometry > 3) return 0;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(wpack)) & 15) return 0;
  if ((int64_t)H * W > 2147483647) return 0;
  const int64_t M = (int64_t)B * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1);
  hipStream_t st = as_stream(stream);
  const uint4 *bp = static_cast<const uint4 *>(wpack);
  switch (activation) {
    case SKD_ACT_NONE:
      return launch3g<kTN, SKD_ACT_NONE, false, PIECES, false, 2, false, FMT>(x, bp, out, nullptr, conv_bias, mean, var, weight, bias, eps,
                                                                              slope, M, H, W, Cin, Cout, 1, geometry, st);
    case SKD_ACT_RELU:
      return launch3g<kTN, SKD_ACT_RELU, false, PIECES, false, 2, false, FMT>(x, bp, out, nullptr, conv_bias, mean, var, weight, bias, eps,
                                                                              slope, M, H, W, Cin, Cout, 1, geometry, st);
    default: return 0;
  }
}

}  // namespace
}  // namespace skd

using namespace skd;

extern "C" {

int skd_conv3x3_split_supported(int Cin, int Cout, int stride, int padding, int dilation, int groups) {
  return supported3<kTN>(Cin, Cout, stride, padding, dilation, groups);
}

int64_t skd_conv3x3_split_pack_bytes(int Cin, int Cout) { return pack_bytes3<kTN>(Cin, Cout); }

int skd_conv3x3_split_train_supported(int Cin, int Cout, int stride, int padding, int dilation, int groups) {
  return supported3<kTN>(Cin, Cout, stride, padding, dilation, groups) && Cin % kTN == 0;
}

int skd_conv3x3_split_pack_pair(int Cin, int Cout, const float *w, int64_t stride_n, int64_t stride_c, int64_t stride_y,
                                int64_t stride_x, void *pack_fwd, int64_t fwd_bytes, void *pack_bwd, int64_t bwd_bytes,
                                skd_stream_t stream) {
  return pack_pair3<kTN>(Cin, Cout, w, stride_n, stride_c, stride_y, stride_x, pack_fwd, fwd_bytes, pack_bwd, bwd_bytes, stream);
}

// The forward image alone (include/skd_eval.h): the same launch without a backward image.
int skd_conv3x3_split_pack_weights(int Cin, int Cout, const float *w, int64_t stride_n, int64_t stride_c, int64_t stride_y,
                                   int64_t stride_x, void *pack, int64_t pack_bytes, skd_stream_t stream) {
  return pack_pair3<kTN>(Cin, Cout, w, stride_n, stride_c, stride_y, stride_x, pack, pack_bytes, nullptr, 0, stream);
}

int skd_conv3x3_split_nhwc(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const void *wpack, float *out,
                           const float *conv_bias, const float *mean, const float *var, const float *weight, const float *bias,
                           float eps, int activation, float slope, int geometry, skd_stream_t stream) {
  return run3<kTN>(B, H, W, Cin, Cout, dilation, x, wpack, out, nullptr, conv_bias, mean, var, weight, bias, eps, activation, slope,
                   geometry, 3, stream);
}

// include/skd_infer.h: the same with the residual pointer.
int skd_conv3x3_split_res_nhwc(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const void *wpack, float *out,
                               const float *residual, const float *conv_bias, const float *mean, const float *var,
                               const float *weight, const float *bias, float eps, int activation, float slope, int geometry,
                               skd_stream_t stream) {
  return run3<kTN>(B, H, W, Cin, Cout, dilation, x, wpack, out, residual, conv_bias, mean, var, weight, bias, eps, activation, slope,
                   geometry, 3, stream);
}

// include/skd_split2.h: the 128-column forward family on two pieces per operand (three products), and its two-plane weight image.
int64_t skd_conv3x3_split2_pack_bytes(int Cin, int Cout) { return pack_bytes3<kTN, 2>(Cin, Cout); }

int skd_conv3x3_split2_pack_weights(int Cin, int Cout, const float *w, int64_t stride_n, int64_t stride_c, int64_t stride_y,
                                    int64_t stride_x, void *pack, int64_t pack_bytes, skd_stream_t stream) {
  return pack_pair3<kTN, 2>(Cin, Cout, w, stride_n, stride_c, stride_y, stride_x, pack, pack_bytes, nullptr, 0, stream);
}

// include/skd_train2.h: both two-plane images of a trained weight in one launch
int skd_conv3x3_split2_pack_pair(int Cin, int Cout, const float *w, int64_t stride_n, int64_t stride_c, int64_t stride_y,
                                 int64_t stride_x, void *pack_fwd, int64_t fwd_bytes, void *pack_bwd, int64_t bwd_bytes,
                                 skd_stream_t stream) {
  return pack_pair3<kTN, 2>(Cin, Cout, w, stride_n, stride_c, stride_y, stride_x, pack_fwd, fwd_bytes, pack_bwd, bwd_bytes, stream);
}

int skd_conv3x3_split2_nhwc(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const void *wpack, float *out,
                            const float *conv_bias, const float *mean, const float *var, const float *weight, const float *bias,
                            float eps, int activation, float slope, int geometry, skd_stream_t stream) {
  return run3<kTN, 2>(B, H, W, Cin, Cout, dilation, x, wpack, out, nullptr, conv_bias, mean, var, weight, bias, eps, activation,
                      slope, geometry, 3, stream);
}

// include/skd_split2h.h: the same family on two FP16 pieces per operand with the scaled residual, and its two-plane weight image.
int64_t skd_conv3x3_split2h_pack_bytes(int Cin, int Cout) { return pack_bytes3<kTN, 2>(Cin, Cout); }

int skd_conv3x3_split2h_pack_weights(int Cin, int Cout, const float *w, int64_t stride_n, int64_t stride_c, int64_t stride_y,
                                     int64_t stride_x, void *pack, int64_t pack_bytes, skd_stream_t stream) {
  return pack_pair3<kTN, 2, kFp16>(Cin, Cout, w, stride_n, stride_c, stride_y, stride_x, pack, pack_bytes, nullptr, 0, stream);
}

int skd_conv3x3_split2h_nhwc(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const void *wpack, float *out,
                             const float *conv_bias, const float *mean, const float *var, const float *weight, const float *bias,
                             float eps, int activation, float slope, int geometry, skd_stream_t stream) {
  return run3<kTN, 2, kFp16>(B, H, W, Cin, Cout, dilation, x, wpack, out, nullptr, conv_bias, mean, var, weight, bias, eps, activation,
                             slope, geometry, 3, stream);
}

// include/skd_infer2h.h: the residual-epilogue, 64-column and stride-2 forms on two fp16 pieces (the student's inference form).
int skd_conv3x3_split2h_res_nhwc(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const void *wpack, float *out,
                                 const float *residual, const float *conv_bias, const float *mean, const float *var,
                                 const float *weight, const float *bias, float eps, int activation, float slope, int geometry,
                                 skd_stream_t stream) {
  return run3<kTN, 2, kFp16>(B, H, W, Cin, Cout, dilation, x, wpack, out, residual, conv_bias, mean, var, weight, bias, eps, activation,
                             slope, geometry, 3, stream);
}

int64_t skd_conv3x3_narrow2h_pack_bytes(int Cin, int Cout) { return pack_bytes3<kNarrowTN, 2>(Cin, Cout); }

int skd_conv3x3_narrow2h_pack_weights(int Cin, int Cout, const float *w, int64_t stride_n, int64_t stride_c, int64_t stride_y,
                                      int64_t stride_x, void *pack, int64_t pack_bytes, skd_stream_t stream) {
  return pack_pair3<kNarrowTN, 2, kFp16>(Cin, Cout, w, stride_n, stride_c, stride_y, stride_x, pack, pack_bytes, nullptr, 0, stream);
}

int skd_conv3x3_narrow2h_nhwc(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const void *wpack, float *out,
                              const float *residual, const float *conv_bias, const float *mean, const float *var,
                              const float *weight, const float *bias, float eps, int activation, float slope, int geometry,
                              skd_stream_t stream) {
  return run3<kNarrowTN, 2, kFp16>(B, H, W, Cin, Cout, dilation, x, wpack, out, residual, conv_bias, mean, var, weight, bias, eps,
                                   activation, slope, geometry, 1, stream);
}

int skd_conv3x3_split2h_s2_nhwc(int B, int H, int W, int Cin, int Cout, const float *x, const void *wpack, float *out,
                                const float *conv_bias, const float *mean, const float *var, const float *weight, const float *bias,
                                float eps, int activation, float slope, int geometry, skd_stream_t stream) {
  return run3_s2<2, kFp16>(B, H, W, Cin, Cout, x, wpack, out, conv_bias, mean, var, weight, bias, eps, activation, slope, geometry,
                           stream);
}

// include/skd_train2h.h: both fp16 two-plane images of a trained weight in one launch, and the data gradient on a scaled g.
int skd_conv3x3_split2h_pack_pair(int Cin, int Cout, const float *w, int64_t stride_n, int64_t stride_c, int64_t stride_y,
                                  int64_t stride_x, void *pack_fwd, int64_t fwd_bytes, void *pack_bwd, int64_t bwd_bytes,
                                  skd_stream_t stream) {
  return pack_pair3<kTN, 2, kFp16>(Cin, Cout, w, stride_n, stride_c, stride_y, stride_x, pack_fwd, fwd_bytes, pack_bwd, bwd_bytes, stream);
}

int skd_conv3x3_split2h_scaled_nhwc(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const void *wpack,
                                    float *out, const uint32_t *word, int geometry, skd_stream_t stream) {
  return run3_scaled(B, H, W, Cin, Cout, dilation, x, wpack, out, word, geometry, stream);
}

// include/skd_narrow.h: the 64-column form.
int skd_conv3x3_narrow_supported(int Cin, int Cout, int stride, int padding, int dilation, int groups) {
  return supported3<kNarrowTN>(Cin, Cout, stride, padding, dilation, groups);
}

int64_t skd_conv3x3_narrow_pack_bytes(int Cin, int Cout) { return pack_bytes3<kNarrowTN>(Cin, Cout); }

int skd_conv3x3_narrow_pack_pair(int Cin, int Cout, const float *w, int64_t stride_n, int64_t stride_c, int64_t stride_y,
                                 int64_t stride_x, void *pack_fwd, int64_t fwd_bytes, void *pack_bwd, int64_t bwd_bytes,
                                 skd_stream_t stream) {
  return pack_pair3<kNarrowTN>(Cin, Cout, w, stride_n, stride_c, stride_y, stride_x, pack_fwd, fwd_bytes, pack_bwd, bwd_bytes, stream);
}

int skd_conv3x3_narrow_nhwc(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const void *wpack, float *out,
                            const float *residual, const float *conv_bias, const float *mean, const float *var,
                            const float *weight, const float *bias, float eps, int activation, float slope, int geometry,
                            skd_stream_t stream) {
  return run3<kNarrowTN>(B, H, W, Cin, Cout, dilation, x, wpack, out, residual, conv_bias, mean, var, weight, bias, eps, activation,
                         slope, geometry, 1, stream);
}

// include/skd_bnstats.h: the training forward with the batch-norm statistics records from its epilogue (the finalize kernel
// that reads them: csrc/abn_nhwc.hip).
int64_t skd_conv3x3_bnstats_floats(int64_t M, int Cout) { return bnstats_floats(M, Cout); }

int skd_conv3x3_split_stats_nhwc(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const void *wpack, float *out,
                                 const float *conv_bias, int geometry, float *stats, int64_t stats_floats, skd_stream_t stream) {
  return run3_stats<kTN>(B, H, W, Cin, Cout, dilation, x, wpack, out, conv_bias, geometry, 3, stats, stats_floats, stream);
}

int skd_conv3x3_narrow_stats_nhwc(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const void *wpack,
                                  float *out, const float *conv_bias, int geometry, float *stats, int64_t stats_floats,
                                  skd_stream_t stream) {
  return run3_stats<kNarrowTN>(B, H, W, Cin, Cout, dilation, x, wpack, out, conv_bias, geometry, 1, stats, stats_floats, stream);
}

// include/skd_planes.h: the wide stride-1 frozen forward on the piece planes of its input.
int skd_conv3x3_split_planes_nhwc(int B, int H, int W, int Cin, int Cout, const void *planes_in, const void *wpack, float *out,
                                  const float *conv_bias, const float *mean, const float *var, const float *weight,
                                  const float *bias, float eps, int activation, float slope, int dilation, int geometry,
                                  skd_stream_t stream) {
  return run3_planes(B, H, W, Cin, Cout, dilation, planes_in, wpack, out, conv_bias, mean, var, weight, bias, eps, activation, slope,
                     geometry, stream);
}

// include/skd_stride2.h: the stride-2 frozen forward of the 128-column family.
int skd_conv3x3_split_s2_supported(int Cin, int Cout, int stride, int padding, int dilation, int groups) {
  return supported3_s2(Cin, Cout, stride, padding, dilation, groups);
}

int skd_conv3x3_split_s2_taps(int H, int W, int64_t m, int64_t *pixel, unsigned *mask) { return taps_s2(H, W, m, pixel, mask); }

int skd_conv3x3_split_s2_nhwc(int B, int H, int W, int Cin, int Cout, const float *x, const void *wpack, float *out,
                              const float *conv_bias, const float *mean, const float *var, const float *weight, const float *bias,
                              float eps, int activation, float slope, int pieces, int geometry, skd_stream_t stream) {
  if (pieces == 3)
    return run3_s2<3>(B, H, W, Cin, Cout, x, wpack, out, conv_bias, mean, var, weight, bias, eps, activation, slope, geometry, stream);
  if (pieces == 2)
    return run3_s2<2>(B, H, W, Cin, Cout, x, wpack, out, conv_bias, mean, var, weight, bias, eps, activation, slope, geometry, stream);
  return 0;
}

}  // extern "C"
