// conv_split_dev.hpp -- the split-operand bf16-MFMA GEMM core shared by conv1x1.hip (1x1 convolution = plain GEMM) and
// conv3x3.hip (3x3 convolution = implicit GEMM): the three-piece split, the LDS image, one K-tile of MFMAs, the epilogue of an
// accumulator block and the device's CU count.  Each is defined here once; what the core computes and why is documented at the
// top of conv1x1.hip.
#pragma once
#include <atomic>

#include "skd_common.hpp"

namespace skd {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// K-tile 16 = ONE k-step of the bf16 MFMA.  A stage of the LDS ring holds, per operand, three bf16 planes (the pieces of the
// split) of 128 rows x 16 k: 24,576 bytes, so that THREE workgroups (12 waves) still share a CU at K <= 256 (with the prologue's
// parameter table: 53,248 bytes each) and the split / prologue / epilogue of one tile hides behind two neighbours' MFMAs.
constexpr int kTM = 128, kTN = 128, kBK = 16, kMinWG = 3;
constexpr int kQK = kBK / 4;                               // float4 per panel row
constexpr int kRPP = kThreads / kQK;                       // panel rows covered by one pass of the workgroup (64)
constexpr int kRB = kTN / kRPP;                            // float4 of the B panel per thread and K-tile (2); A: TM / kRPP (2 or 1)
// LDS image of one piece of one operand, in 16-byte chunks (8 consecutive k of one row in bf16 = one lane's MFMA fragment):
//   chunk(h, row) = h * 128 + (row ^ 4 h),   h = k / 8
// so the 32 lanes of a fragment read's lane half fetch 512 contiguous bytes (ds_read_b128, conflict-free), and the XOR puts the
// 8-byte stores of the four threads that own one row's 16 k (two per h) on distinct banks within a store's 16-lane group.
// PIECES = how many bf16 pieces an operand is split into: 3 (six products, fp32 accuracy) everywhere but in the two-piece forms
// of include/skd_split2.h (PIECES = 2: a0 | a1, three products, a stage of 1024 chunks = 16,384 bytes).
constexpr int kPlaneChunks = 2 * 128;                      // one piece of one operand: 4 KB
constexpr int operand_chunks(int PIECES) { return PIECES * kPlaneChunks; }        // a0 | a1 | a2
constexpr int stage_chunks(int PIECES) { return 2 * operand_chunks(PIECES); }     // A | B: 1536 chunks = 24,576 bytes
constexpr size_t conv_lds(int PIECES) { return sizeof(uint4) * 2 * stage_chunks(PIECES); }
constexpr int kOperandChunks = operand_chunks(3), kStageChunks = stage_chunks(3);
constexpr size_t kConvLds = conv_lds(3);

__device__ __forceinline__ float inv_std_of(float var, float eps) { return (var != 0.f || eps != 0.f) ? 1.f / sqrtf(var + eps) : 0.f; }

// Two fp32 -> two bf16 in one dword, round to nearest even (v_cvt_pk_bf16_f32), and back (exact).
__device__ __forceinline__ uint32_t pack_bf16(float x, float y) {
  const f32x2 v = {x, y};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ float bf16_lo(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }

// The three-piece split of four consecutive k of one row: v = p0 + p1 + p2 with p0 = bf16(v), p1 = bf16(v - p0),
// p2 = bf16(v - p0 - p1); both residuals are exact in fp32 (Sterbenz-like: p0 agrees with v in its leading 8 bits).
__device__ __forceinline__ void split4(float4 v, uint2 &p0, uint2 &p1, uint2 &p2) {
  p0.x = pack_bf16(v.x, v.y);
  p0.y = pack_bf16(v.z, v.w);
  v.x -= bf16_lo(p0.x); v.y -= bf16_hi(p0.x); v.z -= bf16_lo(p0.y); v.w -= bf16_hi(p0.y);
  p1.x = pack_bf16(v.x, v.y);
  p1.y = pack_bf16(v.z, v.w);
  v.x -= bf16_lo(p1.x); v.y -= bf16_hi(p1.x); v.z -= bf16_lo(p1.y); v.w -= bf16_hi(p1.y);
  p2.x = pack_bf16(v.x, v.y);
  p2.y = pack_bf16(v.z, v.w);
}
// The two-piece split: the first two of those pieces, the second residual v - p0 - p1 dropped (include/skd_split2.h).
__device__ __forceinline__ void split4(float4 v, uint2 &p0, uint2 &p1) {
  p0.x = pack_bf16(v.x, v.y);
  p0.y = pack_bf16(v.z, v.w);
  v.x -= bf16_lo(p0.x); v.y -= bf16_hi(p0.x); v.z -= bf16_lo(p0.y); v.w -= bf16_hi(p0.y);
  p1.x = pack_bf16(v.x, v.y);
  p1.y = pack_bf16(v.z, v.w);
}
// The piece FORMAT, beside PIECES: kBf16 everywhere but in the forms of include/skd_split2h.h, which cut an operand into two
// FP16 pieces (PIECES = 2 only).  An fp16 piece carries 11 significant bits, so two carry 22 -- but fp16's exponent is narrow: the
// residual v - fp16(v), about 2^-11 |v|, would be an fp16 subnormal for every |v| < 0.125.  It is therefore SCALED by 2^11 (exact)
// before it is converted: v ~ p0 + 2^-11 p1.  The products a0 b1 and a1 b0 then carry the factor 2^11 and go into `lo`, a0 b0
// into `hi` (tile_mma), and the epilogue joins the sets as hi + 2^-11 lo (join_sets).  Both formats are 16-bit: the LDS image, the
// chunk map, k_loop and the stage size are the bf16 two-piece ones.
constexpr int kBf16 = 0, kFp16 = 1;
constexpr float kResidualScale = 2048.f, kLoScale = 1.f / 2048.f;      // 2^11, 2^-11
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
// Two fp32 -> two fp16 in one dword, round to nearest even (v_cvt_pk_f16_f32), and back (exact).
__device__ __forceinline__ uint32_t pack_f16(float x, float y) {
  const f32x2 v = {x, y};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2));
}
__device__ __forceinline__ f32x2 unpack_f16(uint32_t u) { return __builtin_convertvector(__builtin_bit_cast(f16x2, u), f32x2); }
// The two fp16 pieces of four consecutive k of one row: p0 = fp16(v), p1 = fp16((v - p0) * 2^11).  The residual is exact in fp32
// (p0 agrees with v in its leading 11 bits, or is a subnormal multiple of 2^-24 below a v whose own unit is finer), and so is the
// scaling.  |v| > 65504 rounds p0 to infinity and p1 to the opposite infinity: every product that reads the pair is NaN.
__device__ __forceinline__ void split4_f16(float4 v, uint2 &p0, uint2 &p1) {
  p0.x = pack_f16(v.x, v.y);
  p0.y = pack_f16(v.z, v.w);
  const f32x2 a = unpack_f16(p0.x), b = unpack_f16(p0.y);
  p1.x = pack_f16((v.x - a[0]) * kResidualScale, (v.y - a[1]) * kResidualScale);
  p1.y = pack_f16((v.z - b[0]) * kResidualScale, (v.w - b[1]) * kResidualScale);
}
// The SCALE of a gradient tensor's fp16 split (include/skd_train2h.h): `word` is the largest bits & 0x7fffffff of the tensor
// (csrc/scale_word.hip).  s = 2^k puts a finite amax >= 2^-112 into [2^14, 2^15), k = clamp(14 - e, -126, 126) with e the
// word's unbiased exponent (-127 for an fp32 subnormal); s and inv = 2^-k are normal fp32, so both multiplications are exact
// while nothing leaves the normal range.  A zero or non-finite word gives s = inv = 1: an infinity or a NaN is split as it is.
__host__ __device__ inline void scale_of(uint32_t word, float &s, float &inv) {
  int k = 0;
  if (word != 0u && word < 0x7f800000u) {
    k = 14 - ((int)(word >> 23) - 127);
    k = k < -126 ? -126 : (k > 126 ? 126 : k);
  }
  const uint32_t sb = (uint32_t)(127 + k) << 23, ib = (uint32_t)(127 - k) << 23;
  s = __builtin_bit_cast(float, sb);
  inv = __builtin_bit_cast(float, ib);
}
__device__ __forceinline__ float4 scaled(float4 v, float s) { return make_float4(v.x * s, v.y * s, v.z * s, v.w * s); }
// ... written to the thread's 8-byte slot `dst` of the PIECES planes of one operand's LDS image
template <int PIECES = 3, int FMT = kBf16>
__device__ __forceinline__ void split_store(float4 v, uint2 *dst) {
  static_assert(PIECES == 2 || PIECES == 3, "two or three pieces");
  static_assert(FMT == kBf16 || (FMT == kFp16 && PIECES == 2), "fp16 pieces: two of them");
  uint2 p0, p1, p2;
  if constexpr (FMT == kFp16) split4_f16(v, p0, p1);
  else if constexpr (PIECES == 3) split4(v, p0, p1, p2);
  else split4(v, p0, p1);
  dst[0] = p0;
  dst[2 * kPlaneChunks] = p1;
  if constexpr (PIECES == 3) dst[4 * kPlaneChunks] = p2;
}
// ... the same for an image whose pieces lie `plane` 8-byte slots apart (a TN = 64 B image: 2 * 128)
__device__ __forceinline__ void split_store(float4 v, uint2 *dst, int plane) {
  uint2 p0, p1, p2;
  split4(v, p0, p1, p2);
  dst[0] = p0;
  dst[plane] = p1;
  dst[2 * plane] = p2;
}

// PIECE PLANES (include/skd_planes.h): an (M, C) fp32 activation map stored as its three bf16 pieces, C % 16 == 0, so that a
// consumer stages a K-tile without split4.  THE layout, the one function every kernel and the host entry skd_planes_offset use:
// byte offset of piece `piece` of element (row, channel c).  Interleaved per QUAD of four channels: a row's four consecutive k
// are 24 contiguous bytes (piece 0 | piece 1 | piece 2, 8 bytes each), a row's quads follow each other, rows follow each other:
// 6 C bytes per row, 6 M C in all, no padding (so M does not enter the map).  A thread of the K loop owns exactly one quad of a
// row: its three pieces are one 16-byte and one 8-byte load at 8-byte alignment, and the four threads of a row read the K-tile's
// 96 bytes.  (Interleaved per K-tile -- 32 bytes of each piece, three separate loads per thread -- measured no better:
// profiles/r31_planes_isolated.md.)
// The map is affine in row * C + (c rounded down to 4), so it is also defined for a `c` outside 0 .. C - 1 that is a multiple of
// 4 (channel c + C of a row is channel c of the next row); conv3x3.hip steps its tap cursor that way.
__host__ __device__ inline int64_t planes_offset(int64_t M, int C, int64_t row, int64_t c, int piece) {
  (void)M;
  return (row * C + (c & ~(int64_t)3)) * 6 + piece * 8 + (c & 3) * 2;
}
constexpr int64_t planes_bytes(int64_t M, int C) { return M * C * 6; }

// 8-byte slot, in uint2 units, of (row `row` < 64 + what the caller adds, k quad `gkq` = 0, 4, 8, 12) inside a plane; rows 64
// apart are 128 slots apart.
__device__ __forceinline__ int plane_slot(int row, int gkq) {
  const int kh = gkq >> 3;                          // which 8-k half of the K-tile the quad belongs to
  return 2 * (kh * 128 + (row ^ (kh * 4))) + ((gkq >> 2) & 1);
}

// One K-tile out of LDS: 3 (WM + 2) conflict-free ds_read_b128 (the lane's 8 k of its row, per piece and 32-row block) feed
// 6 * 2 WM bf16 MFMAs: the six products a_i b_j with i + j <= 2, the three smallest first, the four accumulator blocks of the
// wave in turn inside every product (no MFMA waits for its predecessor's result).
// The four waves of a TM x TN tile (TN = 128 or 64 columns): TN / 64 across N, the others across M, each a wave tile of
// (TM / waves across M) x 64 = WM x 2 blocks of 32 x 32 -- waves 2 x 2 and WM = TM / 64 for TN = 128, waves 4 x 1 and WM = TM / 128
// for TN = 64.  The B image has TN rows: chunk(h, row) = h * TN + (row ^ 4 h), 2 TN chunks per piece.
// SWAP: the piece tables change sides -- product t is a_kPB[t] b_kPA[t] -- for a caller whose operands have changed sides
// (conv3x3_wgrad.hip's 128 x 64 form: x is A, g is B) and whose sums must see the pieces in the other caller's order.
// The five products below a0 b0 go into `lo`, a0 b0 into `hi`.  One accumulator for both (conv1x1.hip: lo and hi are the same
// array) rounds six times per 16 k at the magnitude of the running sum; two accumulators (conv3x3.hip, K up to 18432) round
// once per 16 k at that magnitude and five times at 2^-8 of it, and are added in the epilogue.
constexpr int waves_m(int TN) { return 4 / (TN / 64); }                           // waves across M
constexpr int wave_blocks_m(int TM, int TN) { return TM / waves_m(TN) / 32; }       // WM

// PIECES = 2 (include/skd_split2.h): 2 (WM + 2) reads feed 3 * 2 WM MFMAs, the three products a0 b1, a1 b0 (into `lo`), a0 b0
// (into `hi`): the same two-set rule.
template <int PIECES>
struct Products;
template <>
struct Products<3> {
  static constexpr int kN = 6, kPA[6] = {0, 1, 2, 0, 1, 0}, kPB[6] = {2, 1, 0, 1, 0, 0};
};
template <>
struct Products<2> {
  static constexpr int kN = 3, kPA[3] = {0, 1, 0}, kPB[3] = {1, 0, 0};
};

// The fragment type and the MFMA of a piece format: both take the same cycles on gfx950.
template <int FMT>
struct PieceMma;
template <>
struct PieceMma<kBf16> {
  typedef bf16x8 Frag;
  static __device__ __forceinline__ f32x16 mma(Frag a, Frag b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
template <>
struct PieceMma<kFp16> {
  typedef f16x8 Frag;
  static __device__ __forceinline__ f32x16 mma(Frag a, Frag b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};

template <int TM, int TN = kTN, bool SWAP = false, int PIECES = 3, int FMT = kBf16>
__device__ __forceinline__ void tile_mma(const uint4 *stage, f32x16 (&lo)[wave_blocks_m(TM, TN)][2],
                                         f32x16 (&hi)[wave_blocks_m(TM, TN)][2]) {
  constexpr int WM = wave_blocks_m(TM, TN);
  static_assert((TN == 64 || TN == 128) && WM >= 1, "one or two of the four waves across N, a wave tile of at least 32 rows");
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  const int wi = (wid / (TN / 64)) * (TM / waves_m(TN)), wj = (wid % (TN / 64)) * 64;
  const int half = lane >> 5, r = lane & 31;
  const uint4 *pa = stage + half * 128 + ((wi + r) ^ (half * 4));
  const uint4 *pb = stage + operand_chunks(PIECES) + half * TN + ((wj + r) ^ (half * 4));
  static_assert(FMT == kBf16 || PIECES == 2, "fp16 pieces: two of them");
  typedef typename PieceMma<FMT>::Frag Frag;
  Frag a[WM][PIECES], b[2][PIECES];
#pragma unroll
  for (int p = 0; p < PIECES; ++p) {
#pragma unroll
    for (int i = 0; i < WM; ++i) a[i][p] = __builtin_bit_cast(Frag, pa[p * kPlaneChunks + 32 * i]);
#pragma unroll
    for (int j = 0; j < 2; ++j) b[j][p] = __builtin_bit_cast(Frag, pb[p * 2 * TN + 32 * j]);
  }
  typedef Products<PIECES> P;
#pragma unroll
  for (int t = 0; t < P::kN; ++t)
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        f32x16 &dst = t < P::kN - 1 ? lo[i][j] : hi[i][j];
        dst = PieceMma<FMT>::mma(a[i][SWAP ? P::kPB[t] : P::kPA[t]], b[j][SWAP ? P::kPA[t] : P::kPB[t]], dst);
      }
}
template <int TM, int PIECES = 3>
__device__ __forceinline__ void tile_mma(const uint4 *stage, f32x16 (&acc)[TM / 64][2]) {
  tile_mma<TM, kTN, false, PIECES>(stage, acc, acc);
}
// The two accumulator sets of one block joined in front of the epilogue: hi + lo, or -- fp16 pieces, whose `lo` products carry the
// residual's factor 2^11 -- hi + 2^-11 lo as one fma per element.
template <int FMT = kBf16>
__device__ __forceinline__ void join_sets(f32x16 &hi, const f32x16 &lo) {
#pragma unroll
  for (int q = 0; q < 16; ++q) hi[q] = FMT == kFp16 ? __builtin_fmaf(lo[q], kLoScale, hi[q]) : hi[q] + lo[q];
}

// The K loop of one output tile through the two LDS stages, shared by both kernels.  `Tile` supplies
//   Stg                       the staging registers of one K-tile (every member written by load)
//   load(Stg &, kt)           issue the global loads of tile kt (called for kt = 0, 1, 2, ... in order, each once)
//   store(const Stg &, s, kt) prologue (if any) + split of tile kt's staging set, written to LDS stage s
//   mma(s)                    tile_mma on LDS stage s
// DEPTH = how many K-tiles the global loads run ahead of the MFMAs.
//   2: trip kt issues the loads of tile kt + 2, then splits and stores tile kt + 1 -- loaded during trip kt - 1, so it has had a
//      whole trip of every co-resident wave to land and the wait in front of the split is a counted vmcnt that leaves the loads
//      just issued in flight -- into the stage that every wave left at the barrier ending trip kt - 1, then runs the MFMAs of tile kt.
//   1: the loop before round 15: trip kt loads tile kt + 1, runs the MFMAs of tile kt, then splits and stores tile kt + 1.
// Either way: one barrier per trip, tile order and MFMA order as written, no load for a tile index >= nk.  The loop is unrolled by
// two trips so that the two staging sets and the two stages are named, not indexed: nothing is copied at the back edge.  Its
// steady state (STEADY: the caller knows kt + 2 < nk) has no branch, so the compiler's count of the loads in flight is exact
// there (a guard inside the loop made it wait for the loads it had just issued); the last one to three trips carry the guards.
// FENCE: the trip's MFMAs (and their fragment reads) are scheduled behind its split and stores, not among them.  Set by the
// two-piece 1x1 kernel without prologue alone, whose fragment reads the scheduler otherwise hoists above the split at the price of
// 8 registers more than its three-piece twin takes (profiles/r25_kernel_resources.md).
template <int DEPTH, bool STEADY, bool FENCE, class Tile>
__device__ __forceinline__ void k_trip(Tile &t, typename Tile::Stg &fill, typename Tile::Stg &next, const uint4 *cur, uint4 *nxt,
                                       int kt, int nk) {
  static_assert(DEPTH == 1 || DEPTH == 2, "load look-ahead of one or two K-tiles");
  if (DEPTH == 2) {
    if (STEADY || kt + 2 < nk) t.load(fill, kt + 2);       // `fill` held tile kt: stored one trip ago
    if (STEADY || kt + 1 < nk) t.store(next, nxt, kt + 1);
    if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);
    t.mma(cur);
  } else {
    if (STEADY || kt + 1 < nk) t.load(next, kt + 1);
    t.mma(cur);
    if (STEADY || kt + 1 < nk) t.store(next, nxt, kt + 1);
  }
  __syncthreads();
}
template <int DEPTH, int PIECES = 3, bool FENCE = false, class Tile>
__device__ __forceinline__ void k_loop(Tile &t, int nk, uint4 *lds) {
  typename Tile::Stg s0, s1;                     // tiles of even / odd index
  uint4 *const l0 = lds, *const l1 = lds + stage_chunks(PIECES);
  t.load(s0, 0);
  if (DEPTH == 2 && nk > 1) t.load(s1, 1);
  t.store(s0, l0, 0);
  __syncthreads();
  int kt = 0;
  for (; kt + 3 < nk; kt += 2) {
    k_trip<DEPTH, true, FENCE>(t, s0, s1, l0, l1, kt, nk);
    k_trip<DEPTH, true, FENCE>(t, s1, s0, l1, l0, kt + 1, nk);
  }
  k_trip<DEPTH, false, FENCE>(t, s0, s1, l0, l1, kt, nk);                        // one to three trips left, kt even
  if (kt + 1 < nk) k_trip<DEPTH, false, FENCE>(t, s1, s0, l1, l0, kt + 1, nk);
  if (kt + 2 < nk) k_trip<DEPTH, false, FENCE>(t, s0, s1, l0, l1, kt + 2, nk);
}

// Epilogue of one 32 x 32 accumulator block: rows row0 + frag_row(q), column col.  FULL: every row of the tile exists (all
// but the last row tile) -- no per-element branches, and the sixteen residual loads are issued together before the first
// use (round 2 interleaved load -> wait -> store per element behind a branch: 64 serialised HBM round trips per lane).
// NT: the residual is read and the output written with the non-temporal hint (round 6).  For WIDE outputs (the super-tile order,
// K = 512 / N = 2048) the 554 MB residual + output stream of a launch shares each XCD's 4 MB L2 with the operands it is trying to
// keep (2 MB of activations per panel group, 1 MB of weights per chunk) and evicts them: counters showed the activations fetched
// ~4 x (617 MB read for 350 MB algorithmic, profiles/r05j_pmc.json case 135).  Neither stream is read again by this kernel.
template <int ACT, bool HAS_RES, bool FULL, bool NT>
__device__ __forceinline__ void store_block(const f32x16 &acc, const float *__restrict__ R, float *__restrict__ Y, int64_t row0,
                                            int col, int64_t M, int N, float mu, float is, float ga, float be, float slope) {
  const int lane = threadIdx.x & (kWave - 1);
  float rv[16];
  int64_t off[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int64_t row = row0 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
    off[q] = row * N + col;
    rv[q] = 0.f;
    if (HAS_RES && (FULL || row < M)) rv[q] = NT ? __builtin_nontemporal_load(R + off[q]) : R[off[q]];
  }
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int64_t row = row0 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
    float z = ((acc[q] - mu) * is) * ga + be;                 // bn.cu:158-159
    if (HAS_RES) z += rv[q];
    if (ACT == SKD_ACT_RELU) z = z < 0.f ? 0.f : z;
    if (ACT == SKD_ACT_LEAKY_RELU) z = z < 0.f ? z * slope : z;
    if (FULL || row < M) {
      if (NT) __builtin_nontemporal_store(z, Y + off[q]);
      else Y[off[q]] = z;
    }
  }
}

// n / d and n % d for n < 2^31 with rcp = reciprocal32(d) = floor(2^32 / d) (2^32 - 1 for d = 1): the multiply-high is the
// quotient or one short.
__device__ __forceinline__ void divmod(unsigned n, unsigned d, unsigned rcp, unsigned &q, unsigned &r) {
  q = __umulhi(n, rcp);
  r = n - q * d;
  if (r >= d) {
    ++q;
    r -= d;
  }
}
inline unsigned reciprocal32(unsigned d) { return d == 1 ? 0xffffffffu : (unsigned)((1ull << 32) / d); }

// Compute units of the device that `st` belongs to (0: unknown).  Queried once per device; the table is atomic because the
// teacher stream and the main stream may reach their first launch from different host threads (a second query stores the same value).
inline int cu_count(hipStream_t st) {
  static std::atomic<int> cus[64];
  int dev = -1;
  if (hipStreamGetDevice(st, &dev) != hipSuccess) {
    (void)hipGetLastError();             // not an error of the launch that follows
    if (hipGetDevice(&dev) != hipSuccess) return 0;
  }
  if (dev < 0 || dev >= 64) return 0;
  int n = cus[dev].load(std::memory_order_relaxed);
  if (n == 0 && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
    cus[dev].store(n, std::memory_order_relaxed);
  return n > 0 ? n : 0;
}

}  // namespace skd
