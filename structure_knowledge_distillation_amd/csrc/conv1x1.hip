// conv1x1.hip -- 1x1 convolution + eval-mode InPlace-ABN (+ residual) + activation as ONE GEMM for gfx950: fp32 in, fp32 out,
// the products on the bf16 MFMA through a three-piece operand split.
//
// The frozen teacher (ResNet101, eval, no grad) spends 3.9 ms per step in its BatchNorm passes although every one of
// them follows a convolution whose output it merely rescales (networks/pspnet_combine.py:65-84: conv1 -> bn1 -> relu,
// conv3 -> bn3 -> + residual -> relu).  For the 1x1 convolutions -- in channels-last memory a plain GEMM
//     Y[M][N] = act( ((X[M][K] . W[N][K]^T - mean[n]) * invstd[n]) * gamma[n] + beta[n]  [+ R[M][N]] ),   M = B*H*W
// -- the normalisation, the residual add and the ReLU move into the epilogue here: the convolution output is written
// once, already activated, and the separate 8 / 12 byte-per-element ABN pass disappears.  The
// epilogue evaluates exactly the formula of abn_apply (bn.cu:146-159 + ReLU) on the fp32 accumulator, so nothing is folded
// into the weights and checkpoints / state-dict semantics are untouched.
//
// Matrix core.  gfx950 runs v_mfma_f32_32x32x2_f32 at 1/16 of the bf16 MFMA rate and has no xf32, so the fp32 product is built
// from bf16 MFMAs.  Every fp32 operand a (after the prologue, where there is one) is written as a0 + a1 + a2 on its way from
// the global-load staging registers into LDS:
//     a0 = bf16(a),  a1 = bf16(a - a0),  a2 = bf16(a - a0 - a1)        round to nearest even (v_cvt_pk_bf16_f32),
// both residuals exact in fp32 -- three pieces of 8 significant bits carry the 24 of an fp32 value.  The product is the six
// terms with i + j <= 2 (a0 b2, a1 b1, a2 b0, a0 b1, a1 b0, a0 b0: the smallest first), each one
// v_mfma_f32_32x32x16_bf16 per 32 x 32 block and 16 k, all into ONE fp32 accumulator.  The dropped terms a1 b2, a2 b1, a2 b2
// are below 2^-23 |a b|; measured against the double-precision oracle the result is within 4 x of the exact fp32 fma chain
// the fp32 MFMA gave (tests/test_conv1x1_split_gpu.py, profiles/r11_conv1x1_split_accuracy.md) and exact on integer data whose
// sums fit fp32.  At the reduce / down-sample shapes (K up to 2048, and 4096) it is within 1.5 x of the library fp32 GEMM's error and
// below 2e-6 of the output's largest magnitude (1.55e-6 at K = 4096: profiles/r13_conv1x1_reduce_accuracy.md) -- one accumulator
// is enough here, unlike conv3x3.hip.  Six bf16 MFMAs of 32 cycles replace eight fp32 MFMAs of 64 per 16 k of a block: 2.67 x less matrix-pipe time.
// Outside the normal range: a finite |a| above the largest bf16 (about 3.39e38) rounds a0 to infinity and an infinite a has
// an undefined residual, so in both cases the affected outputs are NaN where the fp32 chain would have given +-inf or a finite
// value (a * 0); a NaN input gives NaN outputs as before.  Pieces below the fp32 normal range (|a| < 2^-102 or so) may be
// flushed: an absolute error below 2^-126 |b|.  The teacher's activations and weights are nowhere near either end.
//
// Kernel: 128 x 128 output tile per 256-thread workgroup (4 waves, each 64 x 64 = 2 x 2 blocks of 32 x 32, 64 accumulator
// registers), K streamed in tiles of 16 through a double-buffered LDS ring.  Both operands are K-contiguous in memory
// (activations channels-last, weights (N, K, 1, 1)).  LDS holds three bf16 planes per operand; a lane's fragment for one piece
// and block is the 8 consecutive k of its row = one ds_read_b128 (lanes 0-31: k 0-7, lanes 32-63: k 8-15), laid out so that a
// lane half reads 512 contiguous bytes (see kPlaneChunks).  Per K-tile and wave: 12 ds_read_b128 -> 24 MFMAs (768 matrix-pipe
// cycles); per K-tile and thread 4 global float4 loads, the split (about 5.5 VALU instructions per element) and 12
// ds_write_b64.  The loads run TWO K-tiles ahead of the MFMAs and the split one (k_loop in conv_split_dev.hpp: loads of tile
// kt + 2, then the split of tile kt + 1 behind a counted vmcnt, then the MFMAs of tile kt; round 15, DESIGN.md 9.9: 2-7 % per
// launch over one tile of look-ahead, bit-identical).  48 KB of LDS per workgroup (+ 16 bytes per input channel for the
// prologue's table), 154 VGPRs without and 168 with the prologue, no scratch
// -> 3 workgroups (3 waves per SIMD, limit 168) per CU up to K = 256 with the prologue, 2 at K = 512.
// The fp32-MFMA core this replaces lives on as variant 0 of tools/gemm_lab_kernels.hip for comparison.
// Bound: per launch the larger of the HBM traffic (4*M*K + 4*N*K + 4*M*N (+ 4*M*N residual) bytes) and 6 bf16 products
// (12*M*N*K flops at the bf16-MFMA peak); algorithmic flops stay 2*M*N*K, which is what bench.py's roofline leg reports against
// the fp32-MFMA peak of 157.3 TFLOP/s (its fraction may therefore exceed 1).
#include <stdio.h>
#include <stdlib.h>

#include "conv_split_dev.hpp"
#include "skd_planes.h"
#include "skd_split2.h"
#include "skd_split2h.h"

namespace skd {
namespace {

// The core (split, LDS image, MFMA tile, block epilogue) is conv_split_dev.hpp, shared with conv3x3.hip.
constexpr int kProMaxK = 512;                             // prologue form: the (4, K) parameter table rides in LDS (<= 8 KB)

constexpr int kDepth1x1 = 2;                             // K-tiles of load look-ahead (k_loop, conv_split_dev.hpp)

// Per K-tile a thread moves two (TM = 64: one) float4 of the A panel (rows t/4 + 64h, k quad t%4) and two of the B panel from
// global memory to LDS.  k_loop issues the loads of tile kt + 2 at the top of trip kt, then runs the prologue, the split and the
// LDS stores of tile kt + 1 (loaded a whole trip earlier) in front of the trip's MFMAs; two named staging sets, none copied.
template <int TM>          // TM = rows of the output tile: 128, or 64 for the tiles of a launch's last, partial round (see the kernel)
struct Staging {
  float4 a[TM / kRPP], b[kRB];
};
struct ProParams {         // PRO: the k quad's mean / invstd / gamma / beta of the BatchNorm applied to A on the way in
  float4 pm, pi, pg, pb;   // (kept apart from Staging: a struct with members that one instantiation never writes stayed in scratch)
};

template <bool PRO, int TM>
__device__ __forceinline__ void stage_load(Staging<TM> &s, const float *__restrict__ X, const float *__restrict__ Wt, int k0,
                                           int gkq, const int64_t (&arow)[TM / kRPP], int64_t wrow0, int K) {
  const float *xa = X + k0 + gkq, *wb = Wt + k0 + gkq;
#pragma unroll
  for (int h = 0; h < TM / kRPP; ++h) s.a[h] = *reinterpret_cast<const float4 *>(xa + arow[h]);
#pragma unroll
  for (int h = 0; h < kRB; ++h) s.b[h] = *reinterpret_cast<const float4 *>(wb + wrow0 + (int64_t)(kRPP * h) * K);
}

// relu(bn(x)) with the expression of abn_apply (bn.cu:146-159 + ReLU): ((x - mean) * invstd) * gamma + beta
__device__ __forceinline__ float pro_one(float x, float m, float is, float g, float b) {
  const float z = __builtin_fmaf((x - m) * is, g, b);
  return z < 0.f ? 0.f : z;
}

// `srow`: this thread's 8-byte slot inside a plane, in uint2 units (see conv1x1_tile); rows 64 apart are 128 slots apart.
template <bool PRO, int TM, int PIECES, int FMT = kBf16>
__device__ __forceinline__ void stage_store(const Staging<TM> &s, uint4 *stage, int srow, const float *ptab, int K, int kq) {
  constexpr int kRA = TM / kRPP;
  uint2 *sa = reinterpret_cast<uint2 *>(stage) + srow, *sb = reinterpret_cast<uint2 *>(stage + operand_chunks(PIECES)) + srow;
  if (PRO) {   // ptab (LDS copy of ppack): mean | invstd | gamma | beta, each K floats; kq = first of this thread's four k
    ProParams pp;
    pp.pm = *reinterpret_cast<const float4 *>(ptab + kq);
    pp.pi = *reinterpret_cast<const float4 *>(ptab + K + kq);
    pp.pg = *reinterpret_cast<const float4 *>(ptab + 2 * K + kq);
    pp.pb = *reinterpret_cast<const float4 *>(ptab + 3 * K + kq);
#pragma unroll
    for (int h = 0; h < kRA; ++h) {
      float4 v = s.a[h];
      v.x = pro_one(v.x, pp.pm.x, pp.pi.x, pp.pg.x, pp.pb.x);
      v.y = pro_one(v.y, pp.pm.y, pp.pi.y, pp.pg.y, pp.pb.y);
      v.z = pro_one(v.z, pp.pm.z, pp.pi.z, pp.pg.z, pp.pb.z);
      v.w = pro_one(v.w, pp.pm.w, pp.pi.w, pp.pg.w, pp.pb.w);
      split_store<PIECES, FMT>(v, sa + 2 * kRPP * h);
    }
  } else {
#pragma unroll
    for (int h = 0; h < kRA; ++h) split_store<PIECES, FMT>(s.a[h], sa + 2 * kRPP * h);
  }
#pragma unroll
  for (int h = 0; h < kRB; ++h) split_store<PIECES, FMT>(s.b[h], sb + 2 * kRPP * h);
}

// The accumulator set of the products below a0 b0.  bf16 pieces: the one set `acc` itself (lo and hi are the same array, see
// tile_mma).  fp16 pieces (include/skd_split2h.h): a set of its own -- those products carry the factor 2^11 -- of 32 WM registers.
template <int WM, int FMT>
struct LowSet {
  typedef f32x16 Set[WM][2];
  __device__ __forceinline__ Set &of(Set &acc) { return acc; }
};
template <int WM>
struct LowSet<WM, kFp16> {
  typedef f32x16 Set[WM][2];
  Set v;
  __device__ __forceinline__ Set &of(Set &) { return v; }
};

// What k_loop (conv_split_dev.hpp) needs of a tile of this kernel.
template <bool PRO, int TM, int PIECES = 3, int FMT = kBf16>
struct Tile1 {
  typedef Staging<TM> Stg;
  const float *__restrict__ X, *__restrict__ Wt;
  const float *ptab;
  int K, gkq, srow;
  int64_t wrow0, arow[TM / kRPP];
  f32x16 (&low)[TM / 64][2], (&acc)[TM / 64][2];
  __device__ __forceinline__ void load(Stg &s, int kt) const { stage_load<PRO, TM>(s, X, Wt, kt * kBK, gkq, arow, wrow0, K); }
  __device__ __forceinline__ void store(const Stg &s, uint4 *stage, int kt) const {
    stage_store<PRO, TM, PIECES, FMT>(s, stage, srow, ptab, K, kt * kBK + gkq);
  }
  __device__ __forceinline__ void mma(const uint4 *stage) const { tile_mma<TM, kTN, false, PIECES, FMT>(stage, low, acc); }
};

// PLANES (include/skd_planes.h): the epilogue of one 32 x 32 accumulator block that writes the three bf16 pieces of
// act(bn(acc)) -- store_block's fp32 value, the same expression -- into the piece planes of an (M, N) map (planes_offset,
// conv_split_dev.hpp) and no fp32 output.  A lane holds one column of sixteen rows, and neighbouring columns' pieces are
// neighbouring bf16, so lanes l and l ^ 1 trade every other row first: the even lane keeps rows q = 0, 2, ... of both columns, the
// odd lane rows q = 1, 3, ...; a lane then splits eight column pairs (pack_bf16 on the pair, as split4 does on its quads) and
// issues 24 dword stores instead of 48 two-byte ones.  The pieces of a value do not depend on its neighbour, so every element is
// split4's bit for bit.  The exchange runs on every lane; only the stores look at M.
template <int ACT, bool FULL>
__device__ __forceinline__ void store_block_planes(const f32x16 &acc, unsigned char *__restrict__ P, int64_t row0, int col,
                                                   int64_t M, int N, float mu, float is, float ga, float be, float slope) {
  const int lane = threadIdx.x & (kWave - 1), odd = lane & 1;
  float z[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    z[q] = ((acc[q] - mu) * is) * ga + be;                    // bn.cu:158-159, as store_block
    if (ACT == SKD_ACT_RELU) z[q] = z[q] < 0.f ? 0.f : z[q];
    if (ACT == SKD_ACT_LEAKY_RELU) z[q] = z[q] < 0.f ? z[q] * slope : z[q];
  }
#pragma unroll
  for (int q = 0; q < 16; q += 2) {
    const float got = __shfl_xor(odd ? z[q] : z[q + 1], 1, kWave);
    float lo = odd ? got : z[q], hi = odd ? z[q + 1] : got;   // columns col & ~1 and col | 1 of row q (even lane) / q + 1 (odd lane)
    const int qq = q + odd;
    const int64_t row = row0 + (qq & 3) + 8 * (qq >> 2) + 4 * (lane >> 5);
    const uint32_t p0 = pack_bf16(lo, hi);
    lo -= bf16_lo(p0); hi -= bf16_hi(p0);
    const uint32_t p1 = pack_bf16(lo, hi);
    lo -= bf16_lo(p1); hi -= bf16_hi(p1);
    const uint32_t p2 = pack_bf16(lo, hi);
    if (FULL || row < M) {
      *reinterpret_cast<uint32_t *>(P + planes_offset(M, N, row, col & ~1, 0)) = p0;
      *reinterpret_cast<uint32_t *>(P + planes_offset(M, N, row, col & ~1, 1)) = p1;
      *reinterpret_cast<uint32_t *>(P + planes_offset(M, N, row, col & ~1, 2)) = p2;
    }
  }
}

// One output tile of TM x 128: K loop through the double-buffered LDS ring, then the epilogue.  PLANES: Y is the piece-plane
// allocation of the (M, N) output and the epilogue is store_block_planes (no residual, no prologue, three pieces).
template <int TM, int ACT, bool HAS_RES, bool PRO, bool NT, int PIECES = 3, bool PLANES = false, int FMT = kBf16>
__device__ __forceinline__ void conv1x1_tile(const float *__restrict__ X, const float *__restrict__ Wt, const float *__restrict__ R,
                                             float *__restrict__ Y, const float *__restrict__ mean, const float *__restrict__ var,
                                             const float *__restrict__ weight, const float *__restrict__ bias,
                                             const float *__restrict__ ppack, float eps, float slope, int64_t M, int K, int N,
                                             int64_t m0, int n0, uint4 *lds) {
  constexpr int WM = TM / 64, kRA = TM / kRPP;
  f32x16 acc[WM][2];
#pragma unroll
  for (int i = 0; i < WM; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;
  LowSet<WM, FMT> lowset;
  f32x16 (&low)[WM][2] = lowset.of(acc);
  if constexpr (FMT == kFp16) {
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q) low[i][j][q] = 0.f;
  }
  const int nk = K / kBK;
  const int gt = threadIdx.x, grow = gt / kQK, gkq = (gt % kQK) * 4;
  const int srow = plane_slot(grow, gkq);           // 8-byte slot of (row grow, k quad) inside a plane
  int64_t arow[kRA];   // rows beyond the matrix are clamped (loaded, multiplied, never stored)
#pragma unroll
  for (int h = 0; h < kRA; ++h) {
    const int64_t m = m0 + grow + kRPP * h;
    arow[h] = (m > M - 1 ? M - 1 : m) * K;
  }
  const int64_t wrow0 = (int64_t)(n0 + grow) * K;
  float *ptab = reinterpret_cast<float *>(lds + 2 * stage_chunks(PIECES));   // PRO: the (4, K) parameter table, K <= kProMaxK
  if (PRO) {
    for (int i = gt * 4; i < 4 * K; i += kThreads * 4) *reinterpret_cast<float4 *>(ptab + i) = *reinterpret_cast<const float4 *>(ppack + i);
    __syncthreads();
  }
  Tile1<PRO, TM, PIECES, FMT> tile = {X, Wt, ptab, K, gkq, srow, wrow0, {}, low, acc};
#pragma unroll
  for (int h = 0; h < kRA; ++h) tile.arow[h] = arow[h];
  k_loop<kDepth1x1, PIECES, PIECES == 2 && !PRO && FMT == kBf16>(tile, nk, lds);
  // ---- epilogue: the eval-mode InPlace-ABN formula on the accumulator (+ residual) + activation ----
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  const int wi = (wid >> 1) * (TM / 2), wj = (wid & 1) * 64;
  const bool full = m0 + TM <= M;
#pragma unroll
  for (int bj = 0; bj < 2; ++bj) {
    const int col = n0 + wj + bj * 32 + (lane & 31);
    const float mu = mean[col], is = inv_std_of(var[col], eps);
    const float ga = weight != nullptr ? fabsf(weight[col]) + eps : 1.f;     // bn.cu:153
    const float be = bias != nullptr ? bias[col] : 0.f;
#pragma unroll
    for (int bi = 0; bi < WM; ++bi) {
      const int64_t row0 = m0 + wi + bi * 32;
      if constexpr (FMT == kFp16) join_sets<FMT>(acc[bi][bj], low[bi][bj]);      // hi + 2^-11 lo
      if constexpr (PLANES) {
        unsigned char *P = reinterpret_cast<unsigned char *>(Y);
        if (full) store_block_planes<ACT, true>(acc[bi][bj], P, row0, col, M, N, mu, is, ga, be, slope);
        else store_block_planes<ACT, false>(acc[bi][bj], P, row0, col, M, N, mu, is, ga, be, slope);
      } else if (full)
        store_block<ACT, HAS_RES, true, NT>(acc[bi][bj], R, Y, row0, col, M, N, mu, is, ga, be, slope);
      else
        store_block<ACT, HAS_RES, false, NT>(acc[bi][bj], R, Y, row0, col, M, N, mu, is, ga, be, slope);
    }
  }
}

// Launch geometry of an (M, K, N) problem on a device of `cus` compute units (0: unknown): everything launch() decides and the
// kernel decodes, as plain host arithmetic (exported for the tests as skd_conv1x1_abn_geometry).  The comments in the kernel say
// what the numbers mean.
struct Geometry {
  int tiles_n, ct, pm;          // column tiles; column tiles per chunk and row panels per group of the super-tile order
  int64_t p_full, panels, grid; // row panels of 128 rows; all row panels (those behind p_full: 64 rows); workgroups
  bool nt;                      // wide output (ct < tiles_n): super-tile order, non-temporal epilogue
};
inline bool conv1x1_geometry(int64_t M, int K, int N, int cus, Geometry &g) {
  g.tiles_n = N / kTN;
  const int64_t tiles_m = cdiv(M, kTM);
  // super-tile geometry (see the kernel): column-tile chunks of <= 1 MB of weights, panel groups of <= 2 MB of activations
  const int64_t tile_bytes = (int64_t)kTN * K * sizeof(float);
  // (ten geometries were swept with the counters: profiles/r04g_pmc.json, profiles/r04h_two_ranks_one_gpu_bisect.txt; this is the
  // one that minimised L2 -> fabric reads at K = 512 / N = 2048: 851 -> 617 MB per launch)
  g.ct = (int)((1 << 20) / tile_bytes);
  g.pm = (int)((2 << 20) / tile_bytes);
  if (g.ct < 1) g.ct = 1;
  if (g.pm < 1) g.pm = 1;
  g.nt = g.ct < g.tiles_n;                                  // wide: NT epilogue
  if (!g.nt) { g.ct = g.tiles_n; g.pm = 1; }                // narrow output: plain panel-major order
  while (g.tiles_n % g.ct) --g.ct;                          // chunks of equal width (tiles_n is a power of two in this network)
  // half-height panels for the last, partial round; slots = 3 workgroups per compute unit
  g.p_full = g.panels = tiles_m;
  const int64_t slots = (int64_t)kMinWG * cus;
  const int64_t tiles = tiles_m * g.tiles_n;
  if (slots > 0 && tiles > slots && tiles % slots != 0) {
    g.p_full = (tiles / slots) * slots / g.tiles_n / 8 * 8;          // whole rounds, whole XCD rows of panels
    const int64_t rest_rows = M - g.p_full * kTM;
    g.panels = g.p_full + cdiv(rest_rows, kTM / 2);
  }
  const int64_t panels_per_xcd = cdiv(cdiv(g.panels, 8), g.pm) * g.pm;   // row panels padded to whole groups on each of the 8 XCDs
  g.grid = panels_per_xcd * 8 * g.tiles_n;
  return g.grid <= 2147483647;
}

// Workgroup `block` of that grid -> its output tile: rows [m0, m0 + rows) (rows = 128 or 64; 0: padding, the workgroup exits)
// and columns [n0, n0 + 128).  The order is explained in the kernel, its only caller on the device.
struct TileOf {
  int64_t m0;
  int rows, n0;
};
__host__ __device__ __forceinline__ TileOf conv1x1_tile_of(unsigned block, int64_t M, int tiles_n, int pm, int ct, int p_full) {
  const int xcd = block & 7, j = block >> 3;
  const int per_group = pm * tiles_n;
  const int group = j / per_group, r = j - group * per_group;
  const int per_chunk = pm * ct;
  const int chunk = r / per_chunk, r2 = r - chunk * per_chunk;
  const int pl = r2 / ct;
  const int tn = chunk * ct + (r2 - pl * ct);
  const int64_t tm = ((int64_t)group * pm + pl) * 8 + xcd;
  if (tn >= tiles_n) return TileOf{0, 0, 0};
  if (tm < p_full) {
    const int64_t m0 = tm * kTM;
    if (m0 >= M) return TileOf{0, 0, 0};
    return TileOf{m0, kTM, tn * kTN};
  }
  const int64_t m0 = (int64_t)p_full * kTM + (tm - p_full) * (kTM / 2);
  if (m0 >= M) return TileOf{0, 0, 0};
  return TileOf{m0, kTM / 2, tn * kTN};
}

// PIECES = 2 (include/skd_split2.h): two pieces per operand, the three products a0 b1, a1 b0, a0 b0 into the one accumulator; the
// grid, the tile order and the half-height round are those of the three-piece launch (32 KB of LDS + the prologue's table).
// PLANES (include/skd_planes.h): Y is the piece planes of the output (conv1x1_tile); grid and tile order as the fp32 launch.
// FMT = kFp16 (include/skd_split2h.h): two fp16 pieces, the three products into TWO accumulator sets (128 registers at 128 rows),
// so the kernel is compiled for two workgroups per CU; grid, tile order and half-height round stay the three-piece launch's.
constexpr int conv1x1_wgs(int FMT) { return FMT == kFp16 ? 2 : kMinWG; }
template <int ACT, bool HAS_RES, bool PRO, bool NT, int PIECES = 3, bool PLANES = false, int FMT = kBf16>
__global__ __launch_bounds__(kThreads, conv1x1_wgs(FMT)) void conv1x1_abn_kernel(
    const float *__restrict__ X, const float *__restrict__ Wt, const float *__restrict__ R, float *__restrict__ Y,
    const float *__restrict__ mean, const float *__restrict__ var, const float *__restrict__ weight,
    const float *__restrict__ bias, const float *__restrict__ ppack, float eps, float slope, int64_t M, int K, int N,
    int tiles_n, int pm, int ct, int p_full) {
  static_assert(!PLANES || (!HAS_RES && !PRO && !NT && PIECES == 3), "planes out: the plain three-piece GEMM, plain stores");
  static_assert(FMT == kBf16 || PIECES == 2, "fp16 pieces: two of them");
  extern __shared__ __attribute__((aligned(16))) uint4 lds[];
  // XCD-aware tile order.  Workgroup b runs on XCD b % 8 (observed placement, MI355X_MICROARCH.md; used for traffic only, any
  // placement is correct) and every XCD has its own L2: the tiles_n workgroups that share one 128 x K activation panel are
  // therefore given to ONE XCD, back to back in its dispatch order -- the panel is fetched into one L2 instead of eight.
  // Counters before (profiles/r03d_gemm_lab_pmc.json, K = 256, N = 1024): 421 MB fetched for 174 MB of algorithmic reads
  // (8 x the 35 MB of activations); time-neutral in isolation (the Infinity Cache absorbs the fills), less traffic beside the
  // D stream.  Row panel p lives on XCD p % 8; the grid is padded to a multiple of 8 panels, the padding exits here.
  //
  // Round 4: for WIDE outputs that order thrashes the weights instead.  At K = 512, N = 2048 the 16 column
  // tiles of a panel stream all of W (4 MB = one XCD's whole L2) past every panel: counters showed 850 MB fetched for 350 MB of
  // algorithmic reads.  So an XCD walks SUPER-TILES: groups of `pm` row panels (<= 2 MB of activations) x chunks of `ct` column
  // tiles (<= 1 MB of weights): for group: for chunk: for panel in group: for column tile in chunk.  A weight chunk is reused
  // by pm panels back to back, a panel group stays L2-resident across the chunks; W traffic falls from ~one sweep per panel to one
  // per group.  ct == tiles_n (narrow outputs, e.g. K = 256 / N = 1024: 23 of the 33 launches of a teacher forward) degenerates
  // to the panel-major order above.
  //
  // Round 6: HALF-HEIGHT tiles for the launch's last, partial round.  The layer-3 problem is 2120 tiles of 128 x 128 on 768 slots
  // (3 workgroups per CU): 2.76 rounds -- and the lab shows what the ragged last round costs: the same core reaches 0.72 of the
  // peak on a tile count that divides the chip and 0.63-0.69 on this one (profiles/r06t_gemm_lab_quantisation.jsonl).  The row
  // panels p < p_full are 128 rows high, the panels behind them (the rows a whole number of rounds does not cover) 64: twice the
  // workgroups of half the duration fill the last round's slots (p_full is a multiple of 8: whole XCD rows).
  const TileOf t = conv1x1_tile_of(blockIdx.x, M, tiles_n, pm, ct, p_full);
  if (t.rows == kTM)
    conv1x1_tile<kTM, ACT, HAS_RES, PRO, NT, PIECES, PLANES, FMT>(X, Wt, R, Y, mean, var, weight, bias, ppack, eps, slope, M, K, N, t.m0, t.n0, lds);
  else if (t.rows == kTM / 2)
    conv1x1_tile<kTM / 2, ACT, HAS_RES, PRO, NT, PIECES, PLANES, FMT>(X, Wt, R, Y, mean, var, weight, bias, ppack, eps, slope, M, K, N, t.m0, t.n0, lds);
}

__global__ void pack_eval_params_kernel(int K, const float *__restrict__ mean, const float *__restrict__ var,
                                        const float *__restrict__ weight, const float *__restrict__ bias, float eps,
                                        float *__restrict__ pack) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  pack[k] = mean[k];
  pack[K + k] = inv_std_of(var[k], eps);
  pack[2 * (int64_t)K + k] = weight != nullptr ? fabsf(weight[k]) + eps : 1.f;   // bn.cu:153
  pack[3 * (int64_t)K + k] = bias != nullptr ? bias[k] : 0.f;
}

// PLANES: Y is the piece planes; the tile order is the geometry's (the super-tile order of a wide output included) but the stores
// are plain, never non-temporal -- the planes are read by the next launch -- so the one instantiation NT = false serves.
template <int ACT, bool HAS_RES, bool PRO, int PIECES = 3, bool NT = false, bool PLANES = false, int FMT = kBf16>
static int launch(const float *X, const float *Wt, const float *R, float *Y, const float *mean, const float *var,
                  const float *weight, const float *bias, const float *ppack, float eps, float slope, int64_t M, int K, int N,
                  hipStream_t st) {
  static PerDeviceFlag ready;          // per instantiation AND per device
  bool *rdy = ready.get();
  if (rdy == nullptr) return 0;
  if (!*rdy) {
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(conv1x1_abn_kernel<ACT, HAS_RES, PRO, NT, PIECES, PLANES, FMT>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)(conv_lds(PIECES) + sizeof(float) * 4 * kProMaxK)) != hipSuccess) return 0;
    *rdy = true;
  }
  const size_t lds_bytes = conv_lds(PIECES) + (PRO ? sizeof(float) * 4 * (size_t)K : 0);
  Geometry g;
  if (!conv1x1_geometry(M, K, N, cu_count(st), g)) return 0;
  if (g.nt && !NT && !PLANES) return launch<ACT, HAS_RES, PRO, PIECES, true, false, FMT>(X, Wt, R, Y, mean, var, weight, bias, ppack, eps, slope, M, K, N, st);
  conv1x1_abn_kernel<ACT, HAS_RES, PRO, NT, PIECES, PLANES, FMT><<<dim3((unsigned)g.grid), dim3(kThreads), lds_bytes, st>>>(
      X, Wt, R, Y, mean, var, weight, bias, ppack, eps, slope, M, K, N, g.tiles_n, g.pm, g.ct, (int)g.p_full);
  return ok();
}

}  // namespace
}  // namespace skd

using namespace skd;

extern "C" {

// 1 when the fused kernel takes the problem (K a multiple of 16, N a multiple of 128), 0 when the caller must run
// the convolution and the ABN pass separately.
int skd_conv1x1_abn_supported(int64_t M, int K, int N) { return M > 0 && K > 0 && N > 0 && K % kBK == 0 && N % kTN == 0; }

// Host only, no device needed: the launch geometry of an (M, K, N) problem on `cus` compute units,
//   out[7] = tiles_n, ct, pm, p_full, panels, grid, nt (see Geometry); 0 when the kernel does not take the problem.
int skd_conv1x1_abn_geometry(int64_t M, int K, int N, int cus, int64_t *out) {
  Geometry g;
  if (!skd_conv1x1_abn_supported(M, K, N) || cus < 0 || !out || !conv1x1_geometry(M, K, N, cus, g)) return 0;
  out[0] = g.tiles_n; out[1] = g.ct; out[2] = g.pm; out[3] = g.p_full; out[4] = g.panels; out[5] = g.grid; out[6] = g.nt;
  return 1;
}

// ... and the output tiles of the `count` workgroups from `block` on, by the kernel's own decode: out[3 i ...] = m0, rows, n0 of
// workgroup block + i (rows = 0: the workgroup is padding and exits); 0 when a workgroup is outside the grid.
int skd_conv1x1_abn_tile_of(int64_t M, int K, int N, int cus, int64_t block, int64_t count, int64_t *out) {
  Geometry g;
  if (!skd_conv1x1_abn_supported(M, K, N) || cus < 0 || !out || !conv1x1_geometry(M, K, N, cus, g)) return 0;
  if (block < 0 || count < 0 || block > g.grid || count > g.grid - block) return 0;
  for (int64_t i = 0; i < count; ++i) {
    const TileOf t = conv1x1_tile_of((unsigned)(block + i), M, g.tiles_n, g.pm, g.ct, (int)g.p_full);
    out[3 * i] = t.m0; out[3 * i + 1] = t.rows; out[3 * i + 2] = t.n0;
  }
  return 1;
}

}  // extern "C"

// The host body of the four GEMM entries below: every refusal, then the instantiation that (activation, residual, prologue) name.
template <int PIECES, int FMT = kBf16>
static int conv1x1_dispatch(int64_t M, int K, int N, const float *x, const float *w, const float *residual, float *out,
                            const float *mean, const float *var, const float *weight, const float *bias, const float *ppack,
                            float eps, int activation, float slope, skd_stream_t stream) {
  if (!skd_conv1x1_abn_supported(M, K, N) || !x || !w || !out || !mean || !var) return 0;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(ppack)) & 15) return 0;
  hipStream_t st = as_stream(stream);
#define SKD_C11(A)                                                                                                        \
  if (ppack != nullptr)                                                                                                   \
    return residual ? launch<A, true, true, PIECES, false, false, FMT>(x, w, residual, out, mean, var, weight, bias, ppack, eps, slope, M, K, N, st)   \
                    : launch<A, false, true, PIECES, false, false, FMT>(x, w, residual, out, mean, var, weight, bias, ppack, eps, slope, M, K, N, st); \
  return residual ? launch<A, true, false, PIECES, false, false, FMT>(x, w, residual, out, mean, var, weight, bias, nullptr, eps, slope, M, K, N, st) \
                  : launch<A, false, false, PIECES, false, false, FMT>(x, w, residual, out, mean, var, weight, bias, nullptr, eps, slope, M, K, N, st)
  switch (activation) {
    case SKD_ACT_NONE: SKD_C11(SKD_ACT_NONE);
    case SKD_ACT_RELU: SKD_C11(SKD_ACT_RELU);
    case SKD_ACT_LEAKY_RELU: SKD_C11(SKD_ACT_LEAKY_RELU);
    default: return 0;
  }
#undef SKD_C11
}

extern "C" {

int skd_conv1x1_abn_nhwc(int64_t M, int K, int N, const float *x, const float *w, const float *residual, float *out,
                         const float *mean, const float *var, const float *weight, const float *bias, float eps,
                         int activation, float slope, skd_stream_t stream) {
  return conv1x1_dispatch<3>(M, K, N, x, w, residual, out, mean, var, weight, bias, nullptr, eps, activation, slope, stream);
}

// pack (4, K) = [mean | invstd(var, eps) | |weight| + eps (1 when NULL) | bias (0 when NULL)]: the per-channel constants of an
// eval-mode InPlace-ABN (bn.cu:146-159) in the form the prologue below consumes.  A frozen network computes it once.
int skd_abn_pack_eval_params(int K, const float *mean, const float *var, const float *weight, const float *bias, float eps,
                             float *pack, skd_stream_t stream) {
  if (K <= 0 || !mean || !var || !pack) return 0;
  pack_eval_params_kernel<<<dim3((unsigned)cdiv(K, 256)), dim3(256), 0, as_stream(stream)>>>(K, mean, var, weight, bias, eps, pack);
  return ok();
}

// The same GEMM with the PRECEDING eval-mode BatchNorm + ReLU applied to x on the way into LDS:
//   a[m][k] = relu(((x[m][k] - mean_k) * invstd_k) * gamma_k + beta_k),   (mean | invstd | gamma | beta) = ppack (4, K)
// (networks/pspnet_combine.py:71-75: conv2 -> bn2 -> relu -> conv3 -> bn3 -> + residual -> relu): x is the raw output of the
// 3x3 convolution, neither ABN pass of the block tail exists any more.  ppack: skd_abn_pack_eval_params, 16-byte aligned.
int skd_conv1x1_abn_pro_nhwc(int64_t M, int K, int N, const float *x, const float *w, const float *residual, float *out,
                             const float *mean, const float *var, const float *weight, const float *bias, float eps,
                             const float *ppack, int activation, float slope, skd_stream_t stream) {
  if (!ppack || K > kProMaxK) return 0;
  return conv1x1_dispatch<3>(M, K, N, x, w, residual, out, mean, var, weight, bias, ppack, eps, activation, slope, stream);
}

// include/skd_split2.h: the same two entries on two pieces per operand (three products).
int skd_conv1x1_abn2_nhwc(int64_t M, int K, int N, const float *x, const float *w, const float *residual, float *out,
                          const float *mean, const float *var, const float *weight, const float *bias, float eps,
                          int activation, float slope, skd_stream_t stream) {
  return conv1x1_dispatch<2>(M, K, N, x, w, residual, out, mean, var, weight, bias, nullptr, eps, activation, slope, stream);
}

// include/skd_planes.h: the plain three-piece GEMM with the pieces of its epilogue's value written to piece planes.
int skd_conv1x1_abn_planes_nhwc(int64_t M, int K, int N, const float *x, const float *w, void *planes_out, const float *mean,
                                const float *var, const float *weight, const float *bias, float eps, int activation, float slope,
                                skd_stream_t stream) {
  if (!skd_conv1x1_abn_supported(M, K, N) || !x || !w || !planes_out || !mean || !var) return 0;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(planes_out)) & 15) return 0;
  hipStream_t st = as_stream(stream);
  float *y = static_cast<float *>(planes_out);
#define SKD_C11P(A) \
  case A: return launch<A, false, false, 3, false, true>(x, w, nullptr, y, mean, var, weight, bias, nullptr, eps, slope, M, K, N, st)
  switch (activation) {
    SKD_C11P(SKD_ACT_NONE);
    SKD_C11P(SKD_ACT_RELU);
    SKD_C11P(SKD_ACT_LEAKY_RELU);
    default: return 0;
  }
#undef SKD_C11P
}

int skd_conv1x1_abn2_pro_nhwc(int64_t M, int K, int N, const float *x, const float *w, const float *residual, float *out,
                              const float *mean, const float *var, const float *weight, const float *bias, float eps,
                              const float *ppack, int activation, float slope, skd_stream_t stream) {
  if (!ppack || K > kProMaxK) return 0;
  return conv1x1_dispatch<2>(M, K, N, x, w, residual, out, mean, var, weight, bias, ppack, eps, activation, slope, stream);
}

// include/skd_split2h.h: the same two entries on two fp16 pieces per operand with the scaled residual.
int skd_conv1x1_abn2h_nhwc(int64_t M, int K, int N, const float *x, const float *w, const float *residual, float *out,
                           const float *mean, const float *var, const float *weight, const float *bias, float eps,
                           int activation, float slope, skd_stream_t stream) {
  return conv1x1_dispatch<2, kFp16>(M, K, N, x, w, residual, out, mean, var, weight, bias, nullptr, eps, activation, slope, stream);
}

int skd_conv1x1_abn2h_pro_nhwc(int64_t M, int K, int N, const float *x, const float *w, const float *residual, float *out,
                               const float *mean, const float *var, const float *weight, const float *bias, float eps,
                               const float *ppack, int activation, float slope, skd_stream_t stream) {
  if (!ppack || K > kProMaxK) return 0;
  return conv1x1_dispatch<2, kFp16>(M, K, N, x, w, residual, out, mean, var, weight, bias, ppack, eps, activation, slope, stream);
}

}  // extern "C"
