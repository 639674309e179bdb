// conv3x3_wgrad.hip -- the WEIGHT GRADIENT of a 3x3, stride-1, "same" (padding = dilation) convolution on the split-operand
// bf16-MFMA core of conv_split_dev.hpp (see conv1x1.hip for the core, conv3x3.hip for forward and data gradient): fp32 in, fp32 out.
//
//     dW[n][c][ty][tx] = sum_{m = (b, y, x)} g[m][n] * X[b, y + (ty - 1) d, x + (tx - 1) d, c]      (0 outside the image)
//
// with channels-last x (B, H, W, Cin) and g (B, H, W, Cout): nine GEMMs (Cout x P) (P x Cin), one per tap, reduced over the
// P = B H W pixels.  One kernel, conv3x3_wgrad_kernel<NARROW, TAPS, PIECES>, in two tile forms.
//
// WIDE (skd_wgrad.h; Cin and Cout multiples of 128).  Operand A rows = 128 output channels of g, operand B rows = 128 input
// channels of the shifted x, K = the pixel index in K-tiles of 16 pixels; tile_mma<128> with its two accumulator sets, k_loop<2>
// and store_block as they are.  One workgroup computes one (tap, n-tile, c-tile, K-slice) and writes a 128 x 128 fp32 block of the
// workspace part[slice][n][tap][c]; conv3x3_wgrad_reduce_kernel sums the slices in the order 0 .. S - 1 (no atomics: the same bits
// every time) and writes dW through the destination's strides.
//
// NARROW (skd_narrow_wgrad.h; Cin and Cout multiples of 64).  tile_mma<128, 64>: waves 4 x 1, wave tile 32 x 64, 64 accumulator
// registers for both sets.  The operands change sides: A rows = 128 rows of the shifted x, B rows = 64 output channels of g.  The
// 128 rows are two consecutive UNITS of 64; a unit is (tap, 64-channel slice of Cin), numbered tap-major over U = 9 Cin / 64, so
// that unit u, row i is row 64 u + i = tap * Cin + c of the (9 Cin) x Cout matrix dW^T.  For Cin = 64 a tile holds two taps of the
// same pixels (five tiles, the last half-tile dead: exact zeros in LDS, not stored), for Cin = 128 one tap's two halves; a Cout
// of 128 is two column tiles.  tile_mma's SWAP puts the pieces back in the wide form's order -- step t multiplies piece kPA[t] of
// g by piece kPB[t] of x in both forms -- so with the K-tiles, the slices and the epilogue (acc += low, store_block) unchanged
// every element of dW sees the same operations in the same order: a shape both forms take comes out bit-identical for the same
// slice count.  The accumulator block is (x rows) x (g columns), the transpose of the wide one; it is stored as it lies, in rows of
// 32 consecutive floats, into part[slice][tap * Cin + c][n], and conv3x3_wgrad_reduce_rows_kernel does the re-indexing.
//
// Staging -- the part that is this kernel's own.  Memory is [pixel][channel]; the LDS image wants eight consecutive k (= pixels)
// of one row (= channel) in one chunk, so BOTH operands are transposed on the way in and BOTH are split in the loop (there is no
// frozen pack to stream).  A thread owns (channel quad r, pixel quad q): four float4 loads at pixels 4 q .. 4 q + 3, channels
// 4 r .. 4 r + 3 (the forward's load count), a 4 x 4 transposition in registers, and one split_store per channel row at
// plane_slot(row, 4 q) (twice the forward's split work).  WIDE: 256 rows per K-tile, waves 0, 1 stage g, waves 2, 3 stage x, 32
// channel quads per operand.  NARROW: 192 rows per K-tile = three groups of 64 rows, one per wave and 16 channel quads each:
// wave 0 stages g, wave 1 the tile's first unit, wave 2 its second, wave 3 stages nothing (it has its quarter of the MFMAs like
// the others).  A wave so has ONE tap: one shift, one validity test per pixel and one division pair per K-tile and thread.
//
// Bank conflicts of those stores (ds_write_b64: 16 consecutive lanes per LDS cycle, bank pair = 8-byte slot mod 16):
//     slot(row, q) mod 16 = 2 ((row mod 8) ^ 4 (q >> 1)) + (q & 1).
// With lanes running over r and every lane storing row 4 r + j in its j-th store, row mod 8 takes two values in a lane group
// (4 (r & 1) + j) and q none: EIGHT-way.  So which lane owns which row is changed, not the image: within the 16 lanes of a group,
// bits 0-2 of the lane are bits 0-2 of r and bit 3 is bit 0 of q, and the j-th store of a lane writes row 4 r + (j ^ s) with
// s = (r >> 1) & 3 (the four channels of a load are permuted by XOR with s before the transposition: 8 v_cndmask per load).
// Then (row mod 8, q & 1) takes all sixteen values in a group: conflict-free.  A load instruction of a wave still covers whole
// pixels: two pixels x 32 channel quads = 2 x 512 contiguous bytes.
// NARROW, re-derived.  The x image is the 128-row one; a unit's rows are 64 u' + (0 .. 63) and 64 rows are 128 slots = 0 mod 16, so
// the formula above holds for both units.  The g image has 64 rows: chunk(h, row) = 64 h + (row ^ 4 h), i.e.
// slot(row, q) = 2 (64 (q >> 1) + (row ^ 4 (q >> 1))) + (q & 1), and 128 (q >> 1) = 0 mod 16: the same residue again.  A wave has
// 16 channel quads and 4 pixel quads on its 64 lanes: bits 0-2 of the lane are bits 0-2 of r, bit 3 is bit 0 of q, bit 4 is bit 3
// of r, bit 5 is bit 1 of q.  Inside a 16-lane group bits 3 of r and 1 of q are fixed, r & 1 and s = (r >> 1) & 3 take all eight
// combinations, so row mod 8 = 4 (r & 1) + (j ^ s) takes all eight values for every j, and q & 1 both: sixteen distinct bank
// pairs, conflict-free, for the pieces 256 (g) or 512 (x) slots further on as well.  A load instruction of a wave covers four
// pixels x 16 channel quads = 4 x 256 contiguous bytes.
//
// Shifted operand: x row k = pixel m is read at m + shift(tap) when the shifted pixel stays inside ITS image and m < P, and is an
// exact zero with no load issued otherwise (as stage_load3_a); g rows beyond P are zeros.  (y, x) of the first pixel of a
// thread's quad come from one division pair per K-tile (multiply-high by a host-made reciprocal, one correction), the other three
// pixels by stepping: a quad may straddle a row end or an image end, validity is per pixel.
//
// Grid: id -> (XCD = id & 7, j = id >> 3); the workgroups of one XCD take consecutive logical indices, and a logical index is
// ((slice * tiles_n + tn) * tiles_c + tc) * 9 + tap: the nine taps of one (slice, n-tile, c-tile) are neighbours on ONE XCD and
// read the same pixels of g and (shifted by at most d rows) of x from that L2 (NARROW: (slice * tiles_n + tn) * tiles_u + tu, the
// unit pairs of one slice are neighbours).  -DSKD_WGRAD_GRID_ORDER=1 builds the other order
// for measurements (logical index = blockIdx.x: neighbours land on eight different XCDs); tools/conv3x3_wgrad_bench.py --lib times
// such a build beside the shipped one.
//
// ONE TAP (skd_shortcut.h; TAPS = 1): the weight gradient of a 1x1 convolution of stride 1 or 2 without padding is the centre tap
// alone -- dW[n][c] = sum_m g[m][n] X[pix(m)][c] over the OUTPUT pixels m, pix(m) = (b, y s, x s) -- in either tile form: no shift
// and no validity test, the rows of x picked by index arithmetic in the load, one unit of 64 input channels per 64 of Cin.
#include "conv_split_dev.hpp"
#include "skd_narrow_wgrad.h"
#include "skd_shortcut.h"
#include "skd_train2.h"
#include "skd_train2h.h"
#include "skd_wgrad.h"

#ifndef SKD_WGRAD_GRID_ORDER
#define SKD_WGRAD_GRID_ORDER 0
#endif

namespace skd {
namespace {

constexpr int kWgDepth = 2;                            // K-tiles of load look-ahead (k_loop)
constexpr int kMaxPixels = 1 << 30;                    // P below this: pixel arithmetic in 32 bits, dilation included
constexpr int kMaxDilation = 1 << 24;
constexpr int kUnit = 64;                              // NARROW: rows of a unit, columns of a tile

// The two tile forms, every constant of the host side in one place: the granule of the channel counts, the workgroups of one
// slice, the workgroups that share a CU (the kernel's occupancy: profiles/r23_kernel_resources.md) and the rounds of the device
// the automatic slice count may fill.
template <bool NARROW, int TAPS = 9>
struct Form {
  static constexpr int granule = NARROW ? kUnit : kTM;
  static constexpr int per_cu = NARROW ? 3 : 2;
  static constexpr int max_rounds = NARROW ? 1 : 2;
  static int64_t tiles(int Cin, int Cout) {
    return NARROW ? cdiv(TAPS * (int64_t)(Cin / kUnit), 2) * (Cout / kUnit) : TAPS * (int64_t)(Cin / kTN) * (Cout / kTM);
  }
};

struct StagingW {
  float4 v[4];                                         // pixels 4 q .. 4 q + 3, channels 4 r .. 4 r + 3
};

template <bool NARROW, int TAPS = 9, int PIECES = 3, int FMT = kBf16>
struct TileW {
  typedef StagingW Stg;
  static constexpr int WM = NARROW ? 1 : 2;
  const float *__restrict__ src;      // g or x, at the thread's first channel
  int64_t shift;                      // the tap's pixel shift (0 for g)
  int C;                              // floats per pixel of src
  int P, H, W, hw;                    // P = 0: every row of this thread is an exact zero (a dead unit, a wave that stages nothing)
  unsigned rcp_hw, rcp_w;
  int dy, dx;                         // the tap's (ty - 1) d, (tx - 1) d
  int m_first;                        // first pixel of this thread's quad in K-tile 0 of the slice
  bool is_x;                          // wave-uniform
  bool stages;                        // wave-uniform; NARROW: false for the fourth wave
  int s;                              // channel permutation of this lane
  int slot[4];                        // 8-byte LDS slot of the j-th stored row, the operand's offset included
  int in_hw, in_row, in_step;         // TAPS == 1: pixels of an image of x, and the pixel steps of one output row and column
  float scale;                        // FMT == kFp16: g's rows times s (scale_of), x's rows times 1; otherwise unused
  f32x16 (&low)[WM][2], (&acc)[WM][2];

  __device__ __forceinline__ void load(Stg &st, int kt) const {
    const int m0 = m_first + kt * kBK;
    if constexpr (TAPS == 1) {
      // The 1x1 convolution of stride s, no padding: H, W are the OUTPUT's sizes, row k of x is the input pixel (img, y s, x s)
      // that output pixel m = (img, y, x) reads -- index arithmetic here, always inside the image.
      unsigned img = 0, y = 0, x = 0;
      if (is_x) {
        unsigned pix;
        divmod((unsigned)m0, (unsigned)hw, rcp_hw, img, pix);
        divmod(pix, (unsigned)W, rcp_w, y, x);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t pixel = is_x ? (int64_t)img * in_hw + (int64_t)y * in_row + x * in_step : (int64_t)(m0 + i);
        st.v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (m0 + i < P) st.v[i] = *reinterpret_cast<const float4 *>(src + pixel * C);
        ++x;
        if (x == (unsigned)W) {
          x = 0;
          ++y;
          if (y == (unsigned)H) {
            y = 0;
            ++img;
          }
        }
      }
      return;
    }
    unsigned y = 0, x = 0;
    if (is_x) {
      unsigned img, pix;
      divmod((unsigned)m0, (unsigned)hw, rcp_hw, img, pix);
      divmod(pix, (unsigned)W, rcp_w, y, x);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      // unsigned compares: a negative shifted coordinate is a large one
      const bool live = m0 + i < P && (unsigned)((int)y + dy) < (unsigned)H && (unsigned)((int)x + dx) < (unsigned)W;
      st.v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (live) st.v[i] = *reinterpret_cast<const float4 *>(src + ((int64_t)(m0 + i) + shift) * C);
      // the next pixel: one step, across a row end and an image end
      ++x;
      if (x == (unsigned)W) {
        x = 0;
        ++y;
        if (y == (unsigned)H) y = 0;
      }
    }
  }
  __device__ __forceinline__ void store(const Stg &st, uint4 *stage, int) const {
    if (NARROW && !stages) return;
    float p[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float4 v = st.v[i];
      // component j of the permuted load = channel j ^ s
      const float a0 = (s & 1) ? v.y : v.x, a1 = (s & 1) ? v.x : v.y, a2 = (s & 1) ? v.w : v.z, a3 = (s & 1) ? v.z : v.w;
      p[i][0] = (s & 2) ? a2 : a0;
      p[i][1] = (s & 2) ? a3 : a1;
      p[i][2] = (s & 2) ? a0 : a2;
      p[i][3] = (s & 2) ? a1 : a3;
    }
    uint2 *base = reinterpret_cast<uint2 *>(stage);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float4 row = make_float4(p[0][j], p[1][j], p[2][j], p[3][j]);
      // NARROW: g's 64-row image has its pieces 2 * 128 slots apart; a wave-uniform branch keeps both distances immediates
      if (NARROW && !is_x) split_store(row, base + slot[j], 2 * 2 * kUnit);
      else if constexpr (FMT == kFp16) split_store<PIECES, FMT>(scaled(row, scale), base + slot[j]);
      else split_store<PIECES>(row, base + slot[j]);
    }
  }
  __device__ __forceinline__ void mma(const uint4 *stage) const {
    if constexpr (NARROW) tile_mma<kTM, kUnit, true>(stage, low, acc);
    else tile_mma<kTM, kTN, false, PIECES, FMT>(stage, low, acc);
  }
};

// WIDE: 128 accumulator registers, two staging sets: two workgroups per CU like the TALL forward (profiles/r20_kernel_resources.md).
// NARROW: 64 accumulator registers: three per CU, the LDS ring's limit (3 x 48 KB of 160).
// TAPS == 1 (skd_shortcut.h): the weight gradient of a 1x1 convolution of stride `dil` without padding as the one-tap form of both:
// H, W are the output's sizes (the pixels of g), Hin, Win the input's; the one tap is the centre (no shift, always inside).
// PIECES = 2 (skd_train2.h; WIDE with nine taps alone): both operands are cut into two pieces in the staging and three products
// are kept per K-tile -- a0 b1 and a1 b0 into `low`, a0 b0 into `acc`, the two-set rule as it is.  The LDS ring shrinks to
// conv_lds(2) = 32 KB; the 128 accumulator registers stay, so the two workgroups per CU stay too (three would leave 168
// registers a lane for 128 accumulators, two staging sets and the fragments: profiles/r33_kernel_resources.md).
// FMT = kFp16 (skd_train2h.h; that PIECES = 2 form alone): two fp16 pieces with the scaled residual.  g's rows are multiplied by
// s = scale_of(*word) in front of the split (word == nullptr: s = 1), x's rows are not; the slice's block is
// fma(low, 2^-11, acc) (1 / s).  LDS ring, accumulators, staging sets and the two workgroups per CU are the bf16 twin's
// (profiles/r35_kernel_resources.md).
template <bool NARROW, int TAPS = 9, int PIECES = 3, int FMT = kBf16>
__global__ __launch_bounds__(kThreads, Form<NARROW>::per_cu)
__attribute__((amdgpu_waves_per_eu(Form<NARROW>::per_cu, Form<NARROW>::per_cu)))
void conv3x3_wgrad_kernel(const float *__restrict__ X, const float *__restrict__ G, float *__restrict__ part, int P, int H, int W,
                          int Cin, int Cout, int dil, int nk, int tiles_per_slice, int slices, unsigned rcp_hw, unsigned rcp_w,
                          int total, int Hin, int Win, const uint32_t *__restrict__ word) {
  static_assert(TAPS == 9 || TAPS == 1, "the 3x3 convolution, or its centre tap alone");
  static_assert(FMT == kBf16 || (FMT == kFp16 && PIECES == 2), "fp16 pieces: the two-piece form alone");
  static_assert(PIECES == 3 || (PIECES == 2 && !NARROW && TAPS == 9), "two pieces: the wide nine-tap form alone");
  extern __shared__ __attribute__((aligned(16))) uint4 lds[];
  constexpr int WM = NARROW ? 1 : 2;
  const int per_xcd = (int)(gridDim.x >> 3);
  const int id = SKD_WGRAD_GRID_ORDER == 1 ? (int)blockIdx.x : (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3);
  if (id >= total) return;

  f32x16 acc[WM][2], low[WM][2];
#pragma unroll
  for (int i = 0; i < WM; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][j][q] = low[i][j][q] = 0.f;
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;

  if constexpr (NARROW) {
    const int tiles_n = Cout / kUnit, per_tap = Cin / kUnit, units = TAPS * per_tap, tiles_u = (units + 1) / 2;
    const int tu = id % tiles_u;
    const int rest = id / tiles_u;
    const int tn = rest % tiles_n, slice = rest / tiles_n;
    const int kt0 = slice * tiles_per_slice;
    const int nks = min(tiles_per_slice, nk - kt0);        // >= 1: the plan leaves no slice empty

    // the wave's place in the staging: 0 = g, 1 / 2 = the tile's first / second unit, 3 = none; the lane's inside its 64 rows
    const bool is_x = wid == 1 || wid == 2, stages = wid < 3;
    const int unit = 2 * tu + (wid == 2 ? 1 : 0);
    const bool has_rows = stages && (!is_x || unit < units);   // the second unit of the last tile is dead when U is odd
    const int tap = is_x && unit < units ? unit / per_tap : 4, cs = is_x && unit < units ? unit - tap * per_tap : 0;
    const int ty = TAPS == 1 ? 1 : tap / 3, tx = TAPS == 1 ? 1 : tap - 3 * ty;
    const int r = (lane & 7) | (((lane >> 4) & 1) << 3);   // channel quad 0 .. 15
    const int q = ((lane >> 3) & 1) | (((lane >> 5) & 1) << 1);   // pixel quad 0 .. 3
    const int s = (r >> 1) & 3;
    const float *src = (is_x ? X + cs * kUnit : G + tn * kUnit) + 4 * r;
    TileW<true, TAPS> tile = {src,
                        is_x ? ((int64_t)(ty - 1) * W + (tx - 1)) * dil : 0,
                        is_x ? Cin : Cout, has_rows ? P : 0, H, W, H * W, rcp_hw, rcp_w,
                        is_x ? (ty - 1) * dil : 0, is_x ? (tx - 1) * dil : 0,
                        kt0 * kBK + 4 * q, is_x, stages, s, {}, Hin * Win, dil * Win, dil, 1.f, low, acc};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = 4 * r + (j ^ s), kh = q >> 1;
      tile.slot[j] = is_x ? 2 * kUnit * (wid - 1) + plane_slot(row, 4 * q)
                          : 2 * kOperandChunks + 2 * (kh * kUnit + (row ^ (kh * 4))) + (q & 1);
    }
    k_loop<kWgDepth>(tile, nks, lds);

    // ---- epilogue: the slice's 128 x 64 block of part[slice][tap * Cin + c][n], every element of the slab written ----
    const int64_t rows = TAPS * (int64_t)Cin;
    const int64_t row0 = (int64_t)tu * kTM + wid * 32;
    float *slab = part + (int64_t)slice * rows * Cout;
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[0][bj][e] += low[0][bj][e];
      if (row0 < rows)                                       // wave-uniform: a dead unit's 64 rows lie past the slab
        store_block<SKD_ACT_NONE, false, true, false>(acc[0][bj], nullptr, slab, row0, tn * kUnit + bj * 32 + (lane & 31), rows, Cout,
                                                      0.f, 1.f, 1.f, 0.f, 0.f);
    }
  } else {
    const int tiles_c = Cin / kTN, tiles_n = Cout / kTM;
    const int tap = id % TAPS;
    int rest = id / TAPS;
    const int tc = rest % tiles_c;
    rest /= tiles_c;
    const int tn = rest % tiles_n, slice = rest / tiles_n;
    const int ty = TAPS == 1 ? 1 : tap / 3, tx = TAPS == 1 ? 1 : tap - 3 * ty;
    const int kt0 = slice * tiles_per_slice;
    const int nks = min(tiles_per_slice, nk - kt0);          // >= 1: the plan leaves no slice empty

    // the thread's place in the staging of its operand: l = 0 .. 127 inside the operand's two waves
    const int l = threadIdx.x & 127;
    const bool is_x = threadIdx.x >= 128;
    const int r = (l & 7) | (((l >> 4) & 3) << 3);           // channel quad 0 .. 31
    const int q = ((l >> 3) & 1) | (((l >> 6) & 1) << 1);    // pixel quad 0 .. 3
    const int s = (r >> 1) & 3;
    const int C = is_x ? Cin : Cout;
    const float *src = (is_x ? X + tc * kTN : G + tn * kTM) + 4 * r;
    float scale = 1.f, unscale = 1.f;
    if constexpr (FMT == kFp16) {
      if (word != nullptr) scale_of(*word, scale, unscale);
    }
    TileW<false, TAPS, PIECES, FMT> tile = {src,
                         is_x ? ((int64_t)(ty - 1) * W + (tx - 1)) * dil : 0,
                         C, P, H, W, H * W, rcp_hw, rcp_w,
                         is_x ? (ty - 1) * dil : 0, is_x ? (tx - 1) * dil : 0,
                         kt0 * kBK + 4 * q, is_x, true, s, {}, Hin * Win, dil * Win, dil, is_x ? 1.f : scale, low, acc};
#pragma unroll
    for (int j = 0; j < 4; ++j) tile.slot[j] = (is_x ? 2 * operand_chunks(PIECES) : 0) + plane_slot(4 * r + (j ^ s), 4 * q);
    k_loop<kWgDepth, PIECES>(tile, nks, lds);

    // ---- epilogue: the slice's 128 x 128 block of part[slice][n][tap][c], every element written ----
    const int wi = (wid >> 1) * (kTM / 2), wj = (wid & 1) * 64;
    float *slab = part + (int64_t)slice * TAPS * Cin * Cout;
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
      const int col = tap * Cin + tc * kTN + wj + bj * 32 + (lane & 31);
#pragma unroll
      for (int bi = 0; bi < 2; ++bi) {
        if constexpr (FMT == kFp16) {      // the one join of the fp16 sets (conv_split_dev.hpp), then the scale of g taken out
          join_sets<kFp16>(acc[bi][bj], low[bi][bj]);
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[bi][bj][e] *= unscale;
        } else {
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[bi][bj][e] += low[bi][bj][e];
        }
        store_block<SKD_ACT_NONE, false, true, false>(acc[bi][bj], nullptr, slab, (int64_t)tn * kTM + wi + bi * 32, col, Cout, TAPS * Cin,
                                                      0.f, 1.f, 1.f, 0.f, 0.f);
      }
    }
  }
}

__device__ __forceinline__ void accumulate(float4 &s, const float4 &a) { s.x += a.x; s.y += a.y; s.z += a.z; s.w += a.w; }
__device__ __forceinline__ void accumulate(float &s, const float &a) { s += a; }

// p[0] + p[step] + ... + p[(slices - 1) step], added in that order; four loads in flight.
template <class T>
__device__ __forceinline__ T slice_sum(const T *__restrict__ p, int64_t step, int slices) {
  T sum = p[0];
  int sl = 1;
  for (; sl + 3 < slices; sl += 4) {
    const T a = p[sl * step], b = p[(sl + 1) * step], c = p[(sl + 2) * step], d = p[(sl + 3) * step];
    accumulate(sum, a);
    accumulate(sum, b);
    accumulate(sum, c);
    accumulate(sum, d);
  }
  for (; sl < slices; ++sl) accumulate(sum, p[sl * step]);
  return sum;
}

// dw[n][c][ty][tx] = sum over the slices, in slice order, of part[slice][n][tap][c]; one thread per four consecutive c.
// VEC: the destination takes the four as one 16-byte store (unit channel stride, everything else a multiple of four floats):
// for a dense channels-last weight the whole kernel is a streaming sum.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void conv3x3_wgrad_reduce_kernel(const float *__restrict__ part, float *__restrict__ dw,
                                                                        int Cin, int64_t quads, int64_t slab, int slices,
                                                                        int64_t sn, int64_t sc, int64_t sy, int64_t sx, int taps) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= quads) return;
  const int64_t e = 4 * t;
  const float4 sum = slice_sum(reinterpret_cast<const float4 *>(part + e), slab / 4, slices);
  const int64_t row = taps * (int64_t)Cin;
  const int64_t n = e / row;
  const int rem = (int)(e - n * row);
  const int tap = rem / Cin, c = rem - tap * Cin;
  const int ty = tap / 3, tx = tap - 3 * ty;
  float *dst = dw + n * sn + ty * sy + tx * sx + c * sc;
  if (VEC) {
    *reinterpret_cast<float4 *>(dst) = sum;
  } else {
    dst[0] = sum.x;
    dst[sc] = sum.y;
    dst[2 * sc] = sum.z;
    dst[3 * sc] = sum.w;
  }
}

// The same for the NARROW form's workspace part[slice][tap * Cin + c][n]: one thread per (four consecutive c, n); consecutive
// threads take consecutive n, so each of a thread's four loads per slice is one coalesced row segment of the wave.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void conv3x3_wgrad_reduce_rows_kernel(const float *__restrict__ part, float *__restrict__ dw,
                                                                             int Cin, int Cout, int64_t quads, int64_t slab, int slices,
                                                                             int64_t sn, int64_t sc, int64_t sy, int64_t sx) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= quads) return;
  const int64_t rq = t / Cout;
  const int n = (int)(t - rq * Cout);
  const float *p = part + 4 * rq * Cout + n;
  const float4 sum = make_float4(slice_sum(p, slab, slices), slice_sum(p + Cout, slab, slices), slice_sum(p + 2 * Cout, slab, slices),
                                 slice_sum(p + 3 * (int64_t)Cout, slab, slices));
  const int rem = (int)(4 * rq);                             // < 9 Cin (one tap: < Cin, tap 0)
  const int tap = rem / Cin, c = rem - tap * Cin;
  const int ty = tap / 3, tx = tap - 3 * ty;
  float *dst = dw + n * sn + ty * sy + tx * sx + c * sc;
  if (VEC) {
    *reinterpret_cast<float4 *>(dst) = sum;
  } else {
    dst[0] = sum.x;
    dst[sc] = sum.y;
    dst[2 * sc] = sum.z;
    dst[3 * sc] = sum.w;
  }
}

// Slices asked for -> the slices of an exact cover: T = ceil(nk / S) K-tiles each, and as many slices as that T needs.
void cover(int64_t nk, int64_t slices, int64_t &used, int64_t &per_slice) {
  if (slices > nk) slices = nk;
  per_slice = cdiv(nk, slices);
  used = cdiv(nk, per_slice);
}

template <bool NARROW>
int supported(int Cin, int Cout, int stride, int padding, int dilation, int groups) {
  return Cin > 0 && Cout > 0 && Cin % Form<NARROW>::granule == 0 && Cout % Form<NARROW>::granule == 0 && stride == 1 &&
         dilation >= 1 && padding == dilation && groups == 1;
}

// The rule for slices == 0, both forms (the headers state it with each form's constants).  A launch of tiles * S workgroups
// takes ceil(tiles * S / slots) rounds of the device's slots = per_cu * cus places, each round as long as a slice: ceil(nk / S)
// K-tiles.  S is the count in 1 .. max(1, max_rounds * slots / tiles) (the workspace and the reduce launch grow with S) with the
// smallest rounds * K-tiles-per-slice, the smaller count on a tie.
// WIDE, measured at batch 8, 65 x 65 on 256 CUs (profiles/r20_conv3x3_wgrad_isolated.md): 128 -> 128 (9 tiles)
// 56 slices, 256 -> 256 (36) 14, 256 -> 512 (72) 7 -- one full round each, the counts on either side are slower -- and 512 -> 512
// (144 tiles) 7 slices = 1008 workgroups in two rounds, 10 % ahead of the 3 slices of a single, 84 % full round and 26 % ahead of
// 4 slices (one round and an eighth).
// NARROW (profiles/r23_conv3x3_narrow_wgrad_isolated.md has the sweep): at most ONE round.  The stem's 32,768 K-tiles over five
// tiles would take 307 slices for two rounds against 153 for one, for a cost of 214 against 215 K-tiles: twice the workspace and
// twice the reduce launch for nothing.
// TAPS == 1: H, W are the INPUT's sizes and the pixels summed over are the output's, (H - 1) / stride + 1 by (W - 1) / stride + 1.
template <bool NARROW, int TAPS = 9>
int plan_of(int B, int H, int W, int Cin, int Cout, int slices, int cus, int64_t *plan, int stride = 1) {
  if (!plan || B < 1 || H < 1 || W < 1 || slices < 0 || cus < 0 || stride < 1) return 0;
  if (!supported<NARROW>(Cin, Cout, 1, 1, 1, 1)) return 0;
  if ((int64_t)B * H * W >= kMaxPixels) return 0;
  const int64_t P = (int64_t)B * ((H - 1) / stride + 1) * ((W - 1) / stride + 1);
  const int64_t nk = cdiv(P, kBK);
  int64_t want = slices;
  if (want == 0) {
    const int64_t tiles = Form<NARROW, TAPS>::tiles(Cin, Cout), slots = Form<NARROW>::per_cu * (int64_t)(cus > 0 ? cus : 256);
    int64_t most = Form<NARROW>::max_rounds * slots / tiles, best = 0;
    if (most < 1) most = 1;
    if (most > nk) most = nk;
    for (int64_t s = 1; s <= most; ++s) {
      const int64_t cost = cdiv(tiles * s, slots) * cdiv(nk, s);
      if (want == 0 || cost < best) {
        want = s;
        best = cost;
      }
    }
  }
  int64_t used, per_slice;
  cover(nk, want, used, per_slice);
  plan[0] = used;
  plan[1] = per_slice;
  plan[2] = used * TAPS * Cin * Cout * (int64_t)sizeof(float);
  return 1;
}

// TAPS == 1: `dilation` is 1, x has H x W pixels an image and g (H - 1) / stride + 1 by (W - 1) / stride + 1 (plan_of).
template <bool NARROW, int TAPS = 9, int PIECES = 3, int FMT = kBf16>
int launch(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const float *g, float *dw, int64_t sn, int64_t sc,
           int64_t sy, int64_t sx, void *workspace, int64_t workspace_bytes, int slices, skd_stream_t stream, int stride = 1,
           const uint32_t *word = nullptr) {
  if (!x || !g || !dw || !workspace || B < 1 || H < 1 || W < 1 || stride < 1) return 0;
  if (reinterpret_cast<uintptr_t>(word) & 3) return 0;
  if (dilation < 1 || dilation > kMaxDilation || !supported<NARROW>(Cin, Cout, 1, dilation, dilation, 1)) return 0;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(workspace)) & 15) return 0;
  if (sn < 0 || sc < 0 || sy < 0 || sx < 0) return 0;
  if ((int64_t)B * H * W >= kMaxPixels) return 0;
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  const int64_t P = (int64_t)B * Ho * Wo;
  const int64_t nk = cdiv(P, kBK);
  if (slices < 1 || slices > nk) return 0;
  int64_t used, per_slice;
  cover(nk, slices, used, per_slice);
  if (used != slices) return 0;                              // not a count the plan returns: geometry is decided there
  const int64_t slab = TAPS * (int64_t)Cin * Cout;
  if (workspace_bytes < used * slab * (int64_t)sizeof(float)) return 0;
  const int64_t total = Form<NARROW, TAPS>::tiles(Cin, Cout) * used;
  const int64_t grid = cdiv(total, 8) * 8;
  const int64_t quads = slab / 4, rgrid = cdiv(quads, kThreads);
  if (grid > 2147483647 || rgrid > 2147483647) return 0;
  static PerDeviceFlag ready;
  bool *rdy = ready.get();
  if (rdy == nullptr) return 0;
  if (!*rdy) {
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(conv3x3_wgrad_kernel<NARROW, TAPS, PIECES, FMT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)conv_lds(PIECES)) != hipSuccess) return 0;
    *rdy = true;
  }
  hipStream_t st = as_stream(stream);
  float *part = static_cast<float *>(workspace);
  conv3x3_wgrad_kernel<NARROW, TAPS, PIECES, FMT><<<dim3((unsigned)grid), dim3(kThreads), conv_lds(PIECES), st>>>(
      x, g, part, (int)P, Ho, Wo, Cin, Cout, TAPS == 1 ? stride : dilation, (int)nk, (int)per_slice, (int)used,
      reciprocal32((unsigned)(Ho * Wo)), reciprocal32((unsigned)Wo), (int)total, H, W, word);
  if (!ok()) return 0;
  const bool vec = sc == 1 && (sn | sy | sx) % 4 == 0 && (reinterpret_cast<uintptr_t>(dw) & 15) == 0;
  const dim3 rg((unsigned)rgrid), rb(kThreads);
  if (NARROW) {
    if (vec) conv3x3_wgrad_reduce_rows_kernel<true><<<rg, rb, 0, st>>>(part, dw, Cin, Cout, quads, slab, (int)used, sn, sc, sy, sx);
    else conv3x3_wgrad_reduce_rows_kernel<false><<<rg, rb, 0, st>>>(part, dw, Cin, Cout, quads, slab, (int)used, sn, sc, sy, sx);
  } else {
    if (vec) conv3x3_wgrad_reduce_kernel<true><<<rg, rb, 0, st>>>(part, dw, Cin, quads, slab, (int)used, sn, sc, sy, sx, TAPS);
    else conv3x3_wgrad_reduce_kernel<false><<<rg, rb, 0, st>>>(part, dw, Cin, quads, slab, (int)used, sn, sc, sy, sx, TAPS);
  }
  return ok();
}

}  // namespace
}  // namespace skd

using namespace skd;

extern "C" {

int skd_conv3x3_split_wgrad_supported(int Cin, int Cout, int stride, int padding, int dilation, int groups) {
  return supported<false>(Cin, Cout, stride, padding, dilation, groups);
}

int skd_conv3x3_split_wgrad_plan(int B, int H, int W, int Cin, int Cout, int slices, int cus, int64_t *plan) {
  return plan_of<false>(B, H, W, Cin, Cout, slices, cus, plan);
}

int skd_conv3x3_split_wgrad_nhwc(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const float *g, float *dw,
                                 int64_t sn, int64_t sc, int64_t sy, int64_t sx, void *workspace, int64_t workspace_bytes,
                                 int slices, skd_stream_t stream) {
  return launch<false>(B, H, W, Cin, Cout, dilation, x, g, dw, sn, sc, sy, sx, workspace, workspace_bytes, slices, stream);
}

int skd_conv3x3_narrow_wgrad_supported(int Cin, int Cout, int stride, int padding, int dilation, int groups) {
  return supported<true>(Cin, Cout, stride, padding, dilation, groups);
}

int skd_conv3x3_narrow_wgrad_plan(int B, int H, int W, int Cin, int Cout, int slices, int cus, int64_t *plan) {
  return plan_of<true>(B, H, W, Cin, Cout, slices, cus, plan);
}

int skd_conv3x3_narrow_wgrad_nhwc(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const float *g, float *dw,
                                  int64_t sn, int64_t sc, int64_t sy, int64_t sx, void *workspace, int64_t workspace_bytes,
                                  int slices, skd_stream_t stream) {
  return launch<true>(B, H, W, Cin, Cout, dilation, x, g, dw, sn, sc, sy, sx, workspace, workspace_bytes, slices, stream);
}

// Two pieces per operand (skd_train2.h): the predicate, the plan and the workspace of the three-piece entries, the wide kernel
// with PIECES = 2 and the same reduce launch.
int skd_conv3x3_split2_wgrad_plan(int B, int H, int W, int Cin, int Cout, int slices, int cus, int64_t *plan) {
  return plan_of<false>(B, H, W, Cin, Cout, slices, cus, plan);
}

int skd_conv3x3_split2_wgrad_nhwc(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const float *g, float *dw,
                                  int64_t sn, int64_t sc, int64_t sy, int64_t sx, void *workspace, int64_t workspace_bytes,
                                  int slices, skd_stream_t stream) {
  return launch<false, 9, 2>(B, H, W, Cin, Cout, dilation, x, g, dw, sn, sc, sy, sx, workspace, workspace_bytes, slices, stream);
}

// Two FP16 pieces per operand and the scale word of g (skd_train2h.h): the same predicate, plan, workspace and reduce launch.
int skd_conv3x3_split2h_wgrad_plan(int B, int H, int W, int Cin, int Cout, int slices, int cus, int64_t *plan) {
  return plan_of<false>(B, H, W, Cin, Cout, slices, cus, plan);
}

int skd_conv3x3_split2h_wgrad_nhwc(int B, int H, int W, int Cin, int Cout, int dilation, const float *x, const float *g, float *dw,
                                   int64_t sn, int64_t sc, int64_t sy, int64_t sx, void *workspace, int64_t workspace_bytes,
                                   const uint32_t *word, int slices, skd_stream_t stream) {
  return launch<false, 9, 2, kFp16>(B, H, W, Cin, Cout, dilation, x, g, dw, sn, sc, sy, sx, workspace, workspace_bytes, slices, stream, 1,
                                    word);
}

// The 1x1 convolution of stride 1 or 2 (skd_shortcut.h): the one-tap form of the kernel, the 128 x 128 tiles where both channel
// counts are multiples of 128 and the 128 x 64 ones otherwise; dw is the dense (Cout, Cin) matrix.
int skd_conv1x1_train_wgrad_plan(int B, int H, int W, int Cin, int Cout, int stride, int slices, int cus, int64_t *plan) {
  if (stride != 1 && stride != 2) return 0;
  return supported<false>(Cin, Cout, 1, 1, 1, 1) ? plan_of<false, 1>(B, H, W, Cin, Cout, slices, cus, plan, stride)
                                                 : plan_of<true, 1>(B, H, W, Cin, Cout, slices, cus, plan, stride);
}

int skd_conv1x1_train_wgrad_nhwc(int B, int H, int W, int Cin, int Cout, int stride, const float *x, const float *g, float *dw,
                                 void *workspace, int64_t workspace_bytes, int slices, skd_stream_t stream) {
  if (stride != 1 && stride != 2) return 0;
  return supported<false>(Cin, Cout, 1, 1, 1, 1)
             ? launch<false, 1>(B, H, W, Cin, Cout, 1, x, g, dw, Cin, 1, 0, 0, workspace, workspace_bytes, slices, stream, stride)
             : launch<true, 1>(B, H, W, Cin, Cout, 1, x, g, dw, Cin, 1, 0, 0, workspace, workspace_bytes, slices, stream, stride);
}

}  // extern "C"
