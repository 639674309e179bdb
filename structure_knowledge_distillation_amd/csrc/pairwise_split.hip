// pairwise_split.hip -- the two matrix products of the pair-wise similarity loss (pairwise.hip) on the split-operand bf16-MFMA
// core (conv_split_dev.hpp; what the core computes and why is documented at the top of conv1x1.hip): fp32 in, fp32 out,
// include/skd_pairwise_split.h.  The fp32-MFMA kernels of pairwise.hip stay as they are; these are their opt-in twins.
//
// Both products are one GEMM  Y[TM rows][128 columns] = A[rows][K] . Bm[columns][K]^T  with both operands K-contiguous, the tile of
// conv1x1_train.hip: 64 x 128 per workgroup (a wave tile of 32 x 64), TWO accumulator sets (a0 b0 apart from the five smaller
// products, added in the epilogue), k_loop's two K-tiles of load look-ahead, 48 KB of LDS, three workgroups per compute unit.
//
//   Gram + loss   G = Fh_T^T Fh_T - Fh_S^T Fh_S.  The normalised panels are channel-major (k-major), so the entry first makes ONE
//                 node-major copy X (B, ldm, Kp) in its workspace -- teacher channels, zeros up to a multiple of 16, student
//                 channels, zeros up to a multiple of 16: a K tail contributes zeros -- with a coalesced 32 x 32 LDS transpose
//                 (pairwise.hip's transpose_pad_kernel form).  Then A = rows i of X, Bm = rows j of X, K = Kp, and the student's
//                 sign is applied to the A operand alone when its K-tiles are split into LDS (negation is exact in every piece).
//                 (Measured against it and dropped: a copy that is ALREADY SPLIT -- three bf16 planes in the 16-byte chunks of the
//                 LDS image, so that the loop moves chunks and splits nothing: 757 us against 732 us at B = 8, M = 4225, behind at
//                 M = 289; the split in the loop is not what this kernel waits for.  Transposing while staging, conv3x3_wgrad.hip's
//                 way, was not built: it splits four float4 on three waves where this splits three on four, to save a copy that is
//                 a twentieth of the launch.  profiles/r29_pairwise_split_isolated.md.)
//                 Only the tiles of the upper triangle run, two workgroups (64 rows each) per 128 x 128 tile, and every element is
//                 stored a second time in its mirror position.  The six products are NOT symmetric in (i, j) -- a0 b2 of (i, j) is
//                 a2 b0 of (j, i), at another place of the sum -- so a DIAGONAL tile also keeps only its elements with row <= col
//                 and mirrors them: G equals its transpose bit for bit.  The epilogue squares and reduces the tile (mirrored
//                 elements count twice) into one partial per workgroup; launch_final_sum adds them in a fixed order.
//   backward      dpooled[c][m] = coef g (sum_n Fh_S[c][n] G[m][n]) / norm_S[m]: G is symmetric, so A = rows c of Fh_S and
//                 Bm = rows m of G are K-contiguous as they lie (K = ldm): no copy, no transpose.  Few output tiles and a long
//                 contraction: when the tiles would not fill the chip the node range is cut into S slices, one workgroup each,
//                 whose raw tiles go to the workspace and are added in slice order by a second launch.
// Placement: workgroup x runs on XCD x % 8, and XCD q owns the q-th eighth of the work list in order, so work items that are
// neighbours in the list run on one XCD at about the same time.  The lists are ordered so that neighbours share an operand panel:
// the Gram tiles of one 64-row panel of X, tj ascending; the channel tiles of one 128-row panel of G.
#include "conv_split_dev.hpp"
#include "skd_pairwise_split.h"

namespace skd {
namespace {

constexpr int kDepthPair = 2;                          // K-tiles of load look-ahead (k_loop)
constexpr int kPTM = 64;                               // rows of a tile: one float4 of the A panel per thread and K-tile
constexpr int kMaxChannels = 1 << 20;                  // Cs + Ct of the Gram entry
constexpr int kFillWG = 512;                           // workgroups the backward wants before it stops cutting the node range

struct PairStg {
  float4 a, b[kTN / kRPP];
};

// What k_loop needs of a tile: A rows and Bm rows `ld` floats apart, both K-contiguous.  K-tiles kt >= kneg of the A operand are
// negated on their way into LDS (the student's segment of the Gram product; INT_MAX: none).
struct PairTile {
  typedef PairStg Stg;
  const float *__restrict__ A, *__restrict__ Bm;
  int64_t aoff, boff, ld;              // floats from A / Bm to the thread's row at K-tile 0, the k quad included
  int srow, kneg;                      // 8-byte slot of this thread's (row, k quad) in an operand's LDS image
  f32x16 (&low)[1][2], (&acc)[1][2];
  __device__ __forceinline__ void load(Stg &s, int kt) const {
    s.a = *reinterpret_cast<const float4 *>(A + aoff + kt * kBK);
#pragma unroll
    for (int h = 0; h < kTN / kRPP; ++h) s.b[h] = *reinterpret_cast<const float4 *>(Bm + boff + (int64_t)(kRPP * h) * ld + kt * kBK);
  }
  __device__ __forceinline__ void store(const Stg &s, uint4 *stage, int kt) const {
    uint2 *sa = reinterpret_cast<uint2 *>(stage) + srow, *sb = reinterpret_cast<uint2 *>(stage + kOperandChunks) + srow;
    const float sign = kt >= kneg ? -1.f : 1.f;
    split_store(make_float4(s.a.x * sign, s.a.y * sign, s.a.z * sign, s.a.w * sign), sa);
#pragma unroll
    for (int h = 0; h < kTN / kRPP; ++h) split_store(s.b[h], sb + 2 * kRPP * h);
  }
  __device__ __forceinline__ void mma(const uint4 *stage) const { tile_mma<kPTM, kTN>(stage, low, acc); }
};

__device__ __forceinline__ void clear(f32x16 (&a)[1][2], f32x16 (&b)[1][2]) {
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int q = 0; q < 16; ++q) a[0][j][q] = b[0][j][q] = 0.f;
}

// Work item of this workgroup: XCD q = blockIdx.x % 8 owns items [q * chunk, (q + 1) * chunk) of the list, in order.
__device__ __forceinline__ int work_item(int chunk) { return (int)(blockIdx.x & 7) * chunk + (int)(blockIdx.x >> 3); }

// X[b][n][kk]: kk < Ct the teacher's channel kk, Ktp <= kk < Ktp + Cs the student's channel kk - Ktp, zero elsewhere.
// 32 x 32 tiles through LDS; grid (ldm / 32, ceil(Kp / 32), B), block 256 = 32 x 8.
__global__ __launch_bounds__(kThreads) void pairwise_split_pack_kernel(const float *__restrict__ fs, const float *__restrict__ ft,
                                                                      float *__restrict__ X, int Cs, int Ct, int Ktp, int Kp, int ldm) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int b = blockIdx.z, n0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int kk = k0 + ty + 8 * r;
    float v = 0.f;
    if (kk < Ct) v = ft[((int64_t)b * Ct + kk) * ldm + n0 + tx];
    else if (kk >= Ktp && kk - Ktp < Cs) v = fs[((int64_t)b * Cs + (kk - Ktp)) * ldm + n0 + tx];
    tile[ty + 8 * r][tx] = v;
  }
  __syncthreads();
  const int kk = k0 + tx;
  if (kk < Kp) {
#pragma unroll
    for (int r = 0; r < 4; ++r) X[((int64_t)b * ldm + n0 + ty + 8 * r) * Kp + kk] = tile[tx][ty + 8 * r];
  }
}

// grid (8 * chunk, B); work list of one image: the 64-row halves (ti, half) of the upper triangle's tiles, tj = ti .. ntiles - 1
// for each, `total` = ntiles (ntiles + 1) items.
__global__ __launch_bounds__(kThreads, kMinWG) void pairwise_split_gram_kernel(const float *__restrict__ X, float *__restrict__ G,
                                                                              float *__restrict__ part, int Kp, int kneg, int ldm,
                                                                              int ntiles, int total, int chunk) {
  extern __shared__ __attribute__((aligned(16))) uint4 lds[];
  const int item = work_item(chunk);
  if (item >= total) return;                             // the grid is padded to whole eighths
  const int b = blockIdx.y;
  int ti = 0, rem = item;
  while (rem >= 2 * (ntiles - ti)) {
    rem -= 2 * (ntiles - ti);
    ++ti;
  }
  const int half = rem / (ntiles - ti), tj = ti + rem - half * (ntiles - ti);
  const int i0 = ti * kTN + half * kPTM, j0 = tj * kTN;

  f32x16 acc[1][2], low[1][2];        // a0 b0 | the five smaller products (tile_mma): added in the epilogue
  clear(acc, low);
  const int gt = threadIdx.x, grow = gt / kQK, gkq = (gt % kQK) * 4;
  const float *Xb = X + (int64_t)b * ldm * Kp;
  PairTile tile = {Xb, Xb, (int64_t)(i0 + grow) * Kp + gkq, (int64_t)(j0 + grow) * Kp + gkq, Kp, plane_slot(grow, gkq), kneg, low, acc};
  k_loop<kDepthPair>(tile, Kp / kBK, lds);

  // ---- epilogue: square, store, mirror.  tile_mma's wave map; rows row0 .. row0 + 3 of column col = registers 4 q .. 4 q + 3 ----
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  const int wi = (wid >> 1) * (kPTM / 2), wj = (wid & 1) * 64;
  const bool diag = ti == tj;
  float *Gb = G != nullptr ? G + (int64_t)b * ldm * ldm : nullptr;
  float sq = 0.f, unused = 0.f;
#pragma unroll
  for (int bj = 0; bj < 2; ++bj) {
    const int col = j0 + wj + bj * 32 + (lane & 31);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row0 = i0 + wi + 8 * q + 4 * (lane >> 5);
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = acc[0][bj][4 * q + r] + low[0][bj][4 * q + r];
      if (!diag) {
        sq += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);  // doubled below; padded rows / columns are exactly zero
        if (Gb != nullptr) {
#pragma unroll
          for (int r = 0; r < 4; ++r) Gb[(int64_t)(row0 + r) * ldm + col] = v[r];
          *reinterpret_cast<float4 *>(Gb + (int64_t)col * ldm + row0) = make_float4(v[0], v[1], v[2], v[3]);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = row0 + r;
          if (row > col) continue;                       // the mirror of (col, row), which this or the other half keeps
          sq += row < col ? 2.f * (v[r] * v[r]) : v[r] * v[r];
          if (Gb != nullptr) {
            Gb[(int64_t)row * ldm + col] = v[r];
            if (row < col) Gb[(int64_t)col * ldm + row] = v[r];
          }
        }
      }
    }
  }
  if (!diag) sq *= 2.f;
  block_sum2(sq, unused, reinterpret_cast<float *>(lds));  // the LDS ring is free: k_loop ends on a barrier
  if (threadIdx.x == 0) part[(int64_t)b * total + item] = sq;
}

// The backward's geometry: pure host arithmetic.
struct BwdPlan {
  int ntm, ntc, nk, S, kts, total;     // column (node) tiles, channel tiles, K-tiles, slices, K-tiles per slice, items per image
};
BwdPlan bwd_plan(int B, int Cs, int ldm) {
  BwdPlan p;
  p.ntm = ldm / kTN;
  p.ntc = (int)cdiv(Cs, kPTM);
  p.nk = ldm / kBK;
  const int64_t tiles = (int64_t)p.ntm * p.ntc * B;
  int64_t S = cdiv(kFillWG, tiles);
  if (S > p.nk / 8) S = p.nk / 8;                        // never fewer than 8 K-tiles per workgroup (ldm >= 128: nk >= 8)
  if (S < 1) S = 1;
  p.kts = (int)cdiv(p.nk, S);
  p.S = (int)cdiv(p.nk, p.kts);                          // exact cover: no slice is empty
  const int64_t total = (int64_t)p.ntm * p.S * p.ntc;
  p.total = total > 2147483647 - 8 ? -1 : (int)total;    // -1: refused (the grid is padded to a multiple of 8)
  return p;
}

// grid (8 * chunk, B); work list of one image: (tm, slice, tc), tc fastest -- the channel tiles that read one panel of G.
__global__ __launch_bounds__(kThreads, kMinWG) void pairwise_split_bwd_kernel(const float *__restrict__ fs, const float *__restrict__ G,
                                                                             const float *__restrict__ norm,
                                                                             const float *__restrict__ gscale,
                                                                             float *__restrict__ dpooled, float *__restrict__ part,
                                                                             int Cs, int M, int ldm, BwdPlan p, int chunk, float coef) {
  extern __shared__ __attribute__((aligned(16))) uint4 lds[];
  const int item = work_item(chunk);
  if (item >= p.total) return;
  const int b = blockIdx.y;
  const int tc = item % p.ntc, sl = (item / p.ntc) % p.S, tm = item / (p.ntc * p.S);
  const int c0 = tc * kPTM, m0 = tm * kTN, kt0 = sl * p.kts;
  const int nkl = p.nk - kt0 < p.kts ? p.nk - kt0 : p.kts;

  f32x16 acc[1][2], low[1][2];
  clear(acc, low);
  const int gt = threadIdx.x, grow = gt / kQK, gkq = (gt % kQK) * 4;
  const int crow = c0 + grow < Cs ? c0 + grow : Cs - 1;  // rows beyond the matrix are clamped (loaded, multiplied, never stored)
  PairTile tile = {fs + (int64_t)b * Cs * ldm + (int64_t)kt0 * kBK, G + (int64_t)b * ldm * ldm + (int64_t)kt0 * kBK,
                   (int64_t)crow * ldm + gkq, (int64_t)(m0 + grow) * ldm + gkq, ldm, plane_slot(grow, gkq), 0x7fffffff, low, acc};
  k_loop<kDepthPair>(tile, nkl, lds);

  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  const int wi = (wid >> 1) * (kPTM / 2), wj = (wid & 1) * 64;
  if (p.S == 1) {
    const float scale = coef * gscale[0];
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
      const int m = m0 + wj + bj * 32 + (lane & 31);
      const float inv = m < M ? scale / norm[(int64_t)b * M + m] : 0.f;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int c = c0 + wi + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
        if (c < Cs) dpooled[((int64_t)b * Cs + c) * ldm + m] = m < M ? (acc[0][bj][q] + low[0][bj][q]) * inv : 0.f;
      }
    }
  } else {
    // raw partial of this slice, (64, 128) row-major; the clamped rows are written too (the second launch reads whole tiles)
    float *dst = part + ((int64_t)b * p.total + item) * (kPTM * kTN);
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
      const int ml = wj + bj * 32 + (lane & 31);
#pragma unroll
      for (int q = 0; q < 16; ++q) dst[(wi + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5)) * kTN + ml] = acc[0][bj][q] + low[0][bj][q];
    }
  }
}

// grid (ntm * ntc, B): dpooled tile = coef g / norm * (slice 0 + slice 1 + ...), in slice order; columns >= M: +0.0.
__global__ __launch_bounds__(kThreads) void pairwise_split_bwd_sum_kernel(const float *__restrict__ part, const float *__restrict__ norm,
                                                                         const float *__restrict__ gscale, float *__restrict__ dpooled,
                                                                         int Cs, int M, int ldm, BwdPlan p, float coef) {
  const int b = blockIdx.y;
  const int tc = blockIdx.x % p.ntc, tm = blockIdx.x / p.ntc;
  const int c0 = tc * kPTM, m0 = tm * kTN;
  const float scale = coef * gscale[0];
  const float *nr = norm + (int64_t)b * M;
  for (int e = threadIdx.x; e < kPTM * kTN / 4; e += kThreads) {
    const int cl = e >> 5, ml = (e & 31) * 4;            // 32 float4 per tile row
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int sl = 0; sl < p.S; ++sl) {
      const int item = (tm * p.S + sl) * p.ntc + tc;
      const float4 v = *reinterpret_cast<const float4 *>(part + ((int64_t)b * p.total + item) * (kPTM * kTN) + cl * kTN + ml);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    const int c = c0 + cl, m = m0 + ml;
    if (c >= Cs) continue;
    float4 o;
    o.x = m + 0 < M ? s.x * (scale / nr[m + 0]) : 0.f;
    o.y = m + 1 < M ? s.y * (scale / nr[m + 1]) : 0.f;
    o.z = m + 2 < M ? s.z * (scale / nr[m + 2]) : 0.f;
    o.w = m + 3 < M ? s.w * (scale / nr[m + 3]) : 0.f;
    *reinterpret_cast<float4 *>(dpooled + ((int64_t)b * Cs + c) * ldm + m) = o;
  }
}

template <class Kernel>
bool lds_ready(Kernel kernel, PerDeviceFlag &flag) {
  bool *rdy = flag.get();
  if (rdy == nullptr) return false;
  if (!*rdy) {
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kConvLds) != hipSuccess)
      return false;
    *rdy = true;
  }
  return true;
}

int round16(int c) { return (int)(cdiv(c, kBK) * kBK); }
bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace skd

using namespace skd;

extern "C" {

int64_t skd_pairwise_split_workspace_floats(int B, int Cs, int Ct, int M) {
  if (B <= 0 || Cs <= 0 || Ct <= 0 || M <= 0 || (int64_t)Cs + Ct > kMaxChannels) return 1;
  const int64_t ldm = skd_pairwise_ldm(M), ntiles = ldm / kTN;
  return (int64_t)B * ldm * (round16(Cs) + round16(Ct)) + ntiles * (ntiles + 1) * B;
}

int skd_pairwise_split_gram_loss(int B, int Cs, int Ct, int M, int ldm, const float *fhat_s, const float *fhat_t, float *G,
                                 float *loss, float *workspace, skd_stream_t stream) {
  if (B <= 0 || Cs <= 0 || Ct <= 0 || M <= 0 || !fhat_s || !fhat_t || !loss || !workspace) return 0;
  if (ldm != skd_pairwise_ldm(M) || B > 65535 || (int64_t)Cs + Ct > kMaxChannels) return 0;
  if (!aligned16(fhat_s) || !aligned16(fhat_t) || !aligned16(G) || !aligned16(workspace)) return 0;
  const int Ktp = round16(Ct), Kp = Ktp + round16(Cs);
  const int ntiles = ldm / kTN;
  const int64_t total = (int64_t)ntiles * (ntiles + 1), chunk = cdiv(total, 8);
  if (chunk * 8 > 2147483647 || cdiv(Kp, 32) > 65535) return 0;
  static PerDeviceFlag ready;
  if (!lds_ready(pairwise_split_gram_kernel, ready)) return 0;
  hipStream_t st = as_stream(stream);
  float *X = workspace, *part = workspace + (int64_t)B * ldm * Kp;
  pairwise_split_pack_kernel<<<dim3((unsigned)(ldm / 32), (unsigned)cdiv(Kp, 32), B), dim3(kThreads), 0, st>>>(fhat_s, fhat_t, X, Cs, Ct,
                                                                                                              Ktp, Kp, ldm);
  if (!ok()) return 0;
  pairwise_split_gram_kernel<<<dim3((unsigned)(chunk * 8), B), dim3(kThreads), kConvLds, st>>>(X, G, part, Kp, Ktp / kBK, ldm, ntiles,
                                                                                              (int)total, (int)chunk);
  if (!ok()) return 0;
  // utils.py:181: / (M*M) / B
  return launch_final_sum(part, total * B, loss, 1.0 / ((double)M * (double)M) / (double)B, st);
}

int64_t skd_pairwise_split_backward_workspace_floats(int B, int Cs, int M) {
  if (B <= 0 || Cs <= 0 || M <= 0) return 1;
  const BwdPlan p = bwd_plan(B, Cs, skd_pairwise_ldm(M));
  return p.S == 1 || p.total < 0 ? 1 : (int64_t)B * p.total * (kPTM * kTN);
}

int skd_pairwise_split_backward(int B, int Cs, int M, int ldm, const float *fhat_s, const float *G, const float *norm_s,
                                const float *grad_loss, float *dpooled, float *workspace, skd_stream_t stream) {
  if (B <= 0 || Cs <= 0 || M <= 0 || !fhat_s || !G || !norm_s || !grad_loss || !dpooled || !workspace) return 0;
  if (ldm != skd_pairwise_ldm(M) || B > 65535) return 0;
  if (!aligned16(fhat_s) || !aligned16(G) || !aligned16(dpooled) || !aligned16(workspace)) return 0;
  const BwdPlan p = bwd_plan(B, Cs, ldm);
  if (p.total < 0) return 0;
  const int64_t chunk = cdiv(p.total, 8);
  static PerDeviceFlag ready;
  if (!lds_ready(pairwise_split_bwd_kernel, ready)) return 0;
  // dL/dA_S = -2 G /(M^2 B); dFhat = Fhat (dA + dA^T) = -4/(M^2 B) Fhat G   (G symmetric)
  const float coef = (float)(-4.0 / ((double)M * (double)M * (double)B));
  hipStream_t st = as_stream(stream);
  pairwise_split_bwd_kernel<<<dim3((unsigned)(chunk * 8), B), dim3(kThreads), kConvLds, st>>>(fhat_s, G, norm_s, grad_loss, dpooled,
                                                                                             workspace, Cs, M, ldm, p, (int)chunk, coef);
  if (!ok()) return 0;
  if (p.S == 1) return 1;
  pairwise_split_bwd_sum_kernel<<<dim3((unsigned)(p.ntm * p.ntc), B), dim3(kThreads), 0, st>>>(workspace, norm_s, grad_loss, dpooled, Cs,
                                                                                              M, ldm, p, coef);
  return ok();
}

}  // extern "C"
