// abn_nhwc.hip -- InPlace-ABN for channels-last (NHWC) tensors: the inference apply pass, the training apply / dx passes (one
// 256-thread workgroup per 32 KiB slab), the one-launch ticket reductions (statistics, edz / eydz) with the library's
// ticket-counter pool, and the two-launch entries.  The register-resident one-launch passes on top of them are in
// abn_fused.hip, the planar NCHW passes in abn.hip, the shared device helpers and geometries in abn_dev.hpp.
#include "abn_dev.hpp"
#include "skd_bnstats.h"

namespace skd {
namespace {

// ---------------------------------------------------------------------------------------------
// Inference BN -> (+ residual) -> activation for channels-last (NHWC) tensors: x is (rows = N*H*W, C) row-major,
// the channel is the fastest dimension, so every thread keeps ONE channel quad's parameters in registers and
// streams rows with 16-byte accesses.  Used by the frozen teacher, whose convolutions run NHWC-native in MIOpen
// (no NCHW<->NHWC transposes around the igemm kernels).  C must be a multiple of 4.
// ---------------------------------------------------------------------------------------------
// Fast form for power-of-two channel counts (every layer of this path): a workgroup owns a contiguous run of
// 256 * 8 quads (32 KiB); quad q of thread t sits at base + u*256 + t, so its channel quad is (t + u*256) mod C4 --
// constant for C4 <= 256, cycling through NSETS = C4/256 register sets above that.  Eight 16-byte loads per lane.
template <int ACT, bool HAS_RES, int NSETS>
__global__ __launch_bounds__(kThreads) void abn_apply_nhwc_kernel(float *x, const float *res,
                                                                 const float *__restrict__ mean,
                                                                 const float *__restrict__ var,
                                                                 const float *__restrict__ weight,
                                                                 const float *__restrict__ bias, float eps,
                                                                 float slope, int64_t quads, int C4) {
  constexpr int U = 8;
  const int64_t base = (int64_t)blockIdx.x * (kThreads * U);
  float m[NSETS][4], is[NSETS][4], g[NSETS][4], b[NSETS][4];
#pragma unroll
  for (int s = 0; s < NSETS; ++s) {
    const int c = ((threadIdx.x + s * kThreads) & (C4 - 1)) * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) load_bn_params(mean, var, weight, bias, c + k, eps, m[s][k], is[s][k], g[s][k], b[s][k]);
  }
  float4 v[U], r[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t q = base + u * kThreads + threadIdx.x;
    if (q < quads) {
      v[u] = *reinterpret_cast<const float4 *>(x + 4 * q);
      if (HAS_RES) r[u] = *reinterpret_cast<const float4 *>(res + 4 * q);
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t q = base + u * kThreads + threadIdx.x;
    if (q < quads) {
      constexpr int dummy = 0;
      const int s = NSETS == 1 ? dummy : (u % NSETS);
      float4 z;
      z.x = act_fwd<ACT>(((v[u].x - m[s][0]) * is[s][0]) * g[s][0] + b[s][0] + (HAS_RES ? r[u].x : 0.f), slope);
      z.y = act_fwd<ACT>(((v[u].y - m[s][1]) * is[s][1]) * g[s][1] + b[s][1] + (HAS_RES ? r[u].y : 0.f), slope);
      z.z = act_fwd<ACT>(((v[u].z - m[s][2]) * is[s][2]) * g[s][2] + b[s][2] + (HAS_RES ? r[u].z : 0.f), slope);
      z.w = act_fwd<ACT>(((v[u].w - m[s][3]) * is[s][3]) * g[s][3] + b[s][3] + (HAS_RES ? r[u].w : 0.f), slope);
      *reinterpret_cast<float4 *>(x + 4 * q) = z;
    }
  }
}

// generic channel counts (any C % 4 == 0): grid-stride, total threads a multiple of C4
template <int ACT, bool HAS_RES>
__global__ __launch_bounds__(kThreads) void abn_apply_nhwc_generic_kernel(float *x, const float *res,
                                                                 const float *__restrict__ mean,
                                                                 const float *__restrict__ var,
                                                                 const float *__restrict__ weight,
                                                                 const float *__restrict__ bias, float eps,
                                                                 float slope, int64_t quads, int C4) {
  // total threads is a multiple of C4, so a thread's channel quad never changes while it strides
  const int64_t T = (int64_t)gridDim.x * kThreads;
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int c = (int)(t % C4) * 4;
  float m[4], is[4], g[4], b[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) load_bn_params(mean, var, weight, bias, c + k, eps, m[k], is[k], g[k], b[k]);
  for (int64_t q = t; q < quads; q += 4 * T) {
    float4 v[4], r[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t qq = q + u * T;
      if (qq < quads) {
        v[u] = *reinterpret_cast<const float4 *>(x + 4 * qq);
        if (HAS_RES) r[u] = *reinterpret_cast<const float4 *>(res + 4 * qq);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t qq = q + u * T;
      if (qq < quads) {
        float4 z;
        z.x = act_fwd<ACT>(((v[u].x - m[0]) * is[0]) * g[0] + b[0] + (HAS_RES ? r[u].x : 0.f), slope);
        z.y = act_fwd<ACT>(((v[u].y - m[1]) * is[1]) * g[1] + b[1] + (HAS_RES ? r[u].y : 0.f), slope);
        z.z = act_fwd<ACT>(((v[u].z - m[2]) * is[2]) * g[2] + b[2] + (HAS_RES ? r[u].z : 0.f), slope);
        z.w = act_fwd<ACT>(((v[u].w - m[3]) * is[3]) * g[3] + b[3] + (HAS_RES ? r[u].w : 0.f), slope);
        *reinterpret_cast<float4 *>(x + 4 * qq) = z;
      }
    }
  }
}

// =============================================================================================
// Channels-last (NHWC) TRAINING kernels: x is (rows = N*H*W, C) row-major.
// MIOpen's fastest fp32 kernels on gfx950 are NHWC implicit-GEMM kernels; handing it NCHW tensors costs a
// transpose before and after each of them (4.5 ms per step for the student's forward/backward, profiles/).
// With the channel as the fastest dimension a thread owns ONE channel quad (its statistics accumulate in
// registers, its parameters live in registers) and a workgroup walks a contiguous slab of rows:
//   256 threads = (256 / C4) rows x C4 channel quads per pass, 8 passes in flight per loop trip.
// The two apply-type passes (normalise, dx) below give every 32 KiB slab its own 256-thread workgroup; the reductions
// (statistics, edz / eydz) are the one-launch kernels of the "second design" section further down.
// Power-of-two C with 4 <= C <= 1024 (every training layer of this path: 64 ... 512).
// =============================================================================================

// K2 (NHWC), out of place or in place: out = act(bn(x) [+ residual]) with given mean / var
template <int ACT, bool HAS_RES>
__global__ __launch_bounds__(kThreads) void abn_apply_nhwc_train_kernel(const float *x, const float *res, float *out,
                                                                       const float *__restrict__ mean,
                                                                       const float *__restrict__ var,
                                                                       const float *__restrict__ weight,
                                                                       const float *__restrict__ bias, float eps,
                                                                       float slope, int64_t rows, NhwcGeom g) {
  const int t = threadIdx.x;
  const int cq = t & (g.C4 - 1), rsub = t >> g.log2C4;
  float m[4], is[4], gm[4], b[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) load_bn_params(mean, var, weight, bias, cq * 4 + k, eps, m[k], is[k], gm[k], b[k]);
  const int64_t r0 = (int64_t)blockIdx.x * g.rows_per_wg + rsub;
  float4 v[kNhwcRowsPerThread], r4[kNhwcRowsPerThread];
#pragma unroll
  for (int u = 0; u < kNhwcRowsPerThread; ++u) {
    const int64_t r = r0 + (int64_t)u * g.rpp;
    if (r < rows) {
      const int64_t o = (r << (g.log2C4 + 2)) + cq * 4;
      v[u] = *reinterpret_cast<const float4 *>(x + o);
      if (HAS_RES) r4[u] = *reinterpret_cast<const float4 *>(res + o);
    }
  }
#pragma unroll
  for (int u = 0; u < kNhwcRowsPerThread; ++u) {
    const int64_t r = r0 + (int64_t)u * g.rpp;
    if (r < rows) {
      float4 z;
      z.x = act_fwd<ACT>(HAS_RES ? bn_pre(v[u].x, m[0], is[0], gm[0], b[0]) + r4[u].x : bn_pre(v[u].x, m[0], is[0], gm[0], b[0]), slope);
      z.y = act_fwd<ACT>(HAS_RES ? bn_pre(v[u].y, m[1], is[1], gm[1], b[1]) + r4[u].y : bn_pre(v[u].y, m[1], is[1], gm[1], b[1]), slope);
      z.z = act_fwd<ACT>(HAS_RES ? bn_pre(v[u].z, m[2], is[2], gm[2], b[2]) + r4[u].z : bn_pre(v[u].z, m[2], is[2], gm[2], b[2]), slope);
      z.w = act_fwd<ACT>(HAS_RES ? bn_pre(v[u].w, m[3], is[3], gm[3], b[3]) + r4[u].w : bn_pre(v[u].w, m[3], is[3], gm[3], b[3]), slope);
      *reinterpret_cast<float4 *>(out + (r << (g.log2C4 + 2)) + cq * 4) = z;
    }
  }
}

// K4 (NHWC): dx (and dres for MODE 1), dweight / dbias by workgroup 0.  MODE 2 = MODE 1 for a forward WITHOUT residual:
// inputs (x, dout), the ReLU mask is recomputed from x (bn_pre > 0) -- 4 bytes per element less than reading `out`.
template <int ACT, int MODE, bool WRITE_RES>
__global__ __launch_bounds__(kThreads) void abn_grad_dx_nhwc_kernel(
    const float *a_, const float *b_, const float *c_, const float *__restrict__ mean,
    const float *__restrict__ var, const float *__restrict__ weight, const float *__restrict__ bias,
    const float *__restrict__ edz, const float *__restrict__ eydz, float *dx, float *dres, float *dweight,
    float *dbias, float eps, float slope, int64_t rows, NhwcGeom g, int accumulate) {
  const int t = threadIdx.x;
  const int cq = t & (g.C4 - 1), rsub = t >> g.log2C4;
  float p0[4], p1[4], e[4], ey[4], mul[4], gm[4], bt[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = cq * 4 + k;
    load_grad_params<MODE, true>(mean, var, weight, bias, c, eps, p0[k], p1[k], gm[k], bt[k], mul[k]);
    e[k] = edz[c];
    ey[k] = eydz[c];
  }
  const float inv_slope = 1.f / slope;
  const int64_t r0 = (int64_t)blockIdx.x * g.rows_per_wg + rsub;
  float4 va[kNhwcRowsPerThread], vb[kNhwcRowsPerThread], vc[kNhwcRowsPerThread];
#pragma unroll
  for (int u = 0; u < kNhwcRowsPerThread; ++u) {
    const int64_t r = r0 + (int64_t)u * g.rpp;
    if (r < rows) {
      const int64_t o = (r << (g.log2C4 + 2)) + cq * 4;
      va[u] = *reinterpret_cast<const float4 *>(a_ + o);
      vb[u] = *reinterpret_cast<const float4 *>(b_ + o);
      if (MODE == 1) vc[u] = *reinterpret_cast<const float4 *>(c_ + o);
    }
  }
#pragma unroll
  for (int u = 0; u < kNhwcRowsPerThread; ++u) {
    const int64_t r = r0 + (int64_t)u * g.rpp;
    if (r < rows) {
      const float A[4] = {va[u].x, va[u].y, va[u].z, va[u].w};
      const float B[4] = {vb[u].x, vb[u].y, vb[u].z, vb[u].w};
      const float Cc[4] = {MODE == 1 ? vc[u].x : 0.f, MODE == 1 ? vc[u].y : 0.f, MODE == 1 ? vc[u].z : 0.f,
                           MODE == 1 ? vc[u].w : 0.f};
      float D[4], R[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float y, dz;
        grad_elem<ACT, MODE>(A[k], B[k], Cc[k], p0[k], p1[k], gm[k], bt[k], slope, inv_slope, y, dz);
        D[k] = (dz - e[k] - y * ey[k]) * mul[k];
        R[k] = dz;
      }
      const int64_t o = (r << (g.log2C4 + 2)) + cq * 4;
      *reinterpret_cast<float4 *>(dx + o) = make_float4(D[0], D[1], D[2], D[3]);
      if (WRITE_RES) *reinterpret_cast<float4 *>(dres + o) = make_float4(R[0], R[1], R[2], R[3]);
    }
  }
  if (blockIdx.x == 0 && rsub == 0) {
    store_param_grads4(dweight, dbias, weight, cq * 4, e, ey, (float)rows, accumulate);
  }
}

// =============================================================================================
// Channels-last reductions, second design (round 2): ONE launch per reduction, finalize included.
//
// Round 1 gave every 32 KiB slab its own workgroup (2113 workgroups for an (8,512,65,65) tensor), each scattering
// 2*C floats as 8-byte stores with a stride of 8*P bytes, followed by a one-wave-per-channel finalize launch over the
// strided partials: the partial traffic rivalled the tensor itself and the finalize launch plus its two kernel
// boundaries cost ~14 us of every ~50 us call (0.24-0.43 of HBM peak).  Now:
//   * at most 256 workgroups of 1024 threads (16 waves, one workgroup per CU), each looping over row slabs with a
//     grid stride; a thread owns one channel quad and keeps its two sums in registers for the whole launch;
//   * wide tensors are cut into CB <= 4 channel blocks of >= 64 channels (256-byte row segments), so a workgroup's
//     partial is 2*CW floats and a channel block's partials total <= 128 KiB;
//   * partials are workgroup-major and contiguous: part[cb][rg][CW4][8] (per quad: four first sums, four second sums);
//   * the LAST workgroup of a channel block to arrive (write-through partial stores -> drained -> agent-scope ticket;
//     MI355X_MICROARCH.md "inter-workgroup visibility") sums the RG partial rows in double precision in a fixed
//     order -- bit-identical whichever workgroup happens to be last -- and finishes the statistics in place
//     (mean / var + running update, or edz / eydz).  No finalize launch, no atomically accumulated floats.
// Tickets live in a library-owned, zero-initialised counter pool (one slot per launch, round robin; the last arriver
// re-arms its counter), so the caller's workspace needs no initialisation.
// =============================================================================================

// K1 (NHWC): shifted sums of (x - K), (x - K)^2 with K = median3 of the channel; mean / biased var (+ running update) by the last arriver
template <int U>
__global__ __launch_bounds__(kRedThreads) void abn_stats_nhwc2_kernel(
    const float *__restrict__ x, float *__restrict__ part, unsigned *counters, float *__restrict__ mean,
    float *__restrict__ var, float *running_mean, float *running_var, int64_t rows, RedGeom g, float momentum,
    float n_total) {
  __shared__ double lds[kRedThreads * 4];
  __shared__ double fin[kRedThreads * 2];
  __shared__ unsigned ticket_s;
  const int t = threadIdx.x;
  const int cb = blockIdx.x % g.CB, rg = blockIdx.x / g.CB;
  const int cq = t & (g.CW4 - 1), rsub = t >> g.log2CW4;
  const int col = (cb * g.CW4 + cq) * 4;
  float4 K;   // per-channel pivot: median of the channel's first / middle / last row (median3, abn_dev.hpp)
  {
    const float4 ka = *reinterpret_cast<const float4 *>(x + col);
    const float4 kb = *reinterpret_cast<const float4 *>(x + ((rows / 2) << (g.log2C4 + 2)) + col);
    const float4 kc = *reinterpret_cast<const float4 *>(x + ((rows - 1) << (g.log2C4 + 2)) + col);
    K = make_float4(median3(ka.x, kb.x, kc.x), median3(ka.y, kb.y, kc.y), median3(ka.z, kb.z, kc.z), median3(ka.w, kb.w, kc.w));
  }
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  const int64_t slab = (int64_t)g.rpp * U;
  for (int64_t base = (int64_t)rg * slab + rsub; base < rows; base += (int64_t)g.RG * slab) {
    float4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t r = base + (int64_t)u * g.rpp;
      if (r < rows) v[u] = *reinterpret_cast<const float4 *>(x + (r << (g.log2C4 + 2)) + col);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t r = base + (int64_t)u * g.rpp;
      if (r < rows) {
        const float d0 = v[u].x - K.x, d1 = v[u].y - K.y, d2 = v[u].z - K.z, d3 = v[u].w - K.w;
        s1[0] += d0; s1[1] += d1; s1[2] += d2; s1[3] += d3;
        s2[0] += d0 * d0; s2[1] += d1 * d1; s2[2] += d2 * d2; s2[3] += d3 * d3;
      }
    }
  }
  if (!red_finish(s1, s2, part, counters + cb, g, cb, rg, lds, fin, &ticket_s)) return;
  const int CW = g.CW4 * 4;
  if (t < CW) {
    const int c = cb * CW + t;
    const double cnt = (double)rows;
    const double d = fin[(t >> 2) * 8 + (t & 3)] / cnt;
    double v = fin[(t >> 2) * 8 + 4 + (t & 3)] / cnt - d * d;
    if (v < 0.0) v = 0.0;
    const int64_t ldr = (int64_t)g.C4 * 4;
    const double Kc = (double)median3(x[c], x[(rows / 2) * ldr + c], x[(rows - 1) * ldr + c]);   // the same pivot as above
    const float m_f = (float)(Kc + d), v_f = (float)v;
    mean[c] = m_f;
    var[c] = v_f;
    if (running_mean != nullptr) running_mean[c] = running_mean[c] * (1.f - momentum) + momentum * m_f;
    if (running_var != nullptr) running_var[c] = running_var[c] * (1.f - momentum) + momentum * unbiased_of(v_f, n_total);
  }
}

// K3 (NHWC): edz / eydz.  MODE 0: y from the saved OUTPUT z (activation ACT undone in registers, the in-place ABN);
// MODE 1: fused BN+ReLU: inputs (x, out, dout), y from x, mask = out > 0.
// MODE 2: the same for a forward without residual: inputs (x, dout), mask = bn_pre(x) > 0 recomputed.
template <int ACT, int MODE, int U>
__global__ __launch_bounds__(kRedThreads) void abn_grad_nhwc2_kernel(
    const float *__restrict__ a_, const float *__restrict__ b_, const float *__restrict__ c_,
    const float *__restrict__ mean, const float *__restrict__ var, const float *__restrict__ weight,
    const float *__restrict__ bias, float *__restrict__ part, unsigned *counters, float *__restrict__ edz,
    float *__restrict__ eydz, float eps, float slope, int64_t rows, RedGeom g) {
  __shared__ double lds[kRedThreads * 4];
  __shared__ double fin[kRedThreads * 2];
  __shared__ unsigned ticket_s;
  const int t = threadIdx.x;
  const int cb = blockIdx.x % g.CB, rg = blockIdx.x / g.CB;
  const int cq = t & (g.CW4 - 1), rsub = t >> g.log2CW4;
  const int col = (cb * g.CW4 + cq) * 4;
  float p0[4], p1[4], gm[4], bt[4];  // MODE 0: beta, gamma   MODE 1 / 2: mean, inv_std (+ gamma, beta for the mask in MODE 2)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float mul;   // (the dx factor: not used by the reduction)
    load_grad_params<MODE, false>(mean, var, weight, bias, col + k, eps, p0[k], p1[k], gm[k], bt[k], mul);
  }
  const float inv_slope = 1.f / slope;
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  const int64_t slab = (int64_t)g.rpp * U;
  for (int64_t base = (int64_t)rg * slab + rsub; base < rows; base += (int64_t)g.RG * slab) {
    float4 va[U], vb[U], vc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t r = base + (int64_t)u * g.rpp;
      if (r < rows) {
        const int64_t o = (r << (g.log2C4 + 2)) + col;
        va[u] = *reinterpret_cast<const float4 *>(a_ + o);
        vb[u] = *reinterpret_cast<const float4 *>(b_ + o);
        if (MODE == 1) vc[u] = *reinterpret_cast<const float4 *>(c_ + o);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t r = base + (int64_t)u * g.rpp;
      if (r < rows) {
        const float A[4] = {va[u].x, va[u].y, va[u].z, va[u].w};
        const float B[4] = {vb[u].x, vb[u].y, vb[u].z, vb[u].w};
        const float Cc[4] = {MODE == 1 ? vc[u].x : 0.f, MODE == 1 ? vc[u].y : 0.f, MODE == 1 ? vc[u].z : 0.f,
                             MODE == 1 ? vc[u].w : 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float y, dz;
          grad_elem<ACT, MODE>(A[k], B[k], Cc[k], p0[k], p1[k], gm[k], bt[k], slope, inv_slope, y, dz);
          s1[k] += dz;
          s2[k] += y * dz;
        }
      }
    }
  }
  if (!red_finish(s1, s2, part, counters + cb, g, cb, rg, lds, fin, &ticket_s)) return;
  const int CW = g.CW4 * 4;
  if (t < CW) {
    const int c = cb * CW + t;
    const double cnt = (double)rows;
    edz[c] = (float)(fin[(t >> 2) * 8 + (t & 3)] / cnt);       // bn.cu:176
    eydz[c] = (float)(fin[(t >> 2) * 8 + 4 + (t & 3)] / cnt);  // bn.cu:177
  }
}

template <int ACT, bool HAS_RES>
static void launch_apply_nhwc_act(int64_t quads, int C4, float *x, const float *res, const float *mean,
                                  const float *var, const float *weight, const float *bias, float eps, float slope,
                                  hipStream_t st) {
  const dim3 block(kThreads);
  const bool pow2 = (C4 & (C4 - 1)) == 0;
  if (pow2 && C4 <= 4 * kThreads) {
    const dim3 grid((unsigned)cdiv(quads, (int64_t)kThreads * 8));
    if (C4 <= kThreads)
      abn_apply_nhwc_kernel<ACT, HAS_RES, 1><<<grid, block, 0, st>>>(x, res, mean, var, weight, bias, eps, slope, quads, C4);
    else if (C4 == 2 * kThreads)
      abn_apply_nhwc_kernel<ACT, HAS_RES, 2><<<grid, block, 0, st>>>(x, res, mean, var, weight, bias, eps, slope, quads, C4);
    else
      abn_apply_nhwc_kernel<ACT, HAS_RES, 4><<<grid, block, 0, st>>>(x, res, mean, var, weight, bias, eps, slope, quads, C4);
    return;
  }
  // threads = a multiple of lcm(C4, 256), about quads / 4 (four 16-byte accesses in flight per thread)
  int64_t unit = C4;
  while (unit % kThreads != 0) unit *= 2;
  int64_t threads = cdiv(cdiv(quads, 4), unit) * unit;
  const int64_t cap = cdiv((int64_t)256 * 8 * kThreads, unit) * unit;   // ~8 workgroups per CU, then stride
  if (threads > cap) threads = cap;
  if (threads < unit) threads = unit;
  abn_apply_nhwc_generic_kernel<ACT, HAS_RES><<<dim3((unsigned)(threads / kThreads)), block, 0, st>>>(
      x, res, mean, var, weight, bias, eps, slope, quads, C4);
}

// res may be NULL; 0 for an activation the inference pass is not built for (ELU)
static int launch_apply_nhwc(int64_t rows, int C, float *x, const float *res, const float *mean, const float *var,
                             const float *weight, const float *bias, float eps, int act, float slope, hipStream_t st) {
  const int C4 = C / 4;
  const int64_t quads = rows * C4;
  const bool known = dispatch_act<SKD_ACT_NONE, SKD_ACT_LEAKY_RELU, SKD_ACT_RELU>(act, [&](auto a) {
    constexpr int ACT = decltype(a)::value;
    if (res != nullptr)
      launch_apply_nhwc_act<ACT, true>(quads, C4, x, res, mean, var, weight, bias, eps, slope, st);
    else
      launch_apply_nhwc_act<ACT, false>(quads, C4, x, res, mean, var, weight, bias, eps, slope, st);
  });
  return known ? ok() : 0;
}

// ---------------------------------------------------------------------------------------------
// Finalize of the statistics a convolution's epilogue emitted (include/skd_bnstats.h; csrc/conv3x3.hip, block_stats): per
// channel, nb = ceil(rows / 32) records (mean, M2) of 32 rows each (the last: rows - 32 (nb - 1)) at part[(b * C + c) * 2].
// A workgroup of 1024 threads owns 8 channels: thread (run r = t / 8, channel t % 8) -- 8 lanes read 64 contiguous bytes of one
// block -- takes the blocks r, r + 128, r + 256, ... in ONE pass, in double, as sums shifted by the pivot K = the mean of the
// channel's block 0 (a block mean sits within the channel's spread of its mean, and the finished records are there to take it
// from -- which the epilogue that wrote them had not):  S1 = sum n_b (mean_b - K),  S2 = sum M2_b + n_b (mean_b - K)^2, the way
// abn_stats_nhwc2_kernel's finisher sums its partial rows.  The 128 runs of a channel are added in a fixed order: a butterfly over
// the 8 runs of a wave, then the 16 waves in turn.  mean = K + S1 / rows, M2 = S2 - S1^2 / rows.  Fixed assignment, fixed order,
// no atomics: the same bits on every call; a constant channel gives S1 = S2 = 0 and its value back exactly.  mean / biased var
// and the running update are abn_stats_nhwc2_kernel's, statement for statement.
// ---------------------------------------------------------------------------------------------
constexpr int kFinCh = 8, kFinRuns = 128, kFinThreads = kFinCh * kFinRuns;

__global__ __launch_bounds__(kFinThreads) void abn_stats_from_partials_kernel(
    const float *__restrict__ part, float *__restrict__ mean, float *__restrict__ var, float *running_mean, float *running_var,
    int64_t rows, int C, float momentum) {
  __shared__ double s_1[kFinThreads / kWave][kFinCh], s_2[kFinThreads / kWave][kFinCh];
  const int t = threadIdx.x, cl = t % kFinCh, r = t / kFinCh;
  const int c = blockIdx.x * kFinCh + cl;
  const int64_t nb = (rows + 31) / 32;
  const float2 *rec = reinterpret_cast<const float2 *>(part) + c;
  const double last = (double)(rows - 32 * (nb - 1));       // rows of the last block
  const double K = (double)rec[0].x;
  double a1 = 0.0, a2 = 0.0;
#pragma unroll 4
  for (int64_t b = r; b < nb; b += kFinRuns) {
    const float2 v = rec[b * C];
    const double nbk = b == nb - 1 ? last : 32.0;
    const double d = (double)v.x - K;
    a1 += nbk * d;
    a2 += (double)v.y + nbk * d * d;
  }
#pragma unroll
  for (int m = kFinCh; m < kWave; m *= 2) {                 // the 8 runs of this wave that share the channel
    a1 += __shfl_xor(a1, m, kWave);
    a2 += __shfl_xor(a2, m, kWave);
  }
  const int lane = t & (kWave - 1), wid = t / kWave;
  if (lane < kFinCh) {
    s_1[wid][lane] = a1;
    s_2[wid][lane] = a2;
  }
  __syncthreads();
  if (t < kFinCh) {
    double S1 = 0.0, S2 = 0.0;
#pragma unroll
    for (int w = 0; w < kFinThreads / kWave; ++w) {
      S1 += s_1[w][t];
      S2 += s_2[w][t];
    }
    const double cnt = (double)rows, d = S1 / cnt;
    double v = (S2 - S1 * d) / cnt;
    if (v < 0.0) v = 0.0;
    const float m_f = (float)(K + d), v_f = (float)v;
    mean[c] = m_f;
    var[c] = v_f;
    if (running_mean != nullptr) running_mean[c] = running_mean[c] * (1.f - momentum) + momentum * m_f;
    if (running_var != nullptr) running_var[c] = running_var[c] * (1.f - momentum) + momentum * unbiased_of(v_f, (float)rows);
  }
}

constexpr int kStatsU = 8, kGrad0U = 8, kGrad1U = 4;

#define SKD_RED_DISPATCH(U_, KERNEL_EXPR)                   \
  switch (U_) {                                             \
    case 8: { constexpr int UU = 8; KERNEL_EXPR; } break;   \
    case 4: { constexpr int UU = 4; KERNEL_EXPR; } break;   \
    default: { constexpr int UU = 2; KERNEL_EXPR; } break;  \
  }

}  // namespace
}  // namespace skd

namespace skd {

// ---- the ticket-counter pool: process-wide state, defined HERE only (abn_fused.hip and abn_stem.hip draw their counters through
// red_counters(), declared in abn_dev.hpp) -----------------------------------------------------------------------------------
struct RedPool {
  unsigned *ptr = nullptr;
};
static RedPool g_red_pool[64];
static unsigned g_red_next = 0;

// one ticket counter per channel block for this launch (zero on entry, zero again when the launch retires)
unsigned *red_counters() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  RedPool &p = g_red_pool[dev];
  if (p.ptr == nullptr) {
    unsigned *q = nullptr;
    const size_t bytes = sizeof(unsigned) * kRedSlots * kRedMaxCB * 2;   // ticket counters, then generation words
    if (hipMalloc(reinterpret_cast<void **>(&q), bytes) != hipSuccess) return nullptr;
    if (hipMemset(q, 0, bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
      (void)hipFree(q);
      return nullptr;
    }
    p.ptr = q;
  }
  const unsigned slot = __atomic_fetch_add(&g_red_next, 1u, __ATOMIC_RELAXED) % kRedSlots;
  return p.ptr + (size_t)slot * kRedMaxCB;
}

int launch_stats_nhwc2(int64_t rows, int C, const float *x, float *mean, float *var, float *running_mean, float *running_var,
                       float momentum, float *workspace, hipStream_t st) {
  RedGeom g;
  const int u = pick_u(rows, C, kStatsU, g);
  if (u == 0) return 0;
  unsigned *cnt = red_counters();
  if (cnt == nullptr) return 0;
  SKD_RED_DISPATCH(u, (abn_stats_nhwc2_kernel<UU><<<dim3((unsigned)(g.RG * g.CB)), dim3(kRedThreads), 0, st>>>(
      x, workspace, cnt, mean, var, running_mean, running_var, rows, g, momentum, (float)rows)));
  return ok();
}

int launch_apply_nhwc_train(int act, int64_t rows, int C, const float *x, const float *res, float *out, const float *mean,
                            const float *var, const float *weight, const float *bias, float eps, float slope, hipStream_t st) {
  NhwcGeom g;
  if (!make_nhwc_geom(rows, C, g)) return 0;
  const dim3 grid((unsigned)g.P), block(kThreads);
  const bool known = dispatch_act<SKD_ACT_NONE, SKD_ACT_LEAKY_RELU, SKD_ACT_ELU, SKD_ACT_RELU>(act, [&](auto a) {
    constexpr int ACT = decltype(a)::value;
    if (res != nullptr)
      abn_apply_nhwc_train_kernel<ACT, true><<<grid, block, 0, st>>>(x, res, out, mean, var, weight, bias, eps, slope, rows, g);
    else
      abn_apply_nhwc_train_kernel<ACT, false><<<grid, block, 0, st>>>(x, res, out, mean, var, weight, bias, eps, slope, rows, g);
  });
  return known ? ok() : 0;
}

}  // namespace skd

using namespace skd;

extern "C" {

int skd_abn_apply_nhwc(int64_t rows, int C, float *x, const float *residual, const float *mean, const float *var,
                       const float *weight, const float *bias, float eps, int activation, float slope,
                       skd_stream_t stream) {
  if (rows <= 0 || C <= 0 || (C & 3) || !x || !mean || !var) return 0;
  if ((reinterpret_cast<uintptr_t>(x) & 15) || (residual && (reinterpret_cast<uintptr_t>(residual) & 15))) return 0;
  return launch_apply_nhwc(rows, C, x, residual, mean, var, weight, bias, eps, activation, slope, as_stream(stream));
}

int64_t skd_abn_nhwc_workspace_floats(int64_t rows, int C) {
  NhwcGeom g;
  if (!make_nhwc_geom(rows, C, g)) return 0;
  // workgroup-major partial rows of the one-launch reductions: CB * RG <= kRedMaxWG rows of 2 * C / CB floats, then 2 * C floats
  // for this replica's own [mean | var] in the synchronised entries' three-launch form
  return (int64_t)kRedMaxWG * 2 * C + 2 * (int64_t)C;
}

int skd_abn_stats_nhwc(int64_t rows, int C, const float *x, float *mean, float *var, float *workspace,
                       skd_stream_t stream) {
  NhwcGeom g;
  if (!make_nhwc_geom(rows, C, g) || !x || !mean || !var || !workspace || !aligned16(x)) return 0;
  return launch_stats_nhwc2(rows, C, x, mean, var, nullptr, nullptr, 0.f, workspace, as_stream(stream));
}

// include/skd_bnstats.h: mean / biased var (+ running update) from the records a convolution's epilogue wrote
int skd_abn_stats_from_partials_nhwc(int64_t rows, int C, const float *stats, int64_t stats_floats, float *mean, float *var,
                                     float *running_mean, float *running_var, float momentum, skd_stream_t stream) {
  if (rows < 1 || rows > (int64_t)1 << 40 || C < 16 || C % 16 != 0 || !stats || !mean || !var) return 0;
  if ((reinterpret_cast<uintptr_t>(stats) & 7) || stats_floats < cdiv(rows, 32) * C * 2) return 0;
  abn_stats_from_partials_kernel<<<dim3((unsigned)(C / kFinCh)), dim3(kFinThreads), 0, as_stream(stream)>>>(
      stats, mean, var, running_mean, running_var, rows, C, momentum);
  return ok();
}

int skd_abn_apply_nhwc_to(int64_t rows, int C, const float *x, const float *residual, float *out,
                          const float *mean, const float *var, const float *weight, const float *bias, float eps,
                          int activation, float slope, skd_stream_t stream) {
  NhwcGeom g;
  if (!make_nhwc_geom(rows, C, g) || !x || !out || !mean || !var) return 0;
  if (!aligned16(x) || !aligned16(out) || (residual && !aligned16(residual))) return 0;
  return launch_apply_nhwc_train(activation, rows, C, x, residual, out, mean, var, weight, bias, eps, slope, as_stream(stream));
}

int skd_abn_backward_reduce_nhwc(int64_t rows, int C, const float *z, const float *dz, const float *weight,
                                 const float *bias, float *edz, float *eydz, float eps, int activation, float slope,
                                 float *workspace, skd_stream_t stream) {
  NhwcGeom g;
  if (!make_nhwc_geom(rows, C, g) || rows > 2147483647 || !z || !dz || !edz || !eydz || !workspace) return 0;
  if (!aligned16(z) || !aligned16(dz) || activation == SKD_ACT_RELU) return 0;
  hipStream_t st = as_stream(stream);
  RedGeom rg;
  const int u = pick_u(rows, C, kGrad0U, rg);
  if (u == 0) return 0;
  unsigned *cnt = red_counters();
  if (cnt == nullptr) return 0;
  const dim3 grid((unsigned)(rg.RG * rg.CB)), block(kRedThreads);
  dispatch_act_or_none<SKD_ACT_LEAKY_RELU, SKD_ACT_ELU>(activation, [&](auto a) {
    SKD_RED_DISPATCH(u, (abn_grad_nhwc2_kernel<decltype(a)::value, 0, UU><<<grid, block, 0, st>>>(z, dz, nullptr, nullptr, nullptr, weight, bias, workspace, cnt, edz, eydz, eps, slope, rows, rg)));
  });
  return ok();
}

int skd_abn_backward_dx_nhwc(int64_t rows, int C, const float *z, const float *dz, const float *var,
                             const float *weight, const float *bias, const float *edz, const float *eydz, float *dx,
                             float *dweight, float *dbias, float eps, int activation, float slope, int accumulate,
                             skd_stream_t stream) {
  NhwcGeom g;
  if (!make_nhwc_geom(rows, C, g) || !z || !dz || !var || !edz || !eydz || !dx) return 0;
  if (!aligned16(z) || !aligned16(dz) || !aligned16(dx) || activation == SKD_ACT_RELU || (dweight && !weight)) return 0;
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)g.P), block(kThreads);
  dispatch_act_or_none<SKD_ACT_LEAKY_RELU, SKD_ACT_ELU>(activation, [&](auto a) {
    abn_grad_dx_nhwc_kernel<decltype(a)::value, 0, false><<<grid, block, 0, st>>>(z, dz, nullptr, nullptr, var, weight, bias, edz, eydz, dx, nullptr, dweight, dbias, eps, slope, rows, g, accumulate);
  });
  return ok();
}

int skd_abn_relu_backward_reduce_nhwc(int64_t rows, int C, const float *x, const float *out, const float *dout,
                                      const float *mean, const float *var, float *edz, float *eydz, float eps,
                                      float *workspace, skd_stream_t stream) {
  NhwcGeom g;
  if (!make_nhwc_geom(rows, C, g) || rows > 2147483647 || !x || !out || !dout || !mean || !var || !edz || !eydz || !workspace) return 0;
  if (!aligned16(x) || !aligned16(out) || !aligned16(dout)) return 0;
  hipStream_t st = as_stream(stream);
  RedGeom rg;
  const int u = pick_u(rows, C, kGrad1U, rg);
  if (u == 0) return 0;
  unsigned *cnt = red_counters();
  if (cnt == nullptr) return 0;
  if (u == 4)
    abn_grad_nhwc2_kernel<SKD_ACT_NONE, 1, 4><<<dim3((unsigned)(rg.RG * rg.CB)), dim3(kRedThreads), 0, st>>>(
        x, out, dout, mean, var, nullptr, nullptr, workspace, cnt, edz, eydz, eps, 0.f, rows, rg);
  else
    abn_grad_nhwc2_kernel<SKD_ACT_NONE, 1, 2><<<dim3((unsigned)(rg.RG * rg.CB)), dim3(kRedThreads), 0, st>>>(
        x, out, dout, mean, var, nullptr, nullptr, workspace, cnt, edz, eydz, eps, 0.f, rows, rg);
  return ok();
}

int skd_abn_relu_backward_reduce_nhwc_x(int64_t rows, int C, const float *x, const float *dout, const float *mean,
                                        const float *var, const float *weight, const float *bias, float *edz, float *eydz,
                                        float eps, float *workspace, skd_stream_t stream) {
  NhwcGeom g;
  if (!make_nhwc_geom(rows, C, g) || rows > 2147483647 || !x || !dout || !mean || !var || !edz || !eydz || !workspace) return 0;
  if (!aligned16(x) || !aligned16(dout)) return 0;
  hipStream_t st = as_stream(stream);
  RedGeom rg;
  const int u = pick_u(rows, C, kGrad0U, rg);
  if (u == 0) return 0;
  unsigned *cnt = red_counters();
  if (cnt == nullptr) return 0;
  SKD_RED_DISPATCH(u, (abn_grad_nhwc2_kernel<SKD_ACT_NONE, 2, UU><<<dim3((unsigned)(rg.RG * rg.CB)), dim3(kRedThreads), 0, st>>>(
      x, dout, nullptr, mean, var, weight, bias, workspace, cnt, edz, eydz, eps, 0.f, rows, rg)));
  return ok();
}

int skd_abn_relu_backward_dx_nhwc_x(int64_t rows, int C, const float *x, const float *dout, const float *mean,
                                    const float *var, const float *weight, const float *bias, const float *edz,
                                    const float *eydz, float *dx, float *dweight, float *dbias, float eps, int accumulate,
                                    skd_stream_t stream) {
  NhwcGeom g;
  if (!make_nhwc_geom(rows, C, g) || !x || !dout || !mean || !var || !edz || !eydz || !dx) return 0;
  if (!aligned16(x) || !aligned16(dout) || !aligned16(dx) || (dweight && !weight)) return 0;
  abn_grad_dx_nhwc_kernel<SKD_ACT_NONE, 2, false><<<dim3((unsigned)g.P), dim3(kThreads), 0, as_stream(stream)>>>(
      x, dout, nullptr, mean, var, weight, bias, edz, eydz, dx, nullptr, dweight, dbias, eps, 0.f, rows, g, accumulate);
  return ok();
}

int skd_abn_relu_backward_dx_nhwc(int64_t rows, int C, const float *x, const float *out, const float *dout,
                                  const float *mean, const float *var, const float *weight, const float *edz,
                                  const float *eydz, float *dx, float *dres, float *dweight, float *dbias, float eps,
                                  int accumulate, skd_stream_t stream) {
  NhwcGeom g;
  if (!make_nhwc_geom(rows, C, g) || !x || !out || !dout || !mean || !var || !edz || !eydz || !dx) return 0;
  if (!aligned16(x) || !aligned16(out) || !aligned16(dout) || !aligned16(dx) || (dres && !aligned16(dres)) || (dweight && !weight)) return 0;
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)g.P), block(kThreads);
  if (dres != nullptr)
    abn_grad_dx_nhwc_kernel<SKD_ACT_NONE, 1, true><<<grid, block, 0, st>>>(x, out, dout, mean, var, weight, nullptr, edz, eydz, dx, dres, dweight, dbias, eps, 0.f, rows, g, accumulate);
  else
    abn_grad_dx_nhwc_kernel<SKD_ACT_NONE, 1, false><<<grid, block, 0, st>>>(x, out, dout, mean, var, weight, nullptr, edz, eydz, dx, dres, dweight, dbias, eps, 0.f, rows, g, accumulate);
  return ok();
}

}  // extern "C"
