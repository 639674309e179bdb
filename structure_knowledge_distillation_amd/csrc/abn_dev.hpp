// abn_dev.hpp -- what the InPlace-ABN translation units share: abn.hip (planar NCHW passes, legacy drop-ins), abn_nhwc.hip
// (channels-last two-launch passes and one-launch ticket reductions), abn_fused.hip (register-resident one-launch passes) and
// abn_stem.hip (BN + ReLU + max-pool stem).  Device helpers are __device__ __forceinline__ (the library is built -fno-gpu-rdc),
// every formula has ONE definition here, and process-wide host state is never defined in this header: it lives in one .hip
// file and is reached through the functions declared at the end.
#pragma once
#include <type_traits>

#include "skd_common.hpp"

namespace skd {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float gamma_of(const float *weight, int c, float eps) {
  return weight != nullptr ? fabsf(weight[c]) + eps : 1.f;  // bn.cu:153
}
__device__ __forceinline__ float beta_of(const float *bias, int c) {
  return bias != nullptr ? bias[c] : 0.f;  // bn.cu:154
}
__device__ __forceinline__ float inv_std_of(float var, float eps) {
  return (var != 0.f || eps != 0.f) ? 1.f / sqrtf(var + eps) : 0.f;  // bn.cu:148-151
}

// functions.py:91,209: running_var takes var * n / (n - 1).  With ONE sample per channel (the PSP 1x1 stage at
// batch 1 on a single replica) the reference divides by zero and poisons the buffer with
// NaN / inf; here n == 1 keeps the (zero) biased variance instead -- the one deliberate deviation, see DESIGN.md.
__device__ __forceinline__ float unbiased_of(float var, float n) { return n > 1.f ? var * n / (n - 1.f) : var; }

// Pivot of the one-pass (shifted) statistics: the MEDIAN of three samples of the channel -- first, middle and last element
// of the tensor's channel.  The shifted variance loses ~k^2 * 2^-24 of relative accuracy when the pivot sits k sigma from
// the mean (bn.cu:125-138 is two-pass and has no such term); a single sample as pivot makes that k the tail of the data
// (one outlier element 100 sigma off: 6e-4), the median of three needs TWO outliers among the three probes.  NaN-free
// ordering: fminf / fmaxf return the non-NaN operand, and a NaN anywhere in the channel poisons the sums regardless.
__device__ __forceinline__ float median3(float a, float b, float c) {
  return fmaxf(fminf(a, b), fminf(fmaxf(a, b), c));
}

template <int ACT>
__device__ __forceinline__ float act_fwd(float z, float slope) {
  if (ACT == SKD_ACT_LEAKY_RELU) return z < 0.f ? z * slope : z;        // bn.cu:302-315
  if (ACT == SKD_ACT_ELU) return z < 0.f ? expf(z) - 1.f : z;           // bn.cu:333-346
  if (ACT == SKD_ACT_RELU) return z < 0.f ? 0.f : z;                    // nn.ReLU after BatchNorm2d, pspnet_combine.py:36,68,72
  return z;
}
// undo the activation on (z, dz) in registers: functions.py:54-62 / bn.cu:317-331,348-377
template <int ACT>
__device__ __forceinline__ void act_undo(float &z, float &dz, float slope, float inv_slope) {
  if (ACT == SKD_ACT_LEAKY_RELU) {
    if (z < 0.f) {
      dz *= slope;
      z *= inv_slope;
    }
  } else if (ACT == SKD_ACT_ELU) {
    if (z < 0.f) {
      dz *= (z + 1.f);
      z = log1pf(z);
    }
  }
}

// Host side of every `switch (activation)` around a kernel launch: f(std::integral_constant<int, ACT>) is called for the ONE
// code of Allowed... that equals `act`; false (nothing called) for a code outside the set.  The set a call site names is the
// set of kernel instantiations it creates.
template <int... Allowed, class F>
static inline bool dispatch_act(int act, F &&f) {
  return ((act == Allowed ? (f(std::integral_constant<int, Allowed>{}), true) : false) || ...);
}
// the same for the entries whose `default:` arm is SKD_ACT_NONE (any code outside Allowed... runs without an activation)
template <int... Allowed, class F>
static inline void dispatch_act_or_none(int act, F &&f) {
  if (!dispatch_act<Allowed...>(act, f)) f(std::integral_constant<int, SKD_ACT_NONE>{});
}

static inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- channels-last (NHWC) pieces: x is (rows = N*H*W, C) row-major -----------------------------------------------------------
// geometry of the apply-type passes (abn_nhwc.hip: every 32 KiB slab its own 256-thread workgroup)
constexpr int kNhwcRowsPerThread = 8;

struct NhwcGeom {
  int C4, log2C4, rpp;  // channel quads, log2, rows per pass (256 / C4)
  int rows_per_wg;      // rpp * kNhwcRowsPerThread
  int P;                // workgroups = partial slots per channel
};

static bool make_nhwc_geom(int64_t rows, int C, NhwcGeom &g) {
  if (rows <= 0 || C < 4 || C > 4 * kThreads || (C & (C - 1))) return false;
  g.C4 = C / 4;
  g.log2C4 = 0;
  while ((1 << g.log2C4) < g.C4) ++g.log2C4;
  g.rpp = kThreads / g.C4;
  g.rows_per_wg = g.rpp * kNhwcRowsPerThread;
  const int64_t P = cdiv(rows, g.rows_per_wg);
  if (P > (1 << 24)) return false;
  g.P = (int)P;
  return true;
}

// The pre-activation of the fused BN (+ residual) + ReLU, as ONE expression shared by the forward pass and by the backward
// passes that recompute the ReLU mask from x instead of reading `out` (MODE 2): same instructions, same bits, same sign.
__device__ __forceinline__ float bn_pre(float x, float m, float is, float gm, float b) {
  return __builtin_fmaf((x - m) * is, gm, b);
}

// channel c's mean, inverse standard deviation, gamma and beta: the per-quad parameter prologue of the forward-type passes
__device__ __forceinline__ void load_bn_params(const float *mean, const float *var, const float *weight, const float *bias, int c,
                                               float eps, float &m, float &is, float &gm, float &b) {
  m = mean[c];
  is = inv_std_of(var[c], eps);
  gm = gamma_of(weight, c, eps);
  b = beta_of(bias, c);
}

// The per-element backward of the channels-last passes, ONE definition for the two-launch reduce and dx kernels, the one-launch
// kernel and the stem: from a pass's inputs (A, B, C) to y (the normalised input) and dz (the gradient at the BN output).
//   MODE 0: (z, dz) of the in-place ABN -- y from the saved OUTPUT z, activation ACT undone in registers; p0, p1 = beta, gamma
//   MODE 1: fused BN+ReLU, inputs (x, out, dout) -- y from x, mask = out > 0;                              p0, p1 = mean, inv_std
//   MODE 2: the same for a forward without residual, inputs (x, dout) -- mask = bn_pre(x) > 0 recomputed;  + gm, bt = gamma, beta
template <int ACT, int MODE>
__device__ __forceinline__ void grad_elem(float A, float B, float C, float p0, float p1, float gm, float bt, float slope,
                                          float inv_slope, float &y, float &dz) {
  if (MODE == 0) {
    float zv = A;
    dz = B;
    act_undo<ACT>(zv, dz, slope, inv_slope);
    y = (zv - p0) / p1;
  } else if (MODE == 1) {
    dz = B > 0.f ? C : 0.f;          // (x, out, dout)
    y = (A - p0) * p1;
  } else {
    dz = bn_pre(A, p0, p1, gm, bt) > 0.f ? B : 0.f;   // (x, dout)
    y = (A - p0) * p1;
  }
}
// grad_elem's parameters of channel c; gm = gamma in every MODE.  DX (the dx-type passes): also mul = gamma * inv_std, the factor
// of the dx formula, which needs var in every MODE -- without it MODE 0 reads neither mean nor var (the reduce entries pass NULL).
template <int MODE, bool DX>
__device__ __forceinline__ void load_grad_params(const float *mean, const float *var, const float *weight, const float *bias, int c,
                                                 float eps, float &p0, float &p1, float &gm, float &bt, float &mul) {
  const float gam = gamma_of(weight, c, eps), is = (DX || MODE != 0) ? inv_std_of(var[c], eps) : 0.f;
  if (MODE == 0) {
    p0 = beta_of(bias, c);
    p1 = gam;
  } else {
    p0 = mean[c];
    p1 = is;
  }
  gm = gam;
  bt = MODE == 2 ? beta_of(bias, c) : 0.f;
  mul = gam * is;
}
// dweight / dbias of channel c from its edz / eydz (norm = elements per channel): sign(w) * eydz * norm and edz * norm
__device__ __forceinline__ void store_param_grads(float *dweight, float *dbias, const float *weight, int c, float e, float ey,
                                                  float norm, int accumulate) {
  if (dweight != nullptr) {   // bn.cu:217-229 accumulates; accumulate == 0 writes (no zero-fill needed before the call)
    const float wv = weight[c];
    const float gwt = wv > 0.f ? ey * norm : (wv < 0.f ? -ey * norm : 0.f);
    dweight[c] = accumulate ? dweight[c] + gwt : gwt;
  }
  if (dbias != nullptr) dbias[c] = accumulate ? dbias[c] + e * norm : e * norm;
}

// the same for the channel quad c0 .. c0 + 3 of a thread
__device__ __forceinline__ void store_param_grads4(float *dweight, float *dbias, const float *weight, int c0, const float (&e)[4],
                                                   const float (&ey)[4], float norm, int accumulate) {
#pragma unroll
  for (int k = 0; k < 4; ++k) store_param_grads(dweight, dbias, weight, c0 + k, e[k], ey[k], norm, accumulate);
}

// ---- the one-launch reductions (design notes: abn_nhwc.hip, "second design") -------------------------------------------------
constexpr int kRedThreads = 1024;
constexpr int kRedMaxWG = 256;
constexpr int kRedMaxCB = 4;
constexpr int kRedSlots = 4096;

struct RedGeom {
  int C4, log2C4;     // channel quads per row
  int CB;             // channel blocks
  int CW4, log2CW4;   // quads per channel block
  int rpp;            // rows per pass of one workgroup (1024 / CW4)
  int RG;             // row groups = workgroups per channel block = partial rows per channel block
  int L;              // floats per partial row (CW4 * 8)
};

static bool make_red_geom(int64_t rows, int C, int U, RedGeom &g) {
  if (rows <= 0 || rows > 2147483647 || C < 4 || C > 4 * kThreads || (C & (C - 1))) return false;
  g.C4 = C / 4;
  g.log2C4 = 0;
  while ((1 << g.log2C4) < g.C4) ++g.log2C4;
  g.CB = C >= 256 ? 4 : (C >= 128 ? 2 : 1);
  g.CW4 = g.C4 / g.CB;
  g.log2CW4 = 0;
  while ((1 << g.log2CW4) < g.CW4) ++g.log2CW4;
  g.rpp = kRedThreads / g.CW4;
  const int64_t want = cdiv(rows, (int64_t)g.rpp * U);
  const int64_t cap = kRedMaxWG / g.CB;
  g.RG = (int)(want < cap ? want : cap);
  g.L = g.CW4 * 8;
  return true;
}

// The library-owned ticket-counter pool (defined ONCE, in abn_nhwc.hip): one ticket counter per channel block for this launch
// (zero on entry, zero again when the launch retires); nullptr when the pool could not be allocated.
unsigned *red_counters();
// the generation words (fused one-launch passes) that belong to a counter slot
static inline unsigned *red_gens(unsigned *counters) { return counters + (size_t)kRedSlots * kRedMaxCB; }

// 16-byte write-through store / L1-bypassing load (sc0 sc1): the hand-off traffic of the reductions (abn_nhwc.hip, abn_fused.hip, abn_stem.hip).  A plain
// store would stay dirty in the producer XCD's L2 until an agent-scope release (buffer_wbl2) flushes that WHOLE L2 --
// right after a convolution that is megabytes of unrelated dirty lines on the reduction's critical path.  With
// write-through partials the producer only drains its own stores (s_waitcnt vmcnt(0)) before taking its ticket, and
// the last arriver reads them with sc1 loads: no release / acquire fence at all (MI355X_MICROARCH.md, "valid forms":
// sc0 sc1 stores and loads on both sides).
__device__ __forceinline__ void store_wt16(float *p, f32x4 v) {
  asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" : : "v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void load_wt16x4(const float *p0, const float *p1, const float *p2, const float *p3, f32x4 &v0,
                                            f32x4 &v1, f32x4 &v2, f32x4 &v3) {
  asm volatile(
      "global_load_dwordx4 %0, %4, off sc0 sc1\n\t"
      "global_load_dwordx4 %1, %5, off sc0 sc1\n\t"
      "global_load_dwordx4 %2, %6, off sc0 sc1\n\t"
      "global_load_dwordx4 %3, %7, off sc0 sc1\n\t"
      "s_waitcnt vmcnt(0)"
      : "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(v3)
      : "v"(p0), "v"(p1), "v"(p2), "v"(p3)
      : "memory");
}

// Workgroup epilogue of a channels-last reduction.  In: every thread's eight running sums.  Out: `true` in all
// threads of the channel block's last-arriving workgroup, with the block's totals in fin[cq * 8 + k] (double).
// lds: kRedThreads * 4 doubles; fin: L doubles.
__device__ __forceinline__ bool red_finish(float (&s1)[4], float (&s2)[4], float *__restrict__ part,
                                           unsigned *counter, const RedGeom &g, int cb, int rg, double *lds,
                                           double *fin, unsigned *ticket_s) {
  const int t = threadIdx.x, lane = t & (kWave - 1);
  float a[8] = {s1[0], s1[1], s1[2], s1[3], s2[0], s2[1], s2[2], s2[3]};
  // lanes of a wave that share a channel quad differ only in the row bits of the lane index: butterfly over those
  for (int m = kWave / 2; m >= g.CW4; m >>= 1) {
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] += __shfl_xor(a[k], m, kWave);
  }
  float *ldsf = reinterpret_cast<float *>(lds);
  const int cq = t & (g.CW4 - 1);
  int slot, nslots;
  bool writer;
  if (g.CW4 < kWave) {
    slot = t / kWave;
    nslots = kRedThreads / kWave;
    writer = lane < g.CW4;
  } else {
    slot = t >> g.log2CW4;
    nslots = kRedThreads >> g.log2CW4;
    writer = true;
  }
  if (writer) {
    float *o = ldsf + ((int64_t)slot * g.CW4 + cq) * 8;
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = a[k];
  }
  __syncthreads();
  const int L4 = g.L >> 2;                 // float4 per partial row (a power of two, 2 ... 128)
  float *mine = part + ((int64_t)cb * g.RG + rg) * g.L;
  if (t < L4) {                            // fixed-order sum over the slots, one 16-byte write-through store per lane
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int sl = 0; sl < nslots; ++sl) {
      const float4 v = *reinterpret_cast<const float4 *>(ldsf + sl * g.L + 4 * t);
      s[0] += v.x;
      s[1] += v.y;
      s[2] += v.z;
      s[3] += v.w;
    }
    store_wt16(mine + 4 * t, s);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this lane's partial has left for memory
  }
  __syncthreads();
  if (t == 0) *ticket_s = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  if (*ticket_s != (unsigned)g.RG - 1u) return false;
  if (t == 0) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-arm for a later launch
  // ---- last arriver: fixed-order double-precision sum of the RG partial rows of this channel block ----
  const int NP = kRedThreads / L4;         // row phases
  const int j4 = t & (L4 - 1), ph = t / L4;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  const float *col = part + (int64_t)cb * g.RG * g.L + j4 * 4;
  for (int r = ph; r < g.RG; r += 4 * NP) {
    f32x4 v[4];
    const float *q[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int rr = r + u * NP;
      q[u] = col + (int64_t)(rr < g.RG ? rr : r) * g.L;     // out-of-range phases re-read row r and are not added
    }
    load_wt16x4(q[0], q[1], q[2], q[3], v[0], v[1], v[2], v[3]);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (r + u * NP < g.RG) {
        acc[0] += (double)v[u][0];
        acc[1] += (double)v[u][1];
        acc[2] += (double)v[u][2];
        acc[3] += (double)v[u][3];
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) lds[((int64_t)ph * L4 + j4) * 4 + q] = acc[q];
  __syncthreads();
  for (int i = t; i < g.L; i += kRedThreads) {
    double s = 0.0;
    for (int p = 0; p < NP; ++p) s += lds[(int64_t)p * g.L + i];
    fin[i] = s;
  }
  __syncthreads();
  return true;
}

// Rows in flight per thread and trip (U): the tuned maximum for large tensors; halved while the launch would leave
// workgroup slots unused -- (8, 128, 65, 65) at U = 8 gives 134 workgroups for 256 CUs, at U = 4 it gives 256.
static int pick_u(int64_t rows, int C, int umax, RedGeom &g) {
  int u = umax;
  if (!make_red_geom(rows, C, u, g)) return 0;
  while (u > 2 && (int64_t)g.RG * g.CB < kRedMaxWG) {
    RedGeom h;
    if (!make_red_geom(rows, C, u / 2, h) || h.RG == g.RG) break;
    u /= 2;
    g = h;
  }
  return u;
}

// ---- host functions shared between the translation units (abn_nhwc.hip) -------------------------------------------------------
// one-launch statistics of a channels-last tensor (mean / biased var, running update when the pointers are given); 0 = failed
int launch_stats_nhwc2(int64_t rows, int C, const float *x, float *mean, float *var, float *running_mean, float *running_var,
                       float momentum, float *workspace, hipStream_t st);
// out = act(bn(x) [+ res]) with given statistics, res may be NULL; 0 for a shape or an activation the pass does not take
int launch_apply_nhwc_train(int act, int64_t rows, int C, const float *x, const float *res, float *out, const float *mean,
                            const float *var, const float *weight, const float *bias, float eps, float slope, hipStream_t st);
}  // namespace skd
