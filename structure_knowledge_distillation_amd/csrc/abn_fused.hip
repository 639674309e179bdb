// abn_fused.hip -- the register-resident ONE-launch InPlace-ABN passes for channels-last tensors (forward and backward, with the
// grid barrier per channel block and, in the synchronised entries, the cross-replica exchange inside the launch), their
// process-wide switches (SKD_ABN_FUSED / SKD_ABN_SYNC_FUSED), the workgroup cap and occupancy checks, and the one-call
// entries that choose between this form and the two-launch passes of abn_nhwc.hip.  Shared helpers: abn_dev.hpp.
#include <stdlib.h>

#include <atomic>

#include "abn_dev.hpp"
#include "sync_dev.hpp"

namespace skd {
namespace {

// =============================================================================================
// Channels-last TRAINING passes as ONE launch with the tensor held in registers (round 3).
//
// The two-launch form (abn_nhwc.hip) reads x for the statistics, ends the launch, and reads x again for the normalisation:
// 12 bytes per element, and for the student's 4-70 MB tensors a second launch whose whole life is 8-20 us.  The chip's
// register file is larger than those tensors (256 CUs x 512 KiB = 128 MiB): a launch of <= 256 workgroups x 1024
// threads in which a thread keeps its NR <= 17 float4 of x in VGPRs can hold up to ~71 MB.  So:
//   phase 1  every thread loads its rows ONCE, accumulates the shifted sums, red_finish() as before;
//   hand-off the channel block's last arriver finishes mean / var (+ running statistics), stores them write-through
//            and bumps the block's generation word; the other workgroups of the block spin (bounded) on that word --
//            a grid barrier per channel block, safe because the launch never exceeds one workgroup per CU
//            (MI355X_MICROARCH.md: "size the grid ... bound every spin");
//   phase 2  normalise + affine + activation (+ residual) from the registers, one store.
// HBM traffic: 8 bytes per element instead of 12 (forward), 12 instead of 20 (backward: z and dz are held, y and the
// masked dz are kept instead of the raw inputs).  Tensors that do not fit (the 256 x 256 stem layers, C = 512 in the
// backward) keep the two-launch path.  A spin that times out (2 s of wall clock: the grid was not co-resident) poisons
// the statistics with NaN instead of hanging the device: loud, not fatal.
// The generation word is read by every workgroup BEFORE it takes its ticket and bumped by the last arriver AFTER all
// tickets: no host-side sequence number, so a captured launch can be replayed.
// =============================================================================================
constexpr uint64_t kFuseSpinTicks = 200000000ull;   // wall_clock64(): 100 MHz

__device__ __forceinline__ unsigned gen_load(const unsigned *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// thread 0 spins until the generation word moves on from gen0; false = timed out (status word kStatusFusedTimeout raised)
__device__ __forceinline__ bool gen_wait(const unsigned *p, unsigned gen0, uint64_t ticks, unsigned *status) {
  const uint64_t t0 = wall_clock64();
  while (gen_load(p) == gen0) {
    __builtin_amdgcn_s_sleep(4);
    if (wall_clock64() - t0 > ticks) {
      raise_status(status, kStatusFusedTimeout, 1u);
      return false;
    }
  }
  return true;
}
__device__ __forceinline__ void store_wt4(float *p, float v) {
  asm volatile("global_store_dword %0, %1, off sc0 sc1" : : "v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ f32x4 load_wt16(const float *p) {
  f32x4 v;
  asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
  return v;
}

struct FuseGeom {
  RedGeom r;
  int nr;        // rows per thread actually used (<= NR of the instantiation)
};

// NRmax rows per thread: geometry with the most workgroups (<= 256 / CB per channel block) and the fewest rows each
static bool make_fuse_geom(int64_t rows, int C, int nr_max, int max_wg, FuseGeom &f) {
  if (max_wg < kRedMaxCB || !make_red_geom(rows, C, 1, f.r)) return false;
  RedGeom &g = f.r;
  const int64_t cap = max_wg / g.CB;
  const int64_t want = cdiv(rows, g.rpp);
  g.RG = (int)(want < cap ? want : cap);
  const int64_t nr = cdiv(rows, (int64_t)g.RG * g.rpp);
  if (nr > nr_max) return false;
  f.nr = (int)nr;
  g.RG = (int)cdiv(rows, (int64_t)g.rpp * f.nr);     // drop workgroups that would own no row
  return true;
}

// SYNC: the cross-replica exchange of InPlaceABNSync (libs/functions.py:185-209) happens INSIDE the launch: the channel
// block's last arriver stores the block's local [mean | var] into every replica's mailbox, raises / awaits the block's flag
// word (sync_dev.hpp) and applies the combine rule before it releases the block's workgroups -- the register-resident
// one-launch form survives N > 1 (round 3 fell back to stats + exchange + apply: three launches, 12 B/element).
template <int ACT, bool HAS_RES, int NR, bool SYNC>
__global__ __launch_bounds__(kRedThreads) void abn_fwd_fused_nhwc_kernel(
    const float *x, const float *res, float *out, float *__restrict__ part, unsigned *counters, unsigned *gens,
    float *mean, float *var, float *running_mean, float *running_var, const float *__restrict__ weight,
    const float *__restrict__ bias, int64_t rows, RedGeom g, int nr, float momentum, float eps, float slope,
    SyncArgs sy, const float *__restrict__ rweights, float n_pooled) {
  __shared__ double lds[kRedThreads * 4];
  __shared__ double fin[kRedThreads * 2];
  __shared__ unsigned ticket_s;
  __shared__ unsigned gen_s;
  const int t = threadIdx.x;
  const int cb = blockIdx.x % g.CB, rg = blockIdx.x / g.CB;
  const int cq = t & (g.CW4 - 1), rsub = t >> g.log2CW4;
  const int col = (cb * g.CW4 + cq) * 4;
  if (t == 0) gen_s = gen_load(gens + cb);              // before this workgroup's ticket, hence before the bump
  const int r0 = rg * g.rpp * nr + rsub;      // 32-bit row / element indices: a fused launch holds < 2^27 elements
  const int nrows = (int)rows;
  float4 v[NR];
#pragma unroll
  for (int u = 0; u < NR; ++u) {
    const int r = r0 + u * g.rpp;
    if (u < nr && r < nrows) v[u] = *reinterpret_cast<const float4 *>(x + ((r << (g.log2C4 + 2)) + col));
  }
  float4 K;
  {
    const float4 ka = *reinterpret_cast<const float4 *>(x + col);
    const float4 kb = *reinterpret_cast<const float4 *>(x + ((rows / 2) << (g.log2C4 + 2)) + col);
    const float4 kc = *reinterpret_cast<const float4 *>(x + ((rows - 1) << (g.log2C4 + 2)) + col);
    K = make_float4(median3(ka.x, kb.x, kc.x), median3(ka.y, kb.y, kc.y), median3(ka.z, kb.z, kc.z), median3(ka.w, kb.w, kc.w));
  }
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < NR; ++u) {
    const int r = r0 + u * g.rpp;
    if (u < nr && r < nrows) {
      const float d0 = v[u].x - K.x, d1 = v[u].y - K.y, d2 = v[u].z - K.z, d3 = v[u].w - K.w;
      s1[0] += d0; s1[1] += d1; s1[2] += d2; s1[3] += d3;
      s2[0] += d0 * d0; s2[1] += d1 * d1; s2[2] += d2 * d2; s2[3] += d3 * d3;
    }
  }
  const int CW = g.CW4 * 4;
  bool good = true;
  float loc_m = 0.f, loc_v = 0.f;            // SYNC: this replica's statistics of channel cb * CW + t
  if (red_finish(s1, s2, part, counters + cb, g, cb, rg, lds, fin, &ticket_s)) {
    if (t < CW) {
      const int c = cb * CW + t;
      const double cnt = (double)rows;
      const double d = fin[(t >> 2) * 8 + (t & 3)] / cnt;
      double vv = fin[(t >> 2) * 8 + 4 + (t & 3)] / cnt - d * d;
      if (vv < 0.0) vv = 0.0;
      const int64_t ldr = (int64_t)g.C4 * 4;
      const double Kc = (double)median3(x[c], x[(rows / 2) * ldr + c], x[(rows - 1) * ldr + c]);
      const float m_f = (float)(Kc + d), v_f = (float)vv;
      if (SYNC) {
        loc_m = m_f;
        loc_v = v_f;
      } else {
        store_wt4(mean + c, m_f);
        store_wt4(var + c, v_f);
        if (running_mean != nullptr) running_mean[c] = running_mean[c] * (1.f - momentum) + momentum * m_f;
        if (running_var != nullptr) running_var[c] = running_var[c] * (1.f - momentum) + momentum * unbiased_of(v_f, (float)rows);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    }
    if (SYNC) {
      const int Ct = g.C4 * 4, c = cb * CW + t;
      const bool arrived = sync_exchange(sy, cb, 1, [&](float *dst) {
        if (t < CW) {
          store_sys(dst + c, loc_m);
          store_sys(dst + Ct + c, loc_v);
        }
      }, &ticket_s);
      if (t < CW) {
        float m, v;
        combine_channel(sy.d.world, Ct, c, [&](int gq, int j) { return sync_payload(sy.d, sy.seq, gq, j); }, rweights, sy.d.rank,
                        n_pooled, momentum, m, v, arrived ? running_mean : nullptr, arrived ? running_var : nullptr);
        store_wt4(mean + c, arrived ? m : __builtin_nanf(""));
        store_wt4(var + c, arrived ? v : __builtin_nanf(""));
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    }
    __syncthreads();
    if (t == 0) __hip_atomic_store(gens + cb, gen_s + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
    // (SYNC: the block's last arriver may itself be waiting for a peer replica: its limit on top of the grid barrier's own)
    if (t == 0) ticket_s = gen_wait(gens + cb, gen_s, kFuseSpinTicks + (SYNC ? sy.spin_ticks : 0ull), sy.status) ? 1u : 0u;
    __syncthreads();
    good = ticket_s != 0u;
  }
  const f32x4 m4 = load_wt16(mean + col), v4 = load_wt16(var + col);
  float m[4], is[4], gm[4], b[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    m[k] = good ? m4[k] : __builtin_nanf("");
    is[k] = inv_std_of(v4[k], eps);
    gm[k] = gamma_of(weight, col + k, eps);
    b[k] = beta_of(bias, col + k);
  }
#pragma unroll
  for (int u = 0; u < NR; ++u) {
    const int r = r0 + u * g.rpp;
    if (u < nr && r < nrows) {
      const int o = (r << (g.log2C4 + 2)) + col;
      float4 r4 = make_float4(0.f, 0.f, 0.f, 0.f);
      if (HAS_RES) r4 = *reinterpret_cast<const float4 *>(res + o);
      float4 z;
      z.x = act_fwd<ACT>(HAS_RES ? bn_pre(v[u].x, m[0], is[0], gm[0], b[0]) + r4.x : bn_pre(v[u].x, m[0], is[0], gm[0], b[0]), slope);
      z.y = act_fwd<ACT>(HAS_RES ? bn_pre(v[u].y, m[1], is[1], gm[1], b[1]) + r4.y : bn_pre(v[u].y, m[1], is[1], gm[1], b[1]), slope);
      z.z = act_fwd<ACT>(HAS_RES ? bn_pre(v[u].z, m[2], is[2], gm[2], b[2]) + r4.z : bn_pre(v[u].z, m[2], is[2], gm[2], b[2]), slope);
      z.w = act_fwd<ACT>(HAS_RES ? bn_pre(v[u].w, m[3], is[3], gm[3], b[3]) + r4.w : bn_pre(v[u].w, m[3], is[3], gm[3], b[3]), slope);
      *reinterpret_cast<float4 *>(out + o) = z;
    }
  }
}

// Backward, both passes in one launch.  MODE as in abn_grad_nhwc2_kernel / abn_grad_dx_nhwc_kernel; a thread keeps (y, dz) of
// its NR rows -- the masked / activation-undone gradient and the normalised input -- between the phases.
// SYNC: [edz | eydz] of the channel block are exchanged by the block's last arriver inside the launch (functions.py:263-280).
template <int ACT, int MODE, bool WRITE_RES, int NR, bool SYNC>
__global__ __launch_bounds__(kRedThreads) void abn_bwd_fused_nhwc_kernel(
    const float *a_, const float *b_, const float *c_, const float *__restrict__ mean, const float *__restrict__ var,
    const float *__restrict__ weight, const float *__restrict__ bias, float *__restrict__ part, unsigned *counters,
    unsigned *gens, float *edz, float *eydz, float *dx, float *dres, float *dweight, float *dbias, float eps, float slope,
    int64_t rows, RedGeom g, int nr, int accumulate, SyncArgs sy, const float *__restrict__ rweights) {
  __shared__ double lds[kRedThreads * 4];
  __shared__ double fin[kRedThreads * 2];
  __shared__ unsigned ticket_s;
  __shared__ unsigned gen_s;
  const int t = threadIdx.x;
  const int cb = blockIdx.x % g.CB, rg = blockIdx.x / g.CB;
  const int cq = t & (g.CW4 - 1), rsub = t >> g.log2CW4;
  const int col = (cb * g.CW4 + cq) * 4;
  if (t == 0) gen_s = gen_load(gens + cb);
  float p0[4], p1[4], gm[4], bt[4], mul[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    load_grad_params<MODE, true>(mean, var, weight, bias, col + k, eps, p0[k], p1[k], gm[k], bt[k], mul[k]);
  }
  const float inv_slope = 1.f / slope;
  const int r0 = rg * g.rpp * nr + rsub;      // 32-bit row / element indices: a fused launch holds < 2^27 elements
  const int nrows = (int)rows;
  float4 Y[NR], DZ[NR];
  constexpr int CH = 2;                    // rows loaded per trip: bounds the registers holding raw inputs
#pragma unroll
  for (int u0 = 0; u0 < NR; u0 += CH) {
    float4 va[CH], vb[CH], vc[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const int u = u0 + j;
      const int r = r0 + u * g.rpp;
      if (u < NR && u < nr && r < nrows) {
        const int o = (r << (g.log2C4 + 2)) + col;
        va[j] = *reinterpret_cast<const float4 *>(a_ + o);
        vb[j] = *reinterpret_cast<const float4 *>(b_ + o);
        if (MODE == 1) vc[j] = *reinterpret_cast<const float4 *>(c_ + o);
      }
    }
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const int u = u0 + j;
      const int r = r0 + u * g.rpp;
      if (u < NR && u < nr && r < nrows) {
        const float A[4] = {va[j].x, va[j].y, va[j].z, va[j].w};
        const float B[4] = {vb[j].x, vb[j].y, vb[j].z, vb[j].w};
        const float Cc[4] = {MODE == 1 ? vc[j].x : 0.f, MODE == 1 ? vc[j].y : 0.f, MODE == 1 ? vc[j].z : 0.f,
                             MODE == 1 ? vc[j].w : 0.f};
        float y[4], dz[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) grad_elem<ACT, MODE>(A[k], B[k], Cc[k], p0[k], p1[k], gm[k], bt[k], slope, inv_slope, y[k], dz[k]);
        Y[u] = make_float4(y[0], y[1], y[2], y[3]);
        DZ[u] = make_float4(dz[0], dz[1], dz[2], dz[3]);
      }
    }
  }
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < NR; ++u) {
    const int r = r0 + u * g.rpp;
    if (u < nr && r < nrows) {
      s1[0] += DZ[u].x; s1[1] += DZ[u].y; s1[2] += DZ[u].z; s1[3] += DZ[u].w;
      s2[0] += Y[u].x * DZ[u].x; s2[1] += Y[u].y * DZ[u].y; s2[2] += Y[u].z * DZ[u].z; s2[3] += Y[u].w * DZ[u].w;
    }
  }
  const int CW = g.CW4 * 4;
  bool good = true;
  if (red_finish(s1, s2, part, counters + cb, g, cb, rg, lds, fin, &ticket_s)) {
    float loc_e = 0.f, loc_ey = 0.f;
    if (t < CW) {
      const double cnt = (double)rows;
      loc_e = (float)(fin[(t >> 2) * 8 + (t & 3)] / cnt);          // bn.cu:176
      loc_ey = (float)(fin[(t >> 2) * 8 + 4 + (t & 3)] / cnt);     // bn.cu:177
    }
    bool arrived = true;
    if (SYNC) {
      const int Ct = g.C4 * 4, c = cb * CW + t;
      arrived = sync_exchange(sy, cb, 1, [&](float *dst) {
        if (t < CW) {
          store_sys(dst + c, loc_e);
          store_sys(dst + Ct + c, loc_ey);
        }
      }, &ticket_s);
      if (t < CW) {
        loc_e = arrived ? sync_weighted_sum(sy.d, sy.seq, c, rweights) : __builtin_nanf("");
        loc_ey = arrived ? sync_weighted_sum(sy.d, sy.seq, Ct + c, rweights) : __builtin_nanf("");
      }
    }
    if (t < CW) {
      const int c = cb * CW + t;
      const float e_f = loc_e, ey_f = loc_ey;
      store_wt4(edz + c, e_f);
      store_wt4(eydz + c, ey_f);
      store_param_grads(dweight, dbias, weight, c, e_f, ey_f, (float)rows, accumulate);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    if (t == 0) __hip_atomic_store(gens + cb, gen_s + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
    if (t == 0) ticket_s = gen_wait(gens + cb, gen_s, kFuseSpinTicks + (SYNC ? sy.spin_ticks : 0ull), sy.status) ? 1u : 0u;
    __syncthreads();
    good = ticket_s != 0u;
  }
  const f32x4 e4 = load_wt16(edz + col), ey4 = load_wt16(eydz + col);
  float e[4], ey[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    e[k] = good ? e4[k] : __builtin_nanf("");
    ey[k] = ey4[k];
  }
#pragma unroll
  for (int u = 0; u < NR; ++u) {
    const int r = r0 + u * g.rpp;
    if (u < nr && r < nrows) {
      const int o = (r << (g.log2C4 + 2)) + col;
      float4 D;
      D.x = (DZ[u].x - e[0] - Y[u].x * ey[0]) * mul[0];
      D.y = (DZ[u].y - e[1] - Y[u].y * ey[1]) * mul[1];
      D.z = (DZ[u].z - e[2] - Y[u].z * ey[2]) * mul[2];
      D.w = (DZ[u].w - e[3] - Y[u].w * ey[3]) * mul[3];
      *reinterpret_cast<float4 *>(dx + o) = D;
      if (WRITE_RES) *reinterpret_cast<float4 *>(dres + o) = DZ[u];
    }
  }
}

// SKD_ABN_FUSED=0 keeps the two-launch passes -- the operational switch for a device that is shared with another grid-barrier
// launch (multi-tenant GPU); default: the register-resident one-launch passes when they fit.
// SKD_ABN_SYNC_FUSED=0: the synchronised entries keep the three-launch form (statistics, exchange kernel, normalise).
// Both are LIBRARY STATE (round 6): the environment is read ONCE, at the first query (getenv from autograd threads
// while the host language calls setenv is not safe under glibc, and a process-wide variable is the wrong place for a default that
// depends on the process group); skd_abn_set_fused / skd_abn_set_sync_fused change it afterwards (tests, utils/parallel.py's RCCL
// default, bench.py's fallback chain), -1 = read the environment again at the next query.
constexpr int kFuseFwdMaxNR = 17, kFuseBwdMaxNR = 9;
static std::atomic<int> g_fused_state{-1}, g_sync_fused_state{-1};
static bool switch_state(std::atomic<int> &state, const char *name) {
  int v = state.load(std::memory_order_relaxed);
  if (v < 0) {
    const char *e = getenv(name);
    v = !(e != nullptr && e[0] == '0');
    state.store(v, std::memory_order_relaxed);
  }
  return v != 0;
}
static bool fused_enabled() { return switch_state(g_fused_state, "SKD_ABN_FUSED"); }
static bool sync_fused_enabled() { return switch_state(g_sync_fused_state, "SKD_ABN_SYNC_FUSED"); }

// The grid barrier of the one-launch passes needs every workgroup of the launch co-resident: the grid is
// capped by what THIS device can hold at one 1024-thread workgroup per compute unit -- 256 on a whole MI355X, 32 on a
// CPX partition -- queried once per device, never assumed (a CU MASK is not visible in that attribute: see below).  skd_abn_set_fused_max_workgroups()
// lowers it further (ranks that share one device must share its compute units: utils/parallel.py does that).  A cap too
// small for a tensor (rows per thread > NR) simply sends that call to the two-launch path.
struct FuseCap {
  int cap[64];
  bool known[64];
};
static FuseCap g_fuse_cap = {};
static int g_fuse_user_cap = kRedMaxWG;

static int fuse_wg_cap() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
  if (!g_fuse_cap.known[dev]) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) {
      (void)hipGetLastError();
      cus = 0;
    }
    const char *e = getenv("SKD_ABN_FUSED_MAXWG");
    int env_cap = kRedMaxWG;
    if (e != nullptr && e[0] != 0) env_cap = atoi(e);
    int cap = cus < kRedMaxWG ? cus : kRedMaxWG;
    if (env_cap < cap) cap = env_cap;
    // A CU mask is NOT reflected in hipDeviceAttributeMultiprocessorCount: a masked process that trusted the
    // attribute would launch a grid barrier that cannot be co-resident and sit in it until the time limit.  Parsing the mask
    // formats is not this library's business: with a mask in the environment the one-launch passes are OFF (two-launch path)
    // unless the user states the usable compute units with SKD_ABN_FUSED_MAXWG.
    const char *m1 = getenv("HSA_CU_MASK"), *m2 = getenv("ROC_GLOBAL_CU_MASK");
    if (((m1 != nullptr && m1[0] != 0) || (m2 != nullptr && m2[0] != 0)) && !(e != nullptr && e[0] != 0)) cap = 0;
    g_fuse_cap.cap[dev] = cap > 0 ? cap : 0;
    g_fuse_cap.known[dev] = true;
  }
  const int cap = g_fuse_cap.cap[dev];
  return cap < g_fuse_user_cap ? cap : g_fuse_user_cap;
}

// one workgroup per compute unit must actually be launchable for THIS instantiation (registers, LDS): checked once per
// instantiation and device with the occupancy query, not assumed
template <class K>
static bool fuse_kernel_fits(K kernel, PerDeviceFlag &checked, PerDeviceFlag &fits) {
  bool *c = checked.get(), *f = fits.get();
  if (c == nullptr || f == nullptr) return false;
  if (!*c) {
    int blocks = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, reinterpret_cast<const void *>(kernel), kRedThreads, 0) != hipSuccess) {
      (void)hipGetLastError();
      blocks = 0;
    }
    *f = blocks >= 1;
    *c = true;
  }
  return *f;
}
#define SKD_FUSE_LAUNCH(KERNEL, ...)                                                        \
  do {                                                                                      \
    static PerDeviceFlag checked_, fits_;                                                   \
    if (!fuse_kernel_fits(KERNEL, checked_, fits_)) return -1;                              \
    KERNEL<<<grid, block, 0, st>>>(__VA_ARGS__);                                            \
  } while (0)

// ---- can THIS device launch every synchronised one-launch instantiation?   -------------------------------------
// SKD_FUSE_LAUNCH checks its instantiation when it is about to launch -- for the synchronised entries that is AFTER sync_next()
// has drawn the exchange's sequence number, when "take the other form" is no longer possible: the rank would have to fail while
// its peers spin for it.  So the synchronised entries ask this BEFORE they draw: one occupancy query per instantiation, once per
// device; if any of them cannot hold a 1024-thread workgroup on a compute unit (fewer registers / LDS than gfx950), the device
// takes the three-launch form for every synchronised call (the two forms interoperate rank by rank).
template <class K>
static bool one_block_fits(K kernel) {
  int blocks = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, reinterpret_cast<const void *>(kernel), kRedThreads, 0) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return blocks >= 1;
}
template <int ACT, bool RES>
static bool fwd_sync_fit() {
  return one_block_fits(abn_fwd_fused_nhwc_kernel<ACT, RES, 5, true>) && one_block_fits(abn_fwd_fused_nhwc_kernel<ACT, RES, 9, true>) &&
         one_block_fits(abn_fwd_fused_nhwc_kernel<ACT, RES, 17, true>);
}
template <int ACT, int MODE, bool WRITE_RES>
static bool bwd_sync_fit() {
  return one_block_fits(abn_bwd_fused_nhwc_kernel<ACT, MODE, WRITE_RES, 5, true>) &&
         one_block_fits(abn_bwd_fused_nhwc_kernel<ACT, MODE, WRITE_RES, 9, true>);
}
static bool sync_fused_fits_device() {
  static PerDeviceFlag checked, fits;
  bool *c = checked.get(), *f = fits.get();
  if (c == nullptr || f == nullptr) return false;
  if (!*c) {
    *f = fwd_sync_fit<SKD_ACT_RELU, true>() && fwd_sync_fit<SKD_ACT_RELU, false>() && fwd_sync_fit<SKD_ACT_LEAKY_RELU, false>() &&
         fwd_sync_fit<SKD_ACT_NONE, false>() && bwd_sync_fit<SKD_ACT_LEAKY_RELU, 0, false>() && bwd_sync_fit<SKD_ACT_NONE, 0, false>() &&
         bwd_sync_fit<SKD_ACT_NONE, 2, false>() && bwd_sync_fit<SKD_ACT_NONE, 1, true>() && bwd_sync_fit<SKD_ACT_NONE, 1, false>();
    *c = true;
  }
  return *f;
}

// how often the synchronised entries took each form (tests and bench.py report it: "did the exchange really run inside the kernel?")
static int64_t g_sync_form_calls[2] = {0, 0};     // [one launch with the exchange inside, statistics + exchange kernel + normalise]

static SyncArgs no_sync() {
  SyncArgs a = {};
  a.status = status_words();
  return a;
}

// returns -1 when the call does not take the fused path (not enabled, activation / size not covered), else ok().
// sy != nullptr: the cross-replica exchange happens inside the launch (the caller has drawn sy with sync_next()).
template <bool HAS_RES, bool SYNC>
static int launch_fwd_fused(int act, int64_t rows, int C, const float *x, const float *res, float *out, float *mean,
                            float *var, float *running_mean, float *running_var, const float *weight, const float *bias,
                            float momentum, float eps, float slope, float *workspace, hipStream_t st, const FuseGeom &f,
                            const SyncArgs &sy, const float *rweights, float n_pooled) {
  unsigned *cnt = red_counters();
  if (cnt == nullptr) return 0;
  const dim3 grid((unsigned)(f.r.RG * f.r.CB)), block(kRedThreads);
#define SKD_FWD_FUSED(ACT_, NR_)                                                                                              \
  SKD_FUSE_LAUNCH((abn_fwd_fused_nhwc_kernel<ACT_, HAS_RES, NR_, SYNC>), x, res, out, workspace, cnt, red_gens(cnt), mean, var, \
                  running_mean, running_var, weight, bias, rows, f.r, f.nr, momentum, eps, slope, sy, rweights, n_pooled)
#define SKD_FWD_FUSED_NR(ACT_)                 \
  if (f.nr <= 5) SKD_FWD_FUSED(ACT_, 5);       \
  else if (f.nr <= 9) SKD_FWD_FUSED(ACT_, 9);  \
  else SKD_FWD_FUSED(ACT_, 17)
  // (`if constexpr`: a residual comes with ReLU only, and a run-time `!HAS_RES &&` still instantiated the six <NONE / LEAKY, true>
  // kernels, twelve with the synchronised ones, that no entry can launch)
  if (act == SKD_ACT_RELU) {
    SKD_FWD_FUSED_NR(SKD_ACT_RELU);
  } else if constexpr (!HAS_RES) {
    if (act == SKD_ACT_LEAKY_RELU) {
      SKD_FWD_FUSED_NR(SKD_ACT_LEAKY_RELU);
    } else if (act == SKD_ACT_NONE) {
      SKD_FWD_FUSED_NR(SKD_ACT_NONE);
    } else {
      return -1;
    }
  } else {
    return -1;
  }
#undef SKD_FWD_FUSED_NR
#undef SKD_FWD_FUSED
  return ok();
}

// does this forward take the one-launch form?  (decided BEFORE a sequence number is drawn for the exchange)
static bool fwd_fused_geom(int act, bool has_res, int64_t rows, int C, FuseGeom &f) {
  if (!fused_enabled() || act == SKD_ACT_ELU || (has_res && act != SKD_ACT_RELU)) return false;
  if (act != SKD_ACT_RELU && act != SKD_ACT_LEAKY_RELU && act != SKD_ACT_NONE) return false;
  return make_fuse_geom(rows, C, kFuseFwdMaxNR, fuse_wg_cap(), f);
}
static bool bwd_fused_geom(int64_t rows, int C, FuseGeom &f) {
  return fused_enabled() && make_fuse_geom(rows, C, kFuseBwdMaxNR, fuse_wg_cap(), f);
}

// MODE 0: (z, dz) of the in-place ABN; MODE 1: (x, out, dout); MODE 2: (x, dout).  -1 = not taken.
template <int ACT, int MODE, bool WRITE_RES, bool SYNC>
static int launch_bwd_fused(int64_t rows, int C, const float *a, const float *b, const float *c, const float *mean,
                            const float *var, const float *weight, const float *bias, float *edz, float *eydz, float *dx,
                            float *dres, float *dweight, float *dbias, float eps, float slope, int accumulate,
                            float *workspace, hipStream_t st, const FuseGeom &f, const SyncArgs &sy, const float *rweights) {
  unsigned *cnt = red_counters();
  if (cnt == nullptr) return 0;
  const dim3 grid((unsigned)(f.r.RG * f.r.CB)), block(kRedThreads);
  // instantiations sized to the step's layers (5 rows per thread at C = 128, 9 at C = 64 / 256): one row more and the 18 registers
  // per row (y, dz) of the NR = 10 form spilled 11-13 of them (PMC: 14.3 instead of 12 bytes per element)
  if (f.nr <= 5)
    SKD_FUSE_LAUNCH((abn_bwd_fused_nhwc_kernel<ACT, MODE, WRITE_RES, 5, SYNC>), a, b, c, mean, var, weight, bias, workspace, cnt,
                    red_gens(cnt), edz, eydz, dx, dres, dweight, dbias, eps, slope, rows, f.r, f.nr, accumulate, sy, rweights);
  else
    SKD_FUSE_LAUNCH((abn_bwd_fused_nhwc_kernel<ACT, MODE, WRITE_RES, 9, SYNC>), a, b, c, mean, var, weight, bias, workspace, cnt,
                    red_gens(cnt), edz, eydz, dx, dres, dweight, dbias, eps, slope, rows, f.r, f.nr, accumulate, sy, rweights);
  return ok();
}

// The one-launch backward of a one-call entry, plain (sync_ctx == NULL) or with the cross-replica exchange inside the launch:
// launch(std::bool_constant<SYNC>, sy, rweights) is the entry's launch_bwd_fused<..., SYNC> call.  Plain: its result, -1 = not
// taken (the caller runs the two-launch passes).  Synchronised: 1 / 0 -- the sequence number is drawn first, and once it is
// drawn "not taken" is no longer an option (the peers wait for this rank's payload), so anything but success is a failure.
template <class Launch>
static int bwd_fused_any(void *sync_ctx, const float *rweights, Launch launch) {
  if (sync_ctx == nullptr) return launch(std::false_type{}, no_sync(), nullptr);
  SyncArgs sy;
  if (!sync_next(sync_ctx, sy)) return 0;
  ++g_sync_form_calls[0];
  return launch(std::true_type{}, sy, rweights) > 0 ? 1 : 0;
}

}  // namespace
}  // namespace skd

using namespace skd;

extern "C" {

int skd_abn_forward_train_nhwc(int64_t rows, int C, const float *x, const float *residual, float *out,
                               const float *weight, const float *bias, float *running_mean, float *running_var,
                               float *mean, float *var, float momentum, float eps, int activation, float slope,
                               float *workspace, skd_stream_t stream) {
  NhwcGeom g;
  if (!make_nhwc_geom(rows, C, g) || rows > 2147483647 || !x || !out || !mean || !var || !workspace) return 0;
  if (!aligned16(x) || !aligned16(out) || (residual && !aligned16(residual))) return 0;
  hipStream_t st = as_stream(stream);
  FuseGeom f;
  if (aligned16(mean) && aligned16(var) && fwd_fused_geom(activation, residual != nullptr, rows, C, f)) {
    const SyncArgs sy = no_sync();
    const int r = residual ? launch_fwd_fused<true, false>(activation, rows, C, x, residual, out, mean, var, running_mean, running_var,
                                                           weight, bias, momentum, eps, slope, workspace, st, f, sy, nullptr, 0.f)
                           : launch_fwd_fused<false, false>(activation, rows, C, x, residual, out, mean, var, running_mean, running_var,
                                                            weight, bias, momentum, eps, slope, workspace, st, f, sy, nullptr, 0.f);
    if (r >= 0) return r;
  }
  if (!launch_stats_nhwc2(rows, C, x, mean, var, running_mean, running_var, momentum, workspace, st)) return 0;
  return launch_apply_nhwc_train(activation, rows, C, x, residual, out, mean, var, weight, bias, eps, slope, st);
}

// InPlaceABNSync forward (libs/functions.py:165-218) for a channels-last tensor in ONE call: the arguments of
// skd_abn_forward_train_nhwc plus the mailbox context (skd_sync_create), the per-replica sample weights (NULL = equal
// shards) and n (the pooled sample count without weights, this replica's with: skd_abn_combine_stats).  One
// register-resident launch with the exchange inside it when the tensor fits; else statistics -> skd_abn_sync_stats ->
// normalise.  Either way ONE exchange (one sequence number) in the same place of every rank's call order.
int skd_abn_forward_train_nhwc_sync(void *sync_ctx, int64_t rows, int C, const float *x, const float *residual, float *out,
                                    const float *weight, const float *bias, float *running_mean, float *running_var,
                                    float *mean, float *var, const float *replica_weights, float momentum, float eps,
                                    int activation, float slope, double n, float *workspace, skd_stream_t stream) {
  NhwcGeom g;
  if (!sync_ctx || !make_nhwc_geom(rows, C, g) || rows > 2147483647 || !x || !out || !mean || !var || !workspace) return 0;
  if (!aligned16(x) || !aligned16(out) || (residual && !aligned16(residual)) || 2 * C > kSyncMaxFloats) return 0;
  hipStream_t st = as_stream(stream);
  FuseGeom f;
  if (sync_fused_enabled() && sync_fused_fits_device() && aligned16(mean) && aligned16(var) &&
      fwd_fused_geom(activation, residual != nullptr, rows, C, f)) {
    SyncArgs sy;
    if (!sync_next(sync_ctx, sy)) return 0;
    ++g_sync_form_calls[0];
    const int r = residual ? launch_fwd_fused<true, true>(activation, rows, C, x, residual, out, mean, var, running_mean, running_var,
                                                          weight, bias, momentum, eps, slope, workspace, st, f, sy, replica_weights, (float)n)
                           : launch_fwd_fused<false, true>(activation, rows, C, x, residual, out, mean, var, running_mean, running_var,
                                                           weight, bias, momentum, eps, slope, workspace, st, f, sy, replica_weights, (float)n);
    return r > 0 ? 1 : 0;          // (a sequence number has been drawn: "not taken" is no longer an option)
  }
  ++g_sync_form_calls[1];
  float *local = workspace + (int64_t)kRedMaxWG * 2 * C;       // this replica's [mean | var]
  if (!launch_stats_nhwc2(rows, C, x, local, local + C, nullptr, nullptr, 0.f, workspace, st)) return 0;
  if (!skd_abn_sync_stats(sync_ctx, C, local, replica_weights, mean, var, running_mean, running_var, momentum, n, stream)) return 0;
  return launch_apply_nhwc_train(activation, rows, C, x, residual, out, mean, var, weight, bias, eps, slope, st);
}

// One-call channels-last backward (reduce + dx): ONE register-resident launch when the tensor fits (see "one launch with the
// tensor held in registers" above), the two launches of abn_nhwc.hip's entries otherwise.  edz / eydz are outputs as well.
// sync_ctx != NULL (the *_sync entries below): InPlaceABNSync's backward (libs/functions.py:257-294) -- [edz | eydz] are
// exchanged and averaged over the replicas between the reduction and the dx pass: inside the one launch, or by
// skd_abn_sync_grad_stats between the two (edz, eydz must then be the two halves of ONE (2, C) buffer).
static int abn_backward_nhwc_any(void *sync_ctx, const float *rweights, int64_t rows, int C, const float *z, const float *dz,
                                 const float *var, const float *weight, const float *bias, float *edz, float *eydz, float *dx,
                                 float *dweight, float *dbias, float eps, int activation, float slope, int accumulate,
                                 float *workspace, skd_stream_t stream) {
  NhwcGeom g;
  if (!make_nhwc_geom(rows, C, g) || rows > 2147483647 || !z || !dz || !var || !edz || !eydz || !dx || !workspace) return 0;
  if (!aligned16(z) || !aligned16(dz) || !aligned16(dx) || activation == SKD_ACT_RELU || (dweight && !weight)) return 0;
  if (sync_ctx && (eydz != edz + C || 2 * C > kSyncMaxFloats)) return 0;
  hipStream_t st = as_stream(stream);
  FuseGeom f;
  if (aligned16(edz) && aligned16(eydz) && activation != SKD_ACT_ELU && (!sync_ctx || (sync_fused_enabled() && sync_fused_fits_device())) &&
      bwd_fused_geom(rows, C, f)) {
    const int r = bwd_fused_any(sync_ctx, rweights, [&](auto sync, const SyncArgs &sy, const float *rw) {
      constexpr bool SYNC = decltype(sync)::value;
      return activation == SKD_ACT_LEAKY_RELU
                 ? launch_bwd_fused<SKD_ACT_LEAKY_RELU, 0, false, SYNC>(rows, C, z, dz, nullptr, nullptr, var, weight, bias, edz, eydz, dx, nullptr,
                                                                        dweight, dbias, eps, slope, accumulate, workspace, st, f, sy, rw)
                 : launch_bwd_fused<SKD_ACT_NONE, 0, false, SYNC>(rows, C, z, dz, nullptr, nullptr, var, weight, bias, edz, eydz, dx, nullptr,
                                                                  dweight, dbias, eps, slope, accumulate, workspace, st, f, sy, rw);
    });
    if (sync_ctx || r >= 0) return r;
  }
  if (!skd_abn_backward_reduce_nhwc(rows, C, z, dz, weight, bias, edz, eydz, eps, activation, slope, workspace, stream)) return 0;
  if (sync_ctx) ++g_sync_form_calls[1];
  if (sync_ctx && !skd_abn_sync_grad_stats(sync_ctx, C, edz, rweights, stream)) return 0;
  return skd_abn_backward_dx_nhwc(rows, C, z, dz, var, weight, bias, edz, eydz, dx, dweight, dbias, eps, activation, slope,
                                  accumulate, stream);
}

int skd_abn_backward_nhwc(int64_t rows, int C, const float *z, const float *dz, const float *var, const float *weight,
                          const float *bias, float *edz, float *eydz, float *dx, float *dweight, float *dbias, float eps,
                          int activation, float slope, int accumulate, float *workspace, skd_stream_t stream) {
  return abn_backward_nhwc_any(nullptr, nullptr, rows, C, z, dz, var, weight, bias, edz, eydz, dx, dweight, dbias, eps, activation,
                               slope, accumulate, workspace, stream);
}

int skd_abn_backward_nhwc_sync(void *sync_ctx, int64_t rows, int C, const float *z, const float *dz, const float *var,
                               const float *weight, const float *bias, float *edz, float *eydz, float *dx, float *dweight,
                               float *dbias, const float *replica_weights, float eps, int activation, float slope, int accumulate,
                               float *workspace, skd_stream_t stream) {
  if (!sync_ctx) return 0;
  return abn_backward_nhwc_any(sync_ctx, replica_weights, rows, C, z, dz, var, weight, bias, edz, eydz, dx, dweight, dbias, eps,
                               activation, slope, accumulate, workspace, stream);
}

// The same for the fused BN + ReLU (+ residual) op: out == NULL -> the mask is recomputed from x (forward without residual).
static int abn_relu_backward_nhwc_any(void *sync_ctx, const float *rweights, int64_t rows, int C, const float *x, const float *out,
                                      const float *dout, const float *mean, const float *var, const float *weight, const float *bias,
                                      float *edz, float *eydz, float *dx, float *dres, float *dweight, float *dbias, float eps,
                                      int accumulate, float *workspace, skd_stream_t stream) {
  NhwcGeom g;
  if (!make_nhwc_geom(rows, C, g) || rows > 2147483647 || !x || !dout || !mean || !var || !edz || !eydz || !dx || !workspace) return 0;
  if (!aligned16(x) || !aligned16(dout) || !aligned16(dx) || (out && !aligned16(out)) || (dres && !aligned16(dres)) || (dweight && !weight)) return 0;
  if (out == nullptr && dres != nullptr) return 0;
  if (sync_ctx && (eydz != edz + C || 2 * C > kSyncMaxFloats)) return 0;
  hipStream_t st = as_stream(stream);
  FuseGeom f;
  if (aligned16(edz) && aligned16(eydz) && (!sync_ctx || (sync_fused_enabled() && sync_fused_fits_device())) && bwd_fused_geom(rows, C, f)) {
    const int r = bwd_fused_any(sync_ctx, rweights, [&](auto sync, const SyncArgs &sy, const float *rw) {
      constexpr bool SYNC = decltype(sync)::value;
      if (out == nullptr)
        return launch_bwd_fused<SKD_ACT_NONE, 2, false, SYNC>(rows, C, x, dout, nullptr, mean, var, weight, bias, edz, eydz, dx, nullptr, dweight,
                                                              dbias, eps, 0.f, accumulate, workspace, st, f, sy, rw);
      if (dres != nullptr)
        return launch_bwd_fused<SKD_ACT_NONE, 1, true, SYNC>(rows, C, x, out, dout, mean, var, weight, bias, edz, eydz, dx, dres, dweight, dbias,
                                                             eps, 0.f, accumulate, workspace, st, f, sy, rw);
      return launch_bwd_fused<SKD_ACT_NONE, 1, false, SYNC>(rows, C, x, out, dout, mean, var, weight, bias, edz, eydz, dx, nullptr, dweight,
                                                            dbias, eps, 0.f, accumulate, workspace, st, f, sy, rw);
    });
    if (sync_ctx || r >= 0) return r;
  }
  if (sync_ctx) ++g_sync_form_calls[1];
  if (out == nullptr) {
    if (!skd_abn_relu_backward_reduce_nhwc_x(rows, C, x, dout, mean, var, weight, bias, edz, eydz, eps, workspace, stream)) return 0;
    if (sync_ctx && !skd_abn_sync_grad_stats(sync_ctx, C, edz, rweights, stream)) return 0;
    return skd_abn_relu_backward_dx_nhwc_x(rows, C, x, dout, mean, var, weight, bias, edz, eydz, dx, dweight, dbias, eps, accumulate,
                                           stream);
  }
  if (!skd_abn_relu_backward_reduce_nhwc(rows, C, x, out, dout, mean, var, edz, eydz, eps, workspace, stream)) return 0;
  if (sync_ctx && !skd_abn_sync_grad_stats(sync_ctx, C, edz, rweights, stream)) return 0;
  return skd_abn_relu_backward_dx_nhwc(rows, C, x, out, dout, mean, var, weight, edz, eydz, dx, dres, dweight, dbias, eps, accumulate,
                                       stream);
}

int skd_abn_relu_backward_nhwc(int64_t rows, int C, const float *x, const float *out, const float *dout, const float *mean,
                               const float *var, const float *weight, const float *bias, float *edz, float *eydz, float *dx,
                               float *dres, float *dweight, float *dbias, float eps, int accumulate, float *workspace,
                               skd_stream_t stream) {
  return abn_relu_backward_nhwc_any(nullptr, nullptr, rows, C, x, out, dout, mean, var, weight, bias, edz, eydz, dx, dres, dweight, dbias,
                                    eps, accumulate, workspace, stream);
}

int skd_abn_relu_backward_nhwc_sync(void *sync_ctx, int64_t rows, int C, const float *x, const float *out, const float *dout,
                                    const float *mean, const float *var, const float *weight, const float *bias, float *edz,
                                    float *eydz, float *dx, float *dres, float *dweight, float *dbias, const float *replica_weights,
                                    float eps, int accumulate, float *workspace, skd_stream_t stream) {
  if (!sync_ctx) return 0;
  return abn_relu_backward_nhwc_any(sync_ctx, replica_weights, rows, C, x, out, dout, mean, var, weight, bias, edz, eydz, dx, dres, dweight,
                                    dbias, eps, accumulate, workspace, stream);
}

// out[0] = synchronised calls that ran as ONE launch with the exchange inside, out[1] = as statistics + exchange kernel +
// normalise (three launches), since the library was loaded.  Host counters, process-wide.
int skd_abn_sync_form_counts(int64_t *out) {
  if (!out) return 0;
  out[0] = g_sync_form_calls[0];
  out[1] = g_sync_form_calls[1];
  return 1;
}

// Upper bound of the workgroups of a one-launch (grid-barrier) pass, on top of the device's own limit (compute units):
// ranks that share ONE device must share its compute units or their barrier kernels cannot all be resident.  n > 0 sets the
// bound, n == 0 restores the default, n < 0 only queries.  Process-wide; returns the effective cap on the current device.
// 1 / 0: the one-launch passes on / off; -1: back to the environment (SKD_ABN_FUSED / SKD_ABN_SYNC_FUSED, default on), read at
// the next query.  The getters return the EFFECTIVE state (and resolve an unset one).
int skd_abn_set_fused(int on) {
  g_fused_state.store(on < 0 ? -1 : (on != 0), std::memory_order_relaxed);
  return 1;
}
int skd_abn_get_fused(void) { return fused_enabled() ? 1 : 0; }
int skd_abn_set_sync_fused(int on) {
  g_sync_fused_state.store(on < 0 ? -1 : (on != 0), std::memory_order_relaxed);
  return 1;
}
int skd_abn_get_sync_fused(void) { return sync_fused_enabled() ? 1 : 0; }

int skd_abn_set_fused_max_workgroups(int n) {
  if (n >= 0) g_fuse_user_cap = (n > 0 && n < kRedMaxWG) ? n : kRedMaxWG;
  return fuse_wg_cap();
}

}  // extern "C"
