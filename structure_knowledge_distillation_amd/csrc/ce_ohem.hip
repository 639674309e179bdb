// ce_ohem.hip -- OhemCrossEntropy2d / CriterionOhemDSN fused, for gfx950: online hard-example mining on top of the fused
// upsample + cross-entropy pass of ce_dev.hpp, with the threshold found on the device.
//
// Reference: utils/criterion.py:11-90 (OhemCrossEntropy2d) and :190-209 (CriterionOhemDSN).  Per step it materialises the
// up-sampled (B, C, H, W) logits and their softmax, copies the softmax to the host, runs scipy.ndimage.zoom on it (order 1) and
// on the target (order 0) to 1 / factor resolution, np.partition for the min_kept-th smallest label probability, builds a new
// target on the host, copies it back and only then runs the cross-entropy -- all of it synchronous.
//
// Here:
//   ohem_keys_kernel    FOUR lanes per DOWN-SAMPLED pixel, one per full-resolution pixel around its float64 zoom coordinate: each
//                       lane up-samples the C logits of its pixel (tap_of_strict / ce_lerp: the OHEM main pass's arithmetic), evaluates their softmax
//                       with ce_pixel_softmax and the label's probability with ce_p_label -- the functions the main pass uses, so
//                       a pixel has the same probability in both --; lane 0 of the quad forms scipy's float64 four-term sum and
//                       writes the fp32 key (-1 where the down-sampled label is ignored).  B * Hd * Wd * 4 softmaxes: 1/16 of the
//                       main pass at factor 8.  The (B, C, H, W) softmax never exists.
//   ohem_select_kernel  one workgroup: exact radix select of the k-th smallest key on the fp32 bit patterns (probabilities are
//                       >= 0: unsigned order is float order), four 8-bit passes with an LDS histogram each (wave-aggregated: one
//                       atomic per distinct bin of a wave), any key count.  The first pass's total is num_valid.  Integer
//                       atomics only: bit-reproducible.  Writes threshold and
//                       num_valid to device memory; the host never reads them.
//   ce_cells_kernel<.., OHEM = true> and its finalize / nodes kernels (ce_dev.hpp): the CriterionDSN pass with one comparison per
//                       main-head pixel, a kept count as fourth partial and two normalisers.
#include "ce_dev.hpp"
#include "skd_ohem.h"

#include <math.h>

namespace skd {
namespace {

// one axis of scipy.ndimage.zoom's coordinate map (mode 'constant'): the order-1 taps and weights, the order-0 index, and
// whether the coordinate lies inside the input.  Contraction is off: cc must be the rounded product before floor and subtraction.
struct OhemAxis {
  int i0, i1, near;
  double w0, w1;
  bool inside;
};

__device__ __forceinline__ OhemAxis ohem_axis(int k, int n_in, double step) {
#pragma clang fp contract(off)
  const double cc = (double)k * step;
  const double fl = floor(cc);
  OhemAxis a;
  a.inside = cc <= (double)(n_in - 1);
  a.w1 = cc - fl;
  a.w0 = 1.0 - a.w1;
  int i = (int)fl;
  if (i > n_in - 1) i = n_in - 1;
  if (i < 0) i = 0;
  a.i0 = i;
  a.i1 = i < n_in - 1 ? i + 1 : i;
  int n = (int)floor(cc + 0.5);
  if (n > n_in - 1) n = n_in - 1;
  if (n < 0) n = 0;
  a.near = n;
  return a;
}

// scipy's order-1 value: float64, the four products left to right, summed in this order, one cast
__device__ __forceinline__ float ohem_zoom_sum(float p00, float p01, float p10, float p11, const OhemAxis &ay, const OhemAxis &ax) {
#pragma clang fp contract(off)
  return (float)((double)p00 * ay.w0 * ax.w0 + (double)p01 * ay.w0 * ax.w1 + (double)p10 * ay.w1 * ax.w0 +
                 (double)p11 * ay.w1 * ax.w1);
}

// the softmax probability of class `label` at full-resolution pixel (Y, X) of image b: the main pass's arithmetic
template <int CMAX>
__device__ __forceinline__ float ohem_pixel_p(const float *__restrict__ lm, int b, int C, int h, int w, int Y, int X, float sy,
                                              float sx, int label) {
  const Tap tY = tap_of_strict(Y, sy, h), tX = tap_of_strict(X, sx, w);
  const int hw = h * w;
  const float *p = lm + (int64_t)b * C * hw;
  const unsigned o00 = tY.i0 * w + tX.i0, o01 = tY.i0 * w + tX.i1, o10 = tY.i1 * w + tX.i0, o11 = tY.i1 * w + tX.i1;
  float t0[CMAX], t1[CMAX], v[CMAX];
#pragma unroll
  for (int c = 0; c < CMAX; ++c) {
    const float *q = p + (int64_t)(c < C ? c : 0) * hw;
    const float q00 = q[o00], q01 = q[o01], q10 = q[o10], q11 = q[o11];
    t0[c] = c < C ? ce_lerp(tY.l0, q00, tY.l1, q10) : -1e30f;
    t1[c] = c < C ? ce_lerp(tY.l0, q01, tY.l1, q11) : -1e30f;
  }
  float mx, mxs, z, vt;
  ce_pixel_softmax<CMAX>(t0, t1, tX.l0, tX.l1, label, v, mx, mxs, z, vt);
  return ce_p_label(vt, mxs, z);
}

// keys (B, Hd, Wd): the zoomed probability of the zoomed label, -1 where that label is ignore_index
template <int CMAX>
__global__ __launch_bounds__(kThreads) void ohem_keys_kernel(const float *__restrict__ lm, const int64_t *__restrict__ target,
                                                            float *__restrict__ keys, int B, int C, int h, int w, int H, int W,
                                                            int Hd, int Wd, int ignore_index, float sy, float sx, double step_y,
                                                            double step_x) {
  const int64_t total = (int64_t)B * Hd * Wd;
  const int64_t gid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t pix = gid >> 2;                          // the four lanes of a quad share a down-sampled pixel
  const int corner = (int)(gid & 3);                     // 0: (y0, x0)  1: (y0, x1)  2: (y1, x0)  3: (y1, x1)
  const bool active = pix < total;
  const int64_t q = active ? pix : 0;
  const int xd = (int)(q % Wd), yd = (int)((q / Wd) % Hd), b = (int)(q / ((int64_t)Wd * Hd));
  const OhemAxis ay = ohem_axis(yd, H, step_y), ax = ohem_axis(xd, W, step_x);
  const bool inside = ay.inside && ax.inside;
  const int64_t lab = inside ? target[((int64_t)b * H + ay.near) * W + ax.near] : 0;
  const bool ignored = lab == (int64_t)ignore_index;
  float p = 0.f;
  if (active && inside && !ignored && lab >= 0 && lab < C)
    p = ohem_pixel_p<CMAX>(lm, b, C, h, w, (corner & 2) ? ay.i1 : ay.i0, (corner & 1) ? ax.i1 : ax.i0, sy, sx, (int)lab);
  const int base = (int)(threadIdx.x & (kWave - 1)) & ~3;
  const float p00 = __shfl(p, base, kWave), p01 = __shfl(p, base + 1, kWave);
  const float p10 = __shfl(p, base + 2, kWave), p11 = __shfl(p, base + 3, kWave);
  if (active && corner == 0) keys[pix] = ignored ? -1.f : (inside ? ohem_zoom_sum(p00, p01, p10, p11, ay, ax) : 0.f);
}

constexpr int kSelThreads = 1024, kSelBatch = 8;

// threshold[0], num_valid[0] of find_threshold (criterion.py:27-48) from the keys; one workgroup, launched as <<<1, kSelThreads>>>.
// Label probabilities crowd a few bit patterns (most keys of a trained network lie in [0.5, 1]: ONE value of the top byte), so a
// plain LDS atomic per key would serialise a whole wave on one address.  Each wave therefore first counts its lanes per bin
// with ballots (one iteration per DISTINCT bin among its 64 keys) and issues one atomic per bin; wave 0 then finds the bin that
// holds the wanted rank with a 64-lane scan over four bins per lane.
__global__ __launch_bounds__(kSelThreads) void ohem_select_kernel(const float *__restrict__ keys, int64_t n, float thresh, int mk,
                                                                 float *__restrict__ threshold, int *__restrict__ num_valid) {
  __shared__ unsigned hist[256];
  __shared__ unsigned s_prefix, s_rank;
  __shared__ int s_done;
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  unsigned prefix = 0u, mask = 0u, rank = (unsigned)(mk > 0 ? mk : 0);   // rank: 1-based position of the wanted key among those matching prefix
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (tid < 256) hist[tid] = 0u;
    if (tid == 0) s_done = 0;
    __syncthreads();
    // kSelBatch independent loads per lane are in flight before the first is used: a pass is bound by load latency, not by work
    for (int64_t base = 0; base < n; base += (int64_t)kSelThreads * kSelBatch) {   // the same trip count for every lane of a wave
      unsigned key[kSelBatch];
#pragma unroll
      for (int u = 0; u < kSelBatch; ++u) {
        const int64_t i = base + (int64_t)u * kSelThreads + tid;
        key[u] = i < n ? __float_as_uint(keys[i]) : 0x80000000u;
      }
#pragma unroll
      for (int u = 0; u < kSelBatch; ++u) {
        const unsigned bits = key[u];
        bool want = (bits & 0x80000000u) == 0u && (bits & mask) == prefix;
        const unsigned bin = (bits >> shift) & 255u;
        unsigned long long todo = __ballot(want);
        while (todo != 0ull) {                                           // wave-uniform
          const int leader = __ffsll((long long)todo) - 1;
          const unsigned lb = (unsigned)__shfl((int)bin, leader, kWave);
          const unsigned long long same = __ballot(want && bin == lb);
          if (lane == leader) atomicAdd(&hist[lb], (unsigned)__popcll(same));
          if (bin == lb) want = false;
          todo &= ~same;
        }
      }
    }
    __syncthreads();
    if (tid < kWave) {
      const unsigned h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
      const unsigned own = h0 + h1 + h2 + h3;
      unsigned incl = own;
#pragma unroll
      for (int d = 1; d < kWave; d <<= 1) {
        const unsigned t = (unsigned)__shfl_up((int)incl, d, kWave);
        if (lane >= d) incl += t;
      }
      const unsigned total = (unsigned)__shfl((int)incl, kWave - 1, kWave), excl = incl - own;
      bool done = false;
      if (pass == 0) {                                                 // the first histogram's total is num_valid
        done = (int64_t)mk >= (int64_t)total || mk <= 0;               // (also num_valid == 0)
        if (lane == 0) {
          num_valid[0] = (int)total;
          if (done) {
            threshold[0] = (int64_t)mk >= (int64_t)total ? 1.0f : thresh;
            s_done = 1;
          }
        }
      }
      if (!done && excl < rank && rank <= incl) {                      // exactly one lane: 1 <= rank <= total
        unsigned r = rank - excl, bin = 4u * lane;
        if (r > h0) { r -= h0; ++bin; if (r > h1) { r -= h1; ++bin; if (r > h2) { r -= h2; ++bin; } } }
        s_prefix = prefix | (bin << shift);
        s_rank = r;
      }
    }
    __syncthreads();
    if (s_done) return;
    prefix = s_prefix;
    rank = s_rank;
    mask |= 255u << shift;
  }
  if (tid == 0) {
    const float kth = __uint_as_float(prefix);
    threshold[0] = kth > thresh ? kth : thresh;
  }
}

}  // namespace
}  // namespace skd

using namespace skd;

// Python's round(n * (1.0 / factor)): scipy.ndimage.zoom's output length (half to even in the default rounding mode)
static int ohem_ds_size(int n, int factor) { return (int)nearbyint((double)n * (1.0 / (double)factor)); }

static int64_t ohem_main_floats(int B, int C, int h, int w) {
  int NTy, NTx;
  ce_tiles(h, w, NTy, NTx);
  const int64_t wgs = (int64_t)B * NTy * NTx;
  return 8 + wgs * 4 + (int64_t)B * 2 * C * NTy * (kCeTJ + 1) * NTx * (kCeTI + 1);
}

extern "C" {

int64_t skd_ce_ohem_workspace_floats(int B, int C, int h, int w, int H, int W, int factor) {
  if (B <= 0 || C <= 0 || h <= 0 || w <= 0) return 8;
  int64_t n = ohem_main_floats(B, C, h, w);
  if (H > 0 && W > 0 && factor >= 1) {
    const int64_t keys = (int64_t)B * ohem_ds_size(H, factor) * ohem_ds_size(W, factor);
    if (keys > n) n = keys;
  }
  return n;
}

int skd_ohem_threshold(int B, int C, int h, int w, int H, int W, const float *logits_main, const int64_t *target,
                       int ignore_index, float thresh, int min_kept, int factor, float *threshold, int32_t *num_valid,
                       float *pred_ds, float *workspace, skd_stream_t stream) {
  if (B <= 0 || C <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return 0;
  if (!logits_main || !target || !threshold || !num_valid || !workspace) return 0;
  if (C > 64 || factor < 1 || min_kept < 0) return 0;
  const int Hd = ohem_ds_size(H, factor), Wd = ohem_ds_size(W, factor);
  if (Hd < 1 || Wd < 1) return 0;
  if ((Hd == 1 && H > 1) || (Wd == 1 && W > 1)) return 0;   // scipy's step (n_in - 1) / (n_out - 1) is undefined there
  const int64_t n = (int64_t)B * Hd * Wd;
  if (n > 2147483647 / 4) return 0;
  hipStream_t st = as_stream(stream);
  float *keys = pred_ds ? pred_ds : workspace;
  const double step_y = Hd > 1 ? (double)(H - 1) / (double)(Hd - 1) : 0.0;
  const double step_x = Wd > 1 ? (double)(W - 1) / (double)(Wd - 1) : 0.0;
  const float sy = scale_of(h, H), sx = scale_of(w, W);
  const dim3 grid((unsigned)cdiv(n * 4, kThreads)), block(kThreads);
#define SKD_OHEM_KEYS(CM)                                                                                                  \
  ohem_keys_kernel<CM><<<grid, block, 0, st>>>(logits_main, target, keys, B, C, h, w, H, W, Hd, Wd, ignore_index, sy, sx, \
                                               step_y, step_x)
  switch (ce_cmax(C)) {
    case 12: SKD_OHEM_KEYS(12); break;
    case 19: SKD_OHEM_KEYS(19); break;
    case 24: SKD_OHEM_KEYS(24); break;
    default: SKD_OHEM_KEYS(64); break;
  }
#undef SKD_OHEM_KEYS
  const int64_t mk = (int64_t)min_kept / ((int64_t)factor * factor);
  ohem_select_kernel<<<dim3(1), dim3(kSelThreads), 0, st>>>(keys, n, thresh, (int)mk, threshold, num_valid);
  return ok();
}

int skd_ce_ohem_dsn_forward(int B, int C, int h, int w, int H, int W, const float *logits_main, const float *logits_dsn,
                            const int64_t *target, int ignore_index, float aux_weight, const float *threshold, float *loss,
                            float *n_kept, uint8_t *kept, float *grad_main, float *grad_dsn, float *workspace,
                            skd_stream_t stream) {
  if (B <= 0 || C <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return 0;
  if (!logits_main || !target || !threshold || !loss || !workspace) return 0;
  if (grad_dsn && !logits_dsn) return 0;
  if (C > 64) return 0;
  hipStream_t st = as_stream(stream);
  const bool two = logits_dsn != nullptr;
  const int heads = two ? 2 : 1;
  int NTy, NTx;
  ce_tiles(h, w, NTy, NTx);
  const int64_t wgs = (int64_t)B * NTy * NTx;
  if (wgs > 2147483647) return 0;
  float *stat = workspace;
  float *part = workspace + 8;
  float *pnodes = (grad_main || grad_dsn) ? part + wgs * 4 : nullptr;
  const float sy = scale_of(h, H), sx = scale_of(w, W);
#define SKD_CE_LAUNCH(CM, TWO_)                                                                                              \
  do {                                                                                                                       \
    const size_t lds_ = sizeof(float) * 4 * CM * kCeCells;                                                                   \
    static PerDeviceFlag attr_;                                                                                              \
    bool *done_ = attr_.get();                                                                                               \
    if (done_ && !*done_) {                                                                                                  \
      if (hipFuncSetAttribute(reinterpret_cast<const void *>(ce_cells_kernel<CM, TWO_, true>),                               \
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_) != hipSuccess)                          \
        return 0;                                                                                                            \
      *done_ = true;                                                                                                         \
    }                                                                                                                        \
    ce_cells_kernel<CM, TWO_, true><<<dim3((unsigned)(8 * cdiv(wgs, 8))), dim3(kCeThreads), lds_, st>>>(                     \
        logits_main, logits_dsn, target, pnodes, part, B, C, h, w, H, W, ignore_index, sy, sx, NTy, NTx, threshold, kept);   \
  } while (0)
#define SKD_CE(CM)                    \
  do {                                \
    if (two) SKD_CE_LAUNCH(CM, true); \
    else SKD_CE_LAUNCH(CM, false);    \
  } while (0)
  switch (ce_cmax(C)) {
    case 12: SKD_CE(12); break;
    case 19: SKD_CE(19); break;
    case 24: SKD_CE(24); break;
    default: SKD_CE(64); break;
  }
#undef SKD_CE
#undef SKD_CE_LAUNCH
  ce_finalize_kernel<true><<<dim3(1), dim3(kThreads), 0, st>>>(part, wgs, two ? aux_weight : 0.f, loss, stat, n_kept);
  if (pnodes != nullptr) {
    const int64_t n = (int64_t)B * heads * C * h * w;
    const dim3 grid((unsigned)cdiv(n, kThreads)), block(kThreads);
    ce_nodes_kernel<kCeTJ, kCeTI, true><<<grid, block, 0, st>>>(pnodes, stat, grad_main, grad_dsn, B, C, h, w, heads, aux_weight,
                                                                NTy, NTx);
  }
  return ok();
}

}  // extern "C"
