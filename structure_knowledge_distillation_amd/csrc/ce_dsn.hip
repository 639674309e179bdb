// ce_dsn.hip -- CriterionDSN fused (reference utils/criterion.py:179-188): the C-ABI entry points skd_ce_dsn_workspace_floats and
// skd_ce_dsn_forward.  The kernels, and the description of the design (cells / nodes, thread layout, tile order, class-count
// instantiations), are in ce_dev.hpp, which ce_ohem.hip shares.
#include "ce_dev.hpp"

using namespace skd;

extern "C" {

int64_t skd_ce_dsn_workspace_floats(int B, int C, int h, int w, int H, int W) {
  (void)H;
  (void)W;
  if (B <= 0 || C <= 0 || h <= 0 || w <= 0) return 8;
  int NTy, NTx;
  ce_tiles(h, w, NTy, NTx);
  const int64_t wgs = (int64_t)B * NTy * NTx;
  return 8 + wgs * 3 + (int64_t)B * 2 * C * NTy * (kCeTJ + 1) * NTx * (kCeTI + 1);
}

int skd_ce_dsn_forward(int B, int C, int h, int w, int H, int W, const float *logits_main,
                       const float *logits_dsn, const int64_t *target, int ignore_index, float aux_weight,
                       float *loss, float *grad_main, float *grad_dsn, float *workspace, skd_stream_t stream) {
  if (B <= 0 || C <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return 0;
  if (!logits_main || !target || !loss || !workspace) return 0;
  if (grad_dsn && !logits_dsn) return 0;
  if (C > 64) return 0;  // class count of this path: 19 (Cityscapes), 11 (CamVid), 21 (VOC)
  hipStream_t st = as_stream(stream);
  const bool two = logits_dsn != nullptr;
  const int heads = two ? 2 : 1;
  int NTy, NTx;
  ce_tiles(h, w, NTy, NTx);
  const int64_t wgs = (int64_t)B * NTy * NTx;
  if (wgs > 2147483647) return 0;
  float *stat = workspace;
  float *part = workspace + 8;
  float *pnodes = (grad_main || grad_dsn) ? part + wgs * 3 : nullptr;
  const float sy = scale_of(h, H), sx = scale_of(w, W);
#define SKD_CE_LAUNCH(CM, TWO_)                                                                                              \
  do {                                                                                                                       \
    const size_t lds_ = sizeof(float) * 4 * CM * kCeCells;                                                                   \
    static PerDeviceFlag attr_;                                                                                              \
    bool *done_ = attr_.get();                                                                                               \
    if (done_ && !*done_) {                                                                                                  \
      if (hipFuncSetAttribute(reinterpret_cast<const void *>(ce_cells_kernel<CM, TWO_>),                                     \
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_) != hipSuccess)                          \
        return 0;                                                                                                            \
      *done_ = true;                                                                                                         \
    }                                                                                                                        \
    ce_cells_kernel<CM, TWO_><<<dim3((unsigned)(8 * cdiv(wgs, 8))), dim3(kCeThreads), lds_, st>>>(logits_main, logits_dsn, target, pnodes,  \
                                                                                 part, B, C, h, w, H, W, ignore_index, sy, \
                                                                                 sx, NTy, NTx, nullptr, nullptr);            \
  } while (0)
#define SKD_CE(CM)              \
  do {                          \
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
  ce_finalize_kernel<<<dim3(1), dim3(kThreads), 0, st>>>(part, wgs, two ? aux_weight : 0.f, loss, stat, nullptr);
  if (pnodes != nullptr) {
    const int64_t n = (int64_t)B * heads * C * h * w;
    const dim3 grid((unsigned)cdiv(n, kThreads)), block(kThreads);
    ce_nodes_kernel<kCeTJ, kCeTI><<<grid, block, 0, st>>>(pnodes, stat, grad_main, grad_dsn, B, C, h, w, heads, aux_weight, NTy, NTx);
  }
  return ok();
}

}  // extern "C"
