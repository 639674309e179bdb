"""GPU tool: regenerate the PARENT_ERR / PARENT_TRAIN_ERR constants of tests/test_conv3x3_narrow_gpu.py and the tables of
profiles/r21_conv3x3_narrow_accuracy.md -- per case of that test, on the test's own seeded inputs, max |got - want| / max |want|
against ``F.conv2d`` (and its autograd) in float64 on the CPU of (a) the parent path: MIOpen's fp32 ``F.conv2d`` on the GPU
followed by the library's eval-mode ABN pass (with the residual) where the case has an epilogue, MIOpen's backward-data kernel
for the data gradients, and (b) the 64-column form of the split core (csrc/conv3x3.hip, include/skd_narrow.h).
    python tools/conv3x3_narrow_parent_err.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
os.environ.setdefault("PYTORCH_MIOPEN_SUGGEST_NHWC", "1")


def parent_path(x, wt, p, d, dev="cuda"):
    """MIOpen's fp32 convolution (+ bias) on the GPU, then the library's eval-mode ABN pass (+ residual)."""
    import torch
    import torch.nn.functional as F
    from structure_knowledge_distillation_amd.libs.inplace_abn import abn_eval_fused
    dx = x.to(dev).contiguous(memory_format=torch.channels_last)
    dw = wt.to(dev).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        y = F.conv2d(dx, dw, None if p["cbias"] is None else p["cbias"].to(dev), 1, d, d)
        if p["mean"] is not None:
            y = abn_eval_fused(y, p["gamma"].to(dev), p["beta"].to(dev), p["mean"].to(dev), p["var"].to(dev), p["eps"], p["act"], 0.01,
                               None if p["res"] is None else p["res"].to(dev))
    torch.cuda.synchronize()
    return y.cpu()


def fmt(v):
    return "n/a" if v is None else "%.3e" % v


def main():
    import torch
    import torch.nn.functional as F
    import structure_knowledge_distillation_amd as _skd
    _skd.configure_miopen()
    from structure_knowledge_distillation_amd import _lib
    import test_conv3x3_narrow_gpu as T
    hip = _lib.load()
    print("| case | K = 9 Cin | parent | committed PARENT_ERR | narrow | narrow / parent | bound |")
    print("|---|---|---|---|---|---|---|")
    for name, _, cin, _, _, _, d, _ in T.CASES:
        x, wt, p = T.case_inputs(name)
        want = T.want_of(name)
        parent = T.rel_err(parent_path(x, wt, p, d), want)
        got = T.rel_err(T.run_narrow(hip, x, wt, p, d), want)
        print("| %s | %d | %.3e | %s | %.3e | %.2f | %.3e |" % (name, 9 * cin, parent, fmt(T.PARENT_ERR[name]), got, got / parent,
                                                            min(T.RATIO * parent, T.CAP)), flush=True)
    print()
    print("| training case | parent forward | committed | op forward | parent dgrad | committed | op dgrad |")
    print("|---|---|---|---|---|---|---|")
    for name, _, _ in T.TRAIN_CASES:
        x, wt, go = T.train_inputs(name)
        want_y, want_dx = T.train_want(name)
        dx, dw, dg = x.to("cuda"), wt.to("cuda"), go.to("cuda")
        with torch.no_grad():
            py = F.conv2d(dx, dw, None, 1, 1, 1)
            pdx, _, _ = torch.ops.aten.convolution_backward(dg, dx, dw, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1, (True, False, False))
        y, gx, _, _ = T.run_train_op(name)
        com = T.PARENT_TRAIN_ERR[name]
        print("| %s | %.3e | %s | %.3e | %.3e | %s | %.3e |" % (name, T.rel_err(py.cpu(), want_y), fmt(com[0]), T.rel_err(y.cpu(), want_y),
                                                             T.rel_err(pdx.cpu(), want_dx), fmt(com[1]), T.rel_err(gx.cpu(), want_dx)),
              flush=True)


if __name__ == "__main__":
    main()
