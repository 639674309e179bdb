"""GPU tool: regenerate the PARENT_ERR constants of tests/test_conv3x3_stride2_gpu.py and the table of
profiles/r27_conv3x3_stride2_accuracy.md -- per case of that test, on the test's own seeded inputs, max |got - want| / max |want|
against ``F.conv2d(stride=2, padding=1)`` (+ the eval-mode ABN formula) in float64 on the CPU of (a) the library path: MIOpen's fp32
``F.conv2d`` on the GPU followed by the library's eval-mode ABN pass where the case has the epilogue, and (b) the stride-2 form of
the split core (csrc/conv3x3.hip, include/skd_stride2.h) with three and, for the record, with two pieces.
    python tools/conv3x3_stride2_parent_err.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
os.environ.setdefault("PYTORCH_MIOPEN_SUGGEST_NHWC", "1")


def library_path(x, wt, p, dev="cuda"):
    """MIOpen's fp32 stride-2 convolution (+ bias) on the GPU, then the library's eval-mode ABN pass."""
    import torch
    import torch.nn.functional as F
    from structure_knowledge_distillation_amd.libs.inplace_abn import abn_eval_fused
    dx = x.to(dev).contiguous(memory_format=torch.channels_last)
    dw = wt.to(dev).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        y = F.conv2d(dx, dw, None if p["cbias"] is None else p["cbias"].to(dev), 2, 1, 1)
        if p["mean"] is not None:
            y = abn_eval_fused(y, p["gamma"].to(dev), p["beta"].to(dev), p["mean"].to(dev), p["var"].to(dev), p["eps"], p["act"], 0.01, None)
    torch.cuda.synchronize()
    return y.cpu()


def main():
    import structure_knowledge_distillation_amd as _skd
    _skd.configure_miopen()
    from structure_knowledge_distillation_amd import _lib
    import test_conv3x3_stride2_gpu as T
    hip = _lib.load()
    print("| case | K = 9 Cin | library | committed PARENT_ERR | three pieces | three / library | bound | two pieces |")
    print("|---|---|---|---|---|---|---|---|")
    lines = []
    for shape in T.SHAPES:
        for epi in T.EPILOGUES:
            name = T.case_name(shape, epi)
            x, wt, p = T.case_inputs(shape, epi)
            want = T.want_of(shape, epi)
            parent = T.rel_err(library_path(x, wt, p), want)
            got = T.rel_err(T.run_s2(hip, x, wt, p), want)
            two = T.rel_err(T.run_s2(hip, x, wt, p, 2), want)
            com = T.PARENT_ERR.get(name)
            print("| %s | %d | %.3e | %s | %.3e | %.2f | %.3e | %.3e |" % (name, 9 * shape[3], parent, "n/a" if com is None else "%.3e" % com, got,
                                                                        got / parent, min(T.RATIO * parent, T.CAP), two), flush=True)
            lines.append('    "%s": %.3e,' % (name, parent))
    print()
    print("PARENT_ERR = {")
    print("\n".join(lines))
    print("}")


if __name__ == "__main__":
    main()
