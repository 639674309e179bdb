"""GPU tool: regenerate the PARENT_ERR constants of tests/test_conv3x3_split_gpu.py and the table of
profiles/r12_conv3x3_split_accuracy.md -- per case of that test, on the test's own seeded inputs, max |got - want| / max |want|
against ``F.conv2d`` in float64 on the CPU of (a) the parent path, MIOpen's fp32 ``F.conv2d`` on the GPU followed by the
library's eval-mode ABN pass where the case has an epilogue, and (b) the split-core kernel of csrc/conv3x3.hip.
    python tools/conv3x3_parent_err.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("PYTORCH_MIOPEN_SUGGEST_NHWC", "1")


def parent_path(x, wt, p, d, dev="cuda"):
    """MIOpen's fp32 convolution (+ bias) on the GPU, then the library's eval-mode ABN pass."""
    import torch
    import torch.nn.functional as F
    from structure_knowledge_distillation_amd.libs.inplace_abn import abn_eval_fused
    dx = x.to(dev).contiguous(memory_format=torch.channels_last)
    dw = wt.to(dev).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        y = F.conv2d(dx, dw, None if p["cbias"] is None else p["cbias"].to(dev), 1, d, d)
        if p["mean"] is not None:
            y = abn_eval_fused(y, p["gamma"].to(dev), p["beta"].to(dev), p["mean"].to(dev), p["var"].to(dev), p["eps"], p["act"], 0.01)
    torch.cuda.synchronize()
    return y.cpu()


def main():
    import structure_knowledge_distillation_amd as _skd
    _skd.configure_miopen()
    from structure_knowledge_distillation_amd import _lib
    import test_conv3x3_split_gpu as T
    hip = _lib.load()
    print("| case | K = 9 Cin | parent | committed PARENT_ERR | split | split / parent | bound |")
    print("|---|---|---|---|---|---|---|")
    for name, _, cin, _, _, _, d, _ in T.CASES:
        x, wt, p = T.case_inputs(name)
        want = T.want_of(name)
        parent = T.rel_err(parent_path(x, wt, p, d), want)
        split = T.rel_err(T.run_hip(hip, x, wt, p, d)[0], want)
        print("| %s | %d | %.3e | %.3e | %.3e | %.2f | %.3e |" % (name, 9 * cin, parent, T.PARENT_ERR[name], split, split / parent,
                                                              min(T.RATIO * T.PARENT_ERR[name], T.CAP)), flush=True)


if __name__ == "__main__":
    main()
