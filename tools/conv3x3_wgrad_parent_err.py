"""GPU tool: regenerate the PARENT_WGRAD_ERR constants of tests/test_conv3x3_wgrad_gpu.py and the table of
profiles/r20_conv3x3_wgrad_accuracy.md -- per realistic-data case of that test, on the test's own seeded inputs,
max |got - want| / max |want| against autograd of ``F.conv2d`` in float64 on the CPU of (a) the parent path, MIOpen's fp32
weight-gradient kernels through ``aten.convolution_backward`` with mask (False, True, False), and (b) the two launches of
skd_conv3x3_split_wgrad_nhwc with the plan the case names.
    python tools/conv3x3_wgrad_parent_err.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("PYTORCH_MIOPEN_SUGGEST_NHWC", "1")


def parent_path(x, g, d, dev="cuda"):
    """MIOpen's fp32 weight gradient on the GPU, channels-last operands and weight as in the training student."""
    import torch
    dx, dg = x.to(dev), g.to(dev)
    w = torch.zeros(g.shape[1], x.shape[1], 3, 3, device=dev).contiguous(memory_format=torch.channels_last)
    _, dw, _ = torch.ops.aten.convolution_backward(dg, dx, w, None, [1, 1], [d, d], [d, d], False, [0, 0], 1, (False, True, False))
    torch.cuda.synchronize()
    return dw.cpu()


def main():
    import structure_knowledge_distillation_amd as _skd
    _skd.configure_miopen()
    from structure_knowledge_distillation_amd import _lib
    import test_conv3x3_wgrad_gpu as T
    hip = _lib.load()
    print("| case | P = B H W | slices | parent | committed PARENT_WGRAD_ERR | split | split / parent | bound |")
    print("|---|---|---|---|---|---|---|---|")
    for name, b, _, _, h, w, d, slices in T.REAL_CASES:
        x, g = T.real_inputs(name)
        want = T.want_of(name)
        parent = T.rel_err(parent_path(x, g, d), want)
        split = T.rel_err(T.run_entry(hip, x, g, d, slices), want)
        committed = T.PARENT_WGRAD_ERR[name]
        print("| %s | %d | %d | %.3e | %s | %.3e | %.2f | %.3e |" % (
            name, b * h * w, T.plan_of(hip, x, g, slices)[0], parent, "-" if committed is None else "%.3e" % committed, split,
            split / parent, min(T.RATIO * (parent if committed is None else committed), T.CAP)), flush=True)


if __name__ == "__main__":
    main()
