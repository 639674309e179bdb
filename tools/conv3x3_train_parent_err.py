"""GPU tool: regenerate the PARENT_DGRAD_ERR constants of tests/test_conv3x3_train_gpu.py and the table of
profiles/r18_conv3x3_train_accuracy.md -- per data-gradient case of that test, on the test's own seeded inputs,
max |got - want| / max |want| against autograd of ``F.conv2d`` in float64 on the CPU of (a) the parent path, MIOpen's fp32
backward-data kernel through ``aten.convolution_backward`` with mask (True, False, False), and (b) the split core on the
flipped, transposed image that skd_conv3x3_split_pack_pair writes.
    python tools/conv3x3_train_parent_err.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("PYTORCH_MIOPEN_SUGGEST_NHWC", "1")


def parent_path(go, wt, d, dev="cuda"):
    """MIOpen's fp32 backward-data on the GPU, channels-last operands as in the training student."""
    import torch
    dg = go.to(dev).contiguous(memory_format=torch.channels_last)
    dw = wt.to(dev).contiguous(memory_format=torch.channels_last)
    x = torch.zeros(go.shape[0], wt.shape[1], go.shape[2], go.shape[3], device=dev).contiguous(memory_format=torch.channels_last)
    dx, _, _ = torch.ops.aten.convolution_backward(dg, x, dw, None, [1, 1], [d, d], [d, d], False, [0, 0], 1, (True, False, False))
    torch.cuda.synchronize()
    return dx.cpu()


def main():
    import structure_knowledge_distillation_amd as _skd
    _skd.configure_miopen()
    from structure_knowledge_distillation_amd import _lib
    import test_conv3x3_train_gpu as T
    hip = _lib.load()
    print("| case | K = 9 Cout | parent | committed PARENT_DGRAD_ERR | split | split / parent | bound |")
    print("|---|---|---|---|---|---|---|")
    for name, _, cout, _, _, _, d in T.DGRAD_CASES:
        go, wt = T.dgrad_inputs(name)
        want = T.want_of(name)
        parent = T.rel_err(parent_path(go, wt, d), want)
        split = T.rel_err(T.run_dgrad(hip, go, wt, d), want)
        print("| %s | %d | %.3e | %.3e | %.3e | %.2f | %.3e |" % (name, 9 * cout, parent, T.PARENT_DGRAD_ERR[name], split, split / parent,
                                                              min(T.RATIO * T.PARENT_DGRAD_ERR[name], T.CAP)), flush=True)


if __name__ == "__main__":
    main()
