"""GPU tool: regenerate the routed-shape PARENT_ERR constants of tests/test_conv1x1_split_gpu.py and the table of
profiles/r13_conv1x1_reduce_accuracy.md -- per ROUTED case of that test, on the test's own seeded inputs and at the test's own M
for this device, max |got - want| / max |want| against the float64 product + float64 eval-ABN formula on the CPU of (a) the parent
path, ``functional.conv1x1_bn_blas`` (the library GEMM with the folded BN these layers ran before pspnet_combine.SPLIT_REDUCE),
and (b) the split-core kernel of csrc/conv1x1.hip.
    python tools/conv1x1_parent_err.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def parent_path(x, w, bn, relu, dev="cuda"):
    """conv1x1_bn_blas on a channels-last (1, K, M, 1) map through a Conv2d and an InPlaceABNSync that hold the case's parameters."""
    import torch
    from structure_knowledge_distillation_amd import functional as SF
    from structure_knowledge_distillation_amd.libs import InPlaceABNSync
    m, k = x.shape
    n = w.shape[0]
    mean, var, ga, be, eps = bn
    conv = torch.nn.Conv2d(k, n, 1, bias=False)
    abn = InPlaceABNSync(n, eps=eps, activation="none")
    with torch.no_grad():
        conv.weight.copy_(w.view(n, k, 1, 1))
        abn.weight.copy_(ga)
        abn.bias.copy_(be)
        abn.running_mean.copy_(mean)
        abn.running_var.copy_(var)
    conv, abn = conv.to(dev).eval(), abn.to(dev).eval()
    dx = x.to(dev).view(1, m, 1, k).permute(0, 3, 1, 2)              # (1, K, M, 1), channels-last memory
    with torch.no_grad():
        assert SF.blas_1x1_bn_supported(dx, conv)
        y = SF.conv1x1_bn_blas(dx, conv, abn, relu=relu)
    torch.cuda.synchronize()
    return y.permute(0, 2, 3, 1).reshape(m, n).cpu()


def main():
    from structure_knowledge_distillation_amd import _lib
    import test_conv1x1_split_gpu as T
    hip = _lib.load()
    print("%d compute units" % T.cu_count())
    print("| case | K | M | parent | committed PARENT_ERR | split | split / parent | bound | split / 2e-6 |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name, k, n, act, _, _ in T.ROUTED:
        split, _, (x, w, bn), want = T.routed_case_error(hip, name)
        parent = T.rel_err(parent_path(x, w, bn, act == T.ACT_RELU), want)
        committed = T.PARENT_ERR.get(name)
        bound = min(T.RATIO * (parent if committed is None else committed), T.ROUTED_CAP)
        print("| %s | %d | %d | %.3e | %s | %.3e | %.2f | %.3e | %.2f |" % (
            name, k, x.shape[0], parent, "-" if committed is None else "%.3e" % committed, split, split / parent, bound, split / T.CAP),
            flush=True)


if __name__ == "__main__":
    main()
