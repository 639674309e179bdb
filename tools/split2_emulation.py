"""CPU float64 emulation of the two-piece mode (include/skd_split2.h; the model: tests/split2_ref.py) -- no GPU needed.

    python tools/split2_emulation.py [--seed S] [--skip-cases]

Prints (1) for one product of post-ReLU Gaussian data at K = 256 ... 18432: the error of the three-, two- and one-piece models
against the float64 product, in units of the output's largest magnitude; (2) for the small teacher forward
of the network test (tests/split2_ref.teacher_case: ResNet101 plan, 1 x 3 x 129 x 129): the same two figures on `logits`, `dsn`
and the PSP feature, the largest softmax difference and the argmax agreement, with only the convolutions emulated that run on the
split core today; and whether the fp32 forward agrees with the float64 one on every argmax (how the seed was chosen).  The
two-piece teacher figures are the constants E of tests/test_split2_gpu.py and of profiles/r25_split2_accuracy.md.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import split2_ref as R  # noqa: E402


def single_products():
    print("one product, post-ReLU Gaussian data, exact accumulation: error / max |output|")
    print("| K | three pieces | two pieces | one piece |")
    print("|---|---|---|---|")
    g = torch.Generator().manual_seed(0)
    for k in (256, 2304, 4608, 18432):
        a = torch.relu(torch.randn(256, k, generator=g) + 0.5 * torch.randn(1, k, generator=g))
        b = torch.randn(128, k, generator=g) * (2.0 / k) ** 0.5
        want = a.double() @ b.double().t()
        print("| %d | %.2e | %.2e | %.2e |" % (k, R.rel_err(R.mm_split2(a, b, 3), want), R.rel_err(R.mm_split2(a, b, 2), want),
                                              R.rel_err(R.mm_split2(a, b, 1), want)))


def teacher(seed):
    P, x = R.teacher_case(seed)
    truth = R.teacher_forward64(P, x)
    names = ("logits", "dsn", "psp")
    print("\nteacher forward, seed %d, input %s: error / max |output| against the float64 forward" % (seed, tuple(x.shape)))
    print("| path | logits | dsn | psp | max softmax diff | argmax agreement |")
    print("|---|---|---|---|---|---|")
    sm = torch.softmax(truth[0], 1)

    def row(label, got):
        errs = [R.rel_err(g, t) for g, t in zip(got, truth)]
        agree = float((got[0].argmax(1) == truth[0].argmax(1)).double().mean())
        print("| %s | %.3e | %.3e | %.3e | %.2e | %.6f |" % (label, *errs, float((torch.softmax(got[0].double(), 1) - sm).abs().max()), agree))
        return dict(zip(names, errs)), agree
    _, agree32 = row("fp32 (CPU)", R.teacher_forward32(P, x))
    row("three pieces", R.teacher_forward64(P, x, R.split_core_conv2d(3)))
    e2, agree2 = row("two pieces", R.teacher_forward64(P, x, R.split_core_conv2d(2)))
    print("\nfp32 forward agrees with float64 on every argmax: %s; two-piece emulation: %s" % (agree32 == 1.0, agree2 == 1.0))
    print("E = {%s}" % ", ".join('"%s": %.3e' % (n, e2[n]) for n in names))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=R.TEACHER_SEED)
    ap.add_argument("--skip-cases", action="store_true", help="the teacher forward only")
    a = ap.parse_args()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    if not a.skip_cases:
        single_products()
    teacher(a.seed)
