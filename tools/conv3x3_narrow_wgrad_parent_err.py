"""GPU tool: regenerate the PARENT_NARROW_WGRAD_ERR constants of tests/test_conv3x3_narrow_wgrad_gpu.py and the table of
profiles/r23_conv3x3_narrow_wgrad_accuracy.md -- per realistic-data case of that test, on the test's own seeded inputs,
max |got - want| / max |want| against autograd of ``F.conv2d`` in float64 on the CPU of (a) the parent path, MIOpen's fp32
weight-gradient kernels through ``aten.convolution_backward`` with mask (False, True, False), and (b) the two launches of
skd_conv3x3_narrow_wgrad_nhwc with the plan the case names.  ``--stem`` adds the two reductions of the stem, 64 -> 64 and
64 -> 128 at 8 x 256 x 256 (P = 524,288, 16 x the longest case of the test; their float64 truth takes the CPU a minute or
two, which is why they are in the note and not in the test).
    python tools/conv3x3_narrow_wgrad_parent_err.py [--stem]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("PYTORCH_MIOPEN_SUGGEST_NHWC", "1")

STEM_CASES = [
    ("narrow-wgrad-stem-64-64-256x256-d1", 8, 64, 64, 256, 256, 1, 0),
    ("narrow-wgrad-stem-64-128-256x256-d1", 8, 64, 128, 256, 256, 1, 0),
]


def main():
    import structure_knowledge_distillation_amd as _skd
    _skd.configure_miopen()
    from structure_knowledge_distillation_amd import _lib
    from conv3x3_wgrad_parent_err import parent_path
    import test_conv3x3_narrow_wgrad_gpu as T
    hip = _lib.load()
    cases = [(c, T.PARENT_NARROW_WGRAD_ERR[c[0]]) for c in T.REAL_CASES]
    if "--stem" in sys.argv:
        cases += [(c, None) for c in STEM_CASES]
    print("| case | P = B H W | slices | parent | committed PARENT_NARROW_WGRAD_ERR | split | split / parent | bound |")
    print("|---|---|---|---|---|---|---|---|")
    for case, committed in cases:
        name, b, _, _, h, w, d, slices = case
        x, g = T.real_inputs(name, case)
        want = T.wgrad64(x, g, d)
        parent = T.rel_err(parent_path(x, g, d), want)
        split = T.rel_err(T.run_entry(hip, x, g, d, slices), want)
        print("| %s | %d | %d | %.3e | %s | %.3e | %.2f | %.3e |" % (
            name, b * h * w, T.plan_of(hip, x, g, slices)[0], parent, "-" if committed is None else "%.3e" % committed, split,
            split / parent, min(T.RATIO * (parent if committed is None else committed), T.CAP)), flush=True)


if __name__ == "__main__":
    main()
