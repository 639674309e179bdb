"""Generates tests/golden/student_infer_oracle.pt: the float64 CPU-oracle eval-mode forward of a seeded student on a seeded
(2, 3, 65, 97) image, for tests/test_student_infer_gpu.py (the whole-student check of the fused inference form).

    python tests/golden/make_golden_student_infer.py          (a few seconds)

Conventions of make_golden_gpu_suite.py: nothing large is stored -- the weights come from oracle.step_torch.pspnet_init(seed)
with seeded, trained-looking running statistics, the image from a seeded generator, the fixture carries weight checksums (a
drifted torch RNG is detected, not trusted) and per output a strided sample of the float64 result with its norm (``rec``).
Outputs recorded: ``[x, x_dsn, x_feat_after_psp, x4, x3]`` of ``oracle.step_torch.pspnet_forward`` in eval mode.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
from oracle import step_torch as O  # noqa: E402
from make_golden_gpu_suite import cast, checksum, rec  # noqa: E402

OUT = os.path.join(HERE, "student_infer_oracle.pt")
SEEDS = {"student": 291, "stats": 292, "x": 293}
NAMES = ["x", "x_dsn", "x_feat_after_psp", "x4", "x3"]
NSAMPLE = 4096


def inputs():
    """(fp32 state dict, fp32 image): what the GPU holds; the oracle runs on the same values widened to float64."""
    P = O.pspnet_init(O.STUDENT, 19, seed=SEEDS["student"])
    g = torch.Generator().manual_seed(SEEDS["stats"])
    for k, v in P.items():
        if k.endswith("running_var"):
            v.copy_(torch.rand(v.shape, generator=g) + 0.5)
        elif k.endswith("running_mean"):
            v.copy_(torch.randn(v.shape, generator=g) * 0.1)
    x = torch.randn(2, 3, 65, 97, generator=torch.Generator().manual_seed(SEEDS["x"])) * 57
    return P, x


def main():
    P, x = inputs()
    with torch.no_grad():
        out = O.pspnet_forward(cast(P, torch.float64), x.double(), O.STUDENT, False)
    fx = {"checksums": checksum(P), "names": NAMES, "outputs": [rec(t, n=NSAMPLE) for t in out[:len(NAMES)]]}
    torch.save(fx, OUT)
    print("wrote %s: %d bytes; shapes %s" % (OUT, os.path.getsize(OUT), [r["shape"] for r in fx["outputs"]]))


if __name__ == "__main__":
    main()
