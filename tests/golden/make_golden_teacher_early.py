"""Generates tests/golden/teacher_early_oracle.pt: the float64 CPU-oracle eval-mode forward of a seeded ResNet101-plan teacher on a
seeded (1, 3, 97, 97) image, for tests/test_conv3x3_stride2_gpu.py (the whole-teacher check of route_teacher_early).

    python tests/golden/make_golden_teacher_early.py          (well under a minute)

Conventions of make_golden_student_infer.py: nothing large is stored -- the weights come from oracle.step_torch.pspnet_init(seed)
with seeded, trained-looking running statistics, the image from a seeded generator, the fixture carries weight checksums (a
drifted torch RNG is detected, not trusted) and per output a strided sample of the float64 result with its norm (``rec``).
Outputs recorded: ``x2``, ``x1`` and the logits of ``oracle.step_torch.pspnet_forward`` in eval mode.  At 97 x 97 the stem leaves a
49 x 49 map and its ceil-mode pool a 25 x 25 one, so layer1 runs at 25 x 25 and layer2.0's stride-2 convolution maps 25 x 25 to
13 x 13: the stride-2 form is exercised with an odd size on both axes.  The logits (19 x 13 x 13) are recorded whole.
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

OUT = os.path.join(HERE, "teacher_early_oracle.pt")
SEEDS = {"teacher": 2711, "stats": 2712, "x": 2713}
NAMES = ["x2", "x1", "logits"]
NSAMPLE = 4096


def inputs():
    """(fp32 state dict, fp32 image): what the GPU holds; the oracle runs on the same values widened to float64."""
    P = O.pspnet_init(O.TEACHER, 19, seed=SEEDS["teacher"])
    g = torch.Generator().manual_seed(SEEDS["stats"])
    for k, v in P.items():
        if k.endswith("running_var"):
            v.copy_(torch.rand(v.shape, generator=g) + 0.5)
        elif k.endswith("running_mean"):
            v.copy_(torch.randn(v.shape, generator=g) * 0.1)
    x = torch.randn(1, 3, 97, 97, generator=torch.Generator().manual_seed(SEEDS["x"])) * 57
    return P, x


def main():
    P, x = inputs()
    with torch.no_grad():
        out = O.pspnet_forward(cast(P, torch.float64), x.double(), O.TEACHER, False)
    picked = [out[5], out[6], out[0]]
    fx = {"checksums": checksum(P), "names": NAMES, "outputs": [rec(t, n=NSAMPLE) for t in picked]}
    torch.save(fx, OUT)
    print("wrote %s: %d bytes; shapes %s" % (OUT, os.path.getsize(OUT), [r["shape"] for r in fx["outputs"]]))


if __name__ == "__main__":
    main()
