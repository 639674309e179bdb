"""Generates tests/golden/reference_ohem.pt by running the REFERENCE's own ``OhemCrossEntropy2d`` and ``CriterionOhemDSN``
(utils/criterion.py:11-90, 190-209, imported from where they lie through oracle/ref_import.load_reference: nothing copied) with
scipy's ``ndimage.zoom`` and ``np.partition`` on seeded inputs.  Only runnable where the reference tree exists; the fixture
(inputs, seeds and recorded results) travels.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ohem.py

Inputs: a random low-resolution label field; logits ``randn * 2`` plus a margin of 8-10 on the field's class; the target is the
nearest-upsampled field with 2 % random flips and a band of 255.  Confident pixels sit near probability 1, flipped ones near
0, the pixels along the field's edges in between -- so the k-th smallest down-sampled probability, ``thresh`` and 1.0 each
become the threshold for some case below.  The generator ASSERTS which branch each case took (``CASES``), that all three
occur, and that 256 -> 32 zeroes the last down-sampled row and column.

Before anything is written it checks the restatement (tests/ohem_ref.py) against the reference on every case:
  * fed the reference's own fp32 softmax, the restatement reproduces the threshold and the kept mask EXACTLY and the loss and
    both gradients to 1e-6 (relative);
  * ``eps32`` = max |p_fp32(reference) - p_float64(restatement)| over every valid pixel of every case is measured, and
    ``tau = 4 * eps32`` stored: the distance within which an fp32 evaluation other than the reference's (the kernels') may put
    a pixel on the other side of the threshold -- one rounding noise for its own ``exp``, one for a k-th value that is itself
    such a probability, times two;
  * at most 0.1 % of a case's valid pixels lie within ``tau`` of its threshold (their count is stored as ``near``);
  * on its own float64 path the restatement lands within ``tau`` of the threshold and agrees on every pixel farther than ``tau``
    from it.
"""
import inspect
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import abn_torch, ref_import  # noqa: E402
import ohem_ref as R  # noqa: E402

OUT = os.path.join(HERE, "reference_ohem.pt")
MAX_BYTES = 1 << 20          # no committed file above 1 MiB
IGNORE = 255
# name, (B, C, h, w), (H, W), thresh, min_kept, factor, two heads, seed, the branch find_threshold must take
CASES = [
    ("kth", (2, 19, 9, 17), (64, 128), 0.2, 9600, 8, True, 11, "kth"),
    ("thresh", (2, 19, 9, 17), (64, 128), 0.7, 6400, 8, True, 11, "thresh"),
    ("all_kept", (2, 19, 9, 17), (64, 128), 0.7, 100000, 8, True, 11, "one"),
    ("zero_lines", (1, 7, 33, 33), (256, 256), 0.2, 38400, 8, True, 12, "kth"),
    ("half_even", (3, 11, 14, 10), (100, 72), 0.3, 12800, 8, True, 13, "kth"),
    ("one_row", (1, 5, 5, 7), (40, 56), 0.7, 100000, 4, True, 14, "one"),
    ("single_head", (1, 5, 24, 32), (24, 32), 0.5, 256, 8, False, 15, None),
]


def make_inputs(shape, size, seed, one_row=False):
    B, C, h, w = shape
    H, W = size
    g = torch.Generator().manual_seed(seed)
    field = torch.randint(0, C, (B, h, w), generator=g)
    margin = 8.0 + 2.0 * torch.rand((B, 1, h, w), generator=g)

    def logits():
        return (torch.randn((B, C, h, w), generator=g) * 2.0
                + margin * F.one_hot(field, C).permute(0, 3, 1, 2).float()).contiguous()
    lm, ld = logits(), logits()
    target = F.interpolate(field[:, None].float(), size=(H, W), mode="nearest")[:, 0].long()
    flip = torch.rand((B, H, W), generator=g) < 0.02
    target = torch.where(flip, torch.randint(0, C, (B, H, W), generator=g), target)
    band = max(2, H // 10)
    target[:, H // 3:H // 3 + band, :] = IGNORE
    if one_row:                                   # every pixel ignored except one row (one the order-0 zoom samples)
        keep = target[:, 17].clone()
        target[:] = IGNORE
        target[:, 17] = keep
    return lm, ld, target.contiguous()


def run_reference(ns, case):
    name, shape, size, thresh, min_kept, factor, two, seed, _ = case
    lm, ld, target = make_inputs(shape, size, seed, one_row=(name == "one_row"))
    lm_r, ld_r = lm.clone().requires_grad_(True), ld.clone().requires_grad_(True)
    with ref_import.cpu_cuda_identity():
        if two:
            crit = ns.criterion.CriterionOhemDSN(IGNORE, thresh, min_kept)
            ohem = crit.criterion1
            ohem.factor = factor
            loss = crit([lm_r, ld_r], target)
        else:
            crit = ohem = ns.criterion.OhemCrossEntropy2d(IGNORE, thresh, min_kept, factor)
            loss = crit(lm_r, target)
        loss.backward()
        # the intermediate results, by the reference's own methods on the tensors its forward builds
        with torch.no_grad():
            up = F.interpolate(lm, size=size, mode="bilinear", align_corners=True) if two else lm
            prob = F.softmax(up, 1)
            threshold = ohem.find_threshold(prob.numpy(), target.numpy())
            new_target = ohem.generate_new_target(prob, target)
    return dict(name=name, shape=shape, size=size, thresh=thresh, min_kept=min_kept, factor=factor, two=two, seed=seed,
                logits_main=lm, logits_dsn=ld if two else None, target=target, prob=prob.numpy(),
                threshold=np.float32(threshold), kept=(new_target != IGNORE).numpy(), loss=float(loss),
                grad_main=lm_r.grad.clone(), grad_dsn=ld_r.grad.clone() if two else None)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def branch_of(r, th):
    if th == np.float32(1.0):
        return "one"
    return "thresh" if th == np.float32(r["thresh"]) else "kth"


def main():
    assert ref_import.reference_available(), "the reference tree is needed to generate this fixture"
    ns = ref_import.load_reference(abn_torch)
    runs = [run_reference(ns, c) for c in CASES]
    eps32 = 0.0
    for r in runs:
        dsn = None if r["logits_dsn"] is None else r["logits_dsn"].numpy()
        args = (r["logits_main"].numpy(), dsn, r["target"].numpy(), IGNORE, r["thresh"], r["min_kept"], r["factor"], 0.4)
        exact = R.ohem(*args, probs32=r["prob"])
        assert exact.threshold == r["threshold"], (r["name"], exact.threshold, r["threshold"])
        assert np.array_equal(exact.kept, r["kept"]), r["name"]
        assert abs(exact.loss - r["loss"]) <= 1e-6 * abs(r["loss"]), (r["name"], exact.loss, r["loss"])
        assert rel(exact.grad_main, r["grad_main"].numpy()) <= 1e-6, r["name"]
        if dsn is not None:
            assert rel(exact.grad_dsn, r["grad_dsn"].numpy()) <= 1e-6, r["name"]
        own = R.ohem(*args)
        valid = r["target"].numpy() != IGNORE
        eps32 = max(eps32, float(np.abs(exact.p_label - own.p_label)[valid].max()))
        r["own"], r["valid"], r["num_valid"], r["pred_ds"] = own, valid, exact.num_valid, exact.pred_ds
    tau = 4.0 * eps32
    print("eps32 = %.3e   tau = %.3e" % (eps32, tau))
    branches = set()
    for r, c in zip(runs, CASES):
        own, valid, th = r["own"], r["valid"], float(r["threshold"])
        near = valid & (np.abs(own.p_label - th) <= tau)
        r["near"] = int(near.sum())
        r["branch"] = branch_of(r, r["threshold"])
        branches.add(r["branch"])
        print("%-12s threshold %.7f (%s)  num_valid %d  kept %d of %d valid  near %d  loss %.6f" % (
            r["name"], th, r["branch"], r["num_valid"], int(r["kept"].sum()), int(valid.sum()), r["near"], r["loss"]))
        assert c[8] is None or r["branch"] == c[8], (r["name"], r["branch"], c[8])
        assert r["near"] <= 1e-3 * valid.sum(), (r["name"], r["near"], int(valid.sum()))
        assert abs(float(own.threshold) - th) <= tau, (r["name"], own.threshold, th)
        assert np.array_equal(own.own_kept[~near], r["kept"][~near]), r["name"]
        if r["name"] == "zero_lines":
            keys = r["pred_ds"]
            assert (keys[:, -1, :] == 0).all() and (keys[:, :, -1] == 0).all() and (keys[:, :-1, :-1] != 0).any()
    assert branches == {"kth", "thresh", "one"}, branches
    crit = ns.criterion
    fixture = {
        "tau": tau, "eps32": eps32, "ignore_index": IGNORE,
        "signatures": {"OhemCrossEntropy2d": str(inspect.signature(crit.OhemCrossEntropy2d.__init__)),
                       "CriterionOhemDSN": str(inspect.signature(crit.CriterionOhemDSN.__init__))},
        "cases": [dict(name=r["name"], shape=r["shape"], size=r["size"], thresh=r["thresh"], min_kept=r["min_kept"],
                       factor=r["factor"], two=r["two"], seed=r["seed"], branch=r["branch"], near=r["near"],
                       num_valid=r["num_valid"], logits_main=r["logits_main"], logits_dsn=r["logits_dsn"],
                       target=r["target"].to(torch.uint8), threshold=float(r["threshold"]),
                       kept_bits=torch.from_numpy(np.packbits(r["kept"])), n_kept=int(r["kept"].sum()), loss=r["loss"],
                       grad_main=r["grad_main"], grad_dsn=r["grad_dsn"]) for r in runs]}
    torch.save(fixture, OUT)
    size = os.path.getsize(OUT)
    assert size <= MAX_BYTES, size
    print("wrote %s (%d bytes)" % (OUT, size))


if __name__ == "__main__":
    main()
