"""Generates tests/golden/reference_multiscale.pt by running the REFERENCE's own ``predict_multiscale`` (networks/evaluate.py:
115-134, imported from where it lies through oracle/ref_import.load_reference_evaluate: nothing copied) with scipy's
``ndimage.zoom`` on seeded inputs.  Only runnable where the reference tree exists; the fixture travels.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_multiscale.py

Four small cases pin the resize and the tail: four scales with flip; a size whose 0.5 scale zeroes the last COLUMN and whose
0.75 scale zeroes the last ROW of the scaled image (scipy's ``mode='constant'`` with a last coordinate that rounds above
n - 1); odd scales without flip; one scale with flip.  The net is wrapped so that every forward's INPUT (scipy's output) and
LOGITS are recorded: the kernels and the numpy restatement (tests/multiscale_ref.py) are then fed the very numbers the
reference resized and up-sampled.  The end-to-end part wraps ``predict_multiscale`` so that the reference's
``evaluate_main(whole=True)`` (which hard-codes 1024 x 2048 and ``[1.0], False``) runs it with scales [0.75, 1.0, 1.25] and
flip on one seeded full-size image with ignore regions; 1024 rows at 0.75 is a zeroed-last-row size (row 767).

Before anything is written the generator checks the restatement against the reference on every pixel (bounds of the CPU
tests, see ``check_case``), so a fixture that violates them never exists.
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from oracle import abn_torch, ref_import  # noqa: E402
import multiscale_ref as M  # noqa: E402
from make_golden_sliding import FakeNet, case_image, sample_pixels  # noqa: E402

OUT = os.path.join(HERE, "reference_multiscale.pt")
MAX_BYTES = 1 << 20          # no committed file above 1 MiB
SAMPLES = 1280               # sampled pixels' probabilities per case (the generator itself checks EVERY pixel)
INPUT_SAMPLES = 256          # sampled values of the network's input per scale
# (name, H, W, classes, scales, flip, net seed, image seed)
CASES = [("ms4_flip", 64, 128, 19, [0.75, 1.0, 1.25, 1.5], True, 7, 5),
         ("zero_lines", 100, 56, 7, [0.5, 0.75, 1.0, 1.75], True, 8, 6),
         ("noflip_odd", 72, 104, 21, [0.6, 1.1, 1.75], False, 9, 7),
         ("single_flip", 40, 56, 5, [1.0], True, 10, 8)]
EVAL_SIZE = (1024, 2048)     # evaluate.py:161,170 hard-codes it
EVAL_SCALES = [0.75, 1.0, 1.25]
EVAL_NET_SEED, EVAL_IMAGE_SEED = 7, 31


class Recorder(torch.nn.Module):
    """Records every forward's input and logits (element 0 of the net's list)."""

    def __init__(self, net):
        super().__init__()
        self.net = net
        self.inputs, self.logits = [], []

    def forward(self, x):
        out = self.net(x)
        self.inputs.append(x.detach().cpu().clone())
        self.logits.append(out[0].detach().cpu().clone())
        return out


def eval_batch(seed=EVAL_IMAGE_SEED):
    """One full-size (image, label, size, name) batch with ignore regions, in the manner of make_golden_sliding.eval_batches."""
    g = torch.Generator().manual_seed(seed)
    h, w = EVAL_SIZE
    image = torch.randn(1, 3, h, w, generator=g) * 57.0
    label = torch.randint(0, 19, (1, h, w), generator=g).float()
    label[0, 110:340, :800] = 255
    label[0, -70:, -250:] = 255
    return image, label, torch.tensor([[h, w, 3]]), ["img0"]


def per_scale_logits(rec, n_scales, flip):
    """The recorded forwards as the list of (F, C, h_s, w_s) arrays the tail takes: [plain, mirrored] per scale."""
    f = 2 if flip else 1
    assert len(rec.logits) == n_scales * f, (len(rec.logits), n_scales, f)
    return [torch.cat(rec.logits[f * s:f * s + f]).contiguous() for s in range(n_scales)]


def check_inputs(name, image, scales, flip, rec):
    """The resize restatement equals scipy's output (the network's recorded input) value for value; returns per scale the
    sampled values and the zero-line flags."""
    f = 2 if flip else 1
    out = []
    _, _, H, W = image.shape
    for s, scale in enumerate(scales):
        Ho, Wo = M.zoom_size(H, scale), M.zoom_size(W, scale)
        x = rec.inputs[f * s][0].numpy()
        assert x.shape == (3, Ho, Wo) and x.dtype == np.float32, (name, scale, x.shape, (Ho, Wo))
        mine = M.zoom_linear(image[0].numpy(), Ho, Wo)
        assert np.array_equal(mine, x), (name, scale)
        if flip:
            assert np.array_equal(rec.inputs[f * s + 1][0].numpy(), x[:, :, ::-1]), (name, scale)
        row0, col0 = bool((x[:, -1, :] == 0).all()), bool((x[:, :, -1] == 0).all())
        assert (row0, col0) == (M.zero_lines(H, Ho), M.zero_lines(W, Wo)), (name, scale)
        idx = np.sort(np.random.RandomState(1000 + s).choice(x.size, size=min(INPUT_SAMPLES, x.size), replace=False)).astype(np.int64)
        out.append({"scale": float(scale), "size": (Ho, Wo), "index": torch.from_numpy(idx), "values": torch.from_numpy(x.reshape(-1)[idx].copy()),
                    "last_row_zero": row0, "last_col_zero": col0})
        print("  %-12s scale %.2f -> %3d x %3d  last row zero %s  last column zero %s" % (name, scale, Ho, Wo, row0, col0))
    return out


def check_case(name, logits, flip, H, W, ref_probs, ref_argmax):
    """The CPU-side conditions of tests/test_multiscale_eval_cpu.py on EVERY pixel: restatement within 2^-22 max|logit| of the
    reference's probabilities, at most 1e-5 pixels + 2 argmax disagreements."""
    probs, pred = M.multiscale([lg.numpy() for lg in logits], flip, (H, W))
    peak = max(float(lg.abs().max()) for lg in logits)
    err = float(np.abs(probs - ref_probs).max())
    flips = int((pred != ref_argmax).sum())
    print("%-12s scales %d  max|logit| %.2f  max|dprob| %.3e (bound %.3e)  argmax flips %d of %d"
          % (name, len(logits), peak, err, 2.0 ** -22 * peak, flips, H * W))
    assert err <= 2.0 ** -22 * peak, (name, err)
    assert flips <= 1e-5 * H * W + 2, (name, flips)
    return peak


def main():
    E = ref_import.load_reference_evaluate(abn_torch)
    G = {"cases": {}, "samples": SAMPLES}
    for name, H, W, classes, scales, flip, net_seed, img_seed in CASES:
        rec = Recorder(FakeNet(classes, net_seed).eval())
        image = case_image(H, W, img_seed)
        with ref_import.evaluate_shims(), torch.no_grad():
            ref_probs = E.predict_multiscale(rec, image, (H, W), scales, classes, flip, 1)
        assert ref_probs.shape == (H, W, classes) and ref_probs.dtype == np.float64
        inputs = check_inputs(name, image, scales, flip, rec)
        logits = per_scale_logits(rec, len(scales), flip)
        ref_argmax = np.asarray(np.argmax(ref_probs, axis=2), dtype=np.uint8)          # evaluate.py:187
        peak = check_case(name, logits, flip, H, W, ref_probs, ref_argmax)
        pix = sample_pixels(H, W, img_seed)
        G["cases"][name] = {"H": H, "W": W, "classes": classes, "scales": [float(v) for v in scales], "flip": flip, "net_seed": net_seed,
                            "image_seed": img_seed, "logits": logits, "inputs": inputs, "argmax": torch.from_numpy(ref_argmax),
                            "max_abs_logit": peak, "sample_pixels": torch.from_numpy(pix),
                            "sample_probs": torch.from_numpy(ref_probs.reshape(H * W, classes)[pix].copy())}
    zl = G["cases"]["zero_lines"]["inputs"]
    assert zl[0]["last_col_zero"] and zl[1]["last_row_zero"], "the zero_lines case must hold a zeroed column and a zeroed row"

    # end to end: the reference's evaluate_main(whole=True) with predict_multiscale wrapped to the scales and the flip
    rec = Recorder(FakeNet(19, EVAL_NET_SEED).eval())
    seen, per_image = [], []
    orig_ms, orig_cm = E.predict_multiscale, E.get_confusion_matrix

    def wrapped(net, image, tile_size, scales, classes, flip, recurrence):
        out = orig_ms(net, image, tile_size, EVAL_SCALES, classes, True, recurrence)
        seen.append(out)
        return out

    E.predict_multiscale = wrapped
    E.get_confusion_matrix = lambda *a: per_image.append(orig_cm(*a)) or per_image[-1]
    cwd = os.getcwd()
    batch = eval_batch()
    try:
        with tempfile.TemporaryDirectory() as d, ref_import.evaluate_shims():
            os.chdir(d)                                   # evaluate.py:172-173,191 writes outputs/<name>.png
            mean_iu, iu = E.evaluate_main(rec, [batch], "0", "512,512", 19, True)
    finally:
        os.chdir(cwd)
        E.predict_multiscale, E.get_confusion_matrix = orig_ms, orig_cm
    assert len(seen) == 1 and len(per_image) == 1 and seen[0].shape == EVAL_SIZE + (19,)
    H, W = EVAL_SIZE
    x075 = rec.inputs[0][0].numpy()
    assert x075.shape == (3, 768, 1536) and (x075[:, 767, :] == 0).all() and not (x075[:, 766, :] == 0).all(), "row 767 is zeroed"
    assert np.array_equal(M.zoom_linear(batch[0][0].numpy(), 768, 1536), x075)
    logits = per_scale_logits(rec, len(EVAL_SCALES), True)
    check_case("full-size", logits, True, H, W, seen[0], np.asarray(np.argmax(seen[0], axis=2), dtype=np.uint8))
    G["evaluate_main"] = {"net_seed": EVAL_NET_SEED, "image_seed": EVAL_IMAGE_SEED, "size": EVAL_SIZE, "scales": list(EVAL_SCALES),
                          "flip": True, "mean_IU": float(mean_iu), "IU_array": torch.from_numpy(np.asarray(iu)),
                          "confusion": torch.from_numpy(per_image[0]), "last_row_zero_at_075": True}
    torch.save(G, OUT)
    size = os.path.getsize(OUT)
    print("wrote", OUT, size, "bytes; mean IU", mean_iu)
    if size >= MAX_BYTES:
        os.remove(OUT)
        raise AssertionError("fixture of %d bytes: the limit is %d" % (size, MAX_BYTES))


if __name__ == "__main__":
    main()
