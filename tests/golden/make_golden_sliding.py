"""Generates tests/golden/reference_sliding.pt by running the REFERENCE's own networks/evaluate.py (imported from where it
lies through oracle/ref_import.load_reference_evaluate: cv2 / torchvision stubbed, nothing copied) on seeded inputs.  Only
runnable where the reference tree exists; the fixture travels.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sliding.py

Pins ``predict_sliding`` (evaluate.py:70-104) on four geometries -- landscape with 18 tiles, an image lower than the tile
(zero padding), a portrait image (x-origin clamp), a non-square tile with a six-fold overlap -- scaled down from the
Cityscapes sizes so that the recorded tile logits fit a small file; ``evaluate_main(whole=False)`` (evaluate.py:156-206) over
two images of different sizes that are no multiple of the tile, with ignore regions; the trainId -> id remap of
``id2trainId(reverse=True)`` and ``get_palette(256)``.  The net is wrapped so that EACH TILE'S LOGITS are recorded: the
kernel and the numpy restatement (tests/sliding_ref.py) are then fed the very numbers the reference up-sampled, and only
the tail is compared.  The class count varies over the geometries (19, 7, 5, 21): it keeps the sampled float64
probabilities small and walks the kernel's compile-time class bounds.

Before anything is written the generator checks the restatement against the reference on every pixel (bounds of the
CPU tests, see ``check_case``), so a fixture that violates them never exists.
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
from oracle import abn_torch, ref_import  # noqa: E402
import sliding_ref as R  # noqa: E402

OUT = os.path.join(HERE, "reference_sliding.pt")
MAX_BYTES = 1 << 20          # no committed file above 1 MiB
SAMPLES = 1280               # per case: 5120 sampled pixels over the four cases (the generator itself checks EVERY pixel)
# (name, H, W, tile, classes, net seed, image seed): an eighth of (1024, 2048, 512^2) and a quarter of (400, 1000, 512^2),
# (700, 520, 512^2), (513, 771, 256 x 384) -- the tile counts 18 / 3 / 4 / 12 are those of the full sizes
CASES = [("landscape18", 128, 256, (64, 64), 19, 7, 21),
         ("padded_rows", 100, 250, (128, 128), 7, 8, 22),
         ("portrait", 175, 130, (128, 128), 5, 9, 23),
         ("nonsquare_overlap6", 129, 193, (64, 96), 21, 10, 24)]
TILE_COUNTS = {"landscape18": 18, "padded_rows": 3, "portrait": 4, "nonsquare_overlap6": 12}
# evaluate_main stores matrices only (the inputs are seeded), so its images are full-sized: ~1e5 scored pixels per class keep
# one near-tie flip (the conv library differs between hosts) well inside the per-class IoU bound of the tests
EVAL_TILE = "512,512"
EVAL_SIZES = ((1000, 2000), (1500, 1300))


class FakeNet(torch.nn.Module):
    """3 -> ``classes`` channels, 8 x 8 stride-8 convolution with seeded weights, returned as a list like Res_pspnet.forward
    (evaluate.py:96-97 takes element 0).  ``record`` collects every forward's logits."""

    def __init__(self, classes=19, seed=7):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.conv = torch.nn.Conv2d(3, classes, 8, 8)
        with torch.no_grad():
            self.conv.weight.copy_(torch.randn(classes, 3, 8, 8, generator=g) * 0.02)
            self.conv.bias.copy_(torch.randn(classes, generator=g) * 0.5)
        self.record = None

    def forward(self, x):
        y = self.conv(x)
        if self.record is not None:
            self.record.append((tuple(x.shape), y.detach().cpu().clone()))
        return [y, y]


def case_image(H, W, seed):
    return torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(seed)) * 57.0


def sample_pixels(H, W, seed):
    return np.sort(np.random.RandomState(seed).choice(H * W, size=min(SAMPLES, H * W), replace=False)).astype(np.int32)


def eval_batches(seed=11):
    """Two (image, label, size, name) batches of different sizes; evaluate.py:194-197 masks the full-size prediction with the
    cropped label, so ``size`` is the image's own size."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, (h, w) in enumerate(EVAL_SIZES):
        image = torch.randn(1, 3, h, w, generator=g) * 57.0
        label = torch.randint(0, 19, (1, h, w), generator=g).float()
        label[0, 10 + 100 * i:40 + 300 * i, :300 + 500 * i] = 255
        label[0, -70:, -(50 + 200 * i):] = 255
        out.append((image, label, torch.tensor([[h, w, 3]]), ["img%d" % i]))
    return out


def check_case(name, logits, tiles, tile, H, W, ref_probs, ref_argmax):
    """The CPU-side conditions of tests/test_sliding_eval_cpu.py on EVERY pixel: restatement within 2^-22 max|logit| of the
    reference's probabilities, at most 1e-5 pixels + 2 argmax disagreements."""
    probs, pred = R.sliding(logits, tiles, tile, (H, W))
    peak = float(np.abs(logits).max())
    err = float(np.abs(probs - ref_probs).max())
    flips = int((pred != ref_argmax).sum())
    print("%-20s tiles %2d  max|logit| %.2f  max|dprob| %.3e (bound %.3e)  argmax flips %d of %d"
          % (name, len(tiles), peak, err, 2.0 ** -22 * peak, flips, H * W))
    assert err <= 2.0 ** -22 * peak, (name, err)
    assert flips <= 1e-5 * H * W + 2, (name, flips)
    return peak


def main():
    E = ref_import.load_reference_evaluate(abn_torch)
    G = {"cases": {}, "samples": SAMPLES}
    deepest = 0
    for name, H, W, tile, classes, net_seed, img_seed in CASES:
        net = FakeNet(classes, net_seed).eval()
        net.record = []
        with ref_import.evaluate_shims(), torch.no_grad():
            ref_probs = E.predict_sliding(net, case_image(H, W, img_seed).numpy(), tile, classes, False, 1)
        shapes = [s for s, _ in net.record]
        logits = torch.cat([y for _, y in net.record]).contiguous()
        tiles = R.tiles_of(H, W, tile)
        assert len(tiles) == len(shapes) == TILE_COUNTS[name], (name, len(tiles), len(shapes))
        assert all(s == (1, 3) + tuple(tile) for s in shapes), shapes
        assert ref_probs.shape == (H, W, classes) and ref_probs.dtype == np.float64
        ref_argmax = np.asarray(np.argmax(ref_probs, axis=2), dtype=np.uint8)          # evaluate.py:187
        peak = check_case(name, logits.numpy(), tiles, tile, H, W, ref_probs, ref_argmax)
        deepest = max(deepest, int(R.cover_count(H, W, tiles).max()))
        pix = sample_pixels(H, W, img_seed)
        G["cases"][name] = {"H": H, "W": W, "tile": tuple(tile), "classes": classes, "net_seed": net_seed, "image_seed": img_seed,
                            "n_tiles": len(tiles), "tile_input_shapes": shapes, "logits": logits,
                            "argmax": torch.from_numpy(ref_argmax), "max_abs_logit": peak,
                            "sample_pixels": torch.from_numpy(pix), "sample_probs": torch.from_numpy(ref_probs.reshape(H * W, classes)[pix].copy())}
    assert deepest >= 6, deepest
    assert any(c["H"] < c["tile"][0] for c in G["cases"].values()) and any(c["W"] < c["H"] for c in G["cases"].values())
    assert any(c["tile"][0] != c["tile"][1] for c in G["cases"].values())

    per_image = []
    orig = E.get_confusion_matrix
    E.get_confusion_matrix = lambda *a: per_image.append(orig(*a)) or per_image[-1]
    cwd = os.getcwd()
    try:
        with tempfile.TemporaryDirectory() as d, ref_import.evaluate_shims():
            os.chdir(d)                                   # evaluate.py:172-173,191 writes outputs/<name>.png
            mean_iu, iu = E.evaluate_main(FakeNet(19, 7), eval_batches(), "0", EVAL_TILE, 19, False)
    finally:
        os.chdir(cwd)
        E.get_confusion_matrix = orig
    assert len(per_image) == len(EVAL_SIZES)
    G["evaluate_main"] = {"net_seed": 7, "batch_seed": 11, "tile": EVAL_TILE, "sizes": EVAL_SIZES, "mean_IU": float(mean_iu),
                          "IU_array": torch.from_numpy(np.asarray(iu)), "confusion_per_image": [torch.from_numpy(c) for c in per_image]}
    G["trainid_to_id"] = torch.from_numpy(E.id2trainId(np.arange(19, dtype=np.int64), E.id_to_trainid, reverse=True))
    G["palette256"] = [int(v) for v in E.get_palette(256)]
    torch.save(G, OUT)
    size = os.path.getsize(OUT)
    print("wrote", OUT, size, "bytes; mean IU", mean_iu)
    if size >= MAX_BYTES:
        os.remove(OUT)
        raise AssertionError("fixture of %d bytes: the limit is %d" % (size, MAX_BYTES))


if __name__ == "__main__":
    main()
