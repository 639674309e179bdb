"""Sliding-window evaluation and the test-split prediction dump, host side (no GPU): tests/golden/reference_sliding.pt was
written by tests/golden/make_golden_sliding.py from the REFERENCE's own ``predict_sliding`` / ``evaluate_main(whole=False)``
/ ``id2trainId`` / ``get_palette`` with every tile's logits recorded.  Checked against it: the product's tile arithmetic,
the numpy restatement of the tail (tests/sliding_ref.py, the bit-exact yardstick of the HIP kernel on the GPU), and
``evaluate_main(whole=False)`` end to end through a composite double (the plain-C double of oracle/ for the core entries +
the restatement as ``skd_seg_sliding``).  The plain-C double alone has no ``skd_seg_sliding``: NotImplementedError.

Bounds: probabilities within 2^-22 max|logit| of the reference's (one fp32 ulp of the interpolated value each way: the
reference's CPU upsample rounds the four-term sum differently); argmax disagreements at most 1e-5 pixels + 2 per case (the
near-tie cap of tests/test_eval_golden.py; the generator measured 0); evaluate_main: the bounds of tests/test_eval_golden.py."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from oracle import cref
from structure_knowledge_distillation_amd import _lib
from structure_knowledge_distillation_amd import functional as SF
from structure_knowledge_distillation_amd.networks import evaluate as E

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIR = os.path.join(HERE, "golden")
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import sliding_ref as R  # noqa: E402


def gen():
    spec = importlib.util.spec_from_file_location("make_golden_sliding", os.path.join(GOLDEN_DIR, "make_golden_sliding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def gold():
    return torch.load(os.path.join(GOLDEN_DIR, "reference_sliding.pt"), weights_only=False)


class backend:
    """Install a test back-end for the duration of a block and put back whatever was there."""

    def __init__(self, b):
        self.b = b

    def __enter__(self):
        self.prev = _lib._test_backend
        _lib.install_test_backend(self.b)
        return self.b

    def __exit__(self, *exc):
        _lib.install_test_backend(self.prev)
        return False


def c_double():
    return cref.load(_lib.SIGNATURES)


# ---- 1. tile arithmetic ---------------------------------------------------------------------------------------------

FULL_SIZE = [(1024, 2048, (512, 512), 18), (400, 1000, (512, 512), 3), (700, 520, (512, 512), 4), (513, 771, (256, 384), 12)]
DEGENERATE = [(512, 512, (512, 512), 1), (100, 90, (128, 128), 1), (513, 512, (512, 512), 2), (512, 513, (512, 512), 2),
              (129, 193, (64, 96), 12)]


def test_sliding_tiles_vs_fixture_and_cover_count():
    G = gold()
    for name, c in G["cases"].items():
        tiles = E.sliding_tiles(c["H"], c["W"], c["tile"])
        assert len(tiles) == c["n_tiles"] == len(c["tile_input_shapes"]), name
        assert all(tuple(s) == (1, 3) + tuple(c["tile"]) for s in c["tile_input_shapes"]), name
        assert tiles == R.tiles_of(c["H"], c["W"], c["tile"]), name
    deepest = 0
    for H, W, tile, n in FULL_SIZE + DEGENERATE:
        tiles = E.sliding_tiles(H, W, tile)
        assert len(tiles) == n, (H, W, tile, len(tiles))
        for y1, x1, y2, x2 in tiles:
            assert 0 <= y1 < y2 <= H and 0 <= x1 < x2 <= W and y2 - y1 == min(tile[0], H) and x2 - x1 == min(tile[1], W)
        mine = np.zeros((H, W), dtype=np.int64)
        for y1, x1, y2, x2 in tiles:
            mine[y1:y2, x1:x2] += 1
        want = R.cover_count(H, W, R.tiles_of(H, W, tile))
        assert np.array_equal(mine, want) and mine.min() >= 1, (H, W, tile)
        deepest = max(deepest, int(mine.max()))
    assert deepest >= 6
    # the reference's formula yields NO tile (and 0 / 0) once the image is a whole stride smaller than the tile: one padded tile
    assert R.tiles_of(1, 1, (4, 4)) == [] and E.sliding_tiles(1, 1, (4, 4)) == [(0, 0, 1, 1)]
    with pytest.raises(ValueError):
        E.sliding_tiles(0, 5, (4, 4))


# ---- 2. restatement vs the reference's recorded outputs --------------------------------------------------------------

def test_restatement_vs_reference_fixture():
    G = gold()
    assert sum(len(c["sample_pixels"]) for c in G["cases"].values()) >= 4096
    for name, c in G["cases"].items():
        H, W, C = c["H"], c["W"], c["classes"]
        logits = c["logits"].numpy()
        assert abs(float(np.abs(logits).max()) - c["max_abs_logit"]) == 0.0
        probs, pred = R.sliding(logits, R.tiles_of(H, W, c["tile"]), c["tile"], (H, W))
        pix = c["sample_pixels"].numpy().astype(np.int64)
        err = float(np.abs(probs.reshape(H * W, C)[pix] - c["sample_probs"].numpy()).max())
        flips = int((pred != c["argmax"].numpy()).sum())
        print("%s: max|dprob| %.3e (bound %.3e), argmax flips %d of %d" % (name, err, 2.0 ** -22 * c["max_abs_logit"], flips, H * W))
        assert err <= 2.0 ** -22 * c["max_abs_logit"], name
        assert flips <= 1e-5 * H * W + 2, name


# ---- 3. evaluate_main(whole=False) end to end through the composite double -----------------------------------------

def check_evaluate_main(device, G, mod, **kw):
    """Runs evaluate_main(whole=False) per image and over both; asserts the fixture's bounds; returns the per-image matrices."""
    ev = G["evaluate_main"]
    net = mod.FakeNet(19, ev["net_seed"]).to(device)
    mats = []
    for batch, want in zip(mod.eval_batches(ev["batch_seed"]), ev["confusion_per_image"]):
        seen = []
        orig = E.iou_from_confusion
        E.iou_from_confusion = lambda cm: seen.append(np.array(cm)) or orig(cm)
        try:
            m, iu = E.evaluate_main(net, [batch], "0", ev["tile"], 19, whole=False, **kw)
        finally:
            E.iou_from_confusion = orig
        cm, want = seen[0], want.numpy()
        diff = np.abs(cm - want).sum() / 2                    # a flipped pixel moves one count
        print("confusion vs the reference's: %d of %d scored pixels differ" % (diff, want.sum()))
        assert cm.sum() == want.sum(), "same number of scored pixels (ignore mask, evaluate.py:195-197)"
        assert diff <= 1e-5 * want.sum() + 2
        wm, wiu = E.iou_from_confusion(want)
        assert np.abs(np.asarray(iu) - wiu).max() <= 2e-5 and abs(m - wm) <= 2e-5
        mats.append(cm)
    mean_iu, iu = E.evaluate_main(net, mod.eval_batches(ev["batch_seed"]), "0", ev["tile"], 19, whole=False, **kw)
    assert abs(mean_iu - ev["mean_IU"]) <= 5e-4 * ev["mean_IU"] + 1e-6, (mean_iu, ev["mean_IU"])
    assert np.abs(np.asarray(iu) - ev["IU_array"].numpy()).max() <= 2e-5
    return mats


def test_evaluate_main_sliding_vs_reference_fixture_through_composite_double():
    G, mod = gold(), gen()
    assert [tuple(s) for s in G["evaluate_main"]["sizes"]] == [tuple(s) for s in mod.EVAL_SIZES]
    double = R.SlidingDouble(c_double())
    with backend(double):
        check_evaluate_main(torch.device("cpu"), G, mod)
    assert double.calls == 2 * len(mod.EVAL_SIZES), "one fused call per image"


def test_predict_sliding_and_tile_batch_through_composite_double():
    mod = gen()
    name, H, W, tile, classes, net_seed, img_seed = mod.CASES[3]
    c = gold()["cases"][name]
    net = mod.FakeNet(classes, net_seed)
    image = mod.case_image(H, W, img_seed)
    with backend(R.SlidingDouble(c_double())):
        probs = E.predict_sliding(net, image.numpy(), tile, classes, flip_evaluation=True, recurrence=3)
        one = E.predict_sliding(net, image, tile, classes, tile_batch=1)
        with pytest.raises(ValueError):
            E.predict_sliding(net, image, tile, classes + 1)
    assert isinstance(probs, np.ndarray) and probs.shape == (H, W, classes) and probs.dtype == np.float64
    pix = c["sample_pixels"].numpy().astype(np.int64)
    # same host, same conv library as the generator's run unless the fixture travelled: the logits' own rounding is the slack
    assert np.abs(probs.reshape(H * W, classes)[pix] - c["sample_probs"].numpy()).max() <= 2.0 ** -22 * c["max_abs_logit"] + 1e-4
    assert np.abs(one - probs).max() <= 1e-4, "tile_batch only changes how the forwards are batched"
    assert (probs.argmax(2) != c["argmax"].numpy()).sum() <= 1e-5 * H * W + 2


# ---- 4. back-end without the entry point ---------------------------------------------------------------------------

def test_plain_c_double_has_no_sliding_entry():
    class Exploding(torch.nn.Module):
        def forward(self, x):
            raise AssertionError("the model must not be touched")

    def loader():
        raise AssertionError("the loader must not be touched")
        yield

    with backend(c_double()):
        assert not _lib.has_entry("skd_seg_sliding")
        with pytest.raises(NotImplementedError, match="skd_seg_sliding"):
            E.evaluate_main(Exploding(), loader(), "0", "512,512", 19, whole=False)
        with pytest.raises(NotImplementedError, match="skd_seg_sliding"):
            E.evaluate_main(Exploding(), loader(), "0", "512,512", 19)          # the default IS whole=False
        with pytest.raises(NotImplementedError, match="skd_seg_sliding"):
            E.predict_sliding(Exploding(), np.zeros((1, 3, 8, 8), np.float32), (4, 4), 19)
        with pytest.raises(NotImplementedError, match="skd_seg_sliding"):
            SF.seg_sliding(torch.zeros(1, 2, 2, 2), [(0, 0, 4, 4)], (4, 4), (4, 4))


def test_seg_sliding_argument_checks():
    with backend(R.SlidingDouble(c_double())):
        lg = torch.zeros(1, 3, 2, 2)
        with pytest.raises(TypeError):
            SF.seg_sliding(lg.double(), [(0, 0, 4, 4)], (4, 4), (4, 4))
        with pytest.raises(TypeError):
            SF.seg_sliding(lg, [(0, 0, 4, 4)], (4, 4), (4, 4), target=torch.zeros(4, 4, dtype=torch.int32))
        with pytest.raises(ValueError):
            SF.seg_sliding(lg, [(0, 0, 5, 4)], (4, 4), (4, 4))                # window outside the image
        with pytest.raises(ValueError):
            SF.seg_sliding(lg, [(0, 0, 4, 4), (0, 0, 4, 4)], (4, 4), (4, 4))  # two windows, one logit map
        with pytest.raises(ValueError):
            SF.seg_sliding(torch.zeros(1, 33, 2, 2), [(0, 0, 4, 4)], (4, 4), (4, 4))
        with pytest.raises(TypeError):
            SF.seg_sliding(lg, [(0, 0, 4, 4)], (4, 4), (4, 4), remap=torch.zeros(19, dtype=torch.uint8))
        pred, probs, cm = SF.seg_sliding(lg, [(0, 0, 4, 4)], (4, 4), (4, 4), target=torch.ones(4, 4, dtype=torch.int64), want_probs=True)
        assert pred.dtype == torch.uint8 and int(pred.sum()) == 0 and probs.shape == (4, 4, 3) and int(cm[1, 0]) == 16


# ---- 5. test split: remap, palette, PNG -----------------------------------------------------------------------------

def test_remap_table_palette_and_id2trainid_vs_reference_fixture():
    G = gold()
    want = G["trainid_to_id"].numpy()
    assert list(want) == [7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33]
    table = E.trainid_to_id_table()
    assert table.dtype == np.uint8 and table.shape == (256,) and np.array_equal(table[:19], want)
    assert np.array_equal(table[19:255], np.arange(19, 255)), "values the table does not name are kept"
    assert np.array_equal(E.id2trainId(np.arange(19, dtype=np.int64), E.id_to_trainid, reverse=True), want)
    assert np.array_equal(E.id2trainId(np.arange(19, dtype=np.uint8), E.id_to_trainid, reverse=True), want)   # the reference raises here
    ids = np.arange(-1, 40, dtype=np.int64)
    fwd = E.id2trainId(ids, E.id_to_trainid)
    for i, v in zip(ids, fwd):
        assert v == E.id_to_trainid.get(int(i), int(i))
    assert np.array_equal(E.id2trainId(want, E.id_to_trainid), np.arange(19))
    assert E.get_palette(256) == list(G["palette256"]) and len(E.get_palette(256)) == 768
    assert E.get_palette(3) == [0, 0, 0, 128, 0, 0, 0, 128, 0]
    img = np.arange(24, dtype=np.float32).reshape(1, 2, 3, 4)
    padded = E.pad_image(img, (5, 6))
    assert padded.shape == (1, 2, 5, 6) and np.array_equal(padded[:, :, :3, :4], img) and padded[:, :, 3:].sum() == 0 and padded[..., 4:].sum() == 0


def read_png(path):
    from PIL import Image
    im = Image.open(path)
    return im.mode, list(im.getpalette()), np.array(im)


def check_test_split(device, whole, tmp_path, mod):
    """type='test' writes <outputs>/<name>.png = remap[pred] in mode P with get_palette(256); returns None."""
    net = mod.FakeNet(19, 7).to(device)
    batches = [(b[0], b[2], ["sub/%s_%d" % (b[3][0], int(whole))]) for b in mod.eval_batches(11)]
    batches = [(im[:, :, :300, :420], size, name) for im, size, name in batches]
    out = str(tmp_path / ("test_%d" % whole))
    assert E.evaluate_main(net, batches, "0", "128,192", 19, whole=whole, type="test", outputs=out) is None
    table = E.trainid_to_id_table()
    for image, _, name in batches:
        with torch.no_grad():
            if whole:
                pred, _ = SF.seg_confusion(net(image.to(device))[0], None, 255, None, want_pred=tuple(image.shape[2:]))
                pred = pred[0]
            else:
                tiles = E.sliding_tiles(300, 420, (128, 192))
                # the same batched forward as evaluate_main's, so that the logits carry the same bits on any conv library
                logits = E._tile_logits(net, image.to(device), tiles, (128, 192), False, None)
                assert logits.shape[0] == len(tiles) == 12
                pred, _, _ = SF.seg_sliding(logits, tiles, (128, 192), (300, 420))
        mode, palette, pixels = read_png(os.path.join(out, name[0] + ".png"))
        assert mode == "P" and palette == E.get_palette(256)
        assert pixels.shape == (300, 420) and np.array_equal(pixels, table[pred.cpu().numpy()])
        assert set(np.unique(pixels)) <= set(table[:19].tolist())


@pytest.mark.parametrize("whole", [True, False])
def test_test_split_writes_remapped_palette_png(whole, tmp_path):
    with backend(R.SlidingDouble(c_double())):
        check_test_split(torch.device("cpu"), whole, tmp_path, gen())


def test_test_split_defaults_to_outputs_folder_and_val_writes_nothing(tmp_path, monkeypatch):
    mod = gen()
    monkeypatch.chdir(tmp_path)
    net = mod.FakeNet(19, 7)
    val = [(b[0][:, :, :64, :96], b[1][:, :64, :96], torch.tensor([[64, 96, 3]]), b[3]) for b in mod.eval_batches(11)]
    with backend(c_double()):                                  # whole-image dump needs no extension entry
        res = E.evaluate_main(net, val, "0", "512,512", 19, whole=True)
        assert os.listdir(str(tmp_path)) == [], "type='val' without outputs writes no file"
        again = E.evaluate_main(net, val, "0", "512,512", 19, whole=True, outputs=str(tmp_path / "dump"))
        assert res[0] == again[0] and np.array_equal(res[1], again[1])
        assert sorted(os.listdir(str(tmp_path / "dump"))) == ["img0.png", "img1.png"]
        with torch.no_grad():
            pred, _ = SF.seg_confusion(net(val[0][0])[0], None, 255, None, want_pred=(64, 96))
        assert np.array_equal(read_png(str(tmp_path / "dump" / "img0.png"))[2], pred[0].numpy()), "validation dumps are not remapped"
        assert E.evaluate_main(net, [(b[0], b[2], b[3]) for b in val], "0", "512,512", 19, whole=True, type="test") is None
        assert sorted(os.listdir(str(tmp_path / "outputs"))) == ["img0.png", "img1.png"]
        with pytest.raises(ValueError):
            E.evaluate_main(net, val, "0", "512,512", 19, whole=True, type="train")


def test_missing_pil_is_a_clear_import_error(tmp_path, monkeypatch):
    mod = gen()
    monkeypatch.setitem(sys.modules, "PIL", None)
    b = mod.eval_batches(11)[0]
    with backend(c_double()):
        with pytest.raises(ImportError, match="outputs"):
            E.evaluate_main(mod.FakeNet(19, 7), [(b[0][:, :, :32, :32], b[2], b[3])], "0", "512,512", 19, whole=True, type="test",
                            outputs=str(tmp_path))


# ---- 6. header <-> table <-> exported symbols ----------------------------------------------------------------------

def test_extension_header_table_and_library_agree():
    """What is particular to skd_eval.h; header <-> table <-> library <-> build digest: tests/test_abi.py, for every header."""
    typed = _lib.load()
    assert typed.skd_seg_sliding.argtypes == _lib.ABI["skd_eval.h"]["skd_seg_sliding"][1]
    # host-side refusals need no device: class counts the kernel was not built for, missing tensors
    assert typed.skd_seg_sliding(1, 33, 2, 2, 4, 4, 4, 4, 1, 1, None, 255, None, None, None, None, None) == 0
    assert typed.skd_seg_sliding(1, 19, 2, 2, 4, 4, 4, 4, None, None, None, 255, None, None, None, None, None) == 0
    assert typed.skd_seg_sliding(1, 19, 2, 2, 4, 4, 4, 4, 1, 1, 1, 255, None, None, None, None, None) == 0
