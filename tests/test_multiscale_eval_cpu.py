"""Multi-scale / flip evaluation, host side (no GPU): tests/golden/reference_multiscale.pt was written by
tests/golden/make_golden_multiscale.py from the REFERENCE's own ``predict_multiscale`` / ``evaluate_main(whole=True)`` with
scipy's ``ndimage.zoom`` and every forward's input and logits recorded.  Checked here: the numpy restatement of the resize
(tests/multiscale_ref.py, the bit-exact yardstick of the HIP kernels on the GPU) against scipy itself and against the
fixture; the restatement of the tail against the fixture; ``evaluate_main(whole=True, scales=..., flip=True)``,
``predict_multiscale`` and ``predict_whole`` end to end through a composite double (the plain-C double of oracle/ for the
core entries + the restatement as ``skd_zoom_linear`` / ``skd_seg_multiscale``); argument refusals; header <-> table <->
exported symbols for include/skd_eval_ms.h.

Bounds: resize values equal to scipy's (the sign of a zero is not compared); probabilities within 2^-22 max|logit| of the
reference's (one fp32 ulp of the interpolated value each way: the reference's CPU upsample rounds the four-term sum
differently); argmax disagreements at most 1e-5 pixels + 2 per case (the generator measured 0); evaluate_main: same scored
count, matrix difference <= 1e-5 scored + 2, IU within 2e-5 (tests/test_sliding_eval_cpu.check_evaluate_main)."""
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
import multiscale_ref as M  # noqa: E402
import sliding_ref as R  # noqa: E402

SCALES = (0.5, 0.6, 0.75, 1.0, 1.1, 1.25, 1.5, 1.75, 2.0)
# sizes the issue names as having a zeroed last line: (n, scale)
KNOWN_ZERO_LINES = [(1024, 0.75), (28, 0.5), (30, 0.5), (32, 0.5), (48, 0.5), (56, 0.5), (100, 0.75), (29, 1.5), (123, 1.25),
                    (24, 1.75), (48, 1.75), (96, 1.75)]


def gen():
    if GOLDEN_DIR not in sys.path:
        sys.path.insert(0, GOLDEN_DIR)          # the generator imports make_golden_sliding by name
    spec = importlib.util.spec_from_file_location("make_golden_multiscale", os.path.join(GOLDEN_DIR, "make_golden_multiscale.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_GOLD = []


def gold():
    if not _GOLD:
        _GOLD.append(torch.load(os.path.join(GOLDEN_DIR, "reference_multiscale.pt"), weights_only=False))
    return _GOLD[0]


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


def ms_double():
    return M.MultiscaleDouble(c_double())


# ---- 1. resize: restatement vs scipy ----------------------------------------------------------------------------------

def test_zoom_size_rounds_half_to_even():
    assert M.zoom_size(30, 0.75) == SF.zoom_size(30, 0.75) == 22 and M.zoom_size(50, 0.75) == SF.zoom_size(50, 0.75) == 38
    for n in range(1, 300):
        for s in SCALES:
            assert SF.zoom_size(n, s) == M.zoom_size(n, s) == int(round(n * s))


def test_zoom_restatement_vs_scipy_every_axis_length():
    """Every axis length 16 .. 200 at nine scales, along X (a 2 x n image, Y kept) and along Y (n x 2, X kept): the same size as
    scipy (half-to-even ones included), the same values, and exactly scipy's set of zeroed last lines."""
    nd = pytest.importorskip("scipy.ndimage")
    rng = np.random.RandomState(0)
    mine_zero, scipy_zero, half = set(), set(), 0
    for n in range(16, 201):
        line = (rng.randn(1, 2, n) * 57.0).astype(np.float32) + np.float32(200.0)       # no zero in the data itself
        for s in SCALES:
            half += (n * s) % 1 == 0.5
            for axis, img, zz in ((1, line, (1.0, 1.0, s)), (0, np.ascontiguousarray(line.transpose(0, 2, 1)), (1.0, s, 1.0))):
                want = nd.zoom(img, zz, order=1, prefilter=False)
                Ho, Wo = M.zoom_size(img.shape[1], zz[1]), M.zoom_size(img.shape[2], zz[2])
                assert want.shape == (1, Ho, Wo), (n, s, axis)
                got = M.zoom_linear(img, Ho, Wo)
                assert got.dtype == np.float32 and np.array_equal(got, want), (n, s, axis)
                last = want[:, :, -1] if axis == 1 else want[:, -1, :]
                if (last == 0).all():
                    scipy_zero.add((n, s))
                if M.zero_lines(n, Wo if axis == 1 else Ho):
                    mine_zero.add((n, s))
    assert half > 0, "the sweep must hold sizes that round half to even"
    assert mine_zero == scipy_zero and len(scipy_zero) > 0
    for n, s in KNOWN_ZERO_LINES:
        if n <= 200:
            assert (n, s) in scipy_zero, (n, s)
    assert M.zero_lines(1024, 768), "1024 rows at scale 0.75"


def test_zoom_restatement_vs_scipy_2d():
    nd = pytest.importorskip("scipy.ndimage")
    rng = np.random.RandomState(1)
    for (C, H, W), s in (((3, 100, 56), 0.5), ((3, 100, 56), 0.75), ((3, 100, 56), 1.75), ((3, 30, 50), 0.75), ((3, 33, 47), 1.1),
                         ((3, 33, 47), 2.0), ((1, 16, 16), 1.0), ((2, 29, 123), 1.5), ((2, 123, 29), 1.25)):
        img = (rng.randn(C, H, W) * 57.0).astype(np.float32)
        want = nd.zoom(img[None], (1.0, 1.0, s, s), order=1, prefilter=False)[0]
        got = M.zoom_linear(img, M.zoom_size(H, s), M.zoom_size(W, s))
        assert got.shape == want.shape and np.array_equal(got, want), ((C, H, W), s)
        if s == 1.0:
            assert np.array_equal(got, img), "scale 1.0 is an exact copy"


# ---- 2. restatement vs the reference's recorded inputs and outputs -----------------------------------------------------

def test_zoom_restatement_vs_reference_fixture():
    G, mod = gold(), gen()
    zero_rows = zero_cols = 0
    for name, H, W, classes, scales, flip, net_seed, img_seed in mod.CASES:
        c = G["cases"][name]
        image = mod.case_image(H, W, img_seed)[0].numpy()
        assert len(c["inputs"]) == len(scales)
        for rec, scale in zip(c["inputs"], scales):
            Ho, Wo = M.zoom_size(H, scale), M.zoom_size(W, scale)
            assert tuple(rec["size"]) == (Ho, Wo) and rec["scale"] == scale, (name, scale)
            got = M.zoom_linear(image, Ho, Wo)
            assert np.array_equal(got.reshape(-1)[rec["index"].numpy()], rec["values"].numpy()), (name, scale)
            assert bool((got[:, -1, :] == 0).all()) == rec["last_row_zero"] == M.zero_lines(H, Ho), (name, scale)
            assert bool((got[:, :, -1] == 0).all()) == rec["last_col_zero"] == M.zero_lines(W, Wo), (name, scale)
            zero_rows += rec["last_row_zero"]
            zero_cols += rec["last_col_zero"]
    assert zero_rows >= 1 and zero_cols >= 1


def test_tail_restatement_vs_reference_fixture():
    G = gold()
    assert sum(len(c["sample_pixels"]) for c in G["cases"].values()) >= 4096
    for name, c in G["cases"].items():
        H, W, C = c["H"], c["W"], c["classes"]
        logits = [lg.numpy() for lg in c["logits"]]
        assert max(float(np.abs(lg).max()) for lg in logits) == c["max_abs_logit"]
        probs, pred = M.multiscale(logits, c["flip"], (H, W))
        assert probs.dtype == np.float64 and probs.shape == (H, W, C)
        pix = c["sample_pixels"].numpy().astype(np.int64)
        err = float(np.abs(probs.reshape(H * W, C)[pix] - c["sample_probs"].numpy()).max())
        flips = int((pred != c["argmax"].numpy()).sum())
        print("%s: max|dprob| %.3e (bound %.3e), argmax flips %d of %d" % (name, err, 2.0 ** -22 * c["max_abs_logit"], flips, H * W))
        assert err <= 2.0 ** -22 * c["max_abs_logit"], name
        assert flips <= 1e-5 * H * W + 2, name


# ---- 3. evaluate_main / predict_multiscale / predict_whole through the composite double ---------------------------------

def check_evaluate_main(device, G, mod, net=None):
    """evaluate_main(whole=True, scales, flip) on the fixture's full-size image; asserts the fixture's bounds; returns the matrix."""
    ev = G["evaluate_main"]
    net = net if net is not None else mod.FakeNet(19, ev["net_seed"]).to(device)
    seen = []
    orig = E.iou_from_confusion
    E.iou_from_confusion = lambda cm: seen.append(np.array(cm)) or orig(cm)
    try:
        m, iu = E.evaluate_main(net, [mod.eval_batch(ev["image_seed"])], "0", "512,512", 19, whole=True, scales=ev["scales"], flip=ev["flip"])
    finally:
        E.iou_from_confusion = orig
    cm, want = seen[0], ev["confusion"].numpy()
    diff = np.abs(cm - want).sum() / 2                    # a flipped pixel moves one count
    print("confusion vs the reference's: %d of %d scored pixels differ" % (diff, want.sum()))
    assert cm.sum() == want.sum(), "same number of scored pixels (ignore mask, evaluate.py:195-197)"
    assert diff <= 1e-5 * want.sum() + 2
    wm, wiu = E.iou_from_confusion(want)
    assert np.abs(np.asarray(iu) - wiu).max() <= 2e-5 and abs(m - wm) <= 2e-5
    assert np.abs(np.asarray(iu) - ev["IU_array"].numpy()).max() <= 2e-5 and abs(m - ev["mean_IU"]) <= 2e-5
    return cm


def test_evaluate_main_multiscale_vs_reference_fixture_through_composite_double():
    G, mod = gold(), gen()
    assert tuple(G["evaluate_main"]["size"]) == tuple(mod.EVAL_SIZE) and G["evaluate_main"]["last_row_zero_at_075"]
    double = ms_double()
    with backend(double):
        check_evaluate_main(torch.device("cpu"), G, mod)
    n = len(G["evaluate_main"]["scales"])
    assert (double.zoom_calls, double.ms_calls, double.confusion_calls, double.calls) == (n, 1, 0, 0), "one resize per scale, one fused tail"


class Counting(torch.nn.Module):
    def __init__(self, net):
        super().__init__()
        self.net = net
        self.shapes = []

    def forward(self, x):
        self.shapes.append(tuple(x.shape))
        return self.net(x)


def small_val_batches(mod, H=64, W=96):
    g = torch.Generator().manual_seed(3)
    image = torch.randn(1, 3, H, W, generator=g) * 57.0
    label = torch.randint(0, 19, (1, H, W), generator=g).float()
    label[0, :9, :30] = 255
    return [(image, label, torch.tensor([[H, W, 3]]), ["a"])]


def test_plain_scales_take_the_existing_whole_image_path():
    """``scales`` None and ``[1.0]`` without flip call skd_seg_confusion and neither new entry; ``[1.0]`` WITH flip, or any other
    scale, takes the new path: one forward of batch F per scale, none through skd_seg_confusion."""
    mod = gen()
    batches = small_val_batches(mod)
    net = Counting(mod.FakeNet(19, 7))
    double = ms_double()
    with backend(double):
        base = E.evaluate_main(net, batches, "0", "512,512", 19, whole=True)
        assert (double.confusion_calls, double.zoom_calls, double.ms_calls) == (1, 0, 0)
        for kw in ({"scales": None}, {"scales": [1.0]}, {"scales": (1.0,), "flip": False}):
            again = E.evaluate_main(net, batches, "0", "512,512", 19, whole=True, **kw)
            assert again[0] == base[0] and np.array_equal(again[1], base[1])
        assert (double.confusion_calls, double.zoom_calls, double.ms_calls) == (4, 0, 0)
        assert net.shapes == [(1, 3, 64, 96)] * 4
        net.shapes.clear()
        E.evaluate_main(net, batches, "0", "512,512", 19, whole=True, scales=[1.0], flip=True)
        assert (double.confusion_calls, double.zoom_calls, double.ms_calls) == (4, 1, 1) and net.shapes == [(2, 3, 64, 96)]
        net.shapes.clear()
        one = E.evaluate_main(net, batches, "0", "512,512", 19, whole=True, scales=[0.75, 1.0])
        assert (double.confusion_calls, double.zoom_calls, double.ms_calls) == (4, 3, 2) and net.shapes == [(1, 3, 48, 72), (1, 3, 64, 96)]
        assert 0.0 <= one[0] <= 1.0


def test_predict_multiscale_and_predict_whole_through_composite_double():
    G, mod = gold(), gen()
    name, H, W, classes, scales, flip, net_seed, img_seed = mod.CASES[1]            # zero_lines
    c = G["cases"][name]
    net = Counting(mod.FakeNet(classes, net_seed))
    image = mod.case_image(H, W, img_seed)
    with backend(ms_double()):
        probs = E.predict_multiscale(net, image.numpy(), (H, W), scales, classes, flip, recurrence=3)
        assert [s[0] for s in net.shapes] == [2] * len(scales) and [s[2:] for s in net.shapes] == [tuple(r["size"]) for r in c["inputs"]]
        with pytest.raises(ValueError, match="tile_size"):
            E.predict_multiscale(net, image, (H, W + 1), scales, classes, flip)
        with pytest.raises(ValueError):
            E.predict_multiscale(net, image, (H, W), scales, classes + 1, flip)
        with pytest.raises(ValueError):
            E.predict_multiscale(net, image, (H, W), [0.01], classes, flip)         # an axis below 2
        whole = E.predict_whole(net, image.numpy(), (37, 53))
        with torch.no_grad():
            lg = net(image)[0].numpy()
    assert isinstance(probs, np.ndarray) and probs.shape == (H, W, classes) and probs.dtype == np.float64
    pix = c["sample_pixels"].numpy().astype(np.int64)
    # same host, same conv library as the generator's run unless the fixture travelled: the logits' own rounding is the slack
    assert np.abs(probs.reshape(H * W, classes)[pix] - c["sample_probs"].numpy()).max() <= 2.0 ** -22 * c["max_abs_logit"] + 1e-4
    assert (probs.argmax(2) != c["argmax"].numpy()).sum() <= 1e-5 * H * W + 2
    assert isinstance(whole, np.ndarray) and whole.dtype == np.float32 and whole.shape == (37, 53, classes)
    assert np.array_equal(whole, R.upsample(lg[0], (37, 53)).transpose(1, 2, 0)), "predict_whole is the plain fp32 upsample"


def read_png(path):
    from PIL import Image
    im = Image.open(path)
    return im.mode, list(im.getpalette()), np.array(im)


def check_test_split(device, tmp_path, mod):
    """type='test' in multi-scale mode writes <outputs>/<name>.png = remap[pred] in mode P with get_palette(256); returns None."""
    net = mod.FakeNet(19, 7).to(device)
    g = torch.Generator().manual_seed(12)
    H, W, scales = 100, 56, [0.5, 0.75, 1.0]
    batches = [(torch.randn(1, 3, H, W, generator=g) * 57.0, torch.tensor([[H, W, 3]]), ["sub/im%d" % i]) for i in range(2)]
    out = str(tmp_path / "test_ms")
    assert E.evaluate_main(net, batches, "0", "512,512", 19, whole=True, type="test", outputs=out, scales=scales, flip=True) is None
    table = E.trainid_to_id_table()
    for image, _, name in batches:
        with torch.no_grad():
            # the same batched forwards as evaluate_main's, so that the logits carry the same bits on any conv library
            logits = E._scale_logits(net, image.to(device), scales, True, False)
            pred, _, _ = SF.seg_multiscale(logits, (H, W))
        mode, palette, pixels = read_png(os.path.join(out, name[0] + ".png"))
        assert mode == "P" and palette == E.get_palette(256)
        assert pixels.shape == (H, W) and np.array_equal(pixels, table[pred.cpu().numpy()])
        assert set(np.unique(pixels)) <= set(table[:19].tolist())


def test_test_split_writes_remapped_palette_png(tmp_path):
    with backend(ms_double()):
        check_test_split(torch.device("cpu"), tmp_path, gen())


# ---- 4. refusals ------------------------------------------------------------------------------------------------------

def test_argument_refusals():
    mod = gen()
    batches = small_val_batches(mod)
    net = mod.FakeNet(19, 7)
    with backend(ms_double()):
        with pytest.raises(ValueError, match="whole"):
            E.evaluate_main(net, batches, "0", "32,32", 19, whole=False, scales=[0.75, 1.0])
        with pytest.raises(ValueError, match="whole"):
            E.evaluate_main(net, batches, "0", "32,32", 19, flip=True)
        with pytest.raises(ValueError):
            E.evaluate_main(net, batches, "0", "32,32", 19, whole=True, scales=[])
        with pytest.raises(ValueError):                   # label and image differ in size
            E.evaluate_main(net, [(batches[0][0], batches[0][1][:, :60], torch.tensor([[60, 96, 3]]), ["a"])], "0", "32,32", 19, whole=True, flip=True)
        with pytest.raises(ValueError):                   # out-of-range label, as in the other modes
            E.evaluate_main(net, [(batches[0][0], batches[0][1] * 0 + 19, batches[0][2], ["a"])], "0", "32,32", 19, whole=True, flip=True)
        with pytest.raises(ValueError):                   # 3 rows at 0.5 give 2, 3 columns at 0.5 give 2, but at 0.3 an axis of 1
            SF.zoom_linear(torch.zeros(1, 3, 3, 8), 0.3)
        with pytest.raises(ValueError):
            SF.zoom_linear(torch.zeros(2, 3, 8, 8), 1.0)                            # two images
        with pytest.raises(TypeError):
            SF.zoom_linear(torch.zeros(1, 3, 8, 8, dtype=torch.float64), 1.0)
        a, b = torch.zeros(2, 3, 2, 2), torch.zeros(1, 3, 4, 4)
        with pytest.raises(ValueError):
            SF.seg_multiscale([a, b], (4, 4))                                        # mixed F
        with pytest.raises(ValueError):
            SF.seg_multiscale([b, torch.zeros(1, 4, 2, 2)], (4, 4))                  # mixed C
        with pytest.raises(ValueError):
            SF.seg_multiscale([torch.zeros(1, 33, 2, 2)], (4, 4))                    # more than 32 classes
        with pytest.raises(ValueError):
            SF.seg_multiscale([torch.zeros(3, 3, 2, 2)], (4, 4))                     # F = 3
        with pytest.raises(ValueError):
            SF.seg_multiscale([], (4, 4))
        with pytest.raises(TypeError):
            SF.seg_multiscale([b.double()], (4, 4))
        with pytest.raises(TypeError):
            SF.seg_multiscale([b], (4, 4), target=torch.zeros(4, 4, dtype=torch.int32))
        with pytest.raises(ValueError):
            SF.seg_multiscale([b], (4, 4), target=torch.zeros(4, 5, dtype=torch.int64))
        with pytest.raises(TypeError):
            SF.seg_multiscale([b], (4, 4), remap=torch.zeros(19, dtype=torch.uint8))
        pred, probs, cm = SF.seg_multiscale([a, a], (4, 4), target=torch.ones(4, 4, dtype=torch.int64), want_probs=True)
        assert pred.dtype == torch.uint8 and int(pred.sum()) == 0 and probs.shape == (4, 4, 3) and int(cm[1, 0]) == 16


def test_plain_c_double_has_no_multiscale_entries():
    class Exploding(torch.nn.Module):
        def forward(self, x):
            raise AssertionError("the model must not be touched")

    def loader():
        raise AssertionError("the loader must not be touched")
        yield

    with backend(c_double()):
        assert not _lib.has_entry("skd_zoom_linear") and not _lib.has_entry("skd_seg_multiscale")
        with pytest.raises(NotImplementedError, match="skd_zoom_linear"):
            E.evaluate_main(Exploding(), loader(), "0", "512,512", 19, whole=True, scales=[0.75, 1.0])
        with pytest.raises(NotImplementedError, match="skd_zoom_linear"):
            E.predict_multiscale(Exploding(), np.zeros((1, 3, 8, 8), np.float32), (8, 8), [1.0], 19, True)
        with pytest.raises(NotImplementedError, match="skd_"):
            E.predict_whole(Exploding(), np.zeros((1, 3, 8, 8), np.float32), (8, 8))
        with pytest.raises(NotImplementedError, match="skd_zoom_linear"):
            SF.zoom_linear(torch.zeros(1, 3, 8, 8), 1.0)
        with pytest.raises(NotImplementedError, match="skd_seg_multiscale"):
            SF.seg_multiscale([torch.zeros(1, 2, 2, 2)], (4, 4))


# ---- 5. header <-> table <-> exported symbols --------------------------------------------------------------------------

def test_multiscale_header_table_and_library_agree():
    """What is particular to skd_eval_ms.h; header <-> table <-> library <-> build digest: tests/test_abi.py, for every header."""
    assert sorted(_lib.ABI["skd_eval_ms.h"]) == ["skd_seg_multiscale", "skd_zoom_linear"]
    typed = _lib.load()
    # host-side refusals need no device
    z = typed.skd_zoom_linear
    assert z(0, 8, 8, 4, 4, 1, 1, 0, 0, None) == 0 and z(3, 0, 8, 4, 4, 1, 1, 0, 0, None) == 0 and z(3, 8, -1, 4, 4, 1, 1, 0, 0, None) == 0
    assert z(3, 8, 8, 1, 4, 1, 1, 0, 0, None) == 0 and z(3, 8, 8, 4, 1, 1, 1, 1, 1, None) == 0
    assert z(3, 8, 8, 4, 4, None, 1, 0, 0, None) == 0 and z(3, 8, 8, 4, 4, 1, None, 0, 0, None) == 0
    s = typed.skd_seg_multiscale
    assert s(0, 1, 19, 4, 4, 1, 1, None, 255, None, None, None, None, None) == 0
    assert s(1, 0, 19, 4, 4, 1, 1, None, 255, None, None, None, None, None) == 0
    assert s(1, 3, 19, 4, 4, 1, 1, None, 255, None, None, None, None, None) == 0
    assert s(1, 1, 0, 4, 4, 1, 1, None, 255, None, None, None, None, None) == 0
    assert s(1, 1, 33, 4, 4, 1, 1, None, 255, None, None, None, None, None) == 0
    assert s(1, 1, 19, 0, 4, 1, 1, None, 255, None, None, None, None, None) == 0
    assert s(1, 1, 19, 4, -2, 1, 1, None, 255, None, None, None, None, None) == 0
    assert s(1, 2, 19, 4, 4, None, 1, None, 255, None, None, None, None, None) == 0
    assert s(1, 2, 19, 4, 4, 1, None, None, 255, None, None, None, None, None) == 0
    assert s(1, 2, 19, 4, 4, 1, 1, 1, 255, None, None, None, None, None) == 0          # target without confusion
