"""csrc/evaluate_multiscale.hip on the MI355X: the resize kernel against the numpy restatement of scipy's zoom
(tests/multiscale_ref.py, value for value), the fused multi-scale / flip tail against the restatement (bit for bit) and against
the REFERENCE's recorded outputs in tests/golden/reference_multiscale.pt (bounds of tests/test_multiscale_eval_cpu.py); both
entries between guard bands; ``evaluate_main(whole=True, scales=..., flip=True)`` and ``type='test'`` end to end; the real
student on one full-size image.  None of these can pass without the kernels.  No test double may be active here: the autouse
fixture removes one and puts it back."""
import os
import sys

import numpy as np
import pytest
import torch

from structure_knowledge_distillation_amd import _lib
from structure_knowledge_distillation_amd import functional as SF
from structure_knowledge_distillation_amd.networks import evaluate as E

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import bounds_cases as BC  # noqa: E402  (Arena: guard-banded buffers)
import multiscale_ref as M  # noqa: E402
import test_multiscale_eval_cpu as CPU  # noqa: E402  (shared helpers: fixture loading, evaluate_main / test-split checks)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def no_test_double():
    prev = _lib._test_backend
    _lib.install_test_backend(None)
    yield
    _lib.install_test_backend(prev)


def seeded_target(H, W, C, seed):
    g = np.random.RandomState(seed)
    t = g.randint(0, C, size=(H, W)).astype(np.int64)
    t[g.rand(H, W) < 0.1] = 255
    t[: H // 7, : W // 3] = 255
    return t


# ---- 1. the resize kernel ---------------------------------------------------------------------------------------------

ZOOM_CASES = [((3, 100, 56), 0.5), ((3, 100, 56), 0.75), ((3, 100, 56), 1.75), ((3, 30, 50), 0.75), ((3, 33, 47), 1.1), ((3, 33, 47), 2.0),
              ((1, 16, 16), 1.0)]


@pytest.mark.parametrize("shape,scale", ZOOM_CASES)
def test_zoom_linear_kernel_vs_restatement(shape, scale):
    """Values equal to the restatement (which equals scipy, tests/test_multiscale_eval_cpu.py), zeroed last lines included;
    plain and mirrored, NCHW and channels-last; the mirrored element is the exact X-reverse of element 0."""
    C, H, W = shape
    img = (np.random.RandomState(H + W).randn(C, H, W) * 57.0).astype(np.float32)
    Ho, Wo = M.zoom_size(H, scale), M.zoom_size(W, scale)
    want = M.zoom_linear(img, Ho, Wo)
    if (shape, scale) == ((3, 100, 56), 0.5):
        assert (want[:, :, -1] == 0).all() and not (want[:, :, -2] == 0).all()
    if (shape, scale) == ((3, 100, 56), 0.75):
        assert (want[:, -1, :] == 0).all() and not (want[:, -2, :] == 0).all()
    if (shape, scale) == ((3, 30, 50), 0.75):
        assert (Ho, Wo) == (22, 38), "half to even"
    dev = torch.from_numpy(img).to(DEV)
    for mirror in (False, True):
        for cl in (False, True):
            out = SF.zoom_linear(dev[None] if mirror else dev, scale, mirror=mirror, channels_last=cl)
            assert tuple(out.shape) == (2 if mirror else 1, C, Ho, Wo) and out.dtype == torch.float32
            if cl and C > 1:
                assert out.is_contiguous(memory_format=torch.channels_last)
            got = out.cpu().numpy()
            assert np.array_equal(got[0], want), (shape, scale, mirror, cl)
            if mirror:
                assert np.array_equal(got[1], got[0][:, :, ::-1]), (shape, scale, cl)
    with pytest.raises(_lib.SkdLibraryError):
        SF.zoom_linear(torch.from_numpy(img), scale)                                 # CPU tensors: no fallback


# ---- 2. the fused tail -------------------------------------------------------------------------------------------------

def run_tail_case(name, logits, flip, H, W, ref_argmax=None, samples=None, peak=None):
    """pred / confusion / probs of the kernel vs the restatement (bit-equal), with and without target and remap."""
    C = logits[0].shape[1]
    want_probs, want_pred = M.multiscale(logits, flip, (H, W))
    target = seeded_target(H, W, C, 5)
    want_cm = M.confusion(target, want_pred, C)
    remap_np = np.random.RandomState(3).permutation(256).astype(np.uint8)
    lg = [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in logits]
    tg, remap = torch.from_numpy(target).to(DEV), torch.from_numpy(remap_np).to(DEV)
    # no target, no remap, with probabilities
    pred, probs, cm = SF.seg_multiscale(lg, (H, W), want_probs=True)
    assert cm is None and pred.dtype == torch.uint8 and probs.dtype == torch.float64
    assert np.array_equal(pred.cpu().numpy(), want_pred), name
    got_probs = probs.cpu().numpy()
    exact = np.array_equal(got_probs, want_probs)
    print("%s: probabilities bit-equal to the restatement: %s (max|d| %.3e)" % (name, exact, np.abs(got_probs - want_probs).max()))
    assert exact, name
    # target, no remap; the matrix is accumulated INTO
    cm = torch.ones((C, C), dtype=torch.int64, device=DEV)
    pred, _, cm2 = SF.seg_multiscale(lg, (H, W), target=tg, confusion=cm)
    assert cm2 is cm and np.array_equal(cm.cpu().numpy(), want_cm + 1), name
    assert np.array_equal(pred.cpu().numpy(), want_pred), name
    # target + remap: the written prediction is remapped, the matrix is not
    pred, _, cm = SF.seg_multiscale(lg, (H, W), target=tg, remap=remap)
    assert np.array_equal(pred.cpu().numpy(), remap_np[want_pred]) and np.array_equal(cm.cpu().numpy(), want_cm), name
    # remap, no target; no prediction wanted
    pred, _, cm = SF.seg_multiscale(lg, (H, W), remap=remap)
    assert cm is None and np.array_equal(pred.cpu().numpy(), remap_np[want_pred]), name
    none, _, cm = SF.seg_multiscale(lg, (H, W), target=tg, want_pred=False)
    assert none is None and np.array_equal(cm.cpu().numpy(), want_cm), name
    assert int(want_cm.sum()) == int((target != 255).sum())
    if ref_argmax is not None:
        pix, ref = samples
        err = float(np.abs(got_probs.reshape(H * W, C)[pix] - ref).max())
        flips = int((want_pred != ref_argmax).sum())
        print("%s: vs the reference: max|dprob| %.3e (bound %.3e), argmax flips %d of %d" % (name, err, 2.0 ** -22 * peak, flips, H * W))
        assert err <= 2.0 ** -22 * peak, name
        assert flips <= 1e-5 * H * W + 2, name


@pytest.mark.parametrize("name", ["ms4_flip", "zero_lines", "noflip_odd", "single_flip"])
def test_seg_multiscale_kernel_vs_restatement_and_reference_fixture(name):
    """Every fixture case (recorded logits of the reference's run): ``pred``, the confusion matrix and ``probs`` bit-equal to the
    restatement (fp32 interpolation without contraction, fp32 flip average, exact float -> double, float64 adds in scale order
    and one correctly rounded float64 divide are the same operations in the same order); ``probs`` within 2^-22 max|logit| of
    the reference's sampled probabilities; ``pred`` vs the reference's argmax under the near-tie cap 1e-5 pixels + 2."""
    c = CPU.gold()["cases"][name]
    run_tail_case(name, [lg.numpy() for lg in c["logits"]], c["flip"], c["H"], c["W"], c["argmax"].numpy(),
                  (c["sample_pixels"].numpy().astype(np.int64), c["sample_probs"].numpy()), c["max_abs_logit"])


@pytest.mark.parametrize("C", [1, 8, 9, 16, 17, 19, 20, 21, 22, 32])
def test_seg_multiscale_class_bounds(C):
    """The kernel's compile-time class bounds from both sides, S = 3, F = 2, output 37 x 53 from maps 5 x 7, 9 x 4 and 1 x 1 (the
    1 x 1 map: scale factor zero on both axes)."""
    g = np.random.RandomState(100 + C)
    logits = [(g.randn(2, C, h, w) * 16).astype(np.float32) for h, w in ((5, 7), (9, 4), (1, 1))]
    run_tail_case("classes_%d" % C, logits, True, 37, 53)


def test_seg_multiscale_refusals_on_device():
    with pytest.raises(ValueError):
        SF.seg_multiscale([torch.zeros(1, 33, 2, 2, device=DEV)], (4, 4))
    with pytest.raises(_lib.SkdLibraryError):
        SF.seg_multiscale([torch.zeros(1, 3, 2, 2)], (4, 4))                         # CPU tensors: no fallback


def test_seg_multiscale_single_scale_equals_whole_image_kernel():
    """S = 1, F = 1: the same interpolation as csrc/evaluate.hip, (double)v / 1.0 is exact, so ``pred`` and ``confusion`` equal
    skd_seg_confusion's on the same logits; also an output of one row / one column (scale factor zero on that axis)."""
    g = np.random.RandomState(41)
    for C, (h, w), (H, W) in ((19, (17, 33), (131, 257)), (7, (5, 9), (1, 40)), (21, (4, 4), (33, 1))):
        lg = torch.from_numpy((g.randn(1, C, h, w) * 16).astype(np.float32)).to(DEV)
        tg = torch.from_numpy(seeded_target(H, W, C, 6)).to(DEV)
        pred0, cm0 = SF.seg_confusion(lg, tg[None], 255, None)
        pred1, _, cm1 = SF.seg_multiscale([lg], (H, W), target=tg)
        assert torch.equal(pred0[0], pred1) and torch.equal(cm0, cm1), (C, h, w, H, W)


# ---- 3. guard bands -----------------------------------------------------------------------------------------------------

def guard_zoom(lib, A, scale, mirror, channels_last):
    C, H, W = 3, 100, 56                                   # the fixture's zero_lines image size
    img0 = (np.random.RandomState(9).randn(C, H, W) * 57.0).astype(np.float32)
    Ho, Wo = M.zoom_size(H, scale), M.zoom_size(W, scale)
    F = 2 if mirror else 1
    img = A.inp("image", torch.from_numpy(img0), row=W)
    out = A.out("out", (F, Ho, Wo, C) if channels_last else (F, C, Ho, Wo), row=Wo * C if channels_last else Wo)
    assert lib.skd_zoom_linear(C, H, W, Ho, Wo, BC.P(img), BC.P(out), int(mirror), int(channels_last), None) == 1
    A.check()
    z = M.zoom_linear(img0, Ho, Wo)
    want = np.stack([z, z[:, :, ::-1]][:F])
    if channels_last:
        want = want.transpose(0, 2, 3, 1)
    got = out.cpu().numpy()
    assert not np.isnan(got).any(), "an output element was left unwritten"
    assert np.array_equal(got, want)


def guard_tail(lib, A, with_probs):
    c = CPU.gold()["cases"]["zero_lines"]
    H, W, C = c["H"], c["W"], c["classes"]
    maps = [lg.numpy() for lg in c["logits"]]
    rows, off = [], 0
    for m in maps:
        rows.append((off, m.shape[2], m.shape[3]))
        off += m.size
    packed = np.concatenate([m.reshape(-1) for m in maps])
    tg0 = seeded_target(H, W, C, 5)
    remap0 = np.random.RandomState(3).permutation(256).astype(np.uint8)
    lg, tb = A.inp("logits", torch.from_numpy(packed)), A.inp("table", torch.tensor(rows, dtype=torch.int64))
    tg, rm = A.inp("target", torch.from_numpy(tg0)), A.inp("remap", torch.from_numpy(remap0))
    pred = A.out("pred", (H, W), torch.uint8)
    probs = A.out("probs", (H, W, C), torch.float64) if with_probs else None
    conf = A.io("confusion", torch.ones(C, C, dtype=torch.int64))
    assert lib.skd_seg_multiscale(len(rows), 2, C, H, W, BC.P(lg), BC.P(tb), BC.P(tg), 255, BC.P(rm), BC.P(pred), BC.P(probs), BC.P(conf), None) == 1
    A.check()
    want_probs, want_pred = M.multiscale(maps, True, (H, W))
    assert np.array_equal(pred.cpu().numpy(), remap0[want_pred])
    assert np.array_equal(conf.cpu().numpy(), M.confusion(tg0, want_pred, C) + 1)
    if with_probs:
        got = probs.cpu().numpy()
        assert not np.isnan(got).any(), "an output element was left unwritten"
        assert np.array_equal(got, want_probs)
    # without a remap an unwritten prediction (0xFF) cannot pass for a class id
    plain = A.out("pred_plain", (H, W), torch.uint8)
    assert lib.skd_seg_multiscale(len(rows), 2, C, H, W, BC.P(lg), BC.P(tb), None, 255, None, BC.P(plain), None, None, None) == 1
    A.check()
    assert np.array_equal(plain.cpu().numpy(), want_pred) and int(plain.max()) < C


GUARD_CASES = {
    "zoom-0.5-plain-nchw": ("skd_zoom_linear", guard_zoom, (0.5, False, False)),
    "zoom-0.5-mirror-nhwc": ("skd_zoom_linear", guard_zoom, (0.5, True, True)),
    "zoom-0.75-mirror-nchw": ("skd_zoom_linear", guard_zoom, (0.75, True, False)),
    "zoom-1.75-plain-nhwc": ("skd_zoom_linear", guard_zoom, (1.75, False, True)),
    "tail-probs": ("skd_seg_multiscale", guard_tail, (True,)),
    "tail-no-probs": ("skd_seg_multiscale", guard_tail, (False,)),
}


@pytest.mark.parametrize("name", list(GUARD_CASES))
def test_entries_stay_inside_their_buffers(name):
    """Inputs, outputs and the scale table between 0xFF guard bands, outputs pre-filled with 0xFF: no guard byte changes, no
    output element is left unwritten, values as in the restatement; no device status word is raised."""
    _, fn, args = GUARD_CASES[name]
    lib = _lib.load()
    fn(lib, BC.Arena("cuda"), *args)
    torch.cuda.synchronize()
    assert _lib.device_status() == [0] * lib.skd_status_words()


def test_every_multiscale_entry_has_a_guard_band_case():
    covered = {entry for entry, _, _ in GUARD_CASES.values()}
    assert covered == set(_lib.ABI["skd_eval_ms.h"])
    assert all(_lib.ctypes.c_void_p in args for _, args in _lib.ABI["skd_eval_ms.h"].values()), "both entries take pointers"


# ---- 4. end to end ------------------------------------------------------------------------------------------------------

def test_evaluate_main_multiscale_vs_reference_fixture_on_gpu():
    """evaluate_main(whole=True, scales=[0.75, 1.0, 1.25], flip=True) with the generator's FakeNet against the reference's
    confusion matrix, mean IU and IU array (bounds of the CPU test).  The convolution runs in another library here than on the
    generator's CPU, the same exposure as the sliding test's at the same cap; the count of differing pixels is printed."""
    CPU.check_evaluate_main(DEV, CPU.gold(), CPU.gen())


def test_test_split_multiscale_on_gpu(tmp_path):
    """type='test' in this mode: files named after name[0], mode P, get_palette(256), contents remap[pred]; nothing is scored."""
    CPU.check_test_split(DEV, tmp_path, CPU.gen())


class Recording(torch.nn.Module):
    def __init__(self, net):
        super().__init__()
        self.net = net
        self.inputs, self.logits = [], []

    def forward(self, x):
        out = self.net(x)
        self.inputs.append((tuple(x.shape), x.is_contiguous(memory_format=torch.channels_last)))
        self.logits.append(out[0].detach().float())
        return out


def test_real_student_full_size_multiscale_consistency():
    """The real student (Res_pspnet BasicBlock [2, 2, 2, 2], seeded, eval, channels-last like NetModel keeps it) on one seeded
    1024 x 2048 image, scales [0.75, 1.0] with flip.  No reference fixture exists for this one: it is a consistency test -- one
    channels-last forward of batch 2 per scale, finite result, every non-ignored pixel scored once, predict_multiscale's array
    has the reference's shape and dtype and its argmax is the kernel's prediction on the same logits."""
    from structure_knowledge_distillation_amd.networks import pspnet_combine
    torch.manual_seed(23)
    S = pspnet_combine.Res_pspnet(pspnet_combine.BasicBlock, [2, 2, 2, 2], 19)
    S = S.to(DEV).to(memory_format=torch.channels_last).eval()
    net = Recording(S)
    g = torch.Generator().manual_seed(29)
    image = torch.randn(1, 3, 1024, 2048, generator=g) * 57.0
    label = torch.randint(0, 19, (1, 1024, 2048), generator=g)
    label[0, 100:300, :700] = 255
    scales = [0.75, 1.0]
    probs = E.predict_multiscale(net, image, (1024, 2048), scales, 19, True)
    assert net.inputs == [((2, 3, 768, 1536), True), ((2, 3, 1024, 2048), True)], "one channels-last forward of batch 2 per scale"
    assert isinstance(probs, np.ndarray) and probs.shape == (1024, 2048, 19) and probs.dtype == np.float64
    assert np.isfinite(probs).all()
    pred, _, cm = SF.seg_multiscale(net.logits, (1024, 2048), target=label[0].to(DEV))
    assert np.array_equal(np.argmax(probs, axis=2).astype(np.uint8), pred.cpu().numpy())
    assert int(cm.sum()) == int((label != 255).sum())
    net.inputs.clear()
    mean_iu, iu = E.evaluate_main(net, [(image, label, torch.tensor([[1024, 2048, 3]]), ["a"])], "0", "512,512", 19, whole=True,
                                  scales=scales, flip=True)
    assert [s for s, _ in net.inputs] == [(2, 3, 768, 1536), (2, 3, 1024, 2048)]
    assert np.isfinite(mean_iu) and np.isfinite(np.asarray(iu)).all() and 0.0 <= mean_iu <= 1.0
