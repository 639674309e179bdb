"""csrc/evaluate_sliding.hip on the MI355X: the fused sliding-window tail (per-tile bilinear upsample, float64 accumulation
in tile order, mean, argmax, id remap, confusion matrix) against the numpy restatement tests/sliding_ref.py (bit for bit)
and against the REFERENCE's recorded outputs in tests/golden/reference_sliding.pt (bounds of tests/test_sliding_eval_cpu.py);
``evaluate_main(whole=False)`` and ``type='test'`` end to end; the real student on one full-size image.  None of these can
pass without the kernel.  No test double may be active here: the autouse fixture removes one and puts it back."""
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
import sliding_ref as R  # noqa: E402
import test_sliding_eval_cpu as CPU  # noqa: E402  (shared helpers: fixture loading, evaluate_main / test-split checks)

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


def run_kernel_case(name, logits, tile, H, W, ref_argmax=None, samples=None, peak=None):
    """pred / confusion / probs of the kernel vs the restatement (bit-equal), with and without target and remap."""
    C = logits.shape[1]
    tiles = R.tiles_of(H, W, tile)
    want_probs, want_pred = R.sliding(logits, tiles, tile, (H, W))
    target = seeded_target(H, W, C, 5)
    want_cm = R.confusion(target, want_pred, C)
    remap_np = np.random.RandomState(3).permutation(256).astype(np.uint8)
    lg, tg, remap = torch.from_numpy(logits).to(DEV), torch.from_numpy(target).to(DEV), torch.from_numpy(remap_np).to(DEV)
    # no target, no remap, with probabilities
    pred, probs, cm = SF.seg_sliding(lg, tiles, tile, (H, W), want_probs=True)
    assert cm is None and pred.dtype == torch.uint8 and probs.dtype == torch.float64
    assert np.array_equal(pred.cpu().numpy(), want_pred), name
    got_probs = probs.cpu().numpy()
    exact = np.array_equal(got_probs, want_probs)
    print("%s: probabilities bit-equal to the restatement: %s (max|d| %.3e)" % (name, exact, np.abs(got_probs - want_probs).max()))
    assert exact, name
    # target, no remap; the matrix is accumulated INTO
    cm = torch.ones((C, C), dtype=torch.int64, device=DEV)
    pred, _, cm2 = SF.seg_sliding(lg, tiles, tile, (H, W), target=tg, confusion=cm)
    assert cm2 is cm and np.array_equal(cm.cpu().numpy(), want_cm + 1), name
    assert np.array_equal(pred.cpu().numpy(), want_pred), name
    # target + remap: the written prediction is remapped, the matrix is not
    pred, _, cm = SF.seg_sliding(lg, tiles, tile, (H, W), target=tg, remap=remap)
    assert np.array_equal(pred.cpu().numpy(), remap_np[want_pred]) and np.array_equal(cm.cpu().numpy(), want_cm), name
    # remap, no target; a device tile table; no prediction wanted
    tl = torch.tensor(tiles, dtype=torch.int32, device=DEV)
    pred, _, cm = SF.seg_sliding(lg, tl, tile, (H, W), remap=remap)
    assert cm is None and np.array_equal(pred.cpu().numpy(), remap_np[want_pred]), name
    none, _, cm = SF.seg_sliding(lg, tl, tile, (H, W), target=tg, want_pred=False)
    assert none is None and np.array_equal(cm.cpu().numpy(), want_cm), name
    assert int(want_cm.sum()) == int((target != 255).sum())
    if ref_argmax is not None:
        pix, ref = samples
        err = float(np.abs(got_probs.reshape(H * W, C)[pix] - ref).max())
        flips = int((want_pred != ref_argmax).sum())
        print("%s: vs the reference: max|dprob| %.3e (bound %.3e), argmax flips %d of %d" % (name, err, 2.0 ** -22 * peak, flips, H * W))
        assert err <= 2.0 ** -22 * peak, name
        assert flips <= 1e-5 * H * W + 2, name


def test_seg_sliding_kernel_vs_restatement_and_reference_fixture():
    """Every fixture case (recorded tile logits of the reference's run): ``pred`` and the confusion matrix bit-equal to the
    restatement with / without target and remap; ``probs`` within 2^-22 max|logit| of the reference's sampled
    probabilities AND bit-equal to the restatement (asserted: fp32 interpolation without contraction, exact float -> double,
    float64 adds in tile order and one correctly rounded float64 divide are the same operations in the same order);
    ``pred`` vs the reference's argmax under the near-tie cap 1e-5 pixels + 2."""
    for name, c in CPU.gold()["cases"].items():
        run_kernel_case(name, c["logits"].numpy(), c["tile"], c["H"], c["W"], c["argmax"].numpy(),
                        (c["sample_pixels"].numpy().astype(np.int64), c["sample_probs"].numpy()), c["max_abs_logit"])


def test_seg_sliding_kernel_full_size_18_tiles_vs_restatement():
    """1024 x 2048, tiles of 512^2, 19 x 65 x 65 logits per tile (the student's stride), seeded: no fixture, the restatement
    is the yardstick.  Also the class counts at the edges of the kernel's compile-time bounds on a small geometry."""
    g = np.random.RandomState(17)
    run_kernel_case("full_size", (g.randn(18, 19, 65, 65) * 16).astype(np.float32), (512, 512), 1024, 2048)
    for C in (1, 8, 9, 16, 17, 20, 22, 32):
        run_kernel_case("classes_%d" % C, (g.randn(12, C, 9, 13) * 16).astype(np.float32), (64, 96), 129, 193)
    lg = torch.zeros(1, 33, 2, 2, device=DEV)
    with pytest.raises(ValueError):
        SF.seg_sliding(lg, [(0, 0, 4, 4)], (4, 4), (4, 4))
    with pytest.raises(_lib.SkdLibraryError):
        SF.seg_sliding(torch.zeros(1, 3, 2, 2), [(0, 0, 4, 4)], (4, 4), (4, 4))       # CPU tensors: no fallback


def test_evaluate_main_sliding_vs_reference_fixture_on_gpu():
    """evaluate_main(whole=False) with the generator's FakeNet against the reference's per-image confusion matrices, mean IU
    and IU array (bounds of the CPU test: the convolution runs in another library here); all tiles in one forward and one
    tile per forward agree within the same near-tie cap."""
    G, mod = CPU.gold(), CPU.gen()
    batched = CPU.check_evaluate_main(DEV, G, mod)
    single = CPU.check_evaluate_main(DEV, G, mod, tile_batch=1)
    for a, b in zip(batched, single):
        diff = np.abs(a - b).sum() / 2
        print("tile_batch=None vs 1: %d of %d scored pixels differ" % (diff, a.sum()))
        assert a.sum() == b.sum() and diff <= 1e-5 * a.sum() + 2


class Recording(torch.nn.Module):
    def __init__(self, net):
        super().__init__()
        self.net = net
        self.logits = []

    def forward(self, x):
        out = self.net(x)
        self.logits.append(out[0].detach().float())
        return out


def test_real_student_full_size_sliding_consistency():
    """The real student (Res_pspnet BasicBlock [2, 2, 2, 2], seeded, eval, channels-last like NetModel keeps it) on one seeded
    1024 x 2048 image, tiles of 512^2.  No reference fixture exists for this one: it is a consistency test -- 18 tiles in one
    channels-last forward, finite result, every non-ignored pixel scored once, predict_sliding's array has the reference's
    shape and dtype and its argmax is the kernel's prediction on the same logits."""
    from structure_knowledge_distillation_amd.networks import pspnet_combine
    torch.manual_seed(23)
    S = pspnet_combine.Res_pspnet(pspnet_combine.BasicBlock, [2, 2, 2, 2], 19)
    S = S.to(DEV).to(memory_format=torch.channels_last).eval()
    net = Recording(S)
    g = torch.Generator().manual_seed(29)
    image = torch.randn(1, 3, 1024, 2048, generator=g) * 57.0
    label = torch.randint(0, 19, (1, 1024, 2048), generator=g)
    label[0, 100:300, :700] = 255
    tiles = E.sliding_tiles(1024, 2048, (512, 512))
    assert len(tiles) == 18
    probs = E.predict_sliding(net, image, (512, 512), 19)
    assert len(net.logits) == 1 and net.logits[0].shape[:2] == (18, 19), "all tiles of the image in one forward"
    assert isinstance(probs, np.ndarray) and probs.shape == (1024, 2048, 19) and probs.dtype == np.float64
    assert np.isfinite(probs).all()
    pred, _, cm = SF.seg_sliding(net.logits[0], tiles, (512, 512), (1024, 2048), target=label[0].to(DEV))
    assert np.array_equal(np.argmax(probs, axis=2).astype(np.uint8), pred.cpu().numpy())
    assert int(cm.sum()) == int((label != 255).sum())
    net.logits.clear()
    mean_iu, iu = E.evaluate_main(net, [(image, label, torch.tensor([[1024, 2048, 3]]), ["a"])], "0", "512,512", 19, whole=False)
    assert len(net.logits) == 1 and np.isfinite(mean_iu) and np.isfinite(np.asarray(iu)).all() and 0.0 <= mean_iu <= 1.0
    net.logits.clear()
    E.evaluate_main(net, [(image, label, torch.tensor([[1024, 2048, 3]]), ["a"])], "0", "512,512", 19, whole=False, tile_batch=6)
    assert [t.shape[0] for t in net.logits] == [6, 6, 6]


@pytest.mark.parametrize("whole", [True, False])
def test_test_split_on_gpu(whole, tmp_path):
    """type='test': files named after name[0], mode P, get_palette(256), contents remap[pred]; nothing is scored."""
    CPU.check_test_split(DEV, whole, tmp_path, CPU.gen())
