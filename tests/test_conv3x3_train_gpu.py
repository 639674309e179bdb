"""-m gpu: the training form of the student's 3x3 convolutions (include/skd_train.h, functional.conv3x3_split_train): the
per-step weight split that writes the forward image and the image of the flipped, transposed weight in one launch, the data
gradient as a launch of the split core on that second image, the autograd op and one training step with the routing switched on.

Data gradient: truth is autograd of ``F.conv2d`` in float64 on the CPU.  Error figure of a case: max |got - want| / max |want|
over the whole gradient.  Bound of a case: FOUR times the figure the parent path -- MIOpen's fp32 backward-data kernel through
``aten.convolution_backward`` with mask (True, False, False) -- gave on the same seeded inputs, and never more than 2e-5: the
factor and the cap the forward was accepted under (tests/test_conv3x3_split_gpu.py).  PARENT_DGRAD_ERR holds the parent's figures,
measured once on an MI355X by tools/conv3x3_train_parent_err.py; they and the kernel's own are tabulated in
profiles/r18_conv3x3_train_accuracy.md.  The integer cases must be bit-exact.  Every launch writes into a buffer with sentinel
rows behind row M; both packs of the pack tests sit at their exact size between guard bands (the arena of tests/bounds_cases.py).
"""
import zlib

import pytest
import torch
import torch.nn.functional as F

import bounds_cases as BC
import test_conv3x3_split_gpu as T3
from structure_knowledge_distillation_amd import _lib, functional as SF
from test_conv3x3_split_gpu import CAP, DEV, RATIO, SENTINEL, SLACK_ROWS, P, rel_err

pytestmark = pytest.mark.gpu

# (name, B, Cout -> Cin, H, W, dilation): g is (B, Cout, H, W), dx is (B, Cin, H, W)
DGRAD_CASES = [
    ("dgrad-ragged-13x11-d1", 2, 32, 128, 13, 11, 1),
    ("dgrad-ragged-13x11-d2", 2, 32, 128, 13, 11, 2),
    ("dgrad-ragged-13x11-d4", 2, 32, 128, 13, 11, 4),
    ("dgrad-centre-3x3-d4", 1, 32, 128, 3, 3, 4),
    ("dgrad-longk-512-256-9x9-d4", 1, 512, 256, 9, 9, 4),
    ("dgrad-many-tiles-226x226-d1", 2, 16, 128, 226, 226, 1),
]
DGRAD = {c[0]: c for c in DGRAD_CASES}

# max |parent - want| / max |want| of MIOpen's fp32 backward-data on exactly these inputs, measured once on an MI355X
# (profiles/r18_conv3x3_train_accuracy.md; tools/conv3x3_train_parent_err.py measures them again)
PARENT_DGRAD_ERR = {
    "dgrad-ragged-13x11-d1": 5.646e-07,
    "dgrad-ragged-13x11-d2": 7.168e-07,
    "dgrad-ragged-13x11-d4": 4.634e-07,
    "dgrad-centre-3x3-d4": 1.912e-07,
    "dgrad-longk-512-256-9x9-d4": 4.054e-07,
    "dgrad-many-tiles-226x226-d1": 4.773e-07,
}


@pytest.fixture(scope="module")
def hip():
    return _lib.load()


def dgrad_inputs(name):
    """Seeded output gradient (channels-last) and He-scaled weight of a case."""
    _, b, cout, cin, h, w, _ = DGRAD[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    go = torch.randn(b, cout, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    return go.contiguous(memory_format=torch.channels_last), wt


def dgrad64(go, wt, d):
    """Autograd of F.conv2d in float64 on the CPU: the gradient of the input for the output gradient ``go``."""
    x = torch.zeros(go.shape[0], wt.shape[1], go.shape[2], go.shape[3], dtype=torch.float64, requires_grad=True)
    F.conv2d(x, wt.double(), None, 1, d, d).backward(go.double())
    return x.grad


_WANT = {}


def want_of(name):
    """float64 truth of a case, computed once and shared (never modified)."""
    if name not in _WANT:
        go, wt = dgrad_inputs(name)
        _WANT[name] = dgrad64(go, wt, DGRAD[name][6])
    return _WANT[name]


def pack_pair(hip, wt_dev, fwd=True, bwd=True):
    """(pack_fwd or None, pack_bwd or None) of a device weight view, one launch."""
    cout, cin = wt_dev.shape[:2]
    nbytes = cout * cin * 54
    pf = torch.empty(nbytes, dtype=torch.uint8, device=DEV) if fwd else None
    pb = torch.empty(nbytes, dtype=torch.uint8, device=DEV) if bwd else None
    sn, sc, sy, sx = wt_dev.stride()
    assert hip.skd_conv3x3_split_pack_pair(cin, cout, P(wt_dev), sn, sc, sy, sx, P(pf), nbytes, P(pb), nbytes, None)
    return pf, pb


def launch(hip, x, pk, cout, d):
    """The raw split-core convolution of a channels-last device map on a pack: (B, cout, H, W) on the CPU; checks the sentinel
    rows behind M."""
    b, cin, h, w = x.shape
    m = b * h * w
    out = torch.full((m + SLACK_ROWS, cout), SENTINEL, device=DEV)
    assert hip.skd_conv3x3_split_nhwc(b, h, w, cin, cout, d, P(x), P(pk), P(out), None, None, None, None, None, 0.0, 0, 0.01, 0, None)
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool((out[m:] == SENTINEL).all()), "rows beyond M were written"
    return out[:m].view(b, h, w, cout).permute(0, 3, 1, 2)


def run_dgrad(hip, go, wt, d, wt_format=torch.contiguous_format):
    """dx (B, Cin, H, W) on the CPU: pack_bwd alone from one pack_pair launch, then the data gradient as one launch on it."""
    dg = go.to(DEV).contiguous(memory_format=torch.channels_last)
    dw = wt.to(DEV).contiguous(memory_format=wt_format)
    _, pb = pack_pair(hip, dw, fwd=False)
    return launch(hip, dg, pb, wt.shape[1], d)


# ---- 1. pack bits -------------------------------------------------------------------------------------------------------------

def _weight_view(A, wt, layout):
    """``wt`` (Cout, Cin, 3, 3) on the device between guard bands, as a contiguous tensor, a channels-last one or the channel slice
    [:, 64:] of a weight that is 64 channels wider."""
    if layout == "contiguous":
        return A.inp("w", wt)
    if layout == "channels_last":
        return A.inp("w", wt.permute(0, 2, 3, 1).contiguous()).permute(0, 3, 1, 2)
    wide = torch.cat([torch.full((wt.shape[0], 64, 3, 3), float("nan")), wt], 1)
    return A.inp("w", wide)[:, 64:]


def pack_image(wt):
    """The packed image of a (N, C, 3, 3) fp32 weight as torch computes it on the CPU, from the layout comments of
    csrc/conv_split_dev.hpp and csrc/conv3x3.hip alone: per (column tile tn of 128 rows, K-tile kt of 16 k), tile index
    tn * nk + kt with nk = 9 C / 16, three planes of 256 16-byte chunks; chunk kh * 128 + (row ^ 4 kh) holds the 8 bf16 of
    k = 16 kt + 8 kh + i in ascending i, k = tap * C + c, tap = 3 ty + tx; plane j is piece p_j of v = p0 + p1 + p2,
    p0 = bf16(v), p1 = bf16(v - p0), p2 = bf16(v - p0 - p1), each rounded to nearest even (torch's fp32 -> bf16 cast)."""
    n, c = wt.shape[:2]
    m = wt.permute(0, 2, 3, 1).reshape(n // 128, 128, 9 * c // 16, 2, 8).permute(0, 2, 3, 1, 4)     # (tn, kt, kh, row, i)
    m = torch.stack([m[:, :, 0], m[:, :, 1][:, :, torch.arange(128) ^ 4]], 2).contiguous()          # chunk row' = row ^ 4 kh
    planes = []
    for _ in range(3):
        piece = m.bfloat16()
        planes.append(piece.view(torch.int16))
        m = m - piece.float()
    return torch.stack(planes, 2).contiguous().view(torch.uint8).reshape(-1)                        # (tn, kt, plane, chunk, i)


@pytest.mark.parametrize("layout", ["contiguous", "channels_last", "slice"])
@pytest.mark.parametrize("cout,cin", [(128, 16), (256, 32), (128, 128), (256, 128), (128, 256)])
def test_pack_pair_bits(hip, cout, cin, layout):
    """Both pack entries against pack_image, the torch-on-CPU reference (neither entry is the other's truth: they share one
    kernel).  The backward image is the same function of Wd[c][n][ty][tx] = W[n][c][2 - ty][2 - tx]; it needs Cout a multiple of
    16 and Cin of 128, so the narrow cases take the forward forms only."""
    g = torch.Generator().manual_seed(cout + 3 * cin)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    wt[0, 0, 0, 1], wt[1, 2, 2, 0] = 1e-30, -3.0e4                 # a tiny and a large value: the residual pieces
    nbytes = cout * cin * 54
    want_f = pack_image(wt).to(DEV)
    assert want_f.numel() == nbytes == hip.skd_conv3x3_split_pack_bytes(cin, cout)
    forms = [("weights", True, False), ("pair", True, False)]
    want_b = None
    if cin % 128 == 0:
        want_b = pack_image(wt.flip(2, 3).transpose(0, 1).contiguous()).to(DEV)
        assert want_b.numel() == nbytes == hip.skd_conv3x3_split_pack_bytes(cout, cin) and not torch.equal(want_f, want_b)
        forms += [("pair", True, True), ("pair", False, True)]
    for entry, fwd, bwd in forms:
        A = BC.Arena(DEV)
        w = _weight_view(A, wt, layout)
        assert tuple(w.shape) == (cout, cin, 3, 3) and (layout == "contiguous") == w.is_contiguous()
        pf, pb = A.out("pack_fwd", nbytes, torch.uint8), A.out("pack_bwd", nbytes, torch.uint8)
        sn, sc, sy, sx = w.stride()
        if entry == "weights":
            assert hip.skd_conv3x3_split_pack_weights(cin, cout, P(w), sn, sc, sy, sx, P(pf), nbytes, None)
        else:
            assert hip.skd_conv3x3_split_pack_pair(cin, cout, P(w), sn, sc, sy, sx, P(pf) if fwd else None, nbytes,
                                                   P(pb) if bwd else None, nbytes, None)
        A.check()
        assert torch.equal(pf, want_f) if fwd else bool((pf == BC.FILL).all()), (layout, entry, fwd, bwd)
        assert torch.equal(pb, want_b) if bwd else bool((pb == BC.FILL).all()), (layout, entry, fwd, bwd)


def test_pack_pair_refusals_leave_the_buffers_alone(hip):
    A = BC.Arena(DEV)
    w = A.inp("w", torch.zeros(128, 128, 3, 3))
    n = 128 * 128 * 54
    pf, pb = A.out("pack_fwd", n, torch.uint8), A.out("pack_bwd", n, torch.uint8)
    f = hip.skd_conv3x3_split_pack_pair
    assert not f(128, 128, P(w), 1152, 9, 3, 1, None, n, None, n, None)
    assert not f(128, 128, P(w), 1152, 9, 3, 1, P(pf), n - 1, P(pb), n, None)
    assert not f(128, 128, P(w), 1152, 9, 3, 1, P(pf), n, P(pb), n - 1, None)
    assert not f(128, 128, P(w), -1152, 9, 3, 1, P(pf), n, P(pb), n, None)
    assert not f(128, 64, P(w), 1152, 9, 3, 1, P(pf), n, P(pb), n, None)
    assert not f(128, 128, None, 1152, 9, 3, 1, P(pf), n, P(pb), n, None)
    A.check()
    assert bool((pf == BC.FILL).all()) and bool((pb == BC.FILL).all())


# ---- 2. the data gradient against float64 ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [c[0] for c in DGRAD_CASES])
def test_data_gradient_vs_float64(hip, name):
    go, wt = dgrad_inputs(name)
    got = run_dgrad(hip, go, wt, DGRAD[name][6])
    err = rel_err(got, want_of(name))
    bound = min(RATIO * PARENT_DGRAD_ERR[name], CAP)
    print("%s: err %.3e  parent %.3e  bound %.3e" % (name, err, PARENT_DGRAD_ERR[name], bound))
    assert err <= bound, "%s: max err %.3e > %.3e (parent path: %.3e)" % (name, err, bound, PARENT_DGRAD_ERR[name])


def test_weight_memory_format_does_not_matter_for_the_data_gradient(hip):
    name = "dgrad-ragged-13x11-d2"
    go, wt = dgrad_inputs(name)
    assert torch.equal(run_dgrad(hip, go, wt, 2), run_dgrad(hip, go, wt, 2, wt_format=torch.channels_last))


# ---- 3. integers are exact ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(2, 13, 11, 2), (1, 5, 5, 4), (2, 40, 37, 1)], ids=["13x11-d2", "5x5-d4", "40x37-d1"])
def test_integer_data_gradient_bit_exact(hip, shape):
    b, h, w, d = shape
    cout, cin = 32, 128                    # the data gradient's K is 9 * Cout, its N is Cin
    assert 9 * cout * 7 * 3 < 2 ** 24      # every partial sum is an exact fp32 integer, in any order
    g = torch.Generator().manual_seed(100 * h + d + 1)
    go = torch.randint(-7, 8, (b, cout, h, w), generator=g).float().contiguous(memory_format=torch.channels_last)
    wt = torch.randint(-3, 4, (cout, cin, 3, 3), generator=g).float()
    got = run_dgrad(hip, go, wt, d)
    want = dgrad64(go, wt, d)
    assert float(want.abs().max()) > 100.0
    assert torch.equal(got.double(), want), "%d of %d gradients differ" % (int((got.double() != want).sum()), got.numel())


# ---- 4. adjointness on integers -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [1, 2, 4])
def test_forward_and_data_gradient_are_adjoint_on_integers(hip, d):
    """sum conv(x) . g == sum x . dgrad(g), exactly: pins the flip and the transposition without torch's backward.  Cin != Cout, so
    a forgotten transposition cannot even be launched on the right shapes; the taps are asymmetric (random), so a forgotten flip
    changes the sum."""
    b, cin, cout, h, w = 2, 128, 256, 13, 11
    g = torch.Generator().manual_seed(77 + d)
    x = torch.randint(-7, 8, (b, cin, h, w), generator=g).float().contiguous(memory_format=torch.channels_last)
    go = torch.randint(-7, 8, (b, cout, h, w), generator=g).float().contiguous(memory_format=torch.channels_last)
    wt = torch.randint(-3, 4, (cout, cin, 3, 3), generator=g).float()
    assert 9 * max(cin, cout) * 7 * 3 < 2 ** 24
    pf, pb = pack_pair(hip, wt.to(DEV))
    y = launch(hip, x.to(DEV), pf, cout, d)
    dx = launch(hip, go.to(DEV), pb, cin, d)
    lhs, rhs = float((y.double() * go.double()).sum()), float((x.double() * dx.double()).sum())
    assert lhs == rhs and abs(lhs) > 1000.0, (lhs, rhs)
    assert torch.equal(y.double(), F.conv2d(x.double(), wt.double(), None, 1, d, d))


# ---- 5. the op ------------------------------------------------------------------------------------------------------------------

def _op_case(bias):
    g = torch.Generator().manual_seed(1234 + int(bias))
    b, c, h, w, d = 2, 128, 13, 11, 2
    x = torch.relu(torch.randn(b, c, h, w, generator=g) + torch.randn(1, c, 1, 1, generator=g) * 0.5)
    wt = torch.randn(c, c, 3, 3, generator=g) * (2.0 / (9 * c)) ** 0.5
    bs = torch.randn(c, generator=g) * 0.2 if bias else None
    go = torch.randn(b, c, h, w, generator=g)
    cl = lambda t: t.to(DEV).contiguous(memory_format=torch.channels_last)
    return cl(x), cl(wt), None if bs is None else bs.to(DEV), cl(go), d


@pytest.mark.parametrize("bias", [False, True], ids=["no-bias", "bias"])
def test_op_bits_and_weight_gradient(hip, bias):
    x, wt, bs, go, d = _op_case(bias)
    owner = torch.nn.Module()
    xg, wg = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    bg = None if bs is None else bs.clone().requires_grad_(True)
    assert SF.conv3x3_train_supported(xg, wg, 1, d, d, 1)
    with torch.no_grad():
        assert not SF.conv3x3_train_supported(xg, wg, 1, d, d, 1)
    assert not SF.conv3x3_train_supported(xg.contiguous(), wg, 1, d, d, 1) and not SF.conv3x3_train_supported(xg, wg, 2, d, d, 1)
    y = SF.conv3x3_split_train(xg, wg, d, bg, owner=owner)
    assert y.is_contiguous(memory_format=torch.channels_last) and y.requires_grad
    with torch.no_grad():
        raw = SF.conv3x3_split_eval(x, SF.conv3x3_pack_weights(None, wt, torch.nn.Module()), 128, d, bs)
    assert torch.equal(y.detach(), raw), "the forward is the inference launch, bit for bit"
    ins = (xg, wg) + (() if bg is None else (bg,))
    first = torch.autograd.grad(y, ins, go, retain_graph=True)
    second = torch.autograd.grad(y, ins, go)
    _, pb = pack_pair(hip, wt, fwd=False)
    entry = launch(hip, go, pb, 128, d)
    assert torch.equal(first[0].cpu(), entry), "dx is the entry-level launch on pack_bwd, bit for bit"
    assert torch.equal(first[0], second[0]), "two backward runs give the same dx bits"
    assert first[0].is_contiguous(memory_format=torch.channels_last)
    # a gradient that is not fp32 channels-last is made so first
    third = torch.autograd.grad(SF.conv3x3_split_train(xg, wg, d, bg, owner=owner), xg, go.contiguous())
    assert torch.equal(third[0], first[0])
    # dw / dbias: the library's kernels, as in plain F.conv2d's autograd
    x64, w64 = x.cpu().double().requires_grad_(True), wt.cpu().double().requires_grad_(True)
    b64 = None if bs is None else bs.cpu().double().requires_grad_(True)
    want = torch.autograd.grad(F.conv2d(x64, w64, b64, 1, d, d), (x64, w64) + (() if b64 is None else (b64,)), go.cpu().double())
    plain = torch.autograd.grad(F.conv2d(xg, wg, bg, 1, d, d), ins, go)
    for k, what in list(enumerate(("dx", "dw", "dbias")))[1:len(ins)]:
        err = float((first[k].cpu().double() - want[k]).norm())
        base = float((plain[k].cpu().double() - want[k]).norm())
        norm = float(want[k].norm())
        print("%s: op %.3e  plain autograd %.3e  (of |want| = %.3e)" % (what, err, base, norm))
        assert first[k].shape == ins[k].shape and err <= 4.0 * base + 1e-6 * norm, (what, err, base, norm)
    # needs_input_grad: an input without a gradient gets none, and nothing raises
    y2 = SF.conv3x3_split_train(x, wg, d, bg, owner=owner)
    (dw2,) = torch.autograd.grad(y2, wg, go)
    assert dw2.shape == wg.shape
    y3 = SF.conv3x3_split_train(xg, wt, d, bs, owner=owner)
    (dx3,) = torch.autograd.grad(y3, xg, go)
    assert torch.equal(dx3, first[0])


# ---- 6. weight updates ----------------------------------------------------------------------------------------------------------

def test_weight_update_between_forwards():
    x, wt, _, go, d = _op_case(False)
    conv = torch.nn.Module()
    w = wt.clone().requires_grad_(True)
    xg = x.clone().requires_grad_(True)
    y0 = SF.conv3x3_split_train(xg, w, d, owner=conv)
    packs0 = SF.conv3x3_train_packs(w, conv)
    assert SF.conv3x3_train_packs(w, conv)[0] is packs0[0], "one split per weight version"
    (dx0,) = torch.autograd.grad(y0, xg, go, retain_graph=True)
    with torch.no_grad():
        w.add_(torch.randn(w.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(9)) * 0.05)
    # a backward whose forward ran before the update: autograd's version check on the saved weight, not a silent new pack
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        torch.autograd.grad(y0, xg, go)
    y1 = SF.conv3x3_split_train(xg, w, d, owner=conv)
    packs1 = SF.conv3x3_train_packs(w, conv)
    assert packs1[0] is not packs0[0] and not torch.equal(packs1[1], packs0[1])
    (dx1,) = torch.autograd.grad(y1, xg, go)
    fresh = w.detach().clone().requires_grad_(True)                # fresh packs of the new weight, no owner: no cache
    yf = SF.conv3x3_split_train(xg, fresh, d)
    (dxf,) = torch.autograd.grad(yf, xg, go)
    assert torch.equal(y1.detach(), yf.detach()) and torch.equal(dx1, dxf)
    assert not torch.equal(y1.detach(), y0.detach()) and not torch.equal(dx1, dx0), "the stale result differs"


def test_fused_sgd_step_rebuilds_the_packs():
    """The optimizer NetModel uses on the GPU -- torch's fused SGD -- leaves ``_version`` alone; with the step post-hook NetModel
    registers, the forward behind a step runs on the new weights' packs."""
    from structure_knowledge_distillation_amd.networks.kd_model import advance_versions_after_step
    x, wt, _, go, d = _op_case(False)
    w = torch.nn.Parameter(wt.clone())
    owner = torch.nn.Module()
    opt = torch.optim.SGD([w], 0.5, momentum=0.9, fused=True)
    y0 = SF.conv3x3_split_train(x, w, d, owner=owner)
    y0.backward(go)
    version = w._version
    opt.step()
    if w._version == version:                                       # this torch: the version did not move, and without the hook
        stale = SF.conv3x3_split_train(x, w, d, owner=owner)        # the next forward runs on the old packs
        assert torch.equal(stale.detach(), y0.detach())
    opt.register_step_post_hook(advance_versions_after_step)
    opt.step()
    assert w._version > version
    y1 = SF.conv3x3_split_train(x, w, d, owner=owner)
    fresh = SF.conv3x3_split_train(x, w.detach().clone(), d)
    assert torch.equal(y1.detach(), fresh.detach()) and not torch.equal(y1.detach(), y0.detach())


# ---- 7. the step ----------------------------------------------------------------------------------------------------------------

def test_step_config1_with_the_training_form(monkeypatch):
    """The config-1 step of tests/test_step_gpu.py (batch 2, 256 x 256, 33 x 33 maps, Pi + Pa) with ``split_train`` on, against the
    same fixtures at exactly the bounds of test_step_config1_vs_reference_golden: that test's own body runs, with the switch set
    where its ``default_args`` reads it.  A counting shim sees 13 forward calls and 13 data-gradient launches; off, none."""
    import test_step_gpu as TS
    real_op, real_launch = SF.conv3x3_split_train, SF._conv3x3_raw_launch
    seen = {"forward": 0, "bwd_packs": set(), "fwd_packs": set(), "launch_fwd": 0, "launch_bwd": 0}

    def op(x, weight, dilation, bias=None, owner=None, **kw):
        seen["forward"] += 1
        out = real_op(x, weight, dilation, bias, owner, **kw)
        pf, pb = SF.conv3x3_train_packs(weight, owner)             # the cached pair this forward used
        seen["fwd_packs"].add(pf.data_ptr())
        seen["bwd_packs"].add(pb.data_ptr())
        return out

    def launch_(form, x, pack, cout, dilation, conv_bias=None):      # training's one raw launcher: the wide launches by their entry
        if form.conv != "skd_conv3x3_narrow_nhwc":
            seen["launch_bwd" if pack.data_ptr() in seen["bwd_packs"] else "launch_fwd"] += 1
        return real_launch(form, x, pack, cout, dilation, conv_bias)
    monkeypatch.setattr(SF, "conv3x3_split_train", op)
    monkeypatch.setattr(SF, "_conv3x3_raw_launch", launch_)

    monkeypatch.setenv("SKD_SPLIT_TRAIN", "0")
    model, _, _ = TS._config1_step(pa=True)
    assert not model.split_train and seen["forward"] == seen["launch_fwd"] == seen["launch_bwd"] == 0
    del model

    monkeypatch.setenv("SKD_SPLIT_TRAIN", "1")
    TS.test_step_config1_vs_reference_golden()
    assert seen["forward"] == 13 and seen["launch_fwd"] == 13 and seen["launch_bwd"] == 13, seen
    assert len(seen["bwd_packs"]) == 13 and not seen["bwd_packs"] & seen["fwd_packs"]
