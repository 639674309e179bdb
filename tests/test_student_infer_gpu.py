"""-m gpu: the student's fused inference path -- ``skd_conv3x3_split_res_nhwc`` (include/skd_infer.h; csrc/conv3x3.hip with the
residual in its epilogue), flagged BasicBlocks and the whole flagged student.

Error figure everywhere: max |got - want| / max |want| against a float64 result, except for the whole-student records, which
are strided samples (the ``_rec_err`` estimate of tests/test_step_gpu.py).  Bounds:
  * no residual: the bits of ``skd_conv3x3_split_nhwc``; with a residual r: the bits of act(z + r) in fp32, z that entry's
    ``activation = none`` output -- the residual add is a separate fp32 add behind the BN expression;
  * integer data: equality with float64 ``F.conv2d + r``;
  * random data: the bound of tests/test_conv3x3_split_gpu.py -- four times the error of the fp32 ``F.conv2d`` composition on
    the same GPU and the same inputs, and never more than 2e-5;
  * blocks and the whole student: the flagged form's error at most four times the unflagged form's on the same GPU.
Every figure is printed in front of its assertion.
"""
import ctypes
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from structure_knowledge_distillation_amd import _lib, functional as SF
from structure_knowledge_distillation_amd.networks import fuse_for_inference, pspnet_combine as PC

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(HERE, "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)
import bounds_cases as BC  # noqa: E402  (Arena: guard-banded buffers)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
P = BC.P
CAP, RATIO = 2e-5, 4.0
ACT = {"none": 0, "leaky_relu": 1, "relu": 3}
EPS, SLOPE = 1e-5, 0.01
# (B, H, W, Cin, Cout, dilation): M = 420 = three 128-row panels + 36 rows, two column tiles | M = 126: one partial tile whose rows
# cross the image boundary | 5 x 6 at dilation 4: most taps masked
SHAPES = {"20x21-d2": (1, 20, 21, 32, 256, 2), "7x9-d1": (2, 7, 9, 16, 128, 1), "5x6-d4": (2, 5, 6, 16, 128, 4)}


@pytest.fixture(scope="module")
def hip():
    return _lib.load()


def pack_into(hip, wt_dev, buf=None):
    cout, cin = wt_dev.shape[:2]
    nbytes = hip.skd_conv3x3_split_pack_bytes(cin, cout)
    assert nbytes == cout * cin * 54
    buf = torch.empty(nbytes, dtype=torch.uint8, device=DEV) if buf is None else buf
    sn, sc, sy, sx = wt_dev.stride()
    assert hip.skd_conv3x3_split_pack_weights(cin, cout, P(wt_dev), sn, sc, sy, sx, P(buf), nbytes, None)
    return buf


_DATA = {}


def data(name, integers=False):
    """Seeded inputs of a shape, on the device, made once and never modified: x (B, H, W, Cin), weight, residual (M, Cout), BN."""
    key = (name, integers)
    if key not in _DATA:
        b, h, w, cin, cout, d = SHAPES[name]
        g = torch.Generator().manual_seed(1000 * h + 10 * w + d + int(integers))
        if integers:
            assert 9 * cin * 7 * 3 + 50 < 2 ** 24                       # every partial sum is an exact fp32 integer
            x = torch.randint(-7, 8, (b, h, w, cin), generator=g).float()
            wt = torch.randint(-3, 4, (cout, cin, 3, 3), generator=g).float()
            r = torch.randint(-50, 51, (b * h * w, cout), generator=g).float()
        else:
            x = torch.relu(torch.randn(b, h, w, cin, generator=g) + torch.randn(1, 1, 1, cin, generator=g) * 0.5)
            wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
            r = torch.randn(b * h * w, cout, generator=g)
        bn = dict(mean=torch.randn(cout, generator=g) * 0.3, var=torch.rand(cout, generator=g) + 0.5,
                  gamma=torch.randn(cout, generator=g), beta=torch.randn(cout, generator=g))
        d_ = dict(x=x.to(DEV), wt=wt.to(DEV), r=r.to(DEV), bn={k: v.to(DEV) for k, v in bn.items()})
        d_["pack"] = pack_into(_lib.load(), d_["wt"])
        _DATA[key] = d_
    return _DATA[key]


def launch(hip, name, d, act, geometry=0, residual=None, bn=True, entry="res"):
    """One launch into a fresh NaN-filled (M, Cout) buffer; ``entry='old'``: skd_conv3x3_split_nhwc."""
    b, h, w, cin, cout, dil = SHAPES[name]
    out = torch.full((b * h * w, cout), float("nan"), device=DEV)
    s = d["bn"] if bn else dict(mean=None, var=None, gamma=None, beta=None)
    tail = (None, P(s["mean"]), P(s["var"]), P(s["gamma"]), P(s["beta"]), EPS if bn else 0.0, ACT[act], SLOPE, geometry, None)
    if entry == "old":
        assert residual is None
        assert hip.skd_conv3x3_split_nhwc(b, h, w, cin, cout, dil, P(d["x"]), P(d["pack"]), P(out), *tail)
    else:
        assert hip.skd_conv3x3_split_res_nhwc(b, h, w, cin, cout, dil, P(d["x"]), P(d["pack"]), P(out), P(residual), *tail)
    return out


def act32(z, act):
    if act == "relu":
        return torch.where(z < 0, torch.zeros_like(z), z)
    if act == "leaky_relu":
        return torch.where(z < 0, z * SLOPE, z)
    return z


def want64(name, d, act, bn=True):
    """float64 truth on the CPU: (M, Cout)."""
    b, h, w, cin, cout, dil = SHAPES[name]
    y = F.conv2d(d["x"].cpu().double().permute(0, 3, 1, 2), d["wt"].cpu().double(), None, 1, dil, dil).permute(0, 2, 3, 1).reshape(-1, cout)
    if bn:
        s = {k: v.cpu().double() for k, v in d["bn"].items()}
        y = (y - s["mean"]) / torch.sqrt(s["var"] + EPS) * (s["gamma"].abs() + EPS) + s["beta"]
    y = y + d["r"].cpu().double()
    return torch.where(y < 0, y * (SLOPE if act == "leaky_relu" else 0.0), y) if act != "none" else y


def rel_err(got, want):
    got = got.detach().cpu().double()
    assert bool(torch.isfinite(got).all())
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-30)


# ---- 1. bit identity with the existing entry -----------------------------------------------------------------------------

@pytest.mark.parametrize("act", ["none", "relu", "leaky_relu"])
def test_bits_of_the_existing_entry(hip, act):
    name = "20x21-d2"
    d = data(name)
    z = launch(hip, name, d, "none", entry="old")                     # the BN expression's fp32 value
    want_res = act32(z + d["r"], act)
    old = launch(hip, name, d, act, entry="old")
    assert bool(torch.isfinite(z).all()) and (act == "none" or not torch.equal(old, z))
    for geometry in range(4):
        assert torch.equal(launch(hip, name, d, act, geometry, entry="old"), old)
        assert torch.equal(launch(hip, name, d, act, geometry, residual=None), old), "residual = NULL is the existing entry"
        got = launch(hip, name, d, act, geometry, residual=d["r"])
        assert torch.equal(got, want_res), "%d of %d outputs differ from act(z + r)" % (int((got != want_res).sum()), got.numel())
    assert not torch.equal(want_res, old)


# ---- 2. exactness on integer data ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["7x9-d1", "5x6-d4"])
def test_integers_bit_exact_with_residual(hip, name):
    d = data(name, integers=True)
    want = want64(name, d, "none", bn=False)
    assert float(want.abs().max()) > 100.0
    for geometry in range(4):
        got = launch(hip, name, d, "none", geometry, residual=d["r"], bn=False).cpu().double()
        assert torch.equal(got, want), "%d of %d outputs differ" % (int((got != want).sum()), got.numel())
    relu = launch(hip, name, d, "relu", residual=d["r"], bn=False).cpu().double()
    assert torch.equal(relu, torch.relu(want)) and bool((want < 0).any())


# ---- 3. accuracy ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(SHAPES))
def test_accuracy_bn_relu_residual(hip, name):
    b, h, w, cin, cout, dil = SHAPES[name]
    d = data(name)
    want = want64(name, d, "relu")
    s = d["bn"]
    y = F.conv2d(d["x"].permute(0, 3, 1, 2), d["wt"].contiguous(memory_format=torch.channels_last), None, 1, dil, dil)
    y = y.permute(0, 2, 3, 1).reshape(-1, cout)
    y = ((y - s["mean"]) * (1.0 / torch.sqrt(s["var"] + EPS))) * (s["gamma"].abs() + EPS) + s["beta"]
    parent = rel_err(torch.relu(y + d["r"]), want)
    bound = min(RATIO * parent, CAP)
    for geometry in range(4):
        err = rel_err(launch(hip, name, d, "relu", geometry, residual=d["r"]), want)
        print("%s geometry %d: err %.3e  fp32 composition %.3e  bound %.3e" % (name, geometry, err, parent, bound))
        assert err <= bound, "%s: max err %.3e > %.3e (fp32 composition: %.3e)" % (name, err, bound, parent)


# ---- 4. guard bands --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,geometry", [("20x21-d2", 0), ("20x21-d2", 1), ("20x21-d2", 3), ("7x9-d1", 0), ("5x6-d4", 2)])
def test_guard_bands(hip, name, geometry):
    """Input, packed weights, residual (exactly M * Cout floats) and output between 0xFF guards (NaN as fp32): no guard byte
    changes, and neither a stray read nor an unwritten element leaves a NaN in the output."""
    b, h, w, cin, cout, dil = SHAPES[name]
    d = data(name)
    A = BC.Arena("cuda")
    x = A.inp("x", d["x"].cpu(), row=cin)
    wt = A.inp("weight", d["wt"].cpu())
    pk = A.out("pack", hip.skd_conv3x3_split_pack_bytes(cin, cout), torch.uint8)
    r = A.inp("residual", d["r"].cpu(), row=cout)
    assert r.numel() == b * h * w * cout
    bn = {k: A.inp(k, v.cpu()) for k, v in d["bn"].items()}
    out = A.out("out", (b * h * w, cout), row=cout)
    pack_into(hip, wt, pk)
    A.check()
    assert torch.equal(pk, d["pack"])
    assert hip.skd_conv3x3_split_res_nhwc(b, h, w, cin, cout, dil, P(x), P(pk), P(out), P(r), None, P(bn["mean"]), P(bn["var"]),
                                          P(bn["gamma"]), P(bn["beta"]), EPS, ACT["relu"], SLOPE, geometry, None) == 1
    A.check()
    assert not bool(torch.isnan(out).any())
    assert torch.equal(out, launch(hip, name, d, "relu", geometry, residual=d["r"]))
    # the residual may not overlap the output: refused on the host, nothing is written
    before = out.clone()
    assert hip.skd_conv3x3_split_res_nhwc(b, h, w, cin, cout, dil, P(x), P(pk), P(out), P(out), None, None, None, None, None, 0.0, 0,
                                          SLOPE, geometry, None) == 0
    A.check()
    assert torch.equal(out, before)


# ---- 5. blocks ---------------------------------------------------------------------------------------------------------------

def _randomise(mod, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in mod.modules():
            if hasattr(m, "running_mean"):
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.3)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
                m.weight.copy_(torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
    return mod


def _bn64(y, bn):
    v = lambda t: t.detach().cpu().double().view(1, -1, 1, 1)
    return (y - v(bn.running_mean)) / torch.sqrt(v(bn.running_var) + bn.eps) * (v(bn.weight).abs() + bn.eps) + v(bn.bias)


def block64(block, x):
    """The reference op sequence of a BasicBlock (pspnet_combine.py:46-62 of the reference) in float64 on the CPU."""
    x = x.double()
    c = lambda conv, t: F.conv2d(t, conv.weight.detach().cpu().double(), None, conv.stride, conv.padding, conv.dilation)
    out = torch.relu(_bn64(c(block.conv1, x), block.bn1))
    out = _bn64(c(block.conv2, out), block.bn2)
    res = x if block.downsample is None else _bn64(c(block.downsample[0], x), block.downsample[1])
    return torch.relu(out + res)


@pytest.mark.parametrize("cin,planes,dil", [(256, 256, 2), (512, 512, 4), (128, 256, 2)])
def test_flagged_block_vs_float64(cin, planes, dil):
    torch.manual_seed(cin + planes)
    down = None
    if cin != planes:
        down = torch.nn.Sequential(torch.nn.Conv2d(cin, planes, 1, 1, bias=False), PC.BatchNorm2d(planes, affine=True))
    block = _randomise(PC.BasicBlock(cin, planes, dilation=dil, downsample=down), cin).eval()
    x = torch.relu(torch.randn(2, cin, 13, 17, generator=torch.Generator().manual_seed(dil)))
    want = block64(block, x)
    block = block.to(DEV).to(memory_format=torch.channels_last)
    dx = x.to(DEV).contiguous(memory_format=torch.channels_last)
    calls = []
    with torch.no_grad():
        plain = block(dx.clone())
        assert fuse_for_inference(block) is block
        _lib.enable_kernel_timing(["skd_conv3x3_split_nhwc", "skd_conv3x3_split_res_nhwc"])
        try:
            fused = block(dx.clone())
        finally:
            calls = _lib.disable_kernel_timing()
    assert len(calls["skd_conv3x3_split_nhwc"]) == 1 and len(calls["skd_conv3x3_split_res_nhwc"]) == 1, "both convolutions fused"
    assert fused.shape == plain.shape and fused.is_contiguous(memory_format=torch.channels_last)
    e_plain, e_fused = rel_err(plain, want), rel_err(fused, want)
    print("BasicBlock(%d, %d, d=%d): unflagged %.3e  flagged %.3e  ratio %.2f" % (cin, planes, dil, e_plain, e_fused, e_fused / e_plain))
    assert e_fused <= RATIO * e_plain


# ---- 6. the whole student ------------------------------------------------------------------------------------------------

def _rec_err(t, rec):
    f = t.detach().cpu().double().reshape(-1)
    assert list(t.shape) == rec["shape"], (tuple(t.shape), rec["shape"])
    s = f[::rec["step"]][:rec["sample"].numel()]
    return float((s - rec["sample"]).norm()) * math.sqrt(f.numel() / s.numel())


def test_whole_student_vs_float64_fixture():
    import make_golden_student_infer as G
    fx = torch.load(G.OUT, weights_only=False)
    assert os.path.getsize(G.OUT) <= 400 * 1024 and fx["names"] == G.NAMES
    Pw, x = G.inputs()
    for k, v in G.checksum(Pw).items():
        assert abs(v - fx["checksums"][k]) <= 1e-9 * max(1.0, abs(v)), ("weight RNG drifted from the fixture generator's", k)
    S = PC.Res_pspnet(PC.BasicBlock, [2, 2, 2, 2], 19)
    S.load_state_dict(Pw)
    S = S.to(DEV).to(memory_format=torch.channels_last).eval()
    dx = x.to(DEV).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        plain = S(dx)
        _lib.enable_kernel_timing(["skd_conv3x3_split_res_nhwc"])
        try:
            fused = fuse_for_inference(S)(dx)
        finally:
            calls = _lib.disable_kernel_timing()
    assert len(calls["skd_conv3x3_split_res_nhwc"]) == 6, "layer2, layer3 and layer4: one residual launch per block"
    for name, a, b, r in zip(fx["names"], plain, fused, fx["outputs"]):
        e_plain, e_fused = _rec_err(a, r), _rec_err(b, r)
        print("%-18s unflagged %.3e  flagged %.3e of the norm, ratio %.2f" % (name, e_plain / r["norm"], e_fused / r["norm"], e_fused / e_plain))
        assert e_fused <= RATIO * e_plain, name


# ---- 7. full size --------------------------------------------------------------------------------------------------------

def test_evaluate_main_full_size_flagged_student(monkeypatch):
    """evaluate_main on the flagged student at 1024 x 2048 against tests/golden/gpu_suite_oracle.pt["eval_full"], at the bounds of
    test_evaluate_main_full_size_student_on_gpu; clearing the flag gives the unflagged logits back bit for bit."""
    import numpy as np
    import make_golden_gpu_suite as gen
    from structure_knowledge_distillation_amd.networks import evaluate as E
    fx = torch.load(os.path.join(HERE, "golden", "gpu_suite_oracle.pt"), weights_only=False)["eval_full"]
    Pw, image, label, size = gen.eval_full_inputs()
    for k, v in gen.checksum(Pw).items():
        assert abs(v - fx["checksums"][k]) <= 1e-9 * max(1.0, abs(v)), ("weight RNG drifted from the fixture generator's", k)
    S = PC.Res_pspnet(PC.BasicBlock, [2, 2, 2, 2], 19)
    S.load_state_dict(Pw)
    S = S.to(DEV).to(memory_format=torch.channels_last).eval()
    dx = image.to(DEV).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        before = S(dx)[0].clone()
    scored, real = [], E.iou_from_confusion
    monkeypatch.setattr(E, "iou_from_confusion", lambda cm: (scored.append(int(cm.sum())), real(cm))[1])
    _lib.enable_kernel_timing(["skd_conv3x3_split_res_nhwc"])
    try:
        mean_iu, iu = E.evaluate_main(fuse_for_inference(S), [(image, label, size, ["a"])], "0", "1024,2048", 19, whole=True)
    finally:
        calls = _lib.disable_kernel_timing()
    assert len(calls["skd_conv3x3_split_res_nhwc"]) == 6, "the evaluation ran the fused blocks"
    cm = fx["confusion"].numpy()
    assert int(cm.sum()) == fx["pixels"]
    want_mean, want_iu = real(cm)
    assert scored == [fx["pixels"]], "the same scored-pixel count"
    print("full-size evaluation, flagged student: mean IU gpu %.6f oracle %.6f, worst class %.2e"
          % (mean_iu, want_mean, np.abs(np.asarray(iu) - np.asarray(want_iu)).max()))
    assert abs(mean_iu - want_mean) < 1e-3 and np.abs(np.asarray(iu) - np.asarray(want_iu)).max() < 2e-3
    S.eval()
    with torch.no_grad():
        flagged = S(dx)[0].clone()
        after = fuse_for_inference(S, enable=False)(dx)[0]
    assert not torch.equal(flagged, before), "the flag changed nothing"
    assert torch.equal(after, before)
