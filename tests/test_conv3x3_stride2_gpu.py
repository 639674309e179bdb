"""-m gpu: the stride-2 forward form of the split-core 3x3 convolution (csrc/conv3x3.hip with STRIDE = 2, include/skd_stride2.h),
the frozen teacher flagged by ``route_teacher_early`` and the student flagged by ``fuse_for_inference(stride2=True)``.

The main test has NO tolerance: the form changes the row map of the stride-1 kernel and nothing else, so ``s2(x)`` must be
``skd_conv3x3_split_nhwc(x)[:, ::2, ::2, :]`` bit for bit (``skd_conv3x3_split2_nhwc`` for two pieces) -- raw and with the
bias + BN + ReLU epilogue, for every geometry, on shapes with odd and even sizes, a last output row / column whose bottom / right
taps fall outside, M below one tile, tiles that cross images, a ragged last tile and two column tiles.  Integer data must be
bit-exact against float64 ``F.conv2d(stride=2, padding=1)``.

Against float64 on random data: figure max |got - want| / max |want| over the whole output; bound FOUR times the figure of the
library path -- MIOpen's fp32 ``F.conv2d(stride=2)`` on the GPU, followed by the library's eval-mode ABN pass where the case has
the epilogue -- on the same inputs, and never more than 2e-5 (the contract of DESIGN.md 7.4 / 7.5).  PARENT_ERR holds the library's
figures, measured on an MI355X by tools/conv3x3_stride2_parent_err.py and tabulated with the kernel's own in
profiles/r27_conv3x3_stride2_accuracy.md.  Every launch writes into a buffer with 160 sentinel rows behind row M; the guard-band
cases put every buffer between 0xFF bands (the arena of tests/bounds_cases.py).  Every figure is printed in front of its assertion.
"""
import os
import sys
import zlib

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(HERE, "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)
import bounds_cases as BC  # noqa: E402
import split2_ref as R  # noqa: E402
import test_conv3x3_split_gpu as T3  # noqa: E402
from structure_knowledge_distillation_amd import _lib, functional as SF, networks  # noqa: E402
from structure_knowledge_distillation_amd.networks import pspnet_combine as PC  # noqa: E402
from test_conv3x3_split_gpu import ACT, CAP, DEV, RATIO, SENTINEL, SLACK_ROWS, P, epilogue64, rel_err  # noqa: E402

pytestmark = pytest.mark.gpu

S2, WIDE, WIDE2, NARROW = "skd_conv3x3_split_s2_nhwc", "skd_conv3x3_split_nhwc", "skd_conv3x3_split2_nhwc", "skd_conv3x3_narrow_nhwc"
# (B, H, W, Cin, Cout): odd sizes | even sizes: the last output row and column lose their bottom / right taps | M = 105 on 13 x 10,
# two column tiles, rows cross images | M = 70 on 10 x 13 at the longest K | M = 1 | M = 1 with only the four lower-right taps
SHAPES = [(2, 5, 5, 16, 128), (2, 6, 6, 32, 128), (3, 13, 10, 64, 256), (2, 10, 13, 128, 128), (1, 1, 1, 16, 128), (1, 2, 2, 16, 128)]
IDS = ["%dx%dx%d-%d-%d" % s for s in SHAPES]
EPILOGUES = ("raw", "bias-bn-relu")
RAGGED = [SHAPES[2], SHAPES[3]]

# max |library - want| / max |want| of the library path on exactly these inputs, measured on an MI355X
# (profiles/r27_conv3x3_stride2_accuracy.md; tools/conv3x3_stride2_parent_err.py measures them again on these inputs)
PARENT_ERR = {
    "s2-2x5x5-16-128-raw": 3.002e-07,
    "s2-2x5x5-16-128-bias-bn-relu": 2.388e-07,
    "s2-2x6x6-32-128-raw": 3.077e-07,
    "s2-2x6x6-32-128-bias-bn-relu": 2.829e-07,
    "s2-3x13x10-64-256-raw": 2.922e-07,
    "s2-3x13x10-64-256-bias-bn-relu": 2.523e-07,
    "s2-2x10x13-128-128-raw": 3.309e-07,
    "s2-2x10x13-128-128-bias-bn-relu": 3.044e-07,
    "s2-1x1x1-16-128-raw": 3.097e-08,
    "s2-1x1x1-16-128-bias-bn-relu": 4.451e-08,
    "s2-1x2x2-16-128-raw": 2.801e-08,
    "s2-1x2x2-16-128-bias-bn-relu": 6.823e-08,
}


@pytest.fixture(scope="module")
def hip():
    return _lib.load()


def case_name(shape, epi):
    return "s2-%dx%dx%d-%d-%d-%s" % (shape + (epi,))


def case_inputs(shape, epi, integers=False):
    """Seeded inputs of a case by the recipe of tests/test_conv3x3_split_gpu.py: ReLU-like activations with per-channel offsets,
    He-scaled weights, epilogue parameters; ``integers``: small integers whose every partial sum is an exact fp32 integer."""
    b, h, w, cin, cout = shape
    g = torch.Generator().manual_seed(zlib.crc32(case_name(shape, epi).encode()) + int(integers))
    if integers:
        assert 9 * cin * 7 * 3 < 2 ** 24
        x = torch.randint(-7, 8, (b, cin, h, w), generator=g).float()
        wt = torch.randint(-3, 4, (cout, cin, 3, 3), generator=g).float()
    else:
        x = torch.relu(torch.randn(b, cin, h, w, generator=g) + torch.randn(1, cin, 1, 1, generator=g) * 0.5)
        wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    p = {"cbias": None, "mean": None, "var": None, "gamma": None, "beta": None, "eps": 0.0, "act": "none"}
    if epi != "raw":
        p.update(cbias=torch.randn(cout, generator=g) * 0.2, mean=torch.randn(cout, generator=g) * 0.3, var=torch.rand(cout, generator=g) + 0.5,
                 gamma=torch.randn(cout, generator=g), beta=torch.randn(cout, generator=g), eps=1e-5, act="relu")
    return x.contiguous(memory_format=torch.channels_last), wt, p


_WANT = {}


def want_of(shape, epi):
    """float64 truth of a case on the CPU, computed once and shared (never modified)."""
    key = case_name(shape, epi)
    if key not in _WANT:
        x, wt, p = case_inputs(shape, epi)
        y = F.conv2d(x.double(), wt.double(), None if p["cbias"] is None else p["cbias"].double(), 2, 1, 1)
        _WANT[key] = epilogue64(y, p)
    return _WANT[key]


def pack_of(hip, wt_dev, pieces):
    cout, cin = wt_dev.shape[:2]
    size, entry = ((hip.skd_conv3x3_split_pack_bytes, hip.skd_conv3x3_split_pack_weights) if pieces == 3
                   else (hip.skd_conv3x3_split2_pack_bytes, hip.skd_conv3x3_split2_pack_weights))
    nbytes = size(cin, cout)
    assert nbytes == cout * cin * 18 * pieces
    buf = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    assert entry(cin, cout, P(wt_dev), *wt_dev.stride(), P(buf), nbytes, None)
    return buf


def run_s2(hip, x, wt, p, pieces=3, geometry=0):
    """One launch of the stride-2 entry: (B, Cout, Ho, Wo) on the CPU; checks the sentinel rows behind row M."""
    b, cin, h, w = x.shape
    cout = wt.shape[0]
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    m = b * ho * wo
    dx, pk = x.to(DEV).contiguous(memory_format=torch.channels_last), pack_of(hip, wt.to(DEV), pieces)
    dp = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in p.items()}
    out = torch.full((m + SLACK_ROWS, cout), SENTINEL, device=DEV)
    assert hip.skd_conv3x3_split_s2_nhwc(b, h, w, cin, cout, P(dx), P(pk), P(out), P(dp["cbias"]), P(dp["mean"]), P(dp["var"]),
                                         P(dp["gamma"]), P(dp["beta"]), p["eps"], ACT[p["act"]], 0.01, pieces, geometry, None)
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool((out[m:] == SENTINEL).all()), "rows beyond M were written"
    return out[:m].view(b, ho, wo, cout).permute(0, 3, 1, 2)


def run_s1(hip, x, wt, p, pieces=3):
    """The stride-1 kernel of the same piece count on the same inputs: (B, Cout, H, W) on the CPU."""
    if pieces == 3:
        return T3.run_hip(hip, x, wt, p, 1)[0]
    b, cin, h, w = x.shape
    cout = wt.shape[0]
    dx, pk = x.to(DEV).contiguous(memory_format=torch.channels_last), pack_of(hip, wt.to(DEV), 2)
    dp = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in p.items()}
    out = torch.full((b * h * w, cout), SENTINEL, device=DEV)
    assert hip.skd_conv3x3_split2_nhwc(b, h, w, cin, cout, 1, P(dx), P(pk), P(out), P(dp["cbias"]), P(dp["mean"]), P(dp["var"]),
                                       P(dp["gamma"]), P(dp["beta"]), p["eps"], ACT[p["act"]], 0.01, 0, None)
    torch.cuda.synchronize()
    return out.cpu().view(b, h, w, cout).permute(0, 3, 1, 2)


# ---- 1. the bits of the stride-1 kernel ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("pieces", [3, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bits_of_the_stride1_kernel_at_the_even_pixels(hip, shape, pieces):
    for epi in EPILOGUES:
        x, wt, p = case_inputs(shape, epi)
        want = run_s1(hip, x, wt, p, pieces)[:, :, ::2, ::2]
        assert bool(torch.isfinite(want).all()) and (min(shape[1:3]) < 5 or float(want.abs().max()) > 0.1)
        for geometry in range(4):
            got = run_s2(hip, x, wt, p, pieces, geometry)
            assert got.shape == want.shape
            assert torch.equal(got, want), "%s, %d pieces, geometry %d: %d of %d outputs differ from the stride-1 kernel's" % (
                epi, pieces, geometry, int((got != want).sum()), got.numel())


# ---- 2. integers, float64 -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pieces", [3, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_integers_bit_exact(hip, shape, pieces):
    """|x| <= 7 and |w| <= 3 are one bf16 piece each: either piece count gives the exact product."""
    x, wt, p = case_inputs(shape, "raw", integers=True)
    got = run_s2(hip, x, wt, p, pieces)
    want = F.conv2d(x.double(), wt.double(), None, 2, 1, 1)
    assert min(shape[1:3]) < 5 or float(want.abs().max()) > 50.0
    assert torch.equal(got.double(), want), "%d of %d outputs differ" % (int((got.double() != want).sum()), got.numel())


@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_stride2_vs_float64(hip, shape, epi):
    name = case_name(shape, epi)
    x, wt, p = case_inputs(shape, epi)
    err = rel_err(run_s2(hip, x, wt, p), want_of(shape, epi))
    parent = PARENT_ERR.get(name)
    print("%s: err %.3e  library %s" % (name, err, "not measured" if parent is None else "%.3e  bound %.3e" % (parent, min(RATIO * parent, CAP))))
    assert parent is not None, "PARENT_ERR has no figure for %s" % name
    bound = min(RATIO * parent, CAP)
    assert err <= bound, "%s: max err %.3e > %.3e (library path: %.3e)" % (name, err, bound, parent)


# ---- 3. guard bands, refusals ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pieces", [3, 2])
@pytest.mark.parametrize("shape", RAGGED, ids=[IDS[2], IDS[3]])
def test_guard_bands(hip, shape, pieces):
    """Input, weight, pack, epilogue vectors and output (exactly M * Cout floats) between 0xFF guards (NaN as fp32): no guard byte
    changes, and neither a stray read nor an unwritten element leaves a NaN in the output."""
    b, h, w, cin, cout = shape
    m = b * ((h - 1) // 2 + 1) * ((w - 1) // 2 + 1)
    for epi in EPILOGUES:
        x, wt, p = case_inputs(shape, epi)
        A = BC.Arena(DEV)
        dx = A.inp("x", x.permute(0, 2, 3, 1).contiguous(), row=cin)
        dw = A.inp("weight", wt)
        nbytes = cout * cin * 18 * pieces
        pk = A.out("pack", nbytes, torch.uint8)
        vec = {k: A.inp(k, p[k]) for k in ("cbias", "mean", "var", "gamma", "beta")}
        out = A.out("out", (m, cout), row=cout)
        pack = hip.skd_conv3x3_split_pack_weights if pieces == 3 else hip.skd_conv3x3_split2_pack_weights
        assert pack(cin, cout, P(dw), *dw.stride(), P(pk), nbytes, None)
        A.check()
        for geometry in range(4):
            assert hip.skd_conv3x3_split_s2_nhwc(b, h, w, cin, cout, P(dx), P(pk), P(out), P(vec["cbias"]), P(vec["mean"]), P(vec["var"]),
                                                 P(vec["gamma"]), P(vec["beta"]), p["eps"], ACT[p["act"]], 0.01, pieces, geometry, None) == 1
            A.check()
            assert not bool(torch.isnan(out).any())
            got = out.cpu().view(b, (h - 1) // 2 + 1, (w - 1) // 2 + 1, cout).permute(0, 3, 1, 2)
            assert torch.equal(got, run_s2(hip, x, wt, p, pieces)), (epi, geometry)
            out.fill_(float("nan"))


def test_refusals_launch_nothing_and_leave_out_alone(hip):
    b, h, w, cin, cout = SHAPES[1]
    x, wt, p = case_inputs(SHAPES[1], "raw")
    A = BC.Arena(DEV)
    dx = A.inp("x", x.permute(0, 2, 3, 1).contiguous(), row=cin)
    pk = A.out("pack", cout * cin * 54, torch.uint8)
    var = A.inp("var", torch.ones(cout))
    out = A.out("out", (b * 3 * 3, cout), row=cout)
    dw = wt.to(DEV)
    assert hip.skd_conv3x3_split_pack_weights(cin, cout, P(dw), *dw.stride(), P(pk), cout * cin * 54, None)
    before = out.view(torch.int32).clone()          # the arena's fill is NaN as fp32: compared as bits

    def call(**kw):
        a = dict(b=b, h=h, w=w, cin=cin, cout=cout, x=P(dx), pk=P(pk), out=P(out), mean=None, var=None, act=0, pieces=3, geo=0)
        a.update(kw)
        return hip.skd_conv3x3_split_s2_nhwc(a["b"], a["h"], a["w"], a["cin"], a["cout"], a["x"], a["pk"], a["out"], None, a["mean"],
                                             a["var"], None, None, 0.0, a["act"], 0.01, a["pieces"], a["geo"], None)
    for bad in (dict(pieces=1), dict(pieces=4), dict(pieces=0), dict(geo=4), dict(geo=-1), dict(act=1), dict(act=2), dict(cout=64),
                dict(cin=24), dict(b=0), dict(h=0), dict(w=0), dict(x=None), dict(pk=None), dict(out=None), dict(var=P(var)),
                dict(mean=P(var)), dict(x=dx.data_ptr() + 4), dict(pk=pk.data_ptr() + 8)):
        assert call(**bad) == 0, bad
    torch.cuda.synchronize()
    A.check()
    assert torch.equal(out.view(torch.int32), before), "a refused call wrote the output"
    assert call() == 1
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any())


def test_op_gives_the_entrys_bits(hip):
    """SF.conv3x3_s2_eval on the module's cached pack of either piece count: the entry's bits, a plain channels-last allocation."""
    shape = SHAPES[2]
    x, wt, p = case_inputs(shape, "bias-bn-relu")
    conv = torch.nn.Conv2d(shape[3], shape[4], 3, 2, 1, bias=True)
    bn = PC.InPlaceABNSync(shape[4], activation="none")
    with torch.no_grad():
        conv.weight.copy_(wt)
        conv.bias.copy_(p["cbias"])
        bn.running_mean.copy_(p["mean"])
        bn.running_var.copy_(p["var"])
        bn.weight.copy_(p["gamma"])
        bn.bias.copy_(p["beta"])
    conv, bn = conv.to(DEV), bn.to(DEV).eval()
    dx = x.to(DEV)
    with torch.no_grad():
        assert SF.conv3x3_s2_supported(dx, conv) and not SF.conv3x3_split_supported(dx, conv)
        for pieces in (3, 2):
            got = SF.conv3x3_s2_eval(dx, SF.conv3x3_pack_weights(conv, pieces=pieces), shape[4], conv.bias, bn, "relu", pieces=pieces)
            assert got.is_contiguous(memory_format=torch.channels_last) and got._base is None
            assert torch.equal(got.cpu(), run_s2(hip, x, wt, p, pieces))
        raw = SF.conv3x3_s2_eval(dx, SF.conv3x3_pack_weights(conv), shape[4])
        assert torch.equal(raw.cpu(), run_s2(hip, x, wt, dict(p, cbias=None, mean=None, var=None, gamma=None, beta=None, eps=0.0, act="none")))


# ---- 4. the whole teacher ---------------------------------------------------------------------------------------------------------

COUNTED = [S2, WIDE, WIDE2, NARROW]
_TEACHER = {}


def _rec_err(t, rec):
    import test_student_infer_gpu as TI
    return TI._rec_err(t, rec)


def _teacher():
    """The seeded teacher of tests/golden/make_golden_teacher_early.py on the device, its image and the fixture (made once)."""
    if not _TEACHER:
        import make_golden_teacher_early as G
        fx = torch.load(G.OUT, weights_only=False)
        assert os.path.getsize(G.OUT) <= 400 * 1024 and fx["names"] == G.NAMES == ["x2", "x1", "logits"]
        Pw, x = G.inputs()
        for k, v in G.checksum(Pw).items():
            assert abs(v - fx["checksums"][k]) <= 1e-9 * max(1.0, abs(v)), ("weight RNG drifted from the fixture generator's", k)
        net = PC.Res_pspnet(PC.Bottleneck, [3, 4, 23, 3], 19)
        net.load_state_dict(Pw)
        for q in net.parameters():
            q.requires_grad_(False)
        _TEACHER.update(net=net.eval().to(DEV).to(memory_format=torch.channels_last), fx=fx,
                        x=x.to(DEV).contiguous(memory_format=torch.channels_last))
    return _TEACHER["net"], _TEACHER["x"], _TEACHER["fx"]


def _counted_forward(net, dx):
    _lib.enable_kernel_timing(COUNTED)
    try:
        with torch.no_grad():
            out = net(dx)
    finally:
        calls = _lib.disable_kernel_timing()
    return [out[5], out[6], out[0]], {k: len(v) for k, v in calls.items()}


def test_whole_teacher_vs_float64_fixture():
    """Flagged against unflagged on the same GPU: per recorded output (x2, x1, logits) the flagged error is at most four times the
    unflagged one, and the nine launches are counted -- four on the 64-column entry, four more on the wide one, one on the
    stride-2 entry, whose input is a 25 x 25 map."""
    net, dx, fx = _teacher()
    plain, off = _counted_forward(net, dx)
    assert off[S2] == off[NARROW] == off[WIDE2] == 0
    try:
        assert networks.route_teacher_early(net) is net
        flagged, on = _counted_forward(net, dx)
    finally:
        networks.route_teacher_early(net, enable=False)
    assert on[S2] == 1 and on[NARROW] == 4 and on[WIDE] == off[WIDE] + 4 and on[WIDE2] == 0, (on, off)
    assert list(flagged[0].shape) == [1, 512, 13, 13] and list(flagged[1].shape) == [1, 256, 25, 25]
    for name, a, b, r in zip(fx["names"], plain, flagged, fx["outputs"]):
        e_plain, e_flagged = _rec_err(a, r), _rec_err(b, r)
        print("%-7s unflagged %.3e  flagged %.3e of the norm, ratio %.2f" % (name, e_plain / r["norm"], e_flagged / r["norm"],
                                                                           e_flagged / e_plain))
        assert e_flagged <= RATIO * e_plain, name
        assert not torch.equal(a, b), "the flag changed nothing"
    after, cleared = _counted_forward(net, dx)
    assert cleared == off and not any(hasattr(m, "_skd_teacher_early") for m in net.modules())


def test_whole_teacher_flagged_on_two_pieces():
    """The same network flagged and marked for two pieces: the five wide calls move to the two-piece entries (the stride-2 one
    stays on its entry, with pieces = 2), the four 64-column calls stay.  Bound: that of tests/test_split2_gpu.py for whole outputs
    of the two-piece teacher, max |got - truth| / max |truth| <= 4 E -- E["logits"] for the logits, which the fixture records whole;
    x2 and x1 sit upstream of everything E was measured behind and are held to 4 x the smallest of the three figures, over the
    fixture's strided sample."""
    import test_split2_gpu as T2
    net, dx, fx = _teacher()
    try:
        networks.set_teacher_pieces(net, 2)
        networks.route_teacher_early(net)
        got, on = _counted_forward(net, dx)
    finally:
        networks.route_teacher_early(net, enable=False)
        networks.set_teacher_pieces(net, 3)
    assert on[S2] == 1 and on[NARROW] == 4 and on[WIDE] == 0 and on[WIDE2] == 28 + 4, on
    for name, t, r in zip(fx["names"], got, fx["outputs"]):
        f = t.detach().cpu().double().reshape(-1)[::r["step"]][:r["sample"].numel()]
        assert name != "logits" or f.numel() == t.numel(), "the logits are recorded whole"
        err = R.rel_err(f, r["sample"])
        bound = 4 * (T2.E["logits"] if name == "logits" else min(T2.E.values()))
        print("%-7s two pieces, flagged: %.3e of the largest magnitude (bound %.3e)" % (name, err, bound))
        assert err <= bound, name


# ---- 5. the student, the step -----------------------------------------------------------------------------------------------------

def test_whole_student_with_the_stride2_launch():
    """The student flagged with ``narrow`` and ``stride2`` against tests/golden/student_infer_oracle.pt at that file's bound (four times
    the unflagged form's error on the same GPU), one stride-2 launch counted."""
    import make_golden_student_infer as G
    fx = torch.load(G.OUT, weights_only=False)
    Pw, x = G.inputs()
    S = PC.Res_pspnet(PC.BasicBlock, [2, 2, 2, 2], 19)
    S.load_state_dict(Pw)
    S = S.to(DEV).to(memory_format=torch.channels_last).eval()
    dx = x.to(DEV).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        plain = S(dx)
        _lib.enable_kernel_timing([S2, NARROW])
        try:
            narrow = networks.fuse_for_inference(S, narrow=True)(dx)
        finally:
            off = _lib.disable_kernel_timing()
        _lib.enable_kernel_timing([S2, NARROW])
        try:
            fused = networks.fuse_for_inference(S, narrow=True, stride2=True)(dx)
        finally:
            on = _lib.disable_kernel_timing()
    assert len(off[S2]) == 0 and len(on[S2]) == 1 and len(on[NARROW]) == len(off[NARROW]) == 5
    assert on[S2][0][1] == (2, 17, 25, 64), "layer2.0.conv1 reads the 17 x 25 map of layer1"
    for name, a, b, c, r in zip(fx["names"], plain, fused, narrow, fx["outputs"]):
        e_plain, e_fused = _rec_err(a, r), _rec_err(b, r)
        print("%-18s unflagged %.3e  stride2-flagged %.3e of the norm, ratio %.2f" % (name, e_plain / r["norm"], e_fused / r["norm"],
                                                                                      e_fused / e_plain))
        assert e_fused <= RATIO * e_plain, name
        assert not torch.equal(b, c), "the switch changed nothing"


def test_step_config1_with_the_teacher_early(monkeypatch):
    """The config-1 step of tests/test_step_gpu.py with SKD_TEACHER_EARLY=1 at exactly the bounds of the switch-off test: that
    test's own body runs, with the switch set where its ``default_args`` reads it.  A counting shim sees one stride-2 launch per
    teacher forward (128 -> 128); with the switch off, none."""
    import test_step_gpu as TS
    real = SF.conv3x3_s2_eval
    seen = []

    def shim(x, pack, cout, *args, **kw):
        seen.append((int(x.shape[1]), int(cout)))
        return real(x, pack, cout, *args, **kw)
    monkeypatch.setattr(SF, "conv3x3_s2_eval", shim)
    monkeypatch.setenv("SKD_TEACHER_EARLY", "0")
    model, _, _ = TS._config1_step(pa=True)
    assert not model.teacher_early and seen == []
    del model
    monkeypatch.setenv("SKD_TEACHER_EARLY", "1")
    TS.test_step_config1_vs_reference_golden()
    assert len(seen) >= 1 and set(seen) == {(128, 128)}, seen
