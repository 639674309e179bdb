"""-m gpu: the fp16 two-piece forms of include/skd_split2h.h -- csrc/conv3x3.hip's 128-column forward family and
csrc/conv1x1.hip's GEMM with two FP16 pieces per operand and the residual scaled by 2^11 -- on small shapes:

  3x3: B = 1, 2; H x W = 9 x 13, 7 x 7; Cin = 16, 48; Cout = 128, 256; dilation 1, 2; every geometry 0 .. 3
  1x1: M = 130, 257 (ragged against 64- and 128-row tiles); K = 16, 48 and 272 (through the prologue); N = 128, 256; with and
       without residual

1. EXACT, no tolerance (dyadic operands; "wide" = 1 + 2^-21 k in [1, 2), 22 significant bits; "narrow" = +-1, +-2; the sparse side
   has two non-zeros per output, so every partial sum of both accumulator sets and the joined result fit 24 bits of their unit):
   wide x narrow and narrow x wide equal the exact product, wide x wide equals the three-product MODEL (tests/split2h_ref.py) and
   not the exact product.  Every case carries a non-zero `lo` set, so a wrong 2^-11 cannot pass; and on the same inputs the bf16
   two-piece entry is wrong where this one is exact.
2. fp16-SUBNORMAL first pieces are used as they are (the fp16 MFMA does not flush its A / B operands).
3. Accuracy on post-ReLU normal data at three scales against float64: within 2 x of the three-piece entry's own error on the same
   inputs, and the bf16 two-piece entry at least 4 x worse (both measured in the same test; profiles/r32_split2h_accuracy.md).
4. Overflow is loud: one activation of 70000 makes every output that reads it non-finite and leaves every other output bit-equal.
5. Sentinel rows behind every output, guard bytes around every operand and the pack; a flagged teacher: eager == graph replay, and
   against the float64 oracle within 2 x of the three-piece teacher measured in the same test.
"""
import contextlib
import itertools

import pytest
import torch
import torch.nn.functional as F

import bounds_cases as BC
import split2_ref as R2
import split2h_ref as R
import test_conv_planes_gpu as TP
import test_conv3x3_split_gpu as T3
from structure_knowledge_distillation_amd import _lib, functional as SF
from structure_knowledge_distillation_amd import networks
import structure_knowledge_distillation_amd.networks.pspnet_combine as PC

pytestmark = pytest.mark.gpu
DEV = "cuda"
P, SENTINEL, SLACK_ROWS, ACT = T3.P, T3.SENTINEL, T3.SLACK_ROWS, T3.ACT

# per form: (pack_bytes, pack_weights, 3x3 entry, 1x1 entry, 1x1 entry with prologue)
FORMS = {
    "fp16x2": ("skd_conv3x3_split2h_pack_bytes", "skd_conv3x3_split2h_pack_weights", "skd_conv3x3_split2h_nhwc",
               "skd_conv1x1_abn2h_nhwc", "skd_conv1x1_abn2h_pro_nhwc"),
    "bf16x2": ("skd_conv3x3_split2_pack_bytes", "skd_conv3x3_split2_pack_weights", "skd_conv3x3_split2_nhwc",
               "skd_conv1x1_abn2_nhwc", "skd_conv1x1_abn2_pro_nhwc"),
    "bf16x3": ("skd_conv3x3_split_pack_bytes", "skd_conv3x3_split_pack_weights", "skd_conv3x3_split_nhwc",
               "skd_conv1x1_abn_nhwc", "skd_conv1x1_abn_pro_nhwc"),
}


@pytest.fixture(scope="module")
def hip():
    return _lib.load()


# ---- launchers: every output has SLACK_ROWS sentinel rows behind it ---------------------------------------------------------------

def pack_of(hip, form, wt):
    cout, cin = wt.shape[:2]
    dw = wt.to(DEV).contiguous()
    nbytes = getattr(hip, FORMS[form][0])(cin, cout)
    assert nbytes == cout * cin * 9 * (6 if form == "bf16x3" else 4)
    buf = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    assert getattr(hip, FORMS[form][1])(cin, cout, P(dw), *dw.stride(), P(buf), nbytes, None)
    return buf


def conv3(hip, form, x, wt, d, geometry=0, pk=None, act="none"):
    """(B, Cout, H, W) raw (or activated) output of the form's 3x3 entry, on the CPU."""
    b, cin, h, w = x.shape
    cout, m = wt.shape[0], b * h * w
    dx = x.to(DEV).contiguous(memory_format=torch.channels_last)
    pk = pack_of(hip, form, wt) if pk is None else pk
    out = torch.full((m + SLACK_ROWS, cout), SENTINEL, device=DEV)
    assert getattr(hip, FORMS[form][2])(b, h, w, cin, cout, d, P(dx), P(pk), P(out), None, None, None, None, None, 0.0, ACT[act], 0.01,
                                        geometry, None)
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool((out[m:] == SENTINEL).all()), "rows beyond M were written"
    return out[:m].view(b, h, w, cout).permute(0, 3, 1, 2)


def gemm(hip, form, x, w, r=None, pro=False, act=0):
    """(M, N) output of the form's 1x1 entry with the identity epilogue (mean 0, var 1, eps 0, no affine) [+ r]; ``pro``: through
    the prologue entry with the identity table, which leaves relu(x)."""
    m, k = x.shape
    n = w.shape[0]
    out = torch.full((m + SLACK_ROWS, n), SENTINEL, device=DEV)
    dx, dw, dr = x.to(DEV), w.to(DEV), None if r is None else r.to(DEV)
    mean, var = torch.zeros(n, device=DEV), torch.ones(n, device=DEV)
    head = (m, k, n, P(dx), P(dw), P(dr), P(out), P(mean), P(var), None, None, 0.0)
    if pro:
        table = torch.empty(4, k, device=DEV)
        pm, pv = torch.zeros(k, device=DEV), torch.ones(k, device=DEV)
        assert hip.skd_abn_pack_eval_params(k, P(pm), P(pv), None, None, 0.0, P(table), None)
        assert table.cpu().tolist() == [[0.0] * k, [1.0] * k, [1.0] * k, [0.0] * k]
        assert getattr(hip, FORMS[form][4])(*head, P(table), act, 0.01, None)
    else:
        assert getattr(hip, FORMS[form][3])(*head, act, 0.01, None)
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool((out[m:] == SENTINEL).all()), "rows beyond M were written"
    return out[:m]


# ---- 1. exact ----------------------------------------------------------------------------------------------------------------------

def wide(shape, g, signed=True):
    """1 + 2^-21 k, k in [0, 2^21): 22 significant bits, two fp16 pieces, more than two bf16 pieces hold."""
    v = 1.0 + torch.randint(0, 2 ** 21, shape, generator=g).double() * 2.0 ** -21
    if signed:
        v = v * (torch.randint(0, 2, shape, generator=g).double() * 2 - 1)
    return v.float()


def narrow(shape, g):
    """+-1, +-2: one piece."""
    return (torch.randint(1, 3, shape, generator=g) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)).float()


def two_per_row(t, g):
    """``t`` (rows, ...) with all but two entries of every row zeroed."""
    flat = t.reshape(t.shape[0], -1)
    keep = torch.zeros_like(flat)
    idx = torch.stack([torch.randperm(flat.shape[1], generator=g)[:2] for _ in range(flat.shape[0])])
    keep.scatter_(1, idx, 1.0)
    return (flat * keep).reshape(t.shape)


def lattice(x, g):
    """The (B, C, H, W) map ``x`` with non-zeros at the pixels of a 5-pixel lattice alone, two channels each: a 3 x 3 window of
    dilation <= 2 (five pixels wide) sees one such pixel at most."""
    b, c, h, w = x.shape
    keep = torch.zeros_like(x)
    for bi, hi, wi in itertools.product(range(b), range(0, h, 5), range(0, w, 5)):
        keep[bi, torch.randperm(c, generator=g)[:2], hi, wi] = 1.0
    return x * keep


CLASSES = ("wide x narrow", "narrow x wide", "wide x wide")


def operands1(cls, m, k, n, g, positive_x):
    """(x, w) of an exact 1x1 case; the sparse side leaves two products per output.  ``positive_x``: behind the prologue's ReLU."""
    if cls == "narrow x wide":
        x = two_per_row(narrow((m, k), g), g)
        return (x.abs() if positive_x else x), wide((n, k), g)
    w = two_per_row(narrow((n, k), g) if cls == "wide x narrow" else wide((n, k), g), g)
    return wide((m, k), g, signed=not positive_x), w


def check_exact(cls, got, x2d, w2d, what, bf16=None):
    """``x2d`` (rows, K) / ``w2d`` (N, K): the operands as matrices, for the model's `lo` set and the exact product's bounds."""
    exact = x2d.double() @ w2d.double().t()
    model = R.mm_split2h(x2d, w2d)
    a0, a1 = R.pieces(x2d)
    b0, b1 = R.pieces(w2d)
    lo = a0 @ b1.t() + a1 @ b0.t()
    assert float(exact.abs().max()) < 8.0 and float(exact.abs().max()) > 1.0
    assert int((lo != 0).sum()) > lo.numel() // 8, "%s: the lo set must matter" % what
    assert bool(((a0 @ b0.t()) != model).any()), "%s: hi alone must not be the answer" % what
    got = got.double()
    if cls == "wide x wide":
        want = model.float().double()          # the kernel's one fma rounds the exact hi + 2^-11 lo once
        assert torch.equal(got, want), "%s: %d of %d outputs differ from the model" % (what, int((got != want).sum()), got.numel())
        assert bool((got != exact.float().double()).any()), "%s: every output is the exact product: a1 b1 was not dropped" % what
        return
    assert torch.equal(model, exact) and torch.equal(exact.float().double(), exact), "%s: the case is not an exact one" % what
    assert torch.equal(got, exact), "%s: %d of %d outputs differ from the exact product" % (what, int((got != exact).sum()), got.numel())
    if bf16 is not None:
        wrong = int((bf16.double() != exact).sum())
        assert wrong > got.numel() // 8, "%s: two bf16 pieces were expected to miss these values (%d wrong)" % (what, wrong)


CASES1 = list(itertools.product((130, 257), (16, 48, 272), (128, 256), (False, True)))
# K = 272 runs through the prologue entry; at M = 2113, N = 2048 the launch is cut in column chunks: the NT forms of the two-piece kernel
CASES1 += [(2113, 272, 2048, False), (2113, 272, 2048, True)]
# ... and without the prologue: column chunks depend on K and N alone (128 * K * 4 bytes a column tile against 2^20), K = 144 gives 14 of 16
CASES1 += [(130, 144, 2048, True)]


@pytest.mark.parametrize("m,k,n,res", CASES1, ids=["M%d-K%d-N%d%s" % (m, k, n, "-res" if r else "") for m, k, n, r in CASES1])
def test_conv1x1_exact(hip, m, k, n, res):
    pro = k == 272
    for ci, cls in enumerate(CLASSES):
        g = torch.Generator().manual_seed(1000 * ci + m + k + n)
        x, w = operands1(cls, m, k, n, g, positive_x=pro)
        r = torch.randint(-3, 4, (m, n), generator=g).float() if res else None
        got = gemm(hip, "fp16x2", x, w, r, pro)
        bf16 = gemm(hip, "bf16x2", x, w, None, pro) if cls != "wide x wide" and not res else None
        if res:      # one more fp32 rounding behind the joined sets: undone exactly where it was exact, compared in fp32 otherwise
            plain = gemm(hip, "fp16x2", x, w, None, pro)
            assert torch.equal(got, plain + r), "%s: the residual is one fp32 add behind the joined sets" % cls
            got = plain
        check_exact(cls, got, x, w, "%s M%d K%d N%d" % (cls, m, k, n), bf16)


CASES3 = list(itertools.product((1, 2), ((9, 13), (7, 7)), (16, 48), (128, 256), (1, 2)))


def unfold(x, d):
    """(B * H * W, 9 * Cin) rows of the implicit GEMM, k = c * 9 + tap as F.unfold orders them (the order does not matter here)."""
    b, c, h, w = x.shape
    return F.unfold(x.double(), 3, d, d, 1).permute(0, 2, 1).reshape(b * h * w, c * 9).float()


@pytest.mark.parametrize("b,hw,cin,cout,d", CASES3, ids=["B%d-%dx%d-C%d-N%d-d%d" % (b, hw[0], hw[1], ci, co, d) for b, hw, ci, co, d in CASES3])
def test_conv3x3_exact(hip, b, hw, cin, cout, d):
    for ci, cls in enumerate(CLASSES):
        g = torch.Generator().manual_seed(1000 * ci + 100 * b + hw[0] + cin + cout + d)
        if cls == "narrow x wide":
            x, wt = lattice(narrow((b, cin, *hw), g), g), wide((cout, cin, 3, 3), g)
        else:
            x = wide((b, cin, *hw), g)
            wt = two_per_row(narrow((cout, cin, 3, 3), g) if cls == "wide x narrow" else wide((cout, cin, 3, 3), g), g)
        pk = pack_of(hip, "fp16x2", wt)
        base = conv3(hip, "fp16x2", x, wt, d, 0, pk)
        for geometry in (1, 2, 3):
            assert torch.equal(conv3(hip, "fp16x2", x, wt, d, geometry, pk), base), (cls, geometry)
        rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, cout)
        bf16 = rows(conv3(hip, "bf16x2", x, wt, d)) if cls != "wide x wide" else None
        check_exact(cls, rows(base), unfold(x, d), wt.reshape(cout, cin * 9), "%s B%d %s C%d N%d d%d" % (cls, b, hw, cin, cout, d), bf16)


# ---- 2. subnormal pieces -----------------------------------------------------------------------------------------------------------

def test_fp16_subnormal_pieces_are_used_as_they_are(hip):
    """2^-20 is an fp16 SUBNORMAL (a multiple of 2^-24 below 2^-14): against 1024 the no-flush model gives 2^-10 per product.  A
    core that flushed subnormal A / B operands would return 0.  Measured on the MI355X: not flushed, on either side, in either
    kernel; a second piece that is subnormal (2^-14 + 2^-35: a1 = 2^-24) is kept too."""
    m, k, n = 130, 48, 128
    x, w = torch.zeros(m, k), torch.zeros(n, k)
    x[:, 0], x[:, 5] = 2.0 ** -20, 3 * 2.0 ** -24
    w[:, 0], w[:, 5] = 1024.0, 512.0
    want = R.mm_split2h(x, w)
    assert torch.equal(want, torch.full((m, n), 2.0 ** -10 + 3 * 2.0 ** -15, dtype=torch.float64))
    assert not bool(R.mm_split2h(x, w, flush=True).any()), "the flushing model gives zero: the case discriminates"
    assert torch.equal(gemm(hip, "fp16x2", x, w).double(), want), "a subnormal first piece on the A side"
    xb, wb = torch.zeros(m, k), torch.zeros(n, k)
    xb[:, 0], wb[:, 0] = 1024.0, 2.0 ** -20
    assert torch.equal(gemm(hip, "fp16x2", xb, wb).double(), torch.full((m, n), 2.0 ** -10, dtype=torch.float64)), "on the B side"
    # a subnormal SECOND piece: 2^-14 + 2^-35 -> a0 = 2^-14, a1 = fp16(2^-35 * 2^11) = 2^-24
    x2, w2 = torch.zeros(m, k), torch.zeros(n, k)
    x2[:, 3], w2[:, 3] = 2.0 ** -14 + 2.0 ** -35, 2.0 ** 15
    want2 = R.mm_split2h(x2, w2)
    assert torch.equal(want2, torch.full((m, n), 2.0 + 2.0 ** -20, dtype=torch.float64))
    assert float(R.mm_split2h(x2, w2, flush=True)[0, 0]) == 2.0
    assert torch.equal(gemm(hip, "fp16x2", x2, w2).double(), want2), "a subnormal second piece"
    # the 3x3 kernel: the activation is split in the loop, the weight in the pack kernel
    full = torch.full((1, 128, 7, 7), 2.0 ** -10, dtype=torch.float64)
    xc, wc = torch.zeros(1, 16, 7, 7), torch.zeros(128, 16, 3, 3)
    xc[0, 2], wc[:, 2, 1, 1] = 2.0 ** -20, 1024.0
    assert torch.equal(conv3(hip, "fp16x2", xc, wc, 1).double(), full), "a subnormal activation piece"
    xc[0, 2], wc[:, 2, 1, 1] = 1024.0, 2.0 ** -20
    assert torch.equal(conv3(hip, "fp16x2", xc, wc, 1).double(), full), "a subnormal weight piece, from the pack kernel"


# ---- 3. accuracy -------------------------------------------------------------------------------------------------------------------

SCALES = (1.0, 30.0, 1e-3)


def report(what, scale, errs):
    """One line per shape and scale, in the form profiles/r32_split2h_accuracy.md tabulates; then the two assertions."""
    e3, eh, e2 = errs["bf16x3"], errs["fp16x2"], errs["bf16x2"]
    print("ACC| %s | x%g | %.3e | %.3e | %.3e | %.2f | %.1f |" % (what, scale, e3, eh, e2, eh / e3, e2 / eh))
    assert eh <= 2 * e3, "%s x%g: fp16 two pieces %.3e > 2 x three pieces %.3e" % (what, scale, eh, e3)
    assert e2 >= 4 * eh, "%s x%g: two bf16 pieces %.3e < 4 x %.3e: the test does not discriminate" % (what, scale, e2, eh)


@pytest.mark.parametrize("scale", SCALES)
def test_conv1x1_accuracy(hip, scale):
    m, k, n = 257, 272, 256
    g = torch.Generator().manual_seed(7)
    x = torch.relu(torch.randn(m, k, generator=g)) * scale
    w = torch.randn(n, k, generator=g) * 0.02
    truth = x.double() @ w.double().t()
    for pro in (False, True):
        errs = {form: R.rel_err(gemm(hip, form, x, w, None, pro), truth) for form in FORMS}
        report("1x1 M257 K272 N256%s" % (" pro" if pro else ""), scale, errs)


@pytest.mark.parametrize("scale", SCALES)
def test_conv3x3_accuracy(hip, scale):
    g = torch.Generator().manual_seed(8)
    x = torch.relu(torch.randn(2, 48, 9, 13, generator=g)) * scale
    wt = torch.randn(256, 48, 3, 3, generator=g) * 0.02
    for d in (1, 2):
        truth = F.conv2d(x.double(), wt.double(), None, 1, d, d)
        errs = {form: R.rel_err(conv3(hip, form, x, wt, d), truth) for form in FORMS}
        report("3x3 2x9x13 C48 N256 d%d" % d, scale, errs)


# ---- 4. overflow is loud -----------------------------------------------------------------------------------------------------------

def test_overflow_is_loud(hip):
    """|a| = 70000 > 65504: a0 is infinite and its residual the opposite infinity, so every output that reads the value is
    non-finite (NaN, in fact) -- never a finite wrong value -- and every other output is the bits of the run without it."""
    g = torch.Generator().manual_seed(9)
    m, k, n = 257, 48, 256
    x = torch.relu(torch.randn(m, k, generator=g)) + 0.01
    w = torch.randn(n, k, generator=g) * 0.02
    for pro in (False, True):
        base = gemm(hip, "fp16x2", x, w, None, pro)
        assert bool(torch.isfinite(base).all())
        hot = x.clone()
        hot[131, 7] = 70000.0
        got = gemm(hip, "fp16x2", hot, w, None, pro)
        assert not bool(torch.isfinite(got[131]).any()), "a finite output read the overflowed activation"
        assert bool(torch.isnan(got[131]).all())
        keep = torch.arange(m) != 131
        assert torch.equal(got[keep], base[keep])
    xc = torch.relu(torch.randn(2, 16, 9, 13, generator=g)) + 0.01
    wc = torch.randn(128, 16, 3, 3, generator=g) * 0.02
    for d in (1, 2):
        base = conv3(hip, "fp16x2", xc, wc, d)
        hot = xc.clone()
        hot[1, 3, 4, 6] = 70000.0
        reads = torch.zeros(2, 9, 13, dtype=torch.bool)
        for i, j in itertools.product((-1, 0, 1), (-1, 0, 1)):
            reads[1, 4 + i * d, 6 + j * d] = True
        assert int(reads.sum()) == 9
        for geometry in (0, 1):
            got = conv3(hip, "fp16x2", hot, wc, d, geometry)
            bad = ~torch.isfinite(got)
            assert torch.equal(bad, reads[:, None].expand(2, 128, 9, 13)), "exactly the windows that read it are non-finite"
            assert torch.equal(got[~bad], base[~bad])


# ---- 5. guard bands, the ops, the network ------------------------------------------------------------------------------------------

def test_guard_bands_around_every_operand(hip):
    """Every operand of the five entries at its exact size between 0xFF guards, the outputs pre-filled with 0xFF (an element the
    kernel did not write shows as NaN)."""
    g = torch.Generator().manual_seed(5)
    A = BC.Arena(DEV)
    b, h, w, cin, cout, d = 2, 9, 13, 48, 256, 2
    x = A.inp("x", torch.relu(torch.randn(b, h, w, cin, generator=g)))
    wt = A.inp("w", torch.randn(cout, cin, 3, 3, generator=g) * 0.1)
    vec = lambda name, n, pos=False: A.inp(name, torch.rand(n, generator=g) + 0.5 if pos else torch.randn(n, generator=g))
    cb, mean, var, ga, be = vec("cbias", cout), vec("mean", cout), vec("var", cout, True), vec("gamma", cout), vec("beta", cout)
    nbytes = hip.skd_conv3x3_split2h_pack_bytes(cin, cout)
    pk = A.out("pack", nbytes, torch.uint8, row=4096)
    assert hip.skd_conv3x3_split2h_pack_weights(cin, cout, P(wt), *wt.stride(), P(pk), nbytes, None)
    outs = []
    for geometry in (0, 1, 2, 3):
        y = A.out("y%d" % geometry, (b, h, w, cout))
        assert hip.skd_conv3x3_split2h_nhwc(b, h, w, cin, cout, d, P(x), P(pk), P(y), P(cb), P(mean), P(var), P(ga), P(be), 1e-5,
                                            ACT["leaky_relu"], 0.01, geometry, None)
        outs.append(y)
    for mm, k, n, pro, res in ((257, 48, 256, False, True), (130, 272, 128, True, True), (257, 16, 128, False, False),
                               (130, 272, 256, True, False),
                               (130, 272, 2048, True, False), (130, 144, 2048, False, True)):      # N = 2048: in column chunks (the NT forms with ReLU)
        x1 = A.inp("x1", torch.randn(mm, k, generator=g))
        w1 = A.inp("w1", torch.randn(n, k, generator=g) * 0.05)
        r1 = A.inp("r1", torch.randn(mm, n, generator=g)) if res else None
        bn = [vec("mean1", n), vec("var1", n, True), vec("gamma1", n), vec("beta1", n)]
        y1 = A.out("y1", (mm, n))
        head = (mm, k, n, P(x1), P(w1), P(r1), P(y1), *(P(t) for t in bn), 1e-5)
        if pro:
            src = [vec("pm", k), vec("pv", k, True), vec("pw", k), vec("pb", k)]
            table = A.out("ppack", (4, k))
            assert hip.skd_abn_pack_eval_params(k, *(P(t) for t in src), 1e-5, P(table), None)
            assert hip.skd_conv1x1_abn2h_pro_nhwc(*head, P(table), 3, 0.01, None)
        else:
            assert hip.skd_conv1x1_abn2h_nhwc(*head, 3, 0.01, None)
        outs.append(y1)
    A.check()
    for y in outs:
        assert bool(torch.isfinite(y).all()), "an output element was not written"
    for y in outs[1:4]:
        assert torch.equal(y, outs[0])


def test_ops_give_the_entries_bits(hip):
    g = torch.Generator().manual_seed(12)
    x = torch.relu(torch.randn(2, 48, 9, 13, generator=g))
    conv = torch.nn.Conv2d(48, 256, 3, 1, 2, 2, bias=False).to(DEV).eval()
    dx = x.to(DEV).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        pkh = SF.conv3x3_pack_weights_fp16(conv)
        pk2 = SF.conv3x3_pack_weights(conv, pieces=2)
        assert SF.conv3x3_pack_weights_fp16(conv) is pkh and pkh.numel() == pk2.numel()
        assert not torch.equal(pkh, pk2), "another image of the same size"
        got = SF.conv3x3_split_eval_fp16(dx, pkh, 256, 2)
        with pytest.raises(ValueError):
            SF.conv3x3_split_eval_fp16(dx, SF.conv3x3_pack_weights(conv), 256, 2)      # three planes
    assert torch.equal(got.cpu(), conv3(hip, "fp16x2", x, conv.weight.detach().cpu(), 2))
    m, k, n = 130, 272, 128
    x1, w1 = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g) * 0.02
    r1 = torch.randn(m, n, generator=g)
    as_map = lambda t, c: t.to(DEV).view(1, m, 1, c).permute(0, 3, 1, 2)
    table = torch.empty(4, k, device=DEV)
    assert hip.skd_abn_pack_eval_params(k, P(torch.zeros(k, device=DEV)), P(torch.ones(k, device=DEV)), None, None, 0.0, P(table), None)
    with torch.no_grad():
        for pro in (None, table):
            got = SF.conv1x1_abn_eval_fp16(as_map(x1, k), w1.to(DEV).view(n, k, 1, 1), torch.zeros(n, device=DEV), torch.ones(n, device=DEV),
                                           None, None, 0.0, "none", residual=as_map(r1, n), pro=pro)
            assert torch.equal(got.permute(0, 2, 3, 1).reshape(m, n).cpu(), gemm(hip, "fp16x2", x1, w1, r1, pro is not None))


def small_teacher():
    """The teacher's plan (the ResNet takes no smaller one) for a small input, 65 x 65."""
    torch.manual_seed(41)
    return TP.seeded(PC.Res_pspnet(PC.Bottleneck, [3, 4, 23, 3], 19), 42)


def test_flagged_small_teacher_eager_equals_graph_replay():
    """One hipGraph capture and replay of the teacher, marked for fp16 pieces, on a small input, by the recipe of NetModel._capture_teacher
    (warm-up on a side stream, thread-local capture): the replay's outputs are the eager ones bit for bit, and the marked network
    launched the new entries."""
    net = networks.set_teacher_pieces(small_teacher(), 2, piece_format="fp16")
    x = torch.randn(1, 3, 65, 65, generator=torch.Generator().manual_seed(43)).to(DEV).contiguous(memory_format=torch.channels_last)
    names = list(FORMS["fp16x2"][2:]) + list(FORMS["bf16x2"][2:]) + list(FORMS["bf16x3"][2:])
    with contextlib.ExitStack() as stack:
        stack.enter_context(TP.deterministic_library())
        _lib.enable_kernel_timing(names)
        try:
            with torch.no_grad():
                want = [t.clone() for t in net(x)]
        finally:
            calls = {k: len(v) for k, v in _lib.disable_kernel_timing().items()}
        print("teacher at 65 x 65, fp16 pieces: %s" % calls)
        # layer1's three tails (64 -> 256) are in SPLIT2H_ROUTING_EXCLUDED: three bf16 pieces; two bf16 pieces run nowhere
        assert ("1x1", 64, 256) in PC.SPLIT2H_ROUTING_EXCLUDED and len(PC.SPLIT2H_ROUTING_EXCLUDED) == 1
        assert calls == dict(skd_conv3x3_split2h_nhwc=28, skd_conv1x1_abn2h_nhwc=30, skd_conv1x1_abn2h_pro_nhwc=30,
                             skd_conv1x1_abn_pro_nhwc=3, skd_conv3x3_split2_nhwc=0, skd_conv1x1_abn2_nhwc=0,
                             skd_conv1x1_abn2_pro_nhwc=0, skd_conv3x3_split_nhwc=0, skd_conv1x1_abn_nhwc=0), calls
        static_in = x.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(2):
                net(static_in)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(graph, capture_error_mode="thread_local"):
            outs = net(static_in)
        for t in outs:
            t.fill_(float("nan"))
        static_in.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        TP.same_outputs(outs, want, "fp16 pieces: replay against eager")


def test_teacher_against_the_float64_oracle():
    """The fixture of tests/test_split2_gpu.py's end-to-end case: logits, dsn and PSP feature of the marked ResNet101-plan teacher
    against oracle.step_torch.pspnet_forward in float64, each within 2 x of the three-piece teacher's own error measured here, and
    the same argmax as three pieces everywhere."""
    Pw, x = R2.teacher_case()
    truth = dict(zip(("logits", "dsn", "psp"), R2.teacher_forward64(Pw, x)))
    net = PC.Res_pspnet(PC.Bottleneck, [3, 4, 23, 3], 19)
    net.load_state_dict({k: v.clone() for k, v in Pw.items()})
    net = net.eval().to(DEV).to(memory_format=torch.channels_last)
    dx = x.to(DEV).contiguous(memory_format=torch.channels_last)
    errs, argmax = {}, {}
    for form, args in (("bf16x3", (3,)), ("fp16x2", (2, "fp16")), ("bf16x2", (2,))):
        networks.set_teacher_pieces(net, *args)
        with torch.no_grad():
            out = net(dx)
        got = dict(logits=out[0].cpu(), dsn=out[1].cpu(), psp=out[2].cpu())
        errs[form] = {k: R.rel_err(got[k], truth[k]) for k in truth}
        argmax[form] = got["logits"].argmax(1)
        print("TEACHER| %s | %s |" % (form, " | ".join("%.3e" % errs[form][k] for k in ("logits", "dsn", "psp"))))
    networks.set_teacher_pieces(net, 3)
    assert float((argmax["fp16x2"] == argmax["bf16x3"]).double().mean()) == 1.0
    for k in truth:
        assert errs["fp16x2"][k] <= 2 * errs["bf16x3"][k], (k, errs["fp16x2"][k], errs["bf16x3"][k])
