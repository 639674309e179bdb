"""-m gpu: the fp16 two-piece forms of include/skd_infer2h.h -- csrc/conv3x3.hip's residual-epilogue, 64-column and stride-2 forms
with two FP16 pieces per operand and the residual scaled by 2^11 -- on small shapes:

  B = 1, 2; H x W = 9 x 13, 7 x 7 (ragged against 64- and 128-row tiles); Cin = 16, 48; dilation 1, 2; every geometry an entry takes
  wide (residual entry): Cout = 128, 256;  narrow: Cout = 64, 192;  stride 2: 9 x 13 and 8 x 10 (one odd, one even size)

1. EXACT, no tolerance, with the operand generators, the model (tests/split2h_ref.py) and check_exact of tests/test_split2h_gpu.py:
   wide x narrow and narrow x wide equal the exact product, wide x wide the three-product model and not the exact product; every
   case carries a non-zero `lo` set.  Identity BN; the residual entries with activation none and ReLU and a small dyadic residual.
2. Bit links to the forms that exist, on float post-ReLU data with a real BN: residual NULL = skd_conv3x3_split2h_nhwc; with a
   residual = act(z + r) in fp32 of the z the entry writes with activation none; the narrow entry at Cout = 128 = the wide fp16
   entries; the stride-2 output = the stride-1 fp16 output at the even pixels; every geometry gives the same bits.
3. Accuracy against float64 at three scales: each new entry within 2 x of its own three-piece twin's error on the same inputs
   (the bound tests/test_split2h_gpu.py uses for the 3x3 kernel, whose measured ratio was 1.17 - 1.45).
4. Overflow is loud: one activation of 70000 makes every output that reads it non-finite and leaves every other output bit-equal.
5. Guard bytes around x, the pack (at exactly pack_bytes), the residual and out; sentinel rows behind every output (the launchers).
6. The ops give their entries' bits; the pack caches are separate per form and dropped by drop_conv3x3_packs.
7. A flagged small student: eager == graph replay bit for bit, and each of the four fp16 forms is launched.
8. The whole student against the float64 fixture: the fp16-flagged student's error <= 2 x the three-piece flagged student's.
Every figure is printed in front of its assertion (profiles/r34_infer2h_accuracy.md tabulates them).
"""
import itertools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import bounds_cases as BC
import split2h_ref as R
import test_conv_planes_gpu as TP
import test_conv3x3_split_gpu as T3
import test_split2h_gpu as T2H
import test_student_infer_gpu as TSI
from structure_knowledge_distillation_amd import _lib, functional as SF
from structure_knowledge_distillation_amd.networks import fuse_for_inference
import structure_knowledge_distillation_amd.networks.pspnet_combine as PC

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, "golden") not in sys.path:
    sys.path.insert(0, os.path.join(HERE, "golden"))

pytestmark = pytest.mark.gpu
DEV = "cuda"
P, SENTINEL, SLACK_ROWS, ACT = T3.P, T3.SENTINEL, T3.SLACK_ROWS, T3.ACT
wide, narrow, two_per_row, lattice, check_exact, CLASSES = T2H.wide, T2H.narrow, T2H.two_per_row, T2H.lattice, T2H.check_exact, T2H.CLASSES
EPS, SLOPE = 1e-5, 0.01
NEW = ("skd_conv3x3_split2h_res_nhwc", "skd_conv3x3_narrow2h_nhwc", "skd_conv3x3_split2h_s2_nhwc")
TWIN = ("skd_conv3x3_split_res_nhwc", "skd_conv3x3_narrow_nhwc", "skd_conv3x3_split_s2_nhwc")


@pytest.fixture(scope="module")
def hip():
    return _lib.load()


# ---- launchers: every output has SLACK_ROWS sentinel rows behind it ---------------------------------------------------------------

def pack_of(hip, kind, wt, fp16=True, buf=None):
    """The weight image of the entry kind ("res" / "plain" / "s2": the wide image; "narrow": the 64-column one), fp16 x 2 or
    bf16 x 3, in a buffer of exactly pack_bytes."""
    cout, cin = wt.shape[:2]
    dw = wt.to(DEV).contiguous()
    if kind == "narrow":
        nbytes = (hip.skd_conv3x3_narrow2h_pack_bytes if fp16 else hip.skd_conv3x3_narrow_pack_bytes)(cin, cout)
    else:
        nbytes = (hip.skd_conv3x3_split2h_pack_bytes if fp16 else hip.skd_conv3x3_split_pack_bytes)(cin, cout)
    assert nbytes == cout * cin * 9 * (4 if fp16 else 6)
    buf = torch.empty(nbytes, dtype=torch.uint8, device=DEV) if buf is None else buf
    head = (cin, cout, P(dw), *dw.stride(), P(buf), nbytes)
    if kind == "narrow" and fp16:
        assert hip.skd_conv3x3_narrow2h_pack_weights(*head, None)
    elif kind == "narrow":
        assert hip.skd_conv3x3_narrow_pack_pair(*head, None, 0, None)
    elif fp16:
        assert hip.skd_conv3x3_split2h_pack_weights(*head, None)
    else:
        assert hip.skd_conv3x3_split_pack_weights(*head, None)
    return buf


def out_hw(kind, h, w):
    return ((h - 1) // 2 + 1, (w - 1) // 2 + 1) if kind == "s2" else (h, w)


def run(hip, kind, x, wt, d=1, geometry=0, act="none", r=None, bn=None, pk=None, fp16=True):
    """(B, Cout, Ho, Wo) output, on the CPU, of the entry ``kind`` -- "res", "narrow", "s2" (include/skd_infer2h.h, or their
    three-piece twins with ``fp16=False``) or "plain" (skd_conv3x3_split2h_nhwc / skd_conv3x3_split_nhwc).  ``r``: (B, Cout, H, W)
    residual or None; ``bn``: (mean, var, gamma, beta) device vectors or None for the identity."""
    b, cin, h, w = x.shape
    ho, wo = out_hw(kind, h, w)
    cout, m = wt.shape[0], b * ho * wo
    dx = x.to(DEV).contiguous(memory_format=torch.channels_last)
    pk = pack_of(hip, kind, wt, fp16) if pk is None else pk
    out = torch.full((m + SLACK_ROWS, cout), SENTINEL, device=DEV)
    dr = None if r is None else r.to(DEV).permute(0, 2, 3, 1).contiguous()
    epi = (None,) + (tuple(P(t) for t in bn) + (EPS,) if bn is not None else (None, None, None, None, 0.0)) + (ACT[act], SLOPE)
    if kind == "s2":
        assert r is None and d == 1
        if fp16:
            ok = hip.skd_conv3x3_split2h_s2_nhwc(b, h, w, cin, cout, P(dx), P(pk), P(out), *epi, geometry, None)
        else:
            ok = hip.skd_conv3x3_split_s2_nhwc(b, h, w, cin, cout, P(dx), P(pk), P(out), *epi, 3, geometry, None)
    elif kind == "plain":
        assert r is None
        entry = hip.skd_conv3x3_split2h_nhwc if fp16 else hip.skd_conv3x3_split_nhwc
        ok = entry(b, h, w, cin, cout, d, P(dx), P(pk), P(out), *epi, geometry, None)
    else:
        entry = getattr(hip, (NEW if fp16 else TWIN)[0 if kind == "res" else 1])
        ok = entry(b, h, w, cin, cout, d, P(dx), P(pk), P(out), P(dr), *epi, geometry, None)
    assert ok == 1
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool((out[m:] == SENTINEL).all()), "rows beyond M were written"
    return out[:m].view(b, ho, wo, cout).permute(0, 3, 1, 2)


GEOMETRIES = {"res": (0, 1, 2, 3), "narrow": (0, 1), "s2": (0, 1, 2, 3), "plain": (0, 1, 2, 3)}


def rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def unfold(x, d, stride=1):
    """(B * Ho * Wo, 9 * Cin) rows of the implicit GEMM, k = c * 9 + tap as F.unfold orders them."""
    b, c = x.shape[:2]
    return F.unfold(x.double(), 3, d, d, stride).permute(0, 2, 1).reshape(-1, c * 9).float()


def act32(z, act):
    return torch.where(z < 0, torch.zeros_like(z), z) if act == "relu" else torch.where(z < 0, z * SLOPE, z) if act == "leaky_relu" else z


# ---- 1. exact ----------------------------------------------------------------------------------------------------------------------

def operands3(cls, b, hw, cin, cout, g):
    if cls == "narrow x wide":
        return lattice(narrow((b, cin, *hw), g), g), wide((cout, cin, 3, 3), g)
    x = wide((b, cin, *hw), g)
    return x, two_per_row(narrow((cout, cin, 3, 3), g) if cls == "wide x narrow" else wide((cout, cin, 3, 3), g), g)


def dyadic_residual(z, g):
    """Multiples of 2^-21 with |r| <= 1, signed against ``z`` so that |z + r| <= max(|z|, 1) < 8 keeps the 2^-21 unit in fp32."""
    mag = torch.randint(0, 2 ** 21 + 1, z.shape, generator=g).double() * 2.0 ** -21
    return torch.where(z > 0, -mag, mag).float()


CASES_N = list(itertools.product((1, 2), ((9, 13), (7, 7)), (16, 48), (64, 192), (1, 2)))
CASES_W = list(itertools.product((1, 2), ((9, 13), (7, 7)), (16, 48), (128, 256), (1, 2)))
CASES_S2 = list(itertools.product((1, 2), ((9, 13), (8, 10)), (16, 48), (128, 256)))
_ID = lambda c: "B%d-%dx%d-C%d-N%d" % (c[0], c[1][0], c[1][1], c[2], c[3]) + ("-d%d" % c[4] if len(c) > 4 else "")


@pytest.mark.parametrize("b,hw,cin,cout,d", CASES_N, ids=[_ID(c) for c in CASES_N])
def test_narrow_exact(hip, b, hw, cin, cout, d):
    for ci, cls in enumerate(CLASSES):
        g = torch.Generator().manual_seed(2000 * ci + 100 * b + hw[0] + cin + cout + d)
        x, wt = operands3(cls, b, hw, cin, cout, g)
        pk = pack_of(hip, "narrow", wt)
        base = run(hip, "narrow", x, wt, d, 0, pk=pk)
        assert torch.equal(run(hip, "narrow", x, wt, d, 1, pk=pk), base), (cls, "geometry 1")
        check_exact(cls, rows(base), unfold(x, d), wt.reshape(cout, cin * 9), "narrow %s %s" % (cls, _ID((b, hw, cin, cout, d))))


@pytest.mark.parametrize("b,hw,cin,cout", CASES_S2, ids=[_ID(c) for c in CASES_S2])
def test_stride2_exact(hip, b, hw, cin, cout):
    for ci, cls in enumerate(CLASSES):
        g = torch.Generator().manual_seed(3000 * ci + 100 * b + hw[0] + cin + cout)
        x, wt = operands3(cls, b, hw, cin, cout, g)
        pk = pack_of(hip, "s2", wt)
        base = run(hip, "s2", x, wt, 1, 0, pk=pk)
        assert tuple(base.shape[2:]) == ((hw[0] + 1) // 2, (hw[1] + 1) // 2)
        for geometry in (1, 2, 3):
            assert torch.equal(run(hip, "s2", x, wt, 1, geometry, pk=pk), base), (cls, geometry)
        check_exact(cls, rows(base), unfold(x, 1, 2), wt.reshape(cout, cin * 9), "s2 %s %s" % (cls, _ID((b, hw, cin, cout))))


def _residual_exact(hip, kind, b, hw, cin, cout, d, seed):
    for ci, cls in enumerate(CLASSES):
        g = torch.Generator().manual_seed(seed * ci + 100 * b + hw[0] + cin + cout + d)
        x, wt = operands3(cls, b, hw, cin, cout, g)
        what = "%s+res %s %s" % (kind, cls, _ID((b, hw, cin, cout, d)))
        pk = pack_of(hip, kind, wt)
        z = run(hip, kind, x, wt, d, 0, pk=pk)                       # residual NULL, activation none: the convolution itself
        check_exact(cls, rows(z), unfold(x, d), wt.reshape(cout, cin * 9), what)
        r = dyadic_residual(z.double(), g)
        assert bool((r != 0).sum() > r.numel() // 2) and float(r.abs().max()) <= 1.0
        assert torch.equal((r.double() * 2.0 ** 21).round(), r.double() * 2.0 ** 21), "multiples of 2^-21"
        if cls == "wide x wide":      # z is the model rounded once by the fma; the residual add rounds once more: both in fp32
            want = z + r
        else:                         # z is the exact product: so is z + r, which the test asserts before it compares
            want64 = z.double() + r.double()
            assert torch.equal(want64.float().double(), want64), "%s: z + r is not representable in fp32" % what
            want = want64.float()
        assert bool((want < 0).any()) and bool((want > 0).any())
        for act in ("none", "relu"):
            for geometry in GEOMETRIES[kind]:
                got = run(hip, kind, x, wt, d, geometry, act, r, pk=pk)
                ref = act32(want, act)
                assert torch.equal(got, ref), "%s %s geometry %d: %d of %d outputs differ" % (what, act, geometry, int((got != ref).sum()), got.numel())


@pytest.mark.parametrize("b,hw,cin,cout,d", CASES_W, ids=[_ID(c) for c in CASES_W])
def test_wide_residual_exact(hip, b, hw, cin, cout, d):
    _residual_exact(hip, "res", b, hw, cin, cout, d, 4000)


@pytest.mark.parametrize("b,hw,cin,cout,d", CASES_N, ids=[_ID(c) for c in CASES_N])
def test_narrow_residual_exact(hip, b, hw, cin, cout, d):
    _residual_exact(hip, "narrow", b, hw, cin, cout, d, 5000)


# ---- 2. bit links to the forms that exist ----------------------------------------------------------------------------------------

def float_case(b, hw, cin, cout, seed, scale=1.0):
    """Post-ReLU activations, He-scaled weights, a residual and a real BN."""
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(b, cin, *hw, generator=g)) * scale
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    r = torch.randn(b, cout, *hw, generator=g) * scale
    bn = (torch.randn(cout, generator=g) * 0.3, torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g),
          torch.randn(cout, generator=g))
    return x, wt, r, tuple(t.to(DEV) for t in bn)


@pytest.mark.parametrize("b,hw,cin,cout,d", [(2, (9, 13), 48, 256, 2), (1, (7, 7), 16, 128, 1)])
def test_residual_entry_links(hip, b, hw, cin, cout, d):
    x, wt, r, bn = float_case(b, hw, cin, cout, 21 + d)
    pk = pack_of(hip, "res", wt)
    z = run(hip, "plain", x, wt, d, 0, "none", bn=bn, pk=pk)
    assert bool(torch.isfinite(z).all())
    for act in ("none", "relu", "leaky_relu"):
        old = run(hip, "plain", x, wt, d, 0, act, bn=bn, pk=pk)
        want = act32(z + r, act)
        assert not torch.equal(want, old)
        for geometry in GEOMETRIES["res"]:
            assert torch.equal(run(hip, "res", x, wt, d, geometry, act, None, bn, pk), old), "residual NULL is skd_conv3x3_split2h_nhwc"
            got = run(hip, "res", x, wt, d, geometry, act, r, bn, pk)
            assert torch.equal(got, want), "%s geometry %d: %d of %d outputs differ from act(z + r)" % (act, geometry, int((got != want).sum()), got.numel())
    # z from the entry itself (activation none, residual NULL) is that z
    assert torch.equal(run(hip, "res", x, wt, d, 0, "none", None, bn, pk), z)


@pytest.mark.parametrize("b,hw,cin,d", [(2, (9, 13), 48, 2), (1, (7, 7), 16, 1)])
def test_narrow_entry_at_128_columns_is_the_wide_entry(hip, b, hw, cin, d):
    x, wt, r, bn = float_case(b, hw, cin, 128, 31 + d)
    pkn, pkw = pack_of(hip, "narrow", wt), pack_of(hip, "res", wt)
    assert pkn.numel() == pkw.numel() and not torch.equal(pkn, pkw), "another image of the same weight"
    for act in ("none", "relu", "leaky_relu"):
        for res in (None, r):
            want = run(hip, "res", x, wt, d, 0, act, res, bn, pkw)
            for geometry in GEOMETRIES["narrow"]:
                assert torch.equal(run(hip, "narrow", x, wt, d, geometry, act, res, bn, pkn), want), (act, res is not None, geometry)
    # and at a Cout only the narrow form takes, with a residual: act(z + r) of its own z
    x, wt, r, bn = float_case(b, hw, cin, 192, 41 + d)
    pk = pack_of(hip, "narrow", wt)
    z = run(hip, "narrow", x, wt, d, 0, "none", None, bn, pk)
    for act in ("none", "relu"):
        assert torch.equal(run(hip, "narrow", x, wt, d, 1, act, r, bn, pk), act32(z + r, act)), act


@pytest.mark.parametrize("b,hw,cin,cout", [(2, (9, 13), 48, 256), (1, (8, 10), 16, 128)])
def test_stride2_is_stride1_at_the_even_pixels(hip, b, hw, cin, cout):
    x, wt, _, bn = float_case(b, hw, cin, cout, 51)
    pk = pack_of(hip, "s2", wt)
    for act in ("none", "relu"):
        want = run(hip, "plain", x, wt, 1, 0, act, bn=bn, pk=pk)[:, :, ::2, ::2]
        for geometry in GEOMETRIES["s2"]:
            got = run(hip, "s2", x, wt, 1, geometry, act, bn=bn, pk=pk)
            assert got.shape == want.shape and torch.equal(got, want), (act, geometry)
    # leaky ReLU is refused, like the twin
    dx = x.to(DEV).contiguous(memory_format=torch.channels_last)
    out = torch.empty(b * 64 * cout, device=DEV)
    assert hip.skd_conv3x3_split2h_s2_nhwc(b, *hw, cin, cout, P(dx), P(pk), P(out), None, None, None, None, None, 0.0,
                                           ACT["leaky_relu"], SLOPE, 0, None) == 0


# ---- 3. accuracy -------------------------------------------------------------------------------------------------------------------

SCALES = T2H.SCALES


def _truth(kind, x, wt, d, r):
    y = F.conv2d(x.double(), wt.double(), None, 2 if kind == "s2" else 1, d, d)
    return y if r is None else y + r.double()


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("kind,cout,res", [("res", 256, True), ("narrow", 192, False), ("narrow", 192, True), ("s2", 256, False)])
def test_accuracy_against_the_three_piece_twin(hip, kind, cout, res, scale):
    x, wt, r, _ = float_case(2, (9, 13), 48, cout, 8, scale)
    r = r if res else None
    for d in ((1,) if kind == "s2" else (1, 2)):
        truth = _truth(kind, x, wt, d, r)
        e3 = R.rel_err(run(hip, kind, x, wt, d, 0, "none", r, fp16=False), truth)
        eh = R.rel_err(run(hip, kind, x, wt, d, 0, "none", r), truth)
        print("ACC| %s%s 2x9x13 C48 N%d d%d | x%g | %.3e | %.3e | %.2f |" % ("wide" if kind == "res" else kind, "+res" if res else "", cout, d,
                                                                              scale, e3, eh, eh / e3))
        assert eh <= 2 * e3, "%s x%g d%d: fp16 two pieces %.3e > 2 x three pieces %.3e" % (kind, scale, d, eh, e3)


# ---- 4. overflow is loud -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,cout,res", [("res", 128, True), ("narrow", 64, False), ("narrow", 64, True), ("s2", 128, False)])
def test_overflow_is_loud(hip, kind, cout, res):
    """|a| = 70000 > 65504: a0 is infinite and its residual the opposite infinity, so every output whose window reads the value is
    non-finite -- never a finite wrong value -- and every other output is the bits of the run without it."""
    x, wt, r, bn = float_case(2, (9, 13), 16, cout, 9)
    x = x + 0.01
    r = r if res else None
    stride = 2 if kind == "s2" else 1
    for d in ((1,) if kind == "s2" else (1, 2)):
        pk = pack_of(hip, kind, wt)
        base = run(hip, kind, x, wt, d, 0, "none", r, bn, pk)
        assert bool(torch.isfinite(base).all())
        hot = x.clone()
        hot[1, 3, 3, 5] = 70000.0
        mark = torch.zeros(2, 1, 9, 13)
        mark[1, 0, 3, 5] = 1.0
        reads = F.conv2d(mark, torch.ones(1, 1, 3, 3), None, stride, d, d)[:, 0] > 0
        assert int(reads.sum()) == (4 if kind == "s2" else 9)
        for geometry in GEOMETRIES[kind][:2]:
            got = run(hip, kind, hot, wt, d, geometry, "none", r, bn, pk)
            bad = ~torch.isfinite(got)
            assert torch.equal(bad, reads[:, None].expand_as(bad)), "exactly the windows that read it are non-finite"
            assert torch.equal(got[~bad], base[~bad])


# ---- 5. guard bands ------------------------------------------------------------------------------------------------------------------

def test_guard_bands_around_every_operand(hip):
    """x, the pack at exactly pack_bytes, the residual and out of the three entries (and the narrow pack entry) between 0xFF guards,
    the outputs pre-filled with 0xFF: an element the kernel did not write shows as NaN."""
    g = torch.Generator().manual_seed(5)
    A = BC.Arena(DEV)
    b, h, w, cin, d = 2, 9, 13, 48, 2
    x = A.inp("x", torch.relu(torch.randn(b, h, w, cin, generator=g)), row=cin)
    vec = lambda name, n, pos=False: A.inp(name, torch.rand(n, generator=g) + 0.5 if pos else torch.randn(n, generator=g))
    outs = {}
    for kind, cout in (("res", 256), ("narrow", 192), ("s2", 128)):
        wt = A.inp("w_" + kind, torch.randn(cout, cin, 3, 3, generator=g) * 0.1)
        cb, mean, var, ga, be = (vec("cbias", cout), vec("mean", cout), vec("var", cout, True), vec("gamma", cout), vec("beta", cout))
        nbytes = (hip.skd_conv3x3_narrow2h_pack_bytes if kind == "narrow" else hip.skd_conv3x3_split2h_pack_bytes)(cin, cout)
        assert nbytes == 4 * cout * cin * 9
        pk = A.out("pack_" + kind, nbytes, torch.uint8, row=4096)
        pack_of(hip, kind, wt, buf=pk)
        ho, wo = out_hw(kind, h, w)
        epi = (P(cb), P(mean), P(var), P(ga), P(be), EPS, ACT["relu"], SLOPE)
        ys = []
        for geometry in GEOMETRIES[kind]:
            y = A.out("y_%s%d" % (kind, geometry), (b, ho, wo, cout), row=cout)
            if kind == "s2":
                assert hip.skd_conv3x3_split2h_s2_nhwc(b, h, w, cin, cout, P(x), P(pk), P(y), *epi, geometry, None)
            else:
                r = A.inp("r_%s%d" % (kind, geometry), torch.randn(b, h, w, cout, generator=torch.Generator().manual_seed(6)), row=cout)
                entry = hip.skd_conv3x3_split2h_res_nhwc if kind == "res" else hip.skd_conv3x3_narrow2h_nhwc
                assert entry(b, h, w, cin, cout, d, P(x), P(pk), P(y), P(r), *epi, geometry, None)
                # a residual that overlaps the output is refused on the host
                assert entry(b, h, w, cin, cout, d, P(x), P(pk), P(y), P(y), *epi, geometry, None) == 0
            ys.append(y)
        outs[kind] = ys
    A.check()
    for kind, ys in outs.items():
        for y in ys:
            assert bool(torch.isfinite(y).all()), "%s: an output element was not written" % kind
            assert torch.equal(y, ys[0]), kind


# ---- 6. the ops ------------------------------------------------------------------------------------------------------------------------

class _BN:
    def __init__(self, bn, eps=EPS, slope=SLOPE):
        self.running_mean, self.running_var, self.weight, self.bias = bn
        self.eps, self.slope = eps, slope


def test_ops_give_the_entries_bits(hip):
    x, wt, r, bn = float_case(2, (9, 13), 48, 256, 61)
    dx = x.to(DEV).contiguous(memory_format=torch.channels_last)
    dr = r.to(DEV).contiguous(memory_format=torch.channels_last)
    conv = torch.nn.Conv2d(48, 256, 3, 1, 2, 2, bias=False).to(DEV).eval()
    conv.weight.data.copy_(wt)
    with torch.no_grad():
        pkh = SF.conv3x3_pack_weights_fp16(conv)
        got = SF.conv3x3_split_res_eval_fp16(dx, pkh, 256, 2, dr, _BN(bn), "relu")
        assert torch.equal(got.cpu(), run(hip, "res", x, wt, 2, 0, "relu", r, bn))
        none = SF.conv3x3_split_res_eval_fp16(dx, pkh, 256, 2, None, _BN(bn), "relu")
        assert torch.equal(none, SF.conv3x3_split_eval_fp16(dx, pkh, 256, 2, None, _BN(bn), "relu"))
        with pytest.raises(ValueError):
            SF.conv3x3_split_res_eval_fp16(dx, SF.conv3x3_pack_weights(conv), 256, 2, dr, _BN(bn), "relu")      # three planes
        # stride 2 on the same cached pack
        c2 = torch.nn.Conv2d(48, 256, 3, 2, 1, 1, bias=False).to(DEV).eval()
        c2.weight.data.copy_(wt)
        got = SF.conv3x3_s2_eval_fp16(dx, SF.conv3x3_pack_weights_fp16(c2), 256, None, _BN(bn), "relu")
        assert got.shape == (2, 256, 5, 7) and torch.equal(got.cpu(), run(hip, "s2", x, wt, 1, 0, "relu", None, bn))
        with pytest.raises(ValueError):
            SF.conv3x3_s2_eval_fp16(dx, SF.conv3x3_pack_weights(c2), 256)
        # the narrow form: its own pack, in its own slot beside the three-piece one
        xn, wn, rn, bnn = float_case(2, (9, 13), 48, 192, 62)
        cn = torch.nn.Conv2d(48, 192, 3, 1, 1, 1, bias=False).to(DEV).eval()
        cn.weight.data.copy_(wn)
        p3, ph = SF.conv3x3_narrow_pack_weights(cn), SF.conv3x3_narrow_pack_weights_fp16(cn)
        assert SF.conv3x3_narrow_pack_weights_fp16(cn) is ph and SF.conv3x3_narrow_pack_weights(cn) is p3
        assert ph.numel() == 192 * 48 * 36 and p3.numel() == 192 * 48 * 54
        assert torch.equal(ph, pack_of(hip, "narrow", wn))
        assert hasattr(cn, "_skd_conv3x3_narrow_pack") and hasattr(cn, "_skd_conv3x3_narrow_pack2h")
        dxn = xn.to(DEV).contiguous(memory_format=torch.channels_last)
        drn = rn.to(DEV).contiguous(memory_format=torch.channels_last)
        got = SF.conv3x3_narrow_eval_fp16(dxn, ph, 192, 1, drn, None, _BN(bnn), "relu")
        assert torch.equal(got.cpu(), run(hip, "narrow", xn, wn, 1, 0, "relu", rn, bnn))
        with pytest.raises(ValueError):
            SF.conv3x3_narrow_eval_fp16(dxn, p3, 192, 1)
        # a written weight rebuilds the pack
        cn.weight.mul_(2.0)
        assert SF.conv3x3_narrow_pack_weights_fp16(cn) is not ph
    SF.drop_conv3x3_packs(cn)
    assert not hasattr(cn, "_skd_conv3x3_narrow_pack") and not hasattr(cn, "_skd_conv3x3_narrow_pack2h")
    SF.drop_conv3x3_packs(conv)
    assert not hasattr(conv, "_skd_conv3x3_pack2h")


# ---- 7. a flagged small student ------------------------------------------------------------------------------------------------------

COUNTED = NEW + ("skd_conv3x3_split2h_nhwc",) + TWIN + ("skd_conv3x3_split_nhwc",)


def small_student():
    torch.manual_seed(71)
    return TP.seeded(PC.Res_pspnet(PC.BasicBlock, [2, 2, 2, 2], 19), 72)


def test_flagged_small_student_eager_equals_graph_replay(monkeypatch):
    """The student flagged with narrow, stride2 and fp16 pieces at 41 x 57 (the pyramid's 6 x 6 level needs a 6 x 8 feature map):
    each of the four fp16 forms is launched and no three-piece twin of them is; one capture and replay gives the eager bits."""
    for name in ("INFER_ROUTING_EXCLUDED", "NARROW_ROUTING_EXCLUDED", "STRIDE2_ROUTING_EXCLUDED", "INFER2H_ROUTING_EXCLUDED"):
        monkeypatch.setattr(PC, name, frozenset())      # the mechanism; the sets are the policy
    net = small_student()
    x = torch.randn(1, 3, 41, 57, generator=torch.Generator().manual_seed(73)).to(DEV).contiguous(memory_format=torch.channels_last)
    with TP.deterministic_library():
        with torch.no_grad():
            three = [t.clone() for t in fuse_for_inference(net, narrow=True, stride2=True)(x)]
        assert fuse_for_inference(net, narrow=True, stride2=True, piece_format="fp16") is net
        _lib.enable_kernel_timing(list(COUNTED))
        try:
            with torch.no_grad():
                want = [t.clone() for t in net(x)]
        finally:
            calls = {k: len(v) for k, v in _lib.disable_kernel_timing().items()}
        print("student at 41 x 57, fp16 pieces: %s" % calls)
        for name in NEW + ("skd_conv3x3_split2h_nhwc",):
            assert calls[name] >= 1, "%s was never launched: %s" % (name, calls)
        for name in TWIN:
            assert calls[name] == 0, "%s: a flagged convolution ran on three pieces: %s" % (name, calls)
        assert all(bool(torch.isfinite(t).all()) for t in want)
        assert not torch.equal(want[0], three[0]), "the fp16 flag changed nothing"
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
        # the flag cleared: the packs are gone and the three-piece flagged bits are back
        fuse_for_inference(net, enable=False)
        assert not any(hasattr(m, a) for m in net.modules() for a in ("_skd_conv3x3_pack2h", "_skd_conv3x3_narrow_pack2h"))
        with torch.no_grad():
            TP.same_outputs(fuse_for_inference(net, narrow=True, stride2=True)(x), three, "three pieces again")


# ---- 8. the whole student against the float64 fixture ------------------------------------------------------------------------------

def test_whole_student_vs_float64_fixture(monkeypatch):
    """tests/golden/student_infer_oracle.pt (float64 records of the seven outputs): the fp16-flagged student's error is at most
    2 x the three-piece flagged student's, output by output, both measured here.  The share of pixels whose argmax differs
    between the two is printed, not asserted."""
    import make_golden_student_infer as G
    monkeypatch.setattr(PC, "INFER2H_ROUTING_EXCLUDED", frozenset())
    fx = torch.load(G.OUT, weights_only=False)
    Pw, x = G.inputs()
    for k, v in G.checksum(Pw).items():
        assert abs(v - fx["checksums"][k]) <= 1e-9 * max(1.0, abs(v)), ("weight RNG drifted from the fixture generator's", k)
    S = PC.Res_pspnet(PC.BasicBlock, [2, 2, 2, 2], 19)
    S.load_state_dict(Pw)
    S = S.to(DEV).to(memory_format=torch.channels_last).eval()
    dx = x.to(DEV).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        three = [t.clone() for t in fuse_for_inference(S, narrow=True, stride2=True)(dx)]
        _lib.enable_kernel_timing(list(NEW))
        try:
            half = [t.clone() for t in fuse_for_inference(S, narrow=True, stride2=True, piece_format="fp16")(dx)]
        finally:
            calls = {k: len(v) for k, v in _lib.disable_kernel_timing().items()}
    assert calls == {"skd_conv3x3_split2h_res_nhwc": 6, "skd_conv3x3_narrow2h_nhwc": 5, "skd_conv3x3_split2h_s2_nhwc": 1}, calls
    differ = float((three[0].argmax(1) != half[0].argmax(1)).double().mean())
    print("STUDENT| argmax differs from the three-piece flagged student at %.3e of the pixels" % differ)
    for name, a, h, r in zip(fx["names"], three, half, fx["outputs"]):
        e3, eh = TSI._rec_err(a, r), TSI._rec_err(h, r)
        print("STUDENT| %-18s | %.3e | %.3e | %.2f |" % (name, e3 / r["norm"], eh / r["norm"], eh / e3))
        assert eh <= 2 * e3, name
