"""CPU side of the student's wide training convolutions on two fp16 pieces with a device-side gradient scale
(include/skd_train2h.h, ``route_training_convs(pieces=2, piece_format="fp16")``, ``student_piece_format`` /
SKD_STUDENT_PIECE_FORMAT): the word -> scale function swept, the float64 model of the scaled product (tests/train2h_ref.py) with
its invariance, its bound and the reason the scale exists, the proofs of the integer cases tests/test_train2h_gpu.py launches, the
header / table / twins and the host-side refusals of the built library, and the ops, the routing and the configuration switch
under test doubles."""
import copy
import ctypes
import inspect
import math
import os
import struct
import warnings

import numpy as np
import pytest
import torch

import split2_ref as R
import split_exact as SE
import train2h_ref as T
import structure_knowledge_distillation_amd.networks.pspnet_combine as PC
from oracle import cref
from structure_knowledge_distillation_amd import _lib, functional as SF
from structure_knowledge_distillation_amd import networks
from structure_knowledge_distillation_amd.networks import kd_model as KD
from test_conv1x1_train_cpu import ShortcutDouble
from test_conv3x3_narrow_wgrad_cpu import NARROW_ROUTED, NarrowWgradDouble
from test_conv3x3_train_cpu import ROUTED, TrainDouble, _input, _step, _student
from test_student_infer_cpu import _host

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
WORD_BYTES, WORD, PACK_PAIR, SCALED = ("skd_fp16_scale_word_workspace_bytes", "skd_fp16_scale_word",
                                       "skd_conv3x3_split2h_pack_pair", "skd_conv3x3_split2h_scaled_nhwc")
PLAN, WGRAD = "skd_conv3x3_split2h_wgrad_plan", "skd_conv3x3_split2h_wgrad_nhwc"
FWD, BYTES = "skd_conv3x3_split2h_nhwc", "skd_conv3x3_split2h_pack_bytes"
NAMES = [WORD_BYTES, WORD, PACK_PAIR, SCALED, PLAN, WGRAD]


def f32(word):
    return struct.unpack("<f", struct.pack("<I", word))[0]


# ---- 1. the word -> scale function ------------------------------------------------------------------------------------------------

def _is_normal_power_of_two(v):
    m, e = math.frexp(v)
    return m == 0.5 and -125 <= e <= 128 and struct.unpack("<f", struct.pack("<f", v))[0] == v


def test_scale_of_every_exponent_field():
    for field in range(0, 255):
        for mant in (0, 1, 0x400000, 0x7FFFFF):
            word = (field << 23) | mant
            if word == 0:
                continue
            s, inv = T.scale_of_word(word)
            assert _is_normal_power_of_two(s) and _is_normal_power_of_two(inv), hex(word)
            assert s * inv == 1.0
            e = field - 127
            assert s == 2.0 ** max(-126, min(126, 14 - e)), hex(word)
            if e >= -112:
                assert 2.0 ** 14 <= f32(word) * s < 2.0 ** 15, hex(word)
                assert f32(word) * s <= 65504.0
            else:        # the clamp: amax below 2^-112 is scaled by 2^126 and stays below 2^14
                assert s == 2.0 ** 126 and f32(word) * s < 2.0 ** 14


def test_scale_of_the_special_words():
    assert T.scale_of_word(0) == (1.0, 1.0)
    for word in (0x7F800000, 0x7F800001, 0x7FC00000, 0x7FFFFFFF):          # infinity, NaN patterns: never masked
        assert T.scale_of_word(word) == (1.0, 1.0), hex(word)
    for word in (1, 0x1234, 0x7FFFFF):                                     # fp32 subnormals count as e = -127
        assert T.scale_of_word(word) == (2.0 ** 126, 2.0 ** -126), hex(word)
    assert T.scale_of_word(0x7F7FFFFF) == (2.0 ** -113, 2.0 ** 113)          # the largest finite value lands below 2^15
    assert 2.0 ** 14 <= f32(0x7F7FFFFF) * 2.0 ** -113 < 2.0 ** 15
    assert T.scale_of_word(0x3F800000) == (2.0 ** 14, 2.0 ** -14)            # amax 1.0
    # the word of a tensor: the sign is masked, a NaN or an infinity wins
    assert T.word_of(torch.tensor([0.5, -3.0, 1.0])) == 0x40400000
    assert T.word_of(torch.tensor([0.5, float("-inf"), 1.0])) == 0x7F800000
    assert T.word_of(torch.tensor([0.5, float("nan"), 1e30])) >= 0x7F800001
    assert T.word_of(torch.zeros(5)) == 0 and T.word_of(-torch.zeros(5)) == 0


# ---- 2. the float64 model of the scaled product -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def table():
    rows = {}
    for name, (g, w) in T.table_classes().items():
        y64 = g.double() @ w.double().t()
        e3 = float((R.mm_split2(g, w, 3) - y64).abs().max())
        rows[name] = dict(g=g, w=w, y64=y64, e3=e3, scaled=T.mm_scaled(g, w), unscaled=T.mm_scaled(g, w, scaled=False))
    return rows


def test_model_is_scale_invariant_bit_for_bit(table):
    g, w, base = table["N(0,1)"]["g"], table["N(0,1)"]["w"], table["N(0,1)"]["scaled"]
    for k in (-60, -40, -20, 10, 40, 100):
        assert torch.equal(T.mm_scaled(g * 2.0 ** k, w), base * 2.0 ** k), k


def test_model_is_within_the_bound_on_the_five_classes(table):
    for name, r in table.items():
        err = (r["scaled"] - r["y64"]).abs()
        bound = T.bound(SE.gemm_op, r["g"], r["w"], "a", r["e3"])
        share = float((err / bound).max())
        print("%-22s scaled %.2e of max|y|, share of the bound %.3f" % (name, float(err.max()) / float(r["y64"].abs().max()), share))
        assert bool(torch.isfinite(r["scaled"]).all()) and share <= 1.0, name


def test_the_scale_is_what_buys_the_small_and_the_large_gradients(table):
    rel = lambda r, key: float((r[key] - r["y64"]).abs().max()) / float(r["y64"].abs().max())
    assert rel(table["N(0,1) 2^-30"], "unscaled") >= 1e-3 and rel(table["N(0,1) 2^-30"], "scaled") <= 2e-7
    assert rel(table["N(0,1) 1e-12"], "unscaled") >= 0.5 and rel(table["N(0,1) 1e-12"], "scaled") <= 2e-7         # all lost
    assert rel(table["rows e^-25..1, 1e-6"], "unscaled") >= 10 * rel(table["rows e^-25..1, 1e-6"], "scaled")
    assert not bool(torch.isfinite(table["N(0,1) 3e5"]["unscaled"]).all()), "above 65504 an unscaled split is not finite"
    assert bool(torch.isfinite(table["N(0,1) 3e5"]["scaled"]).all()) and rel(table["N(0,1) 3e5"], "scaled") <= 2e-7


def test_a_non_finite_gradient_stays_loud():
    g, w = (t.clone() for t in T.table_classes()["N(0,1)"])
    for poison in (float("inf"), float("nan")):
        gp = g.clone()
        gp[3, 7] = poison
        assert T.scale_of(gp) == (1.0, 1.0)
        assert not bool(torch.isfinite(T.mm_scaled(gp, w)[3]).any())


# ---- 3. the integer cases of the GPU file, proven here ------------------------------------------------------------------------------

def test_case_table_covers_the_issue():
    assert len(T.CASES) == 2 * 2 * 3 * 2 * 2 and len({c.name for c in T.CASES}) == len(T.CASES)
    assert {(c.cin, c.cout) for c in T.CASES} == {(128, 256), (256, 128)} and {c.d for c in T.CASES} == {1, 2, 4}
    assert {c.shift for c in T.CASES} == {-40, 20} and {c.product for c in T.CASES} == {"dgrad", "wgrad"}
    assert (T.B * T.H * T.W) % 16 != 0 and T.B * T.H * T.W > 128 and (T.B * T.H * T.W - 128) % 64 != 0 and T.WGRAD_SLICES == (1, 3)


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.name)
def test_integer_case_is_what_it_claims(case):
    built = T.build(case)
    up = 2.0 ** case.shift
    for cls, t, is_g in zip(case.kind, (built.a, built.b), (built.g_is == "a", built.g_is == "b")):
        v = t.double() / (up if is_g else 1.0)
        nz = v != 0
        assert int(nz.sum()) > 0
        if cls == "N":
            assert set(v[nz].abs().tolist()) <= {1.0, 2.0}, "one piece"
        else:
            assert bool((v[nz].abs() >= 1).all()) and bool((v[nz].abs() < 2).all())
            assert torch.equal(v * 2.0 ** 21, (v * 2.0 ** 21).round()), "22 significant bits"
    # the scaled g: its largest magnitude in [2^14, 2^15); both pieces of every value exact, nothing dropped
    s, inv = T.scale_of(built.g)
    gs = built.g.float() * s
    assert 2.0 ** 14 <= float(gs.abs().max()) < 2.0 ** 15 and s * inv == 1.0
    for t in (gs, built.b if built.g_is == "a" else built.a):
        p0, p1 = T.RH.pieces(t)
        assert torch.equal(p0 + p1 / T.RH.SCALE, t.double()), "two fp16 pieces hold the value"
    exact, model = built.exact(), built.model()
    assert float(exact.abs().max()) > 0 and torch.equal(exact.float().double(), exact), "the exact product is an fp32 value"
    assert torch.equal(model, exact), "the three products of the scaled split ARE the exact product"
    # each output is a sum of two products at most, so every partial sum is exact whatever the order
    count = built.op((built.a != 0).double(), (built.b != 0).double())
    assert float(count.max()) <= 2.0
    # power: hi alone is not the answer, and WITHOUT the scale the case fails (g below fp16's subnormals / above 65504)
    a0, b0 = T.RH.pieces(gs if built.g_is == "a" else built.a)[0], T.RH.pieces(built.b if built.g_is == "a" else gs)[0]
    assert not torch.equal(built.op(a0, b0) * inv, exact)
    unscaled = built.model(scaled=False)
    assert not torch.equal(torch.nan_to_num(unscaled, nan=-1.0), exact)
    if case.shift < 0:
        assert float(unscaled.abs().max()) == 0.0, "2^-40: every piece of an unscaled g is zero"
    else:
        assert not bool(torch.isfinite(unscaled).all()), "2^20: an unscaled g is above fp16's range"


# ---- 4. header, table, twins, host-side refusals ------------------------------------------------------------------------------------

def test_header_table_and_twins():
    assert sorted(_lib.ABI["skd_train2h.h"]) == sorted(NAMES)
    assert _lib.signature(PACK_PAIR) == _lib.signature("skd_conv3x3_split2_pack_pair")
    assert _lib.signature(PLAN) == _lib.signature("skd_conv3x3_split2_wgrad_plan")
    r2, a2 = _lib.signature("skd_conv3x3_split2_wgrad_nhwc")
    rh, ah = _lib.signature(WGRAD)
    assert rh is r2 and list(ah) == list(a2[:15]) + [ctypes.c_void_p] + list(a2[15:]), "the twin's list plus the word"
    rf, af = _lib.signature(FWD)
    rs, as_ = _lib.signature(SCALED)
    assert rs is rf and list(as_) == list(af[:9]) + [ctypes.c_void_p] + list(af[-2:]), "x, wpack, out, the word, geometry, stream"
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name)
    text = open(_lib.header_path("skd_train2h.h")).read()
    for word in ("0x7fffffff", "0x7f800000", "2^14, 2^15", "65504", "bit for bit", "2^-21", "2^-49", "NOT scaled"):
        assert word in text, word
    assert "skd_train2h.h" in open(_lib.header_path("skd_train2.h")).read(), "the bf16 header points to the fp16 form"


def test_plan_is_the_three_piece_plan_and_the_word_needs_its_workspace():
    lib = _lib.load()
    for args in ((2, 9, 11, 128, 256, 0, 256), (2, 9, 11, 256, 128, 3, 0), (8, 65, 65, 512, 512, 0, 256), (1, 1, 1, 128, 128, 1, 4)):
        ph, p3 = (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)()
        assert lib.skd_conv3x3_split2h_wgrad_plan(*args, ctypes.cast(ph, ctypes.c_void_p)) == 1
        assert lib.skd_conv3x3_split_wgrad_plan(*args, ctypes.cast(p3, ctypes.c_void_p)) == 1
        assert list(ph) == list(p3), args
    plan = (ctypes.c_int64 * 3)()
    for bad in ((0, 9, 11, 128, 128, 0, 0), (2, 9, 11, 64, 128, 0, 0), (2, 9, 11, 128, 192, 0, 0), (2, 9, 11, 128, 128, -1, 0)):
        assert lib.skd_conv3x3_split2h_wgrad_plan(*bad, ctypes.cast(plan, ctypes.c_void_p)) == 0, bad
    assert lib.skd_conv3x3_split2h_wgrad_plan(2, 9, 11, 128, 128, 0, 0, None) == 0
    q = lib.skd_fp16_scale_word_workspace_bytes
    assert q(0) == 0 and q(-5) == 0 and q(1) == 4 and q(4097) == 4
    sizes = [q(n) for n in (1, 65536, 65537, 1 << 20, 1 << 26, 1 << 32)]
    assert all(s % 4 == 0 and 4 <= s <= 4096 for s in sizes) and sizes == sorted(sizes) and sizes[-1] == 4096


def test_host_side_refusals_follow_no_pointer():
    """Every refusal is decided in front of the launch: the addresses below are never followed and no device is touched."""
    lib = _lib.load()
    G, WS, WD = 0x10000, 0x2000000, 0x4000000
    ok = dict(n=4097, g=G, ws=WS, wb=4, word=WD)

    def word(**kw):
        a = dict(ok, **kw)
        return lib.skd_fp16_scale_word(a["n"], a["g"], a["ws"], a["wb"], a["word"], None)
    for bad in (dict(g=None), dict(ws=None), dict(word=None), dict(n=0), dict(n=-1), dict(g=G + 4), dict(g=G + 8), dict(wb=3), dict(wb=0),
                dict(ws=WS + 2), dict(word=WD + 1), dict(n=1 << 20, wb=4)):
        assert word(**bad) == 0, bad
    W, PF, PB = 0x10000, 0x2000000, 0x4000000
    n = 128 * 128 * 36
    okp = dict(cin=128, cout=128, w=W, sn=1152, sc=9, sy=3, sx=1, pf=PF, fb=n, pb=PB, bb=n)

    def pair(**kw):
        a = dict(okp, **kw)
        return lib.skd_conv3x3_split2h_pack_pair(a["cin"], a["cout"], a["w"], a["sn"], a["sc"], a["sy"], a["sx"], a["pf"], a["fb"], a["pb"],
                                                 a["bb"], None)
    for bad in (dict(w=None), dict(pf=None, pb=None), dict(pf=PF + 8), dict(pb=PB + 4), dict(fb=n - 1), dict(bb=n - 1), dict(fb=0),
                dict(sn=-1), dict(sc=-9), dict(sy=-3), dict(sx=-1), dict(cin=64), dict(cout=64), dict(cin=24), dict(cout=0),
                dict(cout=32, pb=None), dict(cin=32, pf=None)):
        assert pair(**bad) == 0, bad
    X, PK, OUT = 0x10000, 0x2000000, 0x4000000
    oks = dict(B=2, H=9, W=11, cin=128, cout=256, d=2, x=X, pk=PK, out=OUT, word=WD, geo=0)

    def scaled(**kw):
        a = dict(oks, **kw)
        return lib.skd_conv3x3_split2h_scaled_nhwc(a["B"], a["H"], a["W"], a["cin"], a["cout"], a["d"], a["x"], a["pk"], a["out"], a["word"],
                                                   a["geo"], None)
    for bad in (dict(word=None), dict(word=WD + 2), dict(x=None), dict(pk=None), dict(out=None), dict(x=X + 4), dict(pk=PK + 8), dict(B=0),
                dict(H=0), dict(W=-1), dict(cin=24), dict(cout=192), dict(d=0), dict(geo=-1), dict(geo=4)):
        assert scaled(**bad) == 0, bad
    XX, GG, DW, WSS = 0x10000, 0x2000000, 0x4000000, 0x8000000
    nk = -(-2 * 9 * 11 // 16)
    ws = 9 * 128 * 128 * 4
    good = dict(B=2, H=9, W=11, cin=128, cout=128, d=1, x=XX, g=GG, dw=DW, sn=1152, sc=9, sy=3, sx=1, ws=WSS, wb=ws, word=WD, slices=1)

    def wgrad(**kw):
        a = dict(good, **kw)
        return lib.skd_conv3x3_split2h_wgrad_nhwc(a["B"], a["H"], a["W"], a["cin"], a["cout"], a["d"], a["x"], a["g"], a["dw"], a["sn"],
                                                  a["sc"], a["sy"], a["sx"], a["ws"], a["wb"], a["word"], a["slices"], None)
    for bad in (dict(x=None), dict(g=None), dict(dw=None), dict(ws=None), dict(x=XX + 4), dict(g=GG + 8), dict(ws=WSS + 4), dict(wb=ws - 1),
                dict(sn=-1), dict(sc=-1), dict(sy=-1), dict(sx=-1), dict(slices=0), dict(slices=nk + 1), dict(slices=2, wb=ws), dict(d=0),
                dict(B=0), dict(H=0), dict(W=-1), dict(cin=64), dict(cout=192), dict(word=WD + 2)):
        assert wgrad(**bad) == 0, bad


# ---- 5. the ops and the routing under doubles ---------------------------------------------------------------------------------------

class Fp16Entries:
    """The entries of skd_train2h.h and the two of skd_split2h.h they build on, on raw HOST addresses, computed in fp32 like the
    three-piece ones (wiring: they say which entry ran on which pack with which word, not how).  A mix-in in front of a
    TrainDouble; the owner's ``__init__`` makes ``pairs2h``, ``words`` and ``wgrads2h``."""

    def skd_conv3x3_split2h_pack_bytes(self, cin, cout):
        return cout * cin * 36 if self.skd_conv3x3_split_supported(cin, cout, 1, 1, 1, 1) else 0

    def skd_conv3x3_split2h_pack_pair(self, cin, cout, w, sn, sc, sy, sx, pack_fwd, fwd_bytes, pack_bwd, bwd_bytes, stream):
        assert fwd_bytes == bwd_bytes == cin * cout * 36
        n = len(self.pairs)
        ok = TrainDouble.skd_conv3x3_split_pack_pair(self, cin, cout, w, sn, sc, sy, sx, pack_fwd, cin * cout * 54, pack_bwd,
                                                     cin * cout * 54, stream)
        self.pairs2h.append(self.pairs.pop(n))
        return ok

    def skd_conv3x3_split2h_nhwc(self, B, H, W, cin, cout, dil, x, pack, out, cbias, mean, var, weight, bias, eps, act, slope,
                                 geometry, stream):
        return self._conv(FWD, B, H, W, cin, cout, dil, x, pack, out, None, cbias, mean, var, weight, bias, eps, act, slope)

    def skd_fp16_scale_word_workspace_bytes(self, n):
        return 4 if n >= 1 else 0

    def skd_fp16_scale_word(self, n, g, ws, ws_bytes, word, stream):
        assert g and ws and word and ws_bytes >= 4
        bits = _host(g, (n,)).view(np.uint32) & 0x7FFFFFFF
        ctypes.c_uint32.from_address(word).value = int(bits.max())
        self.words.append(dict(n=n, g=g, word=word, value=int(bits.max())))
        return 1

    def skd_conv3x3_split2h_scaled_nhwc(self, B, H, W, cin, cout, dil, x, pack, out, word, geometry, stream):
        assert word, "the scaled entry takes a word"
        ok = self._conv(SCALED, B, H, W, cin, cout, dil, x, pack, out, None, None, None, None, None, None, 0.0, 0, 0.01)
        self.calls[-1]["word"] = (word, ctypes.c_uint32.from_address(word).value)
        return ok

    def skd_conv3x3_split2h_wgrad_plan(self, B, H, W, cin, cout, slices, cus, plan):
        out = (ctypes.c_int64 * 3).from_address(plan if isinstance(plan, int) else plan.value)
        out[0], out[1], out[2] = 1, -(-B * H * W // 16), 16
        return 1

    def skd_conv3x3_split2h_wgrad_nhwc(self, B, H, W, cin, cout, dil, x, g, dw, sn, sc, sy, sx, ws, ws_bytes, word, slices, stream):
        xt = torch.from_numpy(_host(x, (B, H, W, cin)).copy()).permute(0, 3, 1, 2)
        gt = torch.from_numpy(_host(g, (B, H, W, cout)).copy()).permute(0, 3, 1, 2)
        want = torch.nn.grad.conv2d_weight(xt, (cout, cin, 3, 3), gt, 1, dil, dil)
        base = _host(dw, (1 + (cout - 1) * sn + (cin - 1) * sc + 2 * sy + 2 * sx,))
        np.lib.stride_tricks.as_strided(base, shape=(cout, cin, 3, 3), strides=tuple(4 * s for s in (sn, sc, sy, sx)))[...] = want.numpy()
        self.wgrads2h.append(dict(cin=cin, cout=cout, dilation=dil, g=g, word=(word, ctypes.c_uint32.from_address(word).value if word else None)))
        return 1


class Train2hDouble(Fp16Entries, TrainDouble):
    """TrainDouble + the fp16 entries; skd_wgrad.h is absent (the fp16 weight gradient does not depend on it)."""

    def __init__(self, core, compute):
        super().__init__(core, compute)
        self.pairs2h, self.words, self.wgrads2h = [], [], []


class FullDouble(Fp16Entries, NarrowWgradDouble):
    """Every training entry a flagged student can reach: skd_train.h, skd_wgrad.h, skd_narrow.h, skd_narrow_wgrad.h (NarrowWgradDouble),
    skd_shortcut.h (ShortcutDouble's entries, borrowed) and the fp16 ones."""

    def __init__(self, core, compute):
        super().__init__(core, compute)
        self.pairs2h, self.words, self.wgrads2h = [], [], []
        self.fwd, self.dgrad, self.wgrad = [], [], []          # ShortcutDouble's logs

    skd_conv1x1_train_supported = ShortcutDouble.skd_conv1x1_train_supported
    skd_conv1x1_train_fwd_nhwc = ShortcutDouble.skd_conv1x1_train_fwd_nhwc
    skd_conv1x1_train_dgrad_nhwc = ShortcutDouble.skd_conv1x1_train_dgrad_nhwc
    skd_conv1x1_train_wgrad_plan = ShortcutDouble.skd_conv1x1_train_wgrad_plan
    skd_conv1x1_train_wgrad_nhwc = ShortcutDouble.skd_conv1x1_train_wgrad_nhwc


@pytest.fixture
def fp16_double():
    d = Train2hDouble(cref.load(_lib.SIGNATURES), compute=True)
    _lib.install_test_backend(d)
    yield d
    _lib.install_test_backend(None)


@pytest.fixture
def three_only():
    d = TrainDouble(cref.load(_lib.SIGNATURES), compute=True)
    _lib.install_test_backend(d)
    yield d
    _lib.install_test_backend(None)


def test_plain_c_double_lacks_the_entries_and_the_ops_say_so(three_only):
    assert not any(_lib.has_entry(n) for n in _lib.ABI["skd_train2h.h"]) and not SF.train2h_supported()
    conv = torch.nn.Conv2d(128, 128, 3, 1, 1, 1, bias=False).to(memory_format=torch.channels_last)
    x = torch.randn(1, 128, 4, 5).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    with pytest.raises(NotImplementedError, match=r"skd_fp16_scale_word_workspace_bytes \(include/skd_train2h.h\)"):
        SF.fp16_scale_word(x.detach())
    with pytest.raises(NotImplementedError, match=r"skd_conv3x3_split2h_pack_pair \(include/skd_train2h.h\)"):
        SF.conv3x3_train_packs_fp16(conv.weight, conv)
    with pytest.raises(NotImplementedError, match=r"skd_conv3x3_split2h_wgrad_plan \(include/skd_train2h.h\)"):
        SF.conv3x3_split_wgrad_fp16(x, x, conv.weight, 1)
    with pytest.raises(NotImplementedError, match=r"skd_train2h.h"):
        SF.conv3x3_split_train_fp16(x, conv.weight, 1, None, conv)
    with pytest.raises(NotImplementedError, match=r"skd_train2h.h"):
        SF.ppm_fold_bottleneck_train_fp16([torch.randn(1, 128, 1, 1)], x, torch.randn(128, 256, 3, 3), {}, split_train=True)
    assert three_only.calls == [] and three_only.pairs == []
    # the recorded ops keep their signatures; the twins add nothing but the word
    assert inspect.signature(SF.conv3x3_split_train_fp16) == inspect.signature(SF.conv3x3_split_train)
    assert inspect.signature(SF.conv3x3_train_packs_fp16) == inspect.signature(SF.conv3x3_train_packs)
    assert inspect.signature(SF.ppm_fold_bottleneck_train_fp16) == inspect.signature(SF.ppm_fold_bottleneck_fp16)
    assert list(inspect.signature(SF.conv3x3_split_wgrad_fp16).parameters) == list(inspect.signature(SF.conv3x3_split_wgrad).parameters) + ["word"]
    for f in (SF.conv3x3_split_train, SF.conv3x3_train_packs, SF.conv3x3_split_wgrad, SF.ppm_fold_bottleneck, SF.ppm_fold_bottleneck_fp16):
        assert "word" not in str(inspect.signature(f)) and "piece_format" not in str(inspect.signature(f))


def test_piece_format_validation():
    net = _student()
    for bad in ("fp32", "FP16", None, 16, ""):
        with pytest.raises(ValueError, match="piece_format must be 'bf16' or 'fp16'"):
            networks.route_training_convs(net, pieces=2, piece_format=bad)
    with pytest.raises(ValueError, match="requires pieces=2"):
        networks.route_training_convs(net, pieces=3, piece_format="fp16")
    with pytest.raises(ValueError, match="requires pieces=2"):
        networks.route_training_convs(net, piece_format="fp16")
    assert not any(hasattr(m, "_skd_train_piece_format") or hasattr(m, "_skd_train_min_cin") for m in net.modules()), "refused in front of any mark"
    doc = networks.route_training_convs.__doc__
    for word in ('piece_format="fp16"', "skd_train2h.h", "65504", "STUDENT_FP16_ROUTING_EXCLUDED", "THREE pieces"):
        assert word in doc, word


def _marks(net, attr):
    return [getattr(m, attr, None) for m in net.modules() if isinstance(m, (PC.BasicBlock, PC.ResNet, PC.PSPModule))]


def test_backend_without_the_entries_warns_once_and_keeps_three_pieces(three_only):
    net, inp = _student(), _input()
    with pytest.warns(RuntimeWarning, match="skd_train2h.h") as rec:
        networks.route_training_convs(net, pieces=2, piece_format="fp16")
    assert len([w for w in rec if "skd_train2h.h" in str(w.message)]) == 1
    assert _marks(net, "_skd_train_piece_format") == [None] * 10 and _marks(net, "_skd_train_pieces") == [None] * 10
    net(inp)
    assert [(c["cin"], c["cout"], c["dilation"]) for c in three_only.calls] == ROUTED
    assert {c["entry"] for c in three_only.calls} == {"skd_conv3x3_split_nhwc"}, "three pieces, never two bf16"


def test_routing_takes_the_fp16_entries_for_all_thirteen(fp16_double):
    net, x = _student(), _input()
    plain = copy.deepcopy(net)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        networks.route_training_convs(net, pieces=2, piece_format="fp16")
    assert _marks(net, "_skd_train_piece_format") == ["fp16"] * 10 and _marks(net, "_skd_train_pieces") == [None] * 10
    want_out, want = _step(plain, x)
    assert fp16_double.calls == []
    got_out, got = _step(net, x)
    fw, bw = fp16_double.calls[:13], fp16_double.calls[13:]
    assert {c["entry"] for c in fw} == {FWD} and {c["entry"] for c in bw} == {SCALED}
    assert [(c["cin"], c["cout"], c["dilation"]) for c in fw] == ROUTED
    assert [(c["cout"], c["cin"], c["dilation"]) for c in bw][::-1] == ROUTED
    assert len(fp16_double.pairs2h) == 13 and fp16_double.pairs == [] and fp16_double.wgrads2h == []
    # one word per backward, computed from the very gradient the data gradient reads, and handed over
    assert len(fp16_double.words) == 13
    for c, wd in zip(bw, fp16_double.words):
        assert c["x"] == wd["g"] and c["word"] == (wd["word"], wd["value"]) and wd["n"] % (2 * c["cin"]) == 0 and 0 < wd["value"] < 0x7F800000
    rel = lambda a, b: float((a.detach() - b.detach()).abs().max() / b.detach().abs().max())
    assert all(rel(a, b) <= 1e-6 for a, b in zip(got_out, want_out))
    assert set(got) == set(want) and all(rel(got[k], want[k]) <= 1e-6 for k in want)
    owners = [m for m in net.modules() if isinstance(m, torch.nn.Conv2d) and hasattr(m, SF._TRAIN2H_PACK_ATTR)]
    assert len(owners) == 12 and not any(hasattr(m, "_skd_conv3x3_train_pack") or hasattr(m, SF._TRAIN2_PACK_ATTR) for m in net.modules())
    assert set(net.pspmodule._fold_cache["pack3x3_train"]) == {SF._TRAIN2H_PACK_ATTR}
    # eval-mode and no-grad forwards are untouched
    fp16_double.calls.clear()
    with torch.no_grad():
        net(x)
    net.eval()
    net(x)
    net.train()
    assert fp16_double.calls == []
    # enable=False drops the fp16 packs and the marks
    networks.route_training_convs(net, enable=False)
    assert not any(hasattr(m, SF._TRAIN2H_PACK_ATTR) for m in net.modules()) and "pack3x3_train" not in net.pspmodule._fold_cache
    assert _marks(net, "_skd_train_piece_format") == [None] * 10
    net(x)
    assert fp16_double.calls == []


def test_wgrad_gets_the_same_word_as_the_data_gradient(fp16_double):
    net, x = _student(), _input()
    plain = copy.deepcopy(net)
    networks.route_training_convs(net, wgrad=True, pieces=2, piece_format="fp16")
    _, want = _step(plain, x)
    _, got = _step(net, x)
    bw = [c for c in fp16_double.calls if c["entry"] == SCALED]
    assert len(fp16_double.words) == 13 and len(fp16_double.wgrads2h) == 13 and len(bw) == 13, "the word is computed ONCE per backward"
    for c, wg, wd in zip(bw, fp16_double.wgrads2h, fp16_double.words):
        assert wg["word"] == c["word"] == (wd["word"], wd["value"]) and wg["g"] == c["x"] == wd["g"]
        assert (wg["cin"], wg["cout"], wg["dilation"]) == (c["cout"], c["cin"], c["dilation"])
    rel = lambda a, b: float((a.detach() - b.detach()).abs().max() / b.detach().abs().max())
    assert set(got) == set(want) and all(rel(got[k], want[k]) <= 1e-5 for k in want)


def test_switch_off_and_bf16_two_pieces_see_no_fp16_entry(fp16_double):
    net, x = _student(), _input()
    networks.route_training_convs(net)
    net(x)
    assert {c["entry"] for c in fp16_double.calls} == {"skd_conv3x3_split_nhwc"} and fp16_double.pairs2h == [] and fp16_double.words == []
    assert _marks(net, "_skd_train_piece_format") == [None] * 10
    # fp16 -> bf16 three pieces: the mark goes, the three-piece packs are built beside the fp16 ones
    networks.route_training_convs(net, pieces=2, piece_format="fp16")
    networks.route_training_convs(net, pieces=3)
    assert _marks(net, "_skd_train_piece_format") == [None] * 10


def test_excluded_shape_keeps_three_pieces_never_two(fp16_double, monkeypatch):
    monkeypatch.setattr(PC, "STUDENT_FP16_ROUTING_EXCLUDED", frozenset({(256, 256, 2), (512, 128, 1)}))
    net, x = _student(), _input()
    networks.route_training_convs(net, pieces=2, piece_format="fp16")
    net(x)
    got = [(c["entry"], c["cin"], c["cout"], c["dilation"]) for c in fp16_double.calls]
    want = [("skd_conv3x3_split_nhwc" if s in PC.STUDENT_FP16_ROUTING_EXCLUDED else FWD,) + s for s in ROUTED]
    assert got == want
    assert PC.STUDENT_FP16_ROUTING_EXCLUDED and len(fp16_double.pairs) == 4 and len(fp16_double.pairs2h) == 9


def _full_run(fp16):
    """One step of the student flagged with every opt-in (narrow, narrow_wgrad, shortcut, wgrad) and, ``fp16``, the fp16 mark too,
    on a fresh FullDouble: (the double, outputs, gradients)."""
    d = FullDouble(cref.load(_lib.SIGNATURES), compute=True)
    _lib.install_test_backend(d)
    try:
        net, x = _student(), _input()
        extra = dict(pieces=2, piece_format="fp16") if fp16 else {}
        networks.route_training_convs(net, wgrad=True, narrow=True, narrow_wgrad=True, shortcut=True, **extra)
        out, grads = _step(net, x)
    finally:
        _lib.install_test_backend(None)
    return d, out, grads


def test_stem_shortcuts_and_narrow_forms_stay_on_three_pieces(monkeypatch):
    """Every opt-in together with the fp16 mark: the stem's conv2 / conv3, layer1's four convolutions and the 1x1 shortcuts run the
    entries, on the packs and with the weight gradients they run without the mark; the 13 wide convolutions run the fp16 ones.
    (The measured exclusion sets of the narrow and shortcut weight gradients are emptied, so that every form runs.)"""
    monkeypatch.setattr(PC, "NARROW_WGRAD_ROUTING_EXCLUDED", frozenset())
    monkeypatch.setattr(PC, "SHORTCUT_ROUTING_EXCLUDED", frozenset())
    plain, out3, g3 = _full_run(False)
    half, outh, gh = _full_run(True)
    shape = lambda c: (c["entry"], c["cin"], c["cout"], c["dilation"])
    thin = lambda d: [shape(c) for c in d.calls if c["cin"] % 128 or c["cout"] % 128]
    wide = lambda d: [shape(c) for c in d.calls if not (c["cin"] % 128 or c["cout"] % 128)]
    # the 64-channel forms: the same launches in the same order on both runs, none of them an fp16 entry
    assert thin(half) == thin(plain) and len(thin(plain)) == 12
    assert {e for e, _, _, _ in thin(half)} == {"skd_conv3x3_narrow_nhwc", "skd_conv3x3_split_nhwc"}
    assert [(e, ci, co, dl) for e, ci, co, dl in thin(half)[:6]] == [
        ("skd_conv3x3_split_nhwc" if co % 128 == 0 else "skd_conv3x3_narrow_nhwc", ci, co, dl) for ci, co, dl in NARROW_ROUTED]
    pairs = lambda log: [(p["cin"], p["cout"], bool(p["fwd"]), bool(p["bwd"])) for p in log]
    assert pairs(half.narrow_pairs) == pairs(plain.narrow_pairs) and len(plain.narrow_pairs) == 6
    nwg = lambda d: [(c["cin"], c["cout"], c["dilation"]) for c in d.narrow_wgrads]
    assert nwg(half) == nwg(plain) and sorted(nwg(plain)) == sorted(NARROW_ROUTED)
    # the shortcuts: the same three products of the same shapes
    for log in ("fwd", "dgrad", "wgrad"):
        sc = lambda d: [(c["cin"], c["cout"], c["stride"]) for c in getattr(d, log)]
        assert sc(half) == sc(plain) and len(sc(plain)) == 4, log
    # the 13 wide convolutions: three-piece entries without the mark, fp16 entries with it, and no three-piece launch left
    assert [s[1:] for s in wide(plain)[:13]] == ROUTED and {s[0] for s in wide(plain)} == {"skd_conv3x3_split_nhwc"}
    assert len(plain.wgrads) == 13 and plain.pairs2h == [] and plain.words == [] and plain.wgrads2h == []
    assert [s for s in wide(half)[:13]] == [(FWD,) + r for r in ROUTED]
    assert {s[0] for s in wide(half)[13:]} == {SCALED} and len(wide(half)) == 26
    assert len(half.pairs2h) == 13 and len(half.words) == 13 and len(half.wgrads2h) == 13 and half.wgrads == []
    # the wide three-piece pack pairs of the fp16 run are those of the 64 -> 128 and 128 -> 64 convolutions alone (one image each)
    assert pairs(half.pairs) == [p for p in pairs(plain.pairs) if not (p[2] and p[3])] and len(half.pairs) == 2
    rel = lambda a, b: float((a.detach() - b.detach()).abs().max() / b.detach().abs().max())
    assert all(rel(a, b) <= 1e-5 for a, b in zip(outh, out3))
    assert set(gh) == set(g3) and all(rel(gh[k], g3[k]) <= 1e-4 for k in g3)


def test_the_op_hands_narrow_directions_and_statistics_to_three_pieces():
    d = FullDouble(cref.load(_lib.SIGNATURES), compute=True)
    _lib.install_test_backend(d)
    try:
        x = torch.randn(1, 128, 4, 5).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        thin = torch.nn.Conv2d(128, 64, 3, 1, 1, 1, bias=False).to(memory_format=torch.channels_last)
        y = SF.conv3x3_split_train_fp16(x, thin.weight, 1, None, thin, narrow=True, narrow_wgrad=True)
        y.sum().backward()
        assert d.pairs2h == [] and d.words == [] and not hasattr(thin, SF._TRAIN2H_PACK_ATTR), "a 64-column direction builds no fp16 pack"
        assert [c["entry"] for c in d.calls] == ["skd_conv3x3_narrow_nhwc", "skd_conv3x3_split_nhwc"] and len(d.narrow_wgrads) == 1
        # both sides multiples of 128: ``narrow`` changes nothing, and no three-piece pack is built on the way
        wide = torch.nn.Conv2d(128, 128, 3, 1, 1, 1, bias=False).to(memory_format=torch.channels_last)
        d.calls.clear()
        SF.conv3x3_split_train_fp16(x, wide.weight, 1, None, wide, narrow=True)
        assert [c["entry"] for c in d.calls] == [FWD] and len(d.pairs2h) == 1 and len(d.pairs) == 1 and d.narrow_pairs[1:] == []
        assert not hasattr(wide, "_skd_conv3x3_train_pack")
        with pytest.raises(NotImplementedError, match="skd_bnstats.h"):
            SF.conv3x3_split_train_fp16(x, wide.weight, 1, None, wide, stats=True)
        assert len(d.pairs2h) == 1
    finally:
        _lib.install_test_backend(None)


def test_predicate_reads_its_own_mark():
    class M:
        pass
    m = M()
    assert not PC._student_fp16(m, 128, 128, 1)
    m._skd_train_pieces = 2
    assert not PC._student_fp16(m, 128, 128, 1), "the bf16 mark is another one"
    m._skd_train_piece_format = "fp16"
    _lib.install_test_backend(cref.load(_lib.SIGNATURES))
    try:
        assert not PC._student_fp16(m, 128, 128, 1), "no entries: three pieces"
    finally:
        _lib.install_test_backend(None)
    assert PC.STUDENT_FP16_ROUTING_EXCLUDED == frozenset() or all(len(s) == 3 for s in PC.STUDENT_FP16_ROUTING_EXCLUDED)


def test_fp16_packs_have_a_slot_of_their_own(fp16_double):
    torch.manual_seed(7)
    conv = torch.nn.Conv2d(128, 128, 3, 1, 1, 1, bias=False).to(memory_format=torch.channels_last)
    fh, bh = SF.conv3x3_train_packs_fp16(conv.weight, conv)
    f3, b3 = SF.conv3x3_train_packs(conv.weight, conv)
    assert (fh.numel(), f3.numel()) == (128 * 128 * 36, 128 * 128 * 54) and len(fp16_double.pairs2h) == 1 and len(fp16_double.pairs) == 1
    gh, _ = SF.conv3x3_train_packs_fp16(conv.weight, conv)
    assert gh is fh and len(fp16_double.pairs2h) == 1, "cached per (data_ptr, _version)"
    with torch.no_grad():
        conv.weight.mul_(2.0)
    hh, _ = SF.conv3x3_train_packs_fp16(conv.weight, conv)
    assert hh is not fh and len(fp16_double.pairs2h) == 2
    SF.drop_conv3x3_packs(conv)
    assert not hasattr(conv, SF._TRAIN2H_PACK_ATTR) and not hasattr(conv, "_skd_conv3x3_train_pack")


# ---- 6. the configuration switch ------------------------------------------------------------------------------------------------------

def test_student_piece_format_parsing(monkeypatch):
    for env in ("SKD_STUDENT_PIECES", "SKD_STUDENT_PIECE_FORMAT"):
        monkeypatch.delenv(env, raising=False)
    assert KD.default_args().student_piece_format == "bf16"
    assert KD.default_args(student_pieces=2, student_piece_format="fp16").student_piece_format == "fp16"
    assert KD.default_args(student_pieces=2, student_piece_format=" bf16 ").student_piece_format == "bf16"
    for bad in ("fp32", "", 16, "FP16"):
        with pytest.raises(ValueError, match="SKD_STUDENT_PIECE_FORMAT"):
            KD.default_args(student_pieces=2, student_piece_format=bad)
    with pytest.raises(ValueError, match="requires student_pieces"):
        KD.default_args(student_piece_format="fp16")
    with pytest.raises(ValueError, match="requires student_pieces"):
        KD.default_args(student_pieces=3, student_piece_format="fp16")
    monkeypatch.setenv("SKD_STUDENT_PIECE_FORMAT", "fp16")
    with pytest.raises(ValueError, match="requires student_pieces"):
        KD.default_args()
    monkeypatch.setenv("SKD_STUDENT_PIECES", "2")
    a = KD.default_args()
    assert (a.student_pieces, a.student_piece_format, a.teacher_piece_format, a.infer_piece_format) == (2, "fp16", "bf16", "bf16")
    assert KD.default_args(student_piece_format="bf16").student_piece_format == "bf16"
    assert "student_piece_format" not in [name for name, _, _ in KD.SWITCHES]


def test_netmodel_student_piece_format_flag(monkeypatch):
    for env in ("SKD_STUDENT_PIECES", "SKD_STUDENT_PIECE_FORMAT", "SKD_SPLIT_TRAIN", "SKD_SPLIT_WGRAD"):
        monkeypatch.delenv(env, raising=False)
    kw = dict(device=torch.device("cpu"), batch_size=2, ho=False)
    marks = lambda model, attr: _marks(model.student, attr)
    _lib.install_test_backend(Train2hDouble(cref.load(_lib.SIGNATURES), compute=False))
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            model = KD.NetModel(KD.default_args(**kw))
            assert model.student_piece_format == "bf16" and marks(model, "_skd_train_piece_format") == [None] * 10
            model = KD.NetModel(KD.default_args(split_train=True, student_pieces=2, **kw))
            assert marks(model, "_skd_train_piece_format") == [None] * 10 and marks(model, "_skd_train_pieces") == [2] * 10
            model = KD.NetModel(KD.default_args(split_train=True, student_pieces=2, student_piece_format="fp16", **kw))
            assert model.student_piece_format == "fp16" and marks(model, "_skd_train_piece_format") == ["fp16"] * 10
            assert marks(model, "_skd_train_pieces") == [None] * 10
            assert [getattr(m, "_skd_train_piece_format", None) for m in model.teacher.modules() if isinstance(m, PC.ResNet)] == [None]
        with pytest.warns(RuntimeWarning, match="only together with split_train") as rec:
            model = KD.NetModel(KD.default_args(student_pieces=2, student_piece_format="fp16", **kw))
        assert len([w for w in rec if "student_piece" in str(w.message)]) == 1
        assert marks(model, "_skd_train_piece_format") == [None] * 10 and marks(model, "_skd_train_min_cin") == [None] * 10
        monkeypatch.setenv("SKD_STUDENT_PIECES", "2")
        monkeypatch.setenv("SKD_STUDENT_PIECE_FORMAT", "fp16")
        monkeypatch.setenv("SKD_SPLIT_TRAIN", "1")
        assert marks(KD.NetModel(KD.default_args(**kw)), "_skd_train_piece_format") == ["fp16"] * 10
    finally:
        _lib.install_test_backend(None)
    # on the plain-C double: one warning from the routing, three pieces
    _lib.install_test_backend(cref.load(_lib.SIGNATURES))
    try:
        with pytest.warns(RuntimeWarning, match="skd_train2h.h") as rec:
            model = KD.NetModel(KD.default_args(**kw))
        assert len([w for w in rec if "skd_train2h.h" in str(w.message)]) == 1
        assert marks(model, "_skd_train_piece_format") == [None] * 10 and marks(model, "_skd_train_pieces") == [None] * 10
    finally:
        _lib.install_test_backend(None)


def test_docs_name_the_mode():
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    readme = open(os.path.join(REPO, "README.md")).read()
    assert "7.18" in design
    for text in (design, readme):
        for word in ("skd_train2h.h", "student_piece_format", "65504", "loss curve"):
            assert word in text, word
