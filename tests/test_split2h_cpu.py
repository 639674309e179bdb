"""The frozen teacher on two FP16 pieces with a scaled residual (include/skd_split2h.h), the parts that need no GPU: the float64
model of the mode (tests/split2h_ref.py) and why the residual is scaled, the C ABI (the pinned names and argument lists, the host-side
refusals of the five entries), the fp16 ops beside the four recorded ones, the routing of a network marked by
``set_teacher_pieces(model, 2, piece_format="fp16")`` (a recording double of the 1x1 entries on top of the plain-C double; the 3x3
ops, which refuse host tensors, are recorded at the op) and the public switch."""
import ctypes
import json
import os
import sys
import warnings

import pytest
import torch
import torch.nn.functional as F

import split2h_ref as R
import structure_knowledge_distillation_amd.networks.pspnet_combine as PC
from oracle import cref
from structure_knowledge_distillation_amd import _lib, functional as SF
from structure_knowledge_distillation_amd import networks
from structure_knowledge_distillation_amd.networks.kd_model import NetModel, default_args

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, "golden") not in sys.path:
    sys.path.insert(0, os.path.join(HERE, "golden"))

NAMES = ["skd_conv3x3_split2h_pack_bytes", "skd_conv3x3_split2h_pack_weights", "skd_conv3x3_split2h_nhwc", "skd_conv1x1_abn2h_nhwc",
         "skd_conv1x1_abn2h_pro_nhwc"]
TWINS = dict(zip(NAMES, ["skd_conv3x3_split2_pack_bytes", "skd_conv3x3_split2_pack_weights", "skd_conv3x3_split2_nhwc",
                         "skd_conv1x1_abn2_nhwc", "skd_conv1x1_abn2_pro_nhwc"]))


# ---- 1. the model ----------------------------------------------------------------------------------------------------------------

def test_two_fp16_pieces_carry_twenty_two_bits():
    """a0 + 2^-11 a1 == v for every fp32 v of at most 22 significant bits with 2^-14 <= |v| <= 65504 (and 0): a0 is then a normal
    fp16 and the scaled residual, a multiple of 2^-24 at least, an fp16 value too."""
    g = torch.Generator().manual_seed(1)
    for bits in (1, 11, 12, 21, 22):
        mant = torch.randint(2 ** (bits - 1), 2 ** bits, (8192,), generator=g).double()      # exactly `bits` significant bits
        mant = mant * (torch.randint(0, 2, (8192,), generator=g).double() * 2 - 1)
        expo = torch.randint(-14, 16, (8192,), generator=g).double()                          # the leading bit's weight
        v = (mant * torch.exp2(expo - (bits - 1))).float()
        assert float(v.abs().min()) >= 2.0 ** -14 and float(v.abs().max()) < 65536.0
        v = torch.where(v.abs() > 65504.0, torch.full_like(v, 65504.0), v)
        p0, p1 = R.pieces(v)
        assert torch.equal(p0 + p1 / R.SCALE, v.double()), bits
        if bits <= 11:
            assert not bool(p1.any()), "one piece"
    p0, p1 = R.pieces(torch.tensor([0.0, 65504.0, -65504.0, 2.0 ** -14]))
    assert torch.equal(p0 + p1 / R.SCALE, torch.tensor([0.0, 65504.0, -65504.0, 2.0 ** -14], dtype=torch.float64))
    # 24 bits: not every value survives, and what is lost is below 2^-22 |v|
    v = torch.randint(2 ** 23 + 1, 2 ** 24, (8192,), generator=g).float() * 2.0 ** -20
    p0, p1 = R.pieces(v)
    lost = (p0 + p1 / R.SCALE - v.double()).abs()
    assert bool(lost.any()) and bool((lost <= v.double().abs() * 2.0 ** -22).all())
    # below fp16's normal range the pieces keep absolute resolutions 2^-24 and 2^-35: 2^-40 is lost whole, 2^-30 survives
    p0, p1 = R.pieces(torch.tensor([2.0 ** -40, 2.0 ** -30]))
    assert (p0 + p1 / R.SCALE).tolist() == [0.0, 2.0 ** -30]
    # overflow is loud: infinity and the opposite infinity
    p0, p1 = R.pieces(torch.tensor([70000.0, -1e30, 65519.0]))
    assert p0.tolist() == [float("inf"), float("-inf"), 65504.0] and p1.tolist()[:2] == [float("-inf"), float("inf")]


@pytest.fixture(scope="module")
def table():
    """Per input class of DESIGN.md 7.15's table (M = 64, K = 2304, N = 32): the errors of the model, of the model without the
    residual scaling and of an fp32 multiply-add chain, each max |. - exact| / max |exact|."""
    out = {}
    for name, (a, b) in R.input_classes(64, 2304, 32).items():
        exact = a.double() @ b.double().t()
        out[name] = (R.rel_err(R.mm_split2h(a, b), exact), R.rel_err(R.mm_split2h(a, b, scaled=False), exact),
                     R.rel_err(R.fp32_chain(a, b), exact), float(a.abs().max()))
        print("%-22s max|a| %9.3g  fp16x2 scaled %.2e  unscaled %.2e  fp32 chain %.2e" % ((name, out[name][3]) + out[name][:3]))
    return out


def test_model_error_is_below_the_fp32_chains_own(table):
    """Across six decades of activation scale the split error of the mode is below the rounding of an fp32 accumulation over the
    same K.  (The last class, every activation below fp16's normal range, is outside that claim: there the pieces have absolute,
    not relative, resolution -- the header's range paragraph -- and the scaling must still be what keeps it usable.)"""
    for name in ("relu N(0,1)", "x30", "x1e-3", "columns e^-12..e^5", "x1000, weights 1e-4"):
        scaled, _, chain, _ = table[name]
        assert scaled < chain, (name, scaled, chain)
    scaled, unscaled, _, amax = table["x1e-5"]
    assert amax < 2.0 ** -14 and scaled < unscaled / 10


def test_the_residual_scaling_is_what_buys_the_small_activations(table):
    scaled, unscaled, _, amax = table["x1e-3"]
    assert amax < 0.125, "every residual of this class is an fp16 subnormal unscaled"
    assert unscaled >= 10 * scaled, (unscaled, scaled)


def test_three_product_model_against_the_exact_product():
    g = torch.Generator().manual_seed(2)
    a11 = torch.randint(-2047, 2048, (37, 64), generator=g).float()                    # one piece
    b22 = (torch.randint(-2 ** 21, 2 ** 21, (128, 64), generator=g).float() * 2.0 ** -21 + 1.0)      # 1 + 2^-21 k: two pieces
    want = a11.double() @ b22.double().t()
    assert torch.equal(R.mm_split2h(a11, b22), want) and torch.equal(R.mm_split2h(b22, a11), want.t())
    a22 = torch.randint(-2 ** 21, 2 ** 21, (37, 64), generator=g).float() * 2.0 ** -21 + 1.0
    both, exact = R.mm_split2h(a22, b22), a22.double() @ b22.double().t()
    (_, a1), (_, b1) = R.pieces(a22), R.pieces(b22)
    assert torch.equal(exact - both, (a1 @ b1.t()) / R.SCALE ** 2) and bool((exact != both).any()), "exactly a1 b1 is missing"
    x = torch.randint(0, 8, (2, 16, 7, 6), generator=g).float()
    w = torch.randint(-2 ** 21, 2 ** 21, (128, 16, 3, 3), generator=g).float() * 2.0 ** -11
    assert torch.equal(R.conv2d_split2h(x, w, None, 2, 2), F.conv2d(x.double(), w.double(), None, 1, 2, 2))


# ---- 2. the C ABI ----------------------------------------------------------------------------------------------------------------

def test_header_table_and_library_agree():
    """What is particular to skd_split2h.h; header <-> table <-> library <-> build digest: tests/test_abi.py, for every header."""
    assert sorted(_lib.ABI["skd_split2h.h"]) == sorted(NAMES) and len(NAMES) == 5
    for name, twin in TWINS.items():      # entry for entry the argument lists of include/skd_split2.h
        assert _lib.signature(name) == _lib.signature(twin), name


def test_header_states_the_numerics():
    with open(_lib.header_path("skd_split2h.h")) as fh:
        text = fh.read()
    for phrase in ("a0 = fp16(a)", "(a - a0) * 2^11", "lo += a0 b1", "lo += a1 b0", "hi += a0 b0", "fma(lo, 2^-11, hi)", "a1 b1",
                   "DROPPED", "at most 11 significant bits", "at most 22", "65504", "2^24", "NaN", "skd_split2.h", "SUBNORMAL",
                   "REACHABLE"):
        assert phrase in text, phrase


def test_pack_bytes():
    lib = _lib.load()
    for cin, cout in ((16, 128), (48, 256), (256, 256), (2048, 512)):
        assert lib.skd_conv3x3_split2h_pack_bytes(cin, cout) == 4 * cout * cin * 9 == lib.skd_conv3x3_split2_pack_bytes(cin, cout)
    for cin, cout in ((24, 128), (32, 64), (0, 128), (32, 0), (-16, 128), (32, 192 + 32)):
        assert lib.skd_conv3x3_split2h_pack_bytes(cin, cout) == 0, (cin, cout)


def test_host_side_refusals():
    """Every refusal is decided on the host, in front of the launches: no device is touched (the pointers are never followed).  The
    cases are those of the twins (tests/test_split2_cpu.py)."""
    lib = _lib.load()
    X, W_, OUT, PK, V = 0x10000, 0x2000000, 0x4000000, 0x8000000, 0xA000000
    nbytes = 4 * 128 * 32 * 9
    ok = dict(cin=32, cout=128, w=W_, sn=288, sc=9, sy=3, sx=1, pack=PK, nbytes=nbytes)
    for bad in (dict(w=None), dict(pack=None), dict(nbytes=nbytes - 1), dict(nbytes=0), dict(nbytes=-1), dict(pack=PK + 4),
                dict(pack=PK + 8), dict(sn=-1), dict(sc=-1), dict(sy=-1), dict(sx=-1), dict(cin=24), dict(cout=64), dict(cin=0),
                dict(cout=-128)):
        v = dict(ok, **bad)
        assert lib.skd_conv3x3_split2h_pack_weights(v["cin"], v["cout"], v["w"], v["sn"], v["sc"], v["sy"], v["sx"], v["pack"],
                                                    v["nbytes"], None) == 0, bad
    ok = dict(B=1, H=4, W=5, cin=32, cout=128, d=2, x=X, pk=PK, out=OUT, mean=None, var=None, act=0, geo=0)
    for bad in (dict(x=None), dict(pk=None), dict(out=None), dict(x=X + 4), dict(x=X + 8), dict(pk=PK + 4), dict(B=0), dict(H=0),
                dict(W=-1), dict(cin=24), dict(cin=0), dict(cout=64), dict(cout=0), dict(d=0), dict(d=-1), dict(act=2), dict(act=4),
                dict(act=-1), dict(geo=4), dict(geo=-1), dict(mean=V), dict(var=V)):
        v = dict(ok, **bad)
        assert lib.skd_conv3x3_split2h_nhwc(v["B"], v["H"], v["W"], v["cin"], v["cout"], v["d"], v["x"], v["pk"], v["out"], None,
                                            v["mean"], v["var"], None, None, 0.0, v["act"], 0.01, v["geo"], None) == 0, bad
    ok = dict(M=70, K=64, N=256, x=X, w=W_, out=OUT, mean=V, var=V + 4096, pp=PK, act=3)
    for pro in (False, True):
        bads = [dict(x=None), dict(w=None), dict(out=None), dict(mean=None), dict(var=None), dict(x=X + 4), dict(w=W_ + 8), dict(M=0),
                dict(M=-5), dict(K=0), dict(K=24), dict(N=0), dict(N=64), dict(N=192), dict(act=2), dict(act=9), dict(act=-1)]
        if pro:
            bads += [dict(pp=None), dict(pp=PK + 4), dict(K=1024)]
        for bad in bads:
            v = dict(ok, **bad)
            head = (v["M"], v["K"], v["N"], v["x"], v["w"], None, v["out"], v["mean"], v["var"], None, None, 1e-5)
            if pro:
                assert lib.skd_conv1x1_abn2h_pro_nhwc(*head, v["pp"], v["act"], 0.01, None) == 0, bad
            else:
                assert lib.skd_conv1x1_abn2h_nhwc(*head, v["act"], 0.01, None) == 0, bad


# ---- 3. the ops ------------------------------------------------------------------------------------------------------------------

class Split2hDouble:
    """The plain-C double for every core entry + the 1x1 entries of skd_split2.h and skd_split2h.h, recorded by format and computed
    by the core's three-piece entries (the wiring is what these tests look at), + the pack entries, which copy the fp32 weight into
    the head of the pack."""

    def __init__(self):
        self._core = cref.load(_lib.SIGNATURES)
        self.log, self.packs = [], []

    def __getattr__(self, name):
        return getattr(self._core, name)

    def _gemm(self, what, pro, m, k, n, x, w, r, *rest):
        self.log.append((what, "1x1", k, n, pro, r is not None))
        return (self._core.skd_conv1x1_abn_pro_nhwc if pro else self._core.skd_conv1x1_abn_nhwc)(m, k, n, x, w, r, *rest)

    def skd_conv1x1_abn_nhwc(self, *a):
        return self._gemm("bf16x3", False, *a)

    def skd_conv1x1_abn_pro_nhwc(self, *a):
        return self._gemm("bf16x3", True, *a)

    def skd_conv1x1_abn2_nhwc(self, *a):
        return self._gemm("bf16x2", False, *a)

    def skd_conv1x1_abn2_pro_nhwc(self, *a):
        return self._gemm("bf16x2", True, *a)

    def skd_conv1x1_abn2h_nhwc(self, *a):
        return self._gemm("fp16x2", False, *a)

    def skd_conv1x1_abn2h_pro_nhwc(self, *a):
        return self._gemm("fp16x2", True, *a)

    def skd_conv3x3_narrow_supported(self, cin, cout, s, p, d, g):      # the one rule an op asks the back-end directly
        return int(s == 1 and g == 1 and p == d and cin % 16 == 0 and cout % 64 == 0)

    def skd_conv3x3_split_pack_bytes(self, cin, cout):
        return cout * cin * 54

    def skd_conv3x3_split2_pack_bytes(self, cin, cout):
        return cout * cin * 36

    skd_conv3x3_split2h_pack_bytes = skd_conv3x3_split2_pack_bytes

    def _pack(self, what, cin, cout, w, sn, sc, sy, sx, pack, nbytes, stream):
        ctypes.memmove(pack, w, cout * cin * 36)
        self.packs.append(what)
        return 1

    def skd_conv3x3_split_pack_weights(self, *a):
        return self._pack("bf16x3", *a)

    def skd_conv3x3_split2_pack_weights(self, *a):
        return self._pack("bf16x2", *a)

    def skd_conv3x3_split2h_pack_weights(self, *a):
        return self._pack("fp16x2", *a)

    def skd_conv3x3_split2_nhwc(self, *a):
        raise AssertionError("the 3x3 ops refuse host tensors: never reached under this double")

    skd_conv3x3_split2h_nhwc = skd_conv3x3_split2_nhwc


@pytest.fixture
def double():
    d = Split2hDouble()
    _lib.install_test_backend(d)
    yield d
    _lib.install_test_backend(None)


@pytest.fixture
def c_double():
    _lib.install_test_backend(cref.load(_lib.SIGNATURES))
    yield
    _lib.install_test_backend(None)


def _cl(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).contiguous(memory_format=torch.channels_last)


def test_the_fp16_ops(double):
    """The fp16 form is an op of its own beside each of the four ops (their bound arguments are recorded call by call in
    tests/golden/routing_census.json, so they take no new keyword): same arguments without the piece count."""
    import inspect
    for name in ("conv1x1_abn_eval", "conv3x3_pack_weights", "conv3x3_split_eval", "ppm_fold_bottleneck"):
        base, twin = inspect.signature(getattr(SF, name)), inspect.signature(getattr(SF, name + "_fp16"))
        assert list(base.parameters)[-1] == "pieces" and "piece_format" not in base.parameters
        assert list(twin.parameters) == list(base.parameters)[:-1], name
        assert all(twin.parameters[k].default == base.parameters[k].default for k in twin.parameters), name
    torch.manual_seed(1)
    conv = torch.nn.Conv2d(64, 128, 1, bias=False)
    bn = PC.BatchNorm2d(128).eval()
    x = _cl(1, 64, 5, 6)
    args = (x, conv.weight, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.eps)
    c3 = torch.nn.Conv2d(16, 128, 3, 1, 1)
    with torch.no_grad():
        three = SF.conv1x1_abn_eval(*args)
        assert torch.equal(SF.conv1x1_abn_eval(*args, pieces=2), three) and torch.equal(SF.conv1x1_abn_eval_fp16(*args), three)
        SF.conv1x1_abn_eval_fp16(*args, pro=SF.abn_pack_eval_params(PC.BatchNorm2d(64).eval()), residual=torch.zeros_like(three))
        assert double.log == [("bf16x3", "1x1", 64, 128, False, False), ("bf16x2", "1x1", 64, 128, False, False),
                              ("fp16x2", "1x1", 64, 128, False, False), ("fp16x2", "1x1", 64, 128, True, True)]
        # no piece count and no format to get wrong: the ops take neither
        for kw in (dict(pieces=2), dict(pieces=3), dict(piece_format="fp16")):
            with pytest.raises(TypeError):
                SF.conv1x1_abn_eval_fp16(*args, **kw)
            with pytest.raises(TypeError):
                SF.conv3x3_pack_weights_fp16(c3, **kw)
        with pytest.raises(TypeError):
            SF.conv1x1_abn_eval(*args, pieces=2, piece_format="fp16")
        assert len(double.log) == 4
        # the pack: a slot of its own beside the other two, forgotten with them
        p3, p2, ph = SF.conv3x3_pack_weights(c3), SF.conv3x3_pack_weights(c3, pieces=2), SF.conv3x3_pack_weights_fp16(c3)
        assert SF.conv3x3_pack_weights_fp16(c3) is ph and ph is not p2 and double.packs == ["bf16x3", "bf16x2", "fp16x2"]
        assert all(hasattr(c3, a) for a in ("_skd_conv3x3_pack", "_skd_conv3x3_pack2", "_skd_conv3x3_pack2h"))
        assert ph.numel() == 128 * 16 * 36 and p3.numel() == 128 * 16 * 54
    SF.drop_conv3x3_packs(c3)
    assert not any(hasattr(c3, a) for a in ("_skd_conv3x3_pack", "_skd_conv3x3_pack2", "_skd_conv3x3_pack2h"))
    cache = {"pack3x3": 1, "pack3x3_2": 2, "pack3x3_2h": 3, "mats": 4}
    SF.drop_conv3x3_packs(cache)
    assert cache == {"mats": 4}


def test_fp16_is_never_downgraded(c_double):
    """A back-end without the entries: the ops raise what the other ops raise for a missing entry."""
    conv = torch.nn.Conv2d(64, 128, 1, bias=False)
    bn = PC.BatchNorm2d(128).eval()
    x = _cl(1, 64, 5, 6)
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="skd_conv1x1_abn2h_nhwc"):
            SF.conv1x1_abn_eval_fp16(x, conv.weight, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.eps)
        with pytest.raises(NotImplementedError, match="skd_conv1x1_abn2h_pro_nhwc"):
            SF.conv1x1_abn_eval_fp16(x, conv.weight, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.eps, pro=torch.zeros(4, 64))
        with pytest.raises(NotImplementedError, match="skd_conv3x3_split2h_pack_weights"):
            SF.conv3x3_pack_weights_fp16(torch.nn.Conv2d(16, 128, 3, 1, 1))
        with pytest.raises(NotImplementedError, match="skd_conv3x3_split2h_nhwc"):
            SF.conv3x3_split_eval_fp16(_cl(1, 16, 4, 4), torch.zeros(16 * 128 * 36, dtype=torch.uint8), 128)


# ---- 4. routing ------------------------------------------------------------------------------------------------------------------

def _what(pieces, piece_format):
    return "%sx%d" % (piece_format, pieces)


@pytest.fixture
def recording(double, monkeypatch):
    """``double`` + the 3x3 ops recorded at the op (the frozen 3x3 forms refuse host tensors): the pack ops return the weight with
    the form they were asked for, the convolution ops check it, log and compute ``F.conv2d`` + the module's own ABN."""
    def ok(x, w, s, p, d, g, grad, entries, query, host_ok):
        rule = dict(skd_conv3x3_split_supported=(1, 128), skd_conv3x3_narrow_supported=(1, 64), skd_conv3x3_split_s2_supported=(2, 128))[query]
        return (grad is False and not torch.is_grad_enabled() and SF._fp32_cl_map(x) and s == rule[0] and g == 1
                and (p == d if s == 1 else p == d == 1) and w.shape[1] % 16 == 0 and w.shape[0] % rule[1] == 0)

    def pack(conv, weight=None, owner=None, pieces=3, piece_format="bf16"):
        return (_what(pieces, piece_format), conv.weight if weight is None else weight)

    def pack_fp16(conv, weight=None, owner=None):
        return pack(conv, weight, owner, 2, "fp16")

    def run_fp16(x, pk, cout, dilation=1, conv_bias=None, bn=None, activation="none", geometry=0):
        return run(x, pk, cout, dilation, conv_bias, bn, activation, geometry, 2, "fp16")

    def run(x, pk, cout, dilation=1, conv_bias=None, bn=None, activation="none", geometry=0, pieces=3, piece_format="bf16"):
        assert pk[0] == _what(pieces, piece_format), "the pack of another form"
        double.log.append((pk[0], "3x3", x.shape[1], cout, dilation))
        y = F.conv2d(x, pk[1], conv_bias, 1, dilation, dilation).contiguous(memory_format=torch.channels_last)
        return y if bn is None else bn(y)

    def run_s2(x, pk, cout, conv_bias=None, bn=None, activation="none", pieces=3):
        assert pk[0] == _what(pieces, "bf16"), "the stride-2 form has bf16 packs only"
        double.log.append((pk[0], "s2", x.shape[1], cout, 1))
        y = F.conv2d(x, pk[1], conv_bias, 2, 1, 1).contiguous(memory_format=torch.channels_last)
        return y if bn is None else bn(y)

    def narrow_pack(conv, *a, **kw):
        return ("narrow", conv.weight)

    def run_narrow(x, pk, cout, dilation, residual, conv_bias, bn, activation, *a, **kw):
        assert pk[0] == "narrow"
        double.log.append(("bf16x3", "narrow", x.shape[1], cout, dilation))
        y = F.conv2d(x, pk[1], conv_bias, 1, dilation, dilation).contiguous(memory_format=torch.channels_last)
        return y if bn is None else torch.relu(bn(y)) if activation == "relu" else bn(y)
    has_entry = _lib.has_entry
    monkeypatch.setattr(_lib, "has_entry", lambda name: name in PC._TEACHER_EARLY_ENTRIES or has_entry(name))
    monkeypatch.setattr(SF, "_conv3x3_ok", ok)
    monkeypatch.setattr(SF, "conv3x3_pack_weights", pack)
    monkeypatch.setattr(SF, "conv3x3_split_eval", run)
    monkeypatch.setattr(SF, "conv3x3_pack_weights_fp16", pack_fp16)
    monkeypatch.setattr(SF, "conv3x3_split_eval_fp16", run_fp16)
    monkeypatch.setattr(SF, "conv3x3_s2_eval", run_s2)
    monkeypatch.setattr(SF, "conv3x3_narrow_pack_weights", narrow_pack)
    monkeypatch.setattr(SF, "conv3x3_narrow_eval", run_narrow)
    return double


def _stack():
    """Two Bottlenecks of layer3's shapes: 512 -> (256, 3x3 d 2) -> 1024 with a stride-1 down-sample, then 1024 -> 256 -> 1024."""
    torch.manual_seed(3)
    down = torch.nn.Sequential(torch.nn.Conv2d(512, 1024, 1, 1, bias=False), PC.BatchNorm2d(1024))
    net = torch.nn.Sequential(PC.Bottleneck(512, 256, 1, dilation=2, downsample=down), PC.Bottleneck(1024, 256, dilation=2))
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, PC.InPlaceABNSync):
                m.running_var.uniform_(0.5, 1.5)
                m.running_mean.normal_(0, 0.1)
    return net.eval().to(memory_format=torch.channels_last)


STACK_CALLS = [("1x1", 512, 256, False, False), ("3x3", 256, 256, 2), ("1x1", 512, 1024, False, False), ("1x1", 256, 1024, True, True),
               ("1x1", 1024, 256, False, False), ("3x3", 256, 256, 2), ("1x1", 256, 1024, True, True)]


def _marks(net):
    return sorted({(getattr(m, "_skd_teacher_pieces", 3), getattr(m, "_skd_teacher_piece_format", "bf16")) for m in net.modules()
                   if isinstance(m, (PC.Bottleneck, PC.ResNet, PC.PSPModule))})


def test_marked_stack_hands_exactly_its_split_core_calls_over(recording):
    net, x = _stack(), _cl(1, 512, 6, 7, seed=4)
    with torch.no_grad():
        want = net(x)
    assert recording.log == [("bf16x3",) + c for c in STACK_CALLS]
    recording.log.clear()
    assert networks.set_teacher_pieces(net, 2, piece_format="fp16") is net and _marks(net) == [(2, "fp16")]
    with torch.no_grad():
        got = net(x)
    assert recording.log == [("fp16x2",) + c for c in STACK_CALLS], "the same call sites read the mark"
    assert torch.equal(got, want), "the double computes every form alike: the wiring is the same"
    # the same modules the bf16 switch marks, and switching between the two leaves one mark
    recording.log.clear()
    networks.set_teacher_pieces(net, 2)
    assert _marks(net) == [(2, "bf16")]
    with torch.no_grad():
        net(x)
    assert recording.log == [("bf16x2",) + c for c in STACK_CALLS]
    networks.set_teacher_pieces(net, 2, piece_format="fp16")
    net[0].conv2._skd_conv3x3_pack2h = "a pack"
    recording.log.clear()
    networks.set_teacher_pieces(net, 3)
    assert _marks(net) == [(3, "bf16")] and not hasattr(net[0].conv2, "_skd_conv3x3_pack2h")
    with torch.no_grad():
        net(x)
    assert recording.log == [("bf16x3",) + c for c in STACK_CALLS]
    # none in training mode or under grad
    networks.set_teacher_pieces(net, 2, piece_format="fp16")
    recording.log.clear()
    net.train()
    with torch.no_grad():
        net(x)
    net.eval()
    net(x)
    assert not any(c[0] == "fp16x2" for c in recording.log)


def test_the_format_without_two_pieces_is_an_error(double, monkeypatch):
    net = _stack()
    for args in ((3, "fp16"), (2, "f16"), (2, None), (3, "half")):
        with pytest.raises(ValueError):
            networks.set_teacher_pieces(net, *args)
    assert _marks(net) == [(3, "bf16")]
    monkeypatch.delenv("SKD_TEACHER_PIECES", raising=False)
    monkeypatch.delenv("SKD_TEACHER_PIECE_FORMAT", raising=False)
    a = default_args()
    assert (a.teacher_pieces, a.teacher_piece_format) == (3, "bf16")
    a = default_args(teacher_pieces=2, teacher_piece_format="fp16")
    assert (a.teacher_pieces, a.teacher_piece_format) == (2, "fp16")
    assert default_args(teacher_pieces=2).teacher_piece_format == "bf16"
    for kw in (dict(teacher_piece_format="fp16"), dict(teacher_pieces=3, teacher_piece_format="fp16"),
               dict(teacher_pieces=2, teacher_piece_format="fp8")):
        with pytest.raises(ValueError):
            default_args(**kw)
    monkeypatch.setenv("SKD_TEACHER_PIECE_FORMAT", "fp16")
    with pytest.raises(ValueError, match="requires"):
        default_args()
    monkeypatch.setenv("SKD_TEACHER_PIECES", "2")
    a = default_args()
    assert (a.teacher_pieces, a.teacher_piece_format) == (2, "fp16")
    assert default_args(teacher_piece_format="bf16").teacher_piece_format == "bf16"
    monkeypatch.setenv("SKD_TEACHER_PIECE_FORMAT", "FP16")
    with pytest.raises(ValueError):
        default_args()


def test_netmodel_marks_the_teacher_alone(double, monkeypatch):
    for name in ("SKD_TEACHER_PIECES", "SKD_TEACHER_PIECE_FORMAT", "SKD_SPLIT_TRAIN", "SKD_TEACHER_EARLY"):
        monkeypatch.delenv(name, raising=False)
    kw = dict(device=torch.device("cpu"), batch_size=2, ho=False)
    model = NetModel(default_args(**kw))
    assert _marks(model.teacher) == [(3, "bf16")] and model.teacher_piece_format == "bf16"
    model = NetModel(default_args(teacher_pieces=2, teacher_piece_format="fp16", **kw))
    assert _marks(model.teacher) == [(2, "fp16")] and _marks(model.student) == [(3, "bf16")]
    assert (model.teacher_pieces, model.teacher_piece_format) == (2, "fp16")
    monkeypatch.setenv("SKD_TEACHER_PIECES", "2")
    monkeypatch.setenv("SKD_TEACHER_PIECE_FORMAT", "fp16")
    model = NetModel(default_args(**kw))
    assert _marks(model.teacher) == [(2, "fp16")] and _marks(model.student) == [(3, "bf16")]
    # on a back-end without the entries: the warning, and three pieces
    _lib.install_test_backend(cref.load(_lib.SIGNATURES))
    with pytest.warns(RuntimeWarning, match="three pieces"):
        model = NetModel(default_args(**kw))
    assert _marks(model.teacher) == [(3, "bf16")]


def test_backend_without_the_entries_warns_and_keeps_three_pieces(c_double):
    net = _stack()
    with pytest.warns(RuntimeWarning, match="skd_split2h.h.*three pieces"):
        assert networks.set_teacher_pieces(net, 2, piece_format="fp16") is net
    assert _marks(net) == [(3, "bf16")]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        networks.set_teacher_pieces(net, 3)


def test_excluded_shapes_keep_three_pieces_never_two(recording, monkeypatch):
    assert isinstance(PC.SPLIT2H_ROUTING_EXCLUDED, frozenset)
    assert all(e[0] in ("1x1", "3x3") and len(e) == (3 if e[0] == "1x1" else 4) for e in PC.SPLIT2H_ROUTING_EXCLUDED)
    net, x = networks.set_teacher_pieces(_stack(), 2, piece_format="fp16"), _cl(1, 512, 6, 7, seed=4)
    monkeypatch.setattr(PC, "SPLIT2H_ROUTING_EXCLUDED", frozenset({("1x1", 512, 1024), ("3x3", 256, 256, 2), ("1x1", 256, 1024)}))
    monkeypatch.setattr(PC, "SPLIT2_ROUTING_EXCLUDED", frozenset({("1x1", 512, 256)}))      # the other switch's set is not read
    with torch.no_grad():
        net(x)
    fp16 = [("1x1", 512, 256, False, False), ("1x1", 1024, 256, False, False)]
    assert recording.log == [("fp16x2" if c in fp16 else "bf16x3",) + c for c in STACK_CALLS]


def test_teacher_early_forms_without_an_fp16_twin_stay_on_three_pieces(recording):
    """Under route_teacher_early the 64-column and the stride-2 convolutions have no fp16 form: marked for fp16 pieces they run on
    THREE bf16 pieces (under the bf16 switch the stride-2 one takes two) -- never on two bf16 pieces nobody asked for.  The wide
    stride-1 ones (layer2's conv2 behind the first block) take the fp16 entries."""
    torch.manual_seed(11)
    down = torch.nn.Sequential(torch.nn.Conv2d(256, 512, 1, 2, bias=False), PC.BatchNorm2d(512))
    layer2 = torch.nn.Sequential(PC.Bottleneck(256, 128, 2, downsample=down), PC.Bottleneck(512, 128))
    layer1 = torch.nn.Sequential(PC.Bottleneck(256, 64))
    net = torch.nn.Sequential(layer1, layer2).eval().to(memory_format=torch.channels_last)
    x = _cl(1, 256, 9, 9, seed=12)
    threes = {}
    for fmt in ("bf16", "fp16"):
        networks.set_teacher_pieces(net, 2, piece_format=fmt)
        PC.route_teacher_early(net)
        recording.log.clear()
        with torch.no_grad():
            net(x)
        threes[fmt] = [c for c in recording.log if c[1] in ("3x3", "s2", "narrow")]
        PC.route_teacher_early(net, enable=False)
    assert threes["bf16"] == [("bf16x3", "narrow", 64, 64, 1), ("bf16x2", "s2", 128, 128, 1), ("bf16x2", "3x3", 128, 128, 1)]
    assert threes["fp16"] == [("bf16x3", "narrow", 64, 64, 1), ("bf16x3", "s2", 128, 128, 1), ("fp16x2", "3x3", 128, 128, 1)]
    assert not any(c[0] == "bf16x2" for c in recording.log), "two bf16 pieces were never asked for"


def test_teacher_marks_dsn_and_psp_and_a_student_is_untouched(recording):
    torch.manual_seed(7)
    teacher = PC.Res_pspnet(PC.Bottleneck, [3, 4, 23, 3], 19).eval().to(memory_format=torch.channels_last)
    networks.set_teacher_pieces(teacher, 2, piece_format="fp16")
    marked = [m for m in teacher.modules() if getattr(m, "_skd_teacher_piece_format", None) == "fp16"]
    assert len(marked) == 33 + 2 and {type(m).__name__ for m in marked} == {"Bottleneck", "PSPModule", "ResNet"}
    with torch.no_grad():
        teacher._dsn_head(_cl(1, 1024, 5, 5, seed=8))
        teacher.pspmodule(_cl(1, 2048, 6, 6, seed=9))
    assert [c for c in recording.log if c[1] == "3x3"] == [("fp16x2", "3x3", 1024, 512, 1), ("fp16x2", "3x3", 2048, 512, 1)]
    assert "pack3x3_2h" in teacher.pspmodule._fold_cache and "pack3x3_2" not in teacher.pspmodule._fold_cache
    networks.set_teacher_pieces(teacher, 3)
    assert "pack3x3_2h" not in teacher.pspmodule._fold_cache
    student = PC.Res_pspnet(PC.BasicBlock, [2, 2, 2, 2], 19).eval().to(memory_format=torch.channels_last)
    networks.set_teacher_pieces(student, 2, piece_format="fp16")
    assert _marks(student) == [(3, "bf16")]


def test_the_switch_off_changes_no_routing_decision():
    """The form decisions of the tree are the recorded ones (tests/golden/routing_decisions.json, as tests/test_routing_decisions_cpu.py
    compares them), and a module marked for fp16 pieces is given the form an unmarked one is given: the mark is read behind the
    form decision, never by it."""
    import make_golden_routing_decisions as G
    want = json.load(open(G.OUT))
    got = G.sections()
    for section in ("block", "bottle", "dsn", "stem", "train"):
        assert got[section] == want[section], section
    with G.patched():
        plain, marked = PC.Bottleneck(64, 64).eval(), PC.Bottleneck(64, 64).eval()
        marked._skd_teacher_pieces, marked._skd_teacher_piece_format = 2, "fp16"
        for early in (False, True):
            plain._skd_teacher_early = marked._skd_teacher_early = early
            with torch.no_grad():
                for conv, x in G.convs():
                    assert PC._frozen_form(plain, x, conv) == PC._frozen_form(marked, x, conv)
    assert PC._piece_route(plain, "3x3", 256, 256, 2) == (3, "bf16") and PC._piece_route(None, "1x1", 512, 256) == (3, "bf16")
    assert PC._piece_route(marked, "3x3", 256, 256, 2) == (2, "fp16") and PC._piece_route(marked, "3x3", 128, 128, 1, fp16_form=False) == (3, "bf16")


def test_docs_name_the_mode():
    for fn in (SF.conv1x1_abn_eval, SF.conv3x3_split_eval, SF.conv3x3_pack_weights, SF.ppm_fold_bottleneck, SF.conv1x1_abn_eval_fp16,
               SF.conv3x3_split_eval_fp16, SF.conv3x3_pack_weights_fp16):
        assert "skd_split2h.h" in fn.__doc__ or "_fp16" in fn.__doc__, fn.__name__
    assert "SPLIT2H_ROUTING_EXCLUDED" in PC.set_teacher_pieces.__doc__ and "piece_format" in PC.set_teacher_pieces.__doc__
