"""The student's fused inference form on two FP16 pieces (include/skd_infer2h.h), the parts that need no GPU: the C ABI (the pinned
names and argument lists against the three-piece twins, the header's numerics paragraph, the pack sizes, the host-side refusals of
the five entries), the fp16 twin ops, ``fuse_for_inference(piece_format=...)``, the routing of a flagged student (the 3x3 ops, which
refuse host tensors, recorded at the op on top of tests/test_split2h_cpu.py's double) and the ``infer_piece_format`` switch."""
import ctypes
import inspect
import warnings

import pytest
import torch
import torch.nn.functional as F

import test_split2h_cpu as C
import structure_knowledge_distillation_amd.networks.pspnet_combine as PC
from oracle import cref
from structure_knowledge_distillation_amd import _lib, functional as SF
from structure_knowledge_distillation_amd import networks
from structure_knowledge_distillation_amd.networks.kd_model import NetModel, default_args

NAMES = ["skd_conv3x3_split2h_res_nhwc", "skd_conv3x3_narrow2h_pack_bytes", "skd_conv3x3_narrow2h_pack_weights",
         "skd_conv3x3_narrow2h_nhwc", "skd_conv3x3_split2h_s2_nhwc"]
RES, NBYTES, NPACK, NARROW, S2 = NAMES


# ---- 1. the C ABI ----------------------------------------------------------------------------------------------------------------

def test_header_table_and_twins_agree():
    """What is particular to skd_infer2h.h; header <-> table <-> library <-> build digest: tests/test_abi.py, for every header."""
    assert sorted(_lib.ABI["skd_infer2h.h"]) == sorted(NAMES) and len(NAMES) == 5
    sig = _lib.signature
    assert sig(RES) == sig("skd_conv3x3_split_res_nhwc")
    assert sig(NBYTES) == sig("skd_conv3x3_narrow_pack_bytes")
    assert sig(NPACK) == sig("skd_conv3x3_split2h_pack_weights"), "the forward image alone"
    assert sig(NARROW) == sig("skd_conv3x3_narrow_nhwc")
    twin = sig("skd_conv3x3_split_s2_nhwc")
    assert sig(S2) == (twin[0], twin[1][:16] + twin[1][17:]) and twin[1][16] is ctypes.c_int, "the twin without `pieces`"
    core = cref.load(_lib.SIGNATURES)
    assert not any(hasattr(core, n) for n in NAMES), "the plain-C double lacks the entries, like every extension"


def test_header_states_the_numerics_by_reference():
    with open(_lib.header_path("skd_infer2h.h")) as fh:
        text = " ".join(fh.read().replace("\n *", " ").split())      # the comment's line breaks are not part of a phrase
    for phrase in ("skd_split2h.h", "tests/split2h_ref.py", "a0 = fp16(a)", "(a - a0) * 2^11", "fma(lo, 2^-11, hi)", "EXACT", "at most 11",
                   "at most 22", "65504", "LOUD", "subnormal", "used as it is", "never split", "skd_conv3x3_split_res_nhwc",
                   "skd_conv3x3_narrow_nhwc", "skd_conv3x3_split_s2_nhwc", "bit for bit"):
        assert phrase in text, phrase


def test_pack_bytes():
    lib = _lib.load()
    for cin, cout in ((16, 64), (48, 192), (64, 64), (128, 64), (32, 128)):
        assert lib.skd_conv3x3_narrow2h_pack_bytes(cin, cout) == 4 * cout * cin * 9
        assert lib.skd_conv3x3_narrow_pack_bytes(cin, cout) == 6 * cout * cin * 9
    for cin, cout in ((24, 64), (32, 32), (0, 64), (32, 0), (-16, 64), (32, 96)):
        assert lib.skd_conv3x3_narrow2h_pack_bytes(cin, cout) == 0, (cin, cout)


def test_host_side_refusals():
    """Every refusal is decided on the host, in front of the launches: no device is touched (the pointers are never followed).  The
    cases are those of the twins (tests/test_student_infer_cpu.py, test_conv3x3_narrow_cpu.py, test_conv3x3_stride2_cpu.py)."""
    lib = _lib.load()
    X, W_, OUT, PK, V, R_ = 0x10000, 0x2000000, 0x4000000, 0x8000000, 0xA000000, 0xC000000
    nb = 4 * 64 * 32 * 9
    ok = dict(cin=32, cout=64, w=W_, sn=288, sc=9, sy=3, sx=1, pack=PK, nbytes=nb)
    for bad in (dict(w=None), dict(pack=None), dict(nbytes=nb - 1), dict(nbytes=0), dict(nbytes=-1), dict(pack=PK + 4), dict(pack=PK + 8),
                dict(sn=-1), dict(sc=-1), dict(sy=-1), dict(sx=-1), dict(cin=24), dict(cout=32), dict(cin=0), dict(cout=-64)):
        v = dict(ok, **bad)
        assert lib.skd_conv3x3_narrow2h_pack_weights(v["cin"], v["cout"], v["w"], v["sn"], v["sc"], v["sy"], v["sx"], v["pack"],
                                                     v["nbytes"], None) == 0, bad
    out_bytes = 1 * 4 * 5 * 128 * 4
    common = (dict(x=None), dict(pk=None), dict(out=None), dict(x=X + 4), dict(x=X + 8), dict(pk=PK + 4), dict(B=0), dict(H=0),
              dict(W=-1), dict(cin=24), dict(cin=0), dict(cout=0), dict(d=0), dict(d=-1), dict(act=2), dict(act=4), dict(act=-1),
              dict(geo=-1), dict(mean=V), dict(var=V),
              # a residual that overlaps the output: the same buffer, one float into it from either side, its last float
              dict(res=OUT), dict(res=OUT + 4), dict(res=OUT - 4), dict(res=OUT + out_bytes - 4), dict(res=OUT - out_bytes + 4),
              # the residual-free form refuses the same things
              dict(res=None, x=None), dict(res=None, mean=V), dict(res=None, geo=-1))
    for name, extra in ((RES, (dict(cout=64), dict(geo=4), dict(res=None, cout=64), dict(res=None, geo=4))),
                        (NARROW, (dict(cout=32), dict(cout=96), dict(geo=2), dict(geo=3), dict(res=None, geo=2)))):
        ok = dict(B=1, H=4, W=5, cin=32, cout=128, d=2, x=X, pk=PK, out=OUT, res=R_, mean=None, var=None, act=0, geo=0)
        for bad in common + extra:
            v = dict(ok, **bad)
            assert getattr(lib, name)(v["B"], v["H"], v["W"], v["cin"], v["cout"], v["d"], v["x"], v["pk"], v["out"], v["res"], None,
                                      v["mean"], v["var"], None, None, 0.0, v["act"], 0.01, v["geo"], None) == 0, (name, bad)
    ok = dict(B=1, H=4, W=5, cin=32, cout=128, x=X, pk=PK, out=OUT, mean=None, var=None, act=3, geo=0)
    for bad in (dict(x=None), dict(pk=None), dict(out=None), dict(x=X + 4), dict(pk=PK + 8), dict(B=0), dict(H=0), dict(W=-1), dict(cin=24),
                dict(cin=0), dict(cout=64), dict(cout=0), dict(act=1), dict(act=2), dict(act=-1), dict(geo=4), dict(geo=-1), dict(mean=V),
                dict(var=V)):
        v = dict(ok, **bad)
        assert lib.skd_conv3x3_split2h_s2_nhwc(v["B"], v["H"], v["W"], v["cin"], v["cout"], v["x"], v["pk"], v["out"], None, v["mean"],
                                               v["var"], None, None, 0.0, v["act"], 0.01, v["geo"], None) == 0, bad


# ---- 2. the ops ------------------------------------------------------------------------------------------------------------------

double = C.double
c_double = C.c_double
_cl = C._cl


def test_the_fp16_twin_ops_take_their_twins_arguments():
    """Ops of their own, not a keyword on the recorded ones (tests/golden/routing_census.json records every public conv3x3_* call
    with its defaults): the same parameters, the same defaults, no piece count and no format."""
    for name, drop in (("conv3x3_split_res_eval", ()), ("conv3x3_narrow_pack_weights", ()), ("conv3x3_narrow_eval", ()),
                       ("conv3x3_s2_eval", ("pieces",))):
        base, twin = inspect.signature(getattr(SF, name)), inspect.signature(getattr(SF, name + "_fp16"))
        assert "piece_format" not in base.parameters and "piece_format" not in twin.parameters and "pieces" not in twin.parameters
        assert list(twin.parameters) == [p for p in base.parameters if p not in drop], name
        assert all(twin.parameters[k].default == base.parameters[k].default for k in twin.parameters), name
        assert "skd_infer2h.h" in getattr(SF, name + "_fp16").__doc__


def test_fp16_is_never_downgraded(c_double):
    """A back-end without the entries: the ops raise NotImplementedError naming the header."""
    x, pack = _cl(1, 16, 4, 4), torch.zeros(16 * 128 * 36, dtype=torch.uint8)
    assert not SF.infer2h_supported()
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="skd_conv3x3_split2h_res_nhwc.*skd_infer2h.h"):
            SF.conv3x3_split_res_eval_fp16(x, pack, 128, 1, None, None, "relu")
        with pytest.raises(NotImplementedError, match="skd_conv3x3_narrow2h_pack_weights.*skd_infer2h.h"):
            SF.conv3x3_narrow_pack_weights_fp16(torch.nn.Conv2d(16, 64, 3, 1, 1))
        with pytest.raises(NotImplementedError, match="skd_conv3x3_narrow2h_nhwc.*skd_infer2h.h"):
            SF.conv3x3_narrow_eval_fp16(x, pack, 64, 1)
        with pytest.raises(NotImplementedError, match="skd_conv3x3_split2h_s2_nhwc.*skd_infer2h.h"):
            SF.conv3x3_s2_eval_fp16(x, pack, 128)


class PackDouble(C.Split2hDouble):
    """+ the narrow pack entries of both forms, recorded like the wide ones."""

    def skd_conv3x3_narrow_pack_bytes(self, cin, cout):
        return cout * cin * 54

    def skd_conv3x3_narrow2h_pack_bytes(self, cin, cout):
        return cout * cin * 36

    def skd_conv3x3_narrow_pack_pair(self, cin, cout, w, sn, sc, sy, sx, pack, nbytes, pack_bwd, bwd_bytes, stream):
        return self._pack("narrow bf16x3", cin, cout, w, sn, sc, sy, sx, pack, nbytes, stream)

    def skd_conv3x3_narrow2h_pack_weights(self, *a):
        return self._pack("narrow fp16x2", *a)


def test_the_narrow_fp16_pack_has_a_slot_of_its_own():
    d = PackDouble()
    _lib.install_test_backend(d)
    try:
        conv = torch.nn.Conv2d(16, 64, 3, 1, 1, bias=False)
        with torch.no_grad():
            p3, ph = SF.conv3x3_narrow_pack_weights(conv), SF.conv3x3_narrow_pack_weights_fp16(conv)
            assert SF.conv3x3_narrow_pack_weights_fp16(conv) is ph and SF.conv3x3_narrow_pack_weights(conv) is p3
            assert d.packs == ["narrow bf16x3", "narrow fp16x2"] and ph.numel() == 64 * 16 * 36 and p3.numel() == 64 * 16 * 54
            assert hasattr(conv, "_skd_conv3x3_narrow_pack") and hasattr(conv, "_skd_conv3x3_narrow_pack2h")
            conv.weight.add_(1.0)                                  # a written weight: the version key rebuilds each on its next use
            assert SF.conv3x3_narrow_pack_weights_fp16(conv) is not ph and d.packs[-1] == "narrow fp16x2"
        SF.drop_conv3x3_packs(conv)
        assert not hasattr(conv, "_skd_conv3x3_narrow_pack") and not hasattr(conv, "_skd_conv3x3_narrow_pack2h")
        with pytest.raises(RuntimeError, match="frozen"):
            SF.conv3x3_narrow_pack_weights_fp16(conv)              # grad enabled on a trainable weight
    finally:
        _lib.install_test_backend(None)


# ---- 3. the switch of fuse_for_inference -----------------------------------------------------------------------------------------

def _student():
    torch.manual_seed(5)
    return PC.Res_pspnet(PC.BasicBlock, [2, 2, 2, 2], 19).eval().to(memory_format=torch.channels_last)


def _marks(net):
    return [type(m).__name__ for m in net.modules() if getattr(m, "_skd_infer_piece_format", None) is not None]


def test_piece_format_validation(c_double, monkeypatch):
    net = _student()
    assert inspect.signature(PC.fuse_for_inference).parameters["piece_format"].default == "bf16"
    for junk in ("f16", "fp8", None, 2, "FP16", "bf16x3"):
        with pytest.raises(ValueError, match="piece_format"):
            networks.fuse_for_inference(net, piece_format=junk)
    assert _marks(net) == [] and not any(hasattr(m, "_skd_infer_min_cin") for m in net.modules()), "a refused call flags nothing"
    # a back-end without the entries: one warning, the student flagged on three pieces
    with pytest.warns(RuntimeWarning, match="skd_infer2h.h.*three pieces") as caught:
        assert networks.fuse_for_inference(net, narrow=True, piece_format="fp16") is net
    assert len(caught) == 1 and _marks(net) == [] and net.layer3[0]._skd_infer_min_cin == PC.FUSED_EVAL_MIN_CIN
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        networks.fuse_for_inference(net, piece_format="bf16")
        networks.fuse_for_inference(net, enable=False, piece_format="fp16")      # clearing needs no entry
    # with the entries: the mark sits on the eight BasicBlocks and on the ResNet (its stem), and is not the teacher's
    monkeypatch.setattr(SF, "infer2h_supported", lambda: True)
    monkeypatch.setattr(PC, "_prepack", lambda module, convs: None)
    networks.fuse_for_inference(net, piece_format="fp16")
    assert sorted(_marks(net)) == ["BasicBlock"] * 8 + ["ResNet"]
    assert not any(hasattr(m, "_skd_teacher_pieces") or hasattr(m, "_skd_teacher_piece_format") for m in net.modules())
    networks.fuse_for_inference(net)                                # the default again: the mark goes, the flags stay
    assert _marks(net) == [] and net.layer3[0]._skd_infer_min_cin == PC.FUSED_EVAL_MIN_CIN
    networks.fuse_for_inference(net, piece_format="fp16")
    networks.fuse_for_inference(net, enable=False)
    assert _marks(net) == [] and net.layer3[0]._skd_infer_min_cin is None
    assert "INFER2H_ROUTING_EXCLUDED" in PC.fuse_for_inference.__doc__ and "skd_infer2h.h" in PC.fuse_for_inference.__doc__


# ---- 4. routing ------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def rec(double, monkeypatch):
    """``double`` + every 3x3 op of the frozen forms recorded at the op as (pieces, form, Cin, Cout, dilation): the pack ops return
    the weight tagged with the image they were asked for, the convolution ops check the tag, log and compute ``F.conv2d`` + the
    module's own ABN (+ residual, + ReLU).  The back-end is taken to have every entry."""
    def ok(x, w, s, p, d, g, grad, entries, query, host_ok):
        rule = dict(skd_conv3x3_split_supported=(1, 128), skd_conv3x3_narrow_supported=(1, 64), skd_conv3x3_split_s2_supported=(2, 128))[query]
        return (grad is False and not torch.is_grad_enabled() and SF._fp32_cl_map(x) and s == rule[0] and g == 1
                and (p == d if s == 1 else p == d == 1) and w.shape[1] % 16 == 0 and w.shape[0] % rule[1] == 0)

    def conv(tag, form, x, pk, want, stride, dilation, conv_bias, bn, activation, residual=None):
        assert pk[0] == want, "%s: the pack %r of another form (wanted %r)" % (form, pk[0], want)
        double.log.append((tag, form + ("+res" if residual is not None else ""), x.shape[1], pk[1].shape[0], dilation))
        y = F.conv2d(x, pk[1], conv_bias, stride, dilation, dilation).contiguous(memory_format=torch.channels_last)
        y = y if bn is None else bn(y)
        y = y if residual is None else y + residual
        return torch.relu(y) if activation == "relu" else y

    def pack(conv_, weight=None, owner=None, pieces=3):
        return ("wide bf16x%d" % pieces, conv_.weight if weight is None else weight)

    def run(x, pk, cout, dilation=1, conv_bias=None, bn=None, activation="none", geometry=0, pieces=3):
        return conv("bf16x%d" % pieces, "wide", x, pk, "wide bf16x%d" % pieces, 1, dilation, conv_bias, bn, activation)

    def run_res(x, pk, cout, dilation, residual, bn, activation, conv_bias=None, geometry=0):
        return conv("bf16x3", "wide", x, pk, "wide bf16x3", 1, dilation, conv_bias, bn, activation, residual)

    def run_narrow(x, pk, cout, dilation, residual=None, conv_bias=None, bn=None, activation="none", geometry=0):
        return conv("bf16x3", "narrow", x, pk, "narrow bf16x3", 1, dilation, conv_bias, bn, activation, residual)

    def run_s2(x, pk, cout, conv_bias=None, bn=None, activation="none", pieces=3):
        return conv("bf16x%d" % pieces, "s2", x, pk, "wide bf16x%d" % pieces, 2, 1, conv_bias, bn, activation)
    H = "fp16x2"
    has_entry = _lib.has_entry
    monkeypatch.setattr(_lib, "has_entry", lambda name: name in PC._TEACHER_EARLY_ENTRIES or has_entry(name))
    monkeypatch.setattr(SF, "infer2h_supported", lambda: True)
    monkeypatch.setattr(SF, "_conv3x3_ok", ok)
    monkeypatch.setattr(SF, "conv3x3_pack_weights", pack)
    monkeypatch.setattr(SF, "conv3x3_pack_weights_fp16", lambda c, weight=None, owner=None: ("wide " + H, c.weight if weight is None else weight))
    monkeypatch.setattr(SF, "conv3x3_narrow_pack_weights", lambda c, weight=None, owner=None: ("narrow bf16x3", c.weight))
    monkeypatch.setattr(SF, "conv3x3_narrow_pack_weights_fp16", lambda c, weight=None, owner=None: ("narrow " + H, c.weight))
    monkeypatch.setattr(SF, "conv3x3_split_eval", run)
    monkeypatch.setattr(SF, "conv3x3_split_res_eval", run_res)
    monkeypatch.setattr(SF, "conv3x3_narrow_eval", run_narrow)
    monkeypatch.setattr(SF, "conv3x3_s2_eval", run_s2)
    monkeypatch.setattr(SF, "conv3x3_split_eval_fp16", lambda x, pk, cout, dilation=1, conv_bias=None, bn=None, activation="none", geometry=0:
                        conv(H, "wide", x, pk, "wide " + H, 1, dilation, conv_bias, bn, activation))
    monkeypatch.setattr(SF, "conv3x3_split_res_eval_fp16", lambda x, pk, cout, dilation, residual, bn, activation, conv_bias=None, geometry=0:
                        conv(H, "wide", x, pk, "wide " + H, 1, dilation, conv_bias, bn, activation, residual))
    monkeypatch.setattr(SF, "conv3x3_narrow_eval_fp16",
                        lambda x, pk, cout, dilation, residual=None, conv_bias=None, bn=None, activation="none", geometry=0:
                        conv(H, "narrow", x, pk, "narrow " + H, 1, dilation, conv_bias, bn, activation, residual))
    monkeypatch.setattr(SF, "conv3x3_s2_eval_fp16", lambda x, pk, cout, conv_bias=None, bn=None, activation="none":
                        conv(H, "s2", x, pk, "wide " + H, 2, 1, conv_bias, bn, activation))
    return double


# the 20 convolutions fuse_for_inference(narrow=True, stride2=True) routes, in the order of the forward: (form, Cin, Cout, dilation)
STEM = [("narrow", 64, 64, 1), ("wide", 64, 128, 1)]
LAYER1 = [("narrow", 128, 64, 1), ("narrow+res", 64, 64, 1), ("narrow", 64, 64, 1), ("narrow+res", 64, 64, 1)]
LAYER2 = [("s2", 64, 128, 1), ("wide+res", 128, 128, 1), ("wide", 128, 128, 1), ("wide+res", 128, 128, 1)]
LAYER3 = [("wide", 128, 256, 2), ("wide+res", 256, 256, 2), ("wide", 256, 256, 2), ("wide+res", 256, 256, 2)]
LAYER4 = [("wide", 256, 512, 4), ("wide+res", 512, 512, 4), ("wide", 512, 512, 4), ("wide+res", 512, 512, 4)]
FLAGGED = STEM + LAYER1 + LAYER2 + LAYER3 + LAYER4
UNFLAGGED = [("wide", 256, 128, 1), ("wide", 512, 128, 1)]      # dsn[0] and the PSP bottleneck's feature half: no opt-in is about them


def _forward(net, grad=False):
    x = torch.randn(1, 3, 33, 49, generator=torch.Generator().manual_seed(11)).contiguous(memory_format=torch.channels_last)
    with torch.set_grad_enabled(grad):
        return net(x)


def _convs(log):
    return [c for c in log if c[1] != "1x1"]


def test_routing_of_the_flagged_student(rec, monkeypatch):
    net = _student()
    # the switch off: the recorded calls are today's -- every routed convolution on three bf16 pieces, through the three-piece ops
    networks.fuse_for_inference(net, narrow=True, stride2=True)
    off = _forward(net)
    log_off = _convs(rec.log)
    assert [c for c in log_off if c[1:] not in UNFLAGGED] == [("bf16x3",) + c for c in FLAGGED]
    assert UNFLAGGED[0] in [c[1:] for c in log_off] and all(c[0] == "bf16x3" for c in log_off)      # dsn[0] at least (the pyramid's
    # convolution only where the feature map is 6 x 6 or more)
    # the switch on: the same call sites, each on the fp16 twin of its form; dsn[0] and the PSP half keep three pieces
    rec.log.clear()
    networks.fuse_for_inference(net, narrow=True, stride2=True, piece_format="fp16")
    on = _forward(net)
    log_on = _convs(rec.log)
    assert [c[1:] for c in log_on] == [c[1:] for c in log_off], "the same forms at the same call sites"
    assert all(c[0] == ("bf16x3" if c[1:] in UNFLAGGED else "fp16x2") for c in log_on), log_on
    assert all(torch.equal(a, b) for a, b in zip(on, off)), "the double computes every form alike: the wiring is the same"
    # without ``narrow`` / ``stride2`` the switch adds no call site
    rec.log.clear()
    networks.fuse_for_inference(net, piece_format="fp16")
    _forward(net)
    assert [c for c in _convs(rec.log) if c[1:] not in UNFLAGGED] == [("fp16x2",) + c for c in LAYER2[1:] + LAYER3 + LAYER4]
    # an excluded shape keeps THREE bf16 pieces, form by form
    excluded = {("narrow+res", 64, 64, 1), ("wide", 256, 256, 2), ("s2", 64, 128, 1), ("wide+res", 512, 512, 4), ("wide", 64, 128, 1)}
    monkeypatch.setattr(PC, "INFER2H_ROUTING_EXCLUDED", frozenset(excluded))
    rec.log.clear()
    networks.fuse_for_inference(net, narrow=True, stride2=True, piece_format="fp16")
    _forward(net)
    assert [c for c in _convs(rec.log) if c[1:] not in UNFLAGGED] == [("bf16x3" if c in excluded else "fp16x2",) + c for c in FLAGGED]
    monkeypatch.setattr(PC, "INFER2H_ROUTING_EXCLUDED", frozenset())
    # a grad-enabled or training-mode forward is unrouted
    rec.log.clear()
    _forward(net, grad=True)
    net.train()
    with torch.no_grad():
        net.layer1(torch.randn(2, 128, 5, 6).contiguous(memory_format=torch.channels_last))
        net.layer3(torch.randn(2, 128, 5, 6).contiguous(memory_format=torch.channels_last))
    net.eval()
    assert _convs(rec.log) == []
    # enable=False: the marks and the flags go, and nothing of the blocks is routed
    networks.fuse_for_inference(net, enable=False)
    _forward(net)
    assert [c for c in _convs(rec.log) if c[1:] not in UNFLAGGED] == [] and _marks(net) == []


def test_prepack_makes_the_fp16_packs_when_flagging(rec, monkeypatch):
    made = []
    for name in ("conv3x3_pack_weights", "conv3x3_pack_weights_fp16", "conv3x3_narrow_pack_weights", "conv3x3_narrow_pack_weights_fp16"):
        monkeypatch.setattr(SF, name, lambda c, weight=None, owner=None, pieces=3, name=name: made.append((name, c.in_channels, c.out_channels)))
    net = _student()
    networks.fuse_for_inference(net, narrow=True, stride2=True, piece_format="fp16")
    assert sorted(made) == sorted([("conv3x3_narrow_pack_weights_fp16" if f.startswith("narrow") else "conv3x3_pack_weights_fp16", ci, co)
                                   for f, ci, co, _ in FLAGGED]), "one twin pack per routed convolution, and no three-piece pack"
    del made[:]
    monkeypatch.setattr(PC, "INFER2H_ROUTING_EXCLUDED", frozenset({("s2", 64, 128, 1), ("narrow", 64, 64, 1)}))
    networks.fuse_for_inference(net, narrow=True, stride2=True, piece_format="fp16")
    assert ("conv3x3_pack_weights", 64, 128) in made and made.count(("conv3x3_narrow_pack_weights", 64, 64)) == 2
    # enable=False drops the packs of both forms
    dropped = []
    monkeypatch.setattr(SF, "drop_conv3x3_packs", dropped.append)
    networks.fuse_for_inference(net, enable=False)
    assert len(dropped) == 8 * 2 + 2


def test_a_teacher_marked_for_fp16_pieces_keeps_its_stride2_convolution_on_three(rec):
    """set_teacher_pieces and what it routes are untouched: the teacher's stride-2 convolution has a kernel twin now, and still
    runs on THREE bf16 pieces under the teacher's fp16 mark (tests/test_split2h_cpu.py pins the same)."""
    torch.manual_seed(11)
    down = torch.nn.Sequential(torch.nn.Conv2d(256, 512, 1, 2, bias=False), PC.BatchNorm2d(512))
    layer2 = torch.nn.Sequential(PC.Bottleneck(256, 128, 2, downsample=down), PC.Bottleneck(512, 128))
    net = torch.nn.Sequential(torch.nn.Sequential(PC.Bottleneck(256, 64)), layer2).eval().to(memory_format=torch.channels_last)
    networks.set_teacher_pieces(net, 2, piece_format="fp16")
    PC.route_teacher_early(net)
    with torch.no_grad():
        net(_cl(1, 256, 9, 9, seed=12))
    assert _convs(rec.log) == [("bf16x3", "narrow", 64, 64, 1), ("bf16x3", "s2", 128, 128, 1), ("fp16x2", "wide", 128, 128, 1)]
    assert not any(hasattr(m, "_skd_infer_piece_format") for m in net.modules())
    # and the student's mark means nothing to a Bottleneck network
    rec.log.clear()
    networks.set_teacher_pieces(net, 3)
    for m in net.modules():
        if isinstance(m, PC.Bottleneck):
            m._skd_infer_piece_format = "fp16"
    with torch.no_grad():
        net(_cl(1, 256, 9, 9, seed=12))
    assert all(c[0] == "bf16x3" for c in _convs(rec.log))


# ---- 5. the public switch --------------------------------------------------------------------------------------------------------

def test_infer_piece_format_configuration(double, monkeypatch):
    for name in ("SKD_INFER_PIECE_FORMAT", "SKD_SPLIT_NARROW", "SKD_SPLIT_STRIDE2", "SKD_TEACHER_PIECES", "SKD_TEACHER_PIECE_FORMAT"):
        monkeypatch.delenv(name, raising=False)
    assert default_args().infer_piece_format == "bf16" and default_args(infer_piece_format="fp16").infer_piece_format == "fp16"
    for junk in ("f16", "fp8", 2, "FP16", ""):
        with pytest.raises(ValueError, match="SKD_INFER_PIECE_FORMAT"):
            default_args(infer_piece_format=junk)
    monkeypatch.setenv("SKD_INFER_PIECE_FORMAT", "fp16")
    assert default_args().infer_piece_format == "fp16" and default_args(infer_piece_format="bf16").infer_piece_format == "bf16"
    monkeypatch.setenv("SKD_INFER_PIECE_FORMAT", "half")
    with pytest.raises(ValueError):
        default_args()
    monkeypatch.delenv("SKD_INFER_PIECE_FORMAT")
    from structure_knowledge_distillation_amd.networks import kd_model
    assert "infer_piece_format" not in [s[0] for s in kd_model.SWITCHES], "handled outside SWITCHES"
    kw = dict(device=torch.device("cpu"), batch_size=2, ho=False)
    # without fused_eval: one warning, nothing routed
    with pytest.warns(RuntimeWarning, match="fused_eval") as caught:
        model = NetModel(default_args(infer_piece_format="fp16", **kw))
    assert len([w for w in caught if "fused_eval" in str(w.message)]) == 1
    assert model.infer_piece_format == "fp16" and _marks(model.student) == []
    assert not any(getattr(m, "_skd_infer_min_cin", None) is not None for m in model.student.modules())
    # with fused_eval on a back-end without the entries: the warning, and three pieces
    with pytest.warns(RuntimeWarning, match="skd_infer2h.h.*three pieces"):
        model = NetModel(default_args(infer_piece_format="fp16", fused_eval=True, **kw))
    assert _marks(model.student) == [] and model.student.layer3[0]._skd_infer_min_cin == PC.FUSED_EVAL_MIN_CIN
    # with the entries: the student is marked, the teacher is not
    monkeypatch.setattr(SF, "infer2h_supported", lambda: True)
    monkeypatch.setattr(PC, "_prepack", lambda module, convs: None)
    model = NetModel(default_args(infer_piece_format="fp16", fused_eval=True, **kw))
    assert sorted(_marks(model.student)) == ["BasicBlock"] * 8 + ["ResNet"] and _marks(model.teacher) == []
    # the default: fused_eval flags what it flagged, with no mark and no warning
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        model = NetModel(default_args(fused_eval=True, **kw))
    assert model.infer_piece_format == "bf16" and _marks(model.student) == []
