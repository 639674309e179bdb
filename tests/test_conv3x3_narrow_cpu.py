"""The 64-column form of the split-core 3x3 convolution, the parts that need no GPU: the C ABI of include/skd_narrow.h (header <->
table <-> exported symbols, the truth table of the query, the pack size, host-side refusals), the routing of a ``narrow``-flagged
student in its inference and training forms (a recording double of the entries on top of the plain-C double), the wiring against
the plain op sequence (a torch-implemented double), NetModel's ``split_narrow`` flag and the rebuilding of a stale narrow pack."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import structure_knowledge_distillation_amd.networks.pspnet_combine as PC
from oracle import cref
from structure_knowledge_distillation_amd import _lib, functional as SF
from structure_knowledge_distillation_amd import networks
from test_conv3x3_train_cpu import TrainDouble
from test_student_infer_cpu import ENTRY, RES_ENTRY, _host

SUPPORTED, PACK_BYTES = "skd_conv3x3_narrow_supported", "skd_conv3x3_narrow_pack_bytes"
PACK_PAIR, NARROW = "skd_conv3x3_narrow_pack_pair", "skd_conv3x3_narrow_nhwc"


class NarrowDouble(TrainDouble):
    """TrainDouble + the four entries of skd_narrow.h on raw HOST addresses.  Like its bases' packs, a narrow "pack" is a handle:
    pack_pair remembers w under pack_fwd's address and the flipped, transposed Wd under pack_bwd's; either may be absent, in both
    pack_pair entries (the wide one writes a single image for a convolution with one 64-channel side)."""

    def __init__(self, core, compute):
        super().__init__(core, compute)
        self.narrow_pairs = []

    def _remember(self, log, cin, cout, w, strides, pack_fwd, pack_bwd):
        sn, sc, sy, sx = strides
        base = _host(w, (1 + (cout - 1) * sn + (cin - 1) * sc + 2 * sy + 2 * sx,))
        view = np.lib.stride_tricks.as_strided(base, shape=(cout, cin, 3, 3), strides=tuple(4 * s for s in strides))
        wt = torch.from_numpy(view.copy())
        if pack_fwd:
            self.weights[pack_fwd] = wt
        if pack_bwd:
            self.weights[pack_bwd] = wt.flip(2, 3).transpose(0, 1).contiguous()
        log.append(dict(cin=cin, cout=cout, w=w, strides=strides, fwd=pack_fwd, bwd=pack_bwd))
        return 1

    def skd_conv3x3_split_pack_pair(self, cin, cout, w, sn, sc, sy, sx, pack_fwd, fwd_bytes, pack_bwd, bwd_bytes, stream):
        assert (pack_fwd or pack_bwd) and (not pack_fwd or (cout % 128 == 0 and fwd_bytes == cin * cout * 54))
        assert not pack_bwd or (cin % 128 == 0 and bwd_bytes == cin * cout * 54)
        return self._remember(self.pairs, cin, cout, w, (sn, sc, sy, sx), pack_fwd, pack_bwd)

    def skd_conv3x3_narrow_supported(self, cin, cout, stride, padding, dilation, groups):
        return int(cin > 0 and cout > 0 and cin % 16 == 0 and cout % 64 == 0 and stride == 1 and dilation >= 1
                   and padding == dilation and groups == 1)

    def skd_conv3x3_narrow_pack_bytes(self, cin, cout):
        return cout * cin * 54 if self.skd_conv3x3_narrow_supported(cin, cout, 1, 1, 1, 1) else 0

    def skd_conv3x3_narrow_pack_pair(self, cin, cout, w, sn, sc, sy, sx, pack_fwd, fwd_bytes, pack_bwd, bwd_bytes, stream):
        assert (pack_fwd or pack_bwd) and (not pack_fwd or (cout % 64 == 0 and fwd_bytes == cin * cout * 54))
        assert not pack_bwd or (cin % 64 == 0 and bwd_bytes == cin * cout * 54)
        return self._remember(self.narrow_pairs, cin, cout, w, (sn, sc, sy, sx), pack_fwd, pack_bwd)

    def skd_conv3x3_narrow_nhwc(self, B, H, W, cin, cout, dil, x, pack, out, res, cbias, mean, var, weight, bias, eps, act, slope,
                                geometry, stream):
        return self._conv(NARROW, B, H, W, cin, cout, dil, x, pack, out, res, cbias, mean, var, weight, bias, eps, act, slope)


@pytest.fixture
def recording():
    d = NarrowDouble(cref.load(_lib.SIGNATURES), compute=False)
    _lib.install_test_backend(d)
    yield d
    _lib.install_test_backend(None)


@pytest.fixture
def computing():
    d = NarrowDouble(cref.load(_lib.SIGNATURES), compute=True)
    _lib.install_test_backend(d)
    yield d
    _lib.install_test_backend(None)


# ---- 1. the C ABI ------------------------------------------------------------------------------------------------------------

def test_narrow_header_table_and_library_agree():
    """What is particular to skd_narrow.h; header <-> table <-> library <-> build digest: tests/test_abi.py, for every header."""
    assert sorted(_lib.ABI["skd_narrow.h"]) == sorted([SUPPORTED, PACK_BYTES, PACK_PAIR, NARROW]) and len(_lib.ABI["skd_narrow.h"]) == 4
    # the argument lists of the wide entries
    assert _lib.signature(SUPPORTED) == _lib.signature("skd_conv3x3_split_supported")
    assert _lib.signature(PACK_BYTES) == _lib.signature("skd_conv3x3_split_pack_bytes")
    assert _lib.signature(PACK_PAIR) == _lib.signature("skd_conv3x3_split_pack_pair")
    assert _lib.signature(NARROW) == _lib.signature(RES_ENTRY)


def test_narrow_supported_truth_table_and_pack_bytes():
    lib = _lib.load()
    sup, nbytes = lib.skd_conv3x3_narrow_supported, lib.skd_conv3x3_narrow_pack_bytes
    for cin, cout in ((64, 64), (16, 64), (32, 192), (64, 128), (128, 64), (512, 64), (48, 320), (128, 256)):
        for d in (1, 2, 4):
            assert sup(cin, cout, 1, d, d, 1) == 1, (cin, cout, d)
        # per column tile of 64 channels and K-tile of 16: three planes of 128 chunks of 16 bytes -- 6 bytes per weight
        assert nbytes(cin, cout) == (cout // 64) * (9 * cin // 16) * 384 * 16 == cout * cin * 54
    for bad in ((64, 32, 1, 1, 1, 1), (64, 96, 1, 1, 1, 1), (24, 64, 1, 1, 1, 1), (8, 64, 1, 1, 1, 1), (0, 64, 1, 1, 1, 1),
                (64, 0, 1, 1, 1, 1), (-64, 64, 1, 1, 1, 1), (64, -64, 1, 1, 1, 1), (64, 64, 2, 1, 1, 1), (64, 64, 1, 1, 2, 1),
                (64, 64, 1, 2, 1, 1), (64, 64, 1, 0, 0, 1), (64, 64, 1, 1, 1, 2)):
        assert sup(*bad) == 0, bad
    for cin, cout in ((64, 32), (24, 64), (0, 64), (64, 0)):
        assert nbytes(cin, cout) == 0
    # the existing entries keep refusing a Cout of 64
    assert lib.skd_conv3x3_split_supported(256, 64, 1, 1, 1, 1) == 0 and lib.skd_conv3x3_split_pack_bytes(256, 64) == 0
    assert lib.skd_conv3x3_split_train_supported(64, 128, 1, 1, 1, 1) == 0


def test_narrow_pack_pair_host_side_refusals():
    """Every refusal is decided on the host, in front of the launch: no device is touched (the pointers are never followed)."""
    f = _lib.load().skd_conv3x3_narrow_pack_pair
    W, PF, PB = 0x10000, 0x2000000, 0x4000000
    n = 64 * 64 * 54
    ok = dict(cin=64, cout=64, w=W, sn=576, sc=9, sy=3, sx=1, pf=PF, fb=n, pb=PB, bb=n)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["cin"], a["cout"], a["w"], a["sn"], a["sc"], a["sy"], a["sx"], a["pf"], a["fb"], a["pb"], a["bb"], None)
    for bad in (dict(w=None), dict(pf=None, pb=None), dict(pf=PF + 8), dict(pb=PB + 4), dict(pf=PF + 8, pb=None), dict(pf=None, pb=PB + 4),
                dict(fb=n - 1), dict(bb=n - 1), dict(fb=0), dict(bb=-1), dict(pf=None, bb=n - 1), dict(pb=None, fb=n - 1),
                dict(sn=-1), dict(sc=-9), dict(sy=-3), dict(sx=-1),
                dict(cin=32), dict(cout=32), dict(cin=24), dict(cout=24), dict(cin=0), dict(cout=-64),
                # one image only: its own direction has to fit (N a multiple of 64, K of 16)
                dict(cout=32, pb=None), dict(cin=32, pf=None), dict(cout=24, pf=None), dict(cin=24, pb=None)):
        assert call(**bad) == 0, bad


def test_narrow_conv_host_side_refusals():
    f = _lib.load().skd_conv3x3_narrow_nhwc
    X, WP, OUT, RES, V = 0x10000, 0x20000, 0x4000000, 0x8000000, 0x30000
    ok = dict(B=1, H=4, W=4, cin=32, cout=64, d=1, x=X, wp=WP, out=OUT, res=RES, cb=None, mean=None, var=None, w=None, b=None,
              eps=1e-5, act=3, slope=0.01, geo=0)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["B"], a["H"], a["W"], a["cin"], a["cout"], a["d"], a["x"], a["wp"], a["out"], a["res"], a["cb"], a["mean"], a["var"],
                 a["w"], a["b"], a["eps"], a["act"], a["slope"], a["geo"], None)
    nbytes = 1 * 4 * 4 * 64 * 4
    for bad in (dict(x=None), dict(wp=None), dict(out=None), dict(mean=V), dict(var=V), dict(geo=-1), dict(geo=2), dict(cout=32),
                dict(cout=96), dict(cin=24), dict(d=0), dict(d=-2), dict(B=0), dict(H=0), dict(W=-1), dict(act=2), dict(act=7),
                dict(x=X + 4), dict(wp=WP + 8),
                # a residual that overlaps the output: the same buffer, one float into it from either side, its last float
                dict(res=OUT), dict(res=OUT + 4), dict(res=OUT - 4), dict(res=OUT + nbytes - 4), dict(res=OUT - nbytes + 4),
                # the residual-free form refuses the same things
                dict(res=None, x=None), dict(res=None, cout=32), dict(res=None, geo=2), dict(res=None, mean=V)):
        assert call(**bad) == 0, bad


# ---- 2. routing -------------------------------------------------------------------------------------------------------------

def _student(train=False):
    torch.manual_seed(5)
    net = PC.Res_pspnet(PC.BasicBlock, [2, 2, 2, 2], 19).to(memory_format=torch.channels_last)
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.p = 0.0
    return net.train() if train else net.eval()


def _input(h=33, w=49, b=1):
    return torch.randn(b, 3, h, w, generator=torch.Generator().manual_seed(11)).contiguous(memory_format=torch.channels_last)


def _small(calls):
    return [c for c in calls if 64 in (c["cin"], c["cout"])]


def test_inference_routing_of_a_narrow_flagged_student(recording, monkeypatch):
    net = _student()
    x = _input()
    seen, down = {}, []
    for name, m in net.named_modules():
        if isinstance(m, PC.BasicBlock):
            m.register_forward_pre_hook(lambda mod, args, name=name: seen.__setitem__(name, args[0]))
    net.layer1[0].downsample.register_forward_hook(lambda mod, args, out: down.append(out))
    real = PC._conv1x1_bn_eval
    monkeypatch.setattr(PC, "_conv1x1_bn_eval", lambda x, conv, bn, relu: (down.append(real(x, conv, bn, relu)), down[-1])[1]
                        if conv is net.layer1[0].downsample[0] else real(x, conv, bn, relu))
    with torch.no_grad():
        net(x)
        assert _small(recording.calls) == []
        networks.fuse_for_inference(net)                       # the default flag: no call with 64 channels, nothing packed for them
        net(x)
    assert _small(recording.calls) == [] and recording.narrow_pairs == [] and recording.packs == 11
    assert not any(getattr(m, "_skd_infer_narrow", False) for m in net.modules())

    recording.calls.clear()
    assert networks.fuse_for_inference(net, narrow=True) is net
    flagged = [m for m in net.modules() if isinstance(m, (PC.BasicBlock, PC.ResNet))]
    assert len(flagged) == 9 and all(m._skd_infer_narrow is True for m in flagged)
    # packed at flag time: stem conv2 and layer1's four on the narrow entry, stem conv3 on the wide one
    want_w = [net.conv2, net.layer1[0].conv1, net.layer1[0].conv2, net.layer1[1].conv1, net.layer1[1].conv2]
    assert [p["w"] for p in recording.narrow_pairs] == [c.weight.data_ptr() for c in want_w]
    assert all(p["fwd"] and not p["bwd"] for p in recording.narrow_pairs)
    assert [(p["cin"], p["cout"]) for p in recording.narrow_pairs] == [(64, 64), (128, 64), (64, 64), (64, 64), (64, 64)]
    assert recording.packs == 12 and hasattr(net.conv3, "_skd_conv3x3_pack") and not hasattr(net.conv1, "_skd_conv3x3_pack")
    with torch.no_grad():
        out = net(x)
    assert all(bool(torch.isfinite(o).all()) for o in out)
    assert len(recording.narrow_pairs) == 5 and recording.packs == 12, "nothing is packed again in the forward"
    calls = recording.calls
    six = calls[:6]
    assert _small(calls) == six, "exactly the six 64-channel launches, first"
    assert [(c["entry"], c["cin"], c["cout"], c["dilation"], c["act"]) for c in six] == [
        (NARROW, 64, 64, 1, 3), (ENTRY, 64, 128, 1, 0), (NARROW, 128, 64, 1, 3), (NARROW, 64, 64, 1, 3), (NARROW, 64, 64, 1, 3),
        (NARROW, 64, 64, 1, 3)]       # layer1.0.conv1 reads the stem's 128 channels
    ptrs = lambda bn: tuple(t.data_ptr() for t in (bn.running_mean, bn.running_var, bn.weight, bn.bias))
    l10, l11 = net.layer1[0], net.layer1[1]
    assert [c["bn"] for c in six] == [ptrs(net.bn2), (None,) * 4, ptrs(l10.bn1), ptrs(l10.bn2), ptrs(l11.bn1), ptrs(l11.bn2)]
    del down[:-1]                        # the flagged forward's: layer1.0's residual is its down-sample branch
    assert [c["residual"] for c in six] == [None, None, None, down[0].data_ptr(), None, seen["layer1.1"].data_ptr()]
    assert six[2]["x"] == seen["layer1.0"].data_ptr() and six[4]["x"] == seen["layer1.1"].data_ptr()
    assert six[3]["residual"] != six[3]["x"]
    # the stride-2 convolutions and conv1 never appear; everything else is what the default flag routes
    assert not [c for c in calls if c["cin"] == 3] and len([c for c in calls if (c["cin"], c["cout"]) == (128, 128)]) == 3
    assert len(calls) == 6 + 11

    # training mode, or a graph: nothing is routed
    recording.calls.clear()
    net(x)
    net.train()
    with torch.no_grad():
        net(_input(b=2))
    net.eval()
    assert recording.calls == []

    # an excluded shape keeps the library
    try:
        PC.NARROW_ROUTING_EXCLUDED = frozenset({(64, 64, 1, "infer")})
        with torch.no_grad():
            net(x)
    finally:
        PC.NARROW_ROUTING_EXCLUDED = frozenset()
    assert [(c["entry"], c["cin"], c["cout"]) for c in _small(recording.calls)] == [(ENTRY, 64, 128), (NARROW, 128, 64)]
    recording.calls.clear()
    try:
        PC.NARROW_ROUTING_EXCLUDED = frozenset({(64, 128, 1, "infer"), (64, 64, 1, "train")})
        with torch.no_grad():
            net(x)
    finally:
        PC.NARROW_ROUTING_EXCLUDED = frozenset()
    assert [c["entry"] for c in _small(recording.calls)] == [NARROW] * 5

    # an unflagged network (the teacher is one) is untouched; enable=False drops the new packs too
    recording.calls.clear()
    assert networks.fuse_for_inference(net, enable=False) is net
    assert not any(getattr(m, "_skd_infer_narrow", False) for m in net.modules())
    assert not any(hasattr(m, a) for m in net.modules() for a in ("_skd_conv3x3_pack", "_skd_conv3x3_narrow_pack"))
    with torch.no_grad():
        net(x)
    assert recording.calls == []


def test_training_routing_of_a_narrow_flagged_student(recording):
    from test_conv3x3_train_cpu import ROUTED, RUN
    net = _student(train=True)
    x = _input(49, 57, 2)
    networks.route_training_convs(net)
    net(x)
    assert _small(recording.calls) == [] and recording.narrow_pairs == [] and len(recording.calls) == 13

    recording.calls.clear()
    assert networks.route_training_convs(net, narrow=True) is net
    flagged = [m for m in net.modules() if isinstance(m, (PC.BasicBlock, PC.ResNet, PC.PSPModule))]
    assert len(flagged) == 10 and all(m._skd_train_narrow is True and m._skd_train_min_cin == 128 for m in flagged)
    net(x)
    calls = recording.calls
    assert [(c["entry"], c["cin"], c["cout"]) for c in calls[:6]] == [(NARROW, 64, 64), (RUN, 64, 128), (NARROW, 128, 64)] + [(NARROW, 64, 64)] * 3
    assert _small(calls) == calls[:6] and [(c["cin"], c["cout"], c["dilation"]) for c in calls[6:]] == ROUTED
    assert all(c["act"] == 0 and c["residual"] is None and c["bn"] == (None,) * 4 for c in calls)
    # packs: 64 -> 64 one narrow launch writing both images; 64 -> 128 (stem conv3) and 128 -> 64 (layer1.0.conv1) one launch per
    # entry -- the image whose N is 128 wide, the other narrow
    convs = [net.conv2, net.conv3, net.layer1[0].conv1, net.layer1[0].conv2, net.layer1[1].conv1, net.layer1[1].conv2]
    assert [p["w"] for p in recording.narrow_pairs] == [c.weight.data_ptr() for c in convs]
    assert [(bool(p["fwd"]), bool(p["bwd"])) for p in recording.narrow_pairs] == [(True, True), (False, True), (True, False)] + [(True, True)] * 3
    half = [p for p in recording.pairs if not (p["fwd"] and p["bwd"])]
    assert len(recording.pairs) == 15 and len(half) == 2
    assert half[0]["w"] == net.conv3.weight.data_ptr() and half[0]["fwd"] and not half[0]["bwd"]
    assert half[1]["w"] == net.layer1[0].conv1.weight.data_ptr() and half[1]["bwd"] and not half[1]["fwd"]
    # once per weight version
    net(x)
    assert len(recording.narrow_pairs) == 6 and len(recording.pairs) == 15

    # eval mode or no grad: the training form routes nothing
    recording.calls.clear()
    net.eval()
    net(x)
    net.train()
    with torch.no_grad():
        net(x)
    assert recording.calls == []
    # an excluded shape keeps the library
    try:
        PC.NARROW_ROUTING_EXCLUDED = frozenset({(64, 64, 1, "train"), (64, 128, 1, "infer")})
        net(x)
    finally:
        PC.NARROW_ROUTING_EXCLUDED = frozenset()
    assert [(c["entry"], c["cin"], c["cout"]) for c in _small(recording.calls)] == [(RUN, 64, 128), (NARROW, 128, 64)]
    # enable=False: the first state, and the packs are gone
    recording.calls.clear()
    networks.route_training_convs(net, enable=False)
    assert not any(getattr(m, "_skd_train_narrow", False) for m in net.modules())
    assert not any(hasattr(m, a) for m in net.modules() for a in SF._NARROW_PACK_ATTRS + ("_skd_conv3x3_train_pack",))
    net(x)
    assert recording.calls == []


def test_plain_c_double_keeps_todays_sequence():
    """A back-end without the entries: flagged networks run what they ran, nothing raises."""
    _lib.install_test_backend(cref.load(_lib.SIGNATURES))
    try:
        assert not any(_lib.has_entry(n) for n in _lib.ABI["skd_narrow.h"])
        net, x = _student(), _input()
        with torch.no_grad():
            want = net(x)
            got = networks.fuse_for_inference(net, narrow=True)(x)
        assert all(torch.equal(a, b) for a, b in zip(want, got))
        tr, xt = _student(train=True), _input(49, 57, 2)
        flagged = networks.route_training_convs(copy.deepcopy(tr), narrow=True)
        assert all(torch.equal(a, b) for a, b in zip(tr(xt), flagged(xt)))
        with pytest.raises(NotImplementedError, match=NARROW):
            with torch.no_grad():
                SF.conv3x3_narrow_eval(torch.zeros(1, 16, 2, 2), torch.zeros(4, dtype=torch.uint8), 64, 1)
    finally:
        _lib.install_test_backend(None)


# ---- 3. wiring ----------------------------------------------------------------------------------------------------------------

def _randomise(net, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if hasattr(m, "running_mean") and m.running_mean is not None:
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.3)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
                m.weight.copy_(torch.randn(m.weight.shape, generator=g).abs() * 0.5 + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
    return net


def test_flagged_eval_forward_equals_the_plain_one(computing):
    net = _randomise(_student(), 3)
    x = _input(65, 65)
    with torch.no_grad():
        want = net(x)
        assert computing.calls == []
        got = networks.fuse_for_inference(net, narrow=True)(x)
    assert [(c["entry"], c["cin"]) for c in computing.calls[:6]] == [(NARROW, 64), (ENTRY, 64), (NARROW, 128)] + [(NARROW, 64)] * 3
    for a, b in zip(got, want):
        err = float((a - b).abs().max() / b.abs().max())
        assert a.shape == b.shape and err <= 2e-5, err
    # the check has teeth: the stem's bn2 and layer1's BNs differ
    assert not torch.allclose(net.bn2.running_mean, net.layer1[0].bn1.running_mean)


@pytest.mark.parametrize("cin,cout", [(64, 64), (64, 128), (128, 64)])
def test_training_op_equals_autograd_of_conv2d(computing, cin, cout):
    g = torch.Generator().manual_seed(cin + cout)
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    x = cl(torch.randn(2, cin, 6, 7, generator=g)).requires_grad_(True)
    w = cl(torch.randn(cout, cin, 3, 3, generator=g) * 0.05).requires_grad_(True)
    go = cl(torch.randn(2, cout, 6, 7, generator=g))
    assert SF.conv3x3_narrow_train_supported(x, w, 1, 2, 2, 1) and not SF.conv3x3_train_supported(x, w, 1, 2, 2, 1)
    assert not SF.conv3x3_narrow_train_supported(x, w, 2, 2, 2, 1) and not SF.conv3x3_narrow_train_supported(x, w, 1, 1, 2, 1)
    assert not SF.conv3x3_narrow_train_supported(x.detach().contiguous(), w, 1, 2, 2, 1)
    with torch.no_grad():
        assert not SF.conv3x3_narrow_train_supported(x, w, 1, 2, 2, 1)
    owner = torch.nn.Module()
    y = SF.conv3x3_split_train(x, w, 2, None, owner, narrow=True)
    dx, dw = torch.autograd.grad(y, (x, w), go)
    want = F.conv2d(x, w, None, 1, 2, 2)
    wdx, wdw = torch.autograd.grad(want, (x, w), go)
    rel = lambda a, b: float((a.detach() - b.detach()).abs().max() / b.detach().abs().max())
    assert rel(y, want) <= 1e-6 and rel(dx, wdx) <= 1e-6 and rel(dw, wdw) <= 1e-6
    # each direction on the entry its N chooses
    fwd, bwd = computing.calls
    assert (fwd["entry"], fwd["cin"], fwd["cout"]) == (NARROW if cout == 64 else ENTRY, cin, cout)
    assert (bwd["entry"], bwd["cin"], bwd["cout"]) == (NARROW if cin == 64 else ENTRY, cout, cin)
    assert len(computing.narrow_pairs) == 1 and len(computing.pairs) == (0 if cin == cout else 1)
    # both multiples of 128: narrow=True is the existing op, on the existing cache
    computing.calls.clear()
    w2 = cl(torch.randn(128, 128, 3, 3, generator=g) * 0.05).requires_grad_(True)
    SF.conv3x3_split_train(cl(torch.randn(1, 128, 4, 4, generator=g)), w2, 1, None, owner, narrow=True)
    assert computing.calls[0]["entry"] == ENTRY and hasattr(owner, "_skd_conv3x3_train_pack") and len(computing.narrow_pairs) == 1


def test_fused_optimizer_step_rebuilds_the_narrow_pack(computing):
    from structure_knowledge_distillation_amd.networks.kd_model import advance_versions_after_step
    torch.manual_seed(4)
    w = torch.nn.Parameter((torch.randn(64, 64, 3, 3) * 0.05).contiguous(memory_format=torch.channels_last))
    owner = torch.nn.Module()
    x = torch.randn(1, 64, 4, 5).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    try:
        opt = torch.optim.SGD([w], 0.5, fused=True)
    except (RuntimeError, TypeError, ValueError):                       # a torch without fused SGD on the host: the plain form
        opt = torch.optim.SGD([w], 0.5)
    opt.register_step_post_hook(advance_versions_after_step)
    y0 = SF.conv3x3_split_train(x, w, 1, owner=owner, narrow=True)
    y0.square().sum().backward()
    SF.conv3x3_split_train(x, w, 1, owner=owner, narrow=True)
    assert len(computing.narrow_pairs) == 1, "one split per weight version"
    version, before = w._version, w.detach().clone()
    opt.step()
    assert not torch.equal(w.detach(), before) and w._version > version
    y1 = SF.conv3x3_split_train(x, w, 1, owner=owner, narrow=True)
    assert len(computing.narrow_pairs) == 2, "the new weights were split"
    want = F.conv2d(x, w, None, 1, 1, 1)
    assert float((y1 - want).detach().abs().max()) <= 1e-6 * float(want.detach().abs().max()) and not torch.allclose(y1, y0)
    # the frozen form's pack follows the version as well
    conv = torch.nn.Conv2d(64, 64, 3, 1, 1, bias=False)
    with torch.no_grad():
        p0 = SF.conv3x3_narrow_pack_weights(conv)
        assert SF.conv3x3_narrow_pack_weights(conv) is p0
        conv.weight.mul_(0.5)
        assert SF.conv3x3_narrow_pack_weights(conv) is not p0
    SF.drop_conv3x3_packs(conv)
    assert not hasattr(conv, "_skd_conv3x3_narrow_pack")


# ---- 4. NetModel ----------------------------------------------------------------------------------------------------------------

def test_netmodel_split_narrow_flag(monkeypatch):
    from structure_knowledge_distillation_amd.networks.kd_model import NetModel, default_args
    monkeypatch.delenv("SKD_SPLIT_NARROW", raising=False)
    monkeypatch.delenv("SKD_SPLIT_TRAIN", raising=False)
    assert default_args().split_narrow is False
    monkeypatch.setenv("SKD_SPLIT_NARROW", "1")
    assert default_args().split_narrow is True and default_args(split_narrow=False).split_narrow is False
    monkeypatch.setenv("SKD_SPLIT_NARROW", "0")
    assert default_args().split_narrow is False and default_args(split_narrow=True).split_narrow is True
    _lib.install_test_backend(cref.load(_lib.SIGNATURES))
    try:
        kw = dict(device=torch.device("cpu"), batch_size=2, ho=False)
        infer = lambda model: [bool(getattr(m, "_skd_infer_narrow", False)) for m in model.student.modules()
                               if isinstance(m, (PC.BasicBlock, PC.ResNet))]
        train = lambda model: [bool(getattr(m, "_skd_train_narrow", False)) for m in model.student.modules()
                               if isinstance(m, (PC.BasicBlock, PC.ResNet, PC.PSPModule))]
        model = NetModel(default_args(**kw))
        assert infer(model) == [False] * 9 and train(model) == [False] * 10 and not model.split_narrow
        # alone it routes nothing
        model = NetModel(default_args(split_narrow=True, **kw))
        assert model.split_narrow and infer(model) == [False] * 9 and train(model) == [False] * 10
        model = NetModel(default_args(split_narrow=True, fused_eval=True, **kw))
        assert infer(model) == [True] * 9 and train(model) == [False] * 10
        model = NetModel(default_args(split_narrow=True, split_train=True, **kw))
        assert infer(model) == [False] * 9 and train(model) == [True] * 10
        assert NetModel(default_args(split_train=True, fused_eval=True, **kw)).split_narrow is False
        assert not any(getattr(m, "_skd_infer_narrow", False) or getattr(m, "_skd_train_narrow", False) for m in model.teacher.modules())
        monkeypatch.setenv("SKD_SPLIT_NARROW", "1")
        monkeypatch.setenv("SKD_SPLIT_TRAIN", "1")
        model = NetModel(default_args(**kw))
        assert train(model) == [True] * 10 and model.split_narrow and model.split_train
    finally:
        _lib.install_test_backend(None)


def test_docs_name_the_narrow_form():
    assert "conv3x3.hip" in PC.__doc__ and "64-column" in PC.__doc__ and "narrow" in PC.fuse_for_inference.__doc__ and "narrow" in PC.route_training_convs.__doc__
