"""The weight gradient of the student's 3x3 convolutions on the split core, the parts that need no GPU: the C ABI of
include/skd_wgrad.h (the pinned names and argument lists, the truth table of the predicate, the host-side refusals of the launch
entry, the split-K plan swept over sizes), the routing and the wiring of a student flagged with ``wgrad=True`` (a torch-implemented
double: TrainDouble + the three entries, the weight gradient computed by ``torch.nn.grad.conv2d_weight``) and NetModel's
``split_wgrad`` switch."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import structure_knowledge_distillation_amd.networks.pspnet_combine as PC
from oracle import cref
from structure_knowledge_distillation_amd import _lib, functional as SF
from structure_knowledge_distillation_amd import networks
from test_conv3x3_train_cpu import ROUTED, TrainDouble, _input, _step, _student
from test_student_infer_cpu import _host

SUPPORTED, PLAN, RUN = "skd_conv3x3_split_wgrad_supported", "skd_conv3x3_split_wgrad_plan", "skd_conv3x3_split_wgrad_nhwc"
CHANNEL_PAIRS = sorted({(cin, cout) for cin, cout, _ in ROUTED})


class WgradDouble(TrainDouble):
    """TrainDouble + the three entries of skd_wgrad.h on raw HOST addresses: the plan is one slice, the launch entry is
    ``torch.nn.grad.conv2d_weight`` written through the destination's strides.  Every launch is recorded."""

    def __init__(self, core, compute):
        super().__init__(core, compute)
        self.wgrads = []

    def skd_conv3x3_split_wgrad_supported(self, cin, cout, stride, padding, dilation, groups):
        return self.skd_conv3x3_split_train_supported(cin, cout, stride, padding, dilation, groups)

    def skd_conv3x3_split_wgrad_plan(self, B, H, W, cin, cout, slices, cus, plan):
        out = ctypes.cast(plan, ctypes.POINTER(ctypes.c_int64))
        out[0], out[1], out[2] = 1, -(-B * H * W // 16), 9 * cin * cout * 4
        return 1

    def skd_conv3x3_split_wgrad_nhwc(self, B, H, W, cin, cout, dil, x, g, dw, sn, sc, sy, sx, ws, ws_bytes, slices, stream):
        assert ws and ws_bytes == 9 * cin * cout * 4 and slices == 1
        self.wgrads.append(dict(cin=cin, cout=cout, dilation=dil, x=x, dw=dw, strides=(sn, sc, sy, sx)))
        xt = torch.from_numpy(_host(x, (B, H, W, cin)).copy()).permute(0, 3, 1, 2)
        gt = torch.from_numpy(_host(g, (B, H, W, cout)).copy()).permute(0, 3, 1, 2)
        grad = torch.nn.grad.conv2d_weight(xt, (cout, cin, 3, 3), gt, 1, dil, dil)
        base = _host(dw, (1 + (cout - 1) * sn + (cin - 1) * sc + 2 * sy + 2 * sx,))
        np.lib.stride_tricks.as_strided(base, shape=(cout, cin, 3, 3), strides=tuple(4 * s for s in (sn, sc, sy, sx)))[...] = grad.numpy()
        return 1


@pytest.fixture
def computing():
    d = WgradDouble(cref.load(_lib.SIGNATURES), compute=True)
    _lib.install_test_backend(d)
    yield d
    _lib.install_test_backend(None)


# ---- 1. the C ABI ------------------------------------------------------------------------------------------------------------

def test_wgrad_header_table_and_library_agree():
    """What is particular to skd_wgrad.h; header <-> table <-> library <-> build digest: tests/test_abi.py, for every header."""
    assert sorted(_lib.ABI["skd_wgrad.h"]) == sorted([SUPPORTED, PLAN, RUN]) and len(_lib.ABI["skd_wgrad.h"]) == 3
    assert _lib.signature(SUPPORTED) == _lib.signature("skd_conv3x3_split_train_supported")


def test_wgrad_supported_truth_table():
    lib = _lib.load()
    sup, train = lib.skd_conv3x3_split_wgrad_supported, lib.skd_conv3x3_split_train_supported
    for cin, cout in ((128, 128), (128, 256), (256, 128), (512, 512), (384, 128)):
        for d in (1, 2, 4):
            assert sup(cin, cout, 1, d, d, 1) == 1, (cin, cout, d)
    for bad in ((64, 128, 1, 1, 1, 1), (128, 64, 1, 1, 1, 1), (32, 128, 1, 1, 1, 1), (128, 32, 1, 1, 1, 1), (144, 128, 1, 1, 1, 1),
                (128, 192, 1, 1, 1, 1), (0, 128, 1, 1, 1, 1), (128, 0, 1, 1, 1, 1), (-128, 128, 1, 1, 1, 1),
                (128, 128, 2, 1, 1, 1), (128, 128, 1, 1, 2, 1), (128, 128, 1, 2, 1, 1), (128, 128, 1, 0, 0, 1), (128, 128, 1, 1, 1, 2)):
        assert sup(*bad) == 0, bad
    # the conditions of the training predicate, over a grid
    for cin in (0, 16, 64, 128, 144, 256):
        for cout in (0, 64, 128, 192, 512):
            for s, p, d, g in ((1, 1, 1, 1), (2, 1, 1, 1), (1, 2, 2, 1), (1, 1, 2, 1), (1, 0, 0, 1), (1, 1, 1, 2)):
                assert sup(cin, cout, s, p, d, g) == train(cin, cout, s, p, d, g), (cin, cout, s, p, d, g)


def test_wgrad_launch_host_side_refusals():
    """Every refusal is decided on the host, in front of the launches: no device is touched (the pointers are never followed)."""
    lib = _lib.load()
    X, G, DW, WS = 0x10000, 0x2000000, 0x4000000, 0x8000000
    b, h, w, c = 2, 13, 11, 128
    nk = -(-b * h * w // 16)
    plan = (ctypes.c_int64 * 3)()
    assert lib.skd_conv3x3_split_wgrad_plan(b, h, w, c, c, 3, 0, ctypes.cast(plan, ctypes.c_void_p)) == 1 and plan[0] == 3
    ok = dict(B=b, H=h, W=w, cin=c, cout=c, d=1, x=X, g=G, dw=DW, sn=9 * c, sc=9, sy=3, sx=1, ws=WS, nbytes=int(plan[2]), slices=3)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.skd_conv3x3_split_wgrad_nhwc(a["B"], a["H"], a["W"], a["cin"], a["cout"], a["d"], a["x"], a["g"], a["dw"], a["sn"],
                                                a["sc"], a["sy"], a["sx"], a["ws"], a["nbytes"], a["slices"], None)
    for bad in (dict(x=None), dict(g=None), dict(dw=None), dict(ws=None),
                dict(x=X + 4), dict(x=X + 8), dict(g=G + 4), dict(g=G + 8), dict(ws=WS + 4), dict(ws=WS + 8),
                dict(nbytes=int(plan[2]) - 1), dict(nbytes=0), dict(nbytes=-1), dict(nbytes=int(plan[2]) // 3),
                dict(sn=-1), dict(sc=-9), dict(sy=-3), dict(sx=-1),
                dict(slices=0), dict(slices=-1), dict(slices=nk + 1), dict(slices=1 << 30),
                dict(slices=nk - 1),                                 # in range, but not a count the plan returns: T = 2 needs 9 slices
                dict(d=0), dict(d=-1),
                dict(cin=64), dict(cout=64), dict(cin=144), dict(cout=192), dict(cin=0), dict(cout=-128),
                dict(B=0), dict(H=0), dict(W=-1)):
        assert call(**bad) == 0, bad
    assert nk == 18 and -(-nk // 2) == 9


def _plan(lib, *args):
    plan = (ctypes.c_int64 * 3)(-1, -1, -1)
    assert lib.skd_conv3x3_split_wgrad_plan(*args, ctypes.cast(plan, ctypes.c_void_p)) == 1, args
    return int(plan[0]), int(plan[1]), int(plan[2])


def _auto_slices(tiles, slots, nk):
    """The rule of include/skd_wgrad.h for slices == 0: fewest rounds-of-the-device x K-tiles-per-slice, at most two rounds' worth
    of workgroups, the smaller count on a tie."""
    most = min(max(1, 2 * slots // tiles), nk)
    return min(range(1, most + 1), key=lambda s: (-(-tiles * s // slots) * -(-nk // s), s))


def test_wgrad_plan_sweep():
    lib = _lib.load()
    assert len(CHANNEL_PAIRS) == 7
    seen_many = False
    for b in (1, 2, 8):
        for h, w in ((3, 3), (5, 7), (13, 11), (33, 33), (65, 65)):
            nk = -(-b * h * w // 16)
            for cin, cout in CHANNEL_PAIRS:
                tiles = 9 * (cin // 128) * (cout // 128)
                for cus in (0, 64, 256, 304):
                    for slices in (0, 1, 2, 3, nk, nk + 5):
                        s, t, nbytes = _plan(lib, b, h, w, cin, cout, slices, cus)
                        what = (b, h, w, cin, cout, slices, cus, s, t)
                        assert 1 <= s <= nk, what
                        assert s * t >= nk and (s - 1) * t < nk, what          # an exact cover, no slice empty
                        assert nbytes == s * 9 * cin * cout * 4, what
                        # what was asked for, made an exact cover; the automatic rule of include/skd_wgrad.h
                        asked = min(slices, nk) if slices else _auto_slices(tiles, 2 * (cus or 256), nk)
                        assert t == -(-nk // asked) and s == -(-nk // t), what
                        seen_many |= slices == 0 and s > 8
    assert seen_many
    # the geometry does not depend on the device when the count is given, and 0 compute units means 256
    assert _plan(lib, 8, 65, 65, 128, 128, 7, 64) == _plan(lib, 8, 65, 65, 128, 128, 7, 304)
    assert _plan(lib, 8, 65, 65, 512, 512, 0, 0) == _plan(lib, 8, 65, 65, 512, 512, 0, 256)
    # the student's step on 256 compute units: one full round where a round is reachable, two for 512 -> 512
    assert [_plan(lib, 8, 65, 65, cin, cout, 0, 256)[0] for cin, cout in ((128, 128), (128, 256), (256, 256), (256, 512), (512, 512))] \
        == [56, 28, 14, 7, 7]
    plan = (ctypes.c_int64 * 3)()
    ptr = ctypes.cast(plan, ctypes.c_void_p)
    for bad in ((0, 5, 5, 128, 128, 0, 0), (1, 0, 5, 128, 128, 0, 0), (1, 5, 0, 128, 128, 0, 0), (1, 5, 5, 64, 128, 0, 0),
                (1, 5, 5, 128, 192, 0, 0), (1, 5, 5, 128, 128, -1, 0), (1, 5, 5, 128, 128, 0, -1), (1 << 10, 1 << 10, 1 << 10, 128, 128, 0, 0)):
        assert lib.skd_conv3x3_split_wgrad_plan(*bad, ptr) == 0, bad
    assert lib.skd_conv3x3_split_wgrad_plan(1, 5, 5, 128, 128, 0, 0, None) == 0


# ---- 2. routing and wiring ----------------------------------------------------------------------------------------------------

def test_flagged_student_routes_thirteen_weight_gradients(computing):
    net, x = _student(), _input()
    plain_out, want = _step(net, x)
    assert computing.calls == [] and computing.wgrads == []

    # split_train alone: forward and data gradient on the core, no weight-gradient launch
    first = networks.route_training_convs(copy.deepcopy(net))
    assert all(m._skd_train_wgrad is False for m in first.modules() if isinstance(m, (PC.BasicBlock, PC.ResNet, PC.PSPModule)))
    _step(first, x)
    assert len(computing.calls) == 26 and computing.wgrads == []

    flagged = networks.route_training_convs(copy.deepcopy(net), wgrad=True)
    marks = [m._skd_train_wgrad for m in flagged.modules() if isinstance(m, (PC.BasicBlock, PC.ResNet, PC.PSPModule))]
    assert marks == [True] * 10 and isinstance(PC.WGRAD_ROUTING_EXCLUDED, frozenset)
    computing.calls.clear()
    got_out, got = _step(flagged, x)
    assert len(computing.calls) == 26
    assert [(c["cin"], c["cout"], c["dilation"]) for c in computing.wgrads][::-1] == ROUTED and len(computing.wgrads) == 13
    rel = lambda a, b: float((a.detach() - b.detach()).abs().max() / b.detach().abs().max())
    for a, b in zip(got_out, plain_out):
        assert rel(a, b) <= 1e-6, rel(a, b)
    assert set(got) == set(want) and all(g is not None for g in got.values())
    worst = max((rel(got[k], want[k]), k) for k in want)
    print("worst gradient: %.3e %s" % worst)
    for k in want:
        assert rel(got[k], want[k]) <= 1e-6, (k, rel(got[k], want[k]))
    # the PSP half: the gradient of the channel slice reached the full weight through autograd, beside the priors' half
    wb = got["pspmodule.bottleneck.0.weight"]
    assert float(wb[:, :512].abs().max()) > 0 and float(wb[:, 512:].abs().max()) > 0
    assert computing.wgrads[0]["cin"] == 512 and computing.wgrads[0]["cout"] == 128
    # the result has the weight's own layout (the student's weights are channels-last); the slice gets a channels-last one
    for c in computing.wgrads[1:]:
        assert c["strides"] == (9 * c["cin"], 1, 3 * c["cin"], c["cin"]), c
    assert computing.wgrads[0]["strides"] == (9 * 512, 1, 3 * 512, 512)
    assert float(got["dsn.0.bias"].abs().max()) > 0                 # the bias gradient is still the library's

    # eval mode and no_grad: no backward, nothing launched; an excluded shape keeps the library for its weight gradient only
    computing.wgrads.clear()
    flagged.eval()
    flagged(x)
    flagged.train()
    with torch.no_grad():
        flagged(x)
    assert computing.wgrads == []
    try:
        PC.WGRAD_ROUTING_EXCLUDED = frozenset({(512, 512, 4), (512, 128, 1)})
        computing.calls.clear()
        flagged.zero_grad(set_to_none=True)
        _, part = _step(flagged, x)
    finally:
        PC.WGRAD_ROUTING_EXCLUDED = frozenset()
    assert [(c["cin"], c["cout"], c["dilation"]) for c in computing.wgrads][::-1] == [r for r in ROUTED if r[0] != 512]
    assert len(computing.calls) == 26
    for k in want:
        assert rel(part[k], want[k]) <= 1e-6, k
    # wgrad=False again, and enable=False: the flag is cleared
    computing.wgrads.clear()
    networks.route_training_convs(flagged)
    _step(flagged, x)
    assert computing.wgrads == []
    networks.route_training_convs(flagged, enable=False, wgrad=True)
    assert not any(m._skd_train_wgrad for m in flagged.modules() if isinstance(m, (PC.BasicBlock, PC.ResNet, PC.PSPModule)))


def test_backend_without_the_entries_falls_back_silently():
    """TrainDouble has the training entries and not those of skd_wgrad.h: a student flagged with ``wgrad=True`` takes its weight
    gradients from the library, and nothing raises."""
    d = TrainDouble(cref.load(_lib.SIGNATURES), compute=True)
    _lib.install_test_backend(d)
    try:
        assert not any(_lib.has_entry(n) for n in (SUPPORTED, PLAN, RUN))
        net, x = _student(), _input()
        _, want = _step(networks.route_training_convs(copy.deepcopy(net)), x)
        n = len(d.calls)
        _, got = _step(networks.route_training_convs(copy.deepcopy(net), wgrad=True), x)
        assert len(d.calls) == 2 * n == 52
        assert all(torch.equal(got[k], want[k]) for k in want)
        xs = torch.zeros(1, 128, 2, 2).contiguous(memory_format=torch.channels_last)
        assert SF.conv3x3_train_supported(xs, torch.zeros(128, 128, 3, 3), 1, 1, 1, 1)
        assert not SF.conv3x3_wgrad_supported(xs, torch.zeros(128, 128, 3, 3), 1, 1, 1, 1)
    finally:
        _lib.install_test_backend(None)


def test_op_honours_needs_input_grad_and_layouts(computing):
    torch.manual_seed(2)
    conv = torch.nn.Conv2d(128, 128, 3, 1, 2, 2, bias=True).to(memory_format=torch.channels_last)
    x = torch.randn(2, 128, 5, 6).contiguous(memory_format=torch.channels_last)
    assert SF.conv3x3_wgrad_supported(x, conv.weight, 1, 2, 2, 1)
    assert not SF.conv3x3_wgrad_supported(x, conv.weight, 2, 2, 2, 1) and not SF.conv3x3_wgrad_supported(x.contiguous(), conv.weight, 1, 2, 2, 1)
    with torch.no_grad():
        assert not SF.conv3x3_wgrad_supported(x, conv.weight, 1, 2, 2, 1)
    want = torch.autograd.grad(torch.nn.functional.conv2d(x, conv.weight, conv.bias, 1, 2, 2).sum(), (conv.weight, conv.bias))
    y = SF.conv3x3_split_train(x, conv.weight, 2, conv.bias, owner=conv, wgrad=True)
    y.sum().backward()
    assert len(computing.wgrads) == 1 and len(computing.calls) == 1            # x needs no gradient: no data-gradient launch
    assert float((conv.weight.grad - want[0]).abs().max()) <= 1e-6 * float(want[0].abs().max())
    assert float((conv.bias.grad - want[1]).abs().max()) <= 1e-6 * float(want[1].abs().max())
    # only dx asked (the weight needs no gradient): no weight-gradient launch
    xg = x.clone().requires_grad_(True)
    y = SF.conv3x3_split_train(xg, conv.weight.detach(), 2, conv.bias.detach(), owner=conv, wgrad=True)
    torch.autograd.grad(y.sum(), xg)
    assert len(computing.wgrads) == 1 and len(computing.calls) == 3
    # a weight written between forward and backward: autograd's version error, as without the flag
    y = SF.conv3x3_split_train(xg, conv.weight, 2, conv.bias, owner=conv, wgrad=True)
    with torch.no_grad():
        conv.weight.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.sum().backward()
    # the layouts of the result: the weight's own when it is dense (contiguous here), channels-last for a slice
    g = torch.randn(2, 128, 5, 6).contiguous(memory_format=torch.channels_last)
    for like, strides in ((torch.empty(128, 128, 3, 3), (1152, 9, 3, 1)),
                          (torch.empty(128, 128, 3, 3).contiguous(memory_format=torch.channels_last), (1152, 1, 384, 128)),
                          (torch.empty(128, 192, 3, 3)[:, 64:], (1152, 1, 384, 128))):
        dw = SF.conv3x3_split_wgrad(x, g, like, 2)
        assert tuple(dw.stride()) == strides and computing.wgrads[-1]["strides"] == strides
        ref = torch.nn.grad.conv2d_weight(x, (128, 128, 3, 3), g, 1, 2, 2)
        assert float((dw - ref).abs().max()) <= 1e-6 * float(ref.abs().max())
    with pytest.raises(ValueError):
        SF.conv3x3_split_wgrad(x, g, torch.empty(128, 256, 3, 3), 2)


# ---- 3. NetModel ----------------------------------------------------------------------------------------------------------------

def test_netmodel_split_wgrad_switch(monkeypatch):
    from structure_knowledge_distillation_amd.networks.kd_model import NetModel, default_args
    monkeypatch.delenv("SKD_SPLIT_TRAIN", raising=False)
    monkeypatch.delenv("SKD_SPLIT_WGRAD", raising=False)
    assert default_args().split_wgrad is False
    monkeypatch.setenv("SKD_SPLIT_WGRAD", "1")
    assert default_args().split_wgrad is True and default_args(split_wgrad=False).split_wgrad is False
    assert default_args().split_train is False                      # the two switches are read separately
    monkeypatch.setenv("SKD_SPLIT_WGRAD", "0")
    assert default_args().split_wgrad is False and default_args(split_wgrad=True).split_wgrad is True
    _lib.install_test_backend(cref.load(_lib.SIGNATURES))
    try:
        kw = dict(device=torch.device("cpu"), batch_size=2, ho=False)
        mods = lambda model: [m for m in model.student.modules() if isinstance(m, (PC.BasicBlock, PC.ResNet, PC.PSPModule))]
        flags = lambda model: [(getattr(m, "_skd_train_min_cin", None), getattr(m, "_skd_train_wgrad", False)) for m in mods(model)]
        model = NetModel(default_args(**kw))
        assert flags(model) == [(None, False)] * 10 and not model.split_wgrad
        # split_wgrad without split_train routes nothing
        model = NetModel(default_args(split_wgrad=True, **kw))
        assert flags(model) == [(None, False)] * 10 and not model.split_wgrad and not model.split_train
        model = NetModel(default_args(split_train=True, **kw))
        assert flags(model) == [(PC.TRAIN_SPLIT_MIN_CIN, False)] * 10 and not model.split_wgrad
        model = NetModel(default_args(split_train=True, split_wgrad=True, **kw))
        assert flags(model) == [(PC.TRAIN_SPLIT_MIN_CIN, True)] * 10 and model.split_wgrad and model.split_train
        monkeypatch.setenv("SKD_SPLIT_WGRAD", "1")
        assert flags(NetModel(default_args(**kw))) == [(None, False)] * 10
        monkeypatch.setenv("SKD_SPLIT_TRAIN", "1")
        assert flags(NetModel(default_args(**kw))) == [(PC.TRAIN_SPLIT_MIN_CIN, True)] * 10
        assert not any(getattr(m, "_skd_train_wgrad", False) for m in model.teacher.modules())
    finally:
        _lib.install_test_backend(None)
