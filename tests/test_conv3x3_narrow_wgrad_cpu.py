"""The weight gradient of the student's 64-channel 3x3 convolutions on the split core, the parts that need no GPU: the C ABI of
include/skd_narrow_wgrad.h (the pinned names and argument lists, the truth table of the predicate, the host-side refusals of
the launch entry, the split-K plan swept over sizes), the routing and the wiring of a student flagged with ``narrow_wgrad=True`` (a
torch-implemented double: NarrowDouble + WgradDouble + the three new entries, the weight gradient computed by
``torch.nn.grad.conv2d_weight``) and NetModel's ``split_narrow_wgrad`` switch."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import structure_knowledge_distillation_amd.networks.pspnet_combine as PC
from oracle import cref
from structure_knowledge_distillation_amd import _lib, functional as SF
from structure_knowledge_distillation_amd import networks
from test_conv3x3_narrow_cpu import NarrowDouble
from test_conv3x3_train_cpu import ROUTED, _input, _step, _student
from test_conv3x3_wgrad_cpu import WgradDouble
from test_student_infer_cpu import _host

SUPPORTED, PLAN, RUN = "skd_conv3x3_narrow_wgrad_supported", "skd_conv3x3_narrow_wgrad_plan", "skd_conv3x3_narrow_wgrad_nhwc"
# the student's six, in the order of the forward: stem conv2, conv3, layer1.0.conv1, layer1.0.conv2, layer1.1
NARROW_ROUTED = [(64, 64, 1), (64, 128, 1), (128, 64, 1)] + [(64, 64, 1)] * 3
CHANNEL_PAIRS = [(64, 64), (64, 128), (128, 64), (192, 64), (64, 192), (128, 128), (128, 256)]
FLAGGED = (PC.BasicBlock, PC.ResNet, PC.PSPModule)


class BothDouble(NarrowDouble, WgradDouble):
    """The entries of skd_train.h, skd_narrow.h and skd_wgrad.h, and not those of skd_narrow_wgrad.h."""


class NarrowWgradDouble(BothDouble):
    """BothDouble + the three entries of skd_narrow_wgrad.h on raw HOST addresses, in the manner of WgradDouble: the plan is one
    slice, the launch entry is ``torch.nn.grad.conv2d_weight`` written through the destination's strides.  Every launch is recorded."""

    def __init__(self, core, compute):
        super().__init__(core, compute)
        self.narrow_wgrads = []

    def skd_conv3x3_narrow_wgrad_supported(self, cin, cout, stride, padding, dilation, groups):
        return int(cin > 0 and cout > 0 and cin % 64 == 0 and cout % 64 == 0 and stride == 1 and dilation >= 1
                   and padding == dilation and groups == 1)

    def skd_conv3x3_narrow_wgrad_plan(self, B, H, W, cin, cout, slices, cus, plan):
        out = ctypes.cast(plan, ctypes.POINTER(ctypes.c_int64))
        out[0], out[1], out[2] = 1, -(-B * H * W // 16), 9 * cin * cout * 4
        return 1

    def skd_conv3x3_narrow_wgrad_nhwc(self, B, H, W, cin, cout, dil, x, g, dw, sn, sc, sy, sx, ws, ws_bytes, slices, stream):
        assert ws and ws_bytes == 9 * cin * cout * 4 and slices == 1
        self.narrow_wgrads.append(dict(cin=cin, cout=cout, dilation=dil, x=x, dw=dw, strides=(sn, sc, sy, sx)))
        xt = torch.from_numpy(_host(x, (B, H, W, cin)).copy()).permute(0, 3, 1, 2)
        gt = torch.from_numpy(_host(g, (B, H, W, cout)).copy()).permute(0, 3, 1, 2)
        grad = torch.nn.grad.conv2d_weight(xt, (cout, cin, 3, 3), gt, 1, dil, dil)
        base = _host(dw, (1 + (cout - 1) * sn + (cin - 1) * sc + 2 * sy + 2 * sx,))
        np.lib.stride_tricks.as_strided(base, shape=(cout, cin, 3, 3), strides=tuple(4 * s for s in (sn, sc, sy, sx)))[...] = grad.numpy()
        return 1


@pytest.fixture
def computing():
    d = NarrowWgradDouble(cref.load(_lib.SIGNATURES), compute=True)
    _lib.install_test_backend(d)
    yield d
    _lib.install_test_backend(None)


# ---- 1. the C ABI ------------------------------------------------------------------------------------------------------------

def test_narrow_wgrad_header_table_and_library_agree():
    """What is particular to skd_narrow_wgrad.h; header <-> table <-> library <-> build digest: tests/test_abi.py, for every header."""
    table = _lib.ABI["skd_narrow_wgrad.h"]
    assert sorted(table) == sorted([SUPPORTED, PLAN, RUN]) and len(table) == 3
    # the two tables the neighbouring tests pin have not grown
    assert len(_lib.ABI["skd_wgrad.h"]) == 3 and len(_lib.ABI["skd_narrow.h"]) == 4
    # the argument lists of the wide entries
    for new, old in zip((SUPPORTED, PLAN, RUN), ("skd_conv3x3_split_wgrad_supported", "skd_conv3x3_split_wgrad_plan",
                                                 "skd_conv3x3_split_wgrad_nhwc")):
        assert table[new] == _lib.ABI["skd_wgrad.h"][old]


def test_narrow_wgrad_supported_truth_table():
    lib = _lib.load()
    sup, wide = lib.skd_conv3x3_narrow_wgrad_supported, lib.skd_conv3x3_split_wgrad_supported
    for cin, cout in CHANNEL_PAIRS + [(512, 64), (320, 448)]:
        for d in (1, 2, 4):
            assert sup(cin, cout, 1, d, d, 1) == 1, (cin, cout, d)
    for bad in ((32, 64, 1, 1, 1, 1), (64, 32, 1, 1, 1, 1), (96, 64, 1, 1, 1, 1), (64, 96, 1, 1, 1, 1), (16, 64, 1, 1, 1, 1),
                (0, 64, 1, 1, 1, 1), (64, 0, 1, 1, 1, 1), (-64, 64, 1, 1, 1, 1), (64, -64, 1, 1, 1, 1),
                (64, 64, 2, 1, 1, 1), (64, 64, 1, 1, 2, 1), (64, 64, 1, 2, 1, 1), (64, 64, 1, 0, 0, 1), (64, 64, 1, 1, 1, 2)):
        assert sup(*bad) == 0, bad
    # over a grid: the wide predicate with 64 in the place of 128 -- and the wide one keeps refusing a 64-channel side
    for cin in (0, 16, 64, 128, 144, 192, 256):
        for cout in (0, 32, 64, 128, 192, 512):
            for s, p, d, g in ((1, 1, 1, 1), (2, 1, 1, 1), (1, 2, 2, 1), (1, 1, 2, 1), (1, 0, 0, 1), (1, 1, 1, 2)):
                want = int(cin > 0 and cout > 0 and cin % 64 == 0 and cout % 64 == 0 and s == 1 and d >= 1 and p == d and g == 1)
                assert sup(cin, cout, s, p, d, g) == want, (cin, cout, s, p, d, g)
                assert wide(cin, cout, s, p, d, g) == int(want and cin % 128 == 0 and cout % 128 == 0)


def test_narrow_wgrad_launch_host_side_refusals():
    """Every refusal is decided on the host, in front of the launches: no device is touched (the pointers are never followed)."""
    lib = _lib.load()
    X, G, DW, WS = 0x10000, 0x2000000, 0x4000000, 0x8000000
    b, h, w, c = 2, 13, 11, 64
    nk = -(-b * h * w // 16)
    plan = (ctypes.c_int64 * 3)()
    assert lib.skd_conv3x3_narrow_wgrad_plan(b, h, w, c, c, 3, 0, ctypes.cast(plan, ctypes.c_void_p)) == 1 and plan[0] == 3
    ok = dict(B=b, H=h, W=w, cin=c, cout=c, d=1, x=X, g=G, dw=DW, sn=9 * c, sc=9, sy=3, sx=1, ws=WS, nbytes=int(plan[2]), slices=3)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.skd_conv3x3_narrow_wgrad_nhwc(a["B"], a["H"], a["W"], a["cin"], a["cout"], a["d"], a["x"], a["g"], a["dw"], a["sn"],
                                                 a["sc"], a["sy"], a["sx"], a["ws"], a["nbytes"], a["slices"], None)
    for bad in (dict(x=None), dict(g=None), dict(dw=None), dict(ws=None),
                dict(x=X + 4), dict(x=X + 8), dict(g=G + 4), dict(g=G + 8), dict(ws=WS + 4), dict(ws=WS + 8),
                dict(nbytes=int(plan[2]) - 1), dict(nbytes=0), dict(nbytes=-1), dict(nbytes=int(plan[2]) // 3),
                dict(sn=-1), dict(sc=-9), dict(sy=-3), dict(sx=-1),
                dict(slices=0), dict(slices=-1), dict(slices=nk + 1), dict(slices=1 << 30),
                dict(slices=nk - 1),                                 # in range, but not a count the plan returns: T = 2 needs 9 slices
                dict(d=0), dict(d=-1), dict(d=(1 << 24) + 1),
                dict(cin=32), dict(cout=32), dict(cin=96), dict(cout=160), dict(cin=0), dict(cout=-64),
                dict(B=0), dict(H=0), dict(W=-1),
                dict(B=1 << 10, H=1 << 10, W=1 << 10, slices=1, nbytes=1 << 62)):          # P = 2^30
        assert call(**bad) == 0, bad
    assert nk == 18 and -(-nk // 2) == 9


def _plan(lib, *args):
    plan = (ctypes.c_int64 * 3)(-1, -1, -1)
    assert lib.skd_conv3x3_narrow_wgrad_plan(*args, ctypes.cast(plan, ctypes.c_void_p)) == 1, args
    return int(plan[0]), int(plan[1]), int(plan[2])


def _tiles(cin, cout):
    """Workgroups of one slice: the 9 Cin / 64 units two to a tile, times the column tiles of 64."""
    return -(-(9 * cin // 64) // 2) * (cout // 64)


def _auto_slices(tiles, slots, nk):
    """The rule of include/skd_narrow_wgrad.h for slices == 0: fewest rounds-of-the-device x K-tiles-per-slice, at most ONE
    round's worth of workgroups, the smaller count on a tie."""
    most = min(max(1, slots // tiles), nk)
    return min(range(1, most + 1), key=lambda s: (-(-tiles * s // slots) * -(-nk // s), s))


def test_narrow_wgrad_plan_sweep():
    lib = _lib.load()
    assert [_tiles(*p) for p in CHANNEL_PAIRS] == [5, 10, 9, 14, 15, 18, 36]
    seen_many = False
    for b, h, w in ((1, 3, 3), (1, 5, 7), (2, 13, 11), (8, 33, 33), (8, 129, 129), (8, 256, 256)):
        nk = -(-b * h * w // 16)
        for cin, cout in CHANNEL_PAIRS:
            tiles = _tiles(cin, cout)
            for cus in (0, 64, 256, 304):
                for slices in (0, 1, 2, 3, nk, nk + 5):
                    s, t, nbytes = _plan(lib, b, h, w, cin, cout, slices, cus)
                    what = (b, h, w, cin, cout, slices, cus, s, t)
                    assert 1 <= s <= nk, what
                    assert s * t >= nk and (s - 1) * t < nk, what          # an exact cover, no slice empty
                    assert nbytes == s * 9 * cin * cout * 4, what
                    # what was asked for, made an exact cover; the automatic rule of include/skd_narrow_wgrad.h
                    asked = min(slices, nk) if slices else _auto_slices(tiles, 3 * (cus or 256), nk)
                    assert t == -(-nk // asked) and s == -(-nk // t), what
                    if not slices:
                        assert tiles * s <= max(tiles, 3 * (cus or 256)), what      # one round of the device
                    seen_many |= slices == 0 and s > 100
    assert seen_many
    # the geometry does not depend on the device when the count is given, and 0 compute units means 256
    assert _plan(lib, 8, 129, 129, 64, 64, 7, 64) == _plan(lib, 8, 129, 129, 64, 64, 7, 304)
    assert _plan(lib, 8, 256, 256, 64, 128, 0, 0) == _plan(lib, 8, 256, 256, 64, 128, 0, 256)
    # the student's step on 256 compute units (768 places): one full round each
    assert _plan(lib, 8, 256, 256, 64, 64, 0, 256)[:2] == (153, 215) and _plan(lib, 8, 256, 256, 64, 128, 0, 256)[0] == 76
    assert _plan(lib, 8, 129, 129, 128, 64, 0, 256)[0] == 85 and _plan(lib, 8, 129, 129, 64, 64, 0, 256)[0] == 152
    plan = (ctypes.c_int64 * 3)()
    ptr = ctypes.cast(plan, ctypes.c_void_p)
    for bad in ((0, 5, 5, 64, 64, 0, 0), (1, 0, 5, 64, 64, 0, 0), (1, 5, 0, 64, 64, 0, 0), (1, 5, 5, 32, 64, 0, 0),
                (1, 5, 5, 64, 96, 0, 0), (1, 5, 5, 64, 64, -1, 0), (1, 5, 5, 64, 64, 0, -1), (1 << 10, 1 << 10, 1 << 10, 64, 64, 0, 0)):
        assert lib.skd_conv3x3_narrow_wgrad_plan(*bad, ptr) == 0, bad
    assert lib.skd_conv3x3_narrow_wgrad_plan(1, 5, 5, 64, 64, 0, 0, None) == 0
    # the wide plan is what it was: two rounds allowed, 128-row tiles
    wide = (ctypes.c_int64 * 3)()
    assert lib.skd_conv3x3_split_wgrad_plan(8, 65, 65, 512, 512, 0, 256, ctypes.cast(wide, ctypes.c_void_p)) == 1 and wide[0] == 7
    assert lib.skd_conv3x3_split_wgrad_plan(8, 65, 65, 64, 128, 0, 256, ctypes.cast(wide, ctypes.c_void_p)) == 0


# ---- 2. routing and wiring ----------------------------------------------------------------------------------------------------

def _marks(net, attr):
    return [getattr(m, attr, False) for m in net.modules() if isinstance(m, FLAGGED)]


def test_flagged_student_routes_six_narrow_weight_gradients(computing, monkeypatch):
    # the mechanism, with the policy emptied (test_committed_exclusions_follow_the_isolated_table has the policy)
    monkeypatch.setattr(PC, "NARROW_WGRAD_ROUTING_EXCLUDED", frozenset())
    net, x = _student(), _input()
    plain_out, want = _step(net, x)
    assert computing.calls == [] and computing.wgrads == [] and computing.narrow_wgrads == []

    # split_train + narrow without the new flag: no weight-gradient launch of either kind
    first = networks.route_training_convs(copy.deepcopy(net), narrow=True)
    assert _marks(first, "_skd_train_narrow_wgrad") == [False] * 10
    _step(first, x)
    assert len(computing.calls) == 38 and computing.wgrads == [] and computing.narrow_wgrads == []

    flagged = networks.route_training_convs(copy.deepcopy(net), narrow=True, narrow_wgrad=True)
    assert _marks(flagged, "_skd_train_narrow_wgrad") == [True] * 10 and _marks(flagged, "_skd_train_wgrad") == [False] * 10
    assert isinstance(PC.NARROW_WGRAD_ROUTING_EXCLUDED, frozenset)
    computing.calls.clear()
    got_out, got = _step(flagged, x)
    assert len(computing.calls) == 38 and computing.wgrads == []
    assert [(c["cin"], c["cout"], c["dilation"]) for c in computing.narrow_wgrads][::-1] == NARROW_ROUTED
    rel = lambda a, b: float((a.detach() - b.detach()).abs().max() / b.detach().abs().max())
    for a, b in zip(got_out, plain_out):
        assert rel(a, b) <= 1e-6, rel(a, b)
    assert set(got) == set(want) and all(g is not None for g in got.values())
    worst = max((rel(got[k], want[k]), k) for k in want)
    print("worst gradient: %.3e %s" % worst)
    for k in want:
        assert rel(got[k], want[k]) <= 1e-6, (k, rel(got[k], want[k]))
    # the result has the weight's own layout (the student's weights are channels-last)
    for c in computing.narrow_wgrads:
        assert c["strides"] == (9 * c["cin"], 1, 3 * c["cin"], c["cin"]), c

    # with split_wgrad on as well: 13 wide calls plus the six narrow ones and no more
    both = networks.route_training_convs(copy.deepcopy(net), wgrad=True, narrow=True, narrow_wgrad=True)
    computing.calls.clear()
    computing.narrow_wgrads.clear()
    _, got_both = _step(both, x)
    assert len(computing.calls) == 38
    assert [(c["cin"], c["cout"], c["dilation"]) for c in computing.wgrads][::-1] == ROUTED and len(computing.wgrads) == 13
    assert [(c["cin"], c["cout"], c["dilation"]) for c in computing.narrow_wgrads][::-1] == NARROW_ROUTED
    for k in want:
        assert rel(got_both[k], want[k]) <= 1e-6, (k, rel(got_both[k], want[k]))

    # eval mode and no_grad: no backward, nothing launched
    computing.narrow_wgrads.clear()
    flagged.eval()
    flagged(x)
    flagged.train()
    with torch.no_grad():
        flagged(x)
    assert computing.narrow_wgrads == []
    # an excluded shape keeps the library for its weight gradient only
    monkeypatch.setattr(PC, "NARROW_WGRAD_ROUTING_EXCLUDED", frozenset({(64, 64, 1)}))
    computing.calls.clear()
    flagged.zero_grad(set_to_none=True)
    _, part = _step(flagged, x)
    monkeypatch.setattr(PC, "NARROW_WGRAD_ROUTING_EXCLUDED", frozenset())
    assert [(c["cin"], c["cout"]) for c in computing.narrow_wgrads][::-1] == [(64, 128), (128, 64)]
    assert len(computing.calls) == 38
    for k in want:
        assert rel(part[k], want[k]) <= 1e-6, k
    # the flag without ``narrow`` routes nothing; narrow_wgrad=False again, and enable=False: the flag is cleared
    computing.narrow_wgrads.clear()
    alone = networks.route_training_convs(copy.deepcopy(net), narrow_wgrad=True)
    _step(alone, x)
    networks.route_training_convs(flagged, narrow=True)
    _step(flagged, x)
    assert computing.narrow_wgrads == []
    networks.route_training_convs(flagged, enable=False, narrow=True, narrow_wgrad=True)
    assert not any(_marks(flagged, "_skd_train_narrow_wgrad"))


def test_committed_exclusions_follow_the_isolated_table(computing):
    """profiles/r23_conv3x3_narrow_wgrad_isolated.md: every one of the step's shapes measures behind the library, so the committed
    policy routes none of them -- the switch is wired and, until a shape measures ahead, changes nothing in the student's step."""
    assert PC.NARROW_WGRAD_ROUTING_EXCLUDED == frozenset({(64, 64, 1), (64, 128, 1), (128, 64, 1)}) == frozenset(NARROW_ROUTED)
    net, x = _student(), _input()
    _step(networks.route_training_convs(copy.deepcopy(net), narrow=True, narrow_wgrad=True), x)
    assert computing.narrow_wgrads == [] and len(computing.calls) == 38


def test_backend_without_the_entries_keeps_the_library():
    """BothDouble has every entry but those of skd_narrow_wgrad.h: a student flagged with ``narrow_wgrad=True`` takes the six
    weight gradients from the library, and nothing raises."""
    d = BothDouble(cref.load(_lib.SIGNATURES), compute=True)
    _lib.install_test_backend(d)
    try:
        assert not any(_lib.has_entry(n) for n in (SUPPORTED, PLAN, RUN))
        net, x = _student(), _input()
        _, want = _step(networks.route_training_convs(copy.deepcopy(net), wgrad=True, narrow=True), x)
        n, nw = len(d.calls), len(d.wgrads)
        _, got = _step(networks.route_training_convs(copy.deepcopy(net), wgrad=True, narrow=True, narrow_wgrad=True), x)
        assert len(d.calls) == 2 * n == 76 and len(d.wgrads) == 2 * nw == 26
        assert all(torch.equal(got[k], want[k]) for k in want)
        xs = torch.zeros(1, 64, 2, 2).contiguous(memory_format=torch.channels_last)
        assert SF.conv3x3_narrow_train_supported(xs, torch.zeros(64, 64, 3, 3, requires_grad=True), 1, 1, 1, 1)
        assert not SF.conv3x3_narrow_wgrad_supported(xs, torch.zeros(64, 64, 3, 3, requires_grad=True), 1, 1, 1, 1)
    finally:
        _lib.install_test_backend(None)


@pytest.mark.parametrize("cin,cout", [(64, 64), (64, 128), (128, 64)])
def test_op_honours_needs_input_grad_and_layouts(computing, cin, cout):
    torch.manual_seed(2)
    conv = torch.nn.Conv2d(cin, cout, 3, 1, 2, 2, bias=True).to(memory_format=torch.channels_last)
    x = torch.randn(2, cin, 5, 6).contiguous(memory_format=torch.channels_last)
    assert SF.conv3x3_narrow_wgrad_supported(x, conv.weight, 1, 2, 2, 1)
    assert not SF.conv3x3_narrow_wgrad_supported(x, conv.weight, 2, 2, 2, 1)
    assert not SF.conv3x3_narrow_wgrad_supported(x.contiguous(), conv.weight, 1, 2, 2, 1)
    with torch.no_grad():
        assert not SF.conv3x3_narrow_wgrad_supported(x, conv.weight, 1, 2, 2, 1)
    want = torch.autograd.grad(torch.nn.functional.conv2d(x, conv.weight, conv.bias, 1, 2, 2).sum(), (conv.weight, conv.bias))
    # ``wgrad=True`` keeps being ignored for a narrow shape, with or without ``narrow``'s own flag off
    y = SF.conv3x3_split_train(x, conv.weight, 2, conv.bias, owner=conv, wgrad=True, narrow=True)
    y.sum().backward()
    assert computing.narrow_wgrads == [] and computing.wgrads == []
    conv.zero_grad(set_to_none=True)
    y = SF.conv3x3_split_train(x, conv.weight, 2, conv.bias, owner=conv, narrow=True, narrow_wgrad=True)
    y.sum().backward()
    assert len(computing.narrow_wgrads) == 1 and computing.wgrads == [] and len(computing.calls) == 2   # x needs no gradient
    assert float((conv.weight.grad - want[0]).abs().max()) <= 1e-6 * float(want[0].abs().max())
    assert float((conv.bias.grad - want[1]).abs().max()) <= 1e-6 * float(want[1].abs().max())
    # only dx asked (the weight needs no gradient): no weight-gradient launch
    xg = x.clone().requires_grad_(True)
    y = SF.conv3x3_split_train(xg, conv.weight.detach(), 2, conv.bias.detach(), owner=conv, narrow=True, narrow_wgrad=True)
    torch.autograd.grad(y.sum(), xg)
    assert len(computing.narrow_wgrads) == 1 and len(computing.calls) == 4
    # a weight written between forward and backward: autograd's version error, as without the flag
    y = SF.conv3x3_split_train(xg, conv.weight, 2, conv.bias, owner=conv, narrow=True, narrow_wgrad=True)
    with torch.no_grad():
        conv.weight.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.sum().backward()
    # the layouts of the result: the weight's own when it is dense (contiguous here), channels-last for a slice
    g = torch.randn(2, cout, 5, 6).contiguous(memory_format=torch.channels_last)
    for like, strides in ((torch.empty(cout, cin, 3, 3), (9 * cin, 9, 3, 1)),
                          (torch.empty(cout, cin, 3, 3).contiguous(memory_format=torch.channels_last), (9 * cin, 1, 3 * cin, cin)),
                          (torch.empty(cout, cin + 64, 3, 3)[:, 64:], (9 * cin, 1, 3 * cin, cin))):
        dw = SF.conv3x3_narrow_wgrad(x, g, like, 2)
        assert tuple(dw.stride()) == strides and computing.narrow_wgrads[-1]["strides"] == strides
        ref = torch.nn.grad.conv2d_weight(x, (cout, cin, 3, 3), g, 1, 2, 2)
        assert float((dw - ref).abs().max()) <= 1e-6 * float(ref.abs().max())
    with pytest.raises(ValueError):
        SF.conv3x3_narrow_wgrad(x, g, torch.empty(cout, 2 * cin, 3, 3), 2)
    # both multiples of 128: ``narrow_wgrad`` is about the shapes ``narrow`` is about; the wide op keeps its own flag
    computing.wgrads.clear()
    n = len(computing.narrow_wgrads)
    w2 = (torch.randn(128, 128, 3, 3) * 0.05).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    x2 = torch.randn(1, 128, 4, 4).contiguous(memory_format=torch.channels_last)
    SF.conv3x3_split_train(x2, w2, 1, None, torch.nn.Module(), narrow=True, narrow_wgrad=True).sum().backward()
    assert len(computing.narrow_wgrads) == n and computing.wgrads == []
    SF.conv3x3_split_train(x2, w2, 1, None, torch.nn.Module(), wgrad=True, narrow=True, narrow_wgrad=True).sum().backward()
    assert len(computing.narrow_wgrads) == n and len(computing.wgrads) == 1


# ---- 3. NetModel ----------------------------------------------------------------------------------------------------------------

def test_netmodel_split_narrow_wgrad_switch(monkeypatch):
    from structure_knowledge_distillation_amd.networks.kd_model import NetModel, default_args
    for name in ("SKD_SPLIT_TRAIN", "SKD_SPLIT_WGRAD", "SKD_SPLIT_NARROW", "SKD_SPLIT_NARROW_WGRAD"):
        monkeypatch.delenv(name, raising=False)
    assert default_args().split_narrow_wgrad is False
    monkeypatch.setenv("SKD_SPLIT_NARROW_WGRAD", "1")
    assert default_args().split_narrow_wgrad is True and default_args(split_narrow_wgrad=False).split_narrow_wgrad is False
    assert default_args().split_train is False and default_args().split_narrow is False and default_args().split_wgrad is False
    monkeypatch.setenv("SKD_SPLIT_NARROW_WGRAD", "0")
    assert default_args().split_narrow_wgrad is False and default_args(split_narrow_wgrad=True).split_narrow_wgrad is True
    _lib.install_test_backend(cref.load(_lib.SIGNATURES))
    try:
        kw = dict(device=torch.device("cpu"), batch_size=2, ho=False)
        flags = lambda model: sorted(set(zip(_marks(model.student, "_skd_train_narrow"), _marks(model.student, "_skd_train_wgrad"),
                                             _marks(model.student, "_skd_train_narrow_wgrad"))))
        model = NetModel(default_args(**kw))
        assert flags(model) == [(False, False, False)] and model.split_narrow_wgrad is False
        # without both prerequisites it routes nothing
        for pre in (dict(), dict(split_train=True), dict(split_narrow=True), dict(split_train=True, split_wgrad=True)):
            model = NetModel(default_args(split_narrow_wgrad=True, **pre, **kw))
            assert not model.split_narrow_wgrad and not any(_marks(model.student, "_skd_train_narrow_wgrad")), pre
        model = NetModel(default_args(split_train=True, split_narrow=True, **kw))
        assert flags(model) == [(True, False, False)] and not model.split_narrow_wgrad
        model = NetModel(default_args(split_train=True, split_narrow=True, split_narrow_wgrad=True, **kw))
        assert flags(model) == [(True, False, True)] and model.split_narrow_wgrad and not model.split_wgrad
        assert len(_marks(model.student, "_skd_train_narrow_wgrad")) == 10
        # independent of split_wgrad
        model = NetModel(default_args(split_train=True, split_narrow=True, split_wgrad=True, split_narrow_wgrad=True, **kw))
        assert flags(model) == [(True, True, True)] and model.split_narrow_wgrad and model.split_wgrad
        monkeypatch.setenv("SKD_SPLIT_NARROW_WGRAD", "1")
        assert flags(NetModel(default_args(**kw))) == [(False, False, False)]
        monkeypatch.setenv("SKD_SPLIT_TRAIN", "1")
        monkeypatch.setenv("SKD_SPLIT_NARROW", "1")
        assert flags(NetModel(default_args(**kw))) == [(True, False, True)]
        assert not any(getattr(m, "_skd_train_narrow_wgrad", False) for m in model.teacher.modules())
    finally:
        _lib.install_test_backend(None)


def test_docs_name_the_narrow_weight_gradient():
    assert "narrow_wgrad" in PC.route_training_convs.__doc__ and "narrow_wgrad" in SF.conv3x3_split_train.__doc__
    assert "skd_narrow_wgrad.h" in SF.conv3x3_narrow_wgrad.__doc__
