"""The training form of the student's 1x1 down-sample (shortcut) convolutions on the split core, the parts that need no GPU: the C
ABI of include/skd_shortcut.h (the pinned names and argument lists, the truth table of the predicate, the host-side refusals of
the launch entries, the split-K plan swept over sizes), the routing and the wiring of a student flagged with ``shortcut=True`` (a
torch-implemented double of the entries on raw HOST addresses, on top of the plain-C double) and NetModel's ``split_shortcut``
switch."""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F

import structure_knowledge_distillation_amd.networks.pspnet_combine as PC
from oracle import cref
from structure_knowledge_distillation_amd import _lib, functional as SF
from structure_knowledge_distillation_amd import networks
from test_conv3x3_train_cpu import _input, _step, _student
from test_student_infer_cpu import _host

NAMES = ["skd_conv1x1_train_supported", "skd_conv1x1_train_fwd_nhwc", "skd_conv1x1_train_fwd_cols64_nhwc",
         "skd_conv1x1_train_dgrad_nhwc", "skd_conv1x1_train_dgrad_cols64_nhwc", "skd_conv1x1_train_wgrad_plan",
         "skd_conv1x1_train_wgrad_nhwc"]
# the student's four, in the order of the forward: layer1.0, layer2.0, layer3.0, layer4.0 (Cin, Cout, stride)
SHORTCUTS = [(128, 64, 1), (64, 128, 2), (128, 256, 1), (256, 512, 1)]


def _out(n, s):
    return (n - 1) // s + 1


def _map(addr, b, h, w, c):
    """The (B, C, H, W) tensor of a channels-last host map (a copy)."""
    return torch.from_numpy(_host(addr, (b, h, w, c)).copy()).permute(0, 3, 1, 2)


def _backward(g, x, w, s, which):
    mask = tuple(i == which for i in range(3))
    return torch.ops.aten.convolution_backward(g, x, w, None, [s, s], [0, 0], [1, 1], False, [0, 0], 1, mask)[which]


class ShortcutDouble:
    """The plain-C double for every core entry + the entries of skd_shortcut.h on raw HOST addresses, computed with torch; the plan
    is one slice.  The products are computed by the ops the unflagged student runs (``F.conv2d``, ``aten.convolution_backward``) on
    tensors of the same layout, so that the comparison with the unflagged sequence sees the wiring and not another kernel's
    rounding.  Every launch is recorded."""

    def __init__(self, core):
        self._core = core
        self.fwd, self.dgrad, self.wgrad = [], [], []

    def __getattr__(self, name):
        return getattr(self._core, name)

    def skd_conv1x1_train_supported(self, cin, cout, kernel, stride, padding, dilation, groups):
        return int(cin > 0 and cout > 0 and cin % 64 == 0 and cout % 64 == 0 and kernel == 1 and stride in (1, 2) and padding == 0
                   and dilation == 1 and groups == 1)

    def skd_conv1x1_train_fwd_nhwc(self, B, H, W, cin, cout, s, x, w, y, stream):
        self.fwd.append(dict(cin=cin, cout=cout, stride=s, x=x, w=w, y=y))
        wt = torch.from_numpy(_host(w, (cout, cin)).copy()).reshape(cout, cin, 1, 1)
        out = F.conv2d(_map(x, B, H, W, cin), wt, None, s)
        _host(y, (B, _out(H, s), _out(W, s), cout))[...] = out.permute(0, 2, 3, 1).numpy()
        return 1

    def skd_conv1x1_train_dgrad_nhwc(self, B, H, W, cin, cout, s, g, wt, dx, stream):
        self.dgrad.append(dict(cin=cin, cout=cout, stride=s, g=g, wt=wt, dx=dx))
        w = torch.from_numpy(_host(wt, (cin, cout)).copy()).t().reshape(cout, cin, 1, 1)
        grad = _backward(_map(g, B, _out(H, s), _out(W, s), cout), torch.zeros(B, H, W, cin).permute(0, 3, 1, 2), w, s, 0)
        _host(dx, (B, H, W, cin))[...] = grad.permute(0, 2, 3, 1).numpy()
        return 1

    def skd_conv1x1_train_wgrad_plan(self, B, H, W, cin, cout, s, slices, cus, plan):
        out = ctypes.cast(plan, ctypes.POINTER(ctypes.c_int64))
        out[0], out[1], out[2] = 1, -(-B * _out(H, s) * _out(W, s) // 16), cin * cout * 4
        return 1

    def skd_conv1x1_train_wgrad_nhwc(self, B, H, W, cin, cout, s, x, g, dw, ws, ws_bytes, slices, stream):
        assert ws and ws_bytes == cin * cout * 4 and slices == 1
        self.wgrad.append(dict(cin=cin, cout=cout, stride=s, x=x, dw=dw))
        grad = _backward(_map(g, B, _out(H, s), _out(W, s), cout), _map(x, B, H, W, cin), torch.zeros(cout, cin, 1, 1), s, 1)
        _host(dw, (cout, cin))[...] = grad.reshape(cout, cin).numpy()
        return 1


@pytest.fixture
def double():
    d = ShortcutDouble(cref.load(_lib.SIGNATURES))
    _lib.install_test_backend(d)
    yield d
    _lib.install_test_backend(None)


def _shapes(calls):
    return [(c["cin"], c["cout"], c["stride"]) for c in calls]


# ---- 1. the C ABI ------------------------------------------------------------------------------------------------------------

def test_shortcut_header_table_and_library_agree():
    """What is particular to skd_shortcut.h; header <-> table <-> library <-> build digest: tests/test_abi.py, for every header."""
    assert sorted(_lib.ABI["skd_shortcut.h"]) == sorted(NAMES) and len(NAMES) == 7


def test_shortcut_supported_truth_table():
    sup = _lib.load().skd_conv1x1_train_supported
    for cin, cout, s in SHORTCUTS + [(64, 64, 1), (192, 320, 2), (512, 64, 2)]:
        assert sup(cin, cout, 1, s, 0, 1, 1) == 1, (cin, cout, s)
    for cin in (-64, 0, 16, 32, 64, 96, 128, 192, 256):
        for cout in (0, 32, 64, 100, 128, 512):
            for k, s, p, d, g in ((1, 1, 0, 1, 1), (1, 2, 0, 1, 1), (1, 3, 0, 1, 1), (1, 0, 0, 1, 1), (3, 1, 0, 1, 1), (3, 1, 1, 1, 1),
                                  (1, 1, 1, 1, 1), (1, 1, 0, 2, 1), (1, 1, 0, 1, 2), (0, 1, 0, 1, 1)):
                want = int(cin > 0 and cout > 0 and cin % 64 == 0 and cout % 64 == 0 and k == 1 and s in (1, 2) and p == 0
                           and d == 1 and g == 1)
                assert sup(cin, cout, k, s, p, d, g) == want, (cin, cout, k, s, p, d, g)


def test_shortcut_launches_host_side_refusals():
    """Every refusal is decided on the host, in front of the launches: no device is touched (the pointers are never followed)."""
    lib = _lib.load()
    A, Bm, OUT, WS = 0x10000, 0x2000000, 0x4000000, 0x8000000
    b, h, w, cin, cout, s = 1, 13, 17, 64, 128, 2                    # 7 x 9 = 63 output pixels: four K-tiles
    for f in (lib.skd_conv1x1_train_fwd_nhwc, lib.skd_conv1x1_train_fwd_cols64_nhwc, lib.skd_conv1x1_train_dgrad_nhwc,
              lib.skd_conv1x1_train_dgrad_cols64_nhwc):
        ok = dict(B=b, H=h, W=w, cin=cin, cout=cout, s=s, a=A, m=Bm, o=OUT)
        for bad in (dict(a=None), dict(m=None), dict(o=None), dict(a=A + 4), dict(a=A + 8), dict(m=Bm + 4), dict(B=0), dict(H=0),
                    dict(W=-1), dict(s=0), dict(s=3), dict(s=-1), dict(cin=32), dict(cin=0), dict(cout=96), dict(cout=-64),
                    dict(B=1 << 10, H=1 << 10, W=1 << 10)):
            v = dict(ok, **bad)
            assert f(v["B"], v["H"], v["W"], v["cin"], v["cout"], v["s"], v["a"], v["m"], v["o"], None) == 0, bad
    plan = (ctypes.c_int64 * 3)()
    assert lib.skd_conv1x1_train_wgrad_plan(b, h, w, cin, cout, s, 2, 0, ctypes.cast(plan, ctypes.c_void_p)) == 1
    assert tuple(plan) == (2, 2, 2 * cin * cout * 4)
    ok = dict(B=b, H=h, W=w, cin=cin, cout=cout, s=s, x=A, g=Bm, dw=OUT, ws=WS, nbytes=int(plan[2]), slices=2)
    for bad in (dict(x=None), dict(g=None), dict(dw=None), dict(ws=None), dict(x=A + 4), dict(g=Bm + 8), dict(ws=WS + 4),
                dict(nbytes=int(plan[2]) - 1), dict(nbytes=0), dict(nbytes=-1), dict(slices=0), dict(slices=-1),
                dict(slices=3),                                      # in range, but not a count the plan returns
                dict(slices=5), dict(slices=1 << 30), dict(s=0), dict(s=3), dict(cin=32), dict(cout=96), dict(cin=0),
                dict(B=0), dict(H=0), dict(W=-1), dict(B=1 << 10, H=1 << 10, W=1 << 10, slices=1, nbytes=1 << 62)):
        v = dict(ok, **bad)
        assert lib.skd_conv1x1_train_wgrad_nhwc(v["B"], v["H"], v["W"], v["cin"], v["cout"], v["s"], v["x"], v["g"], v["dw"], v["ws"],
                                                v["nbytes"], v["slices"], None) == 0, bad


def _plan(lib, *args):
    plan = (ctypes.c_int64 * 3)(-1, -1, -1)
    assert lib.skd_conv1x1_train_wgrad_plan(*args, ctypes.cast(plan, ctypes.c_void_p)) == 1, args
    return int(plan[0]), int(plan[1]), int(plan[2])


def _form(cin, cout):
    """(tiles of one slice, workgroups per compute unit, rounds) of the tile form the channel counts select."""
    if cin % 128 == 0 and cout % 128 == 0:
        return (cin // 128) * (cout // 128), 2, 2
    return -(-(cin // 64) // 2) * (cout // 64), 3, 1


def test_shortcut_wgrad_plan_sweep():
    """An exact cover for every size: no empty slice, the pixel tail covered once; the automatic count follows the header's rule."""
    lib = _lib.load()
    seen_many = False
    for b, h, w in ((1, 1, 1), (1, 5, 7), (2, 13, 11), (2, 12, 10), (8, 33, 33), (8, 65, 65), (8, 129, 129)):
        for cin, cout in ((64, 64), (128, 64), (64, 128), (128, 256), (256, 512), (192, 64)):
            tiles, per_cu, rounds = _form(cin, cout)
            for s in (1, 2):
                nk = -(-b * _out(h, s) * _out(w, s) // 16)
                for cus in (0, 64, 256):
                    for slices in (0, 1, 2, 3, nk, nk + 5):
                        used, t, nbytes = _plan(lib, b, h, w, cin, cout, s, slices, cus)
                        what = (b, h, w, cin, cout, s, slices, cus, used, t)
                        assert 1 <= used <= nk and used * t >= nk and (used - 1) * t < nk, what
                        assert nbytes == used * cin * cout * 4, what
                        if slices:
                            asked = min(slices, nk)
                        else:
                            slots = per_cu * (cus or 256)
                            most = min(max(1, rounds * slots // tiles), nk)
                            asked = min(range(1, most + 1), key=lambda n: (-(-tiles * n // slots) * -(-nk // n), n))
                        assert t == -(-nk // asked) and used == -(-nk // t), what
                        seen_many |= slices == 0 and used > 100
    assert seen_many
    assert _plan(lib, 8, 129, 129, 64, 128, 2, 7, 64) == _plan(lib, 8, 129, 129, 64, 128, 2, 7, 304)
    assert _plan(lib, 8, 65, 65, 128, 256, 1, 0, 0) == _plan(lib, 8, 65, 65, 128, 256, 1, 0, 256)
    ptr = ctypes.cast((ctypes.c_int64 * 3)(), ctypes.c_void_p)
    for bad in ((0, 5, 5, 64, 64, 1, 0, 0), (1, 0, 5, 64, 64, 1, 0, 0), (1, 5, 0, 64, 64, 1, 0, 0), (1, 5, 5, 32, 64, 1, 0, 0),
                (1, 5, 5, 64, 96, 1, 0, 0), (1, 5, 5, 64, 64, 0, 0, 0), (1, 5, 5, 64, 64, 3, 0, 0), (1, 5, 5, 64, 64, 1, -1, 0),
                (1, 5, 5, 64, 64, 1, 0, -1), (1 << 10, 1 << 10, 1 << 10, 64, 64, 1, 0, 0)):
        assert lib.skd_conv1x1_train_wgrad_plan(*bad, ptr) == 0, bad
    assert lib.skd_conv1x1_train_wgrad_plan(1, 5, 5, 64, 64, 1, 0, 0, None) == 0
    # the 3x3 plans are what they were
    wide = (ctypes.c_int64 * 3)()
    assert lib.skd_conv3x3_split_wgrad_plan(8, 65, 65, 512, 512, 0, 256, ctypes.cast(wide, ctypes.c_void_p)) == 1 and wide[0] == 7
    assert lib.skd_conv3x3_narrow_wgrad_plan(8, 129, 129, 128, 64, 0, 256, ctypes.cast(wide, ctypes.c_void_p)) == 1 and wide[0] == 85


# ---- 2. routing and wiring ----------------------------------------------------------------------------------------------------

def _marks(net):
    return [getattr(m, "_skd_train_shortcut", False) for m in net.modules() if isinstance(m, PC.BasicBlock)]


def test_flagged_student_hands_over_the_four_shortcuts(double, monkeypatch):
    # the mechanism, with the policy emptied (test_excluded_products_keep_the_library has the policy)
    monkeypatch.setattr(PC, "SHORTCUT_ROUTING_EXCLUDED", frozenset())
    net, x = _student(), _input()
    plain_out, want = _step(net, x)
    assert double.fwd == [] and double.dgrad == [] and double.wgrad == []

    flagged = networks.route_training_convs(copy.deepcopy(net), shortcut=True)
    assert _marks(flagged) == [True] * 8 and _marks(networks.route_training_convs(copy.deepcopy(net))) == [False] * 8
    got_out, got = _step(flagged, x)
    assert _shapes(double.fwd) == SHORTCUTS and _shapes(double.dgrad)[::-1] == SHORTCUTS and _shapes(double.wgrad)[::-1] == SHORTCUTS
    # which convolutions: the weight matrix of call i is that module's weight, read in place
    convs = [getattr(flagged, "layer%d" % i)[0].downsample[0] for i in (1, 2, 3, 4)]
    for c, conv in zip(double.fwd, convs):
        assert c["w"] == conv.weight.data_ptr() and hasattr(conv, "_skd_conv1x1_train_mats")
    rel = lambda a, b: float((a.detach() - b.detach()).abs().max() / b.detach().abs().max())
    for a, b in zip(got_out, plain_out):
        assert rel(a, b) <= 1e-6, rel(a, b)
    assert set(got) == set(want) and all(g is not None for g in got.values())
    worst = max((rel(got[k], want[k]), k) for k in want)
    print("worst gradient: %.3e %s" % worst)
    for k in want:
        assert rel(got[k], want[k]) <= 1e-6, (k, rel(got[k], want[k]))

    # eval mode, no_grad, an NCHW input: nothing is handed over
    for log in (double.fwd, double.dgrad, double.wgrad):
        log.clear()
    flagged.eval()
    flagged(x)
    flagged.train()
    with torch.no_grad():
        flagged(x)
    flagged.layer3[0](torch.randn(2, 128, 5, 6))
    assert double.fwd == []
    flagged.layer3[0](torch.randn(2, 128, 5, 6).contiguous(memory_format=torch.channels_last))
    assert _shapes(double.fwd) == [(128, 256, 1)]
    # the flag cleared (shortcut=False again, and enable=False): nothing, and the cached matrices are gone
    double.fwd.clear()
    networks.route_training_convs(flagged)
    flagged(x)
    assert double.fwd == [] and _marks(flagged) == [False] * 8
    networks.route_training_convs(flagged, shortcut=True)
    flagged(x)
    assert len(double.fwd) == 4
    networks.route_training_convs(flagged, enable=False, shortcut=True)
    assert _marks(flagged) == [False] * 8 and not any(hasattr(c, "_skd_conv1x1_train_mats") for c in convs)
    flagged(x)
    assert len(double.fwd) == 4


def test_backend_without_the_entries_keeps_the_library():
    _lib.install_test_backend(cref.load(_lib.SIGNATURES))
    try:
        assert not any(_lib.has_entry(n) for n in NAMES)
        net, x = _student(), _input()
        flagged = networks.route_training_convs(copy.deepcopy(net), shortcut=True)
        (_, want), (_, got) = _step(net, x), _step(flagged, x)
        assert all(torch.equal(got[k], want[k]) for k in want)
        xs = torch.zeros(1, 64, 2, 2).contiguous(memory_format=torch.channels_last)
        assert not SF.conv1x1_train_supported(xs, torch.zeros(64, 64, 1, 1, requires_grad=True), 1, 0, 1, 1)
    finally:
        _lib.install_test_backend(None)


def test_excluded_products_keep_the_library(double, monkeypatch):
    assert isinstance(PC.SHORTCUT_ROUTING_EXCLUDED, frozenset)
    assert all(e[:3] in SHORTCUTS and e[3] in SF.SHORTCUT_PRODUCTS for e in PC.SHORTCUT_ROUTING_EXCLUDED)
    net, x = _student(), _input()
    _, want = _step(net, x)
    flagged = networks.route_training_convs(copy.deepcopy(net), shortcut=True)
    # the committed policy: every product it does not list is handed over
    _step(flagged, x)
    for p, log in (("fwd", double.fwd), ("dgrad", double.dgrad), ("wgrad", double.wgrad)):
        assert sorted(_shapes(log)) == sorted(s for s in SHORTCUTS if s + (p,) not in PC.SHORTCUT_ROUTING_EXCLUDED), p
        log.clear()
    monkeypatch.setattr(PC, "SHORTCUT_ROUTING_EXCLUDED", frozenset({(64, 128, 2, "dgrad"), (128, 256, 1, "fwd"), (256, 512, 1, "fwd"),
                                                                    (256, 512, 1, "dgrad"), (256, 512, 1, "wgrad")}))
    flagged.zero_grad(set_to_none=True)
    _, got = _step(flagged, x)
    assert _shapes(double.fwd) == [(128, 64, 1), (64, 128, 2)]
    assert _shapes(double.dgrad)[::-1] == [(128, 64, 1), (128, 256, 1)]
    assert _shapes(double.wgrad)[::-1] == [(128, 64, 1), (64, 128, 2), (128, 256, 1)]
    rel = lambda a, b: float((a.detach() - b.detach()).abs().max() / b.detach().abs().max())
    for k in want:
        assert rel(got[k], want[k]) <= 1e-6, (k, rel(got[k], want[k]))


def test_op_honours_needs_input_grad_and_products(double):
    torch.manual_seed(2)
    conv = torch.nn.Conv2d(64, 128, 1, 2, bias=False)
    x = torch.randn(2, 64, 5, 6).contiguous(memory_format=torch.channels_last)
    assert SF.conv1x1_train_supported(x, conv.weight, 2, 0, 1, 1)
    assert not SF.conv1x1_train_supported(x, conv.weight, 3, 0, 1, 1) and not SF.conv1x1_train_supported(x, conv.weight, 1, 1, 1, 1)
    assert not SF.conv1x1_train_supported(x.contiguous(), conv.weight, 2, 0, 1, 1)
    assert not SF.conv1x1_train_supported(x.double(), conv.weight, 2, 0, 1, 1)
    assert not SF.conv1x1_train_supported(x, torch.zeros(128, 64, 3, 3), 2, 0, 1, 1)
    with torch.no_grad():
        assert not SF.conv1x1_train_supported(x, conv.weight, 2, 0, 1, 1)
    want_w = torch.autograd.grad(F.conv2d(x, conv.weight, None, 2).square().sum(), conv.weight)[0]
    y = SF.conv1x1_split_train(x, conv.weight, 2, owner=conv)            # x needs no gradient: no data-gradient launch
    assert y.is_contiguous(memory_format=torch.channels_last) and y._base is None
    y.square().sum().backward()
    assert (len(double.fwd), len(double.dgrad), len(double.wgrad)) == (1, 0, 1)
    assert float((conv.weight.grad - want_w).abs().max()) <= 1e-6 * float(want_w.abs().max())
    xg = x.clone().requires_grad_(True)
    y = SF.conv1x1_split_train(xg, conv.weight.detach(), 2, owner=conv)
    dx = torch.autograd.grad(y.square().sum(), xg)[0]
    assert (len(double.fwd), len(double.dgrad), len(double.wgrad)) == (2, 1, 1)
    want_x = torch.autograd.grad(F.conv2d(xg, conv.weight, None, 2).square().sum(), xg)[0]
    assert float((dx - want_x).abs().max()) <= 1e-6 * float(want_x.abs().max())
    assert bool((dx[:, :, 1::2] == 0).all()) and bool((dx[:, :, :, 1::2] == 0).all())
    # the products not listed come from the library
    y = SF.conv1x1_split_train(xg, conv.weight, 2, owner=conv, products=("wgrad",))
    gx, gw = torch.autograd.grad(y.square().sum(), (xg, conv.weight))
    assert (len(double.fwd), len(double.dgrad), len(double.wgrad)) == (2, 1, 2)
    assert float((gx - want_x).abs().max()) <= 1e-6 * float(want_x.abs().max())
    assert float((gw - want_w).abs().max()) <= 1e-6 * float(want_w.abs().max())
    # the node keeps the transpose its forward was given; a weight written in between raises autograd's version error
    y = SF.conv1x1_split_train(xg, conv.weight, 2, owner=conv)
    with torch.no_grad():
        conv.weight.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.sum().backward()


def test_fused_optimizer_step_rebuilds_the_transpose(double):
    """torch's fused SGD writes the weights without advancing ``_version``, the key of the cached matrices: the step post-hook
    NetModel registers advances it, and the next forward and data gradient run on the new weights."""
    from structure_knowledge_distillation_amd.networks.kd_model import advance_versions_after_step
    torch.manual_seed(4)
    w = torch.nn.Parameter(torch.randn(128, 64, 1, 1) * 0.1)
    owner = torch.nn.Module()
    x = torch.randn(1, 64, 4, 5).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    try:
        opt = torch.optim.SGD([w], 0.5, fused=True)
    except (RuntimeError, TypeError, ValueError):                       # a torch without fused SGD on the host: the plain form
        opt = torch.optim.SGD([w], 0.5)
    opt.register_step_post_hook(advance_versions_after_step)
    y0 = SF.conv1x1_split_train(x, w, 1, owner=owner)
    key0, _, wt0, _ = owner._skd_conv1x1_train_mats
    SF.conv1x1_split_train(x, w, 1, owner=owner)
    assert owner._skd_conv1x1_train_mats[2] is wt0, "once per weight version"
    y0.square().sum().backward()
    version, before = w._version, w.detach().clone()
    opt.step()
    assert not torch.equal(w.detach(), before) and w._version > version
    x.grad = None
    y1 = SF.conv1x1_split_train(x, w, 1, owner=owner)
    key1, _, wt1, _ = owner._skd_conv1x1_train_mats
    assert key1 != key0 and wt1 is not wt0 and torch.equal(wt1, w.detach().reshape(128, 64).t())
    assert double.dgrad[-1]["wt"] == wt0.data_ptr()
    y1.sum().backward()
    assert double.dgrad[-1]["wt"] == wt1.data_ptr()
    want = F.conv2d(x, w, None, 1)
    assert float((y1 - want).detach().abs().max()) <= 1e-6 * float(want.detach().abs().max()) and not torch.allclose(y1, y0)


# ---- 3. NetModel ----------------------------------------------------------------------------------------------------------------

def test_netmodel_split_shortcut_switch(monkeypatch):
    from structure_knowledge_distillation_amd.networks.kd_model import NetModel, default_args
    for name in ("SKD_SPLIT_TRAIN", "SKD_SPLIT_WGRAD", "SKD_SPLIT_NARROW", "SKD_SPLIT_NARROW_WGRAD", "SKD_SPLIT_SHORTCUT"):
        monkeypatch.delenv(name, raising=False)
    assert default_args().split_shortcut is False
    monkeypatch.setenv("SKD_SPLIT_SHORTCUT", "1")
    assert default_args().split_shortcut is True and default_args(split_shortcut=False).split_shortcut is False
    assert default_args().split_train is False and default_args().split_narrow is False and default_args().split_wgrad is False
    monkeypatch.setenv("SKD_SPLIT_SHORTCUT", "0")
    assert default_args().split_shortcut is False and default_args(split_shortcut=True).split_shortcut is True
    _lib.install_test_backend(cref.load(_lib.SIGNATURES))
    try:
        kw = dict(device=torch.device("cpu"), batch_size=2, ho=False)
        model = NetModel(default_args(**kw))
        assert _marks(model.student) == [False] * 8 and model.split_shortcut is False
        # without split_train it routes nothing
        for pre in (dict(), dict(split_narrow=True), dict(split_wgrad=True)):
            model = NetModel(default_args(split_shortcut=True, **pre, **kw))
            assert not model.split_shortcut and not any(_marks(model.student)), pre
        model = NetModel(default_args(split_train=True, **kw))
        assert _marks(model.student) == [False] * 8 and not model.split_shortcut
        model = NetModel(default_args(split_train=True, split_shortcut=True, **kw))
        assert _marks(model.student) == [True] * 8 and model.split_shortcut and not model.split_wgrad and not model.split_narrow
        # independent of the other three
        model = NetModel(default_args(split_train=True, split_wgrad=True, split_narrow=True, split_narrow_wgrad=True,
                                      split_shortcut=True, **kw))
        assert _marks(model.student) == [True] * 8 and model.split_wgrad and model.split_narrow and model.split_narrow_wgrad
        assert not any(getattr(m, "_skd_train_shortcut", False) for m in model.teacher.modules())
        monkeypatch.setenv("SKD_SPLIT_SHORTCUT", "1")
        assert _marks(NetModel(default_args(**kw)).student) == [False] * 8
        monkeypatch.setenv("SKD_SPLIT_TRAIN", "1")
        assert _marks(NetModel(default_args(**kw)).student) == [True] * 8
    finally:
        _lib.install_test_backend(None)


def test_docs_name_the_shortcut_form():
    assert "shortcut" in PC.route_training_convs.__doc__ and "skd_shortcut.h" in SF.conv1x1_split_train.__doc__
    assert "skd_shortcut.h" in SF.conv1x1_train_supported.__doc__
