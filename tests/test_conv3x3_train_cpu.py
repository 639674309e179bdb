"""The training student's 3x3 convolutions on the split core, the parts that need no GPU: the C ABI of include/skd_train.h (header
<-> table <-> exported symbols, host-side refusals, the truth table of the supported query), the routing of a flagged student (a
recording double of the entries on top of the plain-C double), the wiring of the training form against the plain op sequence (a
torch-implemented double: its "packs" are handles to w and to the flipped, transposed Wd, its run entry is F.conv2d) and NetModel's
``split_train`` flag."""
import copy

import numpy as np
import pytest
import torch

import structure_knowledge_distillation_amd.networks.pspnet_combine as PC
from oracle import cref
from structure_knowledge_distillation_amd import _lib, functional as SF
from structure_knowledge_distillation_amd import networks
from test_student_infer_cpu import Conv3x3Double, _host

SUPPORTED, PACK_PAIR, RUN = "skd_conv3x3_split_train_supported", "skd_conv3x3_split_pack_pair", "skd_conv3x3_split_nhwc"


class TrainDouble(Conv3x3Double):
    """Conv3x3Double + the two entries of skd_train.h on raw HOST addresses: pack_pair remembers w under pack_fwd's address and
    Wd[c][n][ty][tx] = w[n][c][2 - ty][2 - tx] under pack_bwd's, so the run entry's F.conv2d is the forward on one and the data
    gradient on the other."""

    def __init__(self, core, compute):
        super().__init__(core, compute)
        self.pairs = []

    def skd_conv3x3_split_train_supported(self, cin, cout, stride, padding, dilation, groups):
        return int(self.skd_conv3x3_split_supported(cin, cout, stride, padding, dilation, groups) and cin % 128 == 0)

    def skd_conv3x3_split_pack_pair(self, cin, cout, w, sn, sc, sy, sx, pack_fwd, fwd_bytes, pack_bwd, bwd_bytes, stream):
        assert pack_fwd and pack_bwd and fwd_bytes == bwd_bytes == cin * cout * 54
        base = _host(w, (1 + (cout - 1) * sn + (cin - 1) * sc + 2 * sy + 2 * sx,))
        view = np.lib.stride_tricks.as_strided(base, shape=(cout, cin, 3, 3), strides=tuple(4 * s for s in (sn, sc, sy, sx)))
        wt = torch.from_numpy(view.copy())
        self.weights[pack_fwd] = wt
        self.weights[pack_bwd] = wt.flip(2, 3).transpose(0, 1).contiguous()
        self.pairs.append(dict(cin=cin, cout=cout, w=w, strides=(sn, sc, sy, sx), fwd=pack_fwd, bwd=pack_bwd))
        return 1


@pytest.fixture
def recording():
    d = TrainDouble(cref.load(_lib.SIGNATURES), compute=False)
    _lib.install_test_backend(d)
    yield d
    _lib.install_test_backend(None)


@pytest.fixture
def computing():
    d = TrainDouble(cref.load(_lib.SIGNATURES), compute=True)
    _lib.install_test_backend(d)
    yield d
    _lib.install_test_backend(None)


# ---- 1. the C ABI ------------------------------------------------------------------------------------------------------------

def test_train_header_table_and_library_agree():
    """What is particular to skd_train.h; header <-> table <-> library <-> build digest: tests/test_abi.py, for every header."""
    assert sorted(_lib.ABI["skd_train.h"]) == sorted([SUPPORTED, PACK_PAIR])
    # the supported query has the arguments of the existing one; pack_pair those of pack_weights with a second (pack, bytes) pair
    assert _lib.signature(SUPPORTED) == _lib.signature("skd_conv3x3_split_supported")
    old, new = _lib.signature("skd_conv3x3_split_pack_weights"), _lib.signature(PACK_PAIR)
    assert new[0] == old[0] and new[1] == old[1][:9] + old[1][7:9] + old[1][9:]


def test_train_supported_truth_table():
    sup = _lib.load().skd_conv3x3_split_train_supported
    for cin, cout in ((128, 128), (128, 256), (256, 128), (512, 512), (384, 128)):
        for d in (1, 2, 4):
            assert sup(cin, cout, 1, d, d, 1) == 1, (cin, cout, d)
    for bad in ((64, 128, 1, 1, 1, 1), (128, 64, 1, 1, 1, 1), (32, 128, 1, 1, 1, 1), (128, 32, 1, 1, 1, 1), (144, 128, 1, 1, 1, 1),
                (128, 192, 1, 1, 1, 1), (0, 128, 1, 1, 1, 1), (128, 0, 1, 1, 1, 1), (-128, 128, 1, 1, 1, 1),
                (128, 128, 2, 1, 1, 1), (128, 128, 1, 1, 2, 1), (128, 128, 1, 2, 1, 1), (128, 128, 1, 0, 0, 1), (128, 128, 1, 1, 1, 2)):
        assert sup(*bad) == 0, bad


def test_pack_pair_host_side_refusals():
    """Every refusal is decided on the host, in front of the launch: no device is touched (the pointers are never followed)."""
    f = _lib.load().skd_conv3x3_split_pack_pair
    W, PF, PB = 0x10000, 0x2000000, 0x4000000
    n = 128 * 128 * 54
    assert _lib.load().skd_conv3x3_split_pack_bytes(128, 128) == n
    ok = dict(cin=128, cout=128, w=W, sn=1152, sc=9, sy=3, sx=1, pf=PF, fb=n, pb=PB, bb=n)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["cin"], a["cout"], a["w"], a["sn"], a["sc"], a["sy"], a["sx"], a["pf"], a["fb"], a["pb"], a["bb"], None)
    for bad in (dict(w=None), dict(pf=None, pb=None), dict(pf=PF + 8), dict(pb=PB + 4), dict(pf=PF + 8, pb=None), dict(pf=None, pb=PB + 4),
                dict(fb=n - 1), dict(bb=n - 1), dict(fb=0), dict(bb=-1), dict(pf=None, bb=n - 1), dict(pb=None, fb=n - 1),
                dict(sn=-1), dict(sc=-9), dict(sy=-3), dict(sx=-1),
                dict(cin=64), dict(cout=64), dict(cin=24), dict(cout=24), dict(cin=0), dict(cout=-128),
                # one image only: its own direction has to fit (N a multiple of 128, K of 16)
                dict(cout=32), dict(cin=32), dict(cout=32, pb=None), dict(cin=32, pf=None), dict(cout=24, pf=None), dict(cin=24, pb=None)):
        assert call(**bad) == 0, bad


# ---- 2. routing -------------------------------------------------------------------------------------------------------------

def _student():
    torch.manual_seed(5)
    net = PC.Res_pspnet(PC.BasicBlock, [2, 2, 2, 2], 19).train().to(memory_format=torch.channels_last)
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.p = 0.0
    return net


def _input():
    return torch.randn(2, 3, 49, 57, generator=torch.Generator().manual_seed(11)).contiguous(memory_format=torch.channels_last)


# (Cin, Cout, dilation) in the order of the forward: layer2.0.conv2, layer2.1, layer3, dsn[0], layer4, the PSP half
ROUTED = ([(128, 128, 1)] * 3 + [(128, 256, 2)] + [(256, 256, 2)] * 3 + [(256, 128, 1)] + [(256, 512, 4)] + [(512, 512, 4)] * 3
          + [(512, 128, 1)])


def test_routing_of_a_flagged_student(recording):
    net = _student()
    x = _input()
    seen = {}
    for name, m in net.named_modules():
        if isinstance(m, (PC.BasicBlock, PC.PSPModule)):
            m.register_forward_pre_hook(lambda mod, args, name=name: seen.__setitem__(name, args[0]))
    net(x)                                                        # unflagged: nothing reaches the entries
    assert recording.calls == [] and recording.pairs == []

    assert networks.route_training_convs(net) is net and PC.route_training_convs is networks.route_training_convs
    assert PC.TRAIN_SPLIT_MIN_CIN == 128 and isinstance(PC.TRAIN_ROUTING_EXCLUDED, frozenset)
    flagged = [m for m in net.modules() if isinstance(m, (PC.BasicBlock, PC.ResNet, PC.PSPModule))]
    assert len(flagged) == 10 and all(m._skd_train_min_cin == 128 for m in flagged)
    out = net(x)
    assert len(out) == 7
    calls = recording.calls
    assert [(c["cin"], c["cout"], c["dilation"]) for c in calls] == ROUTED and len(ROUTED) == 13
    assert all(c["entry"] == RUN and c["act"] == 0 and c["residual"] is None and c["bn"] == (None,) * 4 for c in calls)
    assert not [c for c in calls if 64 in (c["cin"], c["cout"])]            # stem / layer1 and the stride-2 layer2.0.conv1
    # which convolutions: the pack of call i is the forward image of that module's weight, the input is that module's
    mods = dict(net.named_modules())
    convs = [mods[n] for n in ("layer2.0.conv2", "layer2.1.conv1", "layer2.1.conv2", "layer3.0.conv1", "layer3.0.conv2",
                               "layer3.1.conv1", "layer3.1.conv2", "dsn.0", "layer4.0.conv1", "layer4.0.conv2", "layer4.1.conv1",
                               "layer4.1.conv2")]
    assert len(recording.pairs) == 13, "one pack_pair launch per routed weight"
    for c, p, conv in zip(calls[:12], recording.pairs[:12], convs):
        assert p["w"] == conv.weight.data_ptr() and p["strides"] == tuple(conv.weight.stride())
        assert (p["cin"], p["cout"]) == (conv.in_channels, conv.out_channels)
        key, pf, pb, _ = conv._skd_conv3x3_train_pack
        assert (pf.data_ptr(), pb.data_ptr()) == (p["fwd"], p["bwd"])
    # (the packs of the double are handles, so the call's pack is found through the recorded pair)
    for name, i in (("layer2.1", 1), ("layer3.0", 3), ("layer3.1", 5), ("layer4.0", 8), ("layer4.1", 10)):
        assert calls[i]["x"] == seen[name].data_ptr(), name
    assert calls[7]["x"] == seen["layer4.0"].data_ptr()                                # dsn[0] reads x3
    # the PSP half: the strided channel slice of the bottleneck's weight, read in place
    wb = net.pspmodule.bottleneck[0].weight
    p = recording.pairs[12]
    assert wb.shape[1] == 4 * 128 + 512 and p["w"] == wb[:, 512:].data_ptr() and p["strides"] == tuple(wb.stride())
    assert (p["cin"], p["cout"]) == (512, 128) and calls[12]["x"] == seen["pspmodule"].data_ptr()

    # once per weight version: a second forward splits nothing; a written weight is split again, alone
    recording.calls.clear()
    net(x)
    assert len(recording.calls) == 13 and len(recording.pairs) == 13
    with torch.no_grad():
        net.layer3[0].conv2.weight.mul_(0.5)
    net(x)
    assert len(recording.pairs) == 14 and recording.pairs[13]["w"] == net.layer3[0].conv2.weight.data_ptr()

    # eval mode, no_grad, an NCHW input: nothing is routed
    recording.calls.clear()
    net.eval()
    net(x)
    net.train()
    with torch.no_grad():
        net(x)
    assert recording.calls == []
    xn = torch.randn(2, 256, 5, 6)
    net.layer3[1](xn)                   # each convolution is asked on its own: conv1 reads the NCHW map and keeps the library
    assert all(c["x"] != xn.data_ptr() for c in recording.calls) and len(recording.calls) <= 1
    assert not PC._train_form(net.layer3[1], xn, net.layer3[1].conv1)[0]
    recording.calls.clear()
    net.layer3[1](torch.randn(2, 256, 5, 6).contiguous(memory_format=torch.channels_last))
    assert len(recording.calls) == 2
    # min_cin = 256: layer2, layer3.0.conv1 stay on the library
    recording.calls.clear()
    networks.route_training_convs(net, min_cin=256)
    net(x)
    assert [(c["cin"], c["cout"], c["dilation"]) for c in recording.calls] == [r for r in ROUTED if r[0] >= 256]
    # an excluded shape keeps the library
    recording.calls.clear()
    networks.route_training_convs(net)
    try:
        PC.TRAIN_ROUTING_EXCLUDED = frozenset({(512, 512, 4), (512, 128, 1)})
        net(x)
    finally:
        PC.TRAIN_ROUTING_EXCLUDED = frozenset()
    assert [(c["cin"], c["cout"], c["dilation"]) for c in recording.calls] == [r for r in ROUTED if r[0] != 512]

    # enable=False: the first state, and the packs are gone
    recording.calls.clear()
    assert networks.route_training_convs(net, enable=False) is net
    assert all(m._skd_train_min_cin is None for m in flagged)
    assert not any(hasattr(m, "_skd_conv3x3_train_pack") for m in net.modules())
    assert "pack3x3_train" not in net.pspmodule._fold_cache
    net(x)
    assert recording.calls == []


def test_plain_c_double_keeps_todays_sequence():
    """A back-end without the entries: a flagged student runs what it ran, nothing raises."""
    _lib.install_test_backend(cref.load(_lib.SIGNATURES))
    try:
        assert not any(_lib.has_entry(n) for n in (SUPPORTED, PACK_PAIR, RUN))
        net, x = _student(), _input()
        flagged = networks.route_training_convs(copy.deepcopy(net))
        want, got = net(x), flagged(x)
        assert all(torch.equal(a, b) for a, b in zip(want, got))
        assert not SF.conv3x3_train_supported(torch.zeros(1, 128, 2, 2).contiguous(memory_format=torch.channels_last),
                                              torch.zeros(128, 128, 3, 3), 1, 1, 1, 1)
    finally:
        _lib.install_test_backend(None)


# ---- 3. wiring ----------------------------------------------------------------------------------------------------------------

def _step(net, x):
    x = x.clone().requires_grad_(True)
    out = net(x)
    gen = torch.Generator().manual_seed(3)
    loss = sum((o * torch.randn(o.shape, generator=gen)).sum() for o in out)
    loss.backward()
    grads = {k: p.grad for k, p in net.named_parameters()}
    grads["input"] = x.grad
    return out, grads


def test_wiring_equals_the_plain_sequence(computing):
    net, x = _student(), _input()
    flagged = networks.route_training_convs(copy.deepcopy(net))
    want_out, want = _step(net, x)
    assert computing.calls == []
    got_out, got = _step(flagged, x)
    # 13 forward launches, 13 data gradients (transposed channel counts, the other image of the same pair), in reverse order
    fw, bw = computing.calls[:13], computing.calls[13:]
    assert [(c["cin"], c["cout"], c["dilation"]) for c in fw] == ROUTED
    assert [(c["cout"], c["cin"], c["dilation"]) for c in bw][::-1] == ROUTED
    assert len(computing.pairs) == 13
    rel = lambda a, b: float((a.detach() - b.detach()).abs().max() / b.detach().abs().max())
    for a, b in zip(got_out, want_out):
        assert rel(a, b) <= 1e-6, rel(a, b)
    assert set(got) == set(want) and all(g is not None for g in got.values())
    worst = max((rel(got[k], want[k]), k) for k in want)
    print("worst gradient: %.3e %s" % worst)
    for k in want:
        assert rel(got[k], want[k]) <= 1e-6, (k, rel(got[k], want[k]))
    # the bias of dsn[0] went through the epilogue and has its gradient; the PSP weight got both halves of its gradient
    assert float(got["dsn.0.bias"].abs().max()) > 0 and float(got["pspmodule.bottleneck.0.weight"][:, :512].abs().max()) > 0


def test_backward_uses_the_pack_of_its_forward(computing):
    """needs_input_grad is honoured, and a node keeps the pack_bwd its forward was given."""
    torch.manual_seed(2)
    conv = torch.nn.Conv2d(128, 128, 3, 1, 2, 2, bias=True).to(memory_format=torch.channels_last)
    x = torch.randn(2, 128, 5, 6).contiguous(memory_format=torch.channels_last)
    assert SF.conv3x3_train_supported(x, conv.weight, 1, 2, 2, 1)
    assert not SF.conv3x3_train_supported(x, conv.weight, 2, 2, 2, 1) and not SF.conv3x3_train_supported(x, conv.weight, 1, 1, 2, 1)
    assert not SF.conv3x3_train_supported(x.contiguous(), conv.weight, 1, 2, 2, 1)
    assert not SF.conv3x3_train_supported(x.double(), conv.weight, 1, 2, 2, 1)
    with torch.no_grad():
        assert not SF.conv3x3_train_supported(x, conv.weight, 1, 2, 2, 1)
    y = SF.conv3x3_split_train(x, conv.weight, 2, conv.bias, owner=conv)            # x needs no gradient: no data-gradient launch
    y.sum().backward()
    assert len(computing.calls) == 1 and conv.weight.grad is not None and conv.bias.grad is not None
    xg = x.clone().requires_grad_(True)
    y = SF.conv3x3_split_train(xg, conv.weight, 2, conv.bias, owner=conv)
    pair = computing.pairs[-1]
    assert len(computing.pairs) == 1
    with torch.no_grad():
        conv.weight.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.sum().backward()
    y2 = SF.conv3x3_split_train(xg, conv.weight, 2, conv.bias, owner=conv)
    assert len(computing.pairs) == 2 and computing.pairs[-1] is not pair
    y2.sum().backward()
    want = torch.autograd.grad(torch.nn.functional.conv2d(xg, conv.weight, conv.bias, 1, 2, 2).sum(), xg)[0]
    assert float((xg.grad - want).abs().max() / want.abs().max()) <= 1e-6


def test_fused_optimizer_step_rebuilds_the_packs(computing):
    """torch's fused SGD writes the weights without advancing ``_version``, the key of the packs: the step post-hook NetModel
    registers advances it, and the next forward splits the new weights."""
    from structure_knowledge_distillation_amd.networks.kd_model import advance_versions_after_step
    torch.manual_seed(4)
    w = torch.nn.Parameter((torch.randn(128, 128, 3, 3) * 0.05).contiguous(memory_format=torch.channels_last))
    owner = torch.nn.Module()
    x = torch.randn(1, 128, 4, 5).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    try:
        opt = torch.optim.SGD([w], 0.5, fused=True)
    except (RuntimeError, TypeError, ValueError):                       # a torch without fused SGD on the host: the plain form
        opt = torch.optim.SGD([w], 0.5)
    opt.register_step_post_hook(advance_versions_after_step)
    y0 = SF.conv3x3_split_train(x, w, 1, owner=owner)
    y0.square().sum().backward()
    version, before = w._version, w.detach().clone()
    opt.step()
    assert not torch.equal(w.detach(), before) and w._version > version
    y1 = SF.conv3x3_split_train(x, w, 1, owner=owner)
    assert len(computing.pairs) == 2, "the new weights were split"
    want = torch.nn.functional.conv2d(x, w, None, 1, 1, 1)
    assert float((y1 - want).detach().abs().max()) <= 1e-6 * float(want.detach().abs().max()) and not torch.allclose(y1, y0)
    # a parameter the step did not write (no gradient) keeps its version
    idle = torch.nn.Parameter(torch.zeros(3))
    opt2 = torch.optim.SGD([idle], 0.5)
    advance_versions_after_step(opt2)
    assert idle._version == 0


# ---- 4. NetModel ----------------------------------------------------------------------------------------------------------------

def test_netmodel_split_train_flag(monkeypatch):
    from structure_knowledge_distillation_amd.networks.kd_model import NetModel, default_args
    monkeypatch.delenv("SKD_SPLIT_TRAIN", raising=False)
    assert default_args().split_train is False
    monkeypatch.setenv("SKD_SPLIT_TRAIN", "1")
    assert default_args().split_train is True and default_args(split_train=False).split_train is False
    monkeypatch.setenv("SKD_SPLIT_TRAIN", "0")
    assert default_args().split_train is False and default_args(split_train=True).split_train is True
    _lib.install_test_backend(cref.load(_lib.SIGNATURES))
    try:
        kw = dict(device=torch.device("cpu"), batch_size=2, ho=False)
        flags = lambda model: [getattr(m, "_skd_train_min_cin", None) for m in model.student.modules()
                               if isinstance(m, (PC.BasicBlock, PC.ResNet, PC.PSPModule))]
        assert flags(NetModel(default_args(**kw))) == [None] * 10
        model = NetModel(default_args(split_train=True, **kw))
        assert flags(model) == [PC.TRAIN_SPLIT_MIN_CIN] * 10 and model.split_train
        from structure_knowledge_distillation_amd.networks.kd_model import advance_versions_after_step
        assert advance_versions_after_step in model.G_solver._optimizer_step_post_hooks.values()
        # (with the switch off too: the eval-mode caches are keyed on the version as well, tests/test_stale_caches_cpu.py)
        assert advance_versions_after_step in NetModel(default_args(**kw)).G_solver._optimizer_step_post_hooks.values()
        assert [getattr(m, "_skd_train_min_cin", None) for m in model.teacher.modules() if isinstance(m, PC.ResNet)] == [None]
        monkeypatch.setenv("SKD_SPLIT_TRAIN", "1")
        assert flags(NetModel(default_args(**kw))) == [PC.TRAIN_SPLIT_MIN_CIN] * 10
    finally:
        _lib.install_test_backend(None)


def test_module_docstring_names_the_training_form():
    assert "route_training_convs" in PC.__doc__
