"""The student's fused inference path, the parts that need no GPU: the C ABI of include/skd_infer.h (the pinned names and argument lists; header <-> table <-> library is tests/test_abi.py, host-side refusals), the routing of flagged BasicBlocks (a recording double of the two 3x3 entries on top of the plain-C
double), the wiring of the inference form against the plain op sequence (a torch-implemented double of the two entries) and
NetModel's ``fused_eval`` flag."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import structure_knowledge_distillation_amd.networks.pspnet_combine as PC
from oracle import cref
from structure_knowledge_distillation_amd import _lib, functional as SF
from structure_knowledge_distillation_amd import networks

ENTRY, RES_ENTRY = "skd_conv3x3_split_nhwc", "skd_conv3x3_split_res_nhwc"


def _host(addr, shape):
    n = int(np.prod(shape))
    return np.ctypeslib.as_array(ctypes.cast(ctypes.c_void_p(addr), ctypes.POINTER(ctypes.c_float)), shape=(n,)).reshape(shape)


class Conv3x3Double:
    """The plain-C double for every core entry + the 3x3 split entries of skd_eval.h / skd_infer.h on raw HOST addresses.  The
    "pack" is not the kernel's: pack_weights remembers the fp32 weight under the pack's address.  ``compute``: evaluate the two
    convolution entries with torch (F.conv2d, the eval-mode InPlace-ABN formula, residual, activation); otherwise they write
    zeros.  Every convolution call is recorded."""

    def __init__(self, core, compute):
        self._core, self._compute = core, compute
        self.weights, self.calls, self.packs = {}, [], 0

    def __getattr__(self, name):
        return getattr(self._core, name)

    def skd_conv3x3_split_supported(self, cin, cout, stride, padding, dilation, groups):
        return int(cin > 0 and cout > 0 and cin % 16 == 0 and cout % 128 == 0 and stride == 1 and dilation >= 1
                   and padding == dilation and groups == 1)

    def skd_conv3x3_split_pack_bytes(self, cin, cout):
        return cout * cin * 54 if self.skd_conv3x3_split_supported(cin, cout, 1, 1, 1, 1) else 0

    def skd_conv3x3_split_pack_weights(self, cin, cout, w, sn, sc, sy, sx, pack, nbytes, stream):
        self.packs += 1
        base = _host(w, (1 + (cout - 1) * sn + (cin - 1) * sc + 2 * sy + 2 * sx,))
        view = np.lib.stride_tricks.as_strided(base, shape=(cout, cin, 3, 3), strides=tuple(4 * s for s in (sn, sc, sy, sx)))
        self.weights[pack] = torch.from_numpy(view.copy())
        return 1

    def _conv(self, name, B, H, W, cin, cout, dil, x, pack, out, res, cbias, mean, var, weight, bias, eps, act, slope):
        self.calls.append(dict(entry=name, cin=cin, cout=cout, dilation=dil, act=act, x=x, residual=res, bn=(mean, var, weight, bias)))
        o = _host(out, (B, H, W, cout))
        if not self._compute:
            o[...] = 0.0
            return 1
        vec = lambda p: torch.from_numpy(_host(p, (cout,)).copy()) if p else None
        xt = torch.from_numpy(_host(x, (B, H, W, cin)).copy()).permute(0, 3, 1, 2)
        z = F.conv2d(xt, self.weights[pack], vec(cbias), 1, dil, dil).permute(0, 2, 3, 1)
        if mean:
            gamma = vec(weight).abs() + eps if weight else 1.0
            z = ((z - vec(mean)) * (1.0 / torch.sqrt(vec(var) + eps))) * gamma + (vec(bias) if bias else 0.0)
        if res:
            z = z + torch.from_numpy(_host(res, (B, H, W, cout)).copy())
        if act == 3:
            z = torch.relu(z)
        elif act == 1:
            z = torch.where(z < 0, z * slope, z)
        o[...] = z.numpy()
        return 1

    def skd_conv3x3_split_nhwc(self, B, H, W, cin, cout, dil, x, pack, out, cbias, mean, var, weight, bias, eps, act, slope, geometry,
                               stream):
        return self._conv(ENTRY, B, H, W, cin, cout, dil, x, pack, out, None, cbias, mean, var, weight, bias, eps, act, slope)

    def skd_conv3x3_split_res_nhwc(self, B, H, W, cin, cout, dil, x, pack, out, res, cbias, mean, var, weight, bias, eps, act, slope,
                                   geometry, stream):
        return self._conv(RES_ENTRY, B, H, W, cin, cout, dil, x, pack, out, res, cbias, mean, var, weight, bias, eps, act, slope)


@pytest.fixture
def recording():
    d = Conv3x3Double(cref.load(_lib.SIGNATURES), compute=False)
    _lib.install_test_backend(d)
    yield d
    _lib.install_test_backend(None)


@pytest.fixture
def computing():
    d = Conv3x3Double(cref.load(_lib.SIGNATURES), compute=True)
    _lib.install_test_backend(d)
    yield d
    _lib.install_test_backend(None)


# ---- 1. the C ABI ------------------------------------------------------------------------------------------------------------

def test_infer_header_table_and_library_agree():
    """What is particular to skd_infer.h; header <-> table <-> library <-> build digest: tests/test_abi.py, for every header."""
    assert sorted(_lib.ABI["skd_infer.h"]) == [RES_ENTRY]
    # the existing entry's arguments with `residual` behind `out`
    old, new = _lib.signature(ENTRY), _lib.signature(RES_ENTRY)
    assert new[0] == old[0] and new[1] == old[1][:9] + [ctypes.c_void_p] + old[1][9:]


def test_infer_host_side_refusals():
    """Every refusal is decided on the host, in front of the launch: no device is touched (the pointers are never followed)."""
    f = _lib.load().skd_conv3x3_split_res_nhwc
    X, WP, OUT, RES, V = 0x10000, 0x20000, 0x4000000, 0x8000000, 0x30000
    ok = dict(B=1, H=4, W=4, cin=32, cout=128, d=1, x=X, wp=WP, out=OUT, res=RES, cb=None, mean=None, var=None, w=None, b=None,
              eps=1e-5, act=3, slope=0.01, geo=0)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["B"], a["H"], a["W"], a["cin"], a["cout"], a["d"], a["x"], a["wp"], a["out"], a["res"], a["cb"], a["mean"], a["var"],
                 a["w"], a["b"], a["eps"], a["act"], a["slope"], a["geo"], None)
    nbytes = 1 * 4 * 4 * 128 * 4
    for bad in (dict(x=None), dict(wp=None), dict(out=None), dict(mean=V), dict(var=V), dict(geo=-1), dict(geo=4), dict(cout=64),
                dict(cin=24), dict(d=0), dict(d=-2), dict(B=0), dict(H=0), dict(W=-1), dict(act=2), dict(act=7), dict(x=X + 4),
                dict(wp=WP + 8),
                # a residual that overlaps the output: the same buffer, one float into it from either side, its last float
                dict(res=OUT), dict(res=OUT + 4), dict(res=OUT - 4), dict(res=OUT + nbytes - 4), dict(res=OUT - nbytes + 4),
                # the residual-free form refuses the same things
                dict(res=None, x=None), dict(res=None, cout=64), dict(res=None, geo=4), dict(res=None, mean=V)):
        assert call(**bad) == 0, bad


# ---- 3. routing -------------------------------------------------------------------------------------------------------------

def _student():
    torch.manual_seed(5)
    return PC.Res_pspnet(PC.BasicBlock, [2, 2, 2, 2], 19).eval().to(memory_format=torch.channels_last)


def _forward(net, grad=False):
    x = torch.randn(1, 3, 33, 49, generator=torch.Generator().manual_seed(11)).contiguous(memory_format=torch.channels_last)
    with torch.set_grad_enabled(grad):
        return net(x)


def test_routing_of_flagged_blocks(recording, monkeypatch):
    net = _student()
    blocks = {name: m for name, m in net.named_modules() if isinstance(m, PC.BasicBlock)}
    assert len(blocks) == 8
    seen, down = {}, []
    for name, m in blocks.items():
        m.register_forward_pre_hook(lambda mod, args, name=name: seen.__setitem__(name, args[0]))
    real = PC._conv1x1_bn_eval

    def spy(x, conv, bn, relu):
        out = real(x, conv, bn, relu)
        down.append((conv, out))
        return out
    monkeypatch.setattr(PC, "_conv1x1_bn_eval", spy)

    _forward(net)                                                 # unflagged: nothing reaches either entry
    assert recording.calls == [] and recording.packs == 0 and down == []

    assert networks.fuse_for_inference(net) is net and PC.fuse_for_inference is networks.fuse_for_inference
    assert all(m._skd_infer_min_cin == PC.FUSED_EVAL_MIN_CIN for m in blocks.values())
    assert PC.FUSED_EVAL_MIN_CIN == 128 and PC.CONV3X3_SPLIT_MIN_CIN == 256      # the teacher's policy is not the student's
    routed = [blocks[n] for n in ("layer3.0", "layer3.1", "layer4.0", "layer4.1")]
    assert recording.packs == 11, "the routed weights are packed eagerly"
    assert all(hasattr(c, "_skd_conv3x3_pack") for b in routed for c in (b.conv1, b.conv2))
    for conv in (blocks["layer1.0"].conv1, blocks["layer1.0"].conv2, blocks["layer1.1"].conv1, blocks["layer1.1"].conv2,
                 blocks["layer2.0"].conv1):
        assert not hasattr(conv, "_skd_conv3x3_pack")          # Cout = 64, and the stride-2 convolution: never routed

    out = _forward(net)
    assert all(bool(torch.isfinite(o).all()) for o in out)
    assert recording.packs == 11, "nothing is packed again in the forward"
    # layer2's stride-1 convolutions (128 input channels: the measured default); layer2.0.conv1 (stride 2) and layer1 are not routed
    l2 = [c for c in recording.calls if c["cout"] == 128]
    assert [(c["entry"], c["cin"], c["dilation"]) for c in l2] == [(RES_ENTRY, 128, 1), (ENTRY, 128, 1), (RES_ENTRY, 128, 1)]
    assert recording.calls[:3] == l2 and not [c for c in recording.calls if c["cout"] == 64 or c["cin"] == 64]
    assert l2[0]["x"] != seen["layer2.0"].data_ptr() and l2[1]["x"] == seen["layer2.1"].data_ptr() == l2[2]["residual"]
    calls = recording.calls[3:]
    assert [c["entry"] for c in calls] == [ENTRY, RES_ENTRY] * 4                    # exactly two per block of layer3 / layer4
    want = [(128, 256, 2), (256, 256, 2), (256, 256, 2), (256, 256, 2), (256, 512, 4), (512, 512, 4), (512, 512, 4), (512, 512, 4)]
    assert [(c["cin"], c["cout"], c["dilation"]) for c in calls] == want
    assert all(c["act"] == 3 for c in recording.calls), "ReLU in both epilogues"
    assert [conv for conv, _ in down] == [blocks["layer3.0"].downsample[0], blocks["layer4.0"].downsample[0]]
    for i, name in enumerate(("layer3.0", "layer3.1", "layer4.0", "layer4.1")):
        c1, c2, b = calls[2 * i], calls[2 * i + 1], blocks[name]
        assert c1["x"] == seen[name].data_ptr() and c1["residual"] is None
        assert c1["bn"][:2] == (b.bn1.running_mean.data_ptr(), b.bn1.running_var.data_ptr())
        assert c2["bn"] == tuple(t.data_ptr() for t in (b.bn2.running_mean, b.bn2.running_var, b.bn2.weight, b.bn2.bias))
        want_res = down[i // 2][1] if name.endswith(".0") else seen[name]
        assert c2["residual"] == want_res.data_ptr() and c2["residual"] != c2["x"]

    # training mode, or a graph: nothing is routed
    recording.calls.clear()
    _forward(net, grad=True)
    assert recording.calls == []
    net.train()
    with torch.no_grad():
        net.layer3(torch.randn(2, 128, 5, 6).contiguous(memory_format=torch.channels_last))
    net.eval()
    assert recording.calls == []
    # an input that is not channels-last fp32 keeps the old sequence
    with torch.no_grad():
        net.layer3[1](torch.randn(1, 256, 5, 6))
    assert recording.calls == []

    # min_cin = 256, the frozen teacher's policy: layer2 and the 128 -> 256 first convolution of layer3 keep conv -> forward_relu,
    # the other convolution of that block is still fused
    networks.fuse_for_inference(net, min_cin=256)
    _forward(net)
    assert [(c["entry"], c["cin"], c["cout"]) for c in recording.calls[:2]] == [(RES_ENTRY, 256, 256), (ENTRY, 256, 256)]
    assert len(recording.calls) == 7 and min(c["cin"] for c in recording.calls) == 256

    # enable=False: the first state, and the packs are gone
    recording.calls.clear()
    assert networks.fuse_for_inference(net, enable=False) is net
    assert all(m._skd_infer_min_cin is None for m in blocks.values())
    assert not any(hasattr(c, "_skd_conv3x3_pack") for b in blocks.values() for c in (b.conv1, b.conv2))
    _forward(net)
    assert recording.calls == []


def test_plain_c_double_keeps_todays_sequence():
    """A back-end without the entries: flagged blocks run what they ran, nothing raises."""
    _lib.install_test_backend(cref.load(_lib.SIGNATURES))
    try:
        assert not _lib.has_entry(RES_ENTRY) and not _lib.has_entry(ENTRY)
        net = _student()
        want = _forward(net)
        got = _forward(networks.fuse_for_inference(net))
        assert all(torch.equal(a, b) for a, b in zip(want, got))
        with pytest.raises(NotImplementedError, match=RES_ENTRY):
            with torch.no_grad():
                SF.conv3x3_split_res_eval(torch.zeros(1, 16, 2, 2), torch.zeros(4, dtype=torch.uint8), 128, 1, None, None, "relu")
    finally:
        _lib.install_test_backend(None)


# ---- 4. wiring ----------------------------------------------------------------------------------------------------------------

def _randomise(block, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in block.modules():
            if hasattr(m, "running_mean"):
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.3)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
                m.weight.copy_(torch.randn(m.weight.shape, generator=g))           # negative gammas too: |gamma| + eps
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
    return block


@pytest.mark.parametrize("cin", [256, 128])
def test_wiring_equals_the_plain_sequence(computing, cin):
    torch.manual_seed(cin)
    down = None
    if cin != 256:
        down = torch.nn.Sequential(torch.nn.Conv2d(cin, 256, 1, 1, bias=False), PC.BatchNorm2d(256, affine=True))
    block = _randomise(PC.BasicBlock(cin, 256, dilation=2, downsample=down), cin).eval().to(memory_format=torch.channels_last)
    x = torch.randn(2, cin, 6, 7).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        want = block(x.clone())
        assert computing.calls == []
        networks.fuse_for_inference(block)
        got = block(x.clone())
    assert [c["entry"] for c in computing.calls] == [ENTRY, RES_ENTRY]
    assert got.shape == want.shape and got.is_contiguous(memory_format=torch.channels_last)
    err = float((got - want).abs().max() / want.abs().max())
    assert err <= 1e-6, err
    # the check has teeth: bn1 and bn2 differ, and so do the residual and the block's input / conv1's output
    assert not torch.allclose(block.bn1.running_mean, block.bn2.running_mean)


# ---- 5. NetModel ----------------------------------------------------------------------------------------------------------------

def test_netmodel_fused_eval_flag():
    from structure_knowledge_distillation_amd.networks.kd_model import NetModel, default_args
    assert default_args().fused_eval is False
    _lib.install_test_backend(cref.load(_lib.SIGNATURES))
    try:
        kw = dict(device=torch.device("cpu"), batch_size=2, ho=False)
        flags = lambda model: [getattr(m, "_skd_infer_min_cin", None) for m in model.student.modules() if isinstance(m, PC.BasicBlock)]
        assert flags(NetModel(default_args(**kw))) == [None] * 8
        assert flags(NetModel(default_args(fused_eval=True, **kw))) == [PC.FUSED_EVAL_MIN_CIN] * 8
    finally:
        _lib.install_test_backend(None)


def test_evaluate_docstring_names_the_flag():
    from structure_knowledge_distillation_amd.networks import evaluate
    assert "fuse_for_inference" in evaluate.__doc__
