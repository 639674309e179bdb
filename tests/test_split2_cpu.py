"""The frozen teacher's two-piece mode (include/skd_split2.h), the parts that need no GPU: the C ABI (the pinned names and argument lists; header <-> table <-> library is tests/test_abi.py, the pack size, the host-side refusals of the five entries), the ops' ``pieces`` parameter, the routing of a network marked
by ``set_teacher_pieces`` (a recording double of the 1x1 entries on top of the plain-C double; the 3x3 ops, which refuse host
tensors, are recorded at the op), the public switch, the caches behind a fused optimizer step, and the float64 model of the mode
itself (tests/split2_ref.py)."""
import copy
import ctypes
import warnings

import pytest
import torch
import torch.nn.functional as F

import split2_ref as R
import structure_knowledge_distillation_amd.networks.pspnet_combine as PC
from oracle import cref
from structure_knowledge_distillation_amd import _lib, functional as SF
from structure_knowledge_distillation_amd import networks
from structure_knowledge_distillation_amd.networks.kd_model import NetModel, advance_versions_after_step, default_args

NAMES = ["skd_conv3x3_split2_pack_bytes", "skd_conv3x3_split2_pack_weights", "skd_conv3x3_split2_nhwc", "skd_conv1x1_abn2_nhwc",
         "skd_conv1x1_abn2_pro_nhwc"]


# ---- 1. the C ABI ------------------------------------------------------------------------------------------------------------

def test_split2_header_table_and_library_agree():
    """What is particular to skd_split2.h; header <-> table <-> library <-> build digest: tests/test_abi.py, for every header."""
    assert sorted(_lib.ABI["skd_split2.h"]) == sorted(NAMES) and len(NAMES) == 5
    # the parameter lists are the twins'
    for two, three in (("skd_conv3x3_split2_pack_bytes", "skd_conv3x3_split_pack_bytes"),
                       ("skd_conv3x3_split2_pack_weights", "skd_conv3x3_split_pack_weights"),
                       ("skd_conv3x3_split2_nhwc", "skd_conv3x3_split_nhwc"),
                       ("skd_conv1x1_abn2_nhwc", "skd_conv1x1_abn_nhwc"),
                       ("skd_conv1x1_abn2_pro_nhwc", "skd_conv1x1_abn_pro_nhwc")):
        assert _lib.signature(two) == _lib.signature(three), two
    assert all(three in _lib.ABI["skd_eval.h"] for three in ("skd_conv3x3_split_pack_bytes", "skd_conv3x3_split_pack_weights",
                                                             "skd_conv3x3_split_nhwc"))
    assert "skd_conv1x1_abn_nhwc" in _lib.SIGNATURES and "skd_conv1x1_abn_pro_nhwc" in _lib.SIGNATURES


def test_header_states_the_numerics():
    with open(_lib.header_path("skd_split2.h")) as fh:
        text = fh.read()
    for phrase in ("a0 b1,  a1 b0,  a0 b0", "a1 b1", "DROPPED", "2^24", "at most 8 significant bits", "3.39e38", "NaN"):
        assert phrase in text, phrase


def test_pack_bytes():
    lib = _lib.load()
    for cin, cout in ((16, 128), (32, 128), (256, 256), (512, 512), (2048, 512), (1024, 512)):
        assert lib.skd_conv3x3_split_supported(cin, cout, 1, 1, 1, 1)
        assert lib.skd_conv3x3_split2_pack_bytes(cin, cout) == 4 * cout * cin * 9
        assert 3 * lib.skd_conv3x3_split2_pack_bytes(cin, cout) == 2 * lib.skd_conv3x3_split_pack_bytes(cin, cout)
    for cin, cout in ((24, 128), (32, 64), (0, 128), (32, 0), (-16, 128), (32, 192 + 32)):
        assert not lib.skd_conv3x3_split_supported(cin, cout, 1, 1, 1, 1)
        assert lib.skd_conv3x3_split2_pack_bytes(cin, cout) == 0, (cin, cout)


def test_host_side_refusals():
    """Every refusal is decided on the host, in front of the launches: no device is touched (the pointers are never followed)."""
    lib = _lib.load()
    X, W_, OUT, PK, V = 0x10000, 0x2000000, 0x4000000, 0x8000000, 0xA000000
    nbytes = 4 * 128 * 32 * 9
    ok = dict(cin=32, cout=128, w=W_, sn=288, sc=9, sy=3, sx=1, pack=PK, nbytes=nbytes)
    for bad in (dict(w=None), dict(pack=None), dict(nbytes=nbytes - 1), dict(nbytes=0), dict(nbytes=-1), dict(pack=PK + 4),
                dict(pack=PK + 8), dict(sn=-1), dict(sc=-1), dict(sy=-1), dict(sx=-1), dict(cin=24), dict(cout=64), dict(cin=0),
                dict(cout=-128)):
        v = dict(ok, **bad)
        assert lib.skd_conv3x3_split2_pack_weights(v["cin"], v["cout"], v["w"], v["sn"], v["sc"], v["sy"], v["sx"], v["pack"],
                                                   v["nbytes"], None) == 0, bad
    ok = dict(B=1, H=4, W=5, cin=32, cout=128, d=2, x=X, pk=PK, out=OUT, mean=None, var=None, act=0, geo=0)
    for bad in (dict(x=None), dict(pk=None), dict(out=None), dict(x=X + 4), dict(x=X + 8), dict(pk=PK + 4), dict(B=0), dict(H=0),
                dict(W=-1), dict(cin=24), dict(cin=0), dict(cout=64), dict(cout=0), dict(d=0), dict(d=-1), dict(act=2), dict(act=4),
                dict(act=-1), dict(geo=4), dict(geo=-1), dict(mean=V), dict(var=V)):
        v = dict(ok, **bad)
        assert lib.skd_conv3x3_split2_nhwc(v["B"], v["H"], v["W"], v["cin"], v["cout"], v["d"], v["x"], v["pk"], v["out"], None,
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
                assert lib.skd_conv1x1_abn2_pro_nhwc(*head, v["pp"], v["act"], 0.01, None) == 0, bad
            else:
                assert lib.skd_conv1x1_abn2_nhwc(*head, v["act"], 0.01, None) == 0, bad


# ---- 2. the ops ----------------------------------------------------------------------------------------------------------------

class Split2Double:
    """The plain-C double for every core entry + the 1x1 entries of skd_split2.h, recorded and computed by the core's three-piece
    entries (a dot product in double: the wiring is what these tests look at), + the pack entries of both piece counts, which copy
    the fp32 weight into the head of the pack.  The three-piece 1x1 entries are recorded too."""

    def __init__(self):
        self._core = cref.load(_lib.SIGNATURES)
        self.two, self.three, self.packs = [], [], []

    def __getattr__(self, name):
        return getattr(self._core, name)

    def skd_conv1x1_abn2_nhwc(self, m, k, n, x, w, r, *rest):
        self.two.append(("1x1", k, n, False, r is not None))
        return self._core.skd_conv1x1_abn_nhwc(m, k, n, x, w, r, *rest)

    def skd_conv1x1_abn2_pro_nhwc(self, m, k, n, x, w, r, *rest):
        self.two.append(("1x1", k, n, True, r is not None))
        return self._core.skd_conv1x1_abn_pro_nhwc(m, k, n, x, w, r, *rest)

    def skd_conv1x1_abn_nhwc(self, m, k, n, x, w, r, *rest):
        self.three.append(("1x1", k, n, False, r is not None))
        return self._core.skd_conv1x1_abn_nhwc(m, k, n, x, w, r, *rest)

    def skd_conv1x1_abn_pro_nhwc(self, m, k, n, x, w, r, *rest):
        self.three.append(("1x1", k, n, True, r is not None))
        return self._core.skd_conv1x1_abn_pro_nhwc(m, k, n, x, w, r, *rest)

    def skd_conv3x3_split_pack_bytes(self, cin, cout):
        return cout * cin * 54

    def skd_conv3x3_split2_pack_bytes(self, cin, cout):
        return cout * cin * 36

    def _pack(self, pieces, cin, cout, w, sn, sc, sy, sx, pack, nbytes, stream):
        assert (sn, sc, sy, sx) == (cin * 9, 9, 3, 1) and nbytes == cout * cin * 18 * pieces
        ctypes.memmove(pack, w, cout * cin * 36)
        self.packs.append(pieces)
        return 1

    def skd_conv3x3_split_pack_weights(self, *args):
        return self._pack(3, *args)

    def skd_conv3x3_split2_pack_weights(self, *args):
        return self._pack(2, *args)

    def skd_conv3x3_split2_nhwc(self, *args):
        raise AssertionError("the 3x3 ops refuse host tensors: never reached under this double")


@pytest.fixture
def double():
    d = Split2Double()
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


def test_ops_take_pieces(double):
    torch.manual_seed(1)
    conv = torch.nn.Conv2d(64, 128, 1, bias=False)
    bn = PC.BatchNorm2d(128).eval()
    x = _cl(1, 64, 5, 6)
    call = lambda **kw: SF.conv1x1_abn_eval(x, conv.weight, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.eps, **kw)
    with torch.no_grad():
        three = call()
        assert double.three == [("1x1", 64, 128, False, False)] and double.two == []
        assert torch.equal(call(pieces=3), three) and len(double.three) == 2 and double.two == []
        two = call(pieces=2)
        assert double.two == [("1x1", 64, 128, False, False)] and len(double.three) == 2 and torch.equal(two, three)
        pro = SF.abn_pack_eval_params(PC.BatchNorm2d(64).eval())
        call(pieces=2, pro=pro, residual=torch.zeros_like(three))
        assert double.two[-1] == ("1x1", 64, 128, True, True)
        for bad in (1, 4, 0, None, "2", 2.5, 2.0, 3.0, True):
            with pytest.raises(ValueError):
                call(pieces=bad)
            with pytest.raises(ValueError):
                SF.conv3x3_pack_weights(torch.nn.Conv2d(16, 128, 3, 1, 1), pieces=bad)
            with pytest.raises(ValueError):
                SF.conv3x3_split_eval(_cl(1, 16, 4, 4), torch.zeros(16 * 128 * 36, dtype=torch.uint8), 128, pieces=bad)


def test_pieces_2_is_never_downgraded(c_double):
    """A back-end without the entries: the ops raise what the other ops raise for a missing entry."""
    conv = torch.nn.Conv2d(64, 128, 1, bias=False)
    bn = PC.BatchNorm2d(128).eval()
    x = _cl(1, 64, 5, 6)
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="skd_conv1x1_abn2_nhwc"):
            SF.conv1x1_abn_eval(x, conv.weight, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.eps, pieces=2)
        with pytest.raises(NotImplementedError, match="skd_conv1x1_abn2_pro_nhwc"):
            SF.conv1x1_abn_eval(x, conv.weight, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.eps, pieces=2,
                                pro=torch.zeros(4, 64))
        with pytest.raises(NotImplementedError, match="skd_conv3x3_split2_pack_weights"):
            SF.conv3x3_pack_weights(torch.nn.Conv2d(16, 128, 3, 1, 1), pieces=2)
        with pytest.raises(NotImplementedError, match="skd_conv3x3_split2_nhwc"):
            SF.conv3x3_split_eval(_cl(1, 16, 4, 4), torch.zeros(16 * 128 * 36, dtype=torch.uint8), 128, pieces=2)


def fused_sgd(params):
    params = list(params)
    try:
        opt = torch.optim.SGD(params, 0.5, fused=True)
    except (RuntimeError, TypeError, ValueError):      # a torch without fused SGD on the host: the plain form
        opt = torch.optim.SGD(params, 0.5)
    opt.register_step_post_hook(advance_versions_after_step)
    return opt


def test_both_packs_follow_a_fused_step(double):
    """The packs of both piece counts sit on one module under attributes of their own, each is made once per weight version, both
    are rebuilt behind a fused SGD step (with the step post-hook NetModel registers) and drop_conv3x3_packs forgets both."""
    torch.manual_seed(9)
    conv = torch.nn.Conv2d(16, 128, 3, 1, 1)
    head = 128 * 16 * 9 * 4
    with torch.no_grad():
        p3, p2 = SF.conv3x3_pack_weights(conv), SF.conv3x3_pack_weights(conv, pieces=2)
        assert SF.conv3x3_pack_weights(conv) is p3 and SF.conv3x3_pack_weights(conv, pieces=2) is p2 and double.packs == [3, 2]
        assert p3.numel() == 128 * 16 * 54 and p2.numel() == 128 * 16 * 36 == head
        assert hasattr(conv, "_skd_conv3x3_pack") and hasattr(conv, "_skd_conv3x3_pack2")
        for p in (p3, p2):
            assert torch.equal(p[:head].view(torch.float32), conv.weight.reshape(-1))
    opt = fused_sgd(conv.parameters())
    for p in conv.parameters():
        p.grad = torch.ones_like(p)
    version = conv.weight._version
    opt.step()
    assert conv.weight._version > version
    with torch.no_grad():
        q3, q2 = SF.conv3x3_pack_weights(conv), SF.conv3x3_pack_weights(conv, pieces=2)
        assert SF.conv3x3_pack_weights(conv) is q3 and SF.conv3x3_pack_weights(conv, pieces=2) is q2
        assert double.packs == [3, 2, 3, 2], "each re-packed once behind the step"
        for q, p in ((q3, p3), (q2, p2)):
            assert torch.equal(q[:head].view(torch.float32), conv.weight.reshape(-1)) and not torch.equal(q[:head], p[:head])
    SF.drop_conv3x3_packs(conv)
    assert not hasattr(conv, "_skd_conv3x3_pack") and not hasattr(conv, "_skd_conv3x3_pack2")
    cache = {"pack3x3": 1, "pack3x3_2": 2, "mats": 3}
    SF.drop_conv3x3_packs(cache)
    assert cache == {"mats": 3}


# ---- 3. routing ----------------------------------------------------------------------------------------------------------------

@pytest.fixture
def recording(double, monkeypatch):
    """``double`` + the 3x3 ops recorded at the op (the frozen 3x3 form refuses host tensors): conv3x3_pack_weights returns the
    weight with its piece count, conv3x3_split_eval computes ``F.conv2d`` + the module's own ABN.  The log is ``double.two`` /
    ``double.three``, in call order across both kernels."""
    def ok(x, w, s, p, d, g, grad, entries, query, host_ok):
        return (grad is False and not torch.is_grad_enabled() and SF._fp32_cl_map(x) and s == 1 and p == d and g == 1
                and w.shape[1] % 16 == 0 and w.shape[0] % 128 == 0)

    def pack(conv, weight=None, owner=None, pieces=3):
        return (pieces, conv.weight if weight is None else weight)

    def run(x, pk, cout, dilation=1, conv_bias=None, bn=None, activation="none", geometry=0, pieces=3):
        assert pk[0] == pieces, "the pack of the other piece count"
        (double.two if pieces == 2 else double.three).append(("3x3", x.shape[1], cout, dilation))
        y = F.conv2d(x, pk[1], conv_bias, 1, dilation, dilation).contiguous(memory_format=torch.channels_last)
        return y if bn is None else bn(y)
    blas = SF.conv1x1_bn_blas

    def blas_rec(x, conv, bn, relu):
        double.three.append(("blas", conv.in_channels, conv.out_channels))
        return blas(x, conv, bn, relu=relu)
    monkeypatch.setattr(SF, "_conv3x3_ok", ok)
    monkeypatch.setattr(SF, "conv3x3_pack_weights", pack)
    monkeypatch.setattr(SF, "conv3x3_split_eval", run)
    monkeypatch.setattr(SF, "conv1x1_bn_blas", blas_rec)
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


def _marked(net):
    return [type(m).__name__ for m in net.modules() if getattr(m, "_skd_teacher_pieces", 3) != 3]


def test_marked_stack_hands_exactly_its_split_core_calls_over(recording):
    net, x = _stack(), _cl(1, 512, 6, 7, seed=4)
    with torch.no_grad():
        want = net(x)
    assert recording.three == STACK_CALLS and recording.two == []
    recording.three.clear()
    assert networks.set_teacher_pieces(net) is net and _marked(net) == ["Bottleneck"] * 2
    with torch.no_grad():
        got = net(x)
    assert recording.two == STACK_CALLS and recording.three == []
    assert torch.equal(got, want), "the double computes both piece counts alike: the wiring is the same"
    # none in training mode, under grad, for an NCHW input
    recording.two.clear()
    net.train()
    with torch.no_grad():
        net(x)
    net.eval()
    net(x)
    nchw = copy.deepcopy(net).to(memory_format=torch.contiguous_format)     # (channels-last weights would give channels-last maps)
    with torch.no_grad():
        nchw(x.contiguous())
    assert recording.two == []
    # the mark cleared: three pieces again, and the two-plane pack is gone
    net[0].conv2._skd_conv3x3_pack2 = "a pack"
    recording.three.clear()
    networks.set_teacher_pieces(net, 3)
    assert _marked(net) == [] and not hasattr(net[0].conv2, "_skd_conv3x3_pack2")
    with torch.no_grad():
        net(x)
    assert recording.three == STACK_CALLS and recording.two == []
    for bad in (1, 4, None, "2", 2.0, 3.0, True):
        with pytest.raises(ValueError):
            networks.set_teacher_pieces(net, bad)


def test_reduce_512_128_keeps_the_library(recording):
    torch.manual_seed(5)
    block = PC.Bottleneck(512, 128).eval().to(memory_format=torch.channels_last)
    networks.set_teacher_pieces(block)
    with torch.no_grad():
        block(_cl(1, 512, 5, 5, seed=6))
    assert recording.three == [("blas", 512, 128)], "conv1 on the library GEMM, the 128-channel 3x3 on the library"
    assert recording.two == [("1x1", 128, 512, True, True)]


def test_excluded_shapes_keep_three_pieces(recording, monkeypatch):
    assert isinstance(PC.SPLIT2_ROUTING_EXCLUDED, frozenset)
    assert all(e[0] in ("1x1", "3x3") and len(e) == (3 if e[0] == "1x1" else 4) for e in PC.SPLIT2_ROUTING_EXCLUDED)
    net, x = networks.set_teacher_pieces(_stack()), _cl(1, 512, 6, 7, seed=4)
    monkeypatch.setattr(PC, "SPLIT2_ROUTING_EXCLUDED", frozenset({("1x1", 512, 1024), ("3x3", 256, 256, 2), ("1x1", 256, 1024)}))
    with torch.no_grad():
        net(x)
    assert recording.two == [("1x1", 512, 256, False, False), ("1x1", 1024, 256, False, False)]
    assert recording.three == [c for c in STACK_CALLS if c not in recording.two]


def test_teacher_marks_dsn_and_psp_and_a_student_is_untouched(recording):
    torch.manual_seed(7)
    teacher = PC.Res_pspnet(PC.Bottleneck, [3, 4, 23, 3], 19).eval().to(memory_format=torch.channels_last)
    networks.set_teacher_pieces(teacher, 2)
    assert sorted(set(_marked(teacher))) == ["Bottleneck", "PSPModule", "ResNet"] and len(_marked(teacher)) == 33 + 2
    with torch.no_grad():
        teacher._dsn_head(_cl(1, 1024, 5, 5, seed=8))
        assert recording.two == [("3x3", 1024, 512, 1)] and recording.three == []
        teacher.pspmodule(_cl(1, 2048, 6, 6, seed=9))
        assert recording.two == [("3x3", 1024, 512, 1), ("3x3", 2048, 512, 1)] and recording.three == []
        assert "pack3x3_2" in teacher.pspmodule._fold_cache and "pack3x3" not in teacher.pspmodule._fold_cache
    networks.set_teacher_pieces(teacher, 3)
    assert _marked(teacher) == [] and "pack3x3_2" not in teacher.pspmodule._fold_cache
    with torch.no_grad():
        teacher.pspmodule(_cl(1, 2048, 6, 6, seed=9))
    assert recording.three == [("3x3", 2048, 512, 1)]
    # a BasicBlock network (the student): no mark anywhere, nothing handed over in its frozen forward
    recording.two.clear()
    recording.three.clear()
    student = PC.Res_pspnet(PC.BasicBlock, [2, 2, 2, 2], 19).eval().to(memory_format=torch.channels_last)
    networks.set_teacher_pieces(student, 2)
    assert _marked(student) == []
    with torch.no_grad():
        student(_cl(1, 3, 33, 33, seed=10))
    assert recording.two == []


def test_backend_without_the_entries_warns_and_keeps_three_pieces(c_double):
    net = _stack()
    with pytest.warns(RuntimeWarning, match="three pieces"):
        assert networks.set_teacher_pieces(net, 2) is net
    assert _marked(net) == []
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        networks.set_teacher_pieces(net, 3)


# ---- 4. the public switch --------------------------------------------------------------------------------------------------------

def test_default_args_and_the_environment(monkeypatch):
    monkeypatch.delenv("SKD_TEACHER_PIECES", raising=False)
    assert default_args().teacher_pieces == 3 and default_args(teacher_pieces=2).teacher_pieces == 2
    monkeypatch.setenv("SKD_TEACHER_PIECES", "2")
    assert default_args().teacher_pieces == 2 and default_args(teacher_pieces=3).teacher_pieces == 3
    assert default_args().split_train is False and default_args().split_shortcut is False      # independent of the five
    monkeypatch.setenv("SKD_TEACHER_PIECES", "3")
    assert default_args().teacher_pieces == 3
    for bad in ("1", "4", "", "two", "2.0"):
        monkeypatch.setenv("SKD_TEACHER_PIECES", bad)
        with pytest.raises(ValueError):
            default_args()
    monkeypatch.delenv("SKD_TEACHER_PIECES")
    for bad in (1, 4, 0, "x", True):
        with pytest.raises(ValueError):
            default_args(teacher_pieces=bad)


def test_netmodel_marks_the_teacher_alone(double, monkeypatch):
    for name in ("SKD_TEACHER_PIECES", "SKD_SPLIT_TRAIN", "SKD_SPLIT_WGRAD", "SKD_SPLIT_NARROW", "SKD_SPLIT_NARROW_WGRAD",
                 "SKD_SPLIT_SHORTCUT"):
        monkeypatch.delenv(name, raising=False)
    kw = dict(device=torch.device("cpu"), batch_size=2, ho=False)
    model = NetModel(default_args(**kw))
    assert model.teacher_pieces == 3 and _marked(model.teacher) == [] and _marked(model.student) == []
    model = NetModel(default_args(teacher_pieces=2, **kw))
    assert model.teacher_pieces == 2 and len(_marked(model.teacher)) == 35 and _marked(model.student) == []
    assert not model.split_train and not model.split_shortcut
    monkeypatch.setenv("SKD_TEACHER_PIECES", "2")
    model = NetModel(default_args(split_train=True, **kw))
    assert len(_marked(model.teacher)) == 35 and _marked(model.student) == [] and model.split_train
    # on a back-end without the entries: the warning, and three pieces
    _lib.install_test_backend(cref.load(_lib.SIGNATURES))
    with pytest.warns(RuntimeWarning, match="three pieces"):
        model = NetModel(default_args(**kw))
    assert _marked(model.teacher) == []


def test_docs_name_the_mode():
    assert "skd_split2.h" in SF.conv1x1_abn_eval.__doc__ and "skd_split2.h" in SF.conv3x3_split_eval.__doc__
    assert "skd_split2.h" in SF.conv3x3_pack_weights.__doc__ and "SPLIT2_ROUTING_EXCLUDED" in PC.set_teacher_pieces.__doc__


# ---- 5. the model itself ---------------------------------------------------------------------------------------------------------

def test_two_pieces_carry_sixteen_bits():
    g = torch.Generator().manual_seed(1)
    for bits in (1, 8, 9, 15, 16):
        v = torch.randint(-(2 ** bits) + 1, 2 ** bits, (4096,), generator=g).float() * torch.exp2(
            torch.randint(-30, 31, (4096,), generator=g).float())
        p0, p1 = R.pieces(v, 2)
        assert torch.equal(p0 + p1, v.double()), bits
        if bits <= 8:
            assert not bool(p1.any())
    # (the second piece is signed, so 17 bits survive as well); 19 bits: not every value does, and the residual is below 2^-17 |v|
    v = torch.randint(2 ** 18 + 1, 2 ** 19, (4096,), generator=g).float()
    p0, p1 = R.pieces(v, 2)
    assert not torch.equal(p0 + p1, v.double()) and float((p0 + p1 - v.double()).abs().max()) <= 2.0 ** (19 - 17)
    p = R.pieces(torch.randn(4096, generator=g), 3)
    assert torch.equal(p[0], R.pieces(p[0] + p[1] + p[2], 2)[0]) and len(p) == 3


def test_three_product_model_against_the_exact_product():
    g = torch.Generator().manual_seed(2)
    a8 = torch.randint(-255, 256, (37, 64), generator=g).float()            # one piece
    b16 = torch.randint(-65535, 65536, (128, 64), generator=g).float()      # two pieces
    want = a8.double() @ b16.double().t()
    assert torch.equal(R.mm_split2(a8, b16), want) and torch.equal(R.mm_split2(b16, a8), want.t())
    a16 = torch.randint(-65535, 65536, (37, 64), generator=g).float()
    both = R.mm_split2(a16, b16)
    exact = a16.double() @ b16.double().t()
    pa, pb = R.pieces(a16, 2), R.pieces(b16, 2)
    assert torch.equal(exact - both, pa[1] @ pb[1].t()) and bool((exact != both).any()), "exactly a1 b1 is missing"
    assert torch.equal(R.mm_split2(a16, b16, 3), exact)
    x = torch.randint(0, 8, (2, 16, 7, 6), generator=g).float()
    w = torch.randint(-1000, 1001, (128, 16, 3, 3), generator=g).float()
    assert torch.equal(R.conv2d_split2(x, w, None, 1, 2, 2), F.conv2d(x.double(), w.double(), None, 1, 2, 2))
    bias = torch.randn(128, generator=g)
    assert torch.equal(R.conv2d_split2(x, w, bias, 1, 1, 1), F.conv2d(x.double(), w.double(), bias.double(), 1, 1, 1))
