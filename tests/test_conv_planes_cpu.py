"""Piece planes (include/skd_planes.h), the parts that need no GPU: the C ABI (the names and the twins' argument lists; the rest is tests/test_abi.py), the layout as the host-only offset map gives it, the host-side refusals, the routing of
``route_teacher_planes`` under a recording double, the ``teacher_planes`` switch and the documents.

The routing tests empty ``PLANES_ROUTING_EXCLUDED``: they check the mechanism, the set is the policy (one test reads the committed
set and sees it respected)."""
import ctypes
import inspect
import os
import warnings

import pytest
import torch
import torch.nn.functional as F

from oracle import cref
from structure_knowledge_distillation_amd import _lib, functional as SF, networks
from structure_knowledge_distillation_amd.networks import kd_model, pspnet_combine as PC
from structure_knowledge_distillation_amd.networks.kd_model import NetModel, default_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["skd_planes_supported", "skd_planes_bytes", "skd_planes_offset", "skd_planes_split_nhwc", "skd_planes_join_nhwc",
         "skd_conv1x1_abn_planes_nhwc", "skd_conv3x3_split_planes_nhwc"]
HOST_ONLY = NAMES[:3]


# ---- 1. the C ABI ------------------------------------------------------------------------------------------------------------------

def test_header_table_and_library_agree():
    """What is particular to skd_planes.h; header <-> table <-> library <-> build digest: tests/test_abi.py, for every header."""
    table = _lib.ABI["skd_planes.h"]
    assert sorted(table) == sorted(NAMES) and len(table) == 7
    # the consumer takes its twin's arguments (dilation moved behind the epilogue), the producer its twin's without the residual
    twin = _lib.signature("skd_conv3x3_split_nhwc")[1]
    assert sorted(map(str, table["skd_conv3x3_split_planes_nhwc"][1])) == sorted(map(str, twin))
    assert len(table["skd_conv1x1_abn_planes_nhwc"][1]) == len(_lib.signature("skd_conv1x1_abn_nhwc")[1]) - 1


# ---- 2. the layout -----------------------------------------------------------------------------------------------------------------

def _i64():
    v = ctypes.c_int64(-7)
    return v, ctypes.cast(ctypes.byref(v), ctypes.c_void_p)


@pytest.mark.parametrize("c", [16, 48, 256])
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65])
def test_offset_map_is_injective_aligned_and_inside(m, c):
    lib = _lib.load()
    size, ref = _i64()
    assert lib.skd_planes_supported(c) == 1 and lib.skd_planes_bytes(m, c, ref) == 1
    nbytes = size.value
    assert nbytes >= 6 * m * c and nbytes % 16 == 0
    off, oref = _i64()
    seen = set()
    for row in range(m):
        for ch in range(c):
            for piece in range(3):
                assert lib.skd_planes_offset(m, c, row, ch, piece, oref) == 1
                assert off.value % 2 == 0 and 0 <= off.value <= nbytes - 2, (row, ch, piece, off.value)
                seen.add(off.value)
    assert len(seen) == 3 * m * c, "two (row, channel, piece) share a bf16 slot"


# ---- 3. host-side refusals, no device ---------------------------------------------------------------------------------------------

def test_host_side_refusals():
    lib = _lib.load()
    for c, ok in ((16, 1), (32, 1), (2048, 1), (0, 0), (-16, 0), (8, 0), (24, 0), (100, 0)):
        assert lib.skd_planes_supported(c) == ok, c
    size, ref = _i64()
    for m, c, p in ((0, 16, ref), (-1, 16, ref), (4, 24, ref), (4, 0, ref), (4, 16, None), ((1 << 40) + 1, 16, ref)):
        assert lib.skd_planes_bytes(m, c, p) == 0, (m, c)
    assert size.value == -7, "a refused query wrote its result"
    off, oref = _i64()
    for m, c, row, ch, piece, p in ((4, 16, 4, 0, 0, oref), (4, 16, -1, 0, 0, oref), (4, 16, 0, 16, 0, oref), (4, 16, 0, -1, 0, oref),
                                    (4, 16, 0, 0, 3, oref), (4, 16, 0, 0, -1, oref), (4, 24, 0, 0, 0, oref), (0, 16, 0, 0, 0, oref),
                                    (4, 16, 0, 0, 0, None)):
        assert lib.skd_planes_offset(m, c, row, ch, piece, p) == 0, (m, c, row, ch, piece)
    assert off.value == -7
    # the device entries refuse these before they touch a device: host buffers stand in for the pointers
    buf = torch.zeros(1 << 16, dtype=torch.uint8)
    base = (buf.data_ptr() + 15) // 16 * 16
    a, b, c3 = base, base + 4096, base + 8192
    for entry in ("skd_planes_split_nhwc", "skd_planes_join_nhwc"):
        fn = getattr(lib, entry)
        for m, c, p, q in ((0, 16, a, b), (4, 24, a, b), (4, 0, a, b), (4, 16, None, b), (4, 16, a, None), (4, 16, a + 4, b), (4, 16, a, b + 8)):
            assert fn(m, c, p, q, None) == 0, (entry, m, c)
    vecs = (a, a, None, None, 1e-5)
    for m, k, n, x, w, out, act in ((0, 16, 128, a, b, c3, 3), (4, 24, 128, a, b, c3, 3), (4, 16, 64, a, b, c3, 3), (4, 16, 128, None, b, c3, 3),
                                    (4, 16, 128, a, None, c3, 3), (4, 16, 128, a, b, None, 3), (4, 16, 128, a + 4, b, c3, 3),
                                    (4, 16, 128, a, b, c3 + 8, 3), (4, 16, 128, a, b, c3, 2), (4, 16, 128, a, b, c3, 9)):
        assert lib.skd_conv1x1_abn_planes_nhwc(m, k, n, x, w, out, *vecs, act, 0.01, None) == 0, (m, k, n, act)
    assert lib.skd_conv1x1_abn_planes_nhwc(4, 16, 128, a, b, c3, None, a, None, None, 1e-5, 3, 0.01, None) == 0
    good = dict(b=1, h=3, w=3, cin=16, cout=128, src=a, pk=b, out=c3, mean=None, var=None, act=0, d=1, geo=0)
    for bad in (dict(cin=24), dict(cin=0), dict(cout=64), dict(b=0), dict(h=0), dict(w=0), dict(d=0), dict(src=None), dict(pk=None),
                dict(out=None), dict(src=a + 8), dict(pk=b + 8), dict(h=65536, w=32768), dict(geo=4), dict(geo=-1), dict(act=2),
                dict(mean=a), dict(var=a)):
        g = dict(good, **bad)
        assert lib.skd_conv3x3_split_planes_nhwc(g["b"], g["h"], g["w"], g["cin"], g["cout"], g["src"], g["pk"], g["out"], None, g["mean"],
                                                 g["var"], None, None, 0.0, g["act"], 0.01, g["d"], g["geo"], None) == 0, bad
    assert not bool(buf.any()), "a refused call wrote"


# ---- 4. routing under a recording double ------------------------------------------------------------------------------------------

class PlanesDouble:
    """The plain-C double for every core entry + the seven entries of skd_planes.h, recorded.  Its planes are the fp32 map in the
    head of the buffer (4 of the 6 bytes per element): the producer is the core's fp32 GEMM writing there.  The fp32 1x1 entries are
    recorded too; the 3x3 ops are recorded at the op (``recording``: the frozen 3x3 form refuses host tensors)."""

    def __init__(self):
        self._core = cref.load(_lib.SIGNATURES)
        self.log = []

    def __getattr__(self, name):
        return getattr(self._core, name)

    def skd_planes_supported(self, c):
        return int(c >= 1 and c % 16 == 0)

    def skd_planes_bytes(self, m, c, out):
        if m < 1 or not self.skd_planes_supported(c):
            return 0
        ctypes.cast(out, ctypes.POINTER(ctypes.c_int64))[0] = 6 * m * c
        return 1

    def _never(self, *args):
        raise AssertionError("routing never calls this entry")
    skd_planes_offset = skd_planes_split_nhwc = skd_planes_join_nhwc = _never

    def skd_conv3x3_split_planes_nhwc(self, *args):
        raise AssertionError("the 3x3 ops are recorded at the op under this double")

    def skd_conv1x1_abn_planes_nhwc(self, m, k, n, x, w, planes, *rest):
        self.log.append(("planes 1x1", k, n))
        return self._core.skd_conv1x1_abn_nhwc(m, k, n, x, w, None, planes, *rest)

    def skd_conv1x1_abn_nhwc(self, m, k, n, x, w, r, *rest):
        self.log.append(("1x1", k, n))
        return self._core.skd_conv1x1_abn_nhwc(m, k, n, x, w, r, *rest)

    def skd_conv3x3_split_pack_bytes(self, cin, cout):
        return cout * cin * 54


class NoPlanesDouble(PlanesDouble):
    """The same without the planes entries: a back-end that lacks them."""

    def __getattribute__(self, name):
        if name in NAMES:
            raise AttributeError(name)
        return object.__getattribute__(self, name)


def _install(double, monkeypatch):
    def ok(x, w, s, p, d, g, grad, entries, query, host_ok):
        return (grad is False and not torch.is_grad_enabled() and SF._fp32_cl_map(x) and s == 1 and p == d and g == 1
                and w.shape[1] % 16 == 0 and w.shape[0] % 128 == 0)

    def pack(conv, weight=None, owner=None, pieces=3):
        return (pieces, conv.weight if weight is None else weight)

    def run(x, pk, cout, dilation=1, conv_bias=None, bn=None, activation="none", geometry=0, pieces=3):
        assert pk[0] == pieces == 3
        if isinstance(x, SF.Planes):
            b, h, w, c = x.shape
            assert x.M == b * h * w and x.C == c == pk[1].shape[1] and x.data.numel() == 6 * x.M * c and x.data.dtype == torch.uint8
            double.log.append(("planes 3x3", c, cout, dilation))
            x = x.data[:4 * x.M * c].view(torch.float32).view(b, h, w, c).permute(0, 3, 1, 2)
        else:
            double.log.append(("3x3", x.shape[1], cout, dilation))
        y = F.conv2d(x, pk[1], conv_bias, 1, dilation, dilation).contiguous(memory_format=torch.channels_last)
        return y if bn is None else bn(y)
    monkeypatch.setattr(SF, "_conv3x3_ok", ok)
    monkeypatch.setattr(SF, "conv3x3_pack_weights", pack)
    monkeypatch.setattr(SF, "conv3x3_split_eval", run)
    monkeypatch.setattr(PC, "PLANES_ROUTING_EXCLUDED", frozenset())
    _lib.install_test_backend(double)
    return double


@pytest.fixture
def recording(monkeypatch):
    yield _install(PlanesDouble(), monkeypatch)
    _lib.install_test_backend(None)


@pytest.fixture
def without_entries(monkeypatch):
    yield _install(NoPlanesDouble(), monkeypatch)
    _lib.install_test_backend(None)


def _cl(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).contiguous(memory_format=torch.channels_last)


def _seed_bn(net):
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, PC.InPlaceABNSync):
                m.running_var.uniform_(0.5, 1.5)
                m.running_mean.normal_(0, 0.1)
    return net.eval().to(memory_format=torch.channels_last)


def _stack():
    """Two Bottlenecks of layer3's shapes (512 -> 256 with a down-sample branch, 1024 -> 256, 3x3 at dilation 2) and layer2's
    512 -> 128, whose reduce GEMM is the library's."""
    torch.manual_seed(3)
    down = torch.nn.Sequential(torch.nn.Conv2d(512, 1024, 1, 1, bias=False), PC.BatchNorm2d(1024))
    back = torch.nn.Sequential(torch.nn.Conv2d(1024, 512, 1, 1, bias=False), PC.BatchNorm2d(512))
    return _seed_bn(torch.nn.Sequential(PC.Bottleneck(512, 256, 1, dilation=2, downsample=down), PC.Bottleneck(1024, 256, dilation=2),
                                        PC.Bottleneck(1024, 128, downsample=back)))


LINKED = [("planes 1x1", 512, 256), ("planes 3x3", 256, 256, 2), ("planes 1x1", 1024, 256), ("planes 3x3", 256, 256, 2)]
UNLINKED = [("1x1", 512, 256), ("3x3", 256, 256, 2), ("1x1", 1024, 256), ("3x3", 256, 256, 2)]


def _link_calls(log):
    """The calls of the first two blocks' conv1 and conv2, in order (the tails, the down-sample branches and the third block's
    library reduce are not the link's business)."""
    return [c for c in log if c in LINKED + UNLINKED]


def test_flagged_stack_hands_the_link_over(recording):
    net, x = _stack(), _cl(1, 512, 6, 7, seed=4)
    with torch.no_grad():
        want = net(x)
    assert _link_calls(recording.log) == UNLINKED and not any(c[0].startswith("planes") for c in recording.log)
    plain = list(recording.log)
    recording.log.clear()
    assert networks.route_teacher_planes(net) is net and all(getattr(b, "_skd_teacher_planes", False) for b in net)
    with torch.no_grad():
        got = net(x)
    assert _link_calls(recording.log) == LINKED
    # everything else is call for call what it was: the third block (512 -> 128 is the library's reduce, 128 channels are not the
    # wide kernel's), the tails, the down-sample branches
    swap = dict(zip(LINKED[:2] + LINKED[2:], UNLINKED[:2] + UNLINKED[2:]))
    assert [swap.get(c, c) for c in recording.log] == plain
    assert torch.equal(got, want), "the double's planes are the fp32 map: the wiring is the same"
    # no planes call in training mode, under grad, for a block marked for two pieces, for an unflagged network
    for setup in ("train", "grad", "two", "unflagged"):
        recording.log.clear()
        if setup == "train":
            net.train()
            with torch.no_grad():
                net(x)
            net.eval()
        elif setup == "grad":
            net(x)
        elif setup == "two":
            # (the two-piece 1x1 entries are not this double's: only the decision is looked at)
            link = lambda: [PC._planes_link(b, t)[0] for b, t in ((net[0], x), (net[1], _cl(1, 1024, 6, 7)))]
            with torch.no_grad():
                for b in net:
                    b._skd_teacher_pieces = 2
                assert link() == [False, False]
                for b in net:
                    del b._skd_teacher_pieces
                assert link() == [True, True]
            assert link() == [False, False], "under grad"
        else:
            networks.route_teacher_planes(net, enable=False)
            assert not any(hasattr(b, "_skd_teacher_planes") for b in net)
            with torch.no_grad():
                net(x)
        assert not any(c[0].startswith("planes") for c in recording.log), setup


def test_excluded_shapes_keep_the_fp32_link(recording, monkeypatch):
    net, x = networks.route_teacher_planes(_stack()), _cl(1, 512, 6, 7, seed=4)
    monkeypatch.setattr(PC, "PLANES_ROUTING_EXCLUDED", frozenset({(1024, 256, 2)}))
    with torch.no_grad():
        net(x)
    assert _link_calls(recording.log) == LINKED[:2] + UNLINKED[2:]
    # the committed policy: a frozenset of (conv1 Cin, planes, dilation), respected
    monkeypatch.undo()
    _lib.install_test_backend(recording)
    assert isinstance(PC.PLANES_ROUTING_EXCLUDED, frozenset) and all(len(e) == 3 for e in PC.PLANES_ROUTING_EXCLUDED)
    for block, cin in ((net[0], 512), (net[1], 1024)):
        want = (cin, 256, 2) not in PC.PLANES_ROUTING_EXCLUDED
        # (the 3x3 predicate is the real one again and refuses host tensors: the link needs it, so only exclusion is visible here)
        assert PC._planes_link(block, _cl(1, cin, 6, 7))[0] is False or want


def test_decision_is_made_once_per_convolution(recording, monkeypatch):
    """_frozen_form is asked about conv2 exactly once per block, flagged or not, linked or not."""
    net, x = _stack(), _cl(1, 512, 6, 7, seed=4)
    asked = []
    real = PC._frozen_form

    def counting(module, t, conv, *args, **kw):
        asked.append(conv)
        return real(module, t, conv, *args, **kw)
    monkeypatch.setattr(PC, "_frozen_form", counting)
    for flagged in (False, True):
        networks.route_teacher_planes(net, enable=flagged)
        asked.clear()
        with torch.no_grad():
            net(x)
        assert [id(c) for c in asked] == [id(b.conv2) for b in net], flagged


def test_flagged_teacher_issues_26_pairs(recording):
    torch.manual_seed(7)
    teacher = _seed_bn(PC.Res_pspnet(PC.Bottleneck, [3, 4, 23, 3], 19))
    x = _cl(1, 3, 33, 33, seed=10)
    with torch.no_grad():
        want = teacher(x)
    plain = list(recording.log)
    assert not any(c[0].startswith("planes") for c in plain)
    recording.log.clear()
    networks.route_teacher_planes(teacher)
    assert sum(getattr(m, "_skd_teacher_planes", False) for m in teacher.modules()) == 33
    with torch.no_grad():
        got = teacher(x)
    log = recording.log
    producers, consumers = [c for c in log if c[0] == "planes 1x1"], [c for c in log if c[0] == "planes 3x3"]
    assert len(producers) == len(consumers) == 26
    assert producers == [("planes 1x1", 512, 256)] + [("planes 1x1", 1024, 256)] * 22 + [("planes 1x1", 1024, 512)] + [("planes 1x1", 2048, 512)] * 2
    assert consumers == [("planes 3x3", 256, 256, 2)] * 23 + [("planes 3x3", 512, 512, 4)] * 3
    # no fp32 reduce and no fp32 3x3 call is left for those blocks, and every other call is what it was
    gone = lambda c: (c[0] == "1x1" and c[1:] in {p[1:] for p in producers}) or (c[0] == "3x3" and c[1:] in {q[1:] for q in consumers})
    assert not any(gone(c) for c in log)
    assert [c for c in log if not c[0].startswith("planes")] == [c for c in plain if not gone(c)]
    assert len(plain) == len(log)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    # a BasicBlock network (the student) is left untouched
    student = PC.Res_pspnet(PC.BasicBlock, [2, 2, 2, 2], 19)
    assert networks.route_teacher_planes(student) is student
    assert not any(hasattr(m, "_skd_teacher_planes") for m in student.modules())


def test_backend_without_the_entries_warns_once_and_keeps_the_old_calls(without_entries):
    net, x = _stack(), _cl(1, 512, 6, 7, seed=4)
    assert not SF.planes_supported()
    with pytest.warns(RuntimeWarning, match="skd_planes.h") as caught:
        assert networks.route_teacher_planes(net) is net
    assert len(caught) == 1 and not any(hasattr(b, "_skd_teacher_planes") for b in net)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        networks.route_teacher_planes(net, enable=False)
        with torch.no_grad():
            net(x)
    assert _link_calls(without_entries.log) == UNLINKED
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="skd_planes.h"):
            SF.conv1x1_abn_planes_eval(x, net[0].conv1.weight, net[0].bn1.running_mean, net[0].bn1.running_var, None, None)
        with pytest.raises(NotImplementedError, match="skd_planes.h"):
            SF.planes_split(x)


def test_ops_take_and_return_planes(recording):
    net, x = _stack(), _cl(1, 512, 6, 7, seed=4)
    bn = net[0].bn1
    args = (x, net[0].conv1.weight, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.eps, "relu")
    with torch.no_grad():
        planes, fp32 = SF.conv1x1_abn_planes_eval(*args), SF.conv1x1_abn_eval(*args)
        assert isinstance(planes, SF.Planes) and planes.shape == (1, 6, 7, 256) and (planes.M, planes.C) == (42, 256)
        assert planes.data.dtype == torch.uint8 and planes.data.numel() == SF.planes_bytes(42, 256) == 6 * 42 * 256
        assert torch.equal(planes.data[:4 * 42 * 256].view(torch.float32).view(1, 6, 7, 256).permute(0, 3, 1, 2), fp32)
        # conv1x1_abn_eval keeps the signature the routing census records call by call: the planes form is an op of its own
        assert "planes_out" not in inspect.signature(SF.conv1x1_abn_eval).parameters
        with pytest.raises(ValueError):
            SF.planes_bytes(4, 24)


# ---- 5. the switch -----------------------------------------------------------------------------------------------------------------

def test_default_args_and_the_environment(monkeypatch):
    monkeypatch.delenv("SKD_TEACHER_PLANES", raising=False)
    assert default_args().teacher_planes is False and default_args(teacher_planes=True).teacher_planes is True
    monkeypatch.setenv("SKD_TEACHER_PLANES", "1")
    assert default_args().teacher_planes is True and default_args(teacher_planes=False).teacher_planes is False
    assert default_args().teacher_early is False and default_args().split_train is False and default_args().teacher_pieces == 3
    monkeypatch.setenv("SKD_TEACHER_PLANES", "0")
    assert default_args().teacher_planes is False and default_args(teacher_planes=True).teacher_planes is True
    assert len(kd_model.SWITCHES) == 9 and not any(name == "teacher_planes" for name, _, _ in kd_model.SWITCHES)


def _flagged(net):
    return sum(bool(getattr(m, "_skd_teacher_planes", False)) for m in net.modules())


def test_netmodel_flags_the_teacher_alone(recording, monkeypatch):
    for name in ("SKD_TEACHER_PLANES", "SKD_TEACHER_PIECES", "SKD_TEACHER_EARLY", "SKD_SPLIT_TRAIN"):
        monkeypatch.delenv(name, raising=False)
    kw = dict(device=torch.device("cpu"), batch_size=2, ho=False)
    model = NetModel(default_args(**kw))
    assert model.teacher_planes is False and _flagged(model.teacher) == 0 and _flagged(model.student) == 0
    model = NetModel(default_args(teacher_planes=True, **kw))
    assert model.teacher_planes is True and _flagged(model.teacher) == 33 and _flagged(model.student) == 0
    assert not model.teacher_early and not model.split_train and model.teacher_pieces == 3
    monkeypatch.setenv("SKD_TEACHER_PLANES", "1")
    model = NetModel(default_args(teacher_early=True, **kw))
    assert model.teacher_planes and model.teacher_early and _flagged(model.teacher) == 33
    model = NetModel(default_args(teacher_planes=False, **kw))
    assert not model.teacher_planes and _flagged(model.teacher) == 0
    # on a back-end without the entries: one warning that names the header, and the present path
    _lib.install_test_backend(NoPlanesDouble())
    with pytest.warns(RuntimeWarning, match="skd_planes.h") as caught:
        model = NetModel(default_args(**kw))
    assert len([w for w in caught if "skd_planes.h" in str(w.message)]) == 1
    assert model.teacher_planes is False and _flagged(model.teacher) == 0


# ---- 6. the documents ----------------------------------------------------------------------------------------------------------------

def test_documents_name_the_header_and_the_switch():
    for doc in ("README.md", "DESIGN.md"):
        with open(os.path.join(ROOT, doc)) as fh:
            text = fh.read()
        for word in ("skd_planes.h", "SKD_TEACHER_PLANES", "route_teacher_planes", "PLANES_ROUTING_EXCLUDED"):
            assert word in text, (doc, word)
    with open(os.path.join(ROOT, "DESIGN.md")) as fh:
        assert "7.14" in fh.read()
    for fn in (SF.conv1x1_abn_eval, SF.conv1x1_abn_planes_eval, SF.conv3x3_split_eval, SF.Planes, networks.route_teacher_planes, PC._planes_link):
        assert "skd_planes.h" in fn.__doc__, fn
    assert "SKD_TEACHER_PLANES" in kd_model._teacher_planes.__doc__
    with open(_lib.header_path("skd_planes.h")) as fh:
        header = fh.read()
    assert "SKD_TEACHER_PLANES" in header and "BIT FOR BIT" in header and "skd_planes_offset" in header
