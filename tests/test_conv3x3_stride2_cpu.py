"""The stride-2 forward form of the split-core 3x3 convolution and the frozen teacher's early routing, the parts that need no GPU:
the C ABI of include/skd_stride2.h (the pinned names and argument lists, the truth table of the query, the host-side refusals),
the kernel's row map swept on the host against a numpy restatement, the routing of a teacher flagged by ``route_teacher_early`` and
of a student flagged by ``fuse_for_inference(stride2=True)`` (a torch-implemented double of the entries on raw host addresses,
on top of the plain-C double), the wiring against the plain op sequence, the public switches and the packs behind a fused
optimizer step."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import structure_knowledge_distillation_amd.networks.pspnet_combine as PC
from oracle import cref
from structure_knowledge_distillation_amd import _lib, build, functional as SF
from structure_knowledge_distillation_amd import networks
from structure_knowledge_distillation_amd.networks import evaluate
from structure_knowledge_distillation_amd.networks.kd_model import NetModel, advance_versions_after_step, default_args
from test_conv3x3_narrow_cpu import NARROW, NarrowDouble
from test_student_infer_cpu import ENTRY, _host

SUPPORTED, TAPS, S2 = "skd_conv3x3_split_s2_supported", "skd_conv3x3_split_s2_taps", "skd_conv3x3_split_s2_nhwc"
SPLIT2 = "skd_conv3x3_split2_nhwc"


# ---- 1. the C ABI ------------------------------------------------------------------------------------------------------------

def test_stride2_header_table_and_library_agree():
    """What is particular to skd_stride2.h; header <-> table <-> library <-> build digest: tests/test_abi.py, for every header."""
    assert sorted(_lib.ABI["skd_stride2.h"]) == sorted([SUPPORTED, TAPS, S2]) and len(_lib.ABI["skd_stride2.h"]) == 3
    # the argument list of the stride-1 entry without ``dilation``, with ``pieces`` in front of ``geometry``
    one = list(_lib.signature(ENTRY)[1])
    assert _lib.signature(S2)[1] == one[:5] + one[6:17] + [ctypes.c_int] + one[17:]
    assert _lib.signature(SUPPORTED) == _lib.signature("skd_conv3x3_split_supported")


def test_supported_truth_table():
    sup = _lib.load().skd_conv3x3_split_s2_supported
    for cin, cout in ((16, 128), (64, 128), (128, 128), (32, 256), (48, 384), (256, 512)):
        assert sup(cin, cout, 2, 1, 1, 1) == 1, (cin, cout)
    for bad in ((64, 64, 2, 1, 1, 1), (64, 192, 2, 1, 1, 1), (24, 128, 2, 1, 1, 1), (8, 128, 2, 1, 1, 1), (0, 128, 2, 1, 1, 1),
                (64, 0, 2, 1, 1, 1), (-64, 128, 2, 1, 1, 1), (64, -128, 2, 1, 1, 1), (64, 128, 1, 1, 1, 1), (64, 128, 3, 1, 1, 1),
                (64, 128, 0, 1, 1, 1), (64, 128, 2, 0, 1, 1), (64, 128, 2, 2, 1, 1), (64, 128, 2, 2, 2, 1), (64, 128, 2, 1, 2, 1),
                (64, 128, 2, 1, 0, 1), (64, 128, 2, 1, 1, 2), (64, 128, 2, 1, 1, 0)):
        assert sup(*bad) == 0, bad
    # the stride-1 predicates keep refusing stride 2
    lib = _lib.load()
    assert lib.skd_conv3x3_split_supported(64, 128, 2, 1, 1, 1) == 0 and lib.skd_conv3x3_narrow_supported(64, 64, 2, 1, 1, 1) == 0


def test_host_side_refusals():
    """Every refusal is decided on the host, in front of the launch: no device is touched (the pointers are never followed)."""
    lib = _lib.load()
    X, PK, OUT, V = 0x10000, 0x8000000, 0x4000000, 0xA000000
    ok = dict(B=1, H=5, W=4, cin=32, cout=128, x=X, pk=PK, out=OUT, mean=None, var=None, act=0, pieces=3, geo=0)
    for bad in (dict(x=None), dict(pk=None), dict(out=None), dict(x=X + 4), dict(x=X + 8), dict(pk=PK + 4), dict(pk=PK + 8), dict(B=0),
                dict(H=0), dict(W=-1), dict(cin=24), dict(cin=0), dict(cout=64), dict(cout=0), dict(cout=192), dict(act=1), dict(act=2),
                dict(act=4), dict(act=-1), dict(geo=4), dict(geo=-1), dict(mean=V), dict(var=V), dict(pieces=1), dict(pieces=4),
                dict(pieces=0), dict(pieces=-2), dict(H=65536, W=32768),
                # the same with the other piece count and the other epilogue
                dict(pieces=2, x=None), dict(pieces=2, cout=64), dict(pieces=2, geo=4), dict(pieces=2, act=1), dict(act=3, var=V),
                dict(act=3, pk=None)):
        v = dict(ok, **bad)
        assert lib.skd_conv3x3_split_s2_nhwc(v["B"], v["H"], v["W"], v["cin"], v["cout"], v["x"], v["pk"], v["out"], None, v["mean"],
                                             v["var"], None, None, 0.0, v["act"], 0.01, v["pieces"], v["geo"], None) == 0, bad
    pixel, mask = ctypes.c_int64(-7), ctypes.c_uint(77)
    pp, pm = ctypes.addressof(pixel), ctypes.addressof(mask)
    for bad in ((0, 5, 0, pp, pm), (5, 0, 0, pp, pm), (-1, 5, 0, pp, pm), (5, 5, -1, pp, pm), (5, 5, 0, None, pm), (5, 5, 0, pp, None),
                (65536, 32768, 0, pp, pm)):
        assert lib.skd_conv3x3_split_s2_taps(*bad) == 0, bad
    assert (pixel.value, mask.value) == (-7, 77), "a refusal writes nothing"


# ---- 2. the row map ------------------------------------------------------------------------------------------------------------

def _row_map(B, H, W):
    """The numpy restatement: per output row m = (b * Ho + oy) * Wo + ox the centre pixel (b * H + 2 oy) * W + 2 ox and the mask
    with bit 3 ty + tx set iff 0 <= 2 oy + ty - 1 < H and 0 <= 2 ox + tx - 1 < W."""
    ho, wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    b, oy, ox = np.meshgrid(np.arange(B), np.arange(ho), np.arange(wo), indexing="ij")
    pixel = ((b * H + 2 * oy) * W + 2 * ox).reshape(-1).astype(np.int64)
    mask = np.zeros(B * ho * wo, dtype=np.int64)
    for ty in range(3):
        for tx in range(3):
            y, x = 2 * oy + ty - 1, 2 * ox + tx - 1
            mask |= ((y >= 0) & (y < H) & (x >= 0) & (x < W)).reshape(-1).astype(np.int64) << (3 * ty + tx)
    return pixel, mask


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 2, 2), (2, 5, 5), (2, 6, 6), (3, 13, 10), (2, 10, 13), (1, 129, 129)])
def test_taps_equal_the_numpy_restatement(shape):
    """Every m of the shape: the function the kernel calls, evaluated by the host-only entry.  Pixel and mask agree exactly."""
    B, H, W = shape
    taps = _lib.load().skd_conv3x3_split_s2_taps
    want_pixel, want_mask = _row_map(B, H, W)
    pixel, mask = ctypes.c_int64(), ctypes.c_uint()
    pp, pm = ctypes.addressof(pixel), ctypes.addressof(mask)
    got_pixel, got_mask = np.empty_like(want_pixel), np.empty_like(want_mask)
    for m in range(len(want_pixel)):
        assert taps(H, W, m, pp, pm) == 1
        got_pixel[m], got_mask[m] = pixel.value, mask.value
    assert np.array_equal(got_pixel, want_pixel) and np.array_equal(got_mask, want_mask)
    assert bool(((got_mask >> 4) & 1).all()), "the centre tap is always inside"
    if H == W == 1:
        assert got_mask.tolist() == [1 << 4]
    if (H, W) == (2, 2):
        assert got_mask.tolist() == [(1 << 4) | (1 << 5) | (1 << 7) | (1 << 8)]
    # a live tap's pixel is inside its image: what the kernel's loads rely on
    for tap in range(9):
        live = (got_mask >> tap) & 1 == 1
        p = got_pixel[live] + (tap // 3 - 1) * W + (tap % 3 - 1)
        img = got_pixel[live] // (H * W)
        assert bool(((p >= img * H * W) & (p < (img + 1) * H * W)).all())


def test_taps_beyond_two_to_the_31():
    """Rows whose input pixel index does not fit 32 bits (the entry does not bound the image index)."""
    H, W = 129, 129
    per = 65 * 65
    b = (1 << 31) // (H * W) + 5
    pixel, mask = ctypes.c_int64(), ctypes.c_uint()
    assert _lib.load().skd_conv3x3_split_s2_taps(H, W, b * per + 64 * 65 + 64, ctypes.addressof(pixel), ctypes.addressof(mask)) == 1
    assert pixel.value == (b * H + 128) * W + 128 > 1 << 31 and mask.value == 0b000011011


# ---- 3. the double -------------------------------------------------------------------------------------------------------------

class Stride2Double(NarrowDouble):
    """NarrowDouble + the entries of skd_stride2.h and skd_split2.h on raw HOST addresses, computed with torch: the stride-2 entry is
    F.conv2d(stride 2) + the eval-mode ABN formula, the two-piece entries compute what their three-piece twins compute (the wiring
    is what these tests look at).  Every 3x3 call is recorded with its stride and piece count."""

    def __init__(self, core, compute=True):
        super().__init__(core, compute)
        self.packs2, self.piece_of = 0, {}

    def _conv(self, name, *args):
        ok = super()._conv(name, *args)
        self.calls[-1].update(stride=1, pieces=2 if name == SPLIT2 else 3)
        return ok

    def skd_conv3x3_split_s2_supported(self, cin, cout, stride, padding, dilation, groups):
        return int(cin > 0 and cout > 0 and cin % 16 == 0 and cout % 128 == 0 and (stride, padding, dilation, groups) == (2, 1, 1, 1))

    def skd_conv3x3_split_s2_taps(self, *args):
        raise AssertionError("host only: the ops never call it")

    def skd_conv3x3_split_s2_nhwc(self, B, H, W, cin, cout, x, pack, out, cbias, mean, var, weight, bias, eps, act, slope, pieces,
                                  geometry, stream):
        assert pieces in (2, 3) and geometry == 0 and self.weights[pack].shape == (cout, cin, 3, 3)
        assert self.piece_of[pack] == pieces, "the pack of the other piece count"
        self.calls.append(dict(entry=S2, cin=cin, cout=cout, dilation=1, act=act, x=x, residual=None, bn=(mean, var, weight, bias),
                               stride=2, pieces=pieces))
        vec = lambda p: torch.from_numpy(_host(p, (cout,)).copy()) if p else None
        xt = torch.from_numpy(_host(x, (B, H, W, cin)).copy()).permute(0, 3, 1, 2)
        z = F.conv2d(xt, self.weights[pack], vec(cbias), 2, 1, 1).permute(0, 2, 3, 1)
        if mean:
            gamma = vec(weight).abs() + eps if weight else 1.0
            z = ((z - vec(mean)) * (1.0 / torch.sqrt(vec(var) + eps))) * gamma + (vec(bias) if bias else 0.0)
        if act == 3:
            z = torch.relu(z)
        else:
            assert act == 0
        _host(out, tuple(z.shape))[...] = z.numpy()
        return 1

    def skd_conv3x3_split_pack_weights(self, cin, cout, w, sn, sc, sy, sx, pack, nbytes, stream):
        self.piece_of[pack] = 3
        return super().skd_conv3x3_split_pack_weights(cin, cout, w, sn, sc, sy, sx, pack, nbytes, stream)

    def skd_conv3x3_split2_pack_bytes(self, cin, cout):
        return cout * cin * 36 if self.skd_conv3x3_split_supported(cin, cout, 1, 1, 1, 1) else 0

    def skd_conv3x3_split2_pack_weights(self, cin, cout, w, sn, sc, sy, sx, pack, nbytes, stream):
        assert nbytes == cout * cin * 36
        ok = super().skd_conv3x3_split_pack_weights(cin, cout, w, sn, sc, sy, sx, pack, nbytes, stream)      # remembers the weight
        self.packs, self.packs2, self.piece_of[pack] = self.packs - 1, self.packs2 + 1, 2
        return ok

    def skd_conv3x3_split2_nhwc(self, B, H, W, cin, cout, dil, x, pack, out, cbias, mean, var, weight, bias, eps, act, slope, geometry,
                                stream):
        assert self.piece_of[pack] == 2
        return self._conv(SPLIT2, B, H, W, cin, cout, dil, x, pack, out, None, cbias, mean, var, weight, bias, eps, act, slope)

    def skd_conv1x1_abn2_nhwc(self, *args):
        return self._core.skd_conv1x1_abn_nhwc(*args)

    def skd_conv1x1_abn2_pro_nhwc(self, *args):
        return self._core.skd_conv1x1_abn_pro_nhwc(*args)


@pytest.fixture
def double():
    d = Stride2Double(cref.load(_lib.SIGNATURES))
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


def _randomise(net, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, PC.InPlaceABNSync):
                m.running_var.uniform_(0.5, 1.5, generator=g)
                m.running_mean.normal_(0, 0.1, generator=g)
                m.weight.uniform_(0.5, 1.5, generator=g)
                m.bias.normal_(0, 0.1, generator=g)
    return net


_TEACHER = []


def _teacher():
    """The seeded full teacher, eval mode, channels-last, frozen (built once, copied per test)."""
    if not _TEACHER:
        torch.manual_seed(7)
        net = PC.Res_pspnet(PC.Bottleneck, [3, 4, 23, 3], 19)
        for p in net.parameters():
            p.requires_grad_(False)
        _TEACHER.append(_randomise(net, 8).eval().to(memory_format=torch.channels_last))
    return copy.deepcopy(_TEACHER[0])


# the nine calls of a flagged teacher, in order: (entry, Cin, Cout, stride, activation, with bn)
NINE = [(NARROW, 64, 64, 1, 3, True), (ENTRY, 64, 128, 1, 0, False), (NARROW, 64, 64, 1, 0, False), (NARROW, 64, 64, 1, 0, False),
        (NARROW, 64, 64, 1, 0, False), (S2, 128, 128, 2, 0, False), (ENTRY, 128, 128, 1, 0, False), (ENTRY, 128, 128, 1, 0, False),
        (ENTRY, 128, 128, 1, 0, False)]


def _seen(calls):
    return [(c["entry"], c["cin"], c["cout"], c["stride"], c["act"], c["bn"][0] is not None) for c in calls]


def _early(net, x):
    """x1, x2 of the teacher for the image ``x`` (stem, layer1, layer2: where the routing acts; the rest of the network is what
    it was)."""
    hold = {}
    h = net.layer3.register_forward_pre_hook(lambda mod, args: hold.setdefault("x2", args[0]))

    class Stop(Exception):
        pass

    def stop(mod, args):
        raise Stop()
    h2 = net.layer3[0].register_forward_pre_hook(stop)
    h1 = net.layer2.register_forward_pre_hook(lambda mod, args: hold.setdefault("x1", args[0]))
    try:
        net(x)
    except Stop:
        pass
    finally:
        for hh in (h, h1, h2):
            hh.remove()
    return hold["x1"], hold["x2"]


# ---- 4. routing of the teacher ---------------------------------------------------------------------------------------------------

def test_flagged_teacher_hands_exactly_the_nine_calls_over(double):
    net, x = _teacher(), _cl(1, 3, 45, 37, seed=4)
    with torch.no_grad():
        want = _early(net, x)
    assert double.calls == [] and double.packs == double.packs2 == 0 and double.narrow_pairs == []
    assert networks.route_teacher_early(net) is net
    flagged = [m for m in net.modules() if getattr(m, "_skd_teacher_early", False)]
    assert len(flagged) == 34 and all(isinstance(m, (PC.Bottleneck, PC.ResNet)) for m in flagged)
    # packed in the call: four narrow images, five wide ones
    early = [net.conv2, net.conv3] + [b.conv2 for b in net.layer1] + [b.conv2 for b in net.layer2]
    assert [p["w"] for p in double.narrow_pairs] == [c.weight.data_ptr() for c in (net.conv2, *(b.conv2 for b in net.layer1))]
    assert double.packs == 5 and double.packs2 == 0
    assert all(hasattr(c, "_skd_conv3x3_pack") != (c.out_channels == 64) for c in early)
    assert not any(hasattr(b.conv2, "_skd_conv3x3_pack") for layer in (net.layer3, net.layer4) for b in layer)
    with torch.no_grad():
        got = _early(net, x)
    assert _seen(double.calls) == NINE and all(c["pieces"] == 3 and c["dilation"] == 1 for c in double.calls)
    assert len(double.narrow_pairs) == 4 and double.packs == 5, "nothing is packed again in the forward"
    ptrs = lambda bn: tuple(t.data_ptr() for t in (bn.running_mean, bn.running_var, bn.weight, bn.bias))
    assert double.calls[0]["bn"] == ptrs(net.bn2)
    # the wiring against the plain op sequence: the bound of the existing wiring tests
    for g, w in zip(got, want):
        assert g.shape == w.shape and float((g - w).abs().max()) <= 1e-6 * max(1.0, float(w.abs().max()))
    assert want[1].shape[2:] == (6, 5) and want[0].shape[2:] == (12, 10), "layer2.0 halves the map"

    # nothing under grad, in training mode, on an NCHW input
    double.calls.clear()
    _early(net, x)
    net.train()
    with torch.no_grad():
        _early(net, _cl(2, 3, 45, 37, seed=5))
    net.eval()
    nchw = copy.deepcopy(net).to(memory_format=torch.contiguous_format)
    with torch.no_grad():
        _early(nchw, x.contiguous())
    assert double.calls == []

    # an excluded shape keeps the library
    try:
        PC.TEACHER_EARLY_ROUTING_EXCLUDED = frozenset({(128, 128, 2, 1), (64, 64, 1, 1)})
        with torch.no_grad():
            _early(net, x)
    finally:
        PC.TEACHER_EARLY_ROUTING_EXCLUDED = frozenset()
    assert _seen(double.calls) == [NINE[1]] + NINE[6:]
    double.calls.clear()
    try:
        PC.TEACHER_EARLY_ROUTING_EXCLUDED = frozenset({(128, 128, 1, 1), (64, 128, 1, 1)})
        with torch.no_grad():
            _early(net, x)
    finally:
        PC.TEACHER_EARLY_ROUTING_EXCLUDED = frozenset()
    assert _seen(double.calls) == [NINE[0]] + NINE[2:6]

    # enable=False: the flags and the packs are gone, nothing is handed over
    double.calls.clear()
    assert networks.route_teacher_early(net, enable=False) is net
    assert not any(hasattr(m, "_skd_teacher_early") for m in net.modules())
    assert not any(hasattr(c, a) for c in early for a in ("_skd_conv3x3_pack", "_skd_conv3x3_pack2", "_skd_conv3x3_narrow_pack"))
    with torch.no_grad():
        _early(net, x)
    assert double.calls == []


def test_excluded_set_is_empty_or_measured():
    assert isinstance(PC.TEACHER_EARLY_ROUTING_EXCLUDED, frozenset) and isinstance(PC.STRIDE2_ROUTING_EXCLUDED, frozenset)
    assert all(len(e) == 4 for e in PC.TEACHER_EARLY_ROUTING_EXCLUDED) and all(len(e) == 2 for e in PC.STRIDE2_ROUTING_EXCLUDED)


def test_two_piece_mark_moves_the_five_wide_calls(double):
    net, x = _teacher(), _cl(1, 3, 45, 37, seed=4)
    networks.set_teacher_pieces(net, 2)
    networks.route_teacher_early(net)
    assert double.packs2 == 5 and double.packs == 0 and len(double.narrow_pairs) == 4
    with torch.no_grad():
        _early(net, x)
    two = lambda e: SPLIT2 if e == ENTRY else e
    assert _seen(double.calls) == [(two(c[0]),) + c[1:] for c in NINE]
    assert [c["pieces"] for c in double.calls] == [3, 2, 3, 3, 3, 2, 2, 2, 2], "the 64-column calls keep three pieces"
    assert double.packs2 == 5 and double.packs == 0
    # a wide shape SPLIT2_ROUTING_EXCLUDED lists keeps three pieces
    double.calls.clear()
    try:
        PC.SPLIT2_ROUTING_EXCLUDED = frozenset({("3x3", 64, 128, 1)})
        with torch.no_grad():
            _early(net, x)
    finally:
        PC.SPLIT2_ROUTING_EXCLUDED = frozenset()
    assert [c["pieces"] for c in double.calls] == [3, 3, 3, 3, 3, 2, 2, 2, 2] and double.calls[1]["entry"] == ENTRY


def test_backend_without_the_entries_sets_the_flag_and_changes_nothing(c_double):
    net, x = _teacher(), _cl(1, 3, 33, 33, seed=4)
    with torch.no_grad():
        want = _early(net, x)
        networks.route_teacher_early(net)
        assert net._skd_teacher_early is True
        assert not any(hasattr(m, a) for m in net.modules() for a in ("_skd_conv3x3_pack", "_skd_conv3x3_narrow_pack"))
        got = _early(net, x)
    assert all(torch.equal(g, w) for g, w in zip(got, want))


def test_backend_without_the_stride2_entries_routes_none_of_the_nine():
    """The narrow and wide entries alone (the back-end of the 64-column tests): the routing is one unit and stays off."""
    d = NarrowDouble(cref.load(_lib.SIGNATURES), compute=True)
    _lib.install_test_backend(d)
    try:
        net = networks.route_teacher_early(_teacher())
        with torch.no_grad():
            _early(net, _cl(1, 3, 33, 33, seed=4))
        assert d.calls == [] and d.packs == 0 and d.narrow_pairs == []
    finally:
        _lib.install_test_backend(None)


def test_a_student_is_untouched_by_route_teacher_early(double):
    torch.manual_seed(5)
    student = PC.Res_pspnet(PC.BasicBlock, [2, 2, 2, 2], 19).eval().to(memory_format=torch.channels_last)
    assert networks.route_teacher_early(student) is student
    assert not any(hasattr(m, "_skd_teacher_early") for m in student.modules())
    with torch.no_grad():
        student(_cl(1, 3, 33, 33, seed=10))
    assert double.calls == [] and double.packs == 0 and double.narrow_pairs == []


# ---- 5. the student's inference form ---------------------------------------------------------------------------------------------

def _student():
    torch.manual_seed(5)
    net = PC.Res_pspnet(PC.BasicBlock, [2, 2, 2, 2], 19).to(memory_format=torch.channels_last)
    return _randomise(net, 6).eval()


def test_fuse_for_inference_stride2_routes_layer2_0_conv1_and_nothing_else_new(double):
    net, x = _student(), _cl(1, 3, 33, 49, seed=11)
    with torch.no_grad():
        want = net(x)
        networks.fuse_for_inference(net, narrow=True)
        base = net(x)
    before = [(c["entry"], c["cin"], c["cout"], c["dilation"], c["act"], c["residual"] is not None) for c in double.calls]
    assert len(before) == 17 and not [c for c in double.calls if c["stride"] != 1]
    assert not any(getattr(m, "_skd_infer_stride2", False) for m in net.modules())
    double.calls.clear()
    packs = double.packs
    assert networks.fuse_for_inference(net, narrow=True, stride2=True) is net
    assert all(m._skd_infer_stride2 is True for m in net.modules() if isinstance(m, PC.BasicBlock))
    assert double.packs == packs + 1 and hasattr(net.layer2[0].conv1, "_skd_conv3x3_pack"), "packed at flag time"
    with torch.no_grad():
        got = net(x)
    after = [(c["entry"], c["cin"], c["cout"], c["dilation"], c["act"], c["residual"] is not None) for c in double.calls]
    new = [c for c in double.calls if c["entry"] == S2]
    assert len(new) == 1 and after == before[:6] + [(S2, 64, 128, 1, 3, False)] + before[6:]
    bn1 = net.layer2[0].bn1
    assert new[0]["bn"] == tuple(t.data_ptr() for t in (bn1.running_mean, bn1.running_var, bn1.weight, bn1.bias))
    assert new[0]["stride"] == 2 and new[0]["pieces"] == 3 and double.packs == packs + 1
    for g, b, w in zip(got, base, want):
        if g is not None:
            assert float((g - w).abs().max()) <= 1e-6 * max(1.0, float(w.abs().max())), "the wiring against the plain op sequence"
            assert float((g - b).abs().max()) <= 1e-6 * max(1.0, float(w.abs().max()))
    # without ``narrow`` too; under grad or in training mode nothing is routed; an excluded shape keeps the library
    double.calls.clear()
    networks.fuse_for_inference(net, stride2=True)
    with torch.no_grad():
        net(x)
    assert [c["entry"] for c in double.calls].count(S2) == 1 and len(double.calls) == 12
    double.calls.clear()
    net(x)
    net.train()
    with torch.no_grad():
        net(_cl(2, 3, 33, 49, seed=12))
    net.eval()
    assert double.calls == []
    try:
        PC.STRIDE2_ROUTING_EXCLUDED = frozenset({(64, 128)})
        with torch.no_grad():
            net(x)
    finally:
        PC.STRIDE2_ROUTING_EXCLUDED = frozenset()
    assert len(double.calls) == 11 and not [c for c in double.calls if c["entry"] == S2]
    # the default leaves every existing call as it is, and enable=False drops the flag and the pack
    networks.fuse_for_inference(net)
    assert not any(getattr(m, "_skd_infer_stride2", False) for m in net.modules())
    networks.fuse_for_inference(net, enable=False, stride2=True)
    assert not any(getattr(m, "_skd_infer_stride2", False) for m in net.modules())
    assert not hasattr(net.layer2[0].conv1, "_skd_conv3x3_pack")


def test_op_refuses_what_it_does_not_take(double):
    conv = torch.nn.Conv2d(16, 128, 3, 2, 1, bias=False)
    x = _cl(1, 16, 5, 4)
    with torch.no_grad():
        assert SF.conv3x3_s2_supported(x, conv)
        assert not SF.conv3x3_s2_supported(x.contiguous(), conv), "NCHW"
        assert not SF.conv3x3_s2_supported(x.double(), torch.nn.Conv2d(16, 128, 3, 2, 1, bias=False).double())
        assert not SF.conv3x3_s2_supported(x, torch.nn.Conv2d(16, 128, 3, 1, 1)) and not SF.conv3x3_s2_supported(x, torch.nn.Conv2d(16, 64, 3, 2, 1))
        assert not SF.conv3x3_s2_supported(x, torch.nn.Conv2d(16, 128, 3, 2, 2, 2)), "dilation 2"
        pack = SF.conv3x3_pack_weights(conv)
        out = SF.conv3x3_s2_eval(x, pack, 128)
        assert out.shape == (1, 128, 3, 2) and out.is_contiguous(memory_format=torch.channels_last) and out._base is None
        assert float((out - conv(x)).abs().max()) <= 1e-6
        for bad in (1, 4, None, "3", 2.0, True):
            with pytest.raises(ValueError):
                SF.conv3x3_s2_eval(x, pack, 128, pieces=bad)
        with pytest.raises(ValueError):
            SF.conv3x3_s2_eval(x, pack, 128, activation="leaky_relu")
        with pytest.raises(ValueError, match="pack"):
            SF.conv3x3_s2_eval(x, pack, 128, pieces=2)
        with pytest.raises(ValueError, match="pack"):
            SF.conv3x3_s2_eval(x, pack, 256)
    assert not SF.conv3x3_s2_supported(x, conv), "under grad"
    with pytest.raises(RuntimeError):
        SF.conv3x3_s2_eval(x.requires_grad_(), pack, 128)


def test_op_is_never_downgraded(c_double):
    x = _cl(1, 16, 5, 4)
    with torch.no_grad():
        assert not SF.conv3x3_s2_supported(x, torch.nn.Conv2d(16, 128, 3, 2, 1, bias=False))
        with pytest.raises(NotImplementedError, match="skd_conv3x3_split_s2_nhwc"):
            SF.conv3x3_s2_eval(x, torch.zeros(16 * 128 * 54, dtype=torch.uint8), 128)


# ---- 6. the public switches ------------------------------------------------------------------------------------------------------

def test_default_args_and_the_environment(monkeypatch):
    for name in ("SKD_TEACHER_EARLY", "SKD_SPLIT_STRIDE2"):
        monkeypatch.delenv(name, raising=False)
    assert default_args().teacher_early is False and default_args().split_stride2 is False
    assert default_args(teacher_early=True).teacher_early is True and default_args(split_stride2=True).split_stride2 is True
    monkeypatch.setenv("SKD_TEACHER_EARLY", "1")
    assert default_args().teacher_early is True and default_args().split_stride2 is False
    assert default_args(teacher_early=False).teacher_early is False
    assert default_args().split_train is False and default_args().teacher_pieces == 3      # independent of the others
    monkeypatch.setenv("SKD_TEACHER_EARLY", "0")
    monkeypatch.setenv("SKD_SPLIT_STRIDE2", "1")
    assert default_args().teacher_early is False and default_args().split_stride2 is True


def test_netmodel_flags_its_teacher_and_nothing_else(double, monkeypatch):
    for name in ("SKD_TEACHER_EARLY", "SKD_SPLIT_STRIDE2", "SKD_TEACHER_PIECES", "SKD_SPLIT_TRAIN", "SKD_SPLIT_NARROW"):
        monkeypatch.delenv(name, raising=False)
    kw = dict(device=torch.device("cpu"), batch_size=2, ho=False)
    flags = lambda net: [type(m).__name__ for m in net.modules() if getattr(m, "_skd_teacher_early", False)]
    s2 = lambda net: [m for m in net.modules() if getattr(m, "_skd_infer_stride2", False)]
    model = NetModel(default_args(**kw))
    assert model.teacher_early is False and flags(model.teacher) == [] and flags(model.student) == [] and not model.split_stride2
    model = NetModel(default_args(teacher_early=True, **kw))
    assert model.teacher_early is True and len(flags(model.teacher)) == 34 and flags(model.student) == []
    assert not model.split_train and model.teacher_pieces == 3 and s2(model.student) == []
    monkeypatch.setenv("SKD_TEACHER_EARLY", "1")
    model = NetModel(default_args(teacher_pieces=2, **kw))
    assert len(flags(model.teacher)) == 34 and flags(model.student) == [] and model.teacher_pieces == 2
    monkeypatch.delenv("SKD_TEACHER_EARLY")
    # the student's switch: effective together with fused_eval only
    model = NetModel(default_args(split_stride2=True, **kw))
    assert model.split_stride2 is True and s2(model.student) == [] and flags(model.teacher) == []
    model = NetModel(default_args(fused_eval=True, split_stride2=True, **kw))
    assert len(s2(model.student)) == 8 and s2(model.teacher) == []
    monkeypatch.setenv("SKD_SPLIT_STRIDE2", "1")
    model = NetModel(default_args(fused_eval=True, split_narrow=True, **kw))
    assert len(s2(model.student)) == 8 and model.student._skd_infer_narrow is True
    model = NetModel(default_args(fused_eval=True, split_stride2=False, **kw))
    assert s2(model.student) == []


def test_packs_follow_a_fused_optimizer_step(double):
    """The stride-2 form runs on the stride-1 form's cache: one rule (_version_key), rebuilt once behind a fused step."""
    torch.manual_seed(9)
    conv = torch.nn.Conv2d(16, 128, 3, 2, 1, bias=False)
    x = _cl(1, 16, 7, 6, seed=3)
    with torch.no_grad():
        p3, p2 = SF.conv3x3_pack_weights(conv), SF.conv3x3_pack_weights(conv, pieces=2)
        assert SF.conv3x3_pack_weights(conv) is p3 and (double.packs, double.packs2) == (1, 1)
        first = SF.conv3x3_s2_eval(x, p3, 128)
        assert torch.equal(SF.conv3x3_s2_eval(x, p2, 128, pieces=2), first)
    try:
        opt = torch.optim.SGD(conv.parameters(), 0.5, fused=True)
    except (RuntimeError, TypeError, ValueError):      # a torch without fused SGD on the host: the plain form
        opt = torch.optim.SGD(conv.parameters(), 0.5)
    opt.register_step_post_hook(advance_versions_after_step)
    conv.weight.grad = torch.ones_like(conv.weight)
    version = conv.weight._version
    opt.step()
    assert conv.weight._version > version
    with torch.no_grad():
        q3, q2 = SF.conv3x3_pack_weights(conv), SF.conv3x3_pack_weights(conv, pieces=2)
        assert SF.conv3x3_pack_weights(conv) is q3 and SF.conv3x3_pack_weights(conv, pieces=2) is q2
        assert (double.packs, double.packs2) == (2, 2), "each re-packed once behind the step"
        second = SF.conv3x3_s2_eval(x, q3, 128)
        assert float((second - F.conv2d(x, conv.weight, None, 2, 1)).abs().max()) <= 1e-5 and not torch.equal(second, first)


def test_docs_name_both_switches():
    root = build.INCLUDE.rsplit("include", 1)[0]
    for name in ("DESIGN.md", "README.md"):
        with open(root + name) as fh:
            text = fh.read()
        assert "SKD_TEACHER_EARLY" in text and "SKD_SPLIT_STRIDE2" in text, name
        assert "route_teacher_early" in text and "skd_stride2.h" in text, name
    with open(root + "DESIGN.md") as fh:
        assert "7.12" in fh.read()
    assert "TEACHER_EARLY_ROUTING_EXCLUDED" in PC.route_teacher_early.__doc__ and "stride2" in PC.fuse_for_inference.__doc__
    assert "skd_stride2.h" in SF.conv3x3_s2_eval.__doc__ and "skd_stride2.h" in SF.conv3x3_s2_supported.__doc__
    assert "SKD_SPLIT_STRIDE2" in evaluate.__doc__
