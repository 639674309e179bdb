"""-m gpu: piece planes (include/skd_planes.h) -- the stand-alone split and join kernels, the producer (the split reduce GEMM
whose epilogue writes the three bf16 pieces of its result: csrc/conv1x1.hip with PLANES), the consumer (the wide stride-1 3x3
convolution that loads the pieces instead of splitting an fp32 map: csrc/conv3x3.hip with PLANES), and the frozen teacher flagged by
``route_teacher_planes``.

NO tolerance anywhere: the split is a pure function of the fp32 value, so
    planes          == split2_ref.pieces(v, 3), bf16 bit patterns, read through skd_planes_offset (the layout is never hard-coded);
    join(split(v))  == v, bit for bit (-0.0 included);
    producer planes == pieces(skd_conv1x1_abn_nhwc(...));
    consumer output == skd_conv3x3_split_nhwc on the fp32 map, for every geometry and epilogue;
    flagged block / teacher == unflagged, ``torch.equal``.
Every buffer of a kernel test sits between 0xFF guard bands (tests/bounds_cases.Arena), the planes at exactly skd_planes_bytes, and
every case is launched twice with equal bits.
"""
import contextlib
import ctypes
import os
import sys
import zlib

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import bounds_cases as BC  # noqa: E402
import split2_ref as R  # noqa: E402
import split_exact as X  # noqa: E402
from structure_knowledge_distillation_amd import _lib, functional as SF, networks  # noqa: E402
from structure_knowledge_distillation_amd.networks import pspnet_combine as PC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
P = BC.P
ACT = {"none": 0, "leaky_relu": 1, "relu": 3}
SPLIT, JOIN = "skd_planes_split_nhwc", "skd_planes_join_nhwc"
PRODUCER, CONSUMER = "skd_conv1x1_abn_planes_nhwc", "skd_conv3x3_split_planes_nhwc"


@pytest.fixture(scope="module")
def hip():
    return _lib.load()


def nbytes_of(hip, m, c):
    n = ctypes.c_int64(-1)
    assert hip.skd_planes_bytes(m, c, ctypes.cast(ctypes.byref(n), ctypes.c_void_p)) == 1
    return int(n.value)


_OFFSETS = {}


def offsets(hip, m, c):
    """(m, c, 3) int64: skd_planes_offset of every (row, channel, piece), queried once per (m, c) and shared."""
    if (m, c) not in _OFFSETS:
        v = ctypes.c_int64(0)
        ref = ctypes.cast(ctypes.byref(v), ctypes.c_void_p)
        flat = []
        for row in range(m):
            for ch in range(c):
                for piece in range(3):
                    assert hip.skd_planes_offset(m, c, row, ch, piece, ref) == 1
                    flat.append(v.value)
        _OFFSETS[(m, c)] = torch.tensor(flat, dtype=torch.int64).view(m, c, 3)
    return _OFFSETS[(m, c)]


def bf16_bits(t):
    """The bf16 bit patterns (int32 in 0 .. 65535) of a tensor of exact bf16 values (any float dtype)."""
    return (t.float().contiguous().view(torch.int32) >> 16) & 0xFFFF


def want_bits(v):
    """(M, C, 3) bf16 bit patterns of split2_ref.pieces(v, 3) for v (M, C) fp32 on the CPU."""
    return torch.stack([bf16_bits(p) for p in R.pieces(v, 3)], dim=-1)


def decode(hip, planes, m, c):
    """(M, C, 3) bf16 bit patterns read from the planes (a uint8 tensor) through the offset map."""
    words = planes.cpu().view(torch.int16).to(torch.int32) & 0xFFFF
    off = offsets(hip, m, c)
    assert int(off.min()) >= 0 and int(off.max()) + 2 <= planes.numel() and not bool((off % 2).any())
    return words[off // 2]


def encode(hip, v):
    """The planes of v (M, C) fp32 built on the HOST through the offset map: a uint8 tensor of exactly skd_planes_bytes."""
    m, c = v.shape
    words = torch.zeros(nbytes_of(hip, m, c) // 2, dtype=torch.int32)
    words[(offsets(hip, m, c) // 2).reshape(-1)] = want_bits(v).reshape(-1)
    return words.to(torch.int16).view(torch.uint8)          # the low 16 bits of each word


def twice(launch, outs, arena):
    """Run ``launch`` twice on the same buffers: guards intact both times, equal bits; returns the first results (CPU)."""
    assert launch() == 1
    arena.check()
    first = [o.cpu().clone() for o in outs]
    for o in outs:
        o.view(torch.uint8).fill_(BC.FILL)
    assert launch() == 1
    arena.check()
    for o, f in zip(outs, first):
        assert torch.equal(o.cpu().view(torch.uint8), f.view(torch.uint8)), "a second launch on the same buffers gave other bits"
    return first


# ---- 1. split and join ------------------------------------------------------------------------------------------------------------

SPLIT_MS, SPLIT_CS = [1, 63, 64, 65, 257], [16, 48, 256]


def split_data(m, c):
    """(m, c) fp32: normal data at scales 1e-30, 1 and 1e30, +-0, subnormals, exact bf16 values and the integer classes N / T / W."""
    g = torch.Generator().manual_seed(zlib.crc32(b"planes-split-%d-%d" % (m, c)))
    n = m * c
    special = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 1.1754942e-38, 5.9e-39, 1.0, -1.0, 1.5, 3.140625, -0.0078125,
                            2.0 ** -126, 2.0 ** 100, -(2.0 ** -100), 65280.0, 1e-38])
    parts = [special, torch.randn(n, generator=g) * 1e-30, torch.randn(n, generator=g), torch.randn(n, generator=g) * 1e30,
             torch.randn(n, generator=g).bfloat16().float(), X.narrow(g, (n,)), X.two_values(g, n), X.wide_values(g, n),
             (torch.rand(n, generator=g) * 2e-38 - 1e-38)]
    pool = torch.cat(parts)
    v = pool[torch.randint(0, pool.numel(), (n,), generator=g)]
    v[:min(n, special.numel())] = special[:n]          # every special value at least once (the first sixteen at M = 1, C = 16)
    return v.view(m, c).contiguous()


@pytest.mark.parametrize("c", SPLIT_CS)
@pytest.mark.parametrize("m", SPLIT_MS)
def test_split_and_join(hip, m, c):
    v = split_data(m, c)
    assert bool(torch.isfinite(v).all())
    A = BC.Arena(DEV)
    dx = A.inp("x", v, row=c)
    planes = A.out("planes", nbytes_of(hip, m, c), torch.uint8)
    back = A.out("back", (m, c), row=c)
    (got,) = twice(lambda: hip.skd_planes_split_nhwc(m, c, P(dx), P(planes), None), [planes], A)
    bits, want = decode(hip, got, m, c), want_bits(v)
    bad = bits != want
    print("split M%d C%d: %d of %d pieces differ" % (m, c, int(bad.sum()), bad.numel()))
    assert not bool(bad.any()), "first differing (row, channel, piece): %s  value %r  got %#x want %#x" % (
        bad.nonzero()[0].tolist(), float(v[tuple(bad.nonzero()[0][:2].tolist())]), int(bits[bad][0]), int(want[bad][0]))
    (joined,) = twice(lambda: hip.skd_planes_join_nhwc(m, c, P(planes), P(back), None), [back], A)
    # join(split(v)) == v bit for bit for every value three bf16 pieces can carry.  A bf16 piece has no bit below 2^-133, so a value
    # below 2^-109 with low bits set (fp32 reaches down to 2^-149) is not the sum of its pieces on any machine: those come back as
    # the sum of the reference pieces, and there is none of them at or above 2^-109.
    p0, p1, p2 = (p.float() for p in R.pieces(v, 3))
    model = (p0 + p1) + p2
    model = torch.where(model == 0, p0, model)
    carried = (p0.double() + p1.double() + p2.double()) == v.double()
    assert bool(carried[v.abs() >= 2.0 ** -109].all()) and bool(carried[v == 0].all())
    assert torch.equal(joined.view(torch.int32), model.view(torch.int32))
    back_ok = joined.view(torch.int32)[carried] == v.view(torch.int32)[carried]
    assert bool(back_ok.all()), "%d of %d values do not come back bit for bit" % (int((~back_ok).sum()), back_ok.numel())
    # the planes built on the host through the offset map are the kernel's, byte for byte: the layout has no padding
    assert torch.equal(encode(hip, v), got)


# ---- 2. the producer ----------------------------------------------------------------------------------------------------------------

PRO_MS = [1, 63, 65, 129, 2113, "half-height"]      # tests/test_split_core_pipeline_gpu.py's classes for the 1x1 entry
PRO_KS, PRO_NS = [16, 48, 80], [128, 256]
EPILOGUES_1X1 = [("none", False), ("none", True), ("relu", False), ("relu", True)]      # (activation, weight and bias vectors)
MAP_DECODE_MAX_M = 129      # above it the planes are compared with skd_planes_split_nhwc of the reference (checked above)


def producer_m(hip, m, k, n):
    if m != "half-height":
        return m
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    m = 3 * cus * 128 // (n // 128) + 65
    out = (ctypes.c_int64 * 7)()
    assert hip.skd_conv1x1_abn_geometry(m, k, n, cus, ctypes.cast(out, ctypes.c_void_p)) == 1
    assert int(out[3]) > 0 and int(out[4]) >= int(out[3]) + 2, (m, list(out))      # full-height panels and at least two of 64 rows
    return m


@pytest.mark.parametrize("n", PRO_NS)
@pytest.mark.parametrize("k", PRO_KS)
@pytest.mark.parametrize("m", PRO_MS, ids=[str(m) for m in PRO_MS])
def test_producer_planes_are_the_pieces_of_the_fp32_entry(hip, m, k, n):
    m = producer_m(hip, m, k, n)
    g = torch.Generator().manual_seed(zlib.crc32(b"planes-producer-%d-%d-%d" % (m, k, n)))
    x = torch.relu(torch.randn(m, k, generator=g) + torch.randn(1, k, generator=g) * 0.5)
    w = torch.randn(n, k, generator=g) * 0.05
    mean, var = torch.randn(n, generator=g) * 0.3, torch.rand(n, generator=g) + 0.5
    gamma, beta = torch.randn(n, generator=g), torch.randn(n, generator=g)
    A = BC.Arena(DEV)
    dx, dw = A.inp("x", x, row=k), A.inp("w", w, row=k)
    vec = {name: A.inp(name, t) for name, t in (("mean", mean), ("var", var), ("gamma", gamma), ("beta", beta))}
    ref = A.out("ref", (m, n), row=n)
    planes = A.out("planes", nbytes_of(hip, m, n), torch.uint8)
    ref_planes = A.out("ref_planes", nbytes_of(hip, m, n), torch.uint8)
    for act, affine in EPILOGUES_1X1:
        ga, be = (P(vec["gamma"]), P(vec["beta"])) if affine else (None, None)
        tail = (P(vec["mean"]), P(vec["var"]), ga, be, 1e-5, ACT[act], 0.01, None)
        ref.fill_(float("nan"))
        assert hip.skd_conv1x1_abn_nhwc(m, k, n, P(dx), P(dw), None, P(ref), *tail) == 1
        (got,) = twice(lambda: hip.skd_conv1x1_abn_planes_nhwc(m, k, n, P(dx), P(dw), P(planes), *tail), [planes], A)
        fp32 = ref.cpu()
        assert bool(torch.isfinite(fp32).all()) and float(fp32.abs().max()) > 0.1
        if m <= MAP_DECODE_MAX_M:
            bad = decode(hip, got, m, n) != want_bits(fp32)
            assert not bool(bad.any()), "%s affine=%s: %d of %d pieces differ, first at %s" % (
                act, affine, int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist())
        ref_planes.fill_(BC.FILL)
        assert hip.skd_planes_split_nhwc(m, n, P(ref), P(ref_planes), None) == 1
        A.check()
        same = got == ref_planes.cpu()
        assert bool(same.all()), "%s affine=%s: %d of %d plane bytes differ from the split of the fp32 entry's output" % (
            act, affine, int((~same).sum()), same.numel())


# ---- 3. the consumer ----------------------------------------------------------------------------------------------------------------

CON_SHAPES = [(1, 3, 3), (2, 5, 7), (1, 9, 9), (1, 17, 13)]
CON_CASES = [(s, d, cin, cout) for s in CON_SHAPES for d in (1, 2, 4) for cin in (16, 48) for cout in (128, 256)]
CON_IDS = ["%dx%dx%d-d%d-%d-%d" % (s + (d, cin, cout)) for s, d, cin, cout in CON_CASES]


def pack_of(hip, A, wt):
    cout, cin = wt.shape[:2]
    nbytes = hip.skd_conv3x3_split_pack_bytes(cin, cout)
    dw = A.inp("weight", wt)
    pk = A.out("pack", nbytes, torch.uint8)
    assert hip.skd_conv3x3_split_pack_weights(cin, cout, P(dw), *dw.stride(), P(pk), nbytes, None) == 1
    A.check()
    return pk


def conv_args(b, h, w, cin, cout, src, pk, out, vec, eps, act, d, geometry, planes):
    epi = (P(vec["cbias"]), P(vec["mean"]), P(vec["var"]), P(vec["gamma"]), P(vec["beta"]), eps, ACT[act], 0.01)
    if planes:
        return (b, h, w, cin, cout, P(src), P(pk), P(out)) + epi + (d, geometry, None)
    return (b, h, w, cin, cout, d, P(src), P(pk), P(out)) + epi + (geometry, None)


@pytest.mark.parametrize("shape,d,cin,cout", CON_CASES, ids=CON_IDS)
def test_consumer_gives_the_bits_of_the_fp32_entry(hip, shape, d, cin, cout):
    b, h, w = shape
    m = b * h * w
    g = torch.Generator().manual_seed(zlib.crc32(("planes-consumer-" + CON_IDS[CON_CASES.index((shape, d, cin, cout))]).encode()))
    x = torch.relu(torch.randn(m, cin, generator=g) + torch.randn(1, cin, generator=g) * 0.5)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    params = dict(cbias=torch.randn(cout, generator=g) * 0.2, mean=torch.randn(cout, generator=g) * 0.3,
                  var=torch.rand(cout, generator=g) + 0.5, gamma=torch.randn(cout, generator=g), beta=torch.randn(cout, generator=g))
    A = BC.Arena(DEV)
    dx = A.inp("x", x, row=cin)
    pk = pack_of(hip, A, wt)
    vec = {k: A.inp(k, v) for k, v in params.items()}
    none = dict.fromkeys(params)
    nb = nbytes_of(hip, m, cin)
    by_kernel = A.out("planes", nb, torch.uint8)
    assert hip.skd_planes_split_nhwc(m, cin, P(dx), P(by_kernel), None) == 1
    by_host = A.inp("planes_host", encode(hip, x))
    A.check()
    assert by_host.numel() == nb and torch.equal(by_host.cpu(), by_kernel.cpu())
    want, out = A.out("want", (m, cout), row=cout), A.out("out", (m, cout), row=cout)
    for v, eps, act in ((none, 0.0, "none"), (vec, 1e-5, "relu"), (vec, 1e-5, "leaky_relu")):      # (leaky: the <128, 1, *, PLANES> forms)
        for geometry in range(4):
            want.fill_(float("nan"))
            assert hip.skd_conv3x3_split_nhwc(*conv_args(b, h, w, cin, cout, dx, pk, want, v, eps, act, d, geometry, False)) == 1
            ref = want.cpu()
            assert bool(torch.isfinite(ref).all())
            for src in (by_kernel, by_host):
                (got,) = twice(lambda: hip.skd_conv3x3_split_planes_nhwc(
                    *conv_args(b, h, w, cin, cout, src, pk, out, v, eps, act, d, geometry, True)), [out], A)
                assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), "%s, geometry %d: %d of %d outputs differ" % (
                    act, geometry, int((got.view(torch.int32) != ref.view(torch.int32)).sum()), got.numel())


# ---- 4. all six products ----------------------------------------------------------------------------------------------------------

EXACT_1X1 = [c for c in X.CASES if c.group == "conv1x1"]
EXACT_3X3 = [c for c in X.CASES if c.group == "conv3x3"]


@pytest.mark.parametrize("case", EXACT_1X1, ids=[c.name for c in EXACT_1X1])
def test_producer_all_six_products(hip, case):
    """W x N, N x W and T x T (tests/split_exact.py) through the producer with the identity epilogue: the planes hold the float64
    product (an integer below 2^24: three pieces carry it exactly), read back through the join."""
    built = X.build(case)
    m, k = built.a.shape
    n = built.b.shape[0]
    A = BC.Arena(DEV)
    dx, dw = A.inp("x", built.a, row=k), A.inp("w", built.b, row=k)
    mean, var = A.inp("mean", torch.zeros(n)), A.inp("var", torch.ones(n))
    planes, back = A.out("planes", nbytes_of(hip, m, n), torch.uint8), A.out("back", (m, n), row=n)
    twice(lambda: hip.skd_conv1x1_abn_planes_nhwc(m, k, n, P(dx), P(dw), P(planes), P(mean), P(var), None, None, 0.0, 0, 0.01, None),
          [planes], A)
    assert hip.skd_planes_join_nhwc(m, n, P(planes), P(back), None) == 1
    A.check()
    got = back.cpu().double()
    assert torch.equal(got, built.exact()), X.explain(got, built)


@pytest.mark.parametrize("case", EXACT_3X3, ids=[c.name for c in EXACT_3X3])
def test_consumer_all_six_products(hip, case):
    """The same three runs through the consumer on the planes of the integer map: the output IS the float64 convolution."""
    built = X.build(case)
    b, cin, h, w = built.a.shape
    cout, d = built.b.shape[0], case.args["d"]
    m = b * h * w
    A = BC.Arena(DEV)
    dx = A.inp("x", built.a.permute(0, 2, 3, 1).reshape(m, cin).contiguous(), row=cin)
    pk = pack_of(hip, A, built.b)
    planes, out = A.out("planes", nbytes_of(hip, m, cin), torch.uint8), A.out("out", (m, cout), row=cout)
    assert hip.skd_planes_split_nhwc(m, cin, P(dx), P(planes), None) == 1
    none = dict.fromkeys(("cbias", "mean", "var", "gamma", "beta"))
    for geometry in (1, 2, 3):
        (got,) = twice(lambda: hip.skd_conv3x3_split_planes_nhwc(
            *conv_args(b, h, w, cin, cout, planes, pk, out, none, 0.0, "none", d, geometry, True)), [out], A)
        got = got.view(b, h, w, cout).permute(0, 3, 1, 2).double()
        assert torch.equal(got, built.exact()), "geometry %d: %s" % (geometry, X.explain(got, built))


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(hip):
    b, h, w, cin, cout, k = 2, 5, 7, 32, 128, 48
    m = b * h * w
    g = torch.Generator().manual_seed(11)
    A = BC.Arena(DEV)
    dx = A.inp("x", torch.randn(m, cin, generator=g), row=cin)
    dx1, dw1 = A.inp("x1", torch.randn(m, k, generator=g), row=k), A.inp("w1", torch.randn(cout, k, generator=g), row=k)
    pk = pack_of(hip, A, torch.randn(cout, cin, 3, 3, generator=g))
    var = A.inp("var", torch.ones(cout))
    planes_in, planes_out = A.out("planes_in", nbytes_of(hip, m, cin), torch.uint8), A.out("planes_out", nbytes_of(hip, m, cout), torch.uint8)
    out, back = A.out("out", (m, cout), row=cout), A.out("back", (m, cin), row=cin)
    assert hip.skd_planes_split_nhwc(m, cin, P(dx), P(planes_in), None) == 1
    torch.cuda.synchronize()
    outs = (planes_out, out, back)
    before = [t.view(torch.uint8).clone() for t in outs]

    def consumer(**kw):
        a = dict(b=b, h=h, w=w, cin=cin, cout=cout, src=P(planes_in), pk=P(pk), out=P(out), mean=None, var=None, act=0, d=1, geo=0)
        a.update(kw)
        return hip.skd_conv3x3_split_planes_nhwc(a["b"], a["h"], a["w"], a["cin"], a["cout"], a["src"], a["pk"], a["out"], None,
                                                 a["mean"], a["var"], None, None, 0.0, a["act"], 0.01, a["d"], a["geo"], None)

    def producer(**kw):
        a = dict(m=m, k=k, n=cout, x=P(dx1), w=P(dw1), out=P(planes_out), mean=P(var), var=P(var), act=0)
        a.update(kw)
        return hip.skd_conv1x1_abn_planes_nhwc(a["m"], a["k"], a["n"], a["x"], a["w"], a["out"], a["mean"], a["var"], None, None, 0.0,
                                               a["act"], 0.01, None)

    def stream(entry, **kw):
        a = dict(m=m, c=cin, x=P(dx) if entry == SPLIT else P(back), planes=P(planes_in))
        a.update(kw)
        args = (a["m"], a["c"]) + ((a["x"], a["planes"]) if entry == SPLIT else (a["planes"], a["x"])) + (None,)
        return getattr(hip, entry)(*args)
    for bad in (dict(cin=24), dict(cin=0), dict(cout=64), dict(b=0), dict(h=0), dict(w=0), dict(d=0), dict(src=None), dict(pk=None),
                dict(out=None), dict(src=planes_in.data_ptr() + 8), dict(pk=pk.data_ptr() + 8), dict(h=65536, w=32768), dict(geo=4),
                dict(geo=-1), dict(act=2), dict(act=7), dict(mean=P(var)), dict(var=P(var))):
        assert consumer(**bad) == 0, ("consumer", bad)
    for bad in (dict(k=24), dict(n=64), dict(n=0), dict(m=0), dict(m=-1), dict(x=None), dict(w=None), dict(out=None), dict(mean=None),
                dict(var=None), dict(x=dx1.data_ptr() + 4), dict(w=dw1.data_ptr() + 8), dict(out=planes_out.data_ptr() + 8),
                dict(act=2), dict(act=7)):
        assert producer(**bad) == 0, ("producer", bad)
    for entry in (SPLIT, JOIN):
        for bad in (dict(c=24), dict(c=0), dict(m=0), dict(m=-3), dict(x=None), dict(planes=None), dict(x=dx.data_ptr() + 4),
                    dict(planes=planes_in.data_ptr() + 8)):
            assert stream(entry, **bad) == 0, (entry, bad)
    A.check()
    for t, was in zip(outs, before):
        assert torch.equal(t.view(torch.uint8), was), "a refused call wrote an output"
    assert consumer() == 1 and producer() == 1 and stream(JOIN) == 1
    A.check()
    assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(back).any())


# ---- 6. the ops, a block, the teacher --------------------------------------------------------------------------------------------

def counted(fn):
    """``fn()`` under the per-entry timers: (result, {entry: launches}) for the planes entries and their fp32 twins."""
    names = [PRODUCER, CONSUMER, SPLIT, "skd_conv1x1_abn_nhwc", "skd_conv3x3_split_nhwc"]
    _lib.enable_kernel_timing(names)
    try:
        with torch.no_grad():
            out = fn()
    finally:
        calls = _lib.disable_kernel_timing()
    return out, {k: len(v) for k, v in calls.items()}


def seeded(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, PC.InPlaceABNSync):
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) * 0.5 + 0.1)
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.05)
    for q in module.parameters():
        q.requires_grad_(False)
    return module.eval().to(DEV).to(memory_format=torch.channels_last)


def test_block_flagged_equals_unflagged(monkeypatch):
    monkeypatch.setattr(PC, "PLANES_ROUTING_EXCLUDED", frozenset())      # the mechanism; the set is the policy
    torch.manual_seed(21)
    block = seeded(PC.Bottleneck(1024, 256, dilation=2), 22)
    x = torch.randn(1, 1024, 9, 9, generator=torch.Generator().manual_seed(23)).to(DEV).contiguous(memory_format=torch.channels_last)
    assert SF.planes_supported()
    want, off = counted(lambda: block(x))
    assert off[PRODUCER] == off[CONSUMER] == 0 and off["skd_conv1x1_abn_nhwc"] == 1 and off["skd_conv3x3_split_nhwc"] == 1
    try:
        assert networks.route_teacher_planes(block) is block
        got, on = counted(lambda: block(x))
        networks.set_teacher_pieces(block, 2)
        two, marked = counted(lambda: block(x))
    finally:
        networks.set_teacher_pieces(block, 3)
        networks.route_teacher_planes(block, enable=False)
    assert on[PRODUCER] == on[CONSUMER] == 1 and on["skd_conv1x1_abn_nhwc"] == on["skd_conv3x3_split_nhwc"] == 0, on
    assert marked[PRODUCER] == marked[CONSUMER] == 0, "a block marked for two pieces keeps its present path"
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0.1
    assert torch.equal(got, want), "%d of %d outputs differ" % (int((got != want).sum()), got.numel())
    assert not torch.equal(two, want), "two pieces changed nothing"
    # the op level: planes out of the reduce GEMM == planes of its fp32 output; Planes in place of x == the fp32 call
    with torch.no_grad():
        bn = block.bn1
        args = (x, block.conv1.weight, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.eps, "relu")
        fp32, planes = SF.conv1x1_abn_eval(*args), SF.conv1x1_abn_planes_eval(*args)
        assert isinstance(planes, SF.Planes) and planes.shape == (1, 9, 9, 256) and planes.M == 81 and planes.C == 256
        assert torch.equal(planes.data, SF.planes_split(fp32).data) and torch.equal(SF.planes_join(planes), fp32)
        pack = SF.conv3x3_pack_weights(block.conv2)
        assert torch.equal(SF.conv3x3_split_eval(planes, pack, 256, 2), SF.conv3x3_split_eval(fp32, pack, 256, 2))


_TEACHER = {}


@contextlib.contextmanager
def deterministic_library():
    """The libraries' deterministic modes for the duration of a whole-network comparison: with their defaults two UNFLAGGED
    forwards of the teacher differ in most values (accumulation with atomics in the library's kernels), and ``torch.equal`` between a
    flagged and an unflagged forward says something only when an unflagged forward repeats itself -- which the test checks first.
    The convolutions stay on the convolution library (disabling it would leave NCHW maps, and nothing would be routed); the kernels
    under test are the same either way."""
    was = (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark, torch.are_deterministic_algorithms_enabled(),
           torch.is_deterministic_algorithms_warn_only_enabled())
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = was[0], was[1]
        torch.use_deterministic_algorithms(was[2], warn_only=was[3])


def teacher():
    """The seeded teacher, its input and its unflagged outputs -- made once, under deterministic_library, never modified."""
    if not _TEACHER:
        torch.manual_seed(31)
        net = seeded(PC.Res_pspnet(PC.Bottleneck, [3, 4, 23, 3], 19), 32)
        x = torch.randn(1, 3, 65, 65, generator=torch.Generator().manual_seed(33)).to(DEV).contiguous(memory_format=torch.channels_last)
        with deterministic_library():
            want, calls = counted(lambda: net(x))
        assert len(want) == 7 and calls[PRODUCER] == calls[CONSUMER] == 0
        _TEACHER.update(net=net, x=x, want=[t.clone() for t in want])
    return _TEACHER["net"], _TEACHER["x"], _TEACHER["want"]


def same_outputs(got, want, what="flagged against unflagged"):
    assert len(got) == len(want) == 7
    diff = [int((a != b).sum()) for a, b in zip(got, want)]
    print("%s: differing values per output %s" % (what, diff))
    assert all(bool(torch.isfinite(b).all()) for b in want)
    assert not any(diff), "%s: %s of %s values differ" % (what, diff, [b.numel() for b in want])


@pytest.mark.parametrize("early", [False, True], ids=["planes", "planes+early"])
def test_teacher_flagged_equals_unflagged(monkeypatch, early):
    monkeypatch.setattr(PC, "PLANES_ROUTING_EXCLUDED", frozenset())
    net, x, first = teacher()
    try:
        with deterministic_library():
            if early:
                networks.route_teacher_early(net)
            want, calls = counted(lambda: net(x))
            assert calls[PRODUCER] == calls[CONSUMER] == 0
            if not early:
                same_outputs(want, first, "unflagged, run to run")
            networks.route_teacher_planes(net)
            got, calls = counted(lambda: net(x))
    finally:
        networks.route_teacher_planes(net, enable=False)
        networks.route_teacher_early(net, enable=False)
    assert calls[PRODUCER] == calls[CONSUMER] == 26 and calls[SPLIT] == 0, calls      # layer3's 23 blocks and layer4's 3
    same_outputs(got, want)
    assert not any(hasattr(m, "_skd_teacher_planes") for m in net.modules())


def test_teacher_flagged_through_a_graph_capture(monkeypatch):
    """One hipGraph capture and replay of the flagged teacher forward by the recipe of NetModel._capture_teacher (warm-up on a
    side stream, thread-local capture): the replay's outputs are the eager unflagged ones, bit for bit -- the planes are torch
    allocations of the capture's pool like every other temporary."""
    monkeypatch.setattr(PC, "PLANES_ROUTING_EXCLUDED", frozenset())
    net, x, want = teacher()
    try:
        stack = contextlib.ExitStack()
        stack.enter_context(deterministic_library())
        networks.route_teacher_planes(net)
        static_in = x.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(2):
                net(static_in)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(graph, capture_error_mode="thread_local"):
            outs = net(static_in)
        for t in outs:
            t.fill_(float("nan"))
        static_in.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        same_outputs(outs, want, "flagged replay against unflagged eager")
    finally:
        stack.close()
        networks.route_teacher_planes(net, enable=False)
