"""-m gpu: the K loop of the split-operand core (csrc/conv_split_dev.hpp k_loop: global loads two K-tiles ahead of the MFMAs, split
and LDS store one ahead) at the sizes where its prologue, its unrolled-by-two steady state and its drain meet.

The other split-core files start at K = 64 (four K-tiles) and never put a tap boundary of the 3x3 kernel at an odd trip behind
masked taps.  Here:

1x1 (skd_conv1x1_abn_nhwc, and skd_conv1x1_abn_pro_nhwc with a residual): K = 16, 32, 48, 80 -- one, two, three and five K-tiles:
no steady-state trip at all up to three, one pair plus an odd drain at five -- N = 128, M = 1, 63, 65, 129, 2113 (both tile heights
of a launch never occur below one round, so one more case derives M from the device's CU count and takes the half-height branch,
as tests/test_conv1x1_split_gpu.py does).
3x3 (skd_conv3x3_split_nhwc, geometry 1, 2 and 3 passed explicitly: both kernels, both tile heights): Cin = 16 (nine K-tiles, a new
tap every trip) and 48 (27 K-tiles, three per tap, odd total), Cout = 128, on 3 x 3 at dilation 4 (only the centre tap is live
anywhere), 7 x 5 at dilation 2 and 13 x 11 at dilation 1.

Truth as in those files: the plain-C oracle (dot product in double, oracle/abn_ref.c) for the 1x1 entries, ``F.conv2d`` in float64
for the 3x3 entry.  Float data: max |hip - want| / max |want| within those files' caps (2e-6 and 2e-5).  Small-integer data
(|x| <= 7, |w| <= 3): every partial sum is an exact fp32 integer in any order, so the output must equal the integer product bit
for bit -- a dropped, doubled or swapped K-tile cannot pass that.  Every launch: the 160 sentinel rows behind M stay intact, no
device status word is raised, and a second call on the same buffers gives the same bits.
"""
import ctypes
import zlib

import pytest
import torch
import torch.nn.functional as F

from oracle import cref
from structure_knowledge_distillation_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAP_1X1 = 2e-6      # tests/test_conv1x1_split_gpu.py
CAP_3X3 = 2e-5      # tests/test_conv3x3_split_gpu.py
SENTINEL = 7.0
SLACK_ROWS = 160
ACT_NONE, ACT_RELU = 0, 3
N = 128
KS = [16, 32, 48, 80]
MS = [1, 63, 65, 129, 2113]
ENTRIES = ["plain", "pro-res"]


@pytest.fixture(scope="module")
def hip():
    return _lib.load()


@pytest.fixture(scope="module")
def ref():
    return cref.load(_lib.SIGNATURES)


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def status_clean(hip):
    return _lib.device_status() == [0] * hip.skd_status_words()


def identity_bn(n):
    """mean 0, var 1, eps 0, no affine: the ABN formula returns its argument."""
    return torch.zeros(n), torch.ones(n), None, None, 0.0


def call_1x1(lib, m, k, x, w, r, out, bn, pack_src, act, dev):
    """One call of the entry that ``pack_src`` selects on ``lib`` (the HIP library or the oracle), tensors on ``dev``."""
    mean, var, ga, be, eps = bn
    to = lambda t: None if t is None else t.to(dev)
    keep = [to(t) for t in (x, w, r, mean, var, ga, be)]
    args = (P(keep[0]), P(keep[1]), P(keep[2]), P(out), P(keep[3]), P(keep[4]), P(keep[5]), P(keep[6]), eps)
    if pack_src is None:
        assert lib.skd_conv1x1_abn_nhwc(m, k, N, *args, act, 0.01, None)
    else:
        pm, pv, pw, pb, peps = pack_src
        pk = torch.empty(4, k, device=dev)
        src = [to(t) for t in (pm, pv, pw, pb)]
        assert lib.skd_abn_pack_eval_params(k, P(src[0]), P(src[1]), P(src[2]), P(src[3]), peps, P(pk), None)
        assert lib.skd_conv1x1_abn_pro_nhwc(m, k, N, *args, P(pk), act, 0.01, None)
        keep += src + [pk]
    if dev == DEV:
        torch.cuda.synchronize()
    return keep


def run_1x1(hip, m, k, x, w, r, bn, pack_src, act):
    """The kernel's (M, N) output; checks the sentinel rows, the status words and that a second call repeats the bits."""
    out = torch.full((m + SLACK_ROWS, N), SENTINEL, device=DEV)
    call_1x1(hip, m, k, x, w, r, out, bn, pack_src, act, DEV)
    first = out.cpu()
    assert bool((first[m:] == SENTINEL).all()), "rows beyond M were written"
    call_1x1(hip, m, k, x, w, r, out, bn, pack_src, act, DEV)
    assert torch.equal(out.cpu(), first), "a second call on the same buffers gave other bits"
    assert status_clean(hip)
    return first[:m]


def float_inputs_1x1(name, m, k, pro):
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    w = torch.randn(N, k, generator=g) * 0.05
    pack_src, r = None, None
    if pro:      # x is a raw convolution output, the prologue's BatchNorm + ReLU bring it to order 1; with a residual
        x = torch.randn(m, k, generator=g) * 2 + torch.randn(1, k, generator=g)
        pack_src = (torch.randn(k, generator=g) * 0.5, torch.rand(k, generator=g) * 4 + 2, torch.randn(k, generator=g),
                    torch.randn(k, generator=g) * 0.5, 1e-5)
        r = torch.relu(torch.randn(m, N, generator=g))
    else:
        x = torch.relu(torch.randn(m, k, generator=g) + torch.randn(1, k, generator=g) * 0.5)
    bn = (torch.randn(N, generator=g) * 0.3, torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g),
          torch.randn(N, generator=g), 1e-5)
    return x, w, r, bn, pack_src


def int_inputs_1x1(name, m, k, pro):
    """|x| <= 7, |w| <= 3, identity epilogue; the prologue form gets the identity BatchNorm (a = relu(x)) and an integer residual."""
    assert k * 7 * 3 + 7 < 2 ** 24
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    x = torch.randint(-7, 8, (m, k), generator=g).float()
    w = torch.randint(-3, 4, (N, k), generator=g).float()
    if not pro:
        return x, w, None, None, x.double() @ w.double().t()
    r = torch.randint(-7, 8, (m, N), generator=g).float()
    pack_src = (torch.zeros(k), torch.ones(k), None, None, 0.0)
    return x, w, r, pack_src, torch.relu(x).double() @ w.double().t() + r.double()


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("k", KS)
def test_1x1_short_k_float(hip, ref, k, m, entry):
    pro = entry == "pro-res"
    x, w, r, bn, pack_src = float_inputs_1x1("float-K%d-M%d-%s" % (k, m, entry), m, k, pro)
    want = torch.empty(m, N)
    call_1x1(ref, m, k, x, w, r, want, bn, pack_src, ACT_RELU, "cpu")
    got = run_1x1(hip, m, k, x, w, r, bn, pack_src, ACT_RELU).double()
    assert bool(torch.isfinite(got).all())
    err = float((got - want.double()).abs().max()) / max(float(want.abs().max()), 1e-30)
    print("K%d M%d %s: err %.3e  cap %.1e" % (k, m, entry, err, CAP_1X1))
    assert err <= CAP_1X1


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("k", KS)
def test_1x1_short_k_integers_bit_exact(hip, k, m, entry):
    x, w, r, pack_src, want = int_inputs_1x1("int-K%d-M%d-%s" % (k, m, entry), m, k, entry == "pro-res")
    got = run_1x1(hip, m, k, x, w, r, identity_bn(N), pack_src, ACT_NONE)
    assert torch.equal(got.double(), want), "%d of %d outputs differ" % (int((got.double() != want).sum()), got.numel())


@pytest.mark.parametrize("k", [48, 80])
def test_1x1_short_k_half_height_panels(hip, k):
    """M = one round of full-height tiles on three workgroups per compute unit + a whole 64-row panel + one with a single live row."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    m = 3 * cus * 128 + 65
    out = (ctypes.c_int64 * 7)()
    assert hip.skd_conv1x1_abn_geometry(m, k, N, cus, ctypes.cast(out, ctypes.c_void_p)) == 1
    p_full, panels = int(out[3]), int(out[4])
    assert p_full > 0 and panels >= p_full + 2 and (m - p_full * 128) % 64 == 1, (m, p_full, panels)
    x, w, r, pack_src, want = int_inputs_1x1("int-hh-K%d" % k, m, k, False)
    got = run_1x1(hip, m, k, x, w, r, identity_bn(N), pack_src, ACT_NONE)
    assert torch.equal(got.double(), want), "%d of %d outputs differ" % (int((got.double() != want).sum()), got.numel())


# ---- 3x3 ---------------------------------------------------------------------------------------------------------------------------

COUT = 128
CINS = [16, 48]                                                  # nk = 9, 27
SHAPES = [(1, 3, 3, 4), (2, 7, 5, 2), (1, 13, 11, 1)]            # (B, H, W, dilation)
SHAPE_IDS = ["1x3x3-d4", "2x7x5-d2", "1x13x11-d1"]


def run_3x3(hip, x, wt, d, geometry):
    """(B, Cout, H, W) output of the identity-epilogue entry; the same three checks as run_1x1."""
    b, cin, h, w = x.shape
    m = b * h * w
    dx = x.to(DEV).contiguous(memory_format=torch.channels_last)
    dw = wt.to(DEV)
    nbytes = hip.skd_conv3x3_split_pack_bytes(cin, COUT)
    assert nbytes == COUT * cin * 9 * 6
    pk = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    assert hip.skd_conv3x3_split_pack_weights(cin, COUT, P(dw), *dw.stride(), P(pk), nbytes, None)
    out = torch.full((m + SLACK_ROWS, COUT), SENTINEL, device=DEV)

    def call():
        assert hip.skd_conv3x3_split_nhwc(b, h, w, cin, COUT, d, P(dx), P(pk), P(out), None, None, None, None, None, 0.0, ACT_NONE,
                                          0.01, geometry, None)
        torch.cuda.synchronize()
        return out.cpu()

    first = call()
    assert bool((first[m:] == SENTINEL).all()), "rows beyond M were written"
    assert torch.equal(call(), first), "a second call on the same buffers gave other bits"
    assert status_clean(hip)
    return first[:m].view(b, h, w, COUT).permute(0, 3, 1, 2)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("cin", CINS)
def test_3x3_tap_boundaries_integers_bit_exact(hip, cin, shape):
    b, h, w, d = shape
    assert 9 * cin * 7 * 3 < 2 ** 24
    g = torch.Generator().manual_seed(zlib.crc32(("int3-%d-%s" % (cin, shape)).encode()))
    x = torch.randint(-7, 8, (b, cin, h, w), generator=g).float()
    wt = torch.randint(-3, 4, (COUT, cin, 3, 3), generator=g).float()
    want = F.conv2d(x.double(), wt.double(), None, 1, d, d)
    for geometry in (1, 2, 3):
        got = run_3x3(hip, x, wt, d, geometry).double()
        assert torch.equal(got, want), "geometry %d: %d of %d outputs differ" % (geometry, int((got != want).sum()), got.numel())


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("cin", CINS)
def test_3x3_tap_boundaries_float(hip, cin, shape):
    b, h, w, d = shape
    g = torch.Generator().manual_seed(zlib.crc32(("float3-%d-%s" % (cin, shape)).encode()))
    x = torch.relu(torch.randn(b, cin, h, w, generator=g) + torch.randn(1, cin, 1, 1, generator=g) * 0.5)
    wt = torch.randn(COUT, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    want = F.conv2d(x.double(), wt.double(), None, 1, d, d)
    outs = [run_3x3(hip, x, wt, d, geometry) for geometry in (1, 2, 3)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), "the three geometries gave different bits"
    got = outs[0].double()
    assert bool(torch.isfinite(got).all())
    err = float((got - want).abs().max()) / max(float(want.abs().max()), 1e-30)
    print("Cin%d %s: err %.3e  cap %.1e" % (cin, shape, err, CAP_3X3))
    assert err <= CAP_3X3
