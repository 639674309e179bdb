"""-m gpu: the student's wide 3x3 training convolutions on two bf16 pieces (include/skd_train2.h): the two-plane pack pair, the
forward and the data gradient on skd_conv3x3_split2_nhwc, the two-piece weight gradient, the autograd op conv3x3_split_train2 and
one training step with ``student_pieces=2``.  On the HIP back-end a missing entry is a failure of these tests, never a skip.

Every entry-level call hands its inputs, outputs and workspace out of the guard-band arena of tests/bounds_cases.py (0xFF on
both sides, checked after each call); the weight gradient's workspace has exactly plan[2] bytes, starts as 0xFF and is called
twice, left as the first call left it: the same bits, no guard byte changed.

Shapes (tests/train2_cases.py): (Cin, Cout) = (128, 256) and (256, 128), B = 2, 9 x 11 (P = 198: no multiple of 16, pixel quads
straddle row and image ends), dilation 1 and 2, the weight gradient with 1 and 3 slices.  The integer cases are proven in
tests/test_train2_cpu.py.  Float data: every output element against float64,
    |y2 - y64| <= 2^-15 sum |a| |b| + e3
with sum |a| |b| the same product of the absolute values in float64 and e3 the three-piece entry's own largest elementwise error
on the same inputs, measured in the same test; 2^-15 = two dropped residuals of 2^-17 each and a1 b1 below 2^-16 (the header).
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import bounds_cases as BC
import split_exact as SE
import train2_cases as T2
from bounds_cases import P
from structure_knowledge_distillation_amd import _lib, functional as SF

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS2 = 2.0 ** -15
PACK_PAIR2, PLAN2, WGRAD2 = "skd_conv3x3_split2_pack_pair", "skd_conv3x3_split2_wgrad_plan", "skd_conv3x3_split2_wgrad_nhwc"
RUN2, PACK2, BYTES2 = "skd_conv3x3_split2_nhwc", "skd_conv3x3_split2_pack_weights", "skd_conv3x3_split2_pack_bytes"


@pytest.fixture(scope="module")
def hip():
    lib = _lib.load()
    for name in (PACK_PAIR2, PLAN2, WGRAD2, RUN2, PACK2, BYTES2):
        getattr(lib, name)          # a missing entry fails here
    return lib


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ---- the entries, each call between guards ------------------------------------------------------------------------------------

def pack_pair(hip, A, w, pieces=2, fwd=True, bwd=True):
    """(pack_fwd, pack_bwd) of the weight view ``w`` on the device (any strides), as guarded byte buffers; None where not asked."""
    cout, cin = int(w.shape[0]), int(w.shape[1])
    size = hip.skd_conv3x3_split2_pack_bytes if pieces == 2 else hip.skd_conv3x3_split_pack_bytes
    entry = hip.skd_conv3x3_split2_pack_pair if pieces == 2 else hip.skd_conv3x3_split_pack_pair
    nf, nb = int(size(cin, cout)), int(size(cout, cin))
    assert nf == nb == (4 if pieces == 2 else 6) * 9 * cin * cout
    pf = A.out("pack_fwd", (nf,), torch.uint8, row=4096) if fwd else None
    pb = A.out("pack_bwd", (nb,), torch.uint8, row=4096) if bwd else None
    assert entry(cin, cout, P(w), *w.stride(), P(pf), nf if fwd else 0, P(pb), nb if bwd else 0, None) == 1
    A.check()
    return pf, pb


def conv(hip, A, x, pack, cout, d, bias=None, pieces=2):
    """conv3x3(x) + bias, raw, of the channels-last CPU map ``x`` on the image ``pack``: (B, Cout, H, W) on the CPU."""
    b, cin, h, w = x.shape
    xa = A.inp("x", nhwc(x))
    ba = A.inp("bias", bias)
    out = A.out("y", (b, h, w, cout))
    entry = hip.skd_conv3x3_split2_nhwc if pieces == 2 else hip.skd_conv3x3_split_nhwc
    assert entry(b, h, w, cin, cout, d, P(xa), P(pack), P(out), P(ba), None, None, None, None, 0.0, 0, 0.01, 0, None) == 1
    A.check()
    return out.cpu().permute(0, 3, 1, 2)


def wgrad(hip, x, g, d, slices, pieces=2):
    """dw (Cout, Cin, 3, 3) on the CPU, channels-last strides, from two calls on the same guarded buffers."""
    b, cin, h, w = x.shape
    cout = g.shape[1]
    plan = (ctypes.c_int64 * 3)()
    planner = hip.skd_conv3x3_split2_wgrad_plan if pieces == 2 else hip.skd_conv3x3_split_wgrad_plan
    entry = hip.skd_conv3x3_split2_wgrad_nhwc if pieces == 2 else hip.skd_conv3x3_split_wgrad_nhwc
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert planner(b, h, w, cin, cout, slices, cus, ctypes.cast(plan, ctypes.c_void_p)) == 1
    used, nbytes = int(plan[0]), int(plan[2])
    assert nbytes == used * 9 * cin * cout * 4 and (slices == 0 or used == slices)
    A = BC.Arena(DEV)
    xa, ga = A.inp("x", nhwc(x)), A.inp("g", nhwc(g))
    dw = A.out("dw", (cout, 3, 3, cin)).permute(0, 3, 1, 2)
    ws = A.ws("workspace", nbytes // 4)
    assert bool((ws.view(torch.uint8) == BC.FILL).all()), "the workspace starts dirty"
    results = []
    for k in range(2):
        if k:
            A.reset()
        assert entry(b, h, w, cin, cout, d, P(xa), P(ga), P(dw), *dw.stride(), P(ws), nbytes, used, None) == 1
        A.check()
        results.append(dw.detach().cpu().clone())
    assert BC.same_bits(results[0], results[1]), "two calls on the same buffers differ"
    assert bool(torch.isfinite(ws).all()), "every element of the workspace was written"
    return results[0]


def product(hip, case_product, a, b, cin, cout, d, pieces=2, slices=1):
    """One of the three products of a training convolution through the C ABI.  fwd: (x, w); dgrad: (g, w); wgrad: (x, g)."""
    if case_product == "wgrad":
        return wgrad(hip, a, b, d, slices, pieces)
    A = BC.Arena(DEV)
    w = A.inp("w", b.contiguous())
    pf, pb = pack_pair(hip, A, w, pieces)
    if case_product == "fwd":
        return conv(hip, A, a, pf, cout, d, None, pieces)
    return conv(hip, A, a, pb, cin, d, None, pieces)


# ---- 1. the pack pair ---------------------------------------------------------------------------------------------------------

LAYOUTS = ("contiguous", "channels_last", "slice")


def _weight(A, cin, cout, layout, seed):
    """(the (Cout, Cin, 3, 3) view on the device, its values on the CPU): contiguous, channels-last, or the slice [:, 64:] of a
    channels-last weight 64 channels wider (the PSP bottleneck's)."""
    gen = torch.Generator().manual_seed(seed)
    wide = cin + (64 if layout == "slice" else 0)
    w = torch.randn(cout, wide, 3, 3, generator=gen) * torch.exp2(torch.randint(-12, 4, (cout, wide, 1, 1), generator=gen).float())
    if layout == "contiguous":
        view = A.inp("w", w)
    else:
        view = A.inp("w", nhwc(w)).permute(0, 3, 1, 2)
    if layout == "slice":
        view, w = view[:, 64:], w[:, 64:]
    assert tuple(view.shape) == (cout, cin, 3, 3)
    return view, w.contiguous()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("chans", T2.CHANNELS, ids=lambda c: "%dto%d" % c)
def test_pack_pair_equals_pack_weights_byte_for_byte(hip, chans, layout):
    cin, cout = chans
    A = BC.Arena(DEV)
    view, w = _weight(A, cin, cout, layout, 100 + cin // 128)
    n = int(hip.skd_conv3x3_split2_pack_bytes(cin, cout))
    assert n == 36 * cin * cout == int(hip.skd_conv3x3_split2_pack_bytes(cout, cin))
    # the references: the single-image entry on w and on the MATERIALISED Wd[c][n][ty][tx] = w[n][c][2 - ty][2 - tx]
    wd = A.inp("wd", w.flip(2, 3).transpose(0, 1).contiguous())
    wc = A.inp("wc", w)
    want_f, want_b = A.out("want_fwd", (n,), torch.uint8, row=4096), A.out("want_bwd", (n,), torch.uint8, row=4096)
    assert hip.skd_conv3x3_split2_pack_weights(cin, cout, P(wc), *wc.stride(), P(want_f), n, None) == 1
    assert hip.skd_conv3x3_split2_pack_weights(cout, cin, P(wd), *wd.stride(), P(want_b), n, None) == 1
    A.check()
    pf, pb = pack_pair(hip, A, view)
    assert torch.equal(pf, want_f), "forward image: %d bytes differ" % int((pf != want_f).sum())
    assert torch.equal(pb, want_b), "backward image: %d bytes differ" % int((pb != want_b).sum())
    assert not torch.equal(want_f, want_b)
    # one pack NULL, in either position: the other image alone, the same bytes
    only_f, none = pack_pair(hip, A, view, bwd=False)
    assert none is None and torch.equal(only_f, want_f)
    none, only_b = pack_pair(hip, A, view, fwd=False)
    assert none is None and torch.equal(only_b, want_b)
    # a second call on the same buffers: the same bytes
    assert hip.skd_conv3x3_split2_pack_pair(cin, cout, P(view), *view.stride(), P(pf), n, P(pb), n, None) == 1
    A.check()
    assert torch.equal(pf, want_f) and torch.equal(pb, want_b)
    # and the two planes are planes 0 and 1 of the three-piece image, per (column tile, K-tile)
    f3, _ = pack_pair(hip, A, view, pieces=3, bwd=False)
    tiles = n // (2 * 4096)
    assert torch.equal(f3.view(tiles, 3, 4096)[:, :2].reshape(-1), want_f)


def test_pack_pair_refusals_launch_nothing(hip):
    cin, cout = 128, 256
    A = BC.Arena(DEV)
    view, _ = _weight(A, cin, cout, "channels_last", 7)
    n = 36 * cin * cout
    pf, pb = A.out("pack_fwd", (n + 16,), torch.uint8, row=4096), A.out("pack_bwd", (n + 16,), torch.uint8, row=4096)
    s = view.stride()
    f = hip.skd_conv3x3_split2_pack_pair
    off = lambda t, k: ctypes.c_void_p(t.data_ptr() + k)
    refused = [
        f(cin, cout, None, *s, P(pf), n, P(pb), n, None),
        f(cin, cout, P(view), *s, None, 0, None, 0, None),
        f(cin, cout, P(view), *s, off(pf, 8), n, P(pb), n, None),
        f(cin, cout, P(view), *s, P(pf), n, off(pb, 4), n, None),
        f(cin, cout, P(view), *s, P(pf), n - 1, P(pb), n, None),
        f(cin, cout, P(view), *s, P(pf), n, P(pb), n - 16, None),
        f(cin, cout, P(view), -s[0], s[1], s[2], s[3], P(pf), n, P(pb), n, None),
        f(cin, cout, P(view), s[0], s[1], s[2], -1, P(pf), n, P(pb), n, None),
        f(64, cout, P(view), *s, P(pf), n, P(pb), n, None),
        f(cin, 192, P(view), *s, P(pf), n, P(pb), n, None),
        f(cin, 32, P(view), *s, P(pf), n, None, 0, None),
        f(24, cout, P(view), *s, P(pf), n, None, 0, None),
    ]
    assert refused == [0] * len(refused), refused
    A.check()
    assert bool((pf == BC.FILL).all()) and bool((pb == BC.FILL).all()), "a refused call wrote a pack"


# ---- 2. / 3. integers: exact for narrow x wide, the three-product model for two x two --------------------------------------------

@pytest.mark.parametrize("case", T2.CASES, ids=lambda c: c.name)
def test_integer_products(hip, case):
    built = T2.build(case)
    want, exact = T2.want_of(case)
    for slices in (T2.WGRAD_SLICES if case.product == "wgrad" else (1,)):
        got = product(hip, case.product, built.a, built.b, case.cin, case.cout, case.d, 2, slices).double()
        assert got.shape == want.shape
        wrong = int((got != want).sum())
        what = "the exact product" if case.kind != "TT" else "the three-product model"
        assert wrong == 0, "%s, %d slice(s): %d of %d outputs differ from %s (largest difference %g)" % (
            case.name, slices, wrong, want.numel(), what, float((got - want).abs().max()))
        if case.kind == "TT":
            assert int((got != exact).sum()) >= exact.numel() // 8, "two pieces x two pieces must NOT be the exact product"
            # the three-piece twin keeps a1 b1: exact on the same inputs
            got3 = product(hip, case.product, built.a, built.b, case.cin, case.cout, case.d, 3, slices).double()
            assert torch.equal(got3, exact)


# ---- 4. float data --------------------------------------------------------------------------------------------------------------

_FLOAT = {}


def float_case(cin, cout, d):
    """Post-ReLU-like x, Gaussian w and g (He-scaled weight), and the three float64 products with their sums of absolute
    products; made once and shared (never modified)."""
    key = (cin, cout, d)
    if key not in _FLOAT:
        gen = torch.Generator().manual_seed(3300 + cin // 128 + 10 * d)
        x = cl(torch.relu(torch.randn(T2.B, cin, T2.H, T2.W, generator=gen) + torch.randn(1, cin, 1, 1, generator=gen) * 0.5))
        w = torch.randn(cout, cin, 3, 3, generator=gen) * (2.0 / (9 * cin)) ** 0.5
        g = cl(torch.randn(T2.B, cout, T2.H, T2.W, generator=gen))
        ops = {"fwd": (SE.conv_op(1, d, d), x, w), "dgrad": (SE.dgrad_op(1, d, d, (T2.H, T2.W)), g, w),
               "wgrad": (SE.wgrad_op(1, d, d, 3), x, g)}
        ref = {k: (op(a.double(), b.double()), op(a.double().abs(), b.double().abs())) for k, (op, a, b) in ops.items()}
        _FLOAT[key] = (x, w, g, ops, ref)
    return _FLOAT[key]


def library(name, x, w, g, d):
    """The library's fp32 result of the same product (aten), for the accuracy note."""
    xd, wd, gd = cl(x).to(DEV), cl(w).to(DEV), cl(g).to(DEV)
    if name == "fwd":
        return F.conv2d(xd, wd, None, 1, d, d).cpu()
    mask = (True, False, False) if name == "dgrad" else (False, True, False)
    out = torch.ops.aten.convolution_backward(gd, xd, wd, None, [1, 1], [d, d], [d, d], False, [0, 0], 1, mask)
    return out[0 if name == "dgrad" else 1].cpu()


@pytest.mark.parametrize("d", T2.DILATIONS, ids=lambda d: "d%d" % d)
@pytest.mark.parametrize("chans", T2.CHANNELS, ids=lambda c: "%dto%d" % c)
def test_float_products_within_the_two_piece_bound(hip, chans, d):
    cin, cout = chans
    x, w, g, ops, ref = float_case(cin, cout, d)
    failures = []
    for name in T2.PRODUCTS:
        _, a, b = ops[name]
        y64, sabs = ref[name]
        for slices in (T2.WGRAD_SLICES if name == "wgrad" else (1,)):
            y3 = product(hip, name, a, b, cin, cout, d, 3, slices).double()
            y2 = product(hip, name, a, b, cin, cout, d, 2, slices).double()
            yl = library(name, x, w, g, d).double()
            e3 = float((y3 - y64).abs().max())
            err2 = (y2 - y64).abs()
            ratio = float((err2 / (EPS2 * sabs).clamp_min(1e-300)).max())
            over = int((err2 > EPS2 * sabs + e3).sum())
            scale = float(y64.abs().max())
            print("FLOAT %s %dto%d d%d slices %d: two pieces max|err| %.3e (%.3e of max|y|), largest |err| / (2^-15 sum|a||b|) %.4f; "
                  "three pieces e3 %.3e (%.3e); library %.3e (%.3e)"
                  % (name, cin, cout, d, slices, float(err2.max()), float(err2.max()) / scale, ratio, e3, e3 / scale,
                     float((yl - y64).abs().max()), float((yl - y64).abs().max()) / scale))
            assert bool(torch.isfinite(y2).all())
            if over:
                failures.append("%s slices %d: %d of %d elements above 2^-15 sum|a||b| + e3 (largest ratio %.4f, e3 %.3e)"
                                % (name, slices, over, y2.numel(), ratio, e3))
            assert not torch.equal(y2, y3), "two pieces and three give the same bits on float data: the wrong entry ran"
    assert not failures, "; ".join(failures)


# ---- 5. guard bands: every new pointer-taking entry, explicitly ---------------------------------------------------------------------

def test_new_entries_between_guards(hip):
    """The pack pair and the weight gradient with dirty outputs and a dirty workspace of exactly the planned size, each called
    twice: no guard byte changes, both calls give the same bits (``wgrad`` and ``pack_pair`` check after every call)."""
    cin, cout, d = 256, 128, 2
    x, w, g, _, _ = float_case(cin, cout, d)
    for slices in (1, 3, 0):
        wgrad(hip, x, g, d, slices)
    A = BC.Arena(DEV)
    wv = A.inp("w", nhwc(w)).permute(0, 3, 1, 2)
    pf, pb = pack_pair(hip, A, wv)
    first = (pf.cpu().clone(), pb.cpu().clone())
    A.reset()
    assert bool((pf == BC.FILL).all())
    n = pf.numel()
    assert hip.skd_conv3x3_split2_pack_pair(cin, cout, P(wv), *wv.stride(), P(pf), n, P(pb), n, None) == 1
    A.check()
    assert torch.equal(pf.cpu(), first[0]) and torch.equal(pb.cpu(), first[1])
    # the plan writes its three words and nothing else
    buf = (ctypes.c_int64 * 5)(-1, -1, -1, -1, -1)
    at = ctypes.cast(ctypes.addressof(buf) + 8, ctypes.c_void_p)
    assert hip.skd_conv3x3_split2_wgrad_plan(T2.B, T2.H, T2.W, cin, cout, 3, 0, at) == 1
    assert buf[0] == -1 and buf[4] == -1 and list(buf[1:4]) == [3, 5, 3 * 9 * cin * cout * 4]


# ---- 6. autograd ------------------------------------------------------------------------------------------------------------------

class TwoConvs(torch.nn.Module):
    """128 -> 256 -> 128, dilation 2, both with a bias, both on conv3x3_split_train / conv3x3_split_train2 by the module's piece
    count, with the module's ``wgrad``."""

    def __init__(self, w1, b1, w2, b2):
        super().__init__()
        self.c1, self.c2 = torch.nn.Conv2d(128, 256, 3, 1, 2, 2), torch.nn.Conv2d(256, 128, 3, 1, 2, 2)
        with torch.no_grad():
            for conv, wt, bs in ((self.c1, w1, b1), (self.c2, w2, b2)):
                conv.weight.copy_(wt)
                conv.bias.copy_(bs)
        self.to(DEV).to(memory_format=torch.channels_last)
        self.pieces, self.wgrad = 3, False

    def forward(self, x):
        op = SF.conv3x3_split_train2 if self.pieces == 2 else SF.conv3x3_split_train
        h = op(x, self.c1.weight, 2, self.c1.bias, self.c1, wgrad=self.wgrad)
        return op(h, self.c2.weight, 2, self.c2.bias, self.c2, wgrad=self.wgrad)


def _two_convs_case():
    gen = torch.Generator().manual_seed(3306)
    x = cl(torch.relu(torch.randn(T2.B, 128, T2.H, T2.W, generator=gen) + torch.randn(1, 128, 1, 1, generator=gen) * 0.5))
    w1 = torch.randn(256, 128, 3, 3, generator=gen) * (2.0 / (9 * 128)) ** 0.5
    w2 = torch.randn(128, 256, 3, 3, generator=gen) * (2.0 / (9 * 256)) ** 0.5
    b1, b2 = torch.randn(256, generator=gen) * 0.2, torch.randn(128, generator=gen) * 0.2
    go = cl(torch.randn(T2.B, 128, T2.H, T2.W, generator=gen))
    return x, w1, b1, w2, b2, go


def _chain64(x, w1, b1, w2, b2, go):
    """float64 results of the chain and, for each, the bound on a TWO-piece run's deviation from float64 that follows from the
    per-product bound 2^-15 sum |a| |b| of test 4 by linearity and the triangle inequality: a product of an operand that
    already carries the deviation E adds (E convolved with the absolute value of the other operand), first order in 2^-15."""
    X, W1, W2, G = x.double(), w1.double(), w2.double(), go.double()
    fwd, dgr, wgr = SE.conv_op(1, 2, 2), SE.dgrad_op(1, 2, 2, (T2.H, T2.W)), SE.wgrad_op(1, 2, 2, 3)
    h = fwd(X, W1) + b1.double().view(1, -1, 1, 1)
    y = fwd(h, W2) + b2.double().view(1, -1, 1, 1)
    gh = dgr(G, W2)
    want = dict(y=y, dx=dgr(gh, W1), dw1=wgr(X, gh), dw2=wgr(h, G), db1=gh.sum((0, 2, 3)), db2=G.sum((0, 2, 3)))
    Eh = EPS2 * fwd(X.abs(), W1.abs())
    Egh = EPS2 * dgr(G.abs(), W2.abs())
    bound = dict(y=EPS2 * fwd(h.abs(), W2.abs()) + fwd(Eh, W2.abs()),
                 dx=EPS2 * dgr(gh.abs(), W1.abs()) + dgr(Egh, W1.abs()),
                 dw1=EPS2 * wgr(X.abs(), gh.abs()) + wgr(X.abs(), Egh),
                 dw2=EPS2 * wgr(h.abs(), G.abs()) + wgr(Eh, G.abs()),
                 db1=Egh.sum((0, 2, 3)))
    return want, bound


def _run(net, x, go, pieces, wg):
    net.pieces, net.wgrad = pieces, wg
    xg = x.to(DEV).clone().requires_grad_(True)
    y = net(xg)
    grads = torch.autograd.grad(y, [xg, net.c1.weight, net.c2.weight, net.c1.bias, net.c2.bias], go.to(DEV))
    return dict(zip(("y", "dx", "dw1", "dw2", "db1", "db2"), [t.detach().cpu() for t in (y,) + tuple(grads)]))


@pytest.mark.parametrize("wg", [False, True], ids=["library-wgrad", "split-wgrad"])
def test_autograd_two_pieces_against_three(hip, wg, monkeypatch):
    x, w1, b1, w2, b2, go = _two_convs_case()
    want, bound = _chain64(x, w1, b1, w2, b2, go)
    calls = []
    real3, real2 = SF.conv3x3_split_wgrad, SF.conv3x3_split_wgrad2
    monkeypatch.setattr(SF, "conv3x3_split_wgrad", lambda *a, **k: calls.append(3) or real3(*a, **k))
    monkeypatch.setattr(SF, "conv3x3_split_wgrad2", lambda *a, **k: calls.append(2) or real2(*a, **k))
    net = TwoConvs(w1, b1, w2, b2)
    r3 = _run(net, x, go, 3, wg)
    r2 = _run(net, x, go, 2, wg)
    assert calls == ([3, 3, 2, 2] if wg else []), calls
    for k in ("y", "dx", "dw1", "dw2", "db1"):
        e3 = float((r3[k].double() - want[k]).abs().max())
        diff = (r2[k].double() - r3[k].double()).abs()
        # |r2 - r3| <= |r2 - want| + |r3 - want| <= (bound + e3) + e3
        over = int((diff > bound[k] + 2 * e3).sum())
        print("AUTOGRAD wgrad=%s %s: max |two - three| %.3e, largest share of the bound %.4f, e3 %.3e"
              % (wg, k, float(diff.max()), float((diff / (bound[k] + 2 * e3)).max()), e3))
        assert over == 0, "%s: %d of %d elements of |two - three| above the bound" % (k, over, diff.numel())
        assert float(diff.max()) > 0, "%s: two pieces and three give the same bits" % k
    # the bias gradient is the library's sum of the gradient that reaches the convolution: for the last convolution that is the
    # given output gradient, the same in both runs -- the same bits; conv1's sees the two-piece data gradient (bounded above)
    assert torch.equal(r2["db2"], r3["db2"])

    # a weight update between two forwards is seen: the packs are rebuilt
    with torch.no_grad():
        net.c1.weight.mul_(1.5)
        net.c2.weight.add_(0.01)
    after = _run(net, x, go, 2, wg)
    fresh = TwoConvs(net.c1.weight.detach().cpu(), b1, net.c2.weight.detach().cpu(), b2)
    fresh2, fresh3 = _run(fresh, x, go, 2, wg), _run(fresh, x, go, 3, wg)
    assert not torch.equal(after["y"], r2["y"])
    # (compared bit for bit: what the split core computes -- the library's weight gradient need not repeat its bits)
    same = ("y", "dx") + (("dw1", "dw2") if wg else ())
    assert all(torch.equal(after[k], fresh2[k]) for k in same), "a stale two-plane pack was served after the update"
    # 2 -> 3 -> 2 on one owner, the weights written in between: each mode gets the image of its own count and of these weights
    assert all(torch.equal(_run(net, x, go, 3, wg)[k], fresh3[k]) for k in same)
    assert all(torch.equal(_run(net, x, go, 2, wg)[k], fresh2[k]) for k in same)
    with torch.no_grad():
        net.c1.weight.mul_(0.5)
    fresh = TwoConvs(net.c1.weight.detach().cpu(), b1, net.c2.weight.detach().cpu(), b2)
    want3, want2 = _run(fresh, x, go, 3, wg), _run(fresh, x, go, 2, wg)
    assert all(torch.equal(_run(net, x, go, 3, wg)[k], want3[k]) for k in same)
    assert all(torch.equal(_run(net, x, go, 2, wg)[k], want2[k]) for k in same), "a stale image after 2 -> 3 -> 2"
    assert not torch.equal(want2["y"], want3["y"])
    for conv_ in (net.c1, net.c2):
        assert conv_._skd_conv3x3_train_pack2[1].numel() * 3 == conv_._skd_conv3x3_train_pack[1].numel() * 2
        SF.drop_conv3x3_packs(conv_)
        assert not hasattr(conv_, "_skd_conv3x3_train_pack2") and not hasattr(conv_, "_skd_conv3x3_train_pack")


# ---- 7. one step --------------------------------------------------------------------------------------------------------------------

def test_one_step_student_pieces_2_against_3(monkeypatch):
    """The config-1 step of tests/test_step_gpu.py (batch 2, 256 x 256: the smallest the step tests use), same seed and inputs,
    with split_train and split_wgrad on: once on three pieces, once with SKD_STUDENT_PIECES=2.  The two-piece entries are
    counted through the library's kernel-timing hook; the first step's losses agree within 1e-4 relative (the project's parity
    contract); every parameter is finite after the step.  The per-tensor gradient deviations are printed, not bounded."""
    import test_step_gpu as TS
    # (entries the student alone calls: the frozen teacher's three-piece launches may sit inside its captured graph)
    counted = [PACK_PAIR2, RUN2, WGRAD2, "skd_conv3x3_split_pack_pair", "skd_conv3x3_split_wgrad_nhwc"]
    monkeypatch.setenv("SKD_SPLIT_TRAIN", "1")
    monkeypatch.setenv("SKD_SPLIT_WGRAD", "1")
    monkeypatch.delenv("SKD_TEACHER_PIECES", raising=False)
    runs = {}
    for pieces in (3, 2):
        monkeypatch.setenv("SKD_STUDENT_PIECES", str(pieces))
        _lib.enable_kernel_timing(counted)
        try:
            model, grads, _ = TS._config1_step(pa=True)
        finally:
            calls = _lib.disable_kernel_timing()
        assert model.split_train and model.split_wgrad and model.student_pieces == pieces
        losses = {k: float(getattr(model, k)) for k in ("mc_G_loss", "pi_G_loss", "pa_G_loss")}
        finite = all(bool(torch.isfinite(p).all()) for p in model.student.parameters())
        runs[pieces] = (losses, grads, {k: len(v) for k, v in calls.items()}, finite)
        del model
    n3, n2 = runs[3][2], runs[2][2]
    print("STEP calls three pieces: %s" % n3)
    print("STEP calls two pieces:   %s" % n2)
    assert n3[PACK_PAIR2] == n3[WGRAD2] == n3[RUN2] == 0, "the switch off calls no two-piece entry"
    assert (n2[PACK_PAIR2], n2[RUN2], n2[WGRAD2]) == (13, 26, 13), "13 pack pairs, 13 forwards + 13 data gradients, 13 weight gradients"
    assert n2["skd_conv3x3_split_pack_pair"] == 0 and n2["skd_conv3x3_split_wgrad_nhwc"] == 0
    assert (n3["skd_conv3x3_split_pack_pair"], n3["skd_conv3x3_split_wgrad_nhwc"]) == (13, 13)
    assert runs[2][3] and runs[3][3], "a parameter is not finite after the step"
    worst = []
    for k, g3 in runs[3][1].items():
        g2 = runs[2][1][k]
        rel = float((g2 - g3).norm()) / max(float(g3.norm()), 1e-30)
        worst.append((rel, k))
        print("STEP grad %-50s |g2 - g3| / |g3| = %.3e   max|g2 - g3| / max|g3| = %.3e"
              % (k, rel, float((g2 - g3).abs().max()) / max(float(g3.abs().max()), 1e-30)))
    print("STEP worst gradient deviation: %.3e %s" % max(worst))
    bad = []
    for k, l3 in runs[3][0].items():
        l2 = runs[2][0][k]
        rel = abs(l2 - l3) / abs(l3)
        print("STEP loss %s: three %.9g two %.9g rel %.3e" % (k, l3, l2, rel))
        if not rel <= 1e-4:
            bad.append((k, l3, l2, rel))
    assert not bad, bad
