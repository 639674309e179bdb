"""-m gpu: the 64-column form of the split-core 3x3 convolution (csrc/conv3x3_narrow.hip, include/skd_narrow.h): the entry, its
pack, the training op with ``narrow=True`` and the flagged student.

Value: truth is ``F.conv2d`` (+ the eval-mode ABN formula, residual, activation) in float64 on the CPU.  Error figure of a case:
max |hip - want| / max |want| over the whole output.  Bound of a case: FOUR times the figure the parent path -- MIOpen's fp32
``F.conv2d`` on the GPU, followed by the library's eval-mode ABN pass where the case has an epilogue -- gave on the same inputs, and
never more than 2e-5: figure, factor and cap of tests/test_conv3x3_split_gpu.py.  PARENT_ERR holds the parent's figures, measured
once on an MI355X by tools/conv3x3_narrow_parent_err.py; they and the kernel's own are tabulated in
profiles/r21_conv3x3_narrow_accuracy.md.  At a Cout both kernels take, the narrow entry must give the BITS of the wide one: it keeps
the core's product order and only assigns the output elements to other waves.  Integer data must be bit-exact.  Every launch
writes into a buffer with 160 sentinel rows behind row M; the guard-band cases put every buffer, at exactly its queried size,
between 0xFF bands (the arena of tests/bounds_cases.py).
"""
import zlib

import pytest
import torch
import torch.nn.functional as F

import bounds_cases as BC
import test_conv3x3_split_gpu as T3
from structure_knowledge_distillation_amd import _lib, functional as SF
from structure_knowledge_distillation_amd.networks import fuse_for_inference, pspnet_combine as PC
from test_conv3x3_split_gpu import ACT, CAP, DEV, RATIO, SENTINEL, SLACK_ROWS, P, epilogue64, rel_err

pytestmark = pytest.mark.gpu

# (name, B, Cin, Cout, H, W, dilation, epilogue)
CASES = [
    ("n-ragged-13x11-d1", 2, 32, 64, 13, 11, 1, "identity"),          # M = 286: ragged, rows cross image rows and images
    ("n-ragged-13x11-d2", 2, 32, 64, 13, 11, 2, "identity"),
    ("n-ragged-13x11-d4", 2, 32, 64, 13, 11, 4, "identity"),
    ("n-centre-5x5-d4", 1, 32, 64, 5, 5, 4, "identity"),              # almost every tap outside
    ("n-centre-3x3-d4", 1, 32, 64, 3, 3, 4, "identity"),
    ("n-oddk-16-64-13x11-d1", 2, 16, 64, 13, 11, 1, "identity"),      # nk = 9: the odd tail of k_loop
    ("n-longk-512-64-9x9-d4", 1, 512, 64, 9, 9, 4, "identity"),       # long K
    ("n-three-tiles-32-192-13x11-d2", 2, 32, 192, 13, 11, 2, "identity"),
    ("n-many-tiles-226x226-d1", 2, 16, 64, 226, 226, 1, "identity"),  # 798 panels: grid rounding to 8 XCDs
    ("n-ragged-13x11-d2-bias-abn-leaky", 2, 32, 64, 13, 11, 2, "bias-abn-leaky"),
    ("n-ragged-13x11-d2-bn-relu", 2, 32, 64, 13, 11, 2, "bn-relu"),
    ("n-ragged-13x11-d2-bn-res-relu", 2, 32, 64, 13, 11, 2, "bn-res-relu"),
]
CASE = {c[0]: c for c in CASES}

# max |parent - want| / max |want| of the parent path on exactly these inputs, measured once on an MI355X
# (profiles/r21_conv3x3_narrow_accuracy.md; tools/conv3x3_narrow_parent_err.py measures them again on these inputs)
PARENT_ERR = {
    "n-ragged-13x11-d1": 3.936e-07,
    "n-ragged-13x11-d2": 4.091e-07,
    "n-ragged-13x11-d4": 3.696e-07,
    "n-centre-5x5-d4": 3.587e-07,
    "n-centre-3x3-d4": 9.154e-08,
    "n-oddk-16-64-13x11-d1": 2.996e-07,
    "n-longk-512-64-9x9-d4": 4.321e-07,
    "n-three-tiles-32-192-13x11-d2": 4.636e-07,
    "n-many-tiles-226x226-d1": 4.337e-07,
    "n-ragged-13x11-d2-bias-abn-leaky": 3.786e-07,
    "n-ragged-13x11-d2-bn-relu": 3.115e-07,
    "n-ragged-13x11-d2-bn-res-relu": 2.739e-07,
}

# the training op, (name, Cin, Cout) at (2, 13 x 11), dilation 1: figures of MIOpen's forward and backward-data kernels
TRAIN_CASES = [("t-64-64", 64, 64), ("t-64-128", 64, 128), ("t-128-64", 128, 64)]
PARENT_TRAIN_ERR = {
    "t-64-64": (3.791e-07, 4.155e-07),
    "t-64-128": (4.409e-07, 4.670e-07),
    "t-128-64": (3.404e-07, 4.559e-07),
}


@pytest.fixture(scope="module")
def hip():
    return _lib.load()


def case_inputs(name):
    """Seeded inputs of a case, as tests/test_conv3x3_split_gpu.py makes them; ``res``: the residual of the case that has one."""
    _, b, cin, cout, h, w, d, epi = CASE[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    x = torch.relu(torch.randn(b, cin, h, w, generator=g) + torch.randn(1, cin, 1, 1, generator=g) * 0.5)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    p = {"cbias": None, "mean": None, "var": None, "gamma": None, "beta": None, "eps": 0.0, "act": "none", "res": None}
    if epi != "identity":
        p.update(mean=torch.randn(cout, generator=g) * 0.3, var=torch.rand(cout, generator=g) + 0.5,
                 gamma=torch.randn(cout, generator=g), beta=torch.randn(cout, generator=g), eps=1e-5)
        if epi == "bias-abn-leaky":
            p.update(cbias=torch.randn(cout, generator=g) * 0.2, act="leaky_relu")
        else:
            p.update(act="relu")
        if epi == "bn-res-relu":
            p.update(res=torch.randn(b, cout, h, w, generator=g).contiguous(memory_format=torch.channels_last))
    return x.contiguous(memory_format=torch.channels_last), wt, p


_WANT = {}


def want_of(name):
    """float64 truth of a case on the CPU, computed once and shared (never modified)."""
    if name not in _WANT:
        x, wt, p = case_inputs(name)
        d = CASE[name][6]
        y = F.conv2d(x.double(), wt.double(), None if p["cbias"] is None else p["cbias"].double(), 1, d, d)
        if p["res"] is None:
            _WANT[name] = epilogue64(y, p)
        else:                                   # the residual sits behind the normalisation, in front of the activation
            z = epilogue64(y, dict(p, act="none")) + p["res"].double()
            _WANT[name] = torch.relu(z)
    return _WANT[name]


def narrow_pack(hip, wt_dev, fwd=True, bwd=False):
    """(pack_fwd or None, pack_bwd or None) of a device weight view at exactly the queried sizes, one launch."""
    cout, cin = wt_dev.shape[:2]
    nf, nb = hip.skd_conv3x3_narrow_pack_bytes(cin, cout), hip.skd_conv3x3_narrow_pack_bytes(cout, cin)
    pf = torch.empty(nf, dtype=torch.uint8, device=DEV) if fwd else None
    pb = torch.empty(nb, dtype=torch.uint8, device=DEV) if bwd else None
    assert (not fwd or nf == cout * cin * 54) and (not bwd or nb == cout * cin * 54)
    sn, sc, sy, sx = wt_dev.stride()
    assert hip.skd_conv3x3_narrow_pack_pair(cin, cout, P(wt_dev), sn, sc, sy, sx, P(pf), nf if fwd else 0, P(pb), nb if bwd else 0, None)
    return pf, pb


def launch(hip, dx, pk, cout, d, p=None, geometry=0):
    """One launch of the narrow entry on a channels-last device map: (B, cout, H, W) on the CPU; checks the sentinel rows."""
    b, cin, h, w = dx.shape
    m = b * h * w
    p = p or {"cbias": None, "mean": None, "var": None, "gamma": None, "beta": None, "eps": 0.0, "act": "none", "res": None}
    dp = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in p.items()}
    out = torch.full((m + SLACK_ROWS, cout), SENTINEL, device=DEV)
    assert hip.skd_conv3x3_narrow_nhwc(b, h, w, cin, cout, d, P(dx), P(pk), P(out), P(dp["res"]), P(dp["cbias"]), P(dp["mean"]),
                                       P(dp["var"]), P(dp["gamma"]), P(dp["beta"]), p["eps"], ACT[p["act"]], 0.01, geometry, None)
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool((out[m:] == SENTINEL).all()), "rows beyond M were written"
    return out[:m].view(b, h, w, cout).permute(0, 3, 1, 2)


def run_narrow(hip, x, wt, p, d, geometry=0, wt_format=torch.contiguous_format):
    dx = x.to(DEV).contiguous(memory_format=torch.channels_last)
    dw = wt.to(DEV).contiguous(memory_format=wt_format)
    return launch(hip, dx, narrow_pack(hip, dw)[0], wt.shape[0], d, p, geometry)


# ---- 1. value against float64 -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_narrow_conv3x3_vs_float64(hip, name):
    x, wt, p = case_inputs(name)
    got = run_narrow(hip, x, wt, p, CASE[name][6])
    err = rel_err(got, want_of(name))
    bound = min(RATIO * PARENT_ERR[name], CAP)
    print("%s: err %.3e  parent %.3e  bound %.3e" % (name, err, PARENT_ERR[name], bound))
    assert err <= bound, "%s: max err %.3e > %.3e (parent path: %.3e)" % (name, err, bound, PARENT_ERR[name])


# ---- 2. the bits of the wide kernel -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("cout", [128, 256])
@pytest.mark.parametrize("epi", ["identity", "bias-abn-leaky"])
def test_bits_of_the_wide_kernel(hip, cout, epi):
    """Every output element sees the wide kernel's operations in its order; only the assignment of elements to waves changes."""
    g = torch.Generator().manual_seed(cout)
    x = torch.relu(torch.randn(2, 32, 13, 11, generator=g)).contiguous(memory_format=torch.channels_last)
    wt = torch.randn(cout, 32, 3, 3, generator=g) * (2.0 / (9 * 32)) ** 0.5
    p = {"cbias": None, "mean": None, "var": None, "gamma": None, "beta": None, "eps": 0.0, "act": "none", "res": None}
    if epi != "identity":
        p.update(mean=torch.randn(cout, generator=g) * 0.3, var=torch.rand(cout, generator=g) + 0.5, gamma=torch.randn(cout, generator=g),
                 beta=torch.randn(cout, generator=g), eps=1e-5, cbias=torch.randn(cout, generator=g) * 0.2, act="leaky_relu")
    wide, _ = T3.run_hip(hip, x, wt, {k: v for k, v in p.items() if k != "res"}, 2)
    got = run_narrow(hip, x, wt, p, 2)
    assert float(wide.abs().max()) > 0.1
    assert torch.equal(got, wide), "%d of %d outputs differ from skd_conv3x3_split_nhwc" % (int((got != wide).sum()), got.numel())


def test_residual_is_one_fp32_add_behind_the_bn_expression(hip):
    """With a residual r: the bits of relu(z + r) in fp32, z the same launch's ``activation = none`` output without it; and with
    leaky ReLU behind the same sum, the bits of its fp32 expression (slope 0.01, the value ``launch`` passes)."""
    name = "n-ragged-13x11-d2-bn-res-relu"
    x, wt, p = case_inputs(name)
    z = run_narrow(hip, x, wt, dict(p, res=None, act="none"), 2)
    got = run_narrow(hip, x, wt, p, 2)
    want = torch.relu(z + p["res"])
    assert torch.equal(got, want) and not torch.equal(got, torch.relu(z))
    v = z + p["res"]
    leaky = run_narrow(hip, x, wt, dict(p, act="leaky_relu"), 2)
    assert torch.equal(leaky, torch.where(v < 0, v * torch.tensor(0.01), v)) and bool((v < 0).any())


# ---- 3. integers, geometries, weight layout ---------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(2, 13, 11, 2), (1, 5, 5, 4), (2, 40, 37, 1)], ids=["13x11-d2", "5x5-d4", "40x37-d1"])
def test_integers_bit_exact(hip, shape):
    b, h, w, d = shape
    cin, cout = 32, 64
    assert 9 * cin * 7 * 3 < 2 ** 24       # every partial sum is an exact fp32 integer, in any order
    g = torch.Generator().manual_seed(100 * h + d)
    x = torch.randint(-7, 8, (b, cin, h, w), generator=g).float().contiguous(memory_format=torch.channels_last)
    wt = torch.randint(-3, 4, (cout, cin, 3, 3), generator=g).float()
    got = run_narrow(hip, x, wt, None, d)
    want = F.conv2d(x.double(), wt.double(), None, 1, d, d)
    assert float(want.abs().max()) > 100.0
    assert torch.equal(got.double(), want), "%d of %d outputs differ" % (int((got.double() != want).sum()), got.numel())


@pytest.mark.parametrize("geometry", [1])
def test_every_geometry_gives_the_same_bits(hip, geometry):
    for name in ("n-many-tiles-226x226-d1", "n-ragged-13x11-d2-bn-res-relu"):
        x, wt, p = case_inputs(name)
        d = CASE[name][6]
        assert torch.equal(run_narrow(hip, x, wt, p, d, geometry=geometry), run_narrow(hip, x, wt, p, d))


# ---- 4. pack bits -----------------------------------------------------------------------------------------------------------

def narrow_image(wt):
    """The packed image of a (N, C, 3, 3) fp32 weight as torch computes it on the CPU, from the layout comment of
    csrc/conv3x3_narrow.hip alone: per (column tile tn of 64 rows, K-tile kt of 16 k), tile index tn * nk + kt with
    nk = 9 C / 16, three planes of 128 16-byte chunks; chunk kh * 64 + (row ^ 4 kh) holds the 8 bf16 of k = 16 kt + 8 kh + i in
    ascending i, k = tap * C + c, tap = 3 ty + tx; plane j is piece p_j of v = p0 + p1 + p2, each rounded to nearest even."""
    n, c = wt.shape[:2]
    m = wt.permute(0, 2, 3, 1).reshape(n // 64, 64, 9 * c // 16, 2, 8).permute(0, 2, 3, 1, 4)      # (tn, kt, kh, row, i)
    m = torch.stack([m[:, :, 0], m[:, :, 1][:, :, torch.arange(64) ^ 4]], 2).contiguous()          # chunk row' = row ^ 4 kh
    planes = []
    for _ in range(3):
        piece = m.bfloat16()
        planes.append(piece.view(torch.int16))
        m = m - piece.float()
    return torch.stack(planes, 2).contiguous().view(torch.uint8).reshape(-1)                       # (tn, kt, plane, chunk, i)


def _weight_view(A, wt, layout):
    if layout == "contiguous":
        return A.inp("w", wt)
    if layout == "channels_last":
        return A.inp("w", wt.permute(0, 2, 3, 1).contiguous()).permute(0, 3, 1, 2)
    wide = torch.cat([torch.full((wt.shape[0], 64, 3, 3), float("nan")), wt], 1)
    return A.inp("w", wide)[:, 64:]


@pytest.mark.parametrize("layout", ["contiguous", "channels_last", "slice"])
@pytest.mark.parametrize("cout,cin", [(64, 16), (64, 64), (192, 32), (128, 64), (64, 128)])
def test_pack_pair_bits(hip, cout, cin, layout):
    """Both images against narrow_image, between guard bands at exactly the queried sizes.  The backward image is the same
    function of Wd[c][n][ty][tx] = W[n][c][2 - ty][2 - tx]; it needs Cin a multiple of 64 (and Cout of 16)."""
    g = torch.Generator().manual_seed(cout + 3 * cin)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    wt[0, 0, 0, 1], wt[1, 2, 2, 0] = 1e-30, -3.0e4                 # a tiny and a large value: the residual pieces
    nbytes = cout * cin * 54
    want_f = narrow_image(wt).to(DEV)
    assert want_f.numel() == nbytes == hip.skd_conv3x3_narrow_pack_bytes(cin, cout)
    forms, want_b = [(True, False)], None
    if cin % 64 == 0:
        want_b = narrow_image(wt.flip(2, 3).transpose(0, 1).contiguous()).to(DEV)
        assert want_b.numel() == nbytes == hip.skd_conv3x3_narrow_pack_bytes(cout, cin) and not torch.equal(want_f, want_b)
        forms += [(True, True), (False, True)]
    for fwd, bwd in forms:
        A = BC.Arena(DEV)
        w = _weight_view(A, wt, layout)
        assert tuple(w.shape) == (cout, cin, 3, 3) and (layout == "contiguous") == w.is_contiguous()
        pf, pb = A.out("pack_fwd", nbytes, torch.uint8), A.out("pack_bwd", nbytes, torch.uint8)
        sn, sc, sy, sx = w.stride()
        assert hip.skd_conv3x3_narrow_pack_pair(cin, cout, P(w), sn, sc, sy, sx, P(pf) if fwd else None, nbytes,
                                                P(pb) if bwd else None, nbytes, None)
        A.check()
        assert torch.equal(pf, want_f) if fwd else bool((pf == BC.FILL).all()), (layout, fwd, bwd)
        assert torch.equal(pb, want_b) if bwd else bool((pb == BC.FILL).all()), (layout, fwd, bwd)


def test_narrow_image_of_a_128_row_weight_is_the_wide_image_retiled(hip):
    """Same values, other tiles: wide tile (tn, kt), plane p, chunk kh * 128 + r' holds narrow tile (2 tn + r' // 64, kt), plane p,
    chunk kh * 64 + r' % 64 -- the XOR with 4 kh stays inside a block of 64 rows."""
    g = torch.Generator().manual_seed(5)
    wt = (torch.randn(256, 32, 3, 3, generator=g) * 0.1).to(DEV)
    wide = T3.pack(hip, wt).view(2, 18, 3, 2, 2, 64, 16)            # (tn, kt, plane, kh, half, row, byte)
    narrow = narrow_pack(hip, wt)[0].view(2, 2, 18, 3, 2, 64, 16)   # (tn, half, kt, plane, kh, row, byte)
    assert torch.equal(narrow, wide.permute(0, 4, 1, 2, 3, 5, 6))


def test_pack_pair_refusals_leave_the_buffers_alone(hip):
    A = BC.Arena(DEV)
    w = A.inp("w", torch.zeros(64, 64, 3, 3))
    n = 64 * 64 * 54
    pf, pb = A.out("pack_fwd", n, torch.uint8), A.out("pack_bwd", n, torch.uint8)
    f = hip.skd_conv3x3_narrow_pack_pair
    assert not f(64, 64, P(w), 576, 9, 3, 1, None, n, None, n, None)
    assert not f(64, 64, P(w), 576, 9, 3, 1, P(pf), n - 1, P(pb), n, None)
    assert not f(64, 64, P(w), 576, 9, 3, 1, P(pf), n, P(pb), n - 1, None)
    assert not f(64, 64, P(w), -576, 9, 3, 1, P(pf), n, P(pb), n, None)
    assert not f(64, 32, P(w), 576, 9, 3, 1, P(pf), n, P(pb), n, None)
    assert not f(64, 64, None, 576, 9, 3, 1, P(pf), n, P(pb), n, None)
    A.check()
    assert bool((pf == BC.FILL).all()) and bool((pb == BC.FILL).all())


# ---- 5. guard bands ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["n-ragged-13x11-d2-bn-res-relu", "n-centre-3x3-d4", "n-three-tiles-32-192-13x11-d2",
                                  "n-ragged-13x11-d2-bias-abn-leaky"])
def test_guard_bands(hip, name):
    """Input, weight, pack, residual (exactly M * Cout floats), epilogue vectors and output between 0xFF guards (NaN as fp32): no
    guard byte changes, and neither a stray read nor an unwritten element leaves a NaN in the output."""
    _, b, cin, cout, h, w, d, _ = CASE[name]
    x, wt, p = case_inputs(name)
    A = BC.Arena(DEV)
    dx = A.inp("x", x.permute(0, 2, 3, 1).contiguous(), row=cin)
    dw = A.inp("weight", wt)
    nbytes = hip.skd_conv3x3_narrow_pack_bytes(cin, cout)
    pk = A.out("pack", nbytes, torch.uint8)
    r = A.inp("residual", None if p["res"] is None else p["res"].permute(0, 2, 3, 1).contiguous(), row=cout)
    vec = {k: A.inp(k, p[k]) for k in ("cbias", "mean", "var", "gamma", "beta")}
    out = A.out("out", (b * h * w, cout), row=cout)
    assert hip.skd_conv3x3_narrow_pack_pair(cin, cout, P(dw), *dw.stride(), P(pk), nbytes, None, 0, None)
    A.check()
    args = (b, h, w, cin, cout, d, P(dx), P(pk), P(out), P(r), P(vec["cbias"]), P(vec["mean"]), P(vec["var"]), P(vec["gamma"]),
            P(vec["beta"]), p["eps"], ACT[p["act"]], 0.01, 0, None)
    assert hip.skd_conv3x3_narrow_nhwc(*args) == 1
    A.check()
    assert not bool(torch.isnan(out).any())
    assert torch.equal(out.cpu().view(b, h, w, cout).permute(0, 3, 1, 2), run_narrow(hip, x, wt, p, d))
    # a residual that overlaps the output: refused on the host, nothing is written
    before = out.clone()
    assert hip.skd_conv3x3_narrow_nhwc(*(args[:9] + (P(out),) + args[10:])) == 0
    A.check()
    assert torch.equal(out, before)


# ---- 6. the training op -----------------------------------------------------------------------------------------------------

def train_inputs(name):
    _, cin, cout = next(c for c in TRAIN_CASES if c[0] == name)
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    x = torch.relu(torch.randn(2, cin, 13, 11, generator=g) + torch.randn(1, cin, 1, 1, generator=g) * 0.5)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    go = torch.randn(2, cout, 13, 11, generator=g)
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    return cl(x), cl(wt), cl(go)


_TRAIN_WANT = {}


def train_want(name):
    """(y, dx) of F.conv2d and its autograd in float64 on the CPU, computed once."""
    if name not in _TRAIN_WANT:
        x, wt, go = train_inputs(name)
        x64 = x.double().requires_grad_(True)
        y = F.conv2d(x64, wt.double(), None, 1, 1, 1)
        (dx,) = torch.autograd.grad(y, x64, go.double())
        _TRAIN_WANT[name] = (y.detach(), dx)
    return _TRAIN_WANT[name]


def run_train_op(name):
    """(y, dx, dw, a library dw) of conv3x3_split_train(..., narrow=True) on the device."""
    x, wt, go = train_inputs(name)
    xg, wg, god = x.to(DEV).requires_grad_(True), wt.to(DEV).requires_grad_(True), go.to(DEV)
    assert SF.conv3x3_narrow_train_supported(xg, wg, 1, 1, 1, 1)
    assert SF.conv3x3_train_supported(xg, wg, 1, 1, 1, 1) == (wt.shape[0] % 128 == 0 and wt.shape[1] % 128 == 0)
    y = SF.conv3x3_split_train(xg, wg, 1, None, torch.nn.Module(), narrow=True)
    dx, dw = torch.autograd.grad(y, (xg, wg), god)
    _, lib_dw, _ = torch.ops.aten.convolution_backward(god, xg.detach(), wg.detach(), None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1,
                                                       (False, True, False))
    return y.detach(), dx, dw, lib_dw


@pytest.mark.parametrize("name", [c[0] for c in TRAIN_CASES])
def test_training_op_vs_float64(hip, name):
    y, dx, dw, lib_dw = run_train_op(name)
    want_y, want_dx = train_want(name)
    for what, got, want, parent in (("forward", y, want_y, PARENT_TRAIN_ERR[name][0]), ("dgrad", dx, want_dx, PARENT_TRAIN_ERR[name][1])):
        err, bound = rel_err(got.cpu(), want), min(RATIO * parent, CAP)
        print("%s %s: err %.3e  parent %.3e  bound %.3e" % (name, what, err, parent, bound))
        assert err <= bound, "%s %s: max err %.3e > %.3e (parent path: %.3e)" % (name, what, err, bound, parent)
    assert y.is_contiguous(memory_format=torch.channels_last) and dx.is_contiguous(memory_format=torch.channels_last)
    # the weight gradient is the library's.  MIOpen's weight-gradient kernel at these shapes does not repeat its own bits (three
    # calls on the same inputs gave three results, up to 1.9e-5 apart at values near 16: atomics), so "equal" is the contract of
    # tests/test_conv3x3_train_gpu.py for dw -- no further from float64 than the library's own call -- and the split-core weight
    # gradient is never asked for (checked below with the wgrad switch on).
    x64, w64 = train_inputs(name)[0].double(), train_inputs(name)[1].double().requires_grad_(True)
    (want_dw,) = torch.autograd.grad(F.conv2d(x64, w64, None, 1, 1, 1), w64, train_inputs(name)[2].double())
    err, base = (float((t.cpu().double() - want_dw).norm()) for t in (dw, lib_dw))
    norm = float(want_dw.norm())
    print("%s dw: op %.3e  library %.3e  (of |want| = %.3e)" % (name, err, base, norm))
    assert dw.shape == lib_dw.shape and dw.stride() == lib_dw.stride() and err <= 4.0 * base + 1e-6 * norm, (err, base, norm)
    # each direction on the entry its N chooses: the bits of the entry-level launches
    x, wt, go = train_inputs(name)
    cin, cout = wt.shape[1], wt.shape[0]
    dwt = wt.to(DEV)
    if cout % 128 == 0:
        fwd, _ = T3.run_hip(hip, x, wt, {"cbias": None, "mean": None, "var": None, "gamma": None, "beta": None, "eps": 0.0, "act": "none"}, 1)
    else:
        fwd = launch(hip, x.to(DEV), narrow_pack(hip, dwt)[0], cout, 1)
    assert torch.equal(y.cpu(), fwd)
    if cin % 128 != 0:
        assert torch.equal(dx.cpu(), launch(hip, go.to(DEV), narrow_pack(hip, dwt, fwd=False, bwd=True)[1], cin, 1))


def test_narrow_shapes_never_reach_the_split_core_weight_gradient(monkeypatch):
    """``wgrad=True`` with ``narrow=True``: a shape with a 64-channel side keeps the library's weight gradient."""
    calls = []
    real = SF.conv3x3_split_wgrad
    monkeypatch.setattr(SF, "conv3x3_split_wgrad", lambda *a, **k: calls.append(1) or real(*a, **k))
    x, wt, go = train_inputs("t-64-128")
    xg, wg = x.to(DEV).requires_grad_(True), wt.to(DEV).requires_grad_(True)
    y = SF.conv3x3_split_train(xg, wg, 1, None, None, wgrad=True, narrow=True)
    _, dw = torch.autograd.grad(y, (xg, wg), go.to(DEV))
    assert calls == [] and dw.shape == wg.shape


@pytest.mark.parametrize("cin,cout", [(64, 64), (64, 128), (128, 64)])
def test_training_op_integers_bit_exact(cin, cout):
    g = torch.Generator().manual_seed(cin + 2 * cout)
    assert 9 * 128 * 7 * 3 < 2 ** 24
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    x = cl(torch.randint(-7, 8, (2, cin, 13, 11), generator=g).float())
    wt = cl(torch.randint(-3, 4, (cout, cin, 3, 3), generator=g).float())
    go = cl(torch.randint(-7, 8, (2, cout, 13, 11), generator=g).float())
    xg = x.to(DEV).requires_grad_(True)
    y = SF.conv3x3_split_train(xg, wt.to(DEV).requires_grad_(True), 1, None, None, narrow=True)
    (dx,) = torch.autograd.grad(y, xg, go.to(DEV))
    x64 = x.double().requires_grad_(True)
    want = F.conv2d(x64, wt.double(), None, 1, 1, 1)
    (want_dx,) = torch.autograd.grad(want, x64, go.double())
    assert torch.equal(y.detach().cpu().double(), want.detach()) and torch.equal(dx.cpu().double(), want_dx)


def test_fused_sgd_step_rebuilds_the_narrow_packs():
    from structure_knowledge_distillation_amd.networks.kd_model import advance_versions_after_step
    x, wt, go = train_inputs("t-64-128")
    w = torch.nn.Parameter(wt.to(DEV))
    owner = torch.nn.Module()
    opt = torch.optim.SGD([w], 0.5, momentum=0.9, fused=True)
    opt.register_step_post_hook(advance_versions_after_step)
    xd = x.to(DEV).requires_grad_(True)
    y0 = SF.conv3x3_split_train(xd, w, 1, owner=owner, narrow=True)
    (dx0,) = torch.autograd.grad(y0, xd, go.to(DEV), retain_graph=True)
    y0.backward(go.to(DEV))
    opt.step()
    y1 = SF.conv3x3_split_train(xd, w, 1, owner=owner, narrow=True)
    (dx1,) = torch.autograd.grad(y1, xd, go.to(DEV))
    fresh = SF.conv3x3_split_train(xd, w.detach().clone().requires_grad_(True), 1, narrow=True)
    (dxf,) = torch.autograd.grad(fresh, xd, go.to(DEV))
    assert torch.equal(y1.detach(), fresh.detach()) and torch.equal(dx1, dxf)
    assert not torch.equal(y1.detach(), y0.detach()) and not torch.equal(dx1, dx0)


# ---- 7. the model -------------------------------------------------------------------------------------------------------------

NARROW = "skd_conv3x3_narrow_nhwc"


def test_whole_student_vs_float64_fixture():
    """The narrow-flagged student's eval forward against tests/golden/student_infer_oracle.pt at the tolerance
    tests/test_student_infer_gpu.py applies to the fused form: at most four times the unflagged form's error on the same GPU."""
    import test_student_infer_gpu as TI
    import make_golden_student_infer as G
    fx = torch.load(G.OUT, weights_only=False)
    Pw, x = G.inputs()
    S = PC.Res_pspnet(PC.BasicBlock, [2, 2, 2, 2], 19)
    S.load_state_dict(Pw)
    S = S.to(DEV).to(memory_format=torch.channels_last).eval()
    dx = x.to(DEV).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        _lib.enable_kernel_timing([NARROW, "skd_conv3x3_split_nhwc", "skd_conv3x3_split_res_nhwc"])
        try:
            plain = S(dx)
        finally:
            unflagged = _lib.disable_kernel_timing()
        _lib.enable_kernel_timing([NARROW, "skd_conv3x3_split_nhwc"])
        try:
            wide_only = fuse_for_inference(S)(dx)
        finally:
            off = _lib.disable_kernel_timing()
        _lib.enable_kernel_timing([NARROW, "skd_conv3x3_split_nhwc", "skd_conv3x3_split_res_nhwc"])
        try:
            fused = fuse_for_inference(S, narrow=True)(dx)
        finally:
            on = _lib.disable_kernel_timing()
    assert len(off[NARROW]) == 0, "without the switch nothing reaches the narrow entry"
    assert len(on[NARROW]) == 5, "stem conv2 and layer1's four convolutions"
    assert len(on["skd_conv3x3_split_nhwc"]) == len(off["skd_conv3x3_split_nhwc"]) + 1, "stem conv3 on the wide entry"
    assert len(on["skd_conv3x3_split_res_nhwc"]) == 6
    for name, a, b, c, r in zip(fx["names"], plain, fused, wide_only, fx["outputs"]):
        e_plain, e_fused = TI._rec_err(a, r), TI._rec_err(b, r)
        print("%-18s unflagged %.3e  narrow-flagged %.3e of the norm, ratio %.2f" % (name, e_plain / r["norm"], e_fused / r["norm"],
                                                                                     e_fused / e_plain))
        assert e_fused <= RATIO * e_plain, name
        assert not torch.equal(b, c), "the switch changed nothing"
    # enable=False: the launches of the unflagged student again, and no pack left.  (Not its bits: two unflagged forwards of this
    # student do not give equal bits on this library stack -- measured, every output differs -- so there is nothing to pin them to;
    # tests/test_conv3x3_narrow_cpu.py pins the restored op sequence under the double.)
    with torch.no_grad():
        _lib.enable_kernel_timing([NARROW, "skd_conv3x3_split_nhwc", "skd_conv3x3_split_res_nhwc"])
        try:
            after = fuse_for_inference(S, enable=False)(dx)
        finally:
            cleared = _lib.disable_kernel_timing()
    assert {k: len(v) for k, v in cleared.items()} == {k: len(v) for k, v in unflagged.items()} and len(cleared[NARROW]) == 0
    assert not any(hasattr(m, a) for m in S.modules() for a in ("_skd_conv3x3_narrow_pack",) + SF._NARROW_PACK_ATTRS)
    for name, a, r in zip(fx["names"], after, fx["outputs"]):
        assert TI._rec_err(a, r) <= RATIO * TI._rec_err(plain[fx["names"].index(name)], r), name


def test_step_config1_with_the_narrow_form(monkeypatch):
    """The config-1 step of tests/test_step_gpu.py with ``split_train`` and ``split_narrow`` on, at exactly the bounds of
    test_step_config1_vs_reference_golden: that test's own body runs, with the switches set where its ``default_args`` reads
    them.  A counting shim sees the narrow launches: the forward of stem conv2 and of layer1's four (layer1.0.conv1 reads 128
    channels), the data gradient of stem conv2, stem conv3 (128 -> 64) and the three 64 -> 64 of layer1 -- layer1.0.conv1's has
    N = 128 and runs on the wide entry; with SKD_SPLIT_NARROW=0, none."""
    import test_step_gpu as TS
    real = SF._conv3x3_raw_launch
    seen = []

    def shim(form, x, pack, cout, dilation, conv_bias=None):      # training's one raw launcher: the narrow launches by their entry
        if form.conv == NARROW:
            seen.append((int(x.shape[1]), int(cout)))
        return real(form, x, pack, cout, dilation, conv_bias)
    monkeypatch.setattr(SF, "_conv3x3_raw_launch", shim)

    monkeypatch.setenv("SKD_SPLIT_TRAIN", "1")
    monkeypatch.setenv("SKD_SPLIT_NARROW", "0")
    model, _, _ = TS._config1_step(pa=True)
    assert model.split_train and not model.split_narrow and seen == []
    del model

    monkeypatch.setenv("SKD_SPLIT_NARROW", "1")
    TS.test_step_config1_vs_reference_golden()
    assert sorted(seen) == [(64, 64)] * 8 + [(128, 64)] * 2, seen
