"""-m gpu: the training form of the student's 1x1 down-sample (shortcut) convolutions on the split core (include/skd_shortcut.h,
csrc/conv1x1_train.hip, the one-tap form of csrc/conv3x3_wgrad.hip, functional.conv1x1_split_train): the entries through the C
ABI, the autograd op and one training step with the switch on.

Entry level: every operand, output and workspace of a call sits at exact size in the guard-band arena of tests/bounds_cases.py;
outputs are pre-filled with 0xFF (a NaN pattern), so an element the entry does not write shows -- the stride-2 gaps of ``dx``
must be +0.0, bit for bit.  Integer cases (x in [-7, 7], w and g in [-3, 3]: every partial sum is an exact fp32 integer in any
order) must meet float64 ``F.conv2d`` and its autograd on the CPU bit for bit, and sum fwd(x) . g == sum x . dgrad(g) exactly.
Realistic data: error figure max |got - want| / max |want| against the same float64 truth; bound of a case and product
min(RATIO x the parent's figure, CAP) with RATIO = 4 and CAP = 2e-5 of tests/test_conv3x3_split_gpu.py.  The parent's figure is
MIOpen's kernel for that product (``F.conv2d`` / ``aten.convolution_backward``) on exactly these inputs: PARENT_ERR, measured
once on an MI355X by tools/conv1x1_train_parent_err.py and tabulated beside the kernels' own figures in
profiles/r24_conv1x1_train_accuracy.md.
"""
import collections
import ctypes
import zlib

import pytest
import torch
import torch.nn.functional as F

import bounds_cases as BC
from structure_knowledge_distillation_amd import _lib, functional as SF
from test_conv3x3_split_gpu import CAP, DEV, RATIO, P, rel_err

pytestmark = pytest.mark.gpu

# (name, B, Cin, Cout, H, W, stride): the smallest shapes at which each mechanism can go wrong
CASES = [
    ("rows-tail-128-64-13x11-s1", 2, 128, 64, 13, 11, 1),      # two full row tiles and a 30-row tail; 64-column tile
    ("short-64-128-13x11-s2", 2, 64, 128, 13, 11, 2),          # 7 x 6 outputs, 84 rows: less than one tile; four K-tiles
    ("even-64-128-12x10-s2", 2, 64, 128, 12, 10, 2),           # the last input row and column are never read
    ("pixel-64-128-1x1-s2", 1, 64, 128, 1, 1, 2),              # single-pixel edge
    ("columns-128-256-9x9-s1", 1, 128, 256, 9, 9, 1),          # two column tiles
    ("longk-256-512-13x11-s1", 2, 256, 512, 13, 11, 1),        # K = 256; four column tiles
    ("rounds-128-64-161x161-s1", 4, 128, 64, 161, 161, 1),     # 811 row tiles: more than one round of a 256-CU device
]
# integers only (exact against float64, no parent figure needed): the stride-2 data gradient with Cin a multiple of 128, i.e.
# conv1x1_train_kernel<128, kMapY> (csrc/conv1x1_train.hip:165-172) -- every stride-2 case above has Cin = 64, the 64-column form
EXACT_ONLY = [("dgrad-wide-128-128-13x11-s2", 2, 128, 128, 13, 11, 2)]
CASE = {c[0]: c for c in CASES + EXACT_ONLY}
SMALL = [c[0] for c in CASES[:-1]]
PRODUCTS = ("fwd", "dgrad", "wgrad")

# max |parent - want| / max |want| of MIOpen's kernel for the product on exactly these inputs, measured once on an MI355X
# (profiles/r24_conv1x1_train_accuracy.md; tools/conv1x1_train_parent_err.py measures them again)
PARENT_ERR = {
    "rows-tail-128-64-13x11-s1": dict(fwd=1.044e-07, dgrad=1.669e-07, wgrad=1.492e-07),
    "short-64-128-13x11-s2": dict(fwd=2.081e-07, dgrad=1.589e-07, wgrad=8.653e-08),
    "even-64-128-12x10-s2": dict(fwd=1.166e-07, dgrad=1.335e-07, wgrad=1.068e-07),
    "pixel-64-128-1x1-s2": dict(fwd=1.003e-07, dgrad=9.768e-08, wgrad=3.051e-08),
    "columns-128-256-9x9-s1": dict(fwd=1.404e-07, dgrad=1.343e-07, wgrad=1.058e-07),
    "longk-256-512-13x11-s1": dict(fwd=1.170e-07, dgrad=1.761e-07, wgrad=1.593e-07),
    "rounds-128-64-161x161-s1": dict(fwd=3.631e-07, dgrad=3.171e-07, wgrad=1.118e-06),
}


@pytest.fixture(scope="module")
def hip():
    return _lib.load()


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def out_size(n, s):
    return (n - 1) // s + 1


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def real_inputs(name):
    """Seeded post-ReLU activations with a per-channel offset, a He-scaled weight and a normal output gradient."""
    _, b, cin, cout, h, w, s = CASE[name]
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    x = torch.relu(torch.randn(b, cin, h, w, generator=gen) + torch.randn(1, cin, 1, 1, generator=gen) * 0.5)
    wt = torch.randn(cout, cin, 1, 1, generator=gen) * (2.0 / cin) ** 0.5
    g = torch.randn(b, cout, out_size(h, s), out_size(w, s), generator=gen)
    return cl(x), wt, cl(g)


def int_inputs(name):
    _, b, cin, cout, h, w, s = CASE[name]
    gen = torch.Generator().manual_seed(zlib.crc32(("int-" + name).encode()))
    x = torch.randint(-7, 8, (b, cin, h, w), generator=gen).float()
    wt = torch.randint(-3, 4, (cout, cin, 1, 1), generator=gen).float()
    g = torch.randint(-3, 4, (b, cout, out_size(h, s), out_size(w, s)), generator=gen).float()
    assert 21 * max(cin, cout, b * g.shape[2] * g.shape[3]) < 2 ** 24
    return cl(x), wt, cl(g)


def truth64(x, wt, g, s):
    """(y, dx, dw) of ``F.conv2d(x, wt, None, s)`` and its autograd in float64 on the CPU."""
    xd, wd = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    y = F.conv2d(xd, wd, None, s)
    dx, dw = torch.autograd.grad(y, (xd, wd), g.double())
    return dict(fwd=y.detach(), dgrad=dx, wgrad=dw)


_WANT = {}


def want_of(name, ints=False):
    """float64 truth of a case, computed once and shared (never modified)."""
    key = (name, ints)
    if key not in _WANT:
        _WANT[key] = truth64(*(int_inputs if ints else real_inputs)(name), CASE[name][6])
    return _WANT[key]


def run_fwd(hip, x, wt, s, cols64=False):
    b, cin, h, w = x.shape
    cout = wt.shape[0]
    A = BC.Arena(DEV)
    xa, wa = A.inp("x", nhwc(x)), A.inp("w", wt.reshape(cout, cin).contiguous())
    y = A.out("y", (b, out_size(h, s), out_size(w, s), cout))
    f = hip.skd_conv1x1_train_fwd_cols64_nhwc if cols64 else hip.skd_conv1x1_train_fwd_nhwc
    assert f(b, h, w, cin, cout, s, P(xa), P(wa), P(y), None) == 1
    A.check()
    return y.cpu().permute(0, 3, 1, 2)


def run_dgrad(hip, g, wt, s, h, w, cols64=False):
    """dx from an output buffer pre-filled with 0xFF: every element must have been written, the stride-2 gaps with +0.0."""
    b, cout = g.shape[:2]
    cin = wt.shape[1]
    A = BC.Arena(DEV)
    ga, wa = A.inp("g", nhwc(g)), A.inp("wt", wt.reshape(cout, cin).t().contiguous())
    dx = A.out("dx", (b, h, w, cin))
    assert bool((dx.view(torch.uint8) == BC.FILL).all())
    f = hip.skd_conv1x1_train_dgrad_cols64_nhwc if cols64 else hip.skd_conv1x1_train_dgrad_nhwc
    assert f(b, h, w, cin, cout, s, P(ga), P(wa), P(dx), None) == 1
    A.check()
    got = dx.cpu()
    assert bool(torch.isfinite(got).all()), "an element of dx was not written"
    if s == 2:
        gap = torch.ones(h, w, dtype=torch.bool)
        gap[::2, ::2] = False
        assert bool((got[:, gap].view(torch.int32) == 0).all()), "a pixel no output reads is not +0.0"
    return got.permute(0, 3, 1, 2)


def plan_of(hip, x, cout, s, slices):
    b, cin, h, w = x.shape
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    plan = (ctypes.c_int64 * 3)()
    assert hip.skd_conv1x1_train_wgrad_plan(b, h, w, cin, cout, s, slices, cus, ctypes.cast(plan, ctypes.c_void_p)) == 1
    return int(plan[0]), int(plan[1]), int(plan[2])


def run_wgrad(hip, x, g, s, slices=0):
    """dw (Cout, Cin, 1, 1) from the two launches, called twice on the same guarded buffers (the workspace, 0xFF before the first
    call, left as the first call left it): same bits, guards intact."""
    b, cin, h, w = x.shape
    cout = g.shape[1]
    used, _, nbytes = plan_of(hip, x, cout, s, slices)
    assert nbytes == used * cin * cout * 4
    A = BC.Arena(DEV)
    xa, ga = A.inp("x", nhwc(x)), A.inp("g", nhwc(g))
    dw, ws = A.out("dw", (cout, cin)), A.ws("workspace", nbytes // 4)
    results = []
    for k in range(2):
        if k:
            A.reset()
        assert hip.skd_conv1x1_train_wgrad_nhwc(b, h, w, cin, cout, s, P(xa), P(ga), P(dw), P(ws), nbytes, used, None) == 1
        A.check()
        results.append(dw.cpu().clone())
    assert BC.same_bits(results[0], results[1]), "two calls on the same buffers differ"
    return results[0].reshape(cout, cin, 1, 1)


def run_product(hip, product, x, wt, g, s):
    if product == "fwd":
        return run_fwd(hip, x, wt, s)
    if product == "dgrad":
        return run_dgrad(hip, g, wt, s, x.shape[2], x.shape[3])
    return run_wgrad(hip, x, g, s)


# ---- 1. against float64 on realistic data ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("product", PRODUCTS)
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_product_vs_float64(hip, name, product):
    x, wt, g = real_inputs(name)
    err = rel_err(run_product(hip, product, x, wt, g, CASE[name][6]), want_of(name)[product])
    parent = PARENT_ERR[name][product]
    bound = min(RATIO * parent, CAP)
    print("%s %s: err %.3e  parent %.3e  bound %.3e" % (name, product, err, parent, bound))
    assert err <= bound, "%s %s: max err %.3e > %.3e (parent path: %.3e)" % (name, product, err, bound, parent)


# ---- 2. integers are exact ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SMALL + [c[0] for c in EXACT_ONLY])
def test_integers_bit_exact_and_adjoint(hip, name):
    s = CASE[name][6]
    x, wt, g = int_inputs(name)
    want = want_of(name, ints=True)
    y, dx = run_fwd(hip, x, wt, s), run_dgrad(hip, g, wt, s, x.shape[2], x.shape[3])
    assert torch.equal(y.double(), want["fwd"]), "%d outputs differ" % int((y.double() != want["fwd"]).sum())
    assert torch.equal(dx.double(), want["dgrad"]), "%d input gradients differ" % int((dx.double() != want["dgrad"]).sum())
    # the row map and the transpose, without torch's backward: sum fwd(x) . g == sum x . dgrad(g), exactly
    lhs, rhs = float((y.double() * g.double()).sum()), float((x.double() * dx.double()).sum())
    assert lhs == rhs and float(y.abs().max()) > 20.0, (lhs, rhs)
    nk = -(-g.shape[0] * g.shape[2] * g.shape[3] // 16)
    seen = {}
    for slices in (1, 2, 3, nk, 0):
        used = plan_of(hip, x, g.shape[1], s, slices)[0]
        if used not in seen:
            dw = seen[used] = run_wgrad(hip, x, g, s, slices)
            assert torch.equal(dw.double(), want["wgrad"]), "slices %d (%d used): %d of %d gradients differ" % (
                slices, used, int((dw.double() != want["wgrad"]).sum()), dw.numel())
    assert 1 in seen and nk in seen


# ---- 3. both tile widths give the same bits -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["short-64-128-13x11-s2", "even-64-128-12x10-s2", "columns-128-256-9x9-s1", "longk-256-512-13x11-s1",
                                  "rows-tail-128-64-13x11-s1"])
def test_bits_of_the_64_column_tiles(hip, name):
    """An N both tile widths take (Cout for the forward, Cin for the data gradient), on realistic data: equal bit for bit."""
    _, b, cin, cout, h, w, s = CASE[name]
    x, wt, g = real_inputs(name)
    compared = 0
    if cout % 128 == 0:
        wide, thin = run_fwd(hip, x, wt, s), run_fwd(hip, x, wt, s, cols64=True)
        assert float(wide.abs().max()) > 0.5 and torch.equal(wide, thin), "%d outputs differ" % int((wide != thin).sum())
        compared += 1
    if cin % 128 == 0:
        wide, thin = run_dgrad(hip, g, wt, s, h, w), run_dgrad(hip, g, wt, s, h, w, cols64=True)
        assert float(wide.abs().max()) > 0.5 and torch.equal(wide, thin), "%d input gradients differ" % int((wide != thin).sum())
        compared += 1
    assert compared


# ---- 4. the weight gradient's slices -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["rows-tail-128-64-13x11-s1", "short-64-128-13x11-s2", "pixel-64-128-1x1-s2", "columns-128-256-9x9-s1"])
def test_weight_gradient_slice_counts(hip, name):
    """One slice and several, a pixel count that is no multiple of 16 (286, 84, 81) and one smaller than a slice (1): every count
    the plan returns meets float64 within the case's bound, and run_wgrad's two calls on the same workspace give the same bits."""
    _, b, cin, cout, h, w, s = CASE[name]
    x, _, g = real_inputs(name)
    pixels = b * g.shape[2] * g.shape[3]
    nk = -(-pixels // 16)
    assert pixels % 16 != 0
    bound = min(RATIO * PARENT_ERR[name]["wgrad"], CAP)
    used_counts = set()
    for slices in (1, 2, 5, nk, nk + 3):
        used, per_slice, _ = plan_of(hip, x, cout, s, slices)
        assert used * per_slice >= nk > (used - 1) * per_slice
        if used in used_counts:
            continue
        used_counts.add(used)
        err = rel_err(run_wgrad(hip, x, g, s, slices), want_of(name)["wgrad"])
        print("%s slices %d (%d used): err %.3e  bound %.3e" % (name, slices, used, err, bound))
        assert err <= bound, (name, slices, err, bound)
    assert used_counts >= {1, nk}


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_buffers_alone(hip):
    b, cin, cout, h, w, s = 1, 64, 128, 13, 17, 2            # 7 x 9 = 63 output pixels: four K-tiles
    ho, wo = out_size(h, s), out_size(w, s)
    A = BC.Arena(DEV)
    xa, ga = A.inp("x", torch.ones(b, h, w, cin)), A.inp("g", torch.ones(b, ho, wo, cout))
    wa, wta = A.inp("w", torch.ones(cout, cin)), A.inp("wt", torch.ones(cin, cout))
    y, dx, dw = A.out("y", (b, ho, wo, cout)), A.out("dx", (b, h, w, cin)), A.out("dw", (cout, cin))
    used, _, nbytes = plan_of(hip, xa.permute(0, 3, 1, 2), cout, s, 2)
    assert used == 2
    ws = A.ws("workspace", nbytes // 4)
    fwd, dgrad, wgrad = hip.skd_conv1x1_train_fwd_nhwc, hip.skd_conv1x1_train_dgrad_nhwc, hip.skd_conv1x1_train_wgrad_nhwc
    off = lambda t, n: ctypes.c_void_p(t.data_ptr() + n)
    for f, a, m, o in ((fwd, xa, wa, y), (dgrad, ga, wta, dx)):
        assert not f(b, h, w, cin, cout, s, None, P(m), P(o), None)
        assert not f(b, h, w, cin, cout, s, P(a), None, P(o), None)
        assert not f(b, h, w, cin, cout, s, P(a), P(m), None, None)
        assert not f(b, h, w, cin, cout, s, off(a, 4), P(m), P(o), None)
        assert not f(b, h, w, cin, cout, s, P(a), off(m, 8), P(o), None)
        assert not f(0, h, w, cin, cout, s, P(a), P(m), P(o), None)
        assert not f(b, 0, w, cin, cout, s, P(a), P(m), P(o), None)
        assert not f(b, h, -1, cin, cout, s, P(a), P(m), P(o), None)
        assert not f(b, h, w, cin, cout, 0, P(a), P(m), P(o), None)
        assert not f(b, h, w, cin, cout, 3, P(a), P(m), P(o), None)
        assert not f(b, h, w, 32, cout, s, P(a), P(m), P(o), None)
        assert not f(b, h, w, cin, 96, s, P(a), P(m), P(o), None)
    for bad in (dict(x=None), dict(g=None), dict(dw=None), dict(ws=None), dict(x=off(xa, 4)), dict(g=off(ga, 8)), dict(ws=off(ws, 4)),
                dict(nbytes=nbytes - 1), dict(slices=0), dict(slices=3), dict(slices=5), dict(s=0), dict(s=3), dict(cin=32),
                dict(cout=96), dict(B=0), dict(H=0), dict(W=0)):
        a = dict(dict(B=b, H=h, W=w, cin=cin, cout=cout, s=s, x=P(xa), g=P(ga), dw=P(dw), ws=P(ws), nbytes=nbytes, slices=used), **bad)
        assert not wgrad(a["B"], a["H"], a["W"], a["cin"], a["cout"], a["s"], a["x"], a["g"], a["dw"], a["ws"], a["nbytes"],
                         a["slices"], None), bad
    A.check()
    for t in (y, dx, dw, ws):
        assert bool((t.view(torch.uint8) == BC.FILL).all())


# ---- 6. the op ------------------------------------------------------------------------------------------------------------------

class Counting:
    """The library with the launches of include/skd_shortcut.h counted."""

    def __init__(self, lib):
        self.lib, self.n = lib, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not (name.startswith("skd_conv1x1_train_") and name.endswith("_nhwc")):
            return fn

        def counted(*args):
            self.n[name.replace("skd_conv1x1_train_", "").replace("_nhwc", "")] += 1
            return fn(*args)
        return counted


@pytest.mark.parametrize("name", ["rows-tail-128-64-13x11-s1", "short-64-128-13x11-s2"])
def test_op_gives_the_entries_bits_and_falls_back_per_product(hip, name, monkeypatch):
    s = CASE[name][6]
    x, wt, g = real_inputs(name)
    entry = {p: run_product(hip, p, x, wt, g, s) for p in PRODUCTS}
    lib = Counting(hip)
    monkeypatch.setattr(_lib, "get", lambda: lib)
    xd, wd, gd = x.to(DEV), wt.to(DEV), g.to(DEV)

    def grads(products, need_x=True, need_w=True):
        xg, wg = xd.clone().requires_grad_(need_x), wd.clone().requires_grad_(need_w)
        assert SF.conv1x1_train_supported(xg, wg, s, 0, 1, 1)
        y = SF.conv1x1_split_train(xg, wg, s, torch.nn.Module(), products=products)
        assert y.is_contiguous(memory_format=torch.channels_last)
        ins = [t for t in (xg, wg) if t.requires_grad]
        return dict(zip(["fwd"] + [n for n, t in (("dgrad", xg), ("wgrad", wg)) if t.requires_grad],
                        (y.detach(),) + torch.autograd.grad(y, ins, gd)))
    got = grads(PRODUCTS)
    assert lib.n == dict(fwd=1, dgrad=1, wgrad=1)
    for p in PRODUCTS:
        assert torch.equal(got[p].cpu(), entry[p]), "%s is not the entry-level result, bit for bit" % p
    assert tuple(got["wgrad"].shape) == tuple(wd.shape)
    # the library's kernel for every product not listed; the listed ones keep their bits
    want = want_of(name)
    for products in (("fwd",), ("dgrad",), ("wgrad",), ("fwd", "wgrad"), ()):
        lib.n.clear()
        part = grads(products)
        assert lib.n == {p: 1 for p in products}, (products, lib.n)
        for p in PRODUCTS:
            if p in products:
                assert torch.equal(part[p].cpu(), entry[p]), (products, p)
            else:
                assert rel_err(part[p].cpu(), want[p]) <= CAP, (products, p)
    # needs_input_grad
    lib.n.clear()
    only_x, only_w = grads(PRODUCTS, need_w=False), grads(PRODUCTS, need_x=False)
    assert lib.n == dict(fwd=2, dgrad=1, wgrad=1)
    assert torch.equal(only_x["dgrad"].cpu(), entry["dgrad"]) and torch.equal(only_w["wgrad"].cpu(), entry["wgrad"])
    # a weight update between two forwards on the same owner is seen; one between forward and backward raises
    owner = torch.nn.Module()
    wg = wd.clone().requires_grad_(True)
    y0 = SF.conv1x1_split_train(xd, wg, s, owner).detach()
    mats = owner._skd_conv1x1_train_mats
    assert SF.conv1x1_split_train(xd, wg, s, owner) is not None and owner._skd_conv1x1_train_mats is mats
    with torch.no_grad():
        wg.mul_(2.0)
    xg = xd.clone().requires_grad_(True)
    y1 = SF.conv1x1_split_train(xg, wg, s, owner)
    assert torch.equal(y1.detach(), 2.0 * y0)
    assert torch.equal(torch.autograd.grad(y1, xg, gd, retain_graph=True)[0].cpu(), 2.0 * entry["dgrad"])
    with torch.no_grad():
        wg.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        torch.autograd.grad(y1, (xg, wg), gd)


# ---- 7. the step ----------------------------------------------------------------------------------------------------------------

def test_step_config1_with_the_shortcuts_on_the_core(monkeypatch):
    """The config-1 step of tests/test_step_gpu.py with ``split_train`` and ``split_shortcut`` on, at exactly the bounds of
    test_step_config1_vs_reference_golden: that test's own body runs, with the switches set where its ``default_args`` reads
    them.  The counting library sees four forward, four data-gradient and four weight-gradient calls, fewer by whatever
    SHORTCUT_ROUTING_EXCLUDED holds."""
    import structure_knowledge_distillation_amd.networks.pspnet_combine as PC
    import test_step_gpu as TS
    shapes = [(128, 64, 1), (64, 128, 2), (128, 256, 1), (256, 512, 1)]
    lib = Counting(_lib.load())
    monkeypatch.setattr(_lib, "get", lambda: lib)
    monkeypatch.setenv("SKD_SPLIT_TRAIN", "1")
    monkeypatch.setenv("SKD_SPLIT_SHORTCUT", "1")
    TS.test_step_config1_vs_reference_golden()
    want = {p: sum((cin, cout, s, p) not in PC.SHORTCUT_ROUTING_EXCLUDED for cin, cout, s in shapes) for p in PRODUCTS}
    assert dict(lib.n) == {p: n for p, n in want.items() if n}, (lib.n, want)
    assert all(e[3] in PRODUCTS and e[:3] in shapes for e in PC.SHORTCUT_ROUTING_EXCLUDED)
