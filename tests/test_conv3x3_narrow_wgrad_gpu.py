"""-m gpu: the weight gradient of the student's 64-channel 3x3 convolutions on the split core (include/skd_narrow_wgrad.h, the
128 x 64 tile form of csrc/conv3x3_wgrad.hip, functional.conv3x3_narrow_wgrad): the entries through the C ABI, the autograd op
with ``narrow_wgrad=True`` and one training step with the switches on.

It follows tests/test_conv3x3_wgrad_gpu.py.  Entry level: x, g, dw and the workspace of every case sit in the guard-band arena of
tests/bounds_cases.py, the workspace at exactly plan[2] bytes and pre-filled with 0xFF; every case is called twice on the same
buffers and must give the same bits, with the guards intact.  Integer cases (x in [-7, 7], g in [-3, 3], 21 P < 2^24: every
partial sum is an exact fp32 integer in any order) must meet float64 autograd of ``F.conv2d`` on the CPU bit for bit, for every
slice count.  A shape the wide form takes as well must come out with the wide form's bits for the same slice count.
Realistic data: error figure max |got - want| / max |want| against the same float64 autograd; bound of a case
min(RATIO x the parent's figure, CAP) with RATIO = 4 and CAP = 2e-5 of tests/test_conv3x3_split_gpu.py.  The parent's figure is
MIOpen's weight gradient (``aten.convolution_backward``, mask (False, True, False)) on exactly these inputs:
PARENT_NARROW_WGRAD_ERR, measured once on an MI355X by tools/conv3x3_narrow_wgrad_parent_err.py and tabulated beside the
kernel's own figures in profiles/r23_conv3x3_narrow_wgrad_accuracy.md.
"""
import ctypes
import zlib

import pytest
import torch
import torch.nn.functional as F

import bounds_cases as BC
from structure_knowledge_distillation_amd import _lib, functional as SF
from test_conv3x3_split_gpu import CAP, DEV, RATIO, P, rel_err
from test_conv3x3_wgrad_gpu import INT_SHAPES, LAYOUTS, _dw_view, cl, wgrad64
from test_conv3x3_wgrad_gpu import run_entry as run_wide

pytestmark = pytest.mark.gpu

PLAN, RUN = "skd_conv3x3_narrow_wgrad_plan", "skd_conv3x3_narrow_wgrad_nhwc"


@pytest.fixture(scope="module")
def hip():
    return _lib.load()


def plan_of(hip, x, g, slices):
    """(slices used, K-tiles per slice, workspace bytes); slices = 0: the automatic choice for THIS device."""
    b, cin, h, w = x.shape
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    plan = (ctypes.c_int64 * 3)()
    assert getattr(hip, PLAN)(b, h, w, cin, g.shape[1], slices, cus, ctypes.cast(plan, ctypes.c_void_p)) == 1
    return int(plan[0]), int(plan[1]), int(plan[2])


def run_entry(hip, x, g, d, slices=0, layout="channels_last"):
    """dw (Cout, Cin, 3, 3) on the CPU from the two launches of skd_conv3x3_narrow_wgrad_nhwc, called twice on the same guarded
    buffers (the workspace left as the first call left it): same bits, guards intact, nothing written outside a slice."""
    b, cin, h, w = x.shape
    cout = g.shape[1]
    used, per_slice, nbytes = plan_of(hip, x, g, slices)
    assert nbytes == used * 9 * cin * cout * 4 and nbytes % 4 == 0
    A = BC.Arena(DEV)
    xa = A.inp("x", x.permute(0, 2, 3, 1).contiguous())
    ga = A.inp("g", g.permute(0, 2, 3, 1).contiguous())
    dw, full = _dw_view(A, cout, cin, layout)
    ws = A.ws("workspace", nbytes // 4)
    assert bool((ws.view(torch.uint8) == BC.FILL).all())
    results = []
    for k in range(2):
        if k:
            A.reset()
        assert getattr(hip, RUN)(b, h, w, cin, cout, d, P(xa), P(ga), P(dw), *dw.stride(), P(ws), nbytes, used, None) == 1
        A.check()
        results.append(dw.detach().cpu().clone())
        if full is not dw:
            assert bool((full[:, :64].contiguous().view(torch.uint8) == BC.FILL).all()), "columns outside the slice were written"
    assert BC.same_bits(results[0], results[1]), "two calls on the same buffers differ"
    return results[0]


# ---- 1. integers are exact ------------------------------------------------------------------------------------------------------

# unit counts 9 and 27 are odd (a dead half-tile), 18 is even; Cout of 128 and 192: two and three column tiles
INT_CHANNELS = [(64, 64), (64, 128), (128, 64), (192, 64), (64, 192)]
_INT = {}


def int_case(shape, chans):
    """(x, g, float64 truth) of an integer case, made once and shared (never modified)."""
    key = (shape, chans)
    if key not in _INT:
        b, h, w, d = shape
        cin, cout = chans
        assert 21 * b * h * w < 2 ** 24
        gen = torch.Generator().manual_seed(1000 * h + 10 * d + cin // 64 + 5 * (cout // 64))
        x = cl(torch.randint(-7, 8, (b, cin, h, w), generator=gen).float())
        g = cl(torch.randint(-3, 4, (b, cout, h, w), generator=gen).float())
        _INT[key] = (x, g, wgrad64(x, g, d))
    return _INT[key]


@pytest.mark.parametrize("chans", INT_CHANNELS, ids=lambda c: "%dto%d" % c)
@pytest.mark.parametrize("shape", INT_SHAPES, ids=lambda s: "b%d-%dx%d-d%d" % s)
def test_integer_weight_gradient_bit_exact(hip, shape, chans):
    b, h, w, d = shape
    x, g, want = int_case(shape, chans)
    nk = -(-b * h * w // 16)
    assert float(want.abs().max()) > 20.0
    seen = {}
    for slices in (1, 2, 3, nk, 0):
        used = plan_of(hip, x, g, slices)[0]
        if used in seen:
            continue
        got = seen[used] = run_entry(hip, x, g, d, slices)
        assert torch.equal(got.double(), want), "slices %d (%d used): %d of %d gradients differ" % (
            slices, used, int((got.double() != want).sum()), got.numel())
    first = next(iter(seen.values()))
    assert all(BC.same_bits(first, v) for v in seen.values()), "slice counts give different bits on integers"
    assert (1 in seen) and (nk in seen or nk == 1)
    if shape == (1, 3, 3, 4):
        # only the centre tap lives: for Cin = 64 the tiles of taps (0, 1), (2, 3), (6, 7) are dead in both halves, (4, 5) in one
        dead = torch.ones(3, 3, dtype=torch.bool)
        dead[1, 1] = False
        assert bool((first[:, :, dead] == 0).all()) and float(first[:, :, 1, 1].abs().max()) > 0


@pytest.mark.parametrize("chans", [(128, 128), (128, 256)], ids=lambda c: "%dto%d" % c)
def test_bits_of_the_wide_kernel(hip, chans):
    """A shape both forms take, on realistic (non-integer) data, through both entries with the same explicit slice count: every
    element sees the same operations in the same order, so the results are equal bit for bit."""
    b, h, w, d = 2, 13, 11, 2
    cin, cout = chans
    gen = torch.Generator().manual_seed(230 + cout)
    x = cl(torch.relu(torch.randn(b, cin, h, w, generator=gen) + torch.randn(1, cin, 1, 1, generator=gen) * 0.5))
    g = cl(torch.randn(b, cout, h, w, generator=gen))
    nk = -(-b * h * w // 16)
    for slices in (1, 3, nk):
        wide, narrow = run_wide(hip, x, g, d, slices), run_entry(hip, x, g, d, slices)
        assert float(wide.abs().max()) > 1.0
        assert torch.equal(narrow, wide), "slices %d: %d of %d elements differ from the wide kernel's, max %.3e" % (
            slices, int((narrow != wide).sum()), wide.numel(), float((narrow - wide).abs().max()))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_destination_layouts(hip, layout):
    shape, chans = (2, 13, 11, 2), (64, 64)
    x, g, want = int_case(shape, chans)
    got = run_entry(hip, x, g, 2, 3, layout)
    assert torch.equal(got.double(), want), layout


def test_refusals_leave_the_buffers_alone(hip):
    x, g, _ = int_case((1, 5, 7, 1), (64, 64))
    used, _, nbytes = plan_of(hip, x, g, 2)
    A = BC.Arena(DEV)
    xa, ga = A.inp("x", x.permute(0, 2, 3, 1).contiguous()), A.inp("g", g.permute(0, 2, 3, 1).contiguous())
    dw, ws = A.out("dw", (64, 3, 3, 64)).permute(0, 3, 1, 2), A.ws("workspace", nbytes // 4)
    f = getattr(hip, RUN)
    st = dw.stride()
    assert not f(1, 5, 7, 64, 64, 1, None, P(ga), P(dw), *st, P(ws), nbytes, used, None)
    assert not f(1, 5, 7, 64, 64, 1, P(xa), None, P(dw), *st, P(ws), nbytes, used, None)
    assert not f(1, 5, 7, 64, 64, 1, P(xa), P(ga), P(dw), *st, P(ws), nbytes - 1, used, None)
    assert not f(1, 5, 7, 64, 64, 1, P(xa), P(ga), P(dw), *st, P(ws), nbytes, 0, None)
    assert not f(1, 5, 7, 64, 64, 1, P(xa), P(ga), P(dw), *st, P(ws), nbytes, 4, None)       # nk = 3
    assert not f(1, 5, 7, 64, 64, 0, P(xa), P(ga), P(dw), *st, P(ws), nbytes, used, None)
    assert not f(1, 5, 7, 64, 32, 1, P(xa), P(ga), P(dw), *st, P(ws), nbytes, used, None)
    assert not f(1, 5, 7, 96, 64, 1, P(xa), P(ga), P(dw), *st, P(ws), nbytes, used, None)
    assert not f(1, 5, 7, 64, 64, 1, P(xa), P(ga), P(dw), -576, 1, 192, 64, P(ws), nbytes, used, None)
    A.check()
    assert bool((dw.contiguous().view(torch.uint8) == BC.FILL).all()) and bool((ws.view(torch.uint8) == BC.FILL).all())


# ---- 2. adjointness on integers -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [1, 2, 4])
def test_weight_gradient_and_forward_are_adjoint_on_integers(hip, d):
    """sum dW . V == sum g . conv(x, V), exactly, for a random integer V: pins the orientation of the taps (and which operand
    is shifted) without torch's backward.  Cin != Cout, so a forgotten transposition cannot pass."""
    b, cin, cout, h, w = 2, 64, 128, 13, 11
    gen = torch.Generator().manual_seed(277 + d)
    x = cl(torch.randint(-7, 8, (b, cin, h, w), generator=gen).float())
    g = cl(torch.randint(-3, 4, (b, cout, h, w), generator=gen).float())
    v = torch.randint(-3, 4, (cout, cin, 3, 3), generator=gen).double()
    assert 21 * b * h * w < 2 ** 24
    dw = run_entry(hip, x, g, d, 0)
    lhs = float((dw.double() * v).sum())
    rhs = float((g.double() * F.conv2d(x.double(), v, None, 1, d, d)).sum())
    assert lhs == rhs and abs(lhs) > 1000.0, (lhs, rhs)


# ---- 3. against float64 on realistic data ----------------------------------------------------------------------------------------

# (name, B, Cin, Cout, H, W, dilation, slices)
REAL_CASES = [
    ("narrow-wgrad-ragged-64-64-13x11-d1", 2, 64, 64, 13, 11, 1, 0),
    ("narrow-wgrad-ragged-128-64-13x11-d1", 2, 128, 64, 13, 11, 1, 0),
    ("narrow-wgrad-step-length-64-64-129x129-d1", 8, 64, 64, 129, 129, 1, 0),
]
REAL = {c[0]: c for c in REAL_CASES}

# max |parent - want| / max |want| of MIOpen's fp32 weight gradient on exactly these inputs, measured once on an MI355X
# (profiles/r23_conv3x3_narrow_wgrad_accuracy.md; tools/conv3x3_narrow_wgrad_parent_err.py measures them again)
PARENT_NARROW_WGRAD_ERR = {
    "narrow-wgrad-ragged-64-64-13x11-d1": 2.910e-07,
    "narrow-wgrad-ragged-128-64-13x11-d1": 1.413e-07,
    "narrow-wgrad-step-length-64-64-129x129-d1": 6.730e-07,
}


def real_inputs(name, case=None):
    """Seeded post-ReLU activations with a per-channel offset and a normal output gradient, channels-last."""
    _, b, cin, cout, h, w, _, _ = case or REAL[name]
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    x = torch.relu(torch.randn(b, cin, h, w, generator=gen) + torch.randn(1, cin, 1, 1, generator=gen) * 0.5)
    g = torch.randn(b, cout, h, w, generator=gen)
    return cl(x), cl(g)


_WANT = {}


def want_of(name):
    """float64 truth of a case, computed once and shared (never modified)."""
    if name not in _WANT:
        x, g = real_inputs(name)
        _WANT[name] = wgrad64(x, g, REAL[name][6])
    return _WANT[name]


@pytest.mark.parametrize("name", [c[0] for c in REAL_CASES])
def test_weight_gradient_vs_float64(hip, name):
    x, g = real_inputs(name)
    got = run_entry(hip, x, g, REAL[name][6], REAL[name][7])
    err = rel_err(got, want_of(name))
    bound = min(RATIO * PARENT_NARROW_WGRAD_ERR[name], CAP)
    print("%s: err %.3e  parent %.3e  bound %.3e" % (name, err, PARENT_NARROW_WGRAD_ERR[name], bound))
    assert err <= bound, "%s: max err %.3e > %.3e (parent path: %.3e)" % (name, err, bound, PARENT_NARROW_WGRAD_ERR[name])


# ---- 4. the op ------------------------------------------------------------------------------------------------------------------

def _op_case(cin, cout, bias):
    gen = torch.Generator().manual_seed(5432 + cin + 2 * cout + int(bias))
    b, h, w, d = 2, 13, 11, 2
    x = torch.relu(torch.randn(b, cin, h, w, generator=gen) + torch.randn(1, cin, 1, 1, generator=gen) * 0.5)
    wt = torch.randn(cout, cin, 3, 3, generator=gen) * (2.0 / (9 * cin)) ** 0.5
    bs = torch.randn(cout, generator=gen) * 0.2 if bias else None
    go = torch.randn(b, cout, h, w, generator=gen)
    return cl(x), cl(wt), bs, cl(go), d


@pytest.mark.parametrize("cin,cout,bias", [(64, 64, False), (64, 128, True), (128, 64, False)])
def test_op_with_the_narrow_weight_gradient_on_the_core(hip, cin, cout, bias, monkeypatch):
    x, wt, bs, go, d = _op_case(cin, cout, bias)
    entry = run_entry(hip, x, go, d, 0)                       # the automatic plan of this device, as the op asks for it
    xd, wd, god = x.to(DEV), wt.to(DEV), go.to(DEV)
    calls, wide_calls = [], []
    real, real_wide = SF.conv3x3_narrow_wgrad, SF.conv3x3_split_wgrad
    monkeypatch.setattr(SF, "conv3x3_narrow_wgrad", lambda *a, **k: calls.append(1) or real(*a, **k))
    monkeypatch.setattr(SF, "conv3x3_split_wgrad", lambda *a, **k: wide_calls.append(1) or real_wide(*a, **k))

    def grads(extra, need_x=True, need_w=True):
        owner = torch.nn.Module()
        xg = xd.clone().requires_grad_(need_x)
        wg = cl(wd.clone()).requires_grad_(need_w)
        bg = None if bs is None else bs.to(DEV).requires_grad_(need_w)
        y = SF.conv3x3_split_train(xg, wg, d, bg, owner, narrow=True, **extra)
        ins = [t for t in (xg, wg, bg) if t is not None and t.requires_grad]
        return y.detach(), dict(zip([n for n, t in (("dx", xg), ("dw", wg), ("db", bg)) if t is not None and t.requires_grad],
                                    torch.autograd.grad(y, ins, god)))
    assert SF.conv3x3_narrow_wgrad_supported(xd.clone().requires_grad_(True), wd, 1, d, d, 1)
    y0, off = grads({})
    grads(dict(wgrad=True))                                   # ``wgrad`` keeps being ignored for a narrow shape
    assert calls == [] and wide_calls == []                   # (the library's dw is not the same bits from run to run: not compared)
    y1, on = grads(dict(narrow_wgrad=True))
    assert len(calls) == 1 and wide_calls == []
    assert torch.equal(y1, y0) and torch.equal(on["dx"], off["dx"]), "forward and dx keep the bits of narrow_wgrad=False"
    assert on["dw"].shape == wd.shape and on["dw"].is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(on["dw"].cpu(), entry), "dw is the entry-level result, bit for bit"
    if bias:
        _, _, db = torch.ops.aten.convolution_backward(god, xd, wd, [wd.shape[0]], [1, 1], [d, d], [d, d], False, [0, 0], 1,
                                                       (False, False, True))
        assert torch.equal(on["db"], db) and torch.equal(on["db"], off["db"]), "dbias is aten's"
    # needs_input_grad: only dx asked -> no weight-gradient launch; only dw asked -> one, the same bits
    _, only_x = grads(dict(narrow_wgrad=True), need_w=False)
    assert len(calls) == 1 and torch.equal(only_x["dx"], off["dx"])
    _, only_w = grads(dict(narrow_wgrad=True), need_x=False)
    assert len(calls) == 2 and torch.equal(only_w["dw"], on["dw"])
    # a weight written between forward and backward still raises autograd's version error
    xg, wg = xd.clone().requires_grad_(True), cl(wd.clone()).requires_grad_(True)
    y = SF.conv3x3_split_train(xg, wg, d, None, torch.nn.Module(), narrow=True, narrow_wgrad=True)
    with torch.no_grad():
        wg.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        torch.autograd.grad(y, (xg, wg), god)
    assert len(calls) == 2


# ---- 5. the step ----------------------------------------------------------------------------------------------------------------

NARROW_STEP = [(64, 64, 1), (64, 128, 1), (128, 64, 1), (64, 64, 1), (64, 64, 1), (64, 64, 1)]


@pytest.mark.parametrize("wide", ["0", "1"], ids=["narrow-wgrad", "narrow-and-wide-wgrad"])
def test_step_config1_with_the_narrow_weight_gradients_on_the_core(monkeypatch, wide):
    """The config-1 step of tests/test_step_gpu.py with ``split_train``, ``split_narrow`` and ``split_narrow_wgrad`` on, with and
    without ``split_wgrad``, at exactly the bounds of test_step_config1_vs_reference_golden: that test's own body runs, with the
    switches set where its ``default_args`` reads them.  A counting shim sees six narrow weight-gradient calls.  The routing
    policy (NARROW_WGRAD_ROUTING_EXCLUDED: the shapes that measure behind the library) is emptied for the test: it is the routed
    path that is checked here, whatever the policy leaves routed."""
    import structure_knowledge_distillation_amd.networks.pspnet_combine as PC
    import test_step_gpu as TS
    monkeypatch.setattr(PC, "NARROW_WGRAD_ROUTING_EXCLUDED", frozenset())
    from test_conv3x3_train_cpu import ROUTED
    real, real_wide = SF.conv3x3_narrow_wgrad, SF.conv3x3_split_wgrad
    seen, seen_wide = [], []

    def shim(x, g, weight_like, dilation, *a, **k):
        seen.append((int(x.shape[1]), int(g.shape[1]), int(dilation)))
        return real(x, g, weight_like, dilation, *a, **k)

    def shim_wide(x, g, weight_like, dilation, *a, **k):
        seen_wide.append((int(x.shape[1]), int(g.shape[1]), int(dilation)))
        return real_wide(x, g, weight_like, dilation, *a, **k)
    monkeypatch.setattr(SF, "conv3x3_narrow_wgrad", shim)
    monkeypatch.setattr(SF, "conv3x3_split_wgrad", shim_wide)
    monkeypatch.setenv("SKD_SPLIT_TRAIN", "1")
    monkeypatch.setenv("SKD_SPLIT_NARROW", "1")
    monkeypatch.setenv("SKD_SPLIT_NARROW_WGRAD", "1")
    monkeypatch.setenv("SKD_SPLIT_WGRAD", wide)
    TS.test_step_config1_vs_reference_golden()
    assert len(seen) == 6 and sorted(seen) == sorted(NARROW_STEP), seen
    assert sorted(seen_wide) == (sorted(ROUTED) if wide == "1" else []), seen_wide
