"""-m gpu: the weight gradient of the student's 3x3 convolutions on the split core (include/skd_wgrad.h, csrc/conv3x3_wgrad.hip,
functional.conv3x3_split_wgrad): the entries through the C ABI, the autograd op with ``wgrad=True`` and one training step with
both switches on.

Entry level: x, g, dw and the workspace of every case sit in the guard-band arena of tests/bounds_cases.py, the workspace at
exactly plan[2] bytes and pre-filled with 0xFF (it is never assumed initialised); every case is called twice on the same buffers
and must give the same bits, with the guards intact.  Integer cases (x in [-7, 7], g in [-3, 3], 21 P < 2^24: every partial sum
is an exact fp32 integer in any order) must meet float64 autograd of ``F.conv2d`` on the CPU bit for bit, for every slice count.
Realistic data: error figure max |got - want| / max |want| against the same float64 autograd; bound of a case
min(RATIO x the parent's figure, CAP) with RATIO = 4 and CAP = 2e-5 of tests/test_conv3x3_split_gpu.py -- the rule the forward
and the data gradient were accepted under.  The parent's figure is MIOpen's weight gradient (``aten.convolution_backward``, mask
(False, True, False)) on exactly these inputs: PARENT_WGRAD_ERR, measured once on an MI355X by
tools/conv3x3_wgrad_parent_err.py and tabulated beside the kernel's own figures in profiles/r20_conv3x3_wgrad_accuracy.md.
"""
import ctypes
import zlib

import pytest
import torch
import torch.nn.functional as F

import bounds_cases as BC
from structure_knowledge_distillation_amd import _lib, functional as SF
from test_conv3x3_split_gpu import CAP, DEV, RATIO, P, rel_err
from test_conv3x3_train_cpu import ROUTED

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    return _lib.load()


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def wgrad64(x, g, d):
    """Autograd of F.conv2d in float64 on the CPU: the gradient of a (Cout, Cin, 3, 3) weight for the output gradient ``g``."""
    wt = torch.zeros(g.shape[1], x.shape[1], 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), wt, None, 1, d, d).backward(g.double())
    return wt.grad


def plan_of(hip, x, g, slices):
    """(slices used, K-tiles per slice, workspace bytes); slices = 0: the automatic choice for THIS device."""
    b, cin, h, w = x.shape
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    plan = (ctypes.c_int64 * 3)()
    assert hip.skd_conv3x3_split_wgrad_plan(b, h, w, cin, g.shape[1], slices, cus, ctypes.cast(plan, ctypes.c_void_p)) == 1
    return int(plan[0]), int(plan[1]), int(plan[2])


LAYOUTS = ("contiguous", "channels_last", "slice", "slice_channels_last")


def _dw_view(A, cout, cin, layout):
    """(the (Cout, Cin, 3, 3) destination, the whole buffer) in the arena: contiguous, channels-last, or the slice [:, 64:] of a
    weight 64 channels wider (contiguous / channels-last)."""
    if layout == "contiguous":
        full = A.out("dw", (cout, cin, 3, 3))
        return full, full
    if layout == "channels_last":
        full = A.out("dw", (cout, 3, 3, cin)).permute(0, 3, 1, 2)
        return full, full
    if layout == "slice":
        full = A.out("dw", (cout, cin + 64, 3, 3))
    else:
        full = A.out("dw", (cout, 3, 3, cin + 64)).permute(0, 3, 1, 2)
    return full[:, 64:], full


def run_entry(hip, x, g, d, slices=0, layout="channels_last"):
    """dw (Cout, Cin, 3, 3) on the CPU from the two launches of skd_conv3x3_split_wgrad_nhwc, called twice on the same guarded
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
        assert hip.skd_conv3x3_split_wgrad_nhwc(b, h, w, cin, cout, d, P(xa), P(ga), P(dw), *dw.stride(), P(ws), nbytes, used, None) == 1
        A.check()
        results.append(dw.detach().cpu().clone())
        if full is not dw:
            assert bool((full[:, :64].contiguous().view(torch.uint8) == BC.FILL).all()), "columns outside the slice were written"
    assert BC.same_bits(results[0], results[1]), "two calls on the same buffers differ"
    return results[0]


# ---- 1. integers are exact ------------------------------------------------------------------------------------------------------

# P not a multiple of 16, W not a multiple of 4, pixel quads across row and image ends; 3 x 3 at d = 4: only the centre tap lives
INT_SHAPES = [(1, 5, 7, 1), (2, 13, 11, 1), (2, 13, 11, 2), (2, 13, 11, 4), (1, 3, 3, 4)]
INT_CHANNELS = [(128, 128), (128, 256), (256, 128)]
_INT = {}


def int_case(shape, chans):
    """(x, g, float64 truth) of an integer case, made once and shared (never modified)."""
    key = (shape, chans)
    if key not in _INT:
        b, h, w, d = shape
        cin, cout = chans
        assert 21 * b * h * w < 2 ** 24
        gen = torch.Generator().manual_seed(1000 * h + 10 * d + cin // 128 + 3 * (cout // 128))
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
        dead = torch.ones(3, 3, dtype=torch.bool)
        dead[1, 1] = False
        assert bool((first[:, :, dead] == 0).all()) and float(first[:, :, 1, 1].abs().max()) > 0


@pytest.mark.parametrize("layout", LAYOUTS)
def test_destination_layouts(hip, layout):
    shape, chans = (2, 13, 11, 2), (128, 128)
    x, g, want = int_case(shape, chans)
    got = run_entry(hip, x, g, 2, 3, layout)
    assert torch.equal(got.double(), want), layout


def test_refusals_leave_the_buffers_alone(hip):
    x, g, _ = int_case((1, 5, 7, 1), (128, 128))
    used, _, nbytes = plan_of(hip, x, g, 2)
    A = BC.Arena(DEV)
    xa, ga = A.inp("x", x.permute(0, 2, 3, 1).contiguous()), A.inp("g", g.permute(0, 2, 3, 1).contiguous())
    dw, ws = A.out("dw", (128, 3, 3, 128)).permute(0, 3, 1, 2), A.ws("workspace", nbytes // 4)
    f = hip.skd_conv3x3_split_wgrad_nhwc
    st = dw.stride()
    assert not f(1, 5, 7, 128, 128, 1, None, P(ga), P(dw), *st, P(ws), nbytes, used, None)
    assert not f(1, 5, 7, 128, 128, 1, P(xa), P(ga), P(dw), *st, P(ws), nbytes - 1, used, None)
    assert not f(1, 5, 7, 128, 128, 1, P(xa), P(ga), P(dw), *st, P(ws), nbytes, 0, None)
    assert not f(1, 5, 7, 128, 128, 1, P(xa), P(ga), P(dw), *st, P(ws), nbytes, 4, None)       # nk = 3
    assert not f(1, 5, 7, 128, 128, 0, P(xa), P(ga), P(dw), *st, P(ws), nbytes, used, None)
    assert not f(1, 5, 7, 128, 64, 1, P(xa), P(ga), P(dw), *st, P(ws), nbytes, used, None)
    assert not f(1, 5, 7, 128, 128, 1, P(xa), P(ga), P(dw), -1152, 1, 384, 128, P(ws), nbytes, used, None)
    A.check()
    assert bool((dw.contiguous().view(torch.uint8) == BC.FILL).all()) and bool((ws.view(torch.uint8) == BC.FILL).all())


# ---- 2. adjointness on integers -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [1, 2, 4])
def test_weight_gradient_and_forward_are_adjoint_on_integers(hip, d):
    """sum dW . V == sum g . conv(x, V), exactly, for a random integer V: pins the orientation of the taps (and which operand
    is shifted) without torch's backward.  Cin != Cout, so a forgotten transposition cannot pass."""
    b, cin, cout, h, w = 2, 128, 256, 13, 11
    gen = torch.Generator().manual_seed(177 + d)
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
    ("wgrad-ragged-128-128-13x11-d2", 2, 128, 128, 13, 11, 2, 0),
    ("wgrad-ragged-128-256-13x11-d1", 2, 128, 256, 13, 11, 1, 0),
    ("wgrad-512-256-9x9-d4", 1, 512, 256, 9, 9, 4, 0),
    ("wgrad-step-length-128-128-65x65-d1", 8, 128, 128, 65, 65, 1, 0),
]
REAL = {c[0]: c for c in REAL_CASES}

# max |parent - want| / max |want| of MIOpen's fp32 weight gradient on exactly these inputs, measured once on an MI355X
# (profiles/r20_conv3x3_wgrad_accuracy.md; tools/conv3x3_wgrad_parent_err.py measures them again)
PARENT_WGRAD_ERR = {
    "wgrad-ragged-128-128-13x11-d2": 1.836e-07,
    "wgrad-ragged-128-256-13x11-d1": 1.900e-07,
    "wgrad-512-256-9x9-d4": 1.386e-07,
    "wgrad-step-length-128-128-65x65-d1": 4.336e-07,
}


def real_inputs(name):
    """Seeded post-ReLU activations with a per-channel offset and a normal output gradient, channels-last."""
    _, b, cin, cout, h, w, _, _ = REAL[name]
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
    bound = min(RATIO * PARENT_WGRAD_ERR[name], CAP)
    print("%s: err %.3e  parent %.3e  bound %.3e" % (name, err, PARENT_WGRAD_ERR[name], bound))
    assert err <= bound, "%s: max err %.3e > %.3e (parent path: %.3e)" % (name, err, bound, PARENT_WGRAD_ERR[name])


# ---- 4. the op ------------------------------------------------------------------------------------------------------------------

def _op_case(bias):
    gen = torch.Generator().manual_seed(4321 + int(bias))
    b, cin, cout, h, w, d = 2, 128, 256, 13, 11, 2
    x = torch.relu(torch.randn(b, cin, h, w, generator=gen) + torch.randn(1, cin, 1, 1, generator=gen) * 0.5)
    wt = torch.randn(cout, cin, 3, 3, generator=gen) * (2.0 / (9 * cin)) ** 0.5
    bs = torch.randn(cout, generator=gen) * 0.2 if bias else None
    go = torch.randn(b, cout, h, w, generator=gen)
    return cl(x), cl(wt), bs, cl(go), d


@pytest.mark.parametrize("bias", [False, True], ids=["no-bias", "bias"])
def test_op_with_the_weight_gradient_on_the_core(hip, bias, monkeypatch):
    x, wt, bs, go, d = _op_case(bias)
    entry = run_entry(hip, x, go, d, 0)                       # the automatic plan of this device, as the op asks for it
    xd, wd, god = x.to(DEV), wt.to(DEV), go.to(DEV)
    calls = []
    real = SF.conv3x3_split_wgrad
    monkeypatch.setattr(SF, "conv3x3_split_wgrad", lambda *a, **k: calls.append(1) or real(*a, **k))

    def grads(flag, need_x=True, need_w=True):
        owner = torch.nn.Module()
        xg = xd.clone().requires_grad_(need_x)
        wg = cl(wd.clone()).requires_grad_(need_w)
        bg = None if bs is None else bs.to(DEV).requires_grad_(need_w)
        extra = dict(wgrad=True) if flag else {}
        y = SF.conv3x3_split_train(xg, wg, d, bg, owner, **extra)
        ins = [t for t in (xg, wg, bg) if t is not None and t.requires_grad]
        return y.detach(), dict(zip([n for n, t in (("dx", xg), ("dw", wg), ("db", bg)) if t is not None and t.requires_grad],
                                    torch.autograd.grad(y, ins, god)))
    assert SF.conv3x3_wgrad_supported(xd.clone().requires_grad_(True), wd, 1, d, d, 1)
    y0, off = grads(False)
    assert calls == []
    y1, on = grads(True)
    assert len(calls) == 1
    assert torch.equal(y1, y0) and torch.equal(on["dx"], off["dx"]), "forward and dx keep the bits of wgrad=False"
    assert on["dw"].shape == wd.shape and on["dw"].is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(on["dw"].cpu(), entry), "dw is the entry-level result, bit for bit"
    if bias:
        _, _, db = torch.ops.aten.convolution_backward(god, xd, wd, [wd.shape[0]], [1, 1], [d, d], [d, d], False, [0, 0], 1,
                                                       (False, False, True))
        assert torch.equal(on["db"], db) and torch.equal(on["db"], off["db"]), "dbias is aten's"
    # needs_input_grad: only dx asked -> no weight-gradient launch; only dw asked -> one, the same bits
    _, only_x = grads(True, need_w=False)
    assert len(calls) == 1 and torch.equal(only_x["dx"], off["dx"])
    _, only_w = grads(True, need_x=False)
    assert len(calls) == 2 and torch.equal(only_w["dw"], on["dw"])
    # a weight written between forward and backward still raises autograd's version error
    xg, wg = xd.clone().requires_grad_(True), cl(wd.clone()).requires_grad_(True)
    y = SF.conv3x3_split_train(xg, wg, d, None, torch.nn.Module(), wgrad=True)
    with torch.no_grad():
        wg.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        torch.autograd.grad(y, (xg, wg), god)
    assert len(calls) == 2


def test_op_slice_of_a_wider_weight(hip):
    """The PSP half: the weight is the channel slice of a wider one; its gradient reaches the full weight through autograd."""
    x, wt, _, go, d = _op_case(False)
    entry = run_entry(hip, x, go, d, 0)
    wide = cl(torch.cat([torch.zeros(wt.shape[0], 64, 3, 3), wt], 1).to(DEV)).requires_grad_(True)
    y = SF.conv3x3_split_train(x.to(DEV), wide[:, 64:], d, None, {}, wgrad=True)
    (dwide,) = torch.autograd.grad(y, wide, go.to(DEV))
    assert torch.equal(dwide[:, 64:].cpu(), entry) and bool((dwide[:, :64] == 0).all())


# ---- 5. the step ----------------------------------------------------------------------------------------------------------------

def test_step_config1_with_the_weight_gradients_on_the_core(monkeypatch):
    """The config-1 step of tests/test_step_gpu.py with ``split_train`` and ``split_wgrad`` on, at exactly the bounds of
    test_step_config1_vs_reference_golden: that test's own body runs, with the switches set where its ``default_args`` reads
    them.  A counting shim sees 13 weight-gradient calls; with SKD_SPLIT_WGRAD=0, none."""
    import test_step_gpu as TS
    real = SF.conv3x3_split_wgrad
    seen = []

    def shim(x, g, weight_like, dilation, *a, **k):
        seen.append((int(x.shape[1]), int(g.shape[1]), int(dilation)))
        return real(x, g, weight_like, dilation, *a, **k)
    monkeypatch.setattr(SF, "conv3x3_split_wgrad", shim)

    monkeypatch.setenv("SKD_SPLIT_TRAIN", "1")
    monkeypatch.setenv("SKD_SPLIT_WGRAD", "0")
    model, _, _ = TS._config1_step(pa=True)
    assert model.split_train and not model.split_wgrad and seen == []
    del model

    monkeypatch.setenv("SKD_SPLIT_WGRAD", "1")
    TS.test_step_config1_vs_reference_golden()
    assert len(seen) == 13 and sorted(seen) == sorted(ROUTED), seen
