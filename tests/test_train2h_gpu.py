"""-m gpu: the student's wide 3x3 training convolutions on two FP16 pieces with a device-side gradient scale
(include/skd_train2h.h): the scale word, the fp16 pack pair, the scaled data gradient, the fp16 weight gradient, the autograd op
conv3x3_split_train_fp16 and one training step with ``student_pieces=2, student_piece_format="fp16"``.  On the HIP back-end a
missing entry is a failure of these tests, never a skip.

Every entry-level call hands its inputs, outputs and workspaces out of the guard-band arena of tests/bounds_cases.py (0xFF on both
sides, checked after each call); the workspaces have exactly the queried size, start as 0xFF and each workspace entry is called
twice: the same bits, no guard byte changed.

Shapes (tests/train2h_ref.py): (Cin, Cout) = (128, 256) and (256, 128), B = 2, 9 x 11 (198 rows: one 128-row panel, 64-row panels
and a ragged last one; no multiple of 16), dilations 1, 2, 4, the weight gradient with 1 and 3 slices.  The integer cases are proven
in tests/test_train2h_cpu.py.  Float data, per output element of either gradient product against float64 (the header's bound):
    |out - out64| <= 2^-21 sum |a| |b| + 2^-49 amax(g) sum |b| + e3
with e3 the three-piece twin's largest elementwise error on the same inputs, measured in the same test.

Accuracy note (MI355X, the shapes above, Gaussian g 1e-6, post-ReLU-like x, He-scaled w; largest error relative to the largest
|y64|, the fp16 entry against its three-piece twin; asserted <= 2 x): see profiles/r35_student_fp16_accuracy.md.
"""
import ctypes

import pytest
import torch

import bounds_cases as BC
import split_exact as SE
import train2h_ref as T
from bounds_cases import P
from structure_knowledge_distillation_amd import _lib, functional as SF

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = list(_lib.ABI.get("skd_train2h.h", {"skd_fp16_scale_word": None}))
MARGIN = 2.0            # an fp16 entry's largest error against its three-piece twin's (tests/test_split2h_gpu.py, test_infer2h_gpu.py)


@pytest.fixture(scope="module")
def hip():
    lib = _lib.load()
    for name in NAMES + ["skd_conv3x3_split2h_nhwc", "skd_conv3x3_split2h_pack_weights", "skd_conv3x3_split2h_pack_bytes"]:
        getattr(lib, name)          # a missing entry fails here
    assert len(NAMES) == 6
    return lib


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ---- the entries, each call between guards ------------------------------------------------------------------------------------

def scale_word(hip, A, g_dev, n=None):
    """The device word (a guarded one-element int32 tensor) of the dense device tensor ``g_dev``: the workspace has exactly the
    queried size and starts as 0xFF; called twice, the same word."""
    n = int(g_dev.numel()) if n is None else n
    nbytes = int(hip.skd_fp16_scale_word_workspace_bytes(n))
    assert nbytes >= 4 and nbytes % 4 == 0
    ws = A.ws("word_ws", nbytes // 4)
    word = A.out("word", (1,), torch.int32)
    seen = []
    for _ in range(2):
        assert hip.skd_fp16_scale_word(n, P(g_dev), P(ws), nbytes, P(word), None) == 1
        A.check()
        seen.append(int(word.cpu()[0]) & 0xFFFFFFFF)
    assert seen[0] == seen[1], "two calls give two words"
    return word, seen[0]


def pack_pair(hip, A, w, fmt="fp16", fwd=True, bwd=True):
    """(pack_fwd, pack_bwd) of the weight view ``w`` on the device (any strides), as guarded byte buffers; None where not asked."""
    cout, cin = int(w.shape[0]), int(w.shape[1])
    size = hip.skd_conv3x3_split2h_pack_bytes if fmt == "fp16" else hip.skd_conv3x3_split_pack_bytes
    entry = hip.skd_conv3x3_split2h_pack_pair if fmt == "fp16" else hip.skd_conv3x3_split_pack_pair
    nf, nb = int(size(cin, cout)), int(size(cout, cin))
    assert nf == nb == (4 if fmt == "fp16" else 6) * 9 * cin * cout
    pf = A.out("pack_fwd", (nf,), torch.uint8, row=4096) if fwd else None
    pb = A.out("pack_bwd", (nb,), torch.uint8, row=4096) if bwd else None
    assert entry(cin, cout, P(w), *w.stride(), P(pf), nf if fwd else 0, P(pb), nb if bwd else 0, None) == 1
    A.check()
    return pf, pb


def conv(hip, x, w, d, mode, backward=False, word_value=None, geometry=0):
    """conv3x3 of the channels-last CPU map ``x`` with the CPU weight ``w`` (Cout, Cin, 3, 3) -- ``backward``: with its flipped,
    transposed image, the data gradient of a g = x -- through one entry: "scaled" (skd_conv3x3_split2h_scaled_nhwc with the device
    word of x, or the given word value), "unscaled" (skd_conv3x3_split2h_nhwc), "three" (skd_conv3x3_split_nhwc)."""
    A = BC.Arena(DEV)
    wd = A.inp("w", w.contiguous())
    pf, pb = pack_pair(hip, A, wd, 3 if mode == "three" else "fp16", fwd=not backward, bwd=backward)
    pack = pb if backward else pf
    b, cin, h, ww = x.shape
    cout = int(w.shape[1] if backward else w.shape[0])
    xa = A.inp("x", nhwc(x))
    out = A.out("y", (b, h, ww, cout))
    if mode == "scaled":
        if word_value is None:
            word, _ = scale_word(hip, A, xa)
        else:
            word = A.inp("word", torch.tensor([word_value], dtype=torch.int64).to(torch.int32))
        assert hip.skd_conv3x3_split2h_scaled_nhwc(b, h, ww, cin, cout, d, P(xa), P(pack), P(out), P(word), geometry, None) == 1
    else:
        entry = hip.skd_conv3x3_split2h_nhwc if mode == "unscaled" else hip.skd_conv3x3_split_nhwc
        assert entry(b, h, ww, cin, cout, d, P(xa), P(pack), P(out), None, None, None, None, None, 0.0, 0, 0.01, geometry, None) == 1
    A.check()
    return out.cpu().permute(0, 3, 1, 2)


def wgrad(hip, x, g, d, slices, mode):
    """dw (Cout, Cin, 3, 3) on the CPU, channels-last strides, from two calls on the same guarded buffers.  "scaled": the fp16 entry
    with the device word of g; "noword": the fp16 entry with word NULL; "zero": with a zero word (scale 1); "three": three pieces."""
    b, cin, h, w = x.shape
    cout = g.shape[1]
    plan = (ctypes.c_int64 * 3)()
    planner = hip.skd_conv3x3_split_wgrad_plan if mode == "three" else hip.skd_conv3x3_split2h_wgrad_plan
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert planner(b, h, w, cin, cout, slices, cus, ctypes.cast(plan, ctypes.c_void_p)) == 1
    used, nbytes = int(plan[0]), int(plan[2])
    assert nbytes == used * 9 * cin * cout * 4 and (slices == 0 or used == slices)
    A = BC.Arena(DEV)
    xa, ga = A.inp("x", nhwc(x)), A.inp("g", nhwc(g))
    dw = A.out("dw", (cout, 3, 3, cin)).permute(0, 3, 1, 2)
    ws = A.ws("workspace", nbytes // 4)
    assert bool((ws.view(torch.uint8) == BC.FILL).all()), "the workspace starts dirty"
    word = None
    if mode == "scaled":
        word, _ = scale_word(hip, BC.Arena(DEV), ga)        # an arena of its own: ``A.reset()`` below would wipe an output of A
    elif mode == "zero":
        word = A.inp("word", torch.zeros(1, dtype=torch.int32))
    results = []
    for k in range(2):
        if k:
            A.reset()
        if mode == "three":
            assert hip.skd_conv3x3_split_wgrad_nhwc(b, h, w, cin, cout, d, P(xa), P(ga), P(dw), *dw.stride(), P(ws), nbytes, used, None) == 1
        else:
            assert hip.skd_conv3x3_split2h_wgrad_nhwc(b, h, w, cin, cout, d, P(xa), P(ga), P(dw), *dw.stride(), P(ws), nbytes, P(word), used,
                                                      None) == 1
        A.check()
        results.append(dw.detach().cpu().clone())
    assert BC.same_bits(results[0], results[1]), "two calls on the same buffers differ"
    return results[0]


def product(hip, name, a, b, d, mode, slices=1):
    """dgrad: (g, w) -> dx; wgrad: (x, g) -> dw."""
    if name == "wgrad":
        return wgrad(hip, a, b, d, slices, mode)
    return conv(hip, a, b, d, mode, backward=True)


# ---- 1. the pack pair ---------------------------------------------------------------------------------------------------------

LAYOUTS = ("contiguous", "channels_last", "slice")


def _weight(A, cin, cout, layout, seed):
    gen = torch.Generator().manual_seed(seed)
    wide = cin + (64 if layout == "slice" else 0)
    w = torch.randn(cout, wide, 3, 3, generator=gen) * torch.exp2(torch.randint(-12, 4, (cout, wide, 1, 1), generator=gen).float())
    view = A.inp("w", w) if layout == "contiguous" else A.inp("w", nhwc(w)).permute(0, 3, 1, 2)
    if layout == "slice":
        view, w = view[:, 64:], w[:, 64:]
    assert tuple(view.shape) == (cout, cin, 3, 3)
    return view, w.contiguous()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("chans", T.CHANNELS, ids=lambda c: "%dto%d" % c)
def test_pack_pair_equals_pack_weights_byte_for_byte(hip, chans, layout):
    cin, cout = chans
    A = BC.Arena(DEV)
    view, w = _weight(A, cin, cout, layout, 200 + cin // 128)
    n = int(hip.skd_conv3x3_split2h_pack_bytes(cin, cout))
    assert n == 36 * cin * cout == int(hip.skd_conv3x3_split2h_pack_bytes(cout, cin))
    wd = A.inp("wd", w.flip(2, 3).transpose(0, 1).contiguous())          # the MATERIALISED Wd[c][n][ty][tx] = w[n][c][2 - ty][2 - tx]
    wc = A.inp("wc", w)
    want_f, want_b = A.out("want_fwd", (n,), torch.uint8, row=4096), A.out("want_bwd", (n,), torch.uint8, row=4096)
    assert hip.skd_conv3x3_split2h_pack_weights(cin, cout, P(wc), *wc.stride(), P(want_f), n, None) == 1
    assert hip.skd_conv3x3_split2h_pack_weights(cout, cin, P(wd), *wd.stride(), P(want_b), n, None) == 1
    A.check()
    pf, pb = pack_pair(hip, A, view)
    assert torch.equal(pf, want_f), "forward image: %d bytes differ" % int((pf != want_f).sum())
    assert torch.equal(pb, want_b), "backward image: %d bytes differ" % int((pb != want_b).sum())
    assert not torch.equal(want_f, want_b)
    only_f, none = pack_pair(hip, A, view, bwd=False)
    assert none is None and torch.equal(only_f, want_f)
    none, only_b = pack_pair(hip, A, view, fwd=False)
    assert none is None and torch.equal(only_b, want_b)
    assert hip.skd_conv3x3_split2h_pack_pair(cin, cout, P(view), *view.stride(), P(pf), n, P(pb), n, None) == 1
    A.check()
    assert torch.equal(pf, want_f) and torch.equal(pb, want_b), "a second call on the same buffers"


def test_pack_pair_refusals_launch_nothing(hip):
    cin, cout = 128, 256
    A = BC.Arena(DEV)
    view, _ = _weight(A, cin, cout, "channels_last", 7)
    n = 36 * cin * cout
    pf, pb = A.out("pack_fwd", (n + 16,), torch.uint8, row=4096), A.out("pack_bwd", (n + 16,), torch.uint8, row=4096)
    s = view.stride()
    f = hip.skd_conv3x3_split2h_pack_pair
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


# ---- 2. the scale word ----------------------------------------------------------------------------------------------------------

def _word_cases():
    gen = torch.Generator().manual_seed(3501)
    ragged = torch.randn(4097, generator=gen)
    last = torch.randn(4097, generator=gen)
    last[-1] = -77.0
    slabs = torch.randn(3 * 65536 + 5, generator=gen) * 1e-9          # four workgroups and a finishing one; a ragged tail
    slabs_last = slabs.clone()
    slabs_last[-1] = 3e-7
    inf, nan = ragged.clone(), ragged.clone()
    inf[1234], nan[4095] = float("-inf"), float("nan")
    sub = torch.full((37,), 1e-41)
    return {"n=1": torch.tensor([-2.5]), "n=4097": ragged, "maximum last": last, "slabs": slabs, "slabs, maximum last": slabs_last,
            "zeros": torch.zeros(515), "minus zeros": -torch.zeros(515), "one infinity": inf, "one NaN": nan, "subnormal": sub,
            "n=3": torch.tensor([1.0, -4.0, 2.0]), "n=1024 + 3": torch.randn(1027, generator=gen) * 1e20}


@pytest.mark.parametrize("name", list(_word_cases()))
def test_scale_word_is_the_host_maximum_of_the_bit_patterns(hip, name):
    t = _word_cases()[name]
    A = BC.Arena(DEV)
    g = A.inp("g", t)
    _, got = scale_word(hip, A, g)
    want = T.word_of(t)
    assert got == want, "%s: word %#x, host maximum %#x" % (name, got, want)
    if name == "one infinity":
        assert got == 0x7F800000
    if name == "one NaN":
        assert got > 0x7F800000
    if name.endswith("zeros"):
        assert got == 0


def test_scale_word_refusals_write_nothing(hip):
    A = BC.Arena(DEV)
    g = A.inp("g", torch.randn(4100))
    ws, word = A.ws("ws", 4), A.out("word", (1,), torch.int32)
    f = hip.skd_fp16_scale_word
    off = lambda t, k: ctypes.c_void_p(t.data_ptr() + k)
    refused = [f(4097, None, P(ws), 16, P(word), None), f(4097, P(g), None, 16, P(word), None), f(4097, P(g), P(ws), 16, None, None),
               f(0, P(g), P(ws), 16, P(word), None), f(-3, P(g), P(ws), 16, P(word), None), f(4096, off(g, 4), P(ws), 16, P(word), None),
               f(4097, P(g), P(ws), 3, P(word), None), f(4097, P(g), off(ws, 2), 8, P(word), None)]
    assert refused == [0] * len(refused), refused
    A.check()
    assert bool((word.view(torch.uint8) == BC.FILL).all()) and bool((ws.view(torch.uint8) == BC.FILL).all())


# ---- 3. integers: exact, through the scale ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.name)
def test_integer_products_are_exact(hip, case):
    built = T.build(case)
    exact = built.exact()
    for slices in (T.WGRAD_SLICES if case.product == "wgrad" else (1,)):
        got = product(hip, case.product, built.a, built.b, case.d, "scaled", slices).double()
        assert got.shape == exact.shape
        wrong = int((got != exact).sum())
        assert wrong == 0, "%s, %d slice(s): %d of %d outputs differ from the exact product (largest difference %g of %g)" % (
            case.name, slices, wrong, exact.numel(), float((got - exact).abs().max()), float(exact.abs().max()))


# ---- 4. / 5. scale invariance and the bit link -------------------------------------------------------------------------------------

_FLOAT = {}


def float_case(cin, cout, d, factor):
    """Post-ReLU-like x, He-scaled w, Gaussian g times ``factor``, the float64 gradient products and their bounds' ingredients; made
    once per key and shared (never modified)."""
    key = (cin, cout, d, factor)
    if key not in _FLOAT:
        gen = torch.Generator().manual_seed(3500 + cin // 128 + 10 * d)
        x = cl(torch.relu(torch.randn(T.B, cin, T.H, T.W, generator=gen) + torch.randn(1, cin, 1, 1, generator=gen) * 0.5))
        w = torch.randn(cout, cin, 3, 3, generator=gen) * (2.0 / (9 * cin)) ** 0.5
        g = cl(torch.randn(T.B, cout, T.H, T.W, generator=gen) * factor)
        ops = {"dgrad": (SE.dgrad_op(1, d, d, (T.H, T.W)), g, w), "wgrad": (SE.wgrad_op(1, d, d, 3), x, g)}
        ref = {k: op(a.double(), b.double()) for k, (op, a, b) in ops.items()}
        _FLOAT[key] = (x, w, g, ops, ref)
    return _FLOAT[key]


@pytest.mark.parametrize("chans", T.CHANNELS, ids=lambda c: "%dto%d" % c)
def test_scale_invariance_on_the_device(hip, chans):
    cin, cout = chans
    x, w, g, _, _ = float_case(cin, cout, 2, 1.0)
    base_dx = conv(hip, g, w, 2, "scaled", backward=True)
    base_dw = {s: wgrad(hip, x, g, 2, s, "scaled") for s in T.WGRAD_SLICES}
    for geometry in (1, 2, 3):                             # every forced tile height of the scaled entry (1 and 3: the tall tile) gives those bits
        assert BC.same_bits(conv(hip, g, w, 2, "scaled", backward=True, geometry=geometry), base_dx), "data gradient, geometry %d" % geometry
    for j in (-40, -20, 20):
        up = 2.0 ** j
        assert BC.same_bits(conv(hip, cl(g * up), w, 2, "scaled", backward=True), base_dx * up), "data gradient, 2^%d" % j
        for s in T.WGRAD_SLICES:
            assert BC.same_bits(wgrad(hip, x, cl(g * up), 2, s, "scaled"), base_dw[s] * up), "weight gradient, %d slices, 2^%d" % (s, j)


@pytest.mark.parametrize("d", T.DILATIONS, ids=lambda d: "d%d" % d)
@pytest.mark.parametrize("chans", T.CHANNELS, ids=lambda c: "%dto%d" % c)
def test_unit_scale_word_is_the_unscaled_entry(hip, chans, d):
    cin, cout = chans
    x, w, g, _, _ = float_case(cin, cout, d, 1.0)
    g14 = cl(g * (1.5 * 2.0 ** 14 / float(g.abs().max())))              # amax in [2^14, 2^15): the word's own scale is 1
    assert T.scale_of(g14) == (1.0, 1.0)
    want = conv(hip, g14, w, d, "unscaled", backward=True)
    assert BC.same_bits(conv(hip, g14, w, d, "scaled", backward=True), want), "the device word of a g whose scale is 1"
    assert BC.same_bits(conv(hip, g14, w, d, "scaled", backward=True, word_value=0), want), "a zero word"
    assert BC.same_bits(conv(hip, g14, w, d, "scaled", backward=True, word_value=0x7F800000), want), "a non-finite word"
    # ... on the forward image too: the scaled entry is that convolution, whatever the pack holds
    assert BC.same_bits(conv(hip, x, w, d, "scaled", word_value=0), conv(hip, x, w, d, "unscaled"))
    for s in T.WGRAD_SLICES:
        none = wgrad(hip, x, g14, d, s, "noword")
        assert BC.same_bits(wgrad(hip, x, g14, d, s, "zero"), none) and BC.same_bits(wgrad(hip, x, g14, d, s, "scaled"), none)


# ---- 6. the reason the scale exists -------------------------------------------------------------------------------------------------

def _check_bound(hip, name, cin, cout, d, factor, slices=1):
    """(relative error of the fp16 entry, of its three-piece twin) after asserting every element within the header's bound."""
    x, w, g, ops, ref = float_case(cin, cout, d, factor)
    op, a, b = ops[name]
    y64 = ref[name]
    y3 = product(hip, name, a, b, d, "three", slices).double()
    yh = product(hip, name, a, b, d, "scaled", slices).double()
    e3 = float((y3 - y64).abs().max())
    err = (yh - y64).abs()
    bound = T.bound(op, a, b, T.G_IS[name], e3)
    share, scale = float((err / bound).max()), float(y64.abs().max())
    print("FLOAT %s %dto%d d%d slices %d g x %g: fp16 max|err| %.3e (%.3e of max|y|), largest share of the bound %.4f; three pieces e3 %.3e "
          "(%.3e); ratio %.2f" % (name, cin, cout, d, slices, factor, float(err.max()), float(err.max()) / scale, share, e3, e3 / scale,
                                  float(err.max()) / e3))
    assert bool(torch.isfinite(yh).all())
    over = int((err > bound).sum())
    assert over == 0, "%s: %d of %d elements above 2^-21 sum|a||b| + 2^-49 amax(g) sum|b| + e3 (largest share %.4f)" % (
        name, over, err.numel(), share)
    assert not torch.equal(yh, y3), "fp16 pieces and three bf16 pieces give the same bits on float data: the wrong entry ran"
    return float(err.max()) / scale, e3 / scale


@pytest.mark.parametrize("chans", T.CHANNELS, ids=lambda c: "%dto%d" % c)
def test_small_gradients_need_the_scale(hip, chans):
    """Gaussian g 2^-30, He-scaled weights.  The new entries meet the bound; the same data gradient through the EXISTING unscaled
    skd_conv3x3_split2h_nhwc is off by more than 1e-3 of the output's largest magnitude -- the documented reason for the word."""
    cin, cout = chans
    factor = 2.0 ** -30
    _check_bound(hip, "dgrad", cin, cout, 2, factor)
    for s in T.WGRAD_SLICES:
        _check_bound(hip, "wgrad", cin, cout, 2, factor, s)
    x, w, g, _, ref = float_case(cin, cout, 2, factor)
    unscaled = conv(hip, g, w, 2, "unscaled", backward=True).double()
    rel = float((unscaled - ref["dgrad"]).abs().max()) / float(ref["dgrad"].abs().max())
    print("UNSCALED dgrad %dto%d: %.3e of max|y|" % (cin, cout, rel))
    assert rel > 1e-3, "the unscaled fp16 split was expected to lose a 2^-30 gradient (%.3e)" % rel
    noword = wgrad(hip, x, g, 2, 1, "noword").double()
    relw = float((noword - ref["wgrad"]).abs().max()) / float(ref["wgrad"].abs().max())
    print("UNSCALED wgrad %dto%d: %.3e of max|y|" % (cin, cout, relw))
    assert relw > 1e-3


# ---- 7. float products ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", T.DILATIONS, ids=lambda d: "d%d" % d)
@pytest.mark.parametrize("chans", T.CHANNELS, ids=lambda c: "%dto%d" % c)
def test_float_products_within_the_bound_and_twice_the_three_piece_error(hip, chans, d):
    cin, cout = chans
    worst = []
    eh, e3 = _check_bound(hip, "dgrad", cin, cout, d, 1e-6)
    worst.append(("dgrad", eh / e3))
    for s in T.WGRAD_SLICES:
        eh, e3 = _check_bound(hip, "wgrad", cin, cout, d, 1e-6, s)
        worst.append(("wgrad, %d slices" % s, eh / e3))
    bad = [(k, r) for k, r in worst if not r <= MARGIN]
    assert not bad, "largest error against the three-piece twin's above %.1f x: %s" % (MARGIN, bad)


# ---- 8. loudness --------------------------------------------------------------------------------------------------------------------

def test_non_finite_gradients_stay_loud_and_large_ones_are_finite(hip):
    cin, cout, d = 128, 256, 1
    x, w, g, ops, _ = float_case(cin, cout, d, 1.0)
    for poison in (float("inf"), float("nan")):
        gp = g.clone()
        gp[1, 77, 4, 5] = poison
        gp = cl(gp)
        dx = conv(hip, gp, w, d, "scaled", backward=True)
        assert not bool(torch.isfinite(dx[1, :, 3:6, 4:7]).any()), "every data-gradient pixel that reads the poisoned g is non-finite"
        dw = wgrad(hip, x, gp, d, 1, "scaled")
        assert not bool(torch.isfinite(dw[77]).any()) and not bool(torch.isfinite(dw).all())
    # a finite g of magnitude 3e5 is above fp16's range and comes out finite and correct to the bound
    _check_bound(hip, "dgrad", cin, cout, d, 3e5)
    _check_bound(hip, "wgrad", cin, cout, d, 3e5, 3)
    # x is NOT scaled: above 65504 the forward and the weight gradient are NaN (skd_split2h.h's loud contract)
    xb = x.clone()
    xb[0, 5, 2, 3] = 7e4
    xb = cl(xb)
    y = conv(hip, xb, w, d, "unscaled")
    assert bool(torch.isnan(y[0, :, 1:4, 2:5]).all()) and bool(torch.isfinite(y[1]).all())
    dw = wgrad(hip, xb, g, d, 1, "scaled")
    assert bool(torch.isnan(dw[:, 5]).all()) and bool(torch.isfinite(dw[:, 6]).all())


# ---- 9. guard bands: every pointer of the five entries, explicitly ---------------------------------------------------------------------

def test_new_entries_between_guards(hip):
    """Dirty outputs, workspaces of exactly the queried size and uninitialised, each workspace entry called twice (``scale_word``
    and ``wgrad`` do that and check the guards after every call); the plan writes its three words and nothing else."""
    cin, cout, d = 256, 128, 2
    x, w, g, _, _ = float_case(cin, cout, d, 1e-6)
    for slices in (1, 3, 0):
        wgrad(hip, x, g, d, slices, "scaled")
        wgrad(hip, x, g, d, slices, "noword")
    conv(hip, g, w, d, "scaled", backward=True)
    A = BC.Arena(DEV)
    wv = A.inp("w", nhwc(w)).permute(0, 3, 1, 2)
    pf, pb = pack_pair(hip, A, wv)
    first = (pf.cpu().clone(), pb.cpu().clone())
    A.reset()
    assert bool((pf == BC.FILL).all())
    n = pf.numel()
    assert hip.skd_conv3x3_split2h_pack_pair(cin, cout, P(wv), *wv.stride(), P(pf), n, P(pb), n, None) == 1
    A.check()
    assert torch.equal(pf.cpu(), first[0]) and torch.equal(pb.cpu(), first[1])
    for n in (1, 4097, 3 * 65536 + 5):
        scale_word(hip, BC.Arena(DEV), BC.Arena(DEV).inp("g", torch.randn(n)))
    buf = (ctypes.c_int64 * 5)(-1, -1, -1, -1, -1)
    at = ctypes.cast(ctypes.addressof(buf) + 8, ctypes.c_void_p)
    assert hip.skd_conv3x3_split2h_wgrad_plan(T.B, T.H, T.W, cin, cout, 3, 0, at) == 1
    assert buf[0] == -1 and buf[4] == -1 and list(buf[1:4]) == [3, 5, 3 * 9 * cin * cout * 4]


# ---- 10. autograd ---------------------------------------------------------------------------------------------------------------------

class TwoConvs(torch.nn.Module):
    """128 -> 256 -> 128, dilation 2, both with a bias, both on conv3x3_split_train or conv3x3_split_train_fp16 by the module's
    mode, with the module's ``wgrad``."""

    def __init__(self, w1, b1, w2, b2):
        super().__init__()
        self.c1, self.c2 = torch.nn.Conv2d(128, 256, 3, 1, 2, 2), torch.nn.Conv2d(256, 128, 3, 1, 2, 2)
        with torch.no_grad():
            for conv_, wt, bs in ((self.c1, w1, b1), (self.c2, w2, b2)):
                conv_.weight.copy_(wt)
                conv_.bias.copy_(bs)
        self.to(DEV).to(memory_format=torch.channels_last)
        self.fp16, self.wgrad = False, False

    def forward(self, x):
        op = SF.conv3x3_split_train_fp16 if self.fp16 else SF.conv3x3_split_train
        h = op(x, self.c1.weight, 2, self.c1.bias, self.c1, wgrad=self.wgrad)
        return op(h, self.c2.weight, 2, self.c2.bias, self.c2, wgrad=self.wgrad)


def _two_convs_case():
    gen = torch.Generator().manual_seed(3506)
    x = cl(torch.relu(torch.randn(T.B, 128, T.H, T.W, generator=gen) + torch.randn(1, 128, 1, 1, generator=gen) * 0.5))
    w1 = torch.randn(256, 128, 3, 3, generator=gen) * (2.0 / (9 * 128)) ** 0.5
    w2 = torch.randn(128, 256, 3, 3, generator=gen) * (2.0 / (9 * 256)) ** 0.5
    b1, b2 = torch.randn(256, generator=gen) * 0.2, torch.randn(128, generator=gen) * 0.2
    go = cl(torch.randn(T.B, 128, T.H, T.W, generator=gen) * 1e-5)
    return x, w1, b1, w2, b2, go


def _chain64(x, w1, b1, w2, b2, go):
    """float64 results of the chain and, for each, the bound on an fp16 run's deviation from float64 that follows from the
    per-product bound of the header by linearity and the triangle inequality: a product of an operand that already carries the
    deviation E adds (E convolved with the absolute value of the other operand), first order in 2^-21.  The forward products
    carry the first term alone (nothing is scaled there; fp16's subnormal resolution 2^-35 of a residual, against activations of
    order 1 and weights of order 2^-5, is below it by orders of magnitude and is covered by the 2 e3 the caller adds)."""
    X, W1, W2, G = x.double(), w1.double(), w2.double(), go.double()
    fwd, dgr, wgr = SE.conv_op(1, 2, 2), SE.dgrad_op(1, 2, 2, (T.H, T.W)), SE.wgrad_op(1, 2, 2, 3)
    h = fwd(X, W1) + b1.double().view(1, -1, 1, 1)
    y = fwd(h, W2) + b2.double().view(1, -1, 1, 1)
    gh = dgr(G, W2)
    want = dict(y=y, dx=dgr(gh, W1), dw1=wgr(X, gh), dw2=wgr(h, G), db1=gh.sum((0, 2, 3)), db2=G.sum((0, 2, 3)))
    eps = T.EPS2H
    sub = lambda g: T.EPS_SUB * float(g.abs().max())
    one = torch.ones_like
    Eh = eps * fwd(X.abs(), W1.abs())
    Egh = eps * dgr(G.abs(), W2.abs()) + sub(G) * dgr(one(G), W2.abs())
    bound = dict(y=eps * fwd(h.abs(), W2.abs()) + fwd(Eh, W2.abs()),
                 dx=eps * dgr(gh.abs(), W1.abs()) + sub(gh) * dgr(one(gh), W1.abs()) + dgr(Egh, W1.abs()),
                 dw1=eps * wgr(X.abs(), gh.abs()) + sub(gh) * wgr(X.abs(), one(gh)) + wgr(X.abs(), Egh),
                 dw2=eps * wgr(h.abs(), G.abs()) + sub(G) * wgr(h.abs(), one(G)) + wgr(Eh, G.abs()),
                 db1=Egh.sum((0, 2, 3)))
    return want, bound


def _run(net, x, go, fp16, wg):
    net.fp16, net.wgrad = fp16, wg
    xg = x.to(DEV).clone().requires_grad_(True)
    y = net(xg)
    grads = torch.autograd.grad(y, [xg, net.c1.weight, net.c2.weight, net.c1.bias, net.c2.bias], go.to(DEV))
    return dict(zip(("y", "dx", "dw1", "dw2", "db1", "db2"), [t.detach().cpu() for t in (y,) + tuple(grads)]))


@pytest.mark.parametrize("wg", [False, True], ids=["library-wgrad", "split-wgrad"])
def test_autograd_fp16_against_three_pieces(hip, wg, monkeypatch):
    x, w1, b1, w2, b2, go = _two_convs_case()
    want, bound = _chain64(x, w1, b1, w2, b2, go)
    calls = []
    real3, realh, realw = SF.conv3x3_split_wgrad, SF.conv3x3_split_wgrad_fp16, SF.fp16_scale_word
    monkeypatch.setattr(SF, "conv3x3_split_wgrad", lambda *a, **k: calls.append(3) or real3(*a, **k))
    monkeypatch.setattr(SF, "conv3x3_split_wgrad_fp16", lambda *a, **k: calls.append("h" if k.get("word") is not None else "h0") or realh(*a, **k))
    monkeypatch.setattr(SF, "fp16_scale_word", lambda g: calls.append("word") or realw(g))
    net = TwoConvs(w1, b1, w2, b2)
    r3 = _run(net, x, go, False, wg)
    rh = _run(net, x, go, True, wg)
    assert calls == ([3, 3, "word", "h", "word", "h"] if wg else ["word", "word"]), calls
    for k in ("y", "dx", "dw1", "dw2", "db1"):
        e3 = float((r3[k].double() - want[k]).abs().max())
        diff = (rh[k].double() - r3[k].double()).abs()
        over = int((diff > bound[k] + 2 * e3).sum())
        print("AUTOGRAD wgrad=%s %s: max |fp16 - three| %.3e, largest share of the bound %.4f, e3 %.3e; fp16 against float64 %.3e"
              % (wg, k, float(diff.max()), float((diff / (bound[k] + 2 * e3)).max()), e3, float((rh[k].double() - want[k]).abs().max())))
        assert over == 0, "%s: %d of %d elements of |fp16 - three| above the bound" % (k, over, diff.numel())
        if k in ("y", "dx") or wg:
            assert float(diff.max()) > 0, "%s: fp16 pieces and three give the same bits" % k
    assert torch.equal(rh["db2"], r3["db2"]), "the last bias gradient is the library's sum of the given gradient"
    # a weight update between two forwards is seen, and each mode is served the image of its own format and of these weights
    with torch.no_grad():
        net.c1.weight.mul_(1.5)
        net.c2.weight.add_(0.01)
    after = _run(net, x, go, True, wg)
    fresh = TwoConvs(net.c1.weight.detach().cpu(), b1, net.c2.weight.detach().cpu(), b2)
    freshh, fresh3 = _run(fresh, x, go, True, wg), _run(fresh, x, go, False, wg)
    same = ("y", "dx") + (("dw1", "dw2") if wg else ())
    assert not torch.equal(after["y"], rh["y"])
    assert all(torch.equal(after[k], freshh[k]) for k in same), "a stale fp16 pack was served after the update"
    assert all(torch.equal(_run(net, x, go, False, wg)[k], fresh3[k]) for k in same)
    assert all(torch.equal(_run(net, x, go, True, wg)[k], freshh[k]) for k in same), "a stale image after fp16 -> three -> fp16"
    for conv_ in (net.c1, net.c2):
        assert getattr(conv_, SF._TRAIN2H_PACK_ATTR)[1].numel() * 3 == conv_._skd_conv3x3_train_pack[1].numel() * 2
        SF.drop_conv3x3_packs(conv_)
        assert not hasattr(conv_, SF._TRAIN2H_PACK_ATTR) and not hasattr(conv_, "_skd_conv3x3_train_pack")


def test_ops_give_the_entries_bits(hip):
    """fp16_scale_word, conv3x3_train_packs_fp16, conv3x3_split_wgrad_fp16 and the scaled launch are the entries, bit for bit."""
    cin, cout, d = 128, 256, 2
    x, w, g, _, _ = float_case(cin, cout, d, 1e-6)
    gd, xd, wd = g.to(DEV), x.to(DEV), cl(w).to(DEV)
    word = SF.fp16_scale_word(gd)
    assert word.dtype == torch.int32 and int(word.cpu()[0]) == T.word_of(g)
    pf, pb = SF.conv3x3_train_packs_fp16(wd)
    dx = SF._conv3x3_scaled_launch(gd, pb, cin, d, word)
    assert BC.same_bits(dx.cpu(), conv(hip, g, w, d, "scaled", backward=True))
    for s in T.WGRAD_SLICES:
        dw = SF.conv3x3_split_wgrad_fp16(xd, gd, wd, d, slices=s, word=word)
        assert BC.same_bits(dw.cpu(), wgrad(hip, x, g, d, s, "scaled"))
        assert BC.same_bits(SF.conv3x3_split_wgrad_fp16(xd, gd, wd, d, slices=s).cpu(), wgrad(hip, x, g, d, s, "noword"))
    with pytest.raises(ValueError, match="word"):
        SF.conv3x3_split_wgrad_fp16(xd, gd, wd, d, word=word.float())
    with pytest.raises(ValueError, match="fp16_scale_word"):
        SF.fp16_scale_word(gd[:, ::2])


# ---- 11. one step -----------------------------------------------------------------------------------------------------------------------

def test_one_step_student_fp16_against_three_pieces(monkeypatch):
    """The config-1 step of tests/test_step_gpu.py (batch 2, 256 x 256, Pi + Pa), same seed and inputs, with split_train and
    split_wgrad on: on three pieces (twice: the floor two runs of one path leave) and with student_pieces=2,
    student_piece_format="fp16".  The launches are counted through the library's kernel-timing hook; the first step's losses agree
    within 1e-4 relative (the project's parity contract); every parameter is finite after the step.  The per-tensor gradient
    deviations are printed beside the rerun floor, not bounded."""
    import test_step_gpu as TS
    new = ["skd_fp16_scale_word", "skd_conv3x3_split2h_pack_pair", "skd_conv3x3_split2h_scaled_nhwc", "skd_conv3x3_split2h_wgrad_nhwc"]
    fwd, three = "skd_conv3x3_split2h_nhwc", "skd_conv3x3_split_nhwc"
    old = ["skd_conv3x3_split_pack_pair", "skd_conv3x3_split_wgrad_nhwc", "skd_conv3x3_split2_pack_pair", "skd_conv3x3_split2_nhwc",
           "skd_conv3x3_split2_wgrad_nhwc"]
    monkeypatch.setenv("SKD_SPLIT_TRAIN", "1")
    monkeypatch.setenv("SKD_SPLIT_WGRAD", "1")
    for env in ("SKD_TEACHER_PIECES", "SKD_TEACHER_PIECE_FORMAT"):
        monkeypatch.delenv(env, raising=False)
    # skd_conv3x3_split_nhwc serves the frozen teacher too, eagerly or inside its captured graph: counted in a student-only
    # forward + backward of each leg's model instead (26 launches on three pieces -- 13 forwards, 13 data gradients -- none on fp16)
    def student_three_piece_launches(model):
        x = torch.randn(2, 3, 256, 256, device=DEV).contiguous(memory_format=torch.channels_last)
        model.student.train()
        _lib.enable_kernel_timing([three])
        try:
            sum(o.float().sum() for o in model.student(x)).backward()
            torch.cuda.synchronize()
        finally:
            n = len(_lib.disable_kernel_timing()[three])
        model.student.zero_grad(set_to_none=True)
        return n

    runs = {}
    for leg, pieces, fmt in (("three", 3, "bf16"), ("three again", 3, "bf16"), ("fp16", 2, "fp16")):
        monkeypatch.setenv("SKD_STUDENT_PIECES", str(pieces))
        monkeypatch.setenv("SKD_STUDENT_PIECE_FORMAT", fmt)
        _lib.enable_kernel_timing(new + old + [fwd])
        try:
            model, grads, _ = TS._config1_step(pa=True)
        finally:
            calls = _lib.disable_kernel_timing()
        assert model.split_train and model.split_wgrad and (model.student_pieces, model.student_piece_format) == (pieces, fmt)
        losses = {k: float(getattr(model, k)) for k in ("mc_G_loss", "pi_G_loss", "pa_G_loss")}
        finite = all(bool(torch.isfinite(p).all()) for p in model.student.parameters())
        runs[leg] = (losses, grads, {k: len(v) for k, v in calls.items()}, finite, student_three_piece_launches(model))
        del model
    n3, nh = runs["three"][2], runs["fp16"][2]
    print("STEP calls three pieces: %s" % n3)
    print("STEP calls fp16 pieces:  %s" % nh)
    assert all(n3[k] == 0 for k in new) and n3[fwd] == 0, "the switch off calls no fp16 entry"
    assert [nh[k] for k in new] == [13, 13, 13, 13] and nh[fwd] == 13, "13 words, pack pairs, data gradients, weight gradients, forwards"
    assert all(nh[k] == 0 for k in old), "no three-piece and no bf16 two-piece launch for the 13 convolutions"
    print("STEP student-only %s launches: three pieces %d, fp16 %d" % (three, runs["three"][4], runs["fp16"][4]))
    assert (runs["three"][4], runs["fp16"][4]) == (26, 0), "none of the three-piece forwards or data gradients on the fp16 leg"
    assert (n3["skd_conv3x3_split_pack_pair"], n3["skd_conv3x3_split_wgrad_nhwc"]) == (13, 13)
    assert runs["fp16"][3] and runs["three"][3], "a parameter is not finite after the step"
    worst, floor = [], []
    for k, g3 in runs["three"][1].items():
        gh, g3b = runs["fp16"][1][k], runs["three again"][1][k]
        rel = float((gh - g3).norm()) / max(float(g3.norm()), 1e-30)
        again = float((g3b - g3).norm()) / max(float(g3.norm()), 1e-30)
        worst.append((rel, k))
        floor.append((again, k))
        print("STEP grad %-50s |gh - g3| / |g3| = %.3e   rerun floor %.3e" % (k, rel, again))
    print("STEP worst gradient deviation: %.3e %s" % max(worst))
    print("STEP worst rerun floor:        %.3e %s" % max(floor))
    bad = []
    for k, l3 in runs["three"][0].items():
        lh = runs["fp16"][0][k]
        rel = abs(lh - l3) / abs(l3)
        print("STEP loss %s: three %.9g fp16 %.9g rel %.3e" % (k, l3, lh, rel))
        if not rel <= 1e-4:
            bad.append((k, l3, lh, rel))
    assert not bad, bad
