"""-m gpu: the two-piece (three-product) forms of include/skd_split2.h -- csrc/conv3x3.hip's 128-column forward family and
csrc/conv1x1.hip's GEMM with two bf16 pieces per operand -- against their float64 MODEL (tests/split2_ref.py: the products
a0 b0 + a0 b1 + a1 b0, exact accumulation, float64 epilogue) and against the float64 truth.

The inputs of a case are those of the three-piece tests (tests/test_conv3x3_split_gpu.py, tests/test_conv1x1_split_gpu.py: the same
recipes under the same names), so the committed parent figures of those files apply.  Two assertions per case:
  max |gpu - model| / max |model|  <=  min(4 x PARENT_ERR[name], cap)      cap = 2e-5 (3x3), 2e-6 (1x1): what separates the kernel
                                                                          from its model is fp32 accumulation, which is what that
                                                                          bound was set for;
  err(gpu, truth)  <=  err(model, truth) + that bound                     both printed.
On integer data the kernel is bit-equal to the exact product where one operand is one piece, and bit-equal to the MODEL -- and not
to the exact product -- where both operands are two pieces: the assertion that pins "three products, these three".
The network test compares a marked ResNet101-plan teacher with oracle.step_torch.pspnet_forward in float64 at 4 x the CPU emulation
figures E (tools/split2_emulation.py; profiles/r25_split2_accuracy.md); the step test runs the config-1 step with the switch on.
"""
import collections
import ctypes
import zlib

import pytest
import torch
import torch.nn.functional as F

import bounds_cases as BC
import split2_ref as R
import test_conv1x1_split_gpu as T1
import test_conv3x3_split_gpu as T3
from structure_knowledge_distillation_amd import _lib, functional as SF
from structure_knowledge_distillation_amd import networks
import structure_knowledge_distillation_amd.networks.pspnet_combine as PC

pytestmark = pytest.mark.gpu
DEV = "cuda"
P = T3.P
SENTINEL, SLACK_ROWS, RATIO = T3.SENTINEL, T3.SLACK_ROWS, 4.0
CAP3, CAP1 = 2e-5, 2e-6
ACT = T3.ACT
ACT_NAME = {0: "none", 1: "leaky_relu", 3: "relu"}

CASES3 = ["ragged-13x11-d1", "ragged-13x11-d2", "ragged-13x11-d4", "centre-3x3-d4", "longk-512-512-9x9-d4",
          "ragged-13x11-d2-bias-abn-leaky", "ragged-13x11-d2-bn-relu", "many-tiles-226x226-d1"]

# CPU emulation figures of the two-piece mode on the teacher forward of split2_ref.teacher_case (tools/split2_emulation.py,
# max |emulation - float64| / max |float64|; profiles/r25_split2_accuracy.md)
E = {"logits": 1.759e-05, "dsn": 2.125e-05, "psp": 1.509e-05}
# The config-1 step with the switch on against the switch-off run of the same process: largest relative difference of the Pi and Pa
# losses over three input seeds, measured on an MI355X (profiles/r25_split2_accuracy.md); the test asserts 4 x these.
# (Pi: 0, 1.261e-07, 0 -- one fp32 ulp of a loss of 60.48; Pa: 3.611e-07, 4.477e-06, 2.698e-06, beside a run-to-run difference of
# the switch-off step of up to 3.598e-06)
STEP_LOSS_DIFF = {"pi_G_loss": 1.261e-07, "pa_G_loss": 4.477e-06}
# L2 over all student parameters of the difference between TWO switch-off config-1 steps of one process: the largest of three seeds
# (1.441e-03, 1.950e-03, 8.715e-04; the switch-on step differs from a switch-off one by 1.328e-03, 1.755e-03, 9.361e-04)
STEP_PARAM_NOISE = 1.950e-03


@pytest.fixture(scope="module")
def hip():
    return _lib.load()


def no_epilogue():
    return {"cbias": None, "mean": None, "var": None, "gamma": None, "beta": None, "eps": 0.0, "act": "none"}


# ---- 3x3 ------------------------------------------------------------------------------------------------------------------------

def pack2(hip, wt_dev):
    cout, cin = wt_dev.shape[:2]
    nbytes = hip.skd_conv3x3_split2_pack_bytes(cin, cout)
    assert nbytes == cout * cin * 9 * 4
    buf = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    assert hip.skd_conv3x3_split2_pack_weights(cin, cout, P(wt_dev), *wt_dev.stride(), P(buf), nbytes, None)
    return buf


def run3(hip, x, wt, p, d, geometry=0, wt_format=torch.contiguous_format, pk=None, entry=None):
    """(B, Cout, H, W) output of skd_conv3x3_split2_nhwc on the CPU; the sentinel rows behind M must stay untouched."""
    b, cin, h, w = x.shape
    cout = wt.shape[0]
    m = b * h * w
    dx = x.to(DEV).contiguous(memory_format=torch.channels_last)
    if pk is None:
        pk = pack2(hip, wt.to(DEV).contiguous(memory_format=wt_format))
    out = torch.full((m + SLACK_ROWS, cout), SENTINEL, device=DEV)
    dp = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in p.items()}
    assert (entry or hip.skd_conv3x3_split2_nhwc)(b, h, w, cin, cout, d, P(dx), P(pk), P(out), P(dp["cbias"]), P(dp["mean"]),
                                                  P(dp["var"]), P(dp["gamma"]), P(dp["beta"]), p["eps"], ACT[p["act"]], 0.01,
                                                  geometry, None)
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool((out[m:] == SENTINEL).all()), "rows beyond M were written"
    return out[:m].view(b, h, w, cout).permute(0, 3, 1, 2), pk


_MODEL3 = {}


def model3(name):
    """The float64 model of a 3x3 case, computed once and shared (never modified)."""
    if name not in _MODEL3:
        x, wt, p = T3.case_inputs(name)
        d = T3.CASE[name][6]
        _MODEL3[name] = T3.epilogue64(R.conv2d_split2(x, wt, p["cbias"], 1, d, d), p)
    return _MODEL3[name]


def check(name, got, model, truth, parent, cap):
    bound = min(RATIO * parent, cap)
    to_model, to_truth, model_to_truth = R.rel_err(got, model), R.rel_err(got, truth), R.rel_err(model, truth)
    print("%s: gpu-model %.3e (bound %.3e, parent %.3e)  gpu-truth %.3e  model-truth %.3e" % (
        name, to_model, bound, parent, to_truth, model_to_truth))
    assert to_model <= bound, "%s: max |gpu - model| %.3e > %.3e" % (name, to_model, bound)
    assert to_truth <= model_to_truth + bound, "%s: %.3e > %.3e + %.3e" % (name, to_truth, model_to_truth, bound)
    return to_model, to_truth, model_to_truth


@pytest.mark.parametrize("name", CASES3)
def test_conv3x3_two_pieces_vs_model(hip, name):
    x, wt, p = T3.case_inputs(name)
    got, _ = run3(hip, x, wt, p, T3.CASE[name][6])
    check(name, got, model3(name), T3.want_of(name), T3.PARENT_ERR[name], CAP3)


# ---- 1x1 ------------------------------------------------------------------------------------------------------------------------

HH = T1.HH
# (name, K, N, M, prologue, residual, activation, geometry class or None): the recipes and names of tests/test_conv1x1_split_gpu.py
CASES1 = [
    ("ragged-K64-N256-pro-res-relu", 64, 256, T1.RAGGED_M, True, True, 3, None),
    ("ragged-K256-N1024-pro-res-relu", 256, 1024, T1.RAGGED_M, True, True, 3, None),
    ("reduce-K1024-N256", 1024, 256, T1.RAGGED_M, False, False, 3, dict(nt=0, ct=2, pm=1, half=False)),
    ("reduce-K2048-N512", 2048, 512, T1.RAGGED_M, False, False, 3, dict(nt=1, ct=1, pm=2, half=False, padded=True)),
    ("down-K1024-N2048-hh", 1024, 2048, HH, False, False, 0, dict(nt=1, ct=2, pm=4, half=True)),      # NT super-tile + half-height
    ("reduce-K256-N128-hh", 256, 128, HH, False, False, 3, dict(nt=0, ct=1, pm=1, half=True)),        # half-height, panel-major
    # the epilogue / prologue combinations of the two-piece kernel that the rows above do not instantiate (the recipes of the
    # three-piece tests under their own names, hence their measured parent figures): panel-major at K = 64 ...
    ("ragged-K64-N256-pro-res-none", 64, 256, T1.RAGGED_M, True, True, 0, None),
    ("ragged-K64-N256-nopro-res-none", 64, 256, T1.RAGGED_M, False, True, 0, None),
    ("ragged-K64-N256-nopro-res-relu", 64, 256, T1.RAGGED_M, False, True, 3, None),
    ("ragged-K64-N256-pro-nores-relu", 64, 256, T1.RAGGED_M, True, False, 3, None),
    # ... and in column chunks (NT) at K = 512, N = 2048
    ("ragged-K512-N2048-pro-nores-none", 512, 2048, T1.RAGGED_M, True, False, 0, dict(nt=1, ct=4, pm=8, half=False)),
    ("ragged-K512-N2048-nopro-res-none", 512, 2048, T1.RAGGED_M, False, True, 0, dict(nt=1, ct=4, pm=8, half=False)),
    ("ragged-K512-N2048-pro-res-none", 512, 2048, T1.RAGGED_M, True, True, 0, dict(nt=1, ct=4, pm=8, half=False)),
    ("ragged-K512-N2048-nopro-res-relu", 512, 2048, T1.RAGGED_M, False, True, 3, dict(nt=1, ct=4, pm=8, half=False)),
]


def inputs1(name, m, k, n, pro, res):
    """The "teacher" recipe of tests/test_conv1x1_split_gpu.case_outputs (same draws in the same order)."""
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    w = torch.randn(n, k, generator=g) * 0.05
    pack_src = None
    if pro:
        x = torch.randn(m, k, generator=g) * 2 + torch.randn(1, k, generator=g)
        pack_src = (torch.randn(k, generator=g) * 0.5, torch.rand(k, generator=g) * 4 + 2,
                    torch.randn(k, generator=g), torch.randn(k, generator=g) * 0.5)
    else:
        x = torch.relu(torch.randn(m, k, generator=g) + torch.randn(1, k, generator=g) * 0.5)
    r = torch.relu(torch.randn(m, n, generator=g)) if res else None
    mean, var = torch.randn(n, generator=g) * 0.3, torch.rand(n, generator=g) + 0.5
    ga, be, eps = torch.randn(n, generator=g), torch.randn(n, generator=g), 1e-5
    return x, w, r, (mean, var, ga, be, eps), pack_src


def run1(hip, x, w, r, bn, pack_src, act, pieces=2):
    """((M, N) output on the CPU, the prologue's (4, K) table as the device wrote it or None)."""
    m, k = x.shape
    n = w.shape[0]
    mean, var, ga, be, eps = bn
    o_g = torch.full((m + SLACK_ROWS, n), SENTINEL, device=DEV)
    dx, dw, dr, dmean, dvar, dga, dbe = (None if t is None else t.to(DEV) for t in (x, w, r, mean, var, ga, be))
    args = (m, k, n, P(dx), P(dw), P(dr), P(o_g), P(dmean), P(dvar), P(dga), P(dbe), eps)
    pk = None
    if pack_src is None:
        assert (hip.skd_conv1x1_abn2_nhwc if pieces == 2 else hip.skd_conv1x1_abn_nhwc)(*args, act, 0.01, None)
    else:
        pk = torch.empty(4, k, device=DEV)
        dp = [t.to(DEV) for t in pack_src]
        assert hip.skd_abn_pack_eval_params(k, P(dp[0]), P(dp[1]), P(dp[2]), P(dp[3]), 1e-5, P(pk), None)
        assert (hip.skd_conv1x1_abn2_pro_nhwc if pieces == 2 else hip.skd_conv1x1_abn_pro_nhwc)(*args, P(pk), act, 0.01, None)
    torch.cuda.synchronize()
    out = o_g.cpu()
    assert bool((out[m:] == SENTINEL).all()), "rows beyond M were written"
    return out[:m], None if pk is None else pk.cpu()


def finish1(y, r, bn, act):
    """The float64 epilogue of the 1x1 entries on an (M, N) product: eval-mode ABN, + residual, activation."""
    mean, var, ga, be, eps = bn
    y = R.abn_eval64(y, mean, var, ga, be, eps, "none", channel_dim=1)
    if r is not None:
        y = y + r.double()
    return R.abn_eval64(y, None, None, None, None, 0.0, ACT_NAME[act])


@pytest.mark.parametrize("case", CASES1, ids=[c[0] for c in CASES1])
def test_conv1x1_two_pieces_vs_model(hip, case):
    name, k, n, m, pro, res, act, cls = case
    m = T1.routed_m(n, m)
    if cls is not None:
        print(T1.assert_geometry(hip, m, k, n, cls))
    x, w, r, bn, pack_src = inputs1(name, m, k, n, pro, res)
    got, table = run1(hip, x, w, r, bn, pack_src, act)
    a64 = x.double()
    a = x
    if pro:      # the prologue: in float64 for the truth, as the kernel's fp32 expression on the device's table for the model
        pm, pv, pw, pb = (t.double() for t in pack_src)
        a64 = torch.relu((a64 - pm) / torch.sqrt(pv + 1e-5) * (pw.abs() + 1e-5) + pb)
        a = R.prologue_fp32(x, table)
    truth = finish1(a64 @ w.double().t(), r, bn, act)
    model = finish1(R.mm_split2(a, w), r, bn, act)
    check(name, got, model, truth, T1.PARENT_ERR[name], CAP1)


# ---- integers ---------------------------------------------------------------------------------------------------------------------

def int_operands(seed, xshape, wshape, exact):
    """exact: x in [0, 7] (one piece), w in [-1000, 1000] (two pieces); else x in [-1000, 1000], w in [-260, 260] (two pieces each)."""
    g = torch.Generator().manual_seed(seed)
    if exact:
        return torch.randint(0, 8, xshape, generator=g).float(), torch.randint(-1000, 1001, wshape, generator=g).float()
    return torch.randint(-1000, 1001, xshape, generator=g).float(), torch.randint(-260, 261, wshape, generator=g).float()


def check_integers(got, model, product, exact, what):
    got = got.double()
    assert float(product.abs().max()) > 100.0 and float(model.abs().max()) < 2 ** 24 and float(product.abs().max()) < 2 ** 24
    if exact:      # a1 b1 = 0 and every sum is an exact fp32 integer: the float64 product itself
        assert torch.equal(model, product)
        assert torch.equal(got, product), "%s: %d of %d outputs differ" % (what, int((got != product).sum()), got.numel())
    else:          # a1 b1 != 0: the model, bit for bit -- and not the product (a six-product kernel fails here)
        assert torch.equal(got, model), "%s: %d of %d outputs differ from the model" % (what, int((got != model).sum()), got.numel())
        assert bool((got != product).any()), "%s: every output equals the exact product: a1 b1 was not dropped" % what


@pytest.mark.parametrize("exact", [True, False], ids=["one-by-two-pieces", "two-by-two-pieces"])
@pytest.mark.parametrize("shape", [(2, 13, 11, 2), (1, 5, 5, 4)], ids=["13x11-d2", "5x5-d4"])
def test_conv3x3_integers(hip, shape, exact):
    b, h, w, d = shape
    x, wt = int_operands(100 * h + d, (b, 32, h, w), (128, 32, 3, 3), exact)
    x = x.contiguous(memory_format=torch.channels_last)
    got, _ = run3(hip, x, wt, no_epilogue(), d)
    check_integers(got, R.conv2d_split2(x, wt, None, 1, d, d), F.conv2d(x.double(), wt.double(), None, 1, d, d), exact, str(shape))


@pytest.mark.parametrize("exact", [True, False], ids=["one-by-two-pieces", "two-by-two-pieces"])
def test_conv1x1_integers(hip, exact):
    m, k, n = T1.RAGGED_M, 64, 256
    assert k * 1000 * 260 + k * (1000 + 2 * 260) < 2 ** 24       # every partial sum of the one accumulator is an exact fp32 integer
    x, w = int_operands(77 + k, (m, k), (n, k), exact)
    mean, var, ga, be, eps = T1._identity_epilogue(n)
    got, _ = run1(hip, x, w, None, (mean, var, ga, be, eps), None, 0)
    check_integers(got, R.mm_split2(x, w), x.double() @ w.double().t(), exact, "K64-N256")


# ---- the pack ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cin,cout", [(32, 128), (256, 256), (16, 128)])
def test_pack_is_the_first_two_planes(hip, cin, cout):
    """Tile by tile the two-plane image is planes 0 and 1 of the three-plane one; written at exactly pack_bytes between guards."""
    wt = torch.randn(cout, cin, 3, 3, generator=torch.Generator().manual_seed(cin + cout)) * 0.1
    tiles = (cout // 128) * 9 * (cin // 16)
    packs = []
    for fmt in (torch.contiguous_format, torch.channels_last):
        A = BC.Arena(DEV)
        dw = wt.to(DEV).contiguous(memory_format=fmt)
        n2, n3 = hip.skd_conv3x3_split2_pack_bytes(cin, cout), hip.skd_conv3x3_split_pack_bytes(cin, cout)
        assert n2 == 4 * cout * cin * 9 == tiles * 2 * 2 * 128 * 16
        p2, p3 = A.out("pack2", n2, torch.uint8, row=4096), A.out("pack3", n3, torch.uint8, row=4096)
        assert hip.skd_conv3x3_split2_pack_weights(cin, cout, P(dw), *dw.stride(), P(p2), n2, None)
        assert hip.skd_conv3x3_split_pack_weights(cin, cout, P(dw), *dw.stride(), P(p3), n3, None)
        A.check()
        two, three = p2.cpu().view(tiles, 2, 2 * 128 * 16), p3.cpu().view(tiles, 3, 2 * 128 * 16)
        assert torch.equal(two, three[:, :2])
        packs.append(p2.cpu().clone())
    assert torch.equal(packs[0], packs[1]), "either memory format of the weight gives the same pack"


def test_geometries_and_repeats_give_the_same_bits(hip):
    for name in ("many-tiles-226x226-d1", "ragged-13x11-d2", "ragged-13x11-d2-bn-relu"):      # (the last: the tall tile with the ReLU epilogue)
        x, wt, p = T3.case_inputs(name)
        d = T3.CASE[name][6]
        base, pk = run3(hip, x, wt, p, d)
        again, _ = run3(hip, x, wt, p, d, pk=pk)
        assert torch.equal(again, base)
        for geometry in (1, 2, 3):
            got, _ = run3(hip, x, wt, p, d, geometry=geometry, pk=pk)
            assert torch.equal(got, base), (name, geometry)


# ---- guard bands ------------------------------------------------------------------------------------------------------------------

def test_guard_bands_around_every_operand(hip):
    """Every operand of the five entries at its exact size between 0xFF guards, the outputs pre-filled with 0xFF (an element the
    kernel did not write shows as NaN)."""
    g = torch.Generator().manual_seed(5)
    A = BC.Arena(DEV)
    b, h, w, cin, cout, d = 2, 13, 11, 32, 128, 2
    x = A.inp("x", torch.relu(torch.randn(b, h, w, cin, generator=g)))
    wt = A.inp("w", torch.randn(cout, cin, 3, 3, generator=g) * 0.1)
    vec = lambda name, n, pos=False: A.inp(name, torch.rand(n, generator=g) + 0.5 if pos else torch.randn(n, generator=g))
    cb, mean, var, ga, be = vec("cbias", cout), vec("mean", cout), vec("var", cout, True), vec("gamma", cout), vec("beta", cout)
    nbytes = hip.skd_conv3x3_split2_pack_bytes(cin, cout)
    pk = A.out("pack", nbytes, torch.uint8, row=4096)
    assert hip.skd_conv3x3_split2_pack_weights(cin, cout, P(wt), *wt.stride(), P(pk), nbytes, None)
    outs = []
    for geometry in (0, 1, 2, 3):
        y = A.out("y%d" % geometry, (b, h, w, cout))
        assert hip.skd_conv3x3_split2_nhwc(b, h, w, cin, cout, d, P(x), P(pk), P(y), P(cb), P(mean), P(var), P(ga), P(be), 1e-5,
                                           ACT["leaky_relu"], 0.01, geometry, None)
        outs.append(y)
    m = T1.routed_m(256, HH)          # whole rounds of 128-row tiles + a 64-row panel + one with a single live row
    for k, n, pro, res in ((64, 256, True, True), (256, 1024, False, False), (512, 2048, True, False)):
        mm = m if n == 256 else T1.RAGGED_M
        x1 = A.inp("x1", torch.randn(mm, k, generator=g))
        w1 = A.inp("w1", torch.randn(n, k, generator=g) * 0.05)
        r1 = A.inp("r1", torch.randn(mm, n, generator=g)) if res else None
        bn = [vec("mean1", n), vec("var1", n, True), vec("gamma1", n), vec("beta1", n)]
        y1 = A.out("y1", (mm, n))
        head = (mm, k, n, P(x1), P(w1), P(r1), P(y1), *(P(t) for t in bn), 1e-5)
        if pro:
            src = [vec("pm", k), vec("pv", k, True), vec("pw", k), vec("pb", k)]
            table = A.out("ppack", (4, k))
            assert hip.skd_abn_pack_eval_params(k, *(P(t) for t in src), 1e-5, P(table), None)
            assert hip.skd_conv1x1_abn2_pro_nhwc(*head, P(table), 3, 0.01, None)
        else:
            assert hip.skd_conv1x1_abn2_nhwc(*head, 3, 0.01, None)
        outs.append(y1)
    A.check()
    for y in outs:
        assert bool(torch.isfinite(y).all()), "an output element was not written"
    for y in outs[1:4]:
        assert torch.equal(y, outs[0])


# ---- op and routing ---------------------------------------------------------------------------------------------------------------

class Counting:
    """The library with the launches of the split-core convolution entries of both piece counts counted."""
    NAMES = ("skd_conv3x3_split2_nhwc", "skd_conv1x1_abn2_nhwc", "skd_conv1x1_abn2_pro_nhwc", "skd_conv3x3_split_nhwc",
             "skd_conv1x1_abn_nhwc", "skd_conv1x1_abn_pro_nhwc", "skd_conv3x3_split_res_nhwc")

    def __init__(self, lib):
        self.lib, self.n = lib, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if name not in self.NAMES:
            return fn

        def counted(*args):
            self.n[name] += 1
            return fn(*args)
        return counted


def test_ops_give_the_entries_bits(hip):
    from structure_knowledge_distillation_amd.libs import InPlaceABNSync
    name = "ragged-13x11-d2-bias-abn-leaky"
    x, wt, p = T3.case_inputs(name)
    conv = torch.nn.Conv2d(32, 128, 3, 1, 2, 2, bias=True)
    bn = InPlaceABNSync(128)
    with torch.no_grad():
        conv.weight.copy_(wt)
        conv.bias.copy_(p["cbias"])
        bn.weight.copy_(p["gamma"])
        bn.bias.copy_(p["beta"])
        bn.running_mean.copy_(p["mean"])
        bn.running_var.copy_(p["var"])
    conv, bn = conv.to(DEV).eval(), bn.to(DEV).eval()
    dx = x.to(DEV).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        pk2, pk3 = SF.conv3x3_pack_weights(conv, pieces=2), SF.conv3x3_pack_weights(conv)
        assert SF.conv3x3_pack_weights(conv, pieces=2) is pk2 and SF.conv3x3_pack_weights(conv, pieces=3) is pk3
        assert pk2.numel() * 3 == pk3.numel() * 2
        two = SF.conv3x3_split_eval(dx, pk2, 128, 2, conv.bias, bn, bn.activation, pieces=2)
        three = SF.conv3x3_split_eval(dx, pk3, 128, 2, conv.bias, bn, bn.activation)
        with pytest.raises(ValueError):
            SF.conv3x3_split_eval(dx, pk3, 128, 2, conv.bias, bn, bn.activation, pieces=2)      # the other piece count's pack
    want2, _ = run3(hip, x, wt, p, 2)
    want3, _ = T3.run_hip(hip, x, wt, p, 2)
    assert torch.equal(two.cpu(), want2) and torch.equal(three.cpu(), want3) and not torch.equal(want2, want3)
    # 1x1, with prologue and residual
    cname, k, n, m, pro, res, act, _ = CASES1[0]
    x1, w1, r1, (mean, var, ga, be, eps), src = inputs1(cname, m, k, n, pro, res)
    want = {pieces: run1(hip, x1, w1, r1, (mean, var, ga, be, eps), src, act, pieces)[0] for pieces in (2, 3)}
    table = torch.empty(4, k, device=DEV)
    dsrc = [t.to(DEV) for t in src]
    assert hip.skd_abn_pack_eval_params(k, *(P(t) for t in dsrc), 1e-5, P(table), None)
    as_map = lambda t, c: t.to(DEV).view(1, m, 1, c).permute(0, 3, 1, 2)
    with torch.no_grad():
        for pieces in (2, 3):
            got = SF.conv1x1_abn_eval(as_map(x1, k), w1.to(DEV).view(n, k, 1, 1), mean.to(DEV), var.to(DEV), ga.to(DEV), be.to(DEV), eps,
                                      "relu", residual=as_map(r1, n), pro=table, pieces=pieces)
            assert torch.equal(got.permute(0, 2, 3, 1).reshape(m, n).cpu(), want[pieces]), pieces
    assert not torch.equal(want[2], want[3])


def _stack():
    torch.manual_seed(3)
    down = torch.nn.Sequential(torch.nn.Conv2d(512, 1024, 1, 1, bias=False), PC.BatchNorm2d(1024))
    net = torch.nn.Sequential(PC.Bottleneck(512, 256, 1, dilation=2, downsample=down), PC.Bottleneck(1024, 256, dilation=2))
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, PC.InPlaceABNSync):
                m.running_var.uniform_(0.5, 1.5)
                m.running_mean.normal_(0, 0.1)
    return net.eval().to(DEV).to(memory_format=torch.channels_last)


def test_marked_stack_routes_through_the_new_entries(hip, monkeypatch):
    lib = Counting(hip)
    monkeypatch.setattr(_lib, "get", lambda: lib)
    net = _stack()
    x = torch.relu(torch.randn(2, 512, 17, 19, generator=torch.Generator().manual_seed(4))).to(DEV).contiguous(
        memory_format=torch.channels_last)
    with torch.no_grad():
        plain = net(x)
    assert lib.n == dict(skd_conv1x1_abn_nhwc=3, skd_conv3x3_split_nhwc=2, skd_conv1x1_abn_pro_nhwc=2)
    lib.n.clear()
    networks.set_teacher_pieces(net, 2)
    with torch.no_grad():
        marked = net(x)
    assert lib.n == dict(skd_conv1x1_abn2_nhwc=3, skd_conv3x3_split2_nhwc=2, skd_conv1x1_abn2_pro_nhwc=2)
    assert not torch.equal(marked, plain)
    diff = R.rel_err(marked.cpu(), plain.cpu().double())
    print("two blocks: max |two - three| / max |three| = %.3e" % diff)
    assert diff <= 4 * 2e-5
    lib.n.clear()
    networks.set_teacher_pieces(net, 3)
    with torch.no_grad():
        assert torch.equal(net(x), plain)
    assert lib.n == dict(skd_conv1x1_abn_nhwc=3, skd_conv3x3_split_nhwc=2, skd_conv1x1_abn_pro_nhwc=2)


# ---- the network against the float64 oracle ---------------------------------------------------------------------------------------

def test_teacher_against_the_float64_oracle():
    Pw, x = R.teacher_case()
    truth = dict(zip(("logits", "dsn", "psp"), R.teacher_forward64(Pw, x)))
    net = PC.Res_pspnet(PC.Bottleneck, [3, 4, 23, 3], 19)
    net.load_state_dict({k: v.clone() for k, v in Pw.items()})
    net = net.eval().to(DEV).to(memory_format=torch.channels_last)
    dx = x.to(DEV).contiguous(memory_format=torch.channels_last)
    errs = {}
    for pieces in (3, 2):
        networks.set_teacher_pieces(net, pieces)
        with torch.no_grad():
            out = net(dx)
        got = dict(logits=out[0].cpu(), dsn=out[1].cpu(), psp=out[2].cpu())
        errs[pieces] = {k: R.rel_err(got[k], truth[k]) for k in truth}
        agree = float((got["logits"].argmax(1) == truth["logits"].argmax(1)).double().mean())
        print("%d pieces: %s  argmax agreement %.6f" % (pieces, "  ".join("%s %.3e" % kv for kv in errs[pieces].items()), agree))
        assert agree == 1.0
    for k in truth:
        assert errs[2][k] <= 4 * E[k], (k, errs[2][k], E[k])
        assert errs[3][k] < errs[2][k], (k, errs[3][k], errs[2][k])


# ---- the step -----------------------------------------------------------------------------------------------------------------------

TEACHER_LAUNCHES = dict(skd_conv1x1_abn2_pro_nhwc=33, skd_conv1x1_abn2_nhwc=30, skd_conv3x3_split2_nhwc=28)


def test_step_config1_with_the_teacher_on_two_pieces(monkeypatch):
    """The config-1 step of tests/test_step_gpu.py (batch 2, 256 x 256, Pi + Pa; Ho is impossible at that size) with
    ``teacher_pieces=2`` against the switch-off run of the same process.  Per teacher forward the counting library sees the 33
    tails, the 30 reduce / down-sample GEMMs (27 conv1, 3 stride-1 down-samples; 512 -> 128 stays with the library) and the 28
    routed 3x3 convolutions (layer3: 23, layer4: 3, dsn[0], the PSP half) on the new entries and none on their twins (the default
    student has no split-core launch in training).  The CE loss must be bit-equal (the teacher does not enter it); Pi and Pa may move by
    4 x the largest difference recorded over three seeds.  The student's parameters behind the step (L2 over all of them) may move,
    switch on against off, by 4 x what a SECOND switch-off step of this process moves them against the first (the parent's own
    run-to-run difference: MIOpen's atomic weight gradients; 4 = the project's standing margin) plus lr x 4 max(E) x |gradient|:
    the teacher's outputs move by at most 4 E of their magnitude and enter the gradient through Pi and Pa linearly.  The
    run-to-run term is capped by STEP_PARAM_NOISE, the largest such difference recorded (profiles/r25_split2_accuracy.md), so a
    noisier process does not widen the bound."""
    import test_step_gpu as TS
    for name in ("SKD_SPLIT_TRAIN", "SKD_SPLIT_WGRAD", "SKD_SPLIT_NARROW", "SKD_SPLIT_NARROW_WGRAD", "SKD_SPLIT_SHORTCUT"):
        monkeypatch.delenv(name, raising=False)
    lib = Counting(_lib.load())
    monkeypatch.setattr(_lib, "get", lambda: lib)
    monkeypatch.setenv("SKD_TEACHER_PIECES", "3")
    off, g_off, _ = TS._config1_step(pa=True)
    assert off.teacher_pieces == 3 and not any(k in lib.n for k in TEACHER_LAUNCHES)
    print("switch off: %s" % dict(lib.n))
    forwards = lib.n["skd_conv1x1_abn_pro_nhwc"] // 33
    assert forwards >= 1 and lib.n == {k.replace("abn2", "abn").replace("split2", "split"): v * forwards for k, v in TEACHER_LAUNCHES.items()}
    lib.n.clear()
    monkeypatch.setenv("SKD_TEACHER_PIECES", "2")
    on, _, _ = TS._config1_step(pa=True)
    assert on.teacher_pieces == 2
    assert lib.n == {k: v * forwards for k, v in TEACHER_LAUNCHES.items()}, lib.n
    assert on.mc_G_loss == off.mc_G_loss, "the teacher does not enter the CE loss"
    for k in ("pi_G_loss", "pa_G_loss"):
        a, b = getattr(on, k), getattr(off, k)
        diff = abs(a - b) / abs(b)
        print("%s: two pieces %.9g  three %.9g  rel %.3e" % (k, a, b, diff))
        assert diff <= 4 * STEP_LOSS_DIFF[k], (k, diff)
    lr = float(on.G_solver.param_groups[0]["lr"])
    monkeypatch.setenv("SKD_TEACHER_PIECES", "3")
    off2, _, _ = TS._config1_step(pa=True)
    p_on, p_off, p_off2 = on.student.state_dict(), off.student.state_dict(), off2.student.state_dict()
    total = lambda a, b: float(sum(float((a[k].double() - b[k].double()).norm()) ** 2 for k in g_off) ** 0.5)
    moved, noise = total(p_on, p_off), total(p_off2, p_off)
    g_norm = float(sum(float(g.norm()) ** 2 for g in g_off.values()) ** 0.5)
    allowed = RATIO * min(noise, STEP_PARAM_NOISE) + lr * RATIO * max(E.values()) * g_norm
    print("student parameters behind the step: on - off %.3e  off - off %.3e  allowed %.3e  (lr %g, |g| %.3e)" % (
        moved, noise, allowed, lr, g_norm))
    assert moved <= allowed, (moved, noise, allowed)
