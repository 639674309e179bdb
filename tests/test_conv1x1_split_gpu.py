"""-m gpu: the split-operand bf16-MFMA core of csrc/conv1x1.hip (fp32 operands as three bf16 pieces, the six products
a_i b_j with i + j <= 2, fp32 accumulation) against the plain-C oracle (dot product in double, oracle/abn_ref.c) on the
frozen teacher's block-tail shapes.

Error figure of a case: max |hip - oracle| / max |oracle| over the whole output (the ``close()`` form of
tests/test_kernels_gpu.py).  Bound of a case: FOUR times the figure the previous fp32-MFMA core
(v_mfma_f32_32x32x2_f32, an exact fp32 fma chain) gave on the same inputs -- the dropped cross terms a1 b2, a2 b1, a2 b2
add at most 2^-23 per product to the 2^-24 per rounding of the fp32 chain -- and never more than 2e-6, a factor 10 inside
the 2e-5 of the existing conv1x1 tests.  PARENT_ERR holds the measured figures of the fp32 core; they, the split core's
figures and the bounds are tabulated in profiles/r11_conv1x1_split_accuracy.md.  The integer cases must be bit-exact.

ROUTED: the reduce and stride-1 down-sample shapes the frozen teacher also runs on this kernel (pspnet_combine.SPLIT_REDUCE): K up
to 2048 (and 4096 for the clamp of the super-tile constants), no prologue, no residual, each at the launch-geometry class it takes
at batch 8 -- the case asks skd_conv1x1_abn_geometry and asserts that class, with M derived from the device's CU count where the
class needs half-height panels.  Truth: the float64 product and float64 eval-ABN formula on the CPU.  Bound: four times the figure of
the path these layers ran before (functional.conv1x1_bn_blas, the library GEMM with the folded BN) on the same inputs against the
same truth, and never more than ROUTED_CAP = CAP (2e-5, the standing tolerance for convolution outputs, until every case measured
within 2e-6: largest 1.55e-6 at K = 4096); those figures are the "reduce-" / "down-" / "chunk-" / "clamp-" entries of PARENT_ERR,
measured once on an MI355X by tools/conv1x1_parent_err.py and tabulated in profiles/r13_conv1x1_reduce_accuracy.md.

Every launch writes into a buffer with sentinel slack behind row M, which must stay untouched.
(The guard in FRONT of the output, and the guards around every input, are in the bounds table: tests/bounds_cases.py.)
"""
import ctypes
import zlib

import pytest
import torch

from oracle import cref
from structure_knowledge_distillation_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAP = 2e-6          # a factor 10 inside the 2e-5 of test_conv1x1_abn_gemm
RATIO = 4.0         # allowed growth over the fp32-MFMA core's own error on the same inputs
ROUTED_CAP = CAP    # every routed case measured within 2e-6 (profiles/r13_conv1x1_reduce_accuracy.md), so the tail shapes' cap holds for them too
SENTINEL = 7.0
SLACK_ROWS = 160    # more than one tile of rows behind M

# the four block-tail shapes of the batch-8 teacher (K, N, M): conv3 of layer3 / layer4 / layer2 / layer1
TAIL_SHAPES = [(256, 1024, 33800), (512, 2048, 33800), (128, 512, 33800), (64, 256, 133128)]
RAGGED_M = 2113     # 33 * 64 + 1: a last row tile with one live row

ACT_NONE, ACT_RELU = 0, 3


def _cases():
    out = []
    for k, n, m in TAIL_SHAPES:
        out.append(("real-K%d-N%d-M%d-pro-res-relu" % (k, n, m), m, k, n, True, True, ACT_RELU, "teacher"))
        for pro in (True, False):
            for res in (True, False):
                for act in (ACT_RELU, ACT_NONE):
                    name = "ragged-K%d-N%d-%s-%s-%s" % (k, n, "pro" if pro else "nopro", "res" if res else "nores",
                                                      "relu" if act == ACT_RELU else "none")
                    out.append((name, RAGGED_M, k, n, pro, res, act, "teacher"))
    out.append(("wide-range-K256-N1024", RAGGED_M, 256, 1024, False, False, ACT_NONE, "wide"))
    out.append(("wide-range-K512-N2048", RAGGED_M, 512, 2048, False, False, ACT_NONE, "wide"))
    return out


CASES = _cases()
INT_CASES = [("int-small-K256-N1024", RAGGED_M, 256, 1024, 7, 3), ("int-two-piece-K64-N256", RAGGED_M, 64, 256, 1000, 260)]

# max |hip - oracle| / max |oracle| of the fp32-MFMA core (the parent of the split core) on exactly these inputs, measured once
# on an MI355X (profiles/r11_conv1x1_split_accuracy.md)
PARENT_ERR = {
    "real-K256-N1024-M33800-pro-res-relu": 3.693e-07,
    "ragged-K256-N1024-pro-res-relu": 2.876e-07,
    "ragged-K256-N1024-pro-res-none": 3.770e-07,
    "ragged-K256-N1024-pro-nores-relu": 4.915e-07,
    "ragged-K256-N1024-pro-nores-none": 3.376e-07,
    "ragged-K256-N1024-nopro-res-relu": 2.483e-07,
    "ragged-K256-N1024-nopro-res-none": 2.825e-07,
    "ragged-K256-N1024-nopro-nores-relu": 3.936e-07,
    "ragged-K256-N1024-nopro-nores-none": 4.354e-07,
    "real-K512-N2048-M33800-pro-res-relu": 6.163e-07,
    "ragged-K512-N2048-pro-res-relu": 5.552e-07,
    "ragged-K512-N2048-pro-res-none": 8.581e-07,
    "ragged-K512-N2048-pro-nores-relu": 4.841e-07,
    "ragged-K512-N2048-pro-nores-none": 5.162e-07,
    "ragged-K512-N2048-nopro-res-relu": 5.289e-07,
    "ragged-K512-N2048-nopro-res-none": 5.520e-07,
    "ragged-K512-N2048-nopro-nores-relu": 5.157e-07,
    "ragged-K512-N2048-nopro-nores-none": 7.204e-07,
    "real-K128-N512-M33800-pro-res-relu": 3.187e-07,
    "ragged-K128-N512-pro-res-relu": 2.284e-07,
    "ragged-K128-N512-pro-res-none": 3.151e-07,
    "ragged-K128-N512-pro-nores-relu": 2.569e-07,
    "ragged-K128-N512-pro-nores-none": 2.623e-07,
    "ragged-K128-N512-nopro-res-relu": 1.628e-07,
    "ragged-K128-N512-nopro-res-none": 2.231e-07,
    "ragged-K128-N512-nopro-nores-relu": 2.882e-07,
    "ragged-K128-N512-nopro-nores-none": 2.847e-07,
    "real-K64-N256-M133128-pro-res-relu": 2.455e-07,
    "ragged-K64-N256-pro-res-relu": 1.457e-07,
    "ragged-K64-N256-pro-res-none": 1.428e-07,
    "ragged-K64-N256-pro-nores-relu": 2.215e-07,
    "ragged-K64-N256-pro-nores-none": 2.702e-07,
    "ragged-K64-N256-nopro-res-relu": 1.276e-07,
    "ragged-K64-N256-nopro-res-none": 1.371e-07,
    "ragged-K64-N256-nopro-nores-relu": 1.875e-07,
    "ragged-K64-N256-nopro-nores-none": 1.742e-07,
    "wide-range-K256-N1024": 2.815e-07,
    "wide-range-K512-N2048": 4.046e-07,
}


@pytest.fixture(scope="module")
def hip():
    return _lib.load()


@pytest.fixture(scope="module")
def ref():
    return cref.load(_lib.SIGNATURES)


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def gpu(t):
    return None if t is None else t.to(DEV)


def _identity_epilogue(n):
    """mean 0, var 1, eps 0, no affine: the epilogue returns the accumulator itself."""
    return torch.zeros(n), torch.ones(n), None, None, 0.0


def run_hip(hip, m, k, n, x, w, r, mean, var, ga, be, eps, pack_src, act):
    """The kernel's (M, N) output on the CPU; the launch writes into (M + SLACK_ROWS, N) and the rows behind M must keep the sentinel."""
    o_g = torch.full((m + SLACK_ROWS, n), SENTINEL, device=DEV)
    dx, dw, dr, dmean, dvar, dga, dbe = (gpu(t) for t in (x, w, r, mean, var, ga, be))
    args_g = (P(dx), P(dw), P(dr), P(o_g), P(dmean), P(dvar), P(dga), P(dbe), eps)
    if pack_src is None:
        assert hip.skd_conv1x1_abn_nhwc(m, k, n, *args_g, act, 0.01, None)
    else:
        pk_g = torch.empty(4, k, device=DEV)
        dp = [gpu(t) for t in pack_src]
        assert hip.skd_abn_pack_eval_params(k, P(dp[0]), P(dp[1]), P(dp[2]), P(dp[3]), 1e-5, P(pk_g), None)
        assert hip.skd_conv1x1_abn_pro_nhwc(m, k, n, *args_g, P(pk_g), act, 0.01, None)
    torch.cuda.synchronize()
    out = o_g.cpu()
    assert bool((out[m:] == SENTINEL).all()), "rows beyond M were written"
    return out[:m]


def run(hip, ref, m, k, n, x, w, r, mean, var, ga, be, eps, pack_src, act):
    """(hip output, oracle output) of one call; pack_src = (pm, pv, pw, pb) selects the prologue form."""
    o_r = torch.empty(m, n)
    args_r = (P(x), P(w), P(r), P(o_r), P(mean), P(var), P(ga), P(be), eps)
    if pack_src is None:
        assert ref.skd_conv1x1_abn_nhwc(m, k, n, *args_r, act, 0.01, None)
    else:
        pm, pv, pw, pb = pack_src
        pk_r = torch.empty(4, k)
        assert ref.skd_abn_pack_eval_params(k, P(pm), P(pv), P(pw), P(pb), 1e-5, P(pk_r), None)
        assert ref.skd_conv1x1_abn_pro_nhwc(m, k, n, *args_r, P(pk_r), act, 0.01, None)
    return run_hip(hip, m, k, n, x, w, r, mean, var, ga, be, eps, pack_src, act), o_r


def case_outputs(hip, ref, case):
    name, m, k, n, pro, res, act, data = case
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    pack_src = None
    if data == "teacher":
        # activations of order 1 with per-channel offsets, weights of order 0.05 (the teacher's scales)
        w = torch.randn(n, k, generator=g) * 0.05
        if pro:    # x is the raw 3x3-convolution output, bn2 + ReLU bring it to order 1
            x = torch.randn(m, k, generator=g) * 2 + torch.randn(1, k, generator=g)
            pack_src = (torch.randn(k, generator=g) * 0.5, torch.rand(k, generator=g) * 4 + 2,
                        torch.randn(k, generator=g), torch.randn(k, generator=g) * 0.5)
        else:      # x is an activated map: non-negative, offset per channel
            x = torch.relu(torch.randn(m, k, generator=g) + torch.randn(1, k, generator=g) * 0.5)
        r = torch.relu(torch.randn(m, n, generator=g)) if res else None
        mean, var = torch.randn(n, generator=g) * 0.3, torch.rand(n, generator=g) + 0.5
        ga, be, eps = torch.randn(n, generator=g), torch.randn(n, generator=g), 1e-5
    else:          # magnitudes 2^-20 ... 2^20 on both operands, identity epilogue: the bare product
        ex = torch.randint(-20, 21, (m, k), generator=g).float()
        ew = torch.randint(-20, 21, (n, k), generator=g).float()
        x, w = torch.randn(m, k, generator=g) * torch.exp2(ex), torch.randn(n, k, generator=g) * torch.exp2(ew)
        r = None
        mean, var, ga, be, eps = _identity_epilogue(n)
    return run(hip, ref, m, k, n, x, w, r, mean, var, ga, be, eps, pack_src, act)


def case_error(hip, ref, case):
    got, want = case_outputs(hip, ref, case)
    got, want = got.double(), want.double()
    assert bool(torch.isfinite(got).all())
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-30)


def int_case_outputs(hip, ref, case):
    name, m, k, n, xmax, wmax = case
    assert k * xmax * wmax < 2 ** 24       # every partial sum is an exact fp32 integer, in any order
    g = torch.Generator().manual_seed(77 + k)
    x = torch.randint(-xmax, xmax + 1, (m, k), generator=g).float()
    w = torch.randint(-wmax, wmax + 1, (n, k), generator=g).float()
    mean, var, ga, be, eps = _identity_epilogue(n)
    return run(hip, ref, m, k, n, x, w, None, mean, var, ga, be, eps, None, ACT_NONE)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_split_core_vs_oracle(hip, ref, case):
    err = case_error(hip, ref, case)
    bound = min(RATIO * PARENT_ERR[case[0]], CAP)
    print("%s: err %.3e  fp32 core %.3e  bound %.3e" % (case[0], err, PARENT_ERR[case[0]], bound))
    assert err <= bound, "%s: max err %.3e > %.3e (fp32-MFMA core: %.3e)" % (case[0], err, bound, PARENT_ERR[case[0]])


@pytest.mark.parametrize("case", INT_CASES, ids=[c[0] for c in INT_CASES])
def test_split_core_integers_bit_exact(hip, ref, case):
    got, want = int_case_outputs(hip, ref, case)
    assert float(want.abs().max()) > 100.0
    assert torch.equal(got, want), "%s: %d of %d outputs differ" % (case[0], int((got != want).sum()), got.numel())


# ---- the routed reduce / down-sample shapes ------------------------------------------------------------------------------------

HH = None      # M derived from the device: whole rounds of full-height panels + 65 rows (see routed_m)
# (name, K, N, activation, M, class): class = what skd_conv1x1_abn_geometry must report for the case on this device --
# nt / ct / pm, "half" (half-height panels present), "padded" (the last panel group of an XCD holds padding workgroups)
ROUTED = [
    ("reduce-K512-N256", 512, 256, ACT_RELU, RAGGED_M, dict(nt=0, ct=2, pm=1, half=False)),
    ("reduce-K1024-N256", 1024, 256, ACT_RELU, RAGGED_M, dict(nt=0, ct=2, pm=1, half=False)),
    ("reduce-K2048-N512", 2048, 512, ACT_RELU, RAGGED_M, dict(nt=1, ct=1, pm=2, half=False, padded=True)),
    ("reduce-K2048-N512-hh", 2048, 512, ACT_RELU, HH, dict(nt=1, ct=1, pm=2, half=True)),
    ("reduce-K1024-N512-hh", 1024, 512, ACT_RELU, HH, dict(nt=1, ct=2, pm=4, half=True)),
    ("down-K1024-N2048-hh", 1024, 2048, ACT_NONE, HH, dict(nt=1, ct=2, pm=4, half=True)),
    ("down-K512-N1024-hh", 512, 1024, ACT_NONE, HH, dict(nt=1, ct=4, pm=8, half=True)),
    ("reduce-K256-N128-hh", 256, 128, ACT_RELU, HH, dict(nt=0, ct=1, pm=1, half=True)),
    ("down-K128-N256-hh", 128, 256, ACT_NONE, HH, dict(nt=0, ct=2, pm=1, half=True)),
    ("chunk-shrink-K512-N1152", 512, 1152, ACT_NONE, RAGGED_M, dict(nt=1, ct=3, pm=8, half=False)),     # tiles_n = 9: ct 4 -> 3
    ("clamp-K4096-N256", 4096, 256, ACT_NONE, RAGGED_M, dict(nt=1, ct=1, pm=1, half=False)),          # ct = pm = 1 by the clamp
]
ROUTED_CASE = {c[0]: c for c in ROUTED}
ROUTED_INT = [("int-K2048-N512", 2048, 512, RAGGED_M, dict(nt=1, ct=1, pm=2, half=False)),
              ("int-K1024-N2048-hh", 1024, 2048, HH, dict(nt=1, ct=2, pm=4, half=True))]

# max |parent - want| / max |want| of functional.conv1x1_bn_blas on exactly these inputs, measured once on an MI355X (256 compute
# units: the derived M are 24641, 24641, 6209, 12353, 98369, 49217); profiles/r13_conv1x1_reduce_accuracy.md
PARENT_ERR.update({
    "reduce-K512-N256": 5.978e-07,
    "reduce-K1024-N256": 7.272e-07,
    "reduce-K2048-N512": 1.078e-06,
    "reduce-K2048-N512-hh": 1.262e-06,
    "reduce-K1024-N512-hh": 9.750e-07,
    "down-K1024-N2048-hh": 9.019e-07,
    "down-K512-N1024-hh": 5.756e-07,
    "reduce-K256-N128-hh": 4.635e-07,
    "down-K128-N256-hh": 3.143e-07,
    "chunk-shrink-K512-N1152": 4.550e-07,
    "clamp-K4096-N256": 1.403e-06,
})


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def routed_m(n, m):
    """M of a case: as listed, or -- half-height cases -- the rows that 3 workgroups per compute unit cover in one round of
    full-height tiles, plus one whole 64-row half panel, plus one half panel with a single live row."""
    return m if m is not HH else (3 * cu_count() // (n // 128)) * 128 + 65


def assert_geometry(hip, m, k, n, want):
    """The launch-geometry class of the (M, K, N) problem on this device is the one the case means to exercise."""
    out = (ctypes.c_int64 * 7)()
    assert hip.skd_conv1x1_abn_geometry(m, k, n, cu_count(), ctypes.cast(out, ctypes.c_void_p)) == 1
    tiles_n, ct, pm, p_full, panels, grid, nt = (int(v) for v in out)
    what = "M %d K %d N %d on %d CUs: tiles_n %d ct %d pm %d p_full %d panels %d grid %d nt %d" % (
        m, k, n, cu_count(), tiles_n, ct, pm, p_full, panels, grid, nt)
    assert (nt, ct, pm) == (want["nt"], want["ct"], want["pm"]), what
    assert nt == (ct < tiles_n), what
    if want["half"]:      # full-height panels, then at least one whole half-height panel and a ragged one
        assert p_full > 0 and panels >= p_full + 2 and (m - p_full * 128) % 64 == 1, what
    else:
        assert panels == p_full, what
    if want.get("padded"):
        assert grid > -(-panels // 8) * 8 * tiles_n, what
    return what


def routed_inputs(name, m, k, n):
    """The "teacher" recipe of case_outputs without prologue or residual, seeded from the case name."""
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    w = torch.randn(n, k, generator=g) * 0.05
    x = torch.relu(torch.randn(m, k, generator=g) + torch.randn(1, k, generator=g) * 0.5)
    mean, var = torch.randn(n, generator=g) * 0.3, torch.rand(n, generator=g) + 0.5
    ga, be, eps = torch.randn(n, generator=g), torch.randn(n, generator=g), 1e-5
    return x, w, (mean, var, ga, be, eps)


def routed_want(x, w, bn, act):
    """float64 on the CPU: the product, then the eval-mode InPlace-ABN formula and the activation."""
    mean, var, ga, be, eps = bn
    y = x.double() @ w.double().t()
    y = (y - mean.double()) / torch.sqrt(var.double() + eps) * (ga.double().abs() + eps) + be.double()
    return torch.relu(y) if act == ACT_RELU else y


def rel_err(got, want):
    got = got.double()
    assert bool(torch.isfinite(got).all())
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-30)


def routed_case_error(hip, name):
    """(error figure of the kernel, geometry text, inputs, truth) of a ROUTED case; asserts the case's geometry class first."""
    _, k, n, act, m, cls = ROUTED_CASE[name]
    m = routed_m(n, m)
    what = assert_geometry(hip, m, k, n, cls)
    x, w, bn = routed_inputs(name, m, k, n)
    want = routed_want(x, w, bn, act)
    got = run_hip(hip, m, k, n, x, w, None, *bn, None, act)
    return rel_err(got, want), what, (x, w, bn), want


@pytest.mark.parametrize("name", [c[0] for c in ROUTED])
def test_routed_shapes_vs_float64(hip, name):
    err, what, _, _ = routed_case_error(hip, name)
    parent = PARENT_ERR[name]
    bound = min(RATIO * parent, ROUTED_CAP)
    print("%s: err %.3e  parent %.3e  bound %.3e  (%.2f of 2e-6)  %s" % (name, err, parent, bound, err / CAP, what))
    assert err <= bound, "%s: max err %.3e > %.3e (library GEMM: %.3e)" % (name, err, bound, parent)


@pytest.mark.parametrize("case", ROUTED_INT, ids=[c[0] for c in ROUTED_INT])
def test_routed_integers_bit_exact(hip, case):
    name, k, n, m, cls = case
    m = routed_m(n, m)
    assert_geometry(hip, m, k, n, cls)
    assert k * 7 * 3 < 2 ** 24             # every partial sum is an exact fp32 integer, in any order
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    x = torch.randint(-7, 8, (m, k), generator=g).float()
    w = torch.randint(-3, 4, (n, k), generator=g).float()
    got = run_hip(hip, m, k, n, x, w, None, *_identity_epilogue(n), None, ACT_NONE)
    want = x.double() @ w.double().t()
    assert float(want.abs().max()) > 100.0
    assert torch.equal(got.double(), want), "%s: %d of %d outputs differ" % (name, int((got.double() != want).sum()), got.numel())
