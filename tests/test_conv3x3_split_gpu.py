"""-m gpu: the implicit-GEMM 3x3 convolution of csrc/conv3x3.hip (fp32 operands as three bf16 pieces on the bf16 MFMA,
weights split once) against ``F.conv2d`` in float64 on the CPU.

Error figure of a case: max |hip - want| / max |want| over the whole output (the ``close()`` form of tests/test_kernels_gpu.py).
Bound of a case: FOUR times the figure the parent path -- MIOpen's fp32 ``F.conv2d`` on the GPU, followed by the library's
eval-mode ABN pass where the case has an epilogue -- gave on the same inputs, and never more than 2e-5, the project's standing
tolerance for convolution outputs.  PARENT_ERR holds those figures, measured once on an MI355X; they and the kernel's own
figures are tabulated in profiles/r12_conv3x3_split_accuracy.md.  The factor 4 is the one the 1x1 core was accepted under
(tests/test_conv1x1_split_gpu.py).  The integer cases must be bit-exact.  Every launch writes into a buffer with sentinel
slack behind row M, which must stay untouched.
(The guard in FRONT of the output, and the guards around the input, the weights and the pack, are in the bounds table: tests/bounds_cases.py.)
"""
import ctypes
import zlib

import pytest
import torch
import torch.nn.functional as F

from structure_knowledge_distillation_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAP = 2e-5
RATIO = 4.0
SENTINEL = 7.0
SLACK_ROWS = 160          # more than one tile of rows behind M
ACT = {"none": 0, "leaky_relu": 1, "relu": 3}

# (name, B, Cin, Cout, H, W, dilation, epilogue)
CASES = [
    ("ragged-13x11-d1", 2, 32, 128, 13, 11, 1, "identity"),
    ("ragged-13x11-d2", 2, 32, 128, 13, 11, 2, "identity"),
    ("ragged-13x11-d4", 2, 32, 128, 13, 11, 4, "identity"),
    ("centre-5x5-d4", 1, 32, 128, 5, 5, 4, "identity"),
    ("centre-3x3-d4", 1, 32, 128, 3, 3, 4, "identity"),
    ("longk-512-512-9x9-d4", 1, 512, 512, 9, 9, 4, "identity"),
    ("many-tiles-226x226-d1", 2, 16, 128, 226, 226, 1, "identity"),
    ("ragged-13x11-d2-bias-abn-leaky", 2, 32, 128, 13, 11, 2, "bias-abn-leaky"),
    ("ragged-13x11-d2-bn-relu", 2, 32, 128, 13, 11, 2, "bn-relu"),
]
CASE = {c[0]: c for c in CASES}

# max |parent - want| / max |want| of the parent path on exactly these inputs, measured once on an MI355X
# (profiles/r12_conv3x3_split_accuracy.md; tools/conv3x3_parent_err.py measures them again on these inputs)
PARENT_ERR = {
    "ragged-13x11-d1": 4.513e-07,
    "ragged-13x11-d2": 3.589e-07,
    "ragged-13x11-d4": 3.746e-07,
    "centre-5x5-d4": 2.858e-07,
    "centre-3x3-d4": 8.849e-08,
    "longk-512-512-9x9-d4": 2.510e-07,
    "many-tiles-226x226-d1": 4.576e-07,
    "ragged-13x11-d2-bias-abn-leaky": 3.015e-07,
    "ragged-13x11-d2-bn-relu": 3.346e-07,
}


@pytest.fixture(scope="module")
def hip():
    return _lib.load()


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def case_inputs(name):
    """Seeded inputs of a case: ReLU-like activations with per-channel offsets, He-scaled weights, epilogue parameters."""
    _, b, cin, cout, h, w, d, epi = CASE[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    x = torch.relu(torch.randn(b, cin, h, w, generator=g) + torch.randn(1, cin, 1, 1, generator=g) * 0.5)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    p = {"cbias": None, "mean": None, "var": None, "gamma": None, "beta": None, "eps": 0.0, "act": "none"}
    if epi != "identity":
        p.update(mean=torch.randn(cout, generator=g) * 0.3, var=torch.rand(cout, generator=g) + 0.5,
                 gamma=torch.randn(cout, generator=g), beta=torch.randn(cout, generator=g), eps=1e-5)
        if epi == "bias-abn-leaky":
            p.update(cbias=torch.randn(cout, generator=g) * 0.2, act="leaky_relu")
        else:
            p.update(act="relu")
    return x.contiguous(memory_format=torch.channels_last), wt, p


def epilogue64(y, p):
    """The eval-mode InPlace-ABN formula (+ activation, slope 0.01) in float64 on an (B, C, H, W) tensor."""
    if p["mean"] is not None:
        v = lambda t: t.double().view(1, -1, 1, 1)
        y = (y - v(p["mean"])) / torch.sqrt(v(p["var"]) + p["eps"]) * (v(p["gamma"]).abs() + p["eps"]) + v(p["beta"])
    if p["act"] == "relu":
        y = torch.relu(y)
    if p["act"] == "leaky_relu":
        y = torch.where(y < 0, y * 0.01, y)
    return y


_WANT = {}


def want_of(name):
    """float64 truth of a case on the CPU, computed once and shared (never modified)."""
    if name not in _WANT:
        x, wt, p = case_inputs(name)
        d = CASE[name][6]
        y = F.conv2d(x.double(), wt.double(), None if p["cbias"] is None else p["cbias"].double(), 1, d, d)
        _WANT[name] = epilogue64(y, p)
    return _WANT[name]


def pack(hip, wt_dev):
    cout, cin = wt_dev.shape[:2]
    nbytes = hip.skd_conv3x3_split_pack_bytes(cin, cout)
    assert nbytes == cout * cin * 9 * 6
    buf = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    sn, sc, sy, sx = wt_dev.stride()
    assert hip.skd_conv3x3_split_pack_weights(cin, cout, P(wt_dev), sn, sc, sy, sx, P(buf), nbytes, None)
    return buf


def run_hip(hip, x, wt, p, d, geometry=0, wt_format=torch.contiguous_format):
    """(B, Cout, H, W) output on the CPU + the pack; checks the sentinel slack behind row M."""
    b, cin, h, w = x.shape
    cout = wt.shape[0]
    m = b * h * w
    dx = x.to(DEV).contiguous(memory_format=torch.channels_last)
    dw = wt.to(DEV).contiguous(memory_format=wt_format)
    pk = pack(hip, dw)
    out = torch.full((m + SLACK_ROWS, cout), SENTINEL, device=DEV)
    dp = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in p.items()}
    assert hip.skd_conv3x3_split_nhwc(b, h, w, cin, cout, d, P(dx), P(pk), P(out), P(dp["cbias"]), P(dp["mean"]), P(dp["var"]),
                                      P(dp["gamma"]), P(dp["beta"]), p["eps"], ACT[p["act"]], 0.01, geometry, None)
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool((out[m:] == SENTINEL).all()), "rows beyond M were written"
    return out[:m].view(b, h, w, cout).permute(0, 3, 1, 2), pk


def rel_err(got, want):
    got = got.double()
    assert bool(torch.isfinite(got).all())
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-30)


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_split_conv3x3_vs_float64(hip, name):
    x, wt, p = case_inputs(name)
    got, _ = run_hip(hip, x, wt, p, CASE[name][6])
    err = rel_err(got, want_of(name))
    bound = min(RATIO * PARENT_ERR[name], CAP)
    print("%s: err %.3e  parent %.3e  bound %.3e" % (name, err, PARENT_ERR[name], bound))
    assert err <= bound, "%s: max err %.3e > %.3e (parent path: %.3e)" % (name, err, bound, PARENT_ERR[name])


@pytest.mark.parametrize("geometry", [1, 2, 3])
def test_every_geometry_gives_the_same_bits(hip, geometry):
    """Tile height changes which workgroup computes a row, never the order of a row's sum."""
    name = "many-tiles-226x226-d1"
    x, wt, p = case_inputs(name)
    base, _ = run_hip(hip, x, wt, p, 1)
    got, _ = run_hip(hip, x, wt, p, 1, geometry=geometry)
    assert torch.equal(got, base)
    name = "ragged-13x11-d2"
    x, wt, p = case_inputs(name)
    base, _ = run_hip(hip, x, wt, p, 2)
    got, _ = run_hip(hip, x, wt, p, 2, geometry=geometry)
    assert torch.equal(got, base)


def test_weight_memory_format_does_not_matter(hip):
    name = "ragged-13x11-d1"
    x, wt, p = case_inputs(name)
    a, pk_a = run_hip(hip, x, wt, p, 1, wt_format=torch.contiguous_format)
    b, pk_b = run_hip(hip, x, wt, p, 1, wt_format=torch.channels_last)
    assert torch.equal(pk_a, pk_b)
    assert torch.equal(a, b)


@pytest.mark.parametrize("shape", [(2, 13, 11, 2), (1, 5, 5, 4), (2, 40, 37, 1)], ids=["13x11-d2", "5x5-d4", "40x37-d1"])
def test_integers_bit_exact(hip, shape):
    b, h, w, d = shape
    cin, cout = 32, 128
    assert 9 * cin * 7 * 3 < 2 ** 24       # every partial sum is an exact fp32 integer, in any order
    g = torch.Generator().manual_seed(100 * h + d)
    x = torch.randint(-7, 8, (b, cin, h, w), generator=g).float().contiguous(memory_format=torch.channels_last)
    wt = torch.randint(-3, 4, (cout, cin, 3, 3), generator=g).float()
    p = {"cbias": None, "mean": None, "var": None, "gamma": None, "beta": None, "eps": 0.0, "act": "none"}
    got, _ = run_hip(hip, x, wt, p, d)
    want = F.conv2d(x.double(), wt.double(), None, 1, d, d)
    assert float(want.abs().max()) > 100.0
    assert torch.equal(got.double(), want), "%d of %d outputs differ" % (int((got.double() != want).sum()), got.numel())


def test_functional_path_matches_the_entry(hip):
    """functional.conv3x3_split_eval through a module, its cached pack and a bias + ABN epilogue == the direct call."""
    from structure_knowledge_distillation_amd import functional as SF
    from structure_knowledge_distillation_amd.libs import InPlaceABNSync
    name = "ragged-13x11-d2-bias-abn-leaky"
    x, wt, p = case_inputs(name)
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
    assert not SF.conv3x3_split_supported(dx, conv)                  # grad enabled
    with torch.no_grad():
        assert SF.conv3x3_split_supported(dx, conv)
        assert not SF.conv3x3_split_supported(dx.contiguous(), conv)  # NCHW
        pk = SF.conv3x3_pack_weights(conv)
        assert SF.conv3x3_pack_weights(conv) is pk
        got = SF.conv3x3_split_eval(dx, pk, 128, 2, conv.bias, bn, bn.activation)
    want, _ = run_hip(hip, x, wt, p, 2)
    assert got.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(got.cpu(), want)


def test_fused_sgd_step_rebuilds_the_eval_pack():
    """torch's fused SGD writes the weight without advancing ``_version``, the key of the pack; with the step post-hook NetModel
    registers, the pack fetched behind a step is that of the new weight."""
    from structure_knowledge_distillation_amd import functional as SF
    from structure_knowledge_distillation_amd.networks.kd_model import advance_versions_after_step
    torch.manual_seed(21)
    conv = torch.nn.Conv2d(16, 128, 3, 1, 1).to(DEV)
    x = torch.randn(1, 16, 5, 7, device=DEV).contiguous(memory_format=torch.channels_last)
    opt = torch.optim.SGD(conv.parameters(), 0.5, fused=True)
    opt.register_step_post_hook(advance_versions_after_step)
    with torch.no_grad():
        before = SF.conv3x3_split_eval(x, SF.conv3x3_pack_weights(conv), 128, 1, conv.bias)
    for p in conv.parameters():
        p.grad = torch.ones_like(p)
    version = conv.weight._version
    opt.step()
    assert conv.weight._version > version
    with torch.no_grad():
        got = SF.conv3x3_split_eval(x, SF.conv3x3_pack_weights(conv), 128, 1, conv.bias)
        fresh = SF.conv3x3_pack_weights(None, conv.weight.detach().clone(), torch.nn.Module())
        want = SF.conv3x3_split_eval(x, fresh, 128, 1, conv.bias)
    assert torch.equal(got, want) and not torch.equal(got, before)


def test_host_refusals(hip):
    """Refused on the host, before any launch."""
    sup = hip.skd_conv3x3_split_supported
    assert sup(32, 128, 1, 2, 2, 1)
    assert not sup(24, 128, 1, 1, 1, 1)      # Cin not a multiple of 16
    assert not sup(32, 64, 1, 1, 1, 1)       # Cout not a multiple of the column tile
    assert not sup(32, 128, 2, 1, 1, 1)      # stride 2
    assert not sup(32, 128, 1, 1, 2, 1)      # padding != dilation
    assert not sup(32, 128, 1, 2, 2, 2)      # groups
    assert hip.skd_conv3x3_split_pack_bytes(24, 128) == 0
    x = torch.zeros(1, 4, 4, 32, device=DEV)
    wt = torch.zeros(128, 32, 3, 3, device=DEV)
    pk = pack(hip, wt)
    out = torch.full((16, 128), SENTINEL, device=DEV)
    call = lambda cin, cout, d, px, ppk, pout: hip.skd_conv3x3_split_nhwc(1, 4, 4, cin, cout, d, px, ppk, pout, None, None, None, None,
                                                                          None, 0.0, 0, 0.01, 0, None)
    assert not call(32, 128, 1, None, P(pk), P(out))                  # a missing pointer
    assert not call(32, 128, 1, P(x), None, P(out))
    assert not call(32, 128, 1, P(x), P(pk), None)
    assert not call(24, 128, 1, P(x), P(pk), P(out))
    assert not call(32, 64, 1, P(x), P(pk), P(out))
    assert not call(32, 128, 0, P(x), P(pk), P(out))
    assert not call(32, 128, 1, ctypes.c_void_p(x.data_ptr() + 4), P(pk), P(out))     # misaligned
    assert not hip.skd_conv3x3_split_pack_weights(32, 128, P(wt), 288, 9, 3, 1, P(pk), pk.numel() - 1, None)   # pack too small
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
