"""The float64 MODEL of the two-piece mode of include/skd_split2.h (CPU only; helper of tests/test_split2_cpu.py,
tests/test_split2_gpu.py and tools/split2_emulation.py).

An fp32 operand a is cut into bf16 pieces p0 = bf16(a), p1 = bf16(a - p0), ... (round to nearest even, through torch's bfloat16
cast; the residuals are exact in fp32).  The two-piece mode keeps the three products a0 b0 + a0 b1 + a1 b0; here they are
accumulated in float64, and the epilogue follows in float64.  The truncation -- the dropped a1 b1 and the dropped second
residuals -- is BY DESIGN: this model, not the exact product, is the reference of the mode.  What separates a kernel from it is
fp32 accumulation and the fp32 epilogue.
"""
import torch
import torch.nn.functional as F


def pieces(t, n):
    """The first ``n`` bf16 pieces of the fp32 tensor ``t`` (fp32 is taken first of anything wider), as float64 tensors."""
    rest = t.float()
    out = []
    for _ in range(n):
        p = rest.bfloat16().float()
        out.append(p.double())
        rest = rest - p           # exact in fp32: p agrees with rest in its leading 8 bits
    return out


def _pairs(n):
    """(i, j) of the products a_i b_j the n-piece core keeps: i + j <= n - 1 (n = 2: a0 b0, a0 b1, a1 b0; n = 3: the six)."""
    return [(i, j) for i in range(n) for j in range(n) if i + j <= n - 1]


def mm_split2(a, b, n=2):
    """a (M, K) . b (N, K)^T by the n-piece model, float64."""
    pa, pb = pieces(a, n), pieces(b, n)
    return sum(pa[i] @ pb[j].t() for i, j in _pairs(n))


def conv2d_split2(x, w, bias=None, stride=1, padding=0, dilation=1, n=2):
    """F.conv2d(x, w, bias, ...) by the n-piece model, float64 (bias added in float64)."""
    px, pw = pieces(x, n), pieces(w, n)
    y = None
    for i in range(n):            # by linearity: a_i . (sum of the b_j kept beside it)
        t = F.conv2d(px[i], sum(pw[j] for j in range(n - i)), None, stride, padding, dilation)
        y = t if y is None else y + t
    return y if bias is None else y + bias.double().view(1, -1, 1, 1)


def prologue_fp32(x, ppack):
    """relu(fma((x - mean) * invstd, gamma, beta)) as csrc/conv1x1.hip's prologue computes it in fp32, for x (M, K) fp32 and
    ppack (4, K) = mean | invstd | gamma | beta as skd_abn_pack_eval_params wrote it.  The multiply-add is fused: evaluated in
    float64 (the product of two fp32 values is exact there) and rounded once."""
    t = ((x.float() - ppack[0]) * ppack[1]).double()
    z = (t * ppack[2].double() + ppack[3].double()).float()
    return torch.relu(z)


def abn_eval64(y, mean, var, gamma, beta, eps, act, slope=0.01, channel_dim=1):
    """The eval-mode InPlace-ABN formula and the activation in float64: ((y - mean) / sqrt(var + eps)) * (|gamma| + eps) + beta."""
    shape = [1] * y.dim()
    shape[channel_dim] = -1
    v = lambda t: t.double().view(shape)
    if mean is not None:
        y = (y - v(mean)) / torch.sqrt(v(var) + eps)
        y = y * (v(gamma).abs() + eps if gamma is not None else 1.0) + (v(beta) if beta is not None else 0.0)
    if act == "relu":
        y = torch.relu(y)
    if act == "leaky_relu":
        y = torch.where(y < 0, y * slope, y)
    return y


def rel_err(got, want):
    """max |got - want| / max |want|: the error figure of the project's convolution tests."""
    got = got.double()
    assert bool(torch.isfinite(got).all())
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-30)


# ---- the small teacher forward of the network test and of tools/split2_emulation.py ------------------------------------------

TEACHER_SEED = 5          # chosen on the CPU: the float64 and the fp32 forwards agree on every argmax (tools/split2_emulation.py)
TEACHER_HW = 129


def teacher_case(seed=TEACHER_SEED, hw=TEACHER_HW):
    """(P, x): an fp32 ResNet101-plan state dict -- oracle.step_torch.pspnet_init weights, running variance uniform in
    [0.1, 0.6], running mean of sigma 0.05 -- and a (1, 3, hw, hw) fp32 input."""
    from oracle import step_torch as O
    P = O.pspnet_init(O.TEACHER, 19, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    for k in sorted(P):
        if k.endswith("running_var"):
            P[k] = torch.rand(P[k].shape, generator=g) * 0.5 + 0.1
        elif k.endswith("running_mean"):
            P[k] = torch.randn(P[k].shape, generator=g) * 0.05
    x, _ = O.synthetic_batch(1, hw, hw, seed=seed)
    return P, x.float()


def teacher_forward64(P, x, conv2d=None):
    """oracle.step_torch.pspnet_forward in float64, eval mode: (logits, dsn, PSP feature).  ``conv2d``: a replacement for
    ``F.conv2d`` inside that forward (the emulation's hook); the oracle's file is not touched."""
    from oracle import step_torch as O
    P64 = {k: v.double() for k, v in P.items()}
    saved = O.F
    if conv2d is not None:
        class _Shim:
            def __getattr__(self, name):
                return getattr(saved, name)
        shim = _Shim()
        shim.conv2d = conv2d
        O.F = shim
    try:
        with torch.no_grad():
            out = O.pspnet_forward(P64, x.double(), O.TEACHER, False)
    finally:
        O.F = saved
    return out[0], out[1], out[2]


def teacher_forward32(P, x):
    """The same forward in fp32 on the CPU: (logits, dsn, PSP feature)."""
    from oracle import step_torch as O
    with torch.no_grad():
        return tuple(O.pspnet_forward(P, x, O.TEACHER, False)[:3])


def split_core_conv2d(n):
    """An ``F.conv2d`` for teacher_forward64 that runs the convolutions the frozen teacher has on the split core today through
    the n-piece model and everything else exactly: the stride-1 1x1 GEMMs on maps (Cin % 16 == 0, Cout % 128 == 0, not 512 -> 128;
    the pyramid's pooled 1x1 stages are library products), the stride-1 3x3 convolutions with Cin >= 256 (layer3 / layer4 conv2,
    dsn[0]) and the feature-map half of the PSP bottleneck (the last 2048 of its 4096 input channels)."""
    def conv2d(x, w, bias=None, stride=1, padding=0, dilation=1, groups=1):
        s = stride if isinstance(stride, int) else stride[0]
        cout, cin, k = w.shape[0], w.shape[1], w.shape[2]
        routed = s == 1 and groups == 1 and cin % 16 == 0 and cout % 128 == 0
        if routed and k == 1 and min(x.shape[2:]) > 6 and (cin, cout) != (512, 128):
            return conv2d_split2(x, w, bias, 1, 0, 1, n)
        if routed and k == 3 and cin >= 256:
            if cin == 4096:       # the PSP bottleneck: the priors' channels through the fold (exact here), the feature half routed
                return (F.conv2d(x[:, :2048], w[:, :2048], None, 1, padding, dilation)
                        + conv2d_split2(x[:, 2048:], w[:, 2048:], bias, 1, padding, dilation, n))
            return conv2d_split2(x, w, bias, 1, padding, dilation, n)
        return F.conv2d(x, w, bias, stride, padding, dilation, groups)
    return conv2d
