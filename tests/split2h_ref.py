"""The float64 MODEL of the fp16 two-piece mode of include/skd_split2h.h (CPU only; helper of tests/test_split2h_cpu.py and
tests/test_split2h_gpu.py).

An fp32 operand a is cut into two FP16 pieces, round to nearest even through torch's float16 cast (subnormals kept):
    a0 = fp16(a),   a1 = fp16((a - a0) * 2^11)        the residual and its scaling are exact in fp32,
so a ~ a0 + 2^-11 a1 with 22 significant bits.  The mode keeps the three products hi = a0 b0 and lo = a0 b1 + a1 b0 and returns
hi + 2^-11 lo; here they are accumulated in float64 (exact for the operands of the tests: products of two 11-bit values, sums far
below 2^53 of their unit) and the epilogue (split2_ref.abn_eval64) follows in float64.  What is dropped -- a1 b1 and what two pieces
leave of an operand -- is BY DESIGN: this model, not the exact product, is the reference of the mode.
``scaled=False`` is the same split WITHOUT the residual scaling (a1 = fp16(a - a0), out = hi + lo): the form the mode does not use,
kept to pin why the scaling exists.  ``flush=True`` zeroes fp16-subnormal pieces (a hardware that flushed them; the MI355X does not).
"""
import torch
import torch.nn.functional as F

from split2_ref import abn_eval64, prologue_fp32, rel_err  # noqa: F401  (re-exported: the epilogue and the error figure are shared)

SCALE = 2048.0          # 2^11
F16_MIN_NORMAL = 2.0 ** -14


def pieces(t, scaled=True, flush=False):
    """(p0, p1) of the fp32 tensor ``t`` as float64 tensors: t ~ p0 + p1 / SCALE (scaled) or p0 + p1."""
    v = t.float()
    p0 = v.half().float()                       # |v| >= 65520 rounds to +-inf, as v_cvt_pk_f16_f32 does
    r = v - p0                                  # exact in fp32
    p1 = ((r * SCALE) if scaled else r).half().float()
    if flush:
        p0 = torch.where(p0.abs() < F16_MIN_NORMAL, torch.zeros_like(p0), p0)
        p1 = torch.where(p1.abs() < F16_MIN_NORMAL, torch.zeros_like(p1), p1)
    return p0.double(), p1.double()


def join(hi, lo, scaled=True):
    return hi + lo / SCALE if scaled else hi + lo


def mm_split2h(a, b, scaled=True, flush=False):
    """a (M, K) . b (N, K)^T by the model, float64."""
    a0, a1 = pieces(a, scaled, flush)
    b0, b1 = pieces(b, scaled, flush)
    return join(a0 @ b0.t(), a0 @ b1.t() + a1 @ b0.t(), scaled)


def conv2d_split2h(x, w, bias=None, padding=0, dilation=1, scaled=True, flush=False):
    """F.conv2d(x, w, bias, 1, padding, dilation) by the model, float64 (bias added in float64)."""
    x0, x1 = pieces(x, scaled, flush)
    w0, w1 = pieces(w, scaled, flush)
    conv = lambda a, b: F.conv2d(a, b, None, 1, padding, dilation)
    y = join(conv(x0, w0), conv(x0, w1) + conv(x1, w0), scaled)
    return y if bias is None else y + bias.double().view(1, -1, 1, 1)


def fp32_chain(a, b):
    """a (M, K) . b (N, K)^T as an fp32 multiply-add chain over k in order (round to nearest after every step): the error an
    fp32 accumulation over the same K makes, the yardstick of the issue's table."""
    acc = torch.zeros(a.shape[0], b.shape[0], dtype=torch.float32)
    a, b = a.float(), b.float()
    for k in range(a.shape[1]):
        acc = (acc.double() + a[:, k:k + 1].double() * b[:, k].double()).float()      # an fma: one rounding per step
    return acc


def input_classes(m=64, k=576, n=32, seed=0):
    """The input classes of DESIGN.md 7.15's table at a size a CPU test affords: name -> (activations (m, k), weights (n, k))."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, k, generator=g) * 0.02
    base = torch.relu(torch.randn(m, k, generator=g))
    cols = torch.exp(torch.linspace(-12.0, 5.0, k))
    return {
        "relu N(0,1)": (base, w),
        "x30": (base * 30.0, w),
        "x1e-3": (base * 1e-3, w),
        "columns e^-12..e^5": (base * cols, w),
        "x1000, weights 1e-4": (base * 1000.0, torch.randn(n, k, generator=g) * 1e-4),
        "x1e-5": (base * 1e-5, w),
    }
