"""The float64 MODEL of the fp16 two-piece TRAINING mode of include/skd_train2h.h and the integer cases of its two gradient
products (CPU only; helper of tests/test_train2h_cpu.py, which proves what each case claims, and tests/test_train2h_gpu.py, which
launches them).  Built on tests/split2h_ref.py (the pieces, the join) and tests/split_exact.py (the bilinear maps), neither edited.

New beside split2h_ref is the SCALE WORD of a gradient tensor g and the power of two it selects:
    word = max(bits(g) & 0x7fffffff);   s = 1 for word == 0 or word >= 0x7f800000, otherwise 2^clamp(14 - e, -126, 126) with
    e = (word >> 23) - 127.
The scaled product is  split2h(g s, b) (1 / s):  g s in fp32 (exact), the three kept piece products in float64, the join, one
multiplication by 1 / s.

Integer cases (in the manner of tests/train2_cases.py; the values are those of tests/test_split2h_gpu.py's exact classes):
    W  wide     1 + 2^-21 k, k in [0, 2^21), signed: 22 significant bits, TWO fp16 pieces, nothing dropped
    N  narrow   +-1, +-2: ONE piece
    WN, NW      one operand of each class, the sparse side leaving at most two products per output: every piece product and
                every partial sum is exact in fp32 and so is the joined result (24 bits), so the kernel must give the exact
                product bit for bit.  The g operand is multiplied by 2^-40 or 2^20 -- below fp16's subnormals, above its largest
                finite value -- so that the case can only pass THROUGH the scale.
Shapes: (Cin, Cout) = (128, 256) and (256, 128), B = 2, 9 x 11 (198 rows: one 128-row panel, 64-row panels and a ragged last one;
no multiple of 16 for the weight gradient's pixel axis), dilations 1, 2, 4, the weight gradient with 1 and 3 slices.
"""
import functools
import zlib

import torch

import split2h_ref as RH
import split_exact as SE

CHANNELS = ((128, 256), (256, 128))
B, H, W = 2, 9, 11
DILATIONS = (1, 2, 4)
SHIFTS = (-40, 20)
KINDS = ("WN", "NW")
PRODUCTS = ("dgrad", "wgrad")
WGRAD_SLICES = (1, 3)
G_IS = {"dgrad": "a", "wgrad": "b"}         # which operand of the bilinear map is the gradient tensor: (g, w) -> dx, (x, g) -> dw
EPS2H = 2.0 ** -21                          # 22-bit operands and the dropped a1 b1
EPS_SUB = 2.0 ** -49                        # pieces of g s below fp16's subnormal resolution, relative to amax(g)


# ---- the scale word ---------------------------------------------------------------------------------------------------------------

def word_of(t):
    """max(bits & 0x7fffffff) over the fp32 tensor ``t``, as a Python int."""
    return int((t.detach().float().contiguous().view(torch.int32).reshape(-1) & 0x7FFFFFFF).max())


def scale_of_word(word):
    """(s, 1 / s) of a scale word, as Python floats (both exact powers of two)."""
    if word == 0 or word >= 0x7F800000:
        return 1.0, 1.0
    k = max(-126, min(126, 14 - ((word >> 23) - 127)))
    return 2.0 ** k, 2.0 ** -k


def scale_of(t):
    return scale_of_word(word_of(t))


# ---- the model ----------------------------------------------------------------------------------------------------------------------

def product2h(op, a, b):
    """op(a, b) by the fp16 two-piece model: hi = a0 b0, lo = a0 b1 + a1 b0, hi + 2^-11 lo; float64."""
    a0, a1 = RH.pieces(a)
    b0, b1 = RH.pieces(b)
    return RH.join(op(a0, b0), op(a0, b1) + op(a1, b0))


def grad_product(op, a, b, g_is, scaled=True):
    """A gradient product by the model: the g operand (``g_is`` = "a" or "b") times s in fp32, the three products, times 1 / s.
    ``scaled=False``: the split of g as it is -- what the mode would be without the scale word."""
    g = (a if g_is == "a" else b).float()
    s, inv = scale_of(g) if scaled else (1.0, 1.0)
    gs = g * s                                   # fp32: exact while nothing leaves the normal range
    out = product2h(op, gs, b) if g_is == "a" else product2h(op, a, gs)
    return out * inv


def mm_scaled(g, w, scaled=True):
    """g (M, K) . w (N, K)^T with g the scaled operand."""
    return grad_product(SE.gemm_op, g, w, "a", scaled)


def bound(op, a, b, g_is, e3=0.0):
    """2^-21 sum |a| |b| + 2^-49 amax(g) sum |b| + e3 per output, float64, b the unscaled operand."""
    g, other = (a, b) if g_is == "a" else (b, a)
    ones = torch.ones_like(g, dtype=torch.float64)
    sub = op(ones, other.double().abs()) if g_is == "a" else op(other.double().abs(), ones)
    return EPS2H * op(a.double().abs(), b.double().abs()) + EPS_SUB * float(g.abs().max()) * sub + e3


def table_classes(m=64, k=1152, n=32, seed=0):
    """The five input classes of the issue's table: name -> (g (m, k), He-scaled w (n, k))."""
    gen = torch.Generator().manual_seed(seed)
    w = torch.randn(n, k, generator=gen) * (2.0 / k) ** 0.5
    base = torch.randn(m, k, generator=gen)
    rows = torch.exp(torch.linspace(-25.0, 0.0, m)).view(m, 1)
    return {
        "N(0,1) 2^-30": (base * 2.0 ** -30, w),
        "N(0,1) 1e-12": (base * 1e-12, w),
        "rows e^-25..1, 1e-6": (base * rows * 1e-6, w),
        "N(0,1) 3e5": (base * 3e5, w),
        "N(0,1)": (base, w),
    }


# ---- the integer cases ------------------------------------------------------------------------------------------------------------

def wide(shape, gen):
    v = 1.0 + torch.randint(0, 2 ** 21, shape, generator=gen).double() * 2.0 ** -21
    return (v * (torch.randint(0, 2, shape, generator=gen).double() * 2 - 1)).float()


def narrow(shape, gen):
    return (torch.randint(1, 3, shape, generator=gen) * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)).float()


def two_per_row(t, gen):
    """``t`` (rows, ...) with all but two entries of every row zeroed."""
    flat = t.reshape(t.shape[0], -1)
    keep = torch.zeros_like(flat)
    idx = torch.stack([torch.randperm(flat.shape[1], generator=gen)[:2] for _ in range(flat.shape[0])])
    keep.scatter_(1, idx, 1.0)
    return (flat * keep).reshape(t.shape)


def lattice(x, step, gen):
    """The (B, C, H, W) map ``x`` with non-zeros at the pixels of a ``step``-pixel lattice alone, two channels each: a 3 x 3 window
    of dilation d (2 d + 1 pixels wide) sees one such pixel at most for step >= 2 d + 1."""
    b, c, h, w = x.shape
    keep = torch.zeros_like(x)
    for bi in range(b):
        for hi in range(0, h, step):
            for wi in range(0, w, step):
                keep[bi, torch.randperm(c, generator=gen)[:2], hi, wi] = 1.0
    return x * keep


def per_channel(shape, gen):
    """A narrow (B, C, H, W) map with two non-zero pixels per channel (over the whole batch): the pixel axis is the K of the weight
    gradient, so every dw element is a sum of two products at most."""
    b, c, h, w = shape
    return two_per_row(narrow((c, b, h, w), gen), gen).transpose(0, 1).contiguous()


class Case:
    def __init__(self, product, cin, cout, d, kind, shift):
        self.product, self.cin, self.cout, self.d, self.kind, self.shift = product, cin, cout, d, kind, shift
        self.name = "%s-%dto%d-d%d-%s-2^%d" % (product, cin, cout, d, kind, shift)

    def __repr__(self):
        return self.name


CASES = [Case(p, cin, cout, d, k, j) for p in PRODUCTS for cin, cout in CHANNELS for d in DILATIONS for k in KINDS for j in SHIFTS]


class Built:
    """a, b (fp32, the maps channels-last), the bilinear map and which operand is g."""

    def __init__(self, a, b, op, g_is):
        self.a, self.b, self.op, self.g_is = a, b, op, g_is

    @property
    def g(self):
        return self.a if self.g_is == "a" else self.b

    def exact(self):
        return self.op(self.a.double(), self.b.double())

    def model(self, scaled=True):
        return grad_product(self.op, self.a, self.b, self.g_is, scaled)


@functools.lru_cache(maxsize=None)
def build(case):
    """The Built of a case, made once per process and shared (never modified).  dgrad: (g, w) -> dx; wgrad: (x, g) -> dw."""
    gen = torch.Generator().manual_seed(zlib.crc32(("train2h-" + case.name).encode()))
    cin, cout, d, up = case.cin, case.cout, case.d, 2.0 ** case.shift
    if case.product == "dgrad":
        if case.kind == "WN":        # g wide and dense, two weights per INPUT channel (the rows of the data gradient's B operand)
            g = wide((B, cout, H, W), gen)
            w = two_per_row(narrow((cin, cout, 3, 3), gen), gen).transpose(0, 1).contiguous()
        else:
            g = lattice(narrow((B, cout, H, W), gen), 2 * d + 1, gen)
            w = wide((cout, cin, 3, 3), gen)
        return Built(SE.cl(g * up), w, SE.dgrad_op(1, d, d, (H, W)), "a")
    if case.kind == "WN":            # x wide and dense, two pixels per output channel of g
        x, g = wide((B, cin, H, W), gen), per_channel((B, cout, H, W), gen)
    else:
        x, g = per_channel((B, cin, H, W), gen), wide((B, cout, H, W), gen)
    return Built(SE.cl(x), SE.cl(g * up), SE.wgrad_op(1, d, d, 3), "b")
