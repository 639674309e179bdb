"""Integer inputs on which the six-product sum of the three-piece split core IS the exact product (CPU only; helper of
tests/test_split_exact_cpu.py and tests/test_split_exact_gpu.py, which both enumerate CASES below).

The core (csrc/conv_split_dev.hpp) cuts an fp32 operand into three bf16 pieces v = p0 + p1 + p2 (split2_ref.pieces) and keeps
the six products a_i b_j with i + j <= 2 (split2_ref._pairs(3)).  On integers every piece and every piece product is an integer,
so if   sum_k (|a0| + |a1| + |a2|) (|b0| + |b1| + |b2|)  <  2^24   for an output (abs_bound: the ABSOLUTE PIECES, which add up to
slightly more than |a|), every partial sum, in any order, across both accumulator sets and across split-K slices, is an exact
fp32 integer: the kernel must EQUAL the float64 product.  Three operand classes

    N  narrow   integers in [-3, 3] (or [-1, 1] / [0, 3])                               p1 = p2 = 0
    T  two      odd integers of magnitude in [2^8, 2^10), random sign                   p1 != 0, p2 = 0
    W  wide     integers of magnitude in [2^18, 2^19), random sign, kept if p1, p2 != 0 all three != 0

and three runs per kernel -- W x N pins a1 b0 and a2 b0, N x W pins a0 b1 and a0 b2, T x T pins a1 b1 (and a1 b0, a0 b1 again);
W x W and W x T cannot be exact.  T and W are sparse: a few non-zeros per dot product.

A case is described by two operands (a, b) and a bilinear map ``op`` of float64 tensors -- a GEMM, F.conv2d, its two gradients,
the pair-wise Gram with the kernel's mirror, the pair-wise backward -- so one model serves every kernel:
    model(drop) = sum over the kept (i, j) != drop of op(a_i, b_j)            exact = op(a, b)
``explain`` names the single-product-dropped model a wrong output equals, if any.
"""
import functools
import zlib

import torch
import torch.nn.functional as F

import split2_ref as R

LIMIT = 2 ** 24
PAIRS = R._pairs(3)                                   # the six products, (0, 0) first
LOWER = [p for p in PAIRS if p != (0, 0)]             # the five the one-piece integer tests do not see
PINS = {"WN": ((1, 0), (2, 0)), "NW": ((0, 1), (0, 2)), "TT": ((1, 1), (1, 0), (0, 1))}
KINDS = ("WN", "NW", "TT")


# ---- the three classes -------------------------------------------------------------------------------------------------------------

def _signs(gen, n, positive):
    return torch.ones(n) if positive else (torch.randint(0, 2, (n,), generator=gen) * 2 - 1).float()


def narrow(gen, shape, amax=3, positive=False):
    return torch.randint(0 if positive else -amax, amax + 1, shape, generator=gen).float()


def two_values(gen, n, positive=False):
    """n odd integers of magnitude in [2^8, 2^10): nine or ten significant bits with the last one set, so p1 != 0 and p2 = 0."""
    return (torch.randint(2 ** 7, 2 ** 9, (n,), generator=gen) * 2 + 1).float() * _signs(gen, n, positive)


def wide_values(gen, n, positive=False):
    """n integers of magnitude in [2^18, 2^19) whose second and third piece are both non-zero (the others are drawn again)."""
    kept, have = [torch.zeros(0)], 0
    while have < n:
        v = torch.randint(2 ** 18, 2 ** 19, (2 * n + 16,), generator=gen).float()
        p = R.pieces(v, 3)
        v = v[(p[1] != 0) & (p[2] != 0)]
        kept.append(v)
        have += v.numel()
    return torch.cat(kept)[:n] * _signs(gen, n, positive)


VALUES = {"T": two_values, "W": wide_values}


def placed(cls, gen, rows, k, per_row, positive=False):
    """A (rows, k) GEMM panel of class T or W with ``per_row`` non-zeros per row at deterministic positions: value j = per_row r + i
    of the panel sits at k = j s % k, s the first integer from 0.382 k on that is coprime to k.  Any k consecutive values -- a
    64-row block where 64 per_row >= k -- fall on every k exactly once, and neighbours in a row lie about 0.38 k apart."""
    s = max(1, round(0.382 * k))
    while _gcd(s, k) != 1:
        s += 1
    assert per_row <= k
    pos = (torch.arange(rows * per_row) * s % k).view(rows, per_row)
    t = torch.zeros(rows, k)
    t.scatter_(1, pos, VALUES[cls](gen, rows * per_row, positive).view(rows, per_row))
    return t


def scattered(cls, gen, rows, k, per_row):
    """A (rows, k) panel with ``per_row`` non-zeros per row at seeded random positions: rows meet each other irregularly."""
    pos = torch.rand(rows, k, generator=gen).argsort(1)[:, :per_row]
    t = torch.zeros(rows, k)
    t.scatter_(1, pos, VALUES[cls](gen, rows * per_row).view(rows, per_row))
    return t


def _gcd(a, b):
    while b:
        a, b = b, a % b
    return a


def sparse(cls, gen, shape, density, positive=False):
    """A tensor of class T or W: each element non-zero with probability ``density``."""
    hit = torch.rand(shape, generator=gen) < density
    t = torch.zeros(shape)
    t[hit] = VALUES[cls](gen, int(hit.sum()), positive)
    return t


def dense(cls, gen, shape, positive=False):
    n = 1
    for s in shape:
        n *= s
    return VALUES[cls](gen, n, positive).view(shape)


def symmetric(t):
    """The upper triangle of (..., M, M) mirrored below the diagonal."""
    return torch.triu(t) + torch.triu(t, 1).transpose(-1, -2)


# ---- the bilinear maps -------------------------------------------------------------------------------------------------------------

def gemm_op(a, b):
    """a (M, K) . b (N, K)^T"""
    return a @ b.t()


def conv_op(stride, padding, dilation):
    return lambda x, w: F.conv2d(x, w, None, stride, padding, dilation)


def dgrad_op(stride, padding, dilation, hw):
    """The data gradient of F.conv2d(., w, None, stride, padding, dilation) on an (H, W) = hw input: (g, w) -> dx."""
    def op(g, w):
        k = w.shape[2]
        pad = [hw[i] - ((g.shape[2 + i] - 1) * stride - 2 * padding + dilation * (k - 1) + 1) for i in (0, 1)]
        return F.conv_transpose2d(g, w, None, stride, padding, pad, 1, dilation)
    return op


def wgrad_op(stride, padding, dilation, ksize):
    """The weight gradient of the same convolution: (x, g) -> dw (Cout, Cin, k, k).  K is the pixel axis."""
    def op(x, g):
        return torch.nn.grad.conv2d_weight(x, (g.shape[1], x.shape[1], ksize, ksize), g, stride, padding, dilation)
    return op


def gram_op(ct, sign=-1.0):
    """csrc/pairwise_split.hip's Gram on the channel-major panel X = [teacher | student] (B, Ct + Cs, M) taken as both operands:
    G[m][n] = sum_teacher a[k][m] b[k][n] - sum_student a[k][m] b[k][n] for m <= n, MIRRORED below the diagonal as the kernel
    does (the six products are not symmetric in (m, n); the element (n, m) is never computed).  sign = +1: its absolute bound."""
    def op(a, b):
        full = torch.einsum("bkm,bkn->bmn", a[:, :ct], b[:, :ct]) + sign * torch.einsum("bkm,bkn->bmn", a[:, ct:], b[:, ct:])
        return symmetric(full)
    return op


def pair_bwd_op(fs, g):
    """The raw sum of the pair-wise backward: sum_n Fh[c][n] G[m][n] -> (B, Cs, M)."""
    return torch.einsum("bcn,bmn->bcm", fs, g)


# ---- a built case -------------------------------------------------------------------------------------------------------------------

class Built:
    """Operands and float64 results of one case.  ``mask``: the checked outputs (None: all); ``scale``: a power of two applied
    to the raw sum; ``extra``: an integer tensor added behind it (a residual); ``panels``: the (rows, K) views of the T / W
    operands of a GEMM-shaped case, for the coverage check; ``classes``: the class of a and of b; ``rows``: (class, tensor) of
    what the class check looks at (default: a and b themselves; a map with pixels the kernel never reads names the rows it does
    read); ``live``: the outputs that depend on the operands at all, where that is not every one (the pixels of a stride-2
    data gradient that no output reads are +0.0 whatever the kernel does) -- the power figures are shares of these."""

    def __init__(self, a, b, op, classes, op_abs=None, mask=None, scale=1.0, extra=None, panels=(), more=None, rows=None, live=None):
        self.a, self.b, self.op, self.op_abs, self.classes = a, b, op, op_abs or op, classes
        self.mask, self.scale, self.extra, self.panels, self.more = mask, scale, extra, panels, more or {}
        self.rows = rows or [(classes[0], a), (classes[1], b)]
        self.live = live
        self._terms = None

    def _finish(self, raw):
        y = raw * self.scale
        return y if self.extra is None else y + self.extra.double()

    def terms(self):
        if self._terms is None:
            pa, pb = R.pieces(self.a, 3), R.pieces(self.b, 3)
            self._terms = {(i, j): self.op(pa[i], pb[j]) for i, j in PAIRS}
        return self._terms

    def model(self, drop=None):
        """The six-product model in float64, without the product ``drop`` = (i, j) if one is given."""
        return self._finish(sum(t for p, t in self.terms().items() if p != drop))

    def exact(self):
        return self._finish(self.op(self.a.double(), self.b.double()))

    def abs_bound(self):
        """sum_k (|a0| + |a1| + |a2|) (|b0| + |b1| + |b2|) per output, float64 (+ |extra|): what no partial sum can exceed."""
        sa, sb = (sum(p.abs() for p in R.pieces(t, 3)) for t in (self.a, self.b))
        raw = self.op_abs(sa, sb)
        return raw if self.extra is None else raw + self.extra.double().abs()

    def checked(self, t):
        return t if self.mask is None else t[self.mask.expand_as(t)]

    def powered(self, t):
        """The outputs the power figures are shares of: the checked ones that depend on the operands."""
        return self.checked(t) if self.live is None else t[self.live.expand_as(t)]


def abs_bound(op, a, b):
    """The bound of a bare product ``op`` (gemm_op, conv_op(stride, padding, dilation), ...) on fp32 operands a, b."""
    return Built(a, b, op, "??").abs_bound()


def explain(got, built):
    """Why ``got`` (any float dtype, the case's output shape) is not the exact product: which single-product-dropped model it
    equals on the checked outputs, if any."""
    got = built.checked(got.double())
    want = built.checked(built.exact())
    wrong = int((got != want).sum())
    if wrong == 0:
        return "equals the exact product"
    head = "%d of %d checked outputs differ (largest difference %g)" % (wrong, want.numel(), float((got - want).abs().max()))
    hits = ["a%d.b%d" % p for p in PAIRS if torch.equal(got, built.checked(built.model(p)))]
    if hits:
        return head + ": equals the model WITHOUT " + " / ".join(hits)
    if not torch.equal(built.checked(built.model()), want):
        return head + "; the six-product model itself is not exact on these inputs (the case is wrong, not the kernel)"
    return head + "; no single-product-dropped model matches: not one lost product (accumulation, addressing or a tail)"


# ---- the operand triples -------------------------------------------------------------------------------------------------------------

def gemm_panels(kind, gen, rows_a, rows_b, k, positive=False, per_row=4, amax=3):
    """(A (rows_a, k), B (rows_b, k), the T / W panels): W x N and N x W with ``per_row`` wide values per row against a dense
    narrow operand (bound per_row * 2^19 * amax), T x T with ``per_row`` values per A row against a dense T operand (per_row * 2^20)."""
    if kind == "WN":
        a, b = placed("W", gen, rows_a, k, per_row, positive), narrow(gen, (rows_b, k), amax)
        return a, b, (a,)
    if kind == "NW":
        a, b = narrow(gen, (rows_a, k), amax, positive), placed("W", gen, rows_b, k, per_row)
        return a, b, (b,)
    a, b = placed("T", gen, rows_a, k, per_row, positive), dense("T", gen, (rows_b, k))
    return a, b, (a, b)


def map_pair(kind, gen, shape_a, shape_b, dot, wide_nz=8.0, hits=3.0):
    """Two tensors met over dot products of ``dot`` terms, by density: W x N / N x W with about ``wide_nz`` wide values per dot
    product against dense [-1, 1]; T x T with 1/8 of a against a density that gives about ``hits`` coincidences per output."""
    if kind == "WN":
        return sparse("W", gen, shape_a, wide_nz / dot), narrow(gen, shape_b, 1)
    if kind == "NW":
        return narrow(gen, shape_a, 1), sparse("W", gen, shape_b, wide_nz / dot)
    return sparse("T", gen, shape_a, 1.0 / 8), sparse("T", gen, shape_b, min(1.0, 8.0 * hits / dot))


def out_size(n, s):
    return (n - 1) // s + 1


def rows_to_map(rows, b, h, w, s, gen):
    """(B, C, H, W) map whose pixels (b, s ho, s wo) are the rows of ``rows`` (B Ho Wo, C) and whose other pixels -- which a
    stride-s 1x1 convolution never reads -- hold dense [-3, 3]: a wrong row map shows."""
    c = rows.shape[1]
    x = narrow(gen, (b, h, w, c), 3)
    x[:, ::s, ::s] = rows.view(b, out_size(h, s), out_size(w, s), c)
    return x.permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


# ---- the builders of the families -------------------------------------------------------------------------------------------------

def _conv1x1(kind, gen, m, k, n, positive):
    a, b, panels = gemm_panels(kind, gen, m, n, k, positive)
    return Built(a, b, gemm_op, kind, panels=panels)


def _conv3x3(kind, gen, b, cin, cout, h, w, d, stride=1, res=False, taps=9):
    """``taps``: how many taps of an output are inside the map at most (a single pixel: the centre alone), for the densities."""
    x, wt = map_pair(kind, gen, (b, cin, h, w), (cout, cin, 3, 3), taps * cin)
    ho, wo = out_size(h, stride), out_size(w, stride)
    extra = narrow(gen, (b, cout, ho, wo), 50) if res else None
    return Built(cl(x), wt, conv_op(stride, d, d), kind, extra=extra)


def _dgrad3x3(kind, gen, b, cout, cin, h, w, d):
    g, wt = map_pair(kind, gen, (b, cout, h, w), (cout, cin, 3, 3), 9 * cout)
    return Built(cl(g), wt, dgrad_op(1, d, d, (h, w)), kind)


def _wgrad3x3(kind, gen, b, cin, cout, h, w, d):
    x, g = map_pair(kind, gen, (b, cin, h, w), (b, cout, h, w), b * h * w)
    return Built(cl(x), cl(g), wgrad_op(1, d, d, 3), kind)


def _train_fwd(kind, gen, b, cin, cout, h, w, s):
    m = b * out_size(h, s) * out_size(w, s)
    a, wt, panels = gemm_panels(kind, gen, m, cout, cin)
    return Built(rows_to_map(a, b, h, w, s, gen), wt.view(cout, cin, 1, 1), conv_op(s, 0, 1), kind, panels=panels,
                 rows=[(kind[0], a), (kind[1], wt)])


def _train_dgrad(kind, gen, b, cin, cout, h, w, s):
    ho, wo = out_size(h, s), out_size(w, s)
    a, wtt, panels = gemm_panels(kind, gen, b * ho * wo, cin, cout)             # A = g rows, Bm = wt (Cin, Cout)
    g = rows_to_map(a, b, ho, wo, 1, gen)
    live = torch.zeros(h, w, dtype=torch.bool)
    live[::s, ::s] = True
    return Built(g, wtt.t().contiguous().view(cout, cin, 1, 1), dgrad_op(s, 0, 1, (h, w)), kind, panels=panels,
                 live=None if s == 1 else live)


def _train_wgrad(kind, gen, b, cin, cout, h, w, s):
    ho, wo = out_size(h, s), out_size(w, s)
    xt, gt, panels = gemm_panels(kind, gen, cin, cout, b * ho * wo)             # K = the output pixels
    x, g = rows_to_map(xt.t().contiguous(), b, h, w, s, gen), rows_to_map(gt.t().contiguous(), b, ho, wo, 1, gen)
    return Built(x, g, wgrad_op(s, 0, 1, 1), kind, panels=panels, rows=[(kind[0], xt), (kind[1], gt)])


def _gram(kind, gen, b, cs, ct, m):
    """Ft narrow everywhere; Fs {wide | narrow} by node halves (WN), {narrow | wide} (NW), two everywhere (TT).  The rows of the
    node-major copy are the nodes, K the channels.  Checked: everything but the wide x wide block (3/4 of G)."""
    ft = narrow(gen, (b, ct, m), 3)
    half = m // 2
    mask = None
    if kind == "TT":
        rows = [scattered("T", gen, m, cs, 6) for _ in range(b)]     # any two nodes share 36 / 32 channels on average
        panels = tuple(rows)
    else:
        lo = slice(0, half) if kind == "WN" else slice(half, m)
        rows = []
        for _ in range(b):
            t = narrow(gen, (m, cs), 3)
            t[lo] = placed("W", gen, half, cs, 4)
            rows.append(t)
        panels = tuple(t[lo] for t in rows)
        mask = torch.ones(m, m, dtype=torch.bool)
        mask[lo, lo] = False
    fs = torch.stack(rows).transpose(1, 2).contiguous()                        # (B, Cs, M), channel-major as the entry takes it
    x = torch.cat([ft, fs], 1)
    cls = "T" if kind == "TT" else "W"
    rest = [] if kind == "TT" else [("N", torch.stack([t[half:] if kind == "WN" else t[:half] for t in rows]))]
    return Built(x, x, gram_op(ct), kind, op_abs=gram_op(ct, 1.0), mask=mask, panels=panels, more=dict(fs=fs, ft=ft),
                 rows=[(cls, torch.stack(panels)), ("N", ft)] + rest)


def _pair_bwd(kind, gen, b, cs, m):
    """A = rows c of Fh (B, Cs, M), Bm = rows m of the symmetric G (B, M, M), K = the nodes; coef = -4 / (M^2 B), a power of two."""
    if kind == "WN":
        fs = torch.stack([placed("W", gen, cs, m, 4) for _ in range(b)])
        g = symmetric(narrow(gen, (b, m, m), 3))
        panels = tuple(fs)
    elif kind == "NW":
        fs = narrow(gen, (b, cs, m), 1)
        g = symmetric(torch.stack([placed("W", gen, m, m, 2) for _ in range(b)]))
        panels = tuple(g)
    else:
        fs = torch.stack([placed("T", gen, cs, m, 4) for _ in range(b)])
        g = symmetric(dense("T", gen, (b, m, m)))
        panels = tuple(fs) + tuple(g)
    scale = -4.0 / (m * m * b)
    assert scale == -(2.0 ** -13)
    return Built(fs, g, pair_bwd_op, kind, scale=scale, panels=panels)


BUILDERS = {"conv1x1": _conv1x1, "conv3x3": _conv3x3, "dgrad3x3": _dgrad3x3, "wgrad3x3": _wgrad3x3, "train_fwd": _train_fwd,
            "train_dgrad": _train_dgrad, "train_wgrad": _train_wgrad, "gram": _gram, "pair_bwd": _pair_bwd}


# ---- the case table -----------------------------------------------------------------------------------------------------------------

class Case:
    """One run of one family: ``group`` names the entry (or entries) the GPU file launches, ``builder`` + ``args`` the inputs."""

    def __init__(self, group, tag, builder, kind, **args):
        self.group, self.tag, self.builder, self.kind, self.args = group, tag, builder, kind, args
        self.triple = "%s-%s" % (group, tag) if tag else group
        self.name = "%s-%s" % (self.triple, kind)

    def __repr__(self):
        return self.name


def _triple(group, tag, builder, **args):
    return [Case(group, tag, builder, kind, **args) for kind in KINDS]


def _cases():
    c = []
    # skd_conv1x1_abn_nhwc, and again through the prologue form with an identity pack on non-negative activations
    c += _triple("conv1x1", "M2113-K80-N256", "conv1x1", m=2113, k=80, n=256, positive=False)
    c += _triple("conv1x1_pro", "M2113-K80-N256", "conv1x1", m=2113, k=80, n=256, positive=True)
    # skd_conv3x3_split_nhwc / _res_nhwc: 2 x 32 x 13 x 11 -> 128
    for d in (1, 2):
        c += _triple("conv3x3", "13x11-d%d" % d, "conv3x3", b=2, cin=32, cout=128, h=13, w=11, d=d)
        c += _triple("conv3x3_res", "13x11-d%d" % d, "conv3x3", b=2, cin=32, cout=128, h=13, w=11, d=d, res=True)
    # skd_conv3x3_narrow_nhwc: the 64-column B image
    c += _triple("narrow", "64to64-13x11-d2", "conv3x3", b=2, cin=64, cout=64, h=13, w=11, d=2)
    # the data gradient on the backward image of the pack pairs, Cin != Cout
    c += _triple("dgrad", "32to128-13x11-d2", "dgrad3x3", b=2, cout=32, cin=128, h=13, w=11, d=2)
    c += _triple("narrow_dgrad", "32to64-13x11-d2", "dgrad3x3", b=2, cout=32, cin=64, h=13, w=11, d=2)
    # skd_conv3x3_split_s2_nhwc: the smallest shape of the stride-2 integer test, and its smallest ragged one with full taps
    c += _triple("s2", "1x1x1-16-128", "conv3x3", b=1, cin=16, cout=128, h=1, w=1, d=1, stride=2, taps=1)
    c += _triple("s2", "2x6x6-32-128", "conv3x3", b=2, cin=32, cout=128, h=6, w=6, d=1, stride=2)
    # the 3x3 weight gradients: K is the pixel axis, both operands are activations
    for cin, cout in ((128, 128), (128, 256)):
        c += _triple("wgrad", "%dto%d-13x11-d2" % (cin, cout), "wgrad3x3", b=2, cin=cin, cout=cout, h=13, w=11, d=2)
    for cin, cout in ((64, 64), (64, 128)):
        c += _triple("narrow_wgrad", "%dto%d-13x11-d2" % (cin, cout), "wgrad3x3", b=2, cin=cin, cout=cout, h=13, w=11, d=2)
    # the 1x1 training entries at the smallest integer shapes of tests/test_conv1x1_train_gpu.py with a ragged tile and more than
    # two K-tiles, strides 1 and 2
    for tag, shape in (("128-64-13x11-s1", dict(b=2, cin=128, cout=64, h=13, w=11, s=1)),
                       ("64-128-13x11-s2", dict(b=2, cin=64, cout=128, h=13, w=11, s=2)),
                       ("128-256-9x9-s1", dict(b=1, cin=128, cout=256, h=9, w=9, s=1))):
        for product in ("train_fwd", "train_dgrad", "train_wgrad"):
            c += _triple(product, tag, product, **shape)
    # the pair-wise Gram (G only) and backward
    c += _triple("gram", "B2-C32-M128", "gram", b=2, cs=32, ct=32, m=128)
    c += _triple("pair_bwd", "B2-C32-M128", "pair_bwd", b=2, cs=32, m=128)
    return c


CASES = _cases()
TRIPLES = sorted({c.triple for c in CASES})
GROUPS = sorted({c.group for c in CASES})
GEMM_SHAPED = ("conv1x1", "conv1x1_pro", "train_fwd", "train_dgrad", "train_wgrad", "gram", "pair_bwd")


@functools.lru_cache(maxsize=None)
def build(case):
    """The Built of a case, made once per process and shared (never modified)."""
    gen = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    return BUILDERS[case.builder](case.kind, gen, **case.args)
