"""The integer cases of the two-piece training convolutions (include/skd_train2.h): one table for tests/test_train2_cpu.py,
which proves on the CPU what each case claims, and tests/test_train2_gpu.py, which launches it.  A plain module like
tests/split_exact.py, whose operand classes, bilinear maps and ``Built`` it uses (imported, never edited).

Two bf16 pieces hold 16 significant bits and the core keeps a0 b0 + a0 b1 + a1 b0 (split2_ref._pairs(2)).  On integers every
piece and every piece product is an integer, so while the sum of the absolute piece products of an output stays below 2^24
every partial sum -- in any order, across the two accumulator sets and across the split-K slices -- is an exact fp32 integer.

    N  narrow   integers in [-200, 200]: at most 8 significant bits, ONE piece (a1 = 0)
    T  two      split_exact.two_values: odd integers of magnitude in [2^8, 2^10), at most 16 bits, TWO pieces (a1 != 0, r = 0)

    NT, TN   narrow x wide, either way round: a1 b1 = 0, the three products ARE the exact product
    TT       two pieces on both sides: the kernel equals the three-product model and NOT the exact product (a1 b1 is dropped)

Shapes: (Cin, Cout) = (128, 256) and (256, 128) -- more than one 128-tile on either side --, B = 2, 9 x 11 (P = 198 is no
multiple of 16; pixel quads straddle row and image ends), dilation 1 and 2; the three products of a training convolution.
"""
import functools
import zlib

import torch

import split2_ref as R
import split_exact as SE

LIMIT = SE.LIMIT
CHANNELS = ((128, 256), (256, 128))
B, H, W = 2, 9, 11
DILATIONS = (1, 2)
KINDS = ("NT", "TN", "TT")
PRODUCTS = ("fwd", "dgrad", "wgrad")
WGRAD_SLICES = (1, 3)
NARROW_MAX = 200            # < 2^8: one bf16 piece
PAIRS2 = R._pairs(2)        # (0, 0), (0, 1), (1, 0)


class Case:
    def __init__(self, product, cin, cout, d, kind):
        self.product, self.cin, self.cout, self.d, self.kind = product, cin, cout, d, kind
        self.name = "%s-%dto%d-d%d-%s" % (product, cin, cout, d, kind)

    def __repr__(self):
        return self.name


CASES = [Case(p, cin, cout, d, k) for p in PRODUCTS for cin, cout in CHANNELS for d in DILATIONS for k in KINDS]


def _operand(cls, gen, shape, density):
    return SE.narrow(gen, shape, NARROW_MAX) if cls == "N" else SE.sparse("T", gen, shape, density)


def _pair(kind, gen, shape_a, shape_b, dot):
    """NT / TN: about 8 two-piece values per dot product against a dense narrow operand (bound 8 * 200 * 2^10 < 2^21);
    TT: 1/8 of a against a density that gives about two coincidences per output (each product below 2^20)."""
    if kind == "TT":
        return SE.sparse("T", gen, shape_a, 1.0 / 8), SE.sparse("T", gen, shape_b, min(1.0, 16.0 / dot))
    return _operand(kind[0], gen, shape_a, 8.0 / dot), _operand(kind[1], gen, shape_b, 8.0 / dot)


@functools.lru_cache(maxsize=None)
def build(case):
    """The split_exact.Built of a case -- a, b and the bilinear map -- made once per process and shared (never modified).
    fwd: (x, w) -> y; dgrad: (g, w) -> dx; wgrad: (x, g) -> dw."""
    gen = torch.Generator().manual_seed(zlib.crc32(("train2-" + case.name).encode()))
    cin, cout, d = case.cin, case.cout, case.d
    if case.product == "fwd":
        a, b = _pair(case.kind, gen, (B, cin, H, W), (cout, cin, 3, 3), 9 * cin)
        return SE.Built(SE.cl(a), b, SE.conv_op(1, d, d), case.kind)
    if case.product == "dgrad":
        a, b = _pair(case.kind, gen, (B, cout, H, W), (cout, cin, 3, 3), 9 * cout)
        return SE.Built(SE.cl(a), b, SE.dgrad_op(1, d, d, (H, W)), case.kind)
    a, b = _pair(case.kind, gen, (B, cin, H, W), (B, cout, H, W), B * H * W)
    return SE.Built(SE.cl(a), SE.cl(b), SE.wgrad_op(1, d, d, 3), case.kind)


def model2(built):
    """The three-product model of the two-piece core in float64: a0 b0 + a0 b1 + a1 b0."""
    pa, pb = R.pieces(built.a, 2), R.pieces(built.b, 2)
    return sum(built.op(pa[i], pb[j]) for i, j in PAIRS2)


def abs_bound2(built):
    """sum_k (|a0| + |a1|) (|b0| + |b1|) per output, float64: what no partial sum of piece products can exceed."""
    sa, sb = (sum(p.abs() for p in R.pieces(t, 2)) for t in (built.a, built.b))
    return built.op_abs(sa, sb)


def want_of(case):
    """(what the kernel must equal bit for bit, the exact product): the same tensor for NT / TN, the model for TT."""
    built = build(case)
    exact = built.exact()
    return (model2(built) if case.kind == "TT" else exact), exact
