"""The one table of launch-regime cases (test infrastructure, shared by tests/test_kernel_regimes_cpu.py and
tests/test_kernel_regimes_gpu.py; a plain module like tests/bounds_cases.py, whose Arena, run_case, compare and P it uses).

A host function of csrc/ picks a kernel instantiation from the geometry (class count, width, number of tiles), and a kernel
picks a form inside (a second trip of a loop, a staged or an un-staged path).  tools/kernel_coverage.py measures which
INSTANTIATIONS a traced run of the suite launches (profiles/r36_kernel_coverage_before.md / _after.md); this table holds, per
instantiation or in-kernel regime that the value tests' shape lists did not reach, one row with

  * ``entry``     the C-ABI entry (or the two entries of the OHEM pipeline) the case calls,
  * ``kernel``    the instantiation or regime the row is there for,
  * ``line``      the source line that decides the form,
  * ``predicate`` that decision restated on the host from the case's own arguments, as bounds_cases.one_launch_fits restates
                  make_fuse_geom(): tests/test_kernel_regimes_cpu.py asserts it for every row, so a case cannot drift out of its
                  regime when a constant of the library moves (the constants are restated below, next to their source line).

Every buffer lives between 0xFF guard bands, workspaces have exactly the queried size, and workspace entries are called twice on
the same buffers (bounds_cases.run_case).  The expectation ``want`` of every row is plain float64 torch on the CPU -- the
reference formula and its autograd, never the kernel or the C oracle; where the oracle has the entry the CPU file runs the same
case against it inside guards and holds it to the same ``want``.  Tolerances are those of the entry's value test in
tests/test_kernels_gpu.py, named beside each case function.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(HERE, "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import bounds_cases as BC  # noqa: E402
from bounds_cases import EXACT, P  # noqa: E402

# ---- constants of the library, restated (the predicate of a row fails when one of them moves) ----------------------------------
CE_TJ = CE_TI = 8            # kCeTJ, kCeTI: source cells per tile, csrc/ce_dev.hpp:119
CE_ROWS = 8                  # kCeRows: output rows of a cell per trip of the Y0 loop, csrc/ce_dev.hpp:120
CE_TGT_MAX = 8192            # kCeTgtMax: bytes of LDS for a tile's staged target rectangle, csrc/ce_dev.hpp:122
POOL_MAX_W = 1024            # kPoolMaxW, csrc/pairwise.hip:53
WAVE = 64                    # kWave
GRID_Y_MAX = 65535           # planes per launch of maxunpool_kernel, csrc/pairwise.hip:890
GRAM_TILE = 128              # kTile
GRAM_FULL_TILES = 1024       # ntri * B >= 1024 -> gram_loss_kernel<128>, csrc/pairwise.hip:984


def ce_cmax(C):
    """ce_cmax(), csrc/ce_dev.hpp:521: the class-count template of ce_cells_kernel and ohem_keys_kernel."""
    return 12 if C <= 12 else (19 if C <= 19 else (24 if C <= 24 else 64))


def ce_cell_ranges(n_in, n_out):
    """cell_range() on tap_of(), csrc/ce_dev.hpp:47-107, in fp32 as there: per source index the (lo, hi) of the destination
    indices whose first tap it is, or None."""
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0.0)
    i0 = np.minimum((scale * np.arange(n_out, dtype=np.float32)).astype(np.float32).astype(np.int64), n_in - 1)
    out = []
    for s in range(n_in):
        d = np.nonzero(i0 == s)[0]
        out.append((int(d[0]), int(d[-1])) if d.size else None)
    return out


def ce_tiles(h, w, H, W):
    """Per tile of 8 x 8 source cells what ce_cells_kernel (csrc/ce_dev.hpp:210-225, :249) derives from the geometry: ``trips`` of
    the Y0 loop of its tallest cell, the target ``rect`` (Y0, Y1, X0, X1) and whether that rectangle is ``staged`` in LDS."""
    ys, xs = ce_cell_ranges(h, H), ce_cell_ranges(w, W)
    tiles = []
    for ty in range(-(-h // CE_TJ)):
        for tx in range(-(-w // CE_TI)):
            ry = [r for r in ys[ty * CE_TJ:(ty + 1) * CE_TJ] if r]
            rx = [r for r in xs[tx * CE_TI:(tx + 1) * CE_TI] if r]
            if not ry or not rx:
                continue
            rect = (min(r[0] for r in ry), max(r[1] for r in ry), min(r[0] for r in rx), max(r[1] for r in rx))
            area = (rect[1] - rect[0] + 1) * (rect[3] - rect[2] + 1)
            tiles.append(dict(trips=max(-(-(r[1] - r[0] + 1) // CE_ROWS) for r in ry), rect=rect, staged=area <= CE_TGT_MAX))
    return tiles


def ohem_form(C, two_heads):
    """skd_ce_ohem_dsn_forward, csrc/ce_ohem.hip:294: (CMAX, TWO) of the ce_cells_kernel<CMAX, TWO, true> it launches (TWO: a second
    head was given); the key pass is ohem_keys_kernel<CMAX>, :244."""
    return ce_cmax(C), bool(two_heads)


def unpool_chunks(planes):
    """skd_maxunpool_scatter, csrc/pairwise.hip:890: launches of maxunpool_kernel, GRID_Y_MAX planes each."""
    return -(-planes // GRID_Y_MAX)


def ce_has(h, w, H, W, staged, several_trips):
    return any(t["staged"] == staged and (t["trips"] >= 2) == several_trips for t in ce_tiles(h, w, H, W))


def pool_nj(W):
    """skd_maxpool_argmax, csrc/pairwise.hip:857-871: the NJ of maxpool_band_kernel<NJ>, or 0 for maxpool_cell_kernel."""
    if W > POOL_MAX_W:
        return 0
    nj = -(-W // WAVE)
    return next(k for k in (1, 2, 4, 8, 16) if nj <= k)


def gram_form(B, M):
    """skd_pairwise_gram_loss, csrc/pairwise.hip:980-990: (tile height of the kernel it launches, tiles per side)."""
    ntiles = -(-M // GRAM_TILE)
    ntri = ntiles * (ntiles + 1) // 2
    return (64 if ntri * B < GRAM_FULL_TILES else 128), ntiles


class Regime:
    def __init__(self, name, entry, kernel, line, predicate, case=None, oracle=True, nan=False, post=None, ohem=None):
        self.name, self.entry, self.kernel, self.line, self.predicate = name, entry, kernel, line, predicate
        self.case, self.oracle, self.nan, self.post, self.ohem = case, oracle, nan, post, ohem


REGIMES = {}


def add(name, entry, kernel, line, predicate, fn=None, *args, ws=False, bit=False, oracle=True, nan=False, post=None, ohem=None):
    assert name not in REGIMES, name
    entries = (entry,) if isinstance(entry, str) else tuple(entry)
    case = None if fn is None else BC.Case(name, fn, entries, args, ws, bit, False, None)      # always carries its own ``want``
    REGIMES[name] = Regime(name, entries, kernel, line, predicate, case, oracle, nan, post, ohem)


# Kernels that no single-process, single-GPU test can launch, with the reason.  Nothing else may be listed
# (tests/test_kernel_regimes_cpu.py holds the allowed names).
_RANKS = "its launch needs a mailbox context and a second rank (tests/test_distributed_gpu.py owns it, skipped on one GPU)"
EXEMPT = {
    "sync_gather_kernel": _RANKS, "sync_stats_kernel": _RANKS, "sync_grad_stats_kernel": _RANKS,
    "abn_fwd_fused_nhwc_kernel<*, *, *, true>": _RANKS + ": the *_sync instantiations of the one-launch forward",
    "abn_bwd_fused_nhwc_kernel<*, *, *, *, true>": _RANKS + ": the *_sync instantiations of the one-launch backward",
}


def is_exempt(kernel):
    """``kernel``: a short name as tools/kernel_coverage.py prints it."""
    import fnmatch
    return any(fnmatch.fnmatchcase(kernel, pat.replace("<", "[<]").replace(">", "[>]")) for pat in EXEMPT)


# =====================================================================================================================
# 1. Fused cross-entropy with deep supervision, csrc/ce_dev.hpp.  Tolerances: test_ce_dsn (loss 1e-5, gradients 5e-5 of the
#    largest magnitude).  Expectation: F.interpolate(bilinear, align_corners=True) + F.cross_entropy(ignore_index=255) in float64
#    and its autograd.  The value tests and the ce_dsn-* rows of bounds_cases.py up-sample by at most 8 per axis: one trip of the
#    Y0 loop, the target rectangle always staged.
# =====================================================================================================================
def _ce_inputs(B, C, h, w, H, W, bad):
    g = BC._gen(H + C)
    lm, ld = torch.randn(B, C, h, w, generator=g) * 3, torch.randn(B, C, h, w, generator=g) * 3
    y = torch.randint(0, C, (B, H, W), generator=g)
    y[0, : max(1, H // 16)] = 255                                      # ignored rows
    y[-1, -1, -1] = 255
    if bad is not None:
        y[(0,) + tuple(bad)] = C + 3                                   # outside [0, C) and not the ignore value
    return lm, ld, y


def _ce_want(lm, ld, y, H, W):
    a = lm.double().requires_grad_(True)
    loss = F.cross_entropy(F.interpolate(a, size=(H, W), mode="bilinear", align_corners=True), y, ignore_index=255)
    if ld is not None:
        d = ld.double().requires_grad_(True)
        loss = loss + 0.4 * F.cross_entropy(F.interpolate(d, size=(H, W), mode="bilinear", align_corners=True), y, ignore_index=255)
    loss.backward()
    want = {"loss": loss.detach().reshape(1), "grad_main": a.grad}
    if ld is not None:
        want["grad_dsn"] = d.grad
    return want


def ce_regime(lib, A, B, C, h, w, H, W, two, bad=None):
    lm0, ld0, y = _ce_inputs(B, C, h, w, H, W, bad)
    if not two:
        ld0 = None
    lm, ld, yt = A.inp("logits_main", lm0), A.inp("logits_dsn", ld0), A.inp("target", y)
    loss, gm = A.out("loss", 1), A.out("grad_main", (B, C, h, w))
    gd = A.out("grad_dsn", (B, C, h, w)) if two else None
    ws = A.ws("workspace", lib.skd_ce_dsn_workspace_floats(B, C, h, w, H, W))
    call = lambda: lib.skd_ce_dsn_forward(B, C, h, w, H, W, P(lm), P(ld), P(yt), 255, 0.4, P(loss), P(gm), P(gd), P(ws), None)
    outs = {"loss": (loss, 1e-5), "grad_main": (gm, 5e-5)}
    if two:
        outs["grad_dsn"] = (gd, 5e-5)
    if bad is not None:                                                # F.cross_entropy asserts on such a label: the row demands NaN
        return call, outs, {k: torch.full(tuple(v[0].shape), float("nan"), dtype=torch.float64) for k, v in outs.items()}
    return call, outs, _ce_want(lm0, ld0, y, H, W)


CE_GEOMS = {
    # 5 -> 49 rows: cells of 12 rows (two trips); one tile, rectangle 49 x 61 = 2989 bytes: staged
    "trip2-staged": ((2, 19, 5, 7, 49, 61), True, True),
    # 9 -> 129: cells of 16 rows (two trips); tile 0 covers 128 x 128 = 16384 > 8192: un-staged
    "trips-unstaged": ((2, 19, 9, 9, 129, 129), False, True),
    # 9 -> 65 rows: cells of 8 rows (one trip); 3 -> 200 columns: the rectangle is 64 x 200 = 12800: un-staged
    "trip1-unstaged": ((1, 5, 9, 3, 65, 200), False, False),
}
for _n, (_s, _staged, _trips) in CE_GEOMS.items():
    for _two in (True, False):
        add("ce-%s-%s" % (_n, "two-heads" if _two else "main-head"), "skd_ce_dsn_forward",
            "ce_cells_kernel<%d, %s, false>: %s target path, %s of the Y0 loop" % (ce_cmax(_s[1]), "true" if _two else "false",
                                                                                   "staged" if _staged else "un-staged", "two trips" if _trips else "one trip"),
            "csrc/ce_dev.hpp:225 (staged), :249 (Y0 loop)",
            (lambda s=_s, a=_staged, t=_trips: ce_has(*s[2:], staged=a, several_trips=t)),
            ce_regime, *_s, _two, ws=True, bit=True)


def _bad_in_unstaged_tile(s, yx):
    return any(not t["staged"] and t["rect"][0] <= yx[0] <= t["rect"][1] and t["rect"][2] <= yx[1] <= t["rect"][3] for t in ce_tiles(*s[2:]))


# a label outside [0, C) where label() of the un-staged path classifies it itself (csrc/ce_dev.hpp:280-281): loss and both gradients
# NaN, as test_ce_dsn demands on the staged path
add("ce-trips-unstaged-bad-label", "skd_ce_dsn_forward", "ce_cells_kernel<19, true, false>: label() of the un-staged path meets a label outside [0, C)",
    "csrc/ce_dev.hpp:281", lambda: _bad_in_unstaged_tile((2, 19, 9, 9, 129, 129), (70, 40)),
    ce_regime, 2, 19, 9, 9, 129, 129, True, (70, 40), ws=True, nan=True)


# =====================================================================================================================
# 2. OHEM, csrc/ce_ohem.hip.  The fixtures of tests/golden/reference_ohem.pt have C in {5, 7, 11, 19}: the <24> and <64> forms of
#    the key pass and of the main pass never ran.  Run by tests/test_kernel_regimes_gpu.py through test_ohem_gpu.run_abi (both
#    entries, guarded, exact workspace, twice); expectation: tests/ohem_ref.py (float64) with the kink rule of
#    tests/test_ohem_gpu.py; its bounds (tau, loss 1e-5, gradients 5e-5).  The plain-C oracle has no OHEM entries.
#    Inputs: make_inputs() of tests/golden/make_golden_ohem.py; 9 x 17 -> 64 x 128, thresh 0.2, min_kept 9600 as its ``kth`` case.
# =====================================================================================================================
_OHEM = ("skd_ohem_threshold", "skd_ce_ohem_dsn_forward")
for _C in (21, 40):
    for _two in (True, False):
        add("ohem-C%d-%s" % (_C, "two-heads" if _two else "main-head"), _OHEM,
            "ohem_keys_kernel<%d>, ce_cells_kernel<%d, %s, true>" % (ce_cmax(_C), ce_cmax(_C), "true" if _two else "false"),
            "csrc/ce_dev.hpp:521 (ce_cmax), csrc/ce_ohem.hip:244, :294", (lambda C=_C, t=_two: ohem_form(C, t) == ((24 if C == 21 else 64), t)), oracle=False,
            ohem=dict(shape=(2, _C, 9, 17), size=(64, 128), thresh=0.2, min_kept=9600, factor=8, two=_two, seed=30 + _C))
add("ohem-trips-unstaged", _OHEM, "ce_cells_kernel<19, true, true>: un-staged target path, two trips of the Y0 loop",
    "csrc/ce_dev.hpp:225, :249", lambda: ce_has(9, 9, 129, 129, staged=False, several_trips=True), oracle=False,
    ohem=dict(shape=(2, 19, 9, 9), size=(129, 129), thresh=0.2, min_kept=6400, factor=8, two=True, seed=41))

# the one OHEM instantiation at the fixtures' own class counts that no fixture reaches: C = 19 with the main head alone
add("ohem-C19-main-head", _OHEM, "ce_cells_kernel<19, false, true>", "csrc/ce_ohem.hip:294 (TWO = logits_dsn != NULL)", lambda: ohem_form(19, False) == (19, False),
    oracle=False, ohem=dict(shape=(2, 19, 9, 17), size=(64, 128), thresh=0.2, min_kept=9600, factor=8, two=False, seed=11))


# =====================================================================================================================
# 3. Planar max-pool / un-pool, csrc/pairwise.hip.  Values and indices equal (test_maxpool_argmax_bit_exact).  Expectation:
#    F.max_pool2d(ceil_mode=True, return_indices=True): a max-pool selects, so its values are exact in any precision and the fp32
#    input is pooled as it is.  The tested widths 33 .. 130 and 1500 give NJ = 1, 2, 4 and the cell kernel.
# =====================================================================================================================
def _pool_data(planes, H, W):
    g = BC._gen(H * W)
    x = torch.randn(planes, H, W, generator=g)
    x[0] = torch.randint(0, 3, (H, W), generator=g).float()           # many ties: the first maximum wins
    x[1, :, W // 5: W // 5 + 70] = float("-inf")                       # whole windows of -inf
    x[1, H // 2, W // 3] = float("nan")                                # NaN propagates (PyTorch's scan rule)
    x[1, 0, 0] = float("nan")
    x[1, H - 1, W - 1] = float("nan")
    return x


def maxpool_regime(lib, A, planes, H, W, kh, kw):
    x0 = _pool_data(planes, H, W)
    OH, OW = -(-H // kh), -(-W // kw)
    x, p, i = A.inp("x", x0), A.out("pooled", (planes, OH * OW)), A.out("index", (planes, OH * OW), torch.int32)
    tp, ti = F.max_pool2d(x0[None], (kh, kw), (kh, kw), 0, ceil_mode=True, return_indices=True)
    want = {"pooled": tp[0].reshape(planes, -1), "index": ti[0].reshape(planes, -1).int()}
    call = lambda: lib.skd_maxpool_argmax(planes, H, W, kh, kw, P(x), P(p), P(i), None)
    return call, {"pooled": (p, EXACT), "index": (i, EXACT)}, want


for _W in (300, 700, 1024, 1025):
    for _kh, _kw in ((2, 3), (5, 64)):
        _nj = pool_nj(_W)
        add("maxpool-W%d-%dx%d" % (_W, _kh, _kw), "skd_maxpool_argmax",
            "maxpool_band_kernel<%d>" % _nj if _nj else "maxpool_cell_kernel, the neighbour across kPoolMaxW",
            "csrc/pairwise.hip:857, :867-871", (lambda W=_W: pool_nj(W) == {300: 8, 700: 16, 1024: 16, 1025: 0}[W]),
            maxpool_regime, 2, 5, _W, _kh, _kw)


def maxunpool_regime(lib, A, planes, H, W, kh, kw):
    g = BC._gen(planes)
    OH, OW = -(-H // kh), -(-W // kw)
    ldp = OH * OW + 5                                                  # strided rows, as in the value test
    idx = BC._pool_index(torch.randn(planes, H, W, generator=g), kh, kw)
    dp0 = torch.randn(planes, ldp, generator=g)
    dp, i, dx = A.inp("dpooled", dp0), A.inp("index", idx), A.out("dx", (planes, H, W))
    want = torch.zeros(planes, H * W).scatter_(1, idx.long(), dp0[:, :OH * OW]).view(planes, H, W)     # the windows are disjoint: no sums
    return (lambda: lib.skd_maxunpool_scatter(planes, H, W, kh, kw, P(dp), ldp, P(i), P(dx), None)), {"dx": (dx, EXACT)}, {"dx": want}


# every test passes at most 5 planes: the second chunk of the plane loop (gridDim.y <= 65535) never ran
add("maxunpool-65538-planes", "skd_maxunpool_scatter", "maxunpool_kernel: the second chunk of the plane loop", "csrc/pairwise.hip:890",
    lambda: unpool_chunks(65535 + 3) == 2, maxunpool_regime, 65535 + 3, 3, 3, 2, 2)


# =====================================================================================================================
# 4. Pair-wise Gram and loss, csrc/pairwise.hip.  Tolerances: test_pairwise_stages (G 2e-5 with floor 1.0, loss 1e-5).
#    Expectation: the einsum of test_pairwise_stages in float64 on the fp32 panels the entry reads.  Every case of that test
#    launches gram_loss_kernel<64>; the one bounds case at <128> (1024 images, M = 65) has a single diagonal tile per image:
#    the off-diagonal 128 x 128 tiles and their mirrored store were never compared with anything.
# =====================================================================================================================
def gram_regime(lib, A, B, Cs, Ct, M):
    ldm = lib.skd_pairwise_ldm(M)
    g = BC._gen(M + Cs)
    unit = lambda t: F.pad(t / ((t ** 2).sum(1, keepdim=True).sqrt() + 1e-8), (0, ldm - M)).contiguous()
    fs0, ft0 = unit(torch.randn(B, Cs, M, generator=g)), unit(torch.randn(B, Ct, M, generator=g))
    fs, ft, G, loss = A.inp("fhat_s", fs0), A.inp("fhat_t", ft0), A.out("G", (B, ldm, ldm)), A.out("loss", 1)
    ws = A.ws("workspace", max(1, lib.skd_pairwise_workspace_floats(B, M)))
    call = lambda: lib.skd_pairwise_gram_loss(B, Cs, Ct, M, ldm, P(fs), P(ft), P(G), P(loss), P(ws), None)
    Gd = torch.einsum("icm,icn->imn", ft0.double(), ft0.double()) - torch.einsum("icm,icn->imn", fs0.double(), fs0.double())
    want = {"G": Gd, "loss": ((Gd ** 2).sum() / M ** 2 / B).reshape(1)}
    return call, {"G": (G, 2e-5, 1.0), "loss": (loss, 1e-5, 1e-6)}, want


def gram_post(got, B, Cs, Ct, M):
    """The mirrored store: the two triangles of G agree bit for bit, and everything beyond M is an exact zero."""
    G = got["G"]
    assert BC.same_bits(G, G.transpose(1, 2).contiguous()), "G's upper and lower triangles differ"
    assert float(G[:, M:, :].abs().max()) == 0.0 and float(G[:, :, M:].abs().max()) == 0.0, "G's padding beyond M is not exactly zero"


# B = 342, M = 129: ldm = 256, two tiles per side, ntri * B = 1026 >= 1024.  (5, 3): a ragged single K-tile; (40, 70): several K-tiles
# with a ragged last one.  G is 90 MB.
for _Cs, _Ct in ((5, 3), (40, 70)):
    add("gram-128-offdiag-342x%dx%dx129" % (_Cs, _Ct), "skd_pairwise_gram_loss", "gram_loss_kernel<128>: off-diagonal tiles and their mirrored store",
        "csrc/pairwise.hip:984", lambda: gram_form(342, 129) == (128, 2), gram_regime, 342, _Cs, _Ct, 129, ws=True, post=gram_post)



# =====================================================================================================================
# 5. InPlace-ABN, channels-last, the normalise passes (csrc/abn_nhwc.hip).  Tolerances: test_abn_apply_nhwc (2e-5, in place) and
#    the apply_to bound of bounds_cases.py (3e-5).  Expectation: act((x - mean) / sqrt(var + eps) * (|weight| + eps) + bias
#    (+ residual)) in float64 (libs/functions.py of the reference; ELU with alpha 1).
#      * abn_apply_nhwc_kernel<ACT, RES, 4>: launch_apply_nhwc_act(), csrc/abn_nhwc.hip:356-363, takes NSETS = 4 for a power-of-two
#        C / 4 above 512 and up to 1024: C = 4096 only; the value tests stop at 2048 channels.
#      * abn_apply_nhwc_train_kernel<ACT, RES>: launch_apply_nhwc_train(), :512-517, by activation and residual pointer; the value
#        tests call the out-of-place entry with ReLU (with and without a residual) and leaky ReLU without one.
# =====================================================================================================================
ACT_NAME = {BC.ACT_NONE: "none", BC.ACT_LEAKY: "leaky", BC.ACT_ELU: "elu", BC.ACT_RELU: "relu"}
THREADS = 256                # kThreads, csrc/skd_common.hpp:11


def apply_nhwc_nsets(C):
    """launch_apply_nhwc_act(), csrc/abn_nhwc.hip:355-363: NSETS of abn_apply_nhwc_kernel, 0 for the generic kernel."""
    C4 = C // 4
    if C4 & (C4 - 1) or C4 > 4 * THREADS:
        return 0
    return 1 if C4 <= THREADS else (2 if C4 == 2 * THREADS else 4)


def apply_train_form(act, residual):
    """launch_apply_nhwc_train(), csrc/abn_nhwc.hip:512-517: the instantiation by activation code and residual pointer, None for a
    code the dispatch does not know."""
    known = {0: "SKD_ACT_NONE", 1: "SKD_ACT_LEAKY_RELU", 2: "SKD_ACT_ELU", 3: "SKD_ACT_RELU"}       # include/skd.h:32-37
    return "abn_apply_nhwc_train_kernel<%d, %s>" % (act, "true" if residual else "false") if act in known else None


def apply_generic_threads(rows, C):
    """launch_apply_nhwc_act(), csrc/abn_nhwc.hip:366-372, the generic kernel: (threads wanted, cap)."""
    C4 = C // 4
    quads, unit = rows * C4, C4
    while unit % THREADS:
        unit *= 2
    return -(-(-(-quads // 4)) // unit) * unit, -(-(256 * 8 * THREADS) // unit) * unit


def _act64(y, act):
    if act == BC.ACT_LEAKY:
        return torch.where(y < 0, y * BC.SLOPE, y)
    if act == BC.ACT_ELU:
        return torch.where(y > 0, y, torch.expm1(y))
    return torch.relu(y) if act == BC.ACT_RELU else y


def abn_apply_nhwc_regime(lib, A, rows, C, act, residual, to):
    call, outs = BC.abn_apply_nhwc(lib, A, rows, C, act, residual, to)
    d = {k: (v.double() if torch.is_tensor(v) else v) for k, v in BC._nhwc_data(rows, C, rows + C).items()}
    y = (d["x"] - d["rm"]) / torch.sqrt(d["rv"] + BC.EPS) * (d["w"].abs() + BC.EPS) + d["b"]
    return call, outs, {"out" if to else "z": _act64(y + d["r"] if residual else y, act)}


for _act in (BC.ACT_NONE, BC.ACT_LEAKY, BC.ACT_RELU):
    for _res in (False, True):
        add("abn_apply_nhwc-C4096-%s%s" % (ACT_NAME[_act], "-residual" if _res else ""), "skd_abn_apply_nhwc",
            "abn_apply_nhwc_kernel<%d, %s, 4>" % (_act, "true" if _res else "false"), "csrc/abn_nhwc.hip:356-363",
            lambda: apply_nhwc_nsets(4096) == 4, abn_apply_nhwc_regime, 3, 4096, _act, _res, False)
for _act, _res in ((BC.ACT_NONE, False), (BC.ACT_NONE, True), (BC.ACT_LEAKY, True), (BC.ACT_ELU, False), (BC.ACT_ELU, True)):
    add("abn_apply_nhwc_to-35x8-%s%s" % (ACT_NAME[_act], "-residual" if _res else ""), "skd_abn_apply_nhwc_to",
        "abn_apply_nhwc_train_kernel<%d, %s>" % (_act, "true" if _res else "false"), "csrc/abn_nhwc.hip:512-517",
        (lambda a=_act, r=_res: apply_train_form(a, r) == "abn_apply_nhwc_train_kernel<%d, %s>" % (a, "true" if r else "false")),
        abn_apply_nhwc_regime, 35, 8, _act, _res, True)


# =====================================================================================================================
# 6. InPlace-ABN backward with ELU, channels-last (csrc/abn_nhwc.hip).  The one-call entry sends ELU to the two launches
#    (abn_fused.hip:608: `activation != SKD_ACT_ELU`): abn_grad_nhwc2_kernel<2, 0, U> with U from pick_u() (csrc/abn_dev.hpp:320-330),
#    then abn_grad_dx_nhwc_kernel<2, 0, false>.  The value tests run the backward with leaky ReLU and with no activation only.
#    Tolerances: the abn_backward_nhwc rows of bounds_cases.py (test_abn_nhwc_one_call_backward): edz / eydz 5e-5, dx 1e-4 of
#    max |dz| x the largest gamma / sqrt(var + eps), dweight / dbias 5e-5.  Expectation, float64: z = elu(bn(x)) with the batch's own
#    statistics; dx, dweight, dbias by autograd of sum(z * dz); edz = mean(dy), eydz = mean(x_hat * dy) with dy = dz * elu'(y)
#    (bn.cu:175-177) -- from x, not through the kernel's inversion of z.
# =====================================================================================================================
RED_THREADS, RED_MAX_WG, GRAD0_U = 1024, 256, 8      # kRedThreads, kRedMaxWG (csrc/abn_dev.hpp:172-173), kGrad0U (csrc/abn_nhwc.hip:454)


def pick_u(rows, C, umax=GRAD0_U):
    """pick_u() on make_red_geom(), csrc/abn_dev.hpp:186-201, :320-330: rows in flight per thread and trip."""
    CB = 4 if C >= 256 else (2 if C >= 128 else 1)

    def rg(u):
        return min(-(-rows // (RED_THREADS // (C // 4 // CB) * u)), RED_MAX_WG // CB)
    u = umax
    while u > 2 and rg(u) * CB < RED_MAX_WG:
        if rg(u // 2) == rg(u):
            break
        u //= 2
    return u


ELU_EYDZ_W0_BASE = {(35, 8): 3.191e-5, (16200, 256): 6.445e-5, (3000, 256): 1.973e-4}      # measured as described in abn_elu_backward_nhwc


def abn_elu_backward_nhwc(lib, A, rows, C):
    g = BC._gen(rows + C)
    x0 = torch.randn(rows, C, generator=g) * 2.0 + torch.randn(1, C, generator=g)
    w0, b0, dz0 = torch.randn(C, generator=g), torch.randn(C, generator=g) * 0.5, torch.randn(rows, C, generator=g)
    w0[0], w0[1] = 0.0, -abs(w0[1])          # a zero and a negative weight (gamma = |weight| + eps), as bounds_cases._abn_data carries
    x = x0.double().requires_grad_(True)
    w, b = w0.double().requires_grad_(True), b0.double().requires_grad_(True)
    mean, var = x.mean(0), x.var(0, unbiased=False)
    xhat = (x - mean) / torch.sqrt(var + BC.EPS)
    y = xhat * (w.abs() + BC.EPS) + b
    z64 = _act64(y, BC.ACT_ELU)
    (z64 * dz0.double()).sum().backward()
    dy = dz0.double() * torch.where(y > 0, torch.ones_like(y), torch.exp(y)).detach()
    want = {"edz": dy.mean(0), "eydz": (xhat.detach() * dy).mean(0), "dx": x.grad, "dweight": w.grad, "dbias": b.grad}
    var32 = var.detach().float()
    z, dz, v = A.inp("z", z64.detach().float()), A.inp("dz", dz0), A.inp("var", var32)
    wt, bs = A.inp("weight", w0), A.inp("bias", b0)
    e, ey, dx, dw, db = A.out("edz", C), A.out("eydz", C), A.out("dx", (rows, C)), A.out("dweight", C), A.out("dbias", C)
    ws = BC._nhwc_ws(lib, A, rows, C)
    call = lambda: lib.skd_abn_backward_nhwc(rows, C, P(z), P(dz), P(v), P(wt), P(bs), P(e), P(ey), P(dx), P(dw), P(db), BC.EPS, BC.ACT_ELU, 0.0, 0,
                                             P(ws), None)
    mul = float(((w0.abs() + BC.EPS) / torch.sqrt(var32 + BC.EPS)).max())
    # eydz of the ZERO-weight channel: with gamma = eps the fp32 z no longer holds x_hat (the in-place formulation recovers it as
    # (z - beta) / gamma), whoever evaluates the formula.  Its bound is 3 x the measured base (GRAD_BOUND convention): torch's own fp32
    # CPU evaluation of the reference's backward formula (oracle/abn_torch.abn_backward_formula) on these inputs against float64, in
    # units of max |eydz| -- ELU_EYDZ_W0_BASE.  Every other channel, and every other output of that channel, keeps the entry's bound.
    scale = float(want["eydz"].abs().max())
    want["eydz_w0"], want["eydz"] = want["eydz"][:1], want["eydz"][1:]
    outs = {"edz": (e, 5e-5), "eydz": (lambda: ey[1:], 5e-5, scale), "eydz_w0": (lambda: ey[:1], 3 * ELU_EYDZ_W0_BASE[(rows, C)], scale),
            "dx": (dx, 1e-4, float(dz0.abs().max()) * mul), "dweight": (dw, 5e-5, 1e-6), "dbias": (db, 5e-5, 1e-6)}
    return call, outs, want


# (35, 8): one row group at every U -> 8; (16200, 256): 64 row groups (the cap) at U = 4 -> 4; (3000, 256): -> 2 (12 and 24 row groups)
for _rows, _C, _U in ((35, 8, 8), (16200, 256, 4), (3000, 256, 2)):
    add("abn_backward_nhwc-elu-%dx%d" % (_rows, _C), "skd_abn_backward_nhwc", "abn_grad_nhwc2_kernel<2, 0, %d>, abn_grad_dx_nhwc_kernel<2, 0, false>" % _U,
        "csrc/abn_dev.hpp:320-330 (pick_u), csrc/abn_fused.hip:608, csrc/abn_nhwc.hip:583, :598",
        (lambda r=_rows, c=_C, u=_U: pick_u(r, c) == u), abn_elu_backward_nhwc, _rows, _C, ws=True)


# =====================================================================================================================
# 7. Geometry-dependent forms of the host functions of the older files that no kernel name shows (grid caps, chunk loops, caps on
#    slots), read once against the value tests' shape lists.  Reached by an existing test (no row here):
#      * skd_maxunpool_scatter, `gx > 64` (csrc/pairwise.hip:887, H * W > 16384): test_maxpool_argmax_bit_exact[1-129-129-2-2];
#      * skd_maxpool_argmax_nhwc, `S > ww` (csrc/pairwise.hip:912, fewer window columns than column slots: C = 20 gives 51 slots for a
#        window 30 wide): test_maxpool_argmax_channels_last_bit_exact[3-20-46-61-23-30], maxpool_argmax_nhwc-window-3x20x46x61-23x30;
#      * skd_pairwise_backward, `n > kStreamWG` (csrc/pairwise.hip:1010): pairwise_backward-128-7x256x1025 of bounds_cases.py (567 > 512);
#      * skd_spectral_norm_backward / _multi, `parts > kBwdParts` (csrc/spectral.hip:293, :363, h * w > 2^20): test_spectral_norm[512-4096],
#        test_spectral_norm_multi_is_bit_identical_to_the_single_layer_entries[shapes0];
#      * fold_chunks(), `chunks > 8` and `chunks > H` (csrc/ppm.hip:877-878, fewer than 128 fold workgroups): ppm_fold_backward-3x4x7x9-L4
#        (8 capped to H = 7) and test_ppm_fold's small maps;
#      * the three cuts of make_plan() (csrc/abn.hip:35-55) and both forms of the fused-ABN switch: ABN_SHAPES / fused0 / fused1 there.
#    Rows below: `wgs > kMaxStage1` of skd_sum_f32; `g > 1024` of sn_finish_kernel and sn_bwd_apply_kernel and of their *_multi
#    forms (csrc/spectral.hip:281, :299, :337, :375; the largest tested and shipped weight, 512 x 4096, gives 512 and exactly 1024);
#    `threads > cap` of abn_apply_nhwc_generic_kernel (csrc/abn_nhwc.hip:371); `wgs > 8192` of zoom_linear_kernel
#    (csrc/evaluate_multiscale.hip:142);
#    `wgs > 8192` of seg_confusion_kernel (csrc/evaluate.hip:85; more than 2^24 pixels) and of accum_grid() (csrc/eval_dev.hpp:110, the
#    sliding and multi-scale tails; more than 2^23 pixels) have rows too: neither entry needs a target, so the large buffer is the
#    uint8 prediction map in the one and the float64 probability map of ONE class (64 MiB) in the other.
# =====================================================================================================================
SUM_PER_WG, SUM_MAX_WG = 4096, 1024          # csrc/reduce.hip:61, kMaxStage1 (csrc/reduce.hip:35)


def sum_regime(lib, A, n):
    """test_sum_f32: |err| <= 1e-6 max(1, sum |x|); a 2048-float workspace as there."""
    x0 = torch.randn(n, generator=BC._gen(n))
    x, o, ws = A.inp("x", x0), A.out("out", 1), A.ws("workspace", 2048)
    call = lambda: lib.skd_sum_f32(n, P(x), P(o), 0.5, P(ws), None)
    return call, {"out": (o, 1e-6, max(1.0, float(x0.double().abs().sum())))}, {"out": (0.5 * x0.double().sum()).reshape(1)}


# the largest tested n is 2^20 (256 workgroups): above 4096 * 1024 elements the grid is capped and a workgroup's share grows, ragged here
add("sum_f32-capped-grid", "skd_sum_f32", "sum_stage1_kernel: wgs capped at kMaxStage1, per_wg = 4097 with a ragged last workgroup",
    "csrc/reduce.hip:62", lambda: -(-(SUM_PER_WG * SUM_MAX_WG + 777) // SUM_PER_WG) > SUM_MAX_WG, sum_regime, SUM_PER_WG * SUM_MAX_WG + 777,
    ws=True, bit=True)


SN_FINISH_PER_WG, SN_APPLY_PER_WG, SN_MAX_WG = THREADS * 16, THREADS * 8, 1024          # csrc/spectral.hip:279-281, :297-299


def sn_grids(h, w):
    """(uncapped grid of sn_finish_kernel, of sn_bwd_apply_kernel): both are capped at 1024 workgroups, which then stride."""
    return -(-h * w // SN_FINISH_PER_WG), -(-h * w // SN_APPLY_PER_WG)


def _sn_want(W0, u0, v0, gw0, backward):
    """spectral.py:30-35 of the reference in float64: one power iteration with l2normalize(x) = x / (|x| + 1e-12), sigma = u . (W v),
    w = W / sigma; backward: autograd of W / (u . W v) with u and v constants."""
    W, u, v = W0.double(), u0.double(), v0.double()
    if not backward:
        t = W.t() @ u
        v1 = t / (t.norm() + 1e-12)
        t = W @ v1
        u1 = t / (t.norm() + 1e-12)
        sg = (u1 * t).sum()
        return {"u": u1, "v": v1, "sigma": sg.reshape(1), "w": W / sg}
    sig = (u @ W @ v).abs().float().double() + 0.1           # bounds_cases.spectral_backward: sigma is an INPUT of the entry
    Wr = W.clone().requires_grad_(True)
    # w = W / s with s the given sigma where it stands for u . W v: d/dW = gw / s - (sum(gw * W) / s^2) u v^T
    ((Wr / sig) * gw0.double()).sum().backward()
    return {"grad_w_bar": Wr.grad - (gw0.double() * W).sum() / sig ** 2 * torch.outer(u, v)}


def spectral_regime(lib, A, h, w, backward):
    """test_spectral_norm: forward 2e-5, backward 5e-5 (the tolerances bounds_cases.spectral_forward / _backward carry)."""
    call, outs = (BC.spectral_backward if backward else BC.spectral_forward)(lib, A, h, w)
    return call, outs, _sn_want(*BC._sn_data(h, w, BC._gen(h)), backward)


def spectral_multi_regime(lib, A, shapes, backward):
    call, outs = BC.spectral_multi(lib, A, shapes, backward)
    g = BC._gen(len(shapes) * 100 + shapes[0][0])
    want = {}
    for k, (h, w) in enumerate(shapes):                      # the same draws in the same order as bounds_cases.spectral_multi
        for n, t in _sn_want(*BC._sn_data(h, w, g), backward).items():
            want["%s%d" % (n, k)] = t
    return call, outs, want


# 1030 x 4096 = 4218880 elements: 1030 and 2060 workgroups wanted, 1024 launched, each striding twice or three times
for _b in (False, True):
    _n = "backward" if _b else "forward"
    add("spectral_%s-capped-grid-1030x4096" % _n, "skd_spectral_norm_" + _n, "%s: g capped at 1024" % ("sn_bwd_apply_kernel" if _b else "sn_finish_kernel"),
        "csrc/spectral.hip:%d" % (299 if _b else 281), (lambda b=_b: sn_grids(1030, 4096)[int(b)] > SN_MAX_WG), spectral_regime, 1030, 4096, _b, ws=True)
    add("spectral_%s_multi-capped-grid-1030x4096+5x3" % _n, "skd_spectral_norm_%s_multi" % _n,
        "%s: a layer's g capped at 1024, a small layer behind it" % ("sn_bwd_apply_multi_kernel" if _b else "sn_finish_multi_kernel"),
        "csrc/spectral.hip:%d" % (375 if _b else 337), (lambda b=_b: sn_grids(1030, 4096)[int(b)] > SN_MAX_WG and sn_grids(5, 3)[int(b)] == 1),
        spectral_multi_regime, [(1030, 4096), (5, 3)], _b, ws=True)

# C = 20 (no power of two): the generic kernel; 420000 rows are 2.1 M channel quads, 526080 threads wanted against a cap of 524800
add("abn_apply_nhwc-generic-capped-420000x20", "skd_abn_apply_nhwc", "abn_apply_nhwc_generic_kernel<1, false>: threads capped, every thread strides",
    "csrc/abn_nhwc.hip:371", lambda: apply_nhwc_nsets(20) == 0 and apply_generic_threads(420000, 20)[0] > apply_generic_threads(420000, 20)[1],
    abn_apply_nhwc_regime, 420000, 20, BC.ACT_LEAKY, False, False)


def zoom_regime(lib, A, C, H, W, Ho, Wo):
    """skd_zoom_linear against tests/multiscale_ref.zoom_linear (the order-1 zoom of the reference's evaluation restated in float64 and
    rounded once), same bits, as tests/test_multiscale_eval_gpu.guard_zoom compares it."""
    import multiscale_ref as M
    img0 = (np.random.RandomState(Ho).randn(C, H, W) * 57.0).astype(np.float32)
    img, out = A.inp("image", torch.from_numpy(img0), row=W), A.out("out", (1, C, Ho, Wo), row=Wo)
    call = lambda: lib.skd_zoom_linear(C, H, W, Ho, Wo, P(img), P(out), 0, 0, None)
    return call, {"out": (out, EXACT)}, {"out": torch.from_numpy(M.zoom_linear(img0, Ho, Wo))[None]}


# 1025 x 2049 = 2100225 output pixels: 8205 workgroups wanted, 8192 launched
add("zoom_linear-capped-grid-1x40x40-1025x2049", "skd_zoom_linear", "zoom_linear_kernel: wgs capped at 8192", "csrc/evaluate_multiscale.hip:142",
    lambda: -(-1025 * 2049 // THREADS) > 8192, zoom_regime, 1, 40, 40, 1025, 2049, oracle=False)


def seg_confusion_regime(lib, A, C, h, w, H, W):
    """test_seg_confusion_bit_exact: predictions bit-exact.  No target (the entry then writes ``pred`` only), so the one large buffer
    is the uint8 prediction map.  (h - 1) / (H - 1) = 2^-10 and integer logits in [-3, 3]: every interpolated value is a multiple of
    2^-20 below 4, exact in fp32 and in float64 alike, so the float64 expectation -- F.interpolate(bilinear, align_corners=True) and
    the first maximum -- holds bit for bit, ties included."""
    lg0 = torch.randint(-3, 4, (1, C, h, w), generator=BC._gen(H + C)).float()
    lg, pred = A.inp("logits", lg0), A.out("pred", (1, H, W), torch.uint8)
    up = F.interpolate(lg0.double(), size=(H, W), mode="bilinear", align_corners=True)
    call = lambda: lib.skd_seg_confusion(1, C, h, w, H, W, P(lg), None, 255, P(pred), None, None)
    return call, {"pred": (pred, EXACT)}, {"pred": up.argmax(1).to(torch.uint8)}


EVAL_MAX_WG = 8192           # csrc/evaluate.hip:85, csrc/eval_dev.hpp:110
# 4097 x 4097 = 2^24 + 8193 pixels at 8 per lane: 8197 workgroups wanted, 8192 launched (the shipped 1024 x 2048 x 8 gives exactly 8192)
add("seg_confusion-capped-grid-5x5-4097x4097", "skd_seg_confusion", "seg_confusion_kernel: wgs capped at 8192", "csrc/evaluate.hip:85",
    lambda: -(-4097 * 4097 // (THREADS * 8)) > EVAL_MAX_WG and (5 - 1) / (4097 - 1) == 2.0 ** -10, seg_confusion_regime, 2, 5, 5, 4097, 4097)


def seg_sliding_regime(lib, A, C, h, w, H, W):
    """One tile over the whole image, no target, no remap: predictions and the float64 probability map against the numpy restatement
    of the reference's sliding-window recipe (tests/sliding_ref.py), bit for bit, as test_seg_sliding_kernel_full_size_18_tiles_vs_restatement
    and the seg_sliding rows of bounds_cases.py compare them."""
    import sliding_ref as R
    tiles = R.tiles_of(H, W, (H, W))
    assert len(tiles) == 1
    lg0 = (np.random.RandomState(17 + C).randn(1, C, h, w) * 16).astype(np.float32)
    lg, tl = A.inp("logits", torch.from_numpy(lg0), row=w), A.inp("tiles", torch.tensor(tiles, dtype=torch.int32))
    pred, probs = A.out("pred", (H, W), torch.uint8), A.out("probs", (H, W, C), torch.float64)
    call = lambda: lib.skd_seg_sliding(1, C, h, w, H, W, H, W, P(lg), P(tl), None, 255, None, P(pred), P(probs), None, None)
    want_probs, want_pred = R.sliding(lg0, tiles, (H, W), (H, W))
    return call, {"pred": (pred, EXACT), "probs": (probs, EXACT)}, {"pred": torch.from_numpy(want_pred.astype(np.uint8)), "probs": torch.from_numpy(want_probs)}


# 2049 x 4097 = 2^23 + 6145 pixels at 4 per lane: 8199 workgroups wanted, 8192 launched; the float64 map is 64 MiB at one class
add("seg_sliding-capped-grid-9x13-2049x4097", "skd_seg_sliding", "seg_sliding_kernel<8>: accum_grid() capped at 8192",
    "csrc/eval_dev.hpp:110, csrc/evaluate_sliding.hip:78", lambda: -(-2049 * 4097 // (THREADS * 4)) > EVAL_MAX_WG,
    seg_sliding_regime, 1, 9, 13, 2049, 4097, oracle=False)
