"""The regime table of tests/regime_cases.py on the CPU: every row satisfies the predicate that puts it in its regime (the
library's decision restated on the host), the exemptions are the allowed ones by name, and every row whose entry the plain-C
oracle has runs against the oracle inside guard bands and is held to the row's float64 expectation -- which proves shapes, sizes
and argument order before a GPU sees them, and tests the oracle in the new regime."""
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import bounds_cases as BC  # noqa: E402
import regime_cases as RC  # noqa: E402

from oracle import cref  # noqa: E402
from structure_knowledge_distillation_amd import _lib  # noqa: E402

# kernels whose launch needs a second rank or a second GPU: sync.hip and the *_sync instantiations.  Nothing else may be exempt.
ALLOWED_EXEMPT = {
    "sync_gather_kernel", "sync_stats_kernel", "sync_grad_stats_kernel",
    "abn_fwd_fused_nhwc_kernel<*, *, *, true>", "abn_bwd_fused_nhwc_kernel<*, *, *, *, true>",
}
ORACLE_ROWS = [n for n, r in RC.REGIMES.items() if r.oracle and r.case is not None]


@pytest.fixture(scope="module")
def ref():
    return cref.load(_lib.SIGNATURES)


@pytest.mark.parametrize("name", list(RC.REGIMES))
def test_case_satisfies_the_predicate_of_its_regime(name):
    r = RC.REGIMES[name]
    assert r.kernel and all(e in _lib.SIGNATURES or any(e in t for t in _lib.ABI.values()) for e in r.entry), name
    cited = re.findall(r"(csrc/[a-z0-9_]+\.(?:hip|hpp)):(\d+)", r.line)        # every cited file exists and has the cited line
    assert cited and r.line.startswith("csrc/"), name
    for path, line in cited:
        full = os.path.join(os.path.dirname(_lib.__file__), path)
        assert os.path.isfile(full) and int(line) <= sum(1 for _ in open(full)), (name, path, line)
    assert r.predicate() is True, "%s is no longer in its regime (%s, decided at %s)" % (name, r.kernel, r.line)
    assert (r.case is None) != (r.ohem is None)


def test_exemptions_are_the_allowed_ones_by_name():
    assert set(RC.EXEMPT) <= ALLOWED_EXEMPT and all(isinstance(v, str) and v for v in RC.EXEMPT.values())
    assert RC.is_exempt("sync_stats_kernel") and RC.is_exempt("abn_fwd_fused_nhwc_kernel<3, true, 17, true>")
    assert RC.is_exempt("abn_bwd_fused_nhwc_kernel<0, 1, true, 9, true>")
    assert not RC.is_exempt("abn_fwd_fused_nhwc_kernel<3, true, 17, false>") and not RC.is_exempt("abn_bwd_fused_nhwc_kernel<0, 1, true, 9, false>")
    assert not RC.is_exempt("ce_cells_kernel<64, true, true>") and not RC.is_exempt("abn_stats_partial_kernel")


def test_host_restatements_on_the_shapes_the_value_tests_use():
    """The restated decisions give what the comments of the existing tables state for the existing shapes."""
    assert [RC.ce_cmax(C) for C in (3, 12, 13, 19, 21, 24, 25, 40, 64)] == [12, 12, 19, 19, 24, 24, 64, 64, 64]
    for h, w, H, W in ((9, 9, 65, 65), (65, 65, 512, 512), (33, 33, 256, 256), (46, 61, 360, 480), (1, 1, 4, 4), (5, 7, 5, 7), (17, 9, 100, 3)):
        assert all(t["staged"] and t["trips"] == 1 for t in RC.ce_tiles(h, w, H, W)), (h, w, H, W)       # the shapes of test_ce_dsn
    assert len(RC.ce_tiles(65, 65, 512, 512)) == 81 and RC.ce_cell_ranges(5, 49)[:2] == [(0, 11), (12, 23)] and RC.ce_cell_ranges(5, 49)[4] == (48, 48)
    assert RC.ce_tiles(5, 7, 40, 56)[0]["trips"] == 2                                                    # the OHEM fixture ``one_row``
    assert [RC.pool_nj(W) for W in (33, 61, 64, 65, 129, 130, 256, 257, 512, 513, 1024, 1025, 1500)] == [1, 1, 1, 2, 4, 4, 4, 8, 8, 16, 16, 0, 0]
    assert RC.sn_grids(512, 4096) == (512, 1024) and RC.apply_generic_threads(7, 20)[0] < RC.apply_generic_threads(7, 20)[1]
    assert [RC.apply_nhwc_nsets(C) for C in (8, 20, 1024, 2048, 4096, 8192, 48)] == [1, 0, 1, 2, 4, 0, 0]
    assert RC.gram_form(1, 4225) == (64, 34) and RC.gram_form(1024, 65) == (128, 1) and RC.gram_form(341, 129) == (64, 2)


@pytest.mark.parametrize("name", ORACLE_ROWS)
def test_oracle_in_the_regime_inside_guards(ref, name):
    r = RC.REGIMES[name]
    got, tols, want = BC.run_case(r.case, ref, BC.Arena("cpu"))
    for k, g in enumerate(got):
        if r.nan:
            assert all(bool(torch.isnan(g[o]).all()) for o in tols), "%s, call %d: not every output is NaN" % (name, k + 1)
        else:
            BC.compare(g, want, tols, "%s (oracle), call %d" % (name, k + 1))
        if r.post is not None:
            r.post(g, *r.case.args)
    if r.case.ws:                                     # the oracle is sequential: a dirty workspace never changes its bits
        for out in tols:
            assert BC.same_bits(got[0][out], got[1][out]), "%s: %s depends on what the workspace held" % (name, out)


@pytest.mark.parametrize("shape", list(RC.ELU_EYDZ_W0_BASE), ids=lambda s: "%dx%d" % s)
def test_widened_elu_bound_rests_on_a_base_that_still_holds(ref, shape):
    """The one bound of the table that is wider than its entry's (eydz of the zero-weight channel, 3 x base): torch's own fp32 CPU
    evaluation of the reference's backward formula on the case's inputs, against the case's float64 expectation, is still within a
    factor of 2 of the base written beside the case -- so a change of the inputs or of the generator cannot leave a stale bound."""
    from oracle import abn_torch as T
    rows, C = shape
    A = BC.Arena("cpu", guarded=False)
    _, outs, want = RC.abn_elu_backward_nhwc(ref, A, rows, C)
    b = {q["name"]: q["view"] for q in A.buffers}
    eydz = T.abn_backward_formula(b["z"].view(rows, C, 1), b["dz"].view(rows, C, 1), b["var"], b["weight"], b["bias"], True, BC.EPS, T.ACT_ELU, 0.0)[4]
    scale = outs["eydz_w0"][2]
    base = float((eydz[:1].double() - want["eydz_w0"]).abs().max()) / scale
    rest = float((eydz[1:].double() - want["eydz"]).abs().max()) / scale
    table = RC.ELU_EYDZ_W0_BASE[shape]
    assert table / 2 <= base <= table * 2, (shape, base, table)
    assert outs["eydz_w0"][1] == 3 * table and rest <= 5e-5 / 3, (shape, rest)          # the other channels need no such allowance
