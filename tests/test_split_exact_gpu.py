"""-m gpu: all six piece products of every three-piece split-core kernel, by EQUALITY with the float64 product.

The one-piece integer tests of the kernels' own files (|x| <= 7, |w| <= 3) live entirely in piece 0: the planes of pieces 1 and 2
hold zeros there, so they pin a0 b0 and nothing else, and the five lower products -- a1 b0, a2 b0, a0 b1, a0 b2, a1 b1 -- are held
only by the statistical contract (4 x the parent's error), which a fault at the a1 b1 level (about 1e-6 relative: two planes of a
pack swapped, a wrong plane stride, a piece table swapped on one side, a K-tail zeroed in plane 0 only) passes.  Here every entry
runs the case triples of tests/split_exact.py -- wide x narrow, narrow x wide, two x two: integers on which the six-product sum
is the exact product and every partial sum, in any order, is an exact fp32 integer (tests/test_split_exact_cpu.py proves that for
exactly these cases, and that every lower product, dropped, changes at least a quarter of the outputs of the run that pins it).
The assertion is torch.equal on the checked outputs -- the whole output, except the two half / half Gram runs, where it is the
3/4 of G outside the wide x wide block; a red case says which single-product-dropped model the output equals, if any
(split_exact.explain).  Raw or identity epilogues everywhere.  The launch helpers are those of the kernels' own test files.
profiles/r30_split_exact.md tabulates bounds, power and the result on an MI355X.
"""
import pytest
import torch

import split_exact as X
import test_conv1x1_split_gpu as T1
import test_conv1x1_train_gpu as TS
import test_conv3x3_narrow_gpu as TN
import test_conv3x3_narrow_wgrad_gpu as TNW
import test_conv3x3_split_gpu as T3
import test_conv3x3_stride2_gpu as T2
import test_conv3x3_train_gpu as TD
import test_conv3x3_wgrad_gpu as TW
import test_pairwise_split_gpu as TP
from structure_knowledge_distillation_amd import _lib

pytestmark = pytest.mark.gpu
DEV = T3.DEV
P = T3.P
RAW = {"cbias": None, "mean": None, "var": None, "gamma": None, "beta": None, "eps": 0.0, "act": "none"}


@pytest.fixture(scope="module")
def hip():
    return _lib.load()


# ---- one launcher per group: [(label, output in the shape of Built.exact())] -----------------------------------------------------

def _conv1x1(hip, case, built):
    m, k, n = case.args["m"], case.args["k"], case.args["n"]
    mean, var, ga, be, eps = T1._identity_epilogue(n)
    return [("skd_conv1x1_abn_nhwc", T1.run_hip(hip, m, k, n, built.a, built.b, None, mean, var, ga, be, eps, None, T1.ACT_NONE))]


def _conv1x1_pro(hip, case, built):
    """The prologue form with an identity table: mean 0, var 1, |gamma| = 1 (random signs), beta 0, eps 0 -- relu(x) = x on the
    case's non-negative activations.  (T1.run_hip packs with eps = 1e-5, which is no identity: the two calls are made here.)"""
    m, k, n = case.args["m"], case.args["k"], case.args["n"]
    assert float(built.a.min()) >= 0
    gen = torch.Generator().manual_seed(k)
    src = [torch.zeros(k), torch.ones(k), (torch.randint(0, 2, (k,), generator=gen) * 2 - 1).float(), torch.zeros(k)]
    table = torch.empty(4, k, device=DEV)
    dsrc = [t.to(DEV) for t in src]
    assert hip.skd_abn_pack_eval_params(k, *(P(t) for t in dsrc), 0.0, P(table), None)
    assert torch.equal(table.cpu(), torch.stack([src[0], src[1], src[1], src[3]])), "mean 0 | invstd 1 | gamma 1 | beta 0"
    mean, var = torch.zeros(n, device=DEV), torch.ones(n, device=DEV)
    dx, dw = built.a.to(DEV), built.b.to(DEV)
    out = torch.full((m + T1.SLACK_ROWS, n), T1.SENTINEL, device=DEV)
    assert hip.skd_conv1x1_abn_pro_nhwc(m, k, n, P(dx), P(dw), None, P(out), P(mean), P(var), None, None, 0.0, P(table),
                                        T1.ACT_NONE, 0.01, None)
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool((out[m:] == T1.SENTINEL).all()), "rows beyond M were written"
    return [("skd_conv1x1_abn_pro_nhwc", out[:m])]


def _conv3x3(hip, case, built):
    return [("skd_conv3x3_split_nhwc", T3.run_hip(hip, built.a, built.b, RAW, case.args["d"])[0])]


def _conv3x3_res(hip, case, built):
    b, cin, h, w = built.a.shape
    cout, d, m = built.b.shape[0], case.args["d"], b * h * w
    dx = built.a.to(DEV).contiguous(memory_format=torch.channels_last)
    pk = T3.pack(hip, built.b.to(DEV))
    res = built.extra.permute(0, 2, 3, 1).reshape(m, cout).contiguous().to(DEV)
    out = torch.full((m + T3.SLACK_ROWS, cout), T3.SENTINEL, device=DEV)
    assert hip.skd_conv3x3_split_res_nhwc(b, h, w, cin, cout, d, P(dx), P(pk), P(out), P(res), None, None, None, None, None, 0.0, 0,
                                          0.01, 0, None)
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool((out[m:] == T3.SENTINEL).all()), "rows beyond M were written"
    return [("skd_conv3x3_split_res_nhwc", out[:m].view(b, h, w, cout).permute(0, 3, 1, 2))]


def _narrow(hip, case, built):
    return [("skd_conv3x3_narrow_nhwc", TN.run_narrow(hip, built.a, built.b, None, case.args["d"]))]


def _dgrad(hip, case, built):
    return [("skd_conv3x3_split_pack_pair + skd_conv3x3_split_nhwc", TD.run_dgrad(hip, built.a, built.b, case.args["d"]))]


def _narrow_dgrad(hip, case, built):
    dg = built.a.to(DEV).contiguous(memory_format=torch.channels_last)
    _, pb = TN.narrow_pack(hip, built.b.to(DEV), fwd=False, bwd=True)
    return [("skd_conv3x3_narrow_pack_pair + skd_conv3x3_narrow_nhwc", TN.launch(hip, dg, pb, built.b.shape[1], case.args["d"]))]


def _s2(hip, case, built):
    return [("skd_conv3x3_split_s2_nhwc", T2.run_s2(hip, built.a, built.b, RAW))]


def _wgrad_with(module, entry):
    def run(hip, case, built):
        outs, used = [], set()
        for slices in (1, 0):
            n = module.plan_of(hip, built.a, built.b, slices)[0]
            outs.append(("%s, slices %d (%d used)" % (entry, slices, n), module.run_entry(hip, built.a, built.b, case.args["d"], slices)))
            used.add(n)
        assert 1 in used
        return outs
    return run


def _train_fwd(hip, case, built):
    s, cout = case.args["s"], case.args["cout"]
    outs = [("skd_conv1x1_train_fwd_cols64_nhwc", TS.run_fwd(hip, built.a, built.b, s, cols64=True))]
    if cout % 128 == 0:
        outs.append(("skd_conv1x1_train_fwd_nhwc", TS.run_fwd(hip, built.a, built.b, s)))
    return outs


def _train_dgrad(hip, case, built):
    s, cin, h, w = (case.args[k] for k in ("s", "cin", "h", "w"))
    outs = [("skd_conv1x1_train_dgrad_cols64_nhwc", TS.run_dgrad(hip, built.a, built.b, s, h, w, cols64=True))]
    if cin % 128 == 0:
        outs.append(("skd_conv1x1_train_dgrad_nhwc", TS.run_dgrad(hip, built.a, built.b, s, h, w)))
    return outs


def _train_wgrad(hip, case, built):
    s = case.args["s"]
    return [("skd_conv1x1_train_wgrad_nhwc, slices %d" % slices, TS.run_wgrad(hip, built.a, built.b, s, slices)) for slices in (1, 0)]


def _gram(hip, case, built):
    b, cs, ct, m = (case.args[k] for k in ("b", "cs", "ct", "m"))
    ldm = hip.skd_pairwise_ldm(m)
    assert ldm == m
    G, _ = TP.gram(hip, True, (b, cs, ct, m), ldm, built.more["fs"].to(DEV), built.more["ft"].to(DEV))
    assert torch.equal(TP.bits(G), TP.bits(G.transpose(1, 2))), "G is not bit-for-bit symmetric"
    return [("skd_pairwise_split_gram_loss", G.cpu())]


def _pair_bwd(hip, case, built):
    b, cs, m = (case.args[k] for k in ("b", "cs", "m"))
    ldm = hip.skd_pairwise_ldm(m)
    assert ldm == m
    nrm = torch.ones(b, m, device=DEV)
    return [("skd_pairwise_split_backward", TP.backward(hip, True, (b, cs, 0, m), ldm, built.a.to(DEV), built.b.to(DEV), nrm, gl=1.0).cpu())]


RUN = {"conv1x1": _conv1x1, "conv1x1_pro": _conv1x1_pro, "conv3x3": _conv3x3, "conv3x3_res": _conv3x3_res, "narrow": _narrow,
       "dgrad": _dgrad, "narrow_dgrad": _narrow_dgrad, "s2": _s2, "wgrad": _wgrad_with(TW, "skd_conv3x3_split_wgrad_nhwc"),
       "narrow_wgrad": _wgrad_with(TNW, "skd_conv3x3_narrow_wgrad_nhwc"), "train_fwd": _train_fwd, "train_dgrad": _train_dgrad,
       "train_wgrad": _train_wgrad, "gram": _gram, "pair_bwd": _pair_bwd}
# the entries each group must have launched: a case cannot go green on fewer
ENTRIES = {"train_fwd": {"128-64-13x11-s1": 1, "64-128-13x11-s2": 2, "128-256-9x9-s1": 2},
           "train_dgrad": {"128-64-13x11-s1": 2, "64-128-13x11-s2": 1, "128-256-9x9-s1": 2}}


def test_every_group_has_a_launcher():
    assert set(RUN) == set(X.GROUPS)


@pytest.mark.parametrize("case", X.CASES, ids=[c.name for c in X.CASES])
def test_six_products_exact(hip, case):
    built = X.build(case)
    want = built.exact()
    outs = RUN[case.group](hip, case, built)
    assert len(outs) == ENTRIES.get(case.group, {}).get(case.tag, len(outs)) and outs
    for label, got in outs:
        got = got.double()
        assert got.shape == want.shape, (label, got.shape, want.shape)
        same = torch.equal(built.checked(got), built.checked(want))
        print("%s | %s: %s" % (case.name, label, "exact" if same else X.explain(got, built)))
        assert same, "%s | %s: %s" % (case.name, label, X.explain(got, built))
