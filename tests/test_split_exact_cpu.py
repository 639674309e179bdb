"""The case table of tests/split_exact.py on the CPU: what tests/test_split_exact_gpu.py asserts with equality on the GPU is only
worth something if, for every case, (1) no partial sum can leave the exact fp32 integers, (2) the operands are of the classes
they claim, (3) the six-product model is the exact product, (4) every product the case is meant to pin changes at least a quarter
of the checked outputs when dropped and every other one changes none, and over a case triple all five lower products are pinned,
and (5) in a GEMM-shaped case every k mod 16 and every K-tile carries a T / W value in some row of each 64-row block.
Every figure is printed in front of its assertion (profiles/r30_split_exact.md tabulates them).
"""
import pytest
import torch

import split2_ref as R
import split_exact as X

IDS = [c.name for c in X.CASES]
MIN_SHARE = 0.25


def shares(built):
    """{(i, j): share of the checked outputs that dropping a_i b_j changes} for the five lower products."""
    full = built.powered(built.model())
    return {p: float((built.powered(built.model(p)) != full).double().mean()) for p in X.LOWER}


@pytest.mark.parametrize("case", X.CASES, ids=IDS)
def test_bound_below_two_to_the_24(case):
    built = X.build(case)
    worst = float(built.checked(built.abs_bound()).max()) / X.LIMIT
    print("%s: largest sum of absolute piece products = %.3f * 2^24" % (case.name, worst))
    assert 0 < worst < 1
    if built.mask is not None:
        assert float(built.mask.double().mean()) >= 0.75, "at least 3/4 of G is checked"


@pytest.mark.parametrize("case", X.CASES, ids=IDS)
def test_operand_classes(case):
    built = X.build(case)
    assert {cls for cls, _ in built.rows} >= set(case.kind)      # (the Gram's teacher panel is narrow in every run)
    for cls, t in built.rows:
        assert bool((t == t.round()).all()), "integers"
        p = R.pieces(t, 3)
        assert torch.equal(p[0] + p[1] + p[2], t.double()), "three pieces hold the value"
        nz = t != 0
        assert int(nz.sum()) > 0
        if cls == "W":
            assert bool((p[1][nz] != 0).all()) and bool((p[2][nz] != 0).all())
            assert float(t[nz].abs().min()) >= 2 ** 18 and float(t.abs().max()) < 2 ** 19
        elif cls == "T":
            assert bool((p[1][nz] != 0).all()) and bool((p[2] == 0).all())
            assert float(t[nz].abs().min()) >= 2 ** 8 and float(t.abs().max()) < 2 ** 10 and bool((t[nz] % 2 == 1).all())
        else:
            assert bool((p[1] == 0).all()) and bool((p[2] == 0).all()) and float(t.abs().max()) <= 3


@pytest.mark.parametrize("case", X.CASES, ids=IDS)
def test_model_is_the_exact_product(case):
    built = X.build(case)
    exact = built.exact()
    assert torch.equal(built.checked(built.model()), built.checked(exact))
    assert bool((exact == exact.round()).all()) or built.scale != 1.0
    assert float(built.checked(exact).abs().max()) > 100.0 * abs(built.scale)
    assert X.explain(exact, built) == "equals the exact product"
    if case.builder == "gram":
        assert torch.equal(exact, exact.transpose(1, 2))


@pytest.mark.parametrize("case", X.CASES, ids=IDS)
def test_power(case):
    built = X.build(case)
    got = shares(built)
    print("%s: %s" % (case.name, "  ".join("a%d.b%d %.3f" % (p + (s,)) for p, s in got.items())))
    for p, share in got.items():
        if p in X.PINS[case.kind]:
            assert share >= MIN_SHARE, "dropping a%d.b%d changes only %.3f of the checked outputs" % (p + (share,))
        else:
            assert share == 0.0, "a%d.b%d is not what this run pins, yet dropping it changes outputs" % p
    # explain names the product of a model that lost one
    p = X.PINS[case.kind][0]
    assert "WITHOUT a%d.b%d" % p in X.explain(built.model(p), built)


@pytest.mark.parametrize("triple", X.TRIPLES)
def test_every_lower_product_is_pinned_by_the_triple(triple):
    cases = [c for c in X.CASES if c.triple == triple]
    assert sorted(c.kind for c in cases) == sorted(X.KINDS)
    pinned = {p for c in cases for p, s in shares(X.build(c)).items() if s >= MIN_SHARE}
    assert pinned == set(X.LOWER)


@pytest.mark.parametrize("case", [c for c in X.CASES if c.group in X.GEMM_SHAPED], ids=lambda c: c.name)
def test_gemm_coverage(case):
    """Every k mod 16 and every K-tile carries a T / W value in some row of each 64-row block of each such panel (a last block
    of fewer rows is not asked; a panel of fewer than 64 rows is one block)."""
    built = X.build(case)
    assert built.panels
    for panel in built.panels:
        rows, k = panel.shape
        blocks = [panel[r:r + 64] for r in range(0, rows - 63, 64)] or [panel]
        for blk in blocks:
            ks = torch.nonzero((blk != 0).any(0)).flatten()
            assert set((ks % 16).tolist()) == set(range(min(16, k))), "a k mod 16 without a value"
            assert set((ks // 16).tolist()) == set(range(-(-k // 16))), "a K-tile without a value"


def test_every_family_is_in_the_table():
    assert set(X.GROUPS) == {"conv1x1", "conv1x1_pro", "conv3x3", "conv3x3_res", "narrow", "dgrad", "narrow_dgrad", "s2", "wgrad",
                             "narrow_wgrad", "train_fwd", "train_dgrad", "train_wgrad", "gram", "pair_bwd"}
    assert len(X.CASES) == 3 * len(X.TRIPLES) and len({c.name for c in X.CASES}) == len(X.CASES)


def test_abs_bound_uses_the_absolute_pieces():
    """The pieces are signed: their magnitudes add up to more than |a|, and the bound must use them."""
    a = torch.tensor([[383.0]])           # 384 - 1: p0 = 384, p1 = -1
    b = torch.tensor([[1.0]])
    assert float(X.abs_bound(X.gemm_op, a, b)) == 385.0
    x = torch.full((1, 1, 3, 3), 383.0)
    w = torch.ones(1, 1, 3, 3)
    assert float(X.abs_bound(X.conv_op(1, 1, 1), x, w)[0, 0, 1, 1]) == 9 * 385.0
