"""OHEM criterion, the parts that need no GPU: the restatement (tests/ohem_ref.py) against the reference's recorded results
(tests/golden/reference_ohem.pt), against the live reference where its tree exists and against scipy's zoom; the C ABI of
include/skd_ohem.h (the pinned names and argument lists, host-side refusals); the module surface (constructor signatures,
refusals, the C double has no OHEM entries); NetModel's choice of criterion.

Bounds.  ``tau`` (stored by the generator: 4 x the largest difference between the reference's fp32 label probability and the
restatement's float64 one) is the distance from the threshold within which two evaluations may disagree about a pixel; farther
away they must agree.  On the reference's own mask the float64 loss and gradients are within 1e-6 (relative) of the recorded
fp32 ones, the bound the generator itself held before writing the fixture."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

from oracle import abn_torch, cref, ref_import
from structure_knowledge_distillation_amd import _lib, build
from structure_knowledge_distillation_amd import functional as SF
from structure_knowledge_distillation_amd.utils import criterion as CR

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(HERE, "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)
import ohem_ref as R  # noqa: E402

GOLD = os.path.join(HERE, "golden", "reference_ohem.pt")
_cache = {}


def gold():
    if "g" not in _cache:
        g = torch.load(GOLD, weights_only=False)
        for c in g["cases"]:
            B, H, W = c["target"].shape
            c["kept"] = np.unpackbits(c["kept_bits"].numpy())[:B * H * W].reshape(B, H, W).astype(bool)
            c["target64"] = c["target"].long()
        g["by_name"] = {c["name"]: c for c in g["cases"]}
        _cache["g"] = g
    return _cache["g"]


def gen():
    import make_golden_ohem
    return make_golden_ohem


def restate(c, **kw):
    """The restatement on a fixture case (cached for the default arguments: the GPU tests share it)."""
    key = ("own", c["name"]) if not kw else None
    if key and key in _cache:
        return _cache[key]
    dsn = None if c["logits_dsn"] is None else c["logits_dsn"].numpy()
    r = R.ohem(c["logits_main"].numpy(), dsn, c["target64"].numpy(), gold()["ignore_index"], c["thresh"], c["min_kept"],
               c["factor"], 0.4, **kw)
    if key:
        _cache[key] = r
    return r


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


CASE_NAMES = ["kth", "thresh", "all_kept", "zero_lines", "half_even", "one_row", "single_head"]


# ---- 1. the restatement ----------------------------------------------------------------------------------------------------

def test_fixture_covers_the_branches():
    G = gold()
    assert [c["name"] for c in G["cases"]] == CASE_NAMES
    assert {c["branch"] for c in G["cases"]} == {"kth", "thresh", "one"}
    assert 0 < G["eps32"] < 2e-6 and G["tau"] == 4 * G["eps32"]
    by = G["by_name"]
    assert by["thresh"]["threshold"] == float(np.float32(0.7)) and by["all_kept"]["threshold"] == 1.0
    assert by["kth"]["branch"] == "kth" and by["kth"]["threshold"] > 0.2
    assert (R.zoom_size(100, 8), R.zoom_size(72, 8), R.zoom_size(512, 8)) == (12, 9, 64)   # half to even both ways
    assert os.path.getsize(GOLD) <= 1 << 20


@pytest.mark.parametrize("name", CASE_NAMES)
def test_restatement_vs_reference_fixture(name):
    G = gold()
    c, tau = G["by_name"][name], G["tau"]
    own = restate(c)
    valid = c["target64"].numpy() != G["ignore_index"]
    assert own.num_valid == c["num_valid"]
    if c["branch"] == "kth":
        assert abs(float(own.threshold) - c["threshold"]) <= tau
    else:
        assert float(own.threshold) == c["threshold"]
    near = valid & (np.abs(own.p_label - c["threshold"]) <= tau)
    assert int(near.sum()) == c["near"] <= 1e-3 * valid.sum()
    assert np.array_equal(own.own_kept[~near], c["kept"][~near])
    assert int((own.own_kept != c["kept"]).sum()) <= c["near"]
    assert not c["kept"][~valid].any() and int(c["kept"].sum()) == c["n_kept"]
    # the loss and the gradients on the reference's own mask
    on = own if np.array_equal(own.own_kept, c["kept"]) else restate(c, kept=c["kept"])
    assert abs(on.loss - c["loss"]) <= 1e-6 * abs(c["loss"])
    assert rel(on.grad_main, c["grad_main"].numpy()) <= 1e-6
    if c["two"]:
        assert rel(on.grad_dsn, c["grad_dsn"].numpy()) <= 1e-6
    if name == "zero_lines":
        keys = own.pred_ds
        assert (keys[:, -1, :] == 0).all() and (keys[:, :, -1] == 0).all() and (keys[:, :-1, :-1] > 0).any()
    if name == "one_row":
        assert valid.sum() == c["target"].shape[2] and c["num_valid"] > 0


@pytest.mark.reference
@pytest.mark.skipif(not ref_import.reference_available(), reason="reference tree not present")
@pytest.mark.parametrize("index", [0, 5, 6])
def test_restatement_vs_live_reference(index):
    """The reference class, unchanged, on the generator's inputs: fed the reference's own fp32 softmax the restatement gives
    its threshold and its mask exactly, and the recorded fixture is what the reference still computes."""
    mod, G = gen(), gold()
    ns = ref_import.load_reference(abn_torch)
    r = mod.run_reference(ns, mod.CASES[index])
    c = G["cases"][index]
    dsn = None if r["logits_dsn"] is None else r["logits_dsn"].numpy()
    exact = R.ohem(r["logits_main"].numpy(), dsn, r["target"].numpy(), mod.IGNORE, r["thresh"], r["min_kept"], r["factor"], 0.4,
                   probs32=r["prob"])
    assert exact.threshold == r["threshold"] and np.array_equal(exact.kept, r["kept"])
    assert abs(exact.loss - r["loss"]) <= 1e-6 * abs(r["loss"])
    assert torch.equal(r["logits_main"], c["logits_main"]) and torch.equal(r["target"], c["target64"])
    assert abs(float(r["threshold"]) - c["threshold"]) <= G["tau"] and abs(r["loss"] - c["loss"]) <= 1e-6 * abs(c["loss"])


@pytest.mark.parametrize("factor", [2, 4, 8])
def test_zoom_rules_vs_scipy_every_axis_length(factor):
    """Order 0 and order 1 of the restatement against scipy.ndimage.zoom for every axis length 16 .. 200, along X (2 x n) and
    along Y (n x 2): the same size, the same values (the sign of a zero is not compared), scipy's zeroed last lines."""
    nd = pytest.importorskip("scipy.ndimage")
    rng = np.random.RandomState(factor)
    zeroed = 0
    for n in range(16, 201):
        m = R.zoom_size(n, factor)
        p = rng.rand(2, n).astype(np.float32)
        t = rng.randint(1, 20, size=(2, n)).astype(np.int64)        # labels >= 1: a zeroed line shows
        for axis in (1, 0):
            pa, ta = (p, t) if axis == 1 else (p.T.copy(), t.T.copy())
            zoom = (1.0, 1.0 / factor) if axis == 1 else (1.0 / factor, 1.0)
            want1, want0 = nd.zoom(pa, zoom, order=1), nd.zoom(ta, zoom, order=0)
            shape = (2, m) if axis == 1 else (m, 2)
            assert want1.shape == want0.shape == shape, (n, factor)
            got1, got0 = R.zoom_linear(pa, *shape), R.zoom_nearest(ta, *shape)
            assert got1.dtype == np.float32 and np.array_equal(got1, want1), (n, factor, axis)
            assert np.array_equal(got0, want0), (n, factor, axis)
            zeroed += int((want0 == 0).any())
    assert zeroed > 0 or factor == 2, "no length with a zeroed last line at this factor"
    assert (nd.zoom(np.ones((256, 2), np.int64), (1 / 8, 1), order=0)[-1] == 0).all()      # 256 -> 32 is one (the fixture's case)


# ---- 2. the C ABI ----------------------------------------------------------------------------------------------------------

OHEM_ENTRIES = ["skd_ce_ohem_dsn_forward", "skd_ce_ohem_workspace_floats", "skd_ohem_threshold"]


def test_ohem_header_table_and_library_agree():
    """What is particular to skd_ohem.h; header <-> table <-> library <-> build digest: tests/test_abi.py, for every header."""
    assert sorted(_lib.ABI["skd_ohem.h"]) == OHEM_ENTRIES
    assert os.path.join(build.CSRC, "ce_ohem.hip") in build.sources()


def test_ohem_host_side_refusals_and_workspace_size():
    lib = _lib.load()
    wsf = lib.skd_ce_ohem_workspace_floats
    assert wsf(0, 19, 9, 17, 64, 128, 8) == 8 and wsf(2, 19, 9, 17, 64, 128, 8) >= lib.skd_ce_dsn_workspace_floats(2, 19, 9, 17, 64, 128)
    # full-resolution logits with few classes: the keys outgrow nothing, the main pass's partials still fit
    assert wsf(1, 1, 1, 1, 512, 512, 1) >= 512 * 512
    t = lib.skd_ohem_threshold
    ok = dict(B=2, C=19, h=9, w=17, H=64, W=128, lm=1, tg=1, ig=255, th=0.7, mk=100, f=8, thr=1, nv=1, keys=None, ws=1, st=None)

    def call(**kw):
        a = dict(ok, **kw)
        return t(a["B"], a["C"], a["h"], a["w"], a["H"], a["W"], a["lm"], a["tg"], a["ig"], a["th"], a["mk"], a["f"], a["thr"],
                 a["nv"], a["keys"], a["ws"], a["st"])
    for bad in (dict(B=0), dict(C=0), dict(C=65), dict(h=0), dict(W=-1), dict(lm=None), dict(tg=None), dict(thr=None), dict(nv=None),
                dict(ws=None), dict(f=0), dict(mk=-1), dict(H=8, f=8), dict(W=11, f=8), dict(H=3, f=8)):
        assert call(**bad) == 0, bad
    f = lib.skd_ce_ohem_dsn_forward
    assert f(2, 19, 9, 17, 64, 128, 1, 1, 1, 255, 0.4, None, 1, None, None, None, None, 1, None) == 0       # no threshold
    assert f(2, 65, 9, 17, 64, 128, 1, 1, 1, 255, 0.4, 1, 1, None, None, None, None, 1, None) == 0
    assert f(2, 19, 9, 17, 64, 128, 1, None, 1, 255, 0.4, 1, 1, None, None, None, 1, 1, None) == 0          # grad_dsn without dsn
    assert f(2, 19, 9, 17, 64, 128, 1, 1, 1, 255, 0.4, 1, None, None, None, None, None, 1, None) == 0
    assert f(2, 19, 9, 17, 64, 128, 1, 1, 1, 255, 0.4, 1, 1, None, None, None, None, None, None) == 0


# ---- 3. the module surface ---------------------------------------------------------------------------------------------------

def test_constructor_signatures_equal_the_references():
    G = gold()
    for name in ("OhemCrossEntropy2d", "CriterionOhemDSN"):
        ours = str(inspect.signature(getattr(CR, name).__init__))
        assert ours == G["signatures"][name], (name, ours)
    if ref_import.reference_available():
        ns = ref_import.load_reference(abn_torch)
        for name in ("OhemCrossEntropy2d", "CriterionOhemDSN"):
            assert inspect.signature(getattr(CR, name).__init__) == inspect.signature(getattr(ns.criterion, name).__init__)
    o = CR.OhemCrossEntropy2d()
    assert (o.ignore_label, o.thresh, o.min_kept, o.factor) == (255, 0.7, 100000, 8)
    assert isinstance(o.thresh, float) and isinstance(CR.OhemCrossEntropy2d(min_kept=5.0).min_kept, int)
    d = CR.CriterionOhemDSN(ignore_index=7, thresh=0.5, min_kept=10)
    assert d.ignore_index == 7 and (d.criterion1.ignore_label, d.criterion1.thresh, d.criterion1.min_kept) == (7, 0.5, 10)
    assert d.criterion1.factor == 8 and callable(o.find_threshold)
    assert "out of scope" not in CR.__doc__


def test_refusals_of_the_modules(capsys):
    with pytest.raises(NotImplementedError, match="reduce=False"):
        CR.CriterionOhemDSN(reduce=False)
    with pytest.raises(NotImplementedError, match="weight"):
        CR.OhemCrossEntropy2d()(torch.zeros(1, 3, 16, 16), torch.zeros(1, 16, 16, dtype=torch.int64), weight=torch.ones(3))
    CR.CriterionOhemDSN()
    assert capsys.readouterr().out == ""                      # neither class prints


def test_plain_c_double_has_no_ohem_entries():
    prev = _lib._test_backend
    _lib.install_test_backend(cref.load(_lib.SIGNATURES))
    try:
        lm, tg = torch.zeros(1, 3, 4, 4, requires_grad=True), torch.zeros(1, 16, 16, dtype=torch.int64)
        with pytest.raises(NotImplementedError, match="skd_ce_ohem_workspace_floats|skd_ohem_threshold"):
            SF.ce_ohem_dsn(lm, lm, tg)
        with pytest.raises(NotImplementedError, match="skd_"):
            CR.CriterionOhemDSN()([lm, lm], tg)
        with pytest.raises(NotImplementedError, match="skd_"):
            CR.OhemCrossEntropy2d().find_threshold(np.zeros((1, 3, 16, 16), np.float32), np.zeros((1, 16, 16), np.int64))
        with pytest.raises(NotImplementedError, match="skd_ohem_threshold|skd_ce_ohem_workspace_floats"):
            SF.ohem_threshold(lm, tg)
    finally:
        _lib.install_test_backend(prev)


def test_argument_checks_of_the_op():
    prev = _lib._test_backend                                 # a back-end that has the entries and may not be called: the checks come first
    _lib.install_test_backend(type("B", (), {n: staticmethod(lambda *a: 1 / 0) for n in _lib.ABI["skd_ohem.h"]})())
    try:
        lm, tg = torch.zeros(1, 3, 4, 4), torch.zeros(1, 16, 16, dtype=torch.int64)
        with pytest.raises(TypeError):
            SF.ce_ohem_dsn(lm.double(), None, tg)
        with pytest.raises(TypeError):
            SF.ce_ohem_dsn(lm, None, tg.int())
        with pytest.raises(ValueError):
            SF.ce_ohem_dsn(lm, torch.zeros(1, 3, 5, 4), tg)
        with pytest.raises(ValueError):
            SF.ce_ohem_dsn(lm, None, tg[0])
        with pytest.raises(ValueError):
            SF.ce_ohem_dsn(lm, None, tg, factor=0)
        with pytest.raises(ValueError, match="down-samples to 1"):
            SF.ce_ohem_dsn(lm, None, tg, factor=16)
        with pytest.raises(ValueError):
            SF.ce_ohem_dsn(lm, None, tg, min_kept=-1)
        with pytest.raises(ValueError):
            SF.ce_ohem_dsn(torch.zeros(1, 65, 4, 4), None, tg)
    finally:
        _lib.install_test_backend(prev)


# ---- 4. NetModel ---------------------------------------------------------------------------------------------------------

def test_netmodel_picks_the_criterion_by_the_flag():
    from structure_knowledge_distillation_amd.networks.kd_model import NetModel, default_args
    a = default_args()
    assert a.ohem is False and a.ohem_thresh == 0.7 and a.ohem_keep == 100000
    prev = _lib._test_backend
    _lib.install_test_backend(cref.load(_lib.SIGNATURES))
    try:
        kw = dict(device=torch.device("cpu"), batch_size=2, ho=False)
        plain = NetModel(default_args(**kw))
        assert type(plain.criterion.module) is CR.CriterionDSN
        mined = NetModel(default_args(ohem=True, ohem_thresh=0.6, ohem_keep=5000, **kw))
        assert type(mined.criterion.module) is CR.CriterionOhemDSN
        c1 = mined.criterion.module.criterion1
        assert (c1.thresh, c1.min_kept, c1.factor, c1.ignore_label) == (0.6, 5000, 8, 255)
    finally:
        _lib.install_test_backend(prev)
