"""OHEM criterion on the GPU (csrc/ce_ohem.hip), through the C ABI of include/skd_ohem.h and through the modules: every case of
tests/golden/reference_ohem.pt (the reference's own run) and one full-size case against a torch composition on the same GPU.
None of these can pass without the kernels.  No test double may be active here.

Bounds.  ``tau`` comes from the fixture (4 x the measured difference between the reference's fp32 label probability and the
float64 restatement's): the keys and a k-th threshold lie within ``tau`` of the restatement's, a ``thresh`` / 1.0 threshold is
the same bits, and the kept mask equals the restatement's at every pixel farther than ``tau`` from the threshold -- at most the
``near`` pixels the fixture counted may differ.  Loss and gradients are compared with the restatement evaluated ON THE MASK THE
KERNEL CHOSE (a pixel within rounding of the threshold may fall either way; tests/kinks.py), with test_ce_dsn's bounds: 1e-5 of
the loss, 5e-5 of the largest gradient element.  When the masks are equal the loss is also within 1e-4 (relative) of the loss the
reference recorded."""
import os
import sys

import numpy as np
import pytest
import torch

from structure_knowledge_distillation_amd import _lib
from structure_knowledge_distillation_amd.utils import criterion as CR

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import bounds_cases as BC  # noqa: E402  (Arena: guard-banded buffers)
import ohem_ref as R  # noqa: E402
import test_ohem_cpu as CPU  # noqa: E402  (shared helpers: fixture loading, the cached restatement)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
P = BC.P
LOSS_TOL, GRAD_TOL, PARITY = 1e-5, 5e-5, 1e-4


@pytest.fixture(autouse=True)
def no_test_double():
    prev = _lib._test_backend
    _lib.install_test_backend(None)
    yield
    _lib.install_test_backend(prev)


def close(got, want, tol, what):
    """max |got - want| <= tol * max |want| (tests/test_kernels_gpu.py)."""
    got, want = torch.as_tensor(got).detach().cpu().double().reshape(-1), torch.as_tensor(want).detach().cpu().double().reshape(-1)
    scale = max(float(want.abs().max()), 1e-30)
    err = float((got - want).abs().max()) / scale
    print("%s: max err %.3e of %.3e (bound %.1e)" % (what, err, scale, tol))
    assert err <= tol, "%s: max err %.3e (rel to %.3e) > %.1e" % (what, err, scale, tol)


class Plain:
    """The Arena's interface on ordinary tensors (workspace filled with NaN bytes all the same)."""

    def inp(self, name, data, row=None):
        return None if data is None else data.to(DEV)

    def out(self, name, shape, dtype=torch.float32, row=None):
        return _filled(shape, dtype)

    def ws(self, name, n):
        return _filled((int(n),), torch.float32)

    def check(self):
        torch.cuda.synchronize()


def _filled(shape, dtype):
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    return torch.full((n,), 0xFF, dtype=torch.uint8, device=DEV).view(dtype).view(shape)


def run_abi(A, lm0, ld0, tg0, thresh, min_kept, factor, ignore=255, grads=True, want_keys=True, want_kept=True, ws=None):
    """Both entries on one workspace of exactly the queried size, 0xFF-filled.  Returns a dict of host results."""
    lib = _lib.load()
    B, C, h, w = lm0.shape
    H, W = tg0.shape[1:]
    Hd, Wd = R.zoom_size(H, factor), R.zoom_size(W, factor)
    lm, ld, tg = A.inp("logits_main", lm0, row=w), A.inp("logits_dsn", ld0, row=w), A.inp("target", tg0, row=W)
    thr, nv = A.out("threshold", (1,)), A.out("num_valid", (1,), torch.int32)
    keys = A.out("pred_ds", (B, Hd, Wd), row=Wd) if want_keys else None
    if ws is None:
        ws = A.ws("workspace", lib.skd_ce_ohem_workspace_floats(B, C, h, w, H, W, factor))
    assert lib.skd_ohem_threshold(B, C, h, w, H, W, P(lm), P(tg), ignore, thresh, min_kept, factor, P(thr), P(nv), P(keys), P(ws),
                                  None) == 1
    loss, nk = A.out("loss", (1,)), A.out("n_kept", (1,))
    kept = A.out("kept", (B, H, W), torch.uint8, row=W) if want_kept else None
    gm = A.out("grad_main", (B, C, h, w), row=w) if grads else None
    gd = A.out("grad_dsn", (B, C, h, w), row=w) if grads and ld is not None else None
    assert lib.skd_ce_ohem_dsn_forward(B, C, h, w, H, W, P(lm), P(ld), P(tg), ignore, 0.4, P(thr), P(loss), P(nk), P(kept), P(gm),
                                       P(gd), P(ws), None) == 1
    A.check()
    host = lambda t: None if t is None else t.cpu().clone()
    return dict(threshold=host(thr), num_valid=int(nv.cpu()), pred_ds=host(keys), loss=host(loss), n_kept=host(nk), kept=host(kept),
                grad_main=host(gm), grad_dsn=host(gd), ws=ws)


def check_case(c, got, G):
    """The assertions of the module docstring for one fixture case."""
    tau = G["tau"]
    own = CPU.restate(c)
    th_gpu = float(got["threshold"])
    # keys: within tau, ignored positions equal, none left unwritten
    keys = got["pred_ds"].numpy()
    assert not np.isnan(keys).any(), "a key was left unwritten"
    assert np.array_equal(keys == -1, own.pred_ds == -1)
    kerr = float(np.abs(keys.astype(np.float64) - own.pred_ds.astype(np.float64)).max())
    print("%s: keys max err %.3e (tau %.3e), threshold gpu %.9g fixture %.9g" % (c["name"], kerr, tau, th_gpu, c["threshold"]))
    assert kerr <= tau
    assert got["num_valid"] == c["num_valid"]
    if c["branch"] == "kth":
        assert abs(th_gpu - c["threshold"]) <= tau
    else:
        assert th_gpu == c["threshold"]                    # float32(thresh) / 1.0f: the same bits
    # the mask
    valid = c["target64"].numpy() != G["ignore_index"]
    near = valid & (np.abs(own.p_label - c["threshold"]) <= tau)
    kept = got["kept"].numpy()
    assert set(np.unique(kept)) <= {0, 1}, "a mask byte was left unwritten"
    kept = kept.astype(bool)
    assert not kept[~valid].any()
    assert np.array_equal(kept[~near], own.own_kept[~near])
    differing = int((kept != own.own_kept).sum())
    print("%s: %d mask pixels differ from the restatement's (%d within tau of the threshold)" % (c["name"], differing, c["near"]))
    assert differing <= c["near"]
    assert float(got["n_kept"]) == kept.sum()
    # loss and gradients on the kernel's mask
    on = own if np.array_equal(kept, own.own_kept) else CPU.restate(c, kept=kept)
    close(got["loss"], [on.loss], LOSS_TOL, c["name"] + " loss")
    if got["grad_main"] is not None:
        close(got["grad_main"], on.grad_main, GRAD_TOL, c["name"] + " grad main")
    if got["grad_dsn"] is not None:
        close(got["grad_dsn"], on.grad_dsn, GRAD_TOL, c["name"] + " grad dsn")
    if np.array_equal(kept, c["kept"]):
        assert abs(float(got["loss"]) - c["loss"]) <= PARITY * abs(c["loss"])


def case_inputs(c):
    return c["logits_main"], c["logits_dsn"], c["target64"], c["thresh"], c["min_kept"], c["factor"]


# ---- 1. the C ABI against the reference's fixture ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", CPU.CASE_NAMES)
def test_ohem_entries_vs_reference_fixture(name):
    G = CPU.gold()
    c = G["by_name"][name]
    got = run_abi(Plain(), *case_inputs(c))
    check_case(c, got, G)
    if name == "zero_lines":
        keys = got["pred_ds"].numpy()
        assert (keys[:, -1, :] == 0).all() and (keys[:, :, -1] == 0).all()


def test_special_cases():
    """Gradient pointers NULL; twice on the same dirty workspace; every pixel ignored; a label out of range."""
    G = CPU.gold()
    c = G["by_name"]["kth"]
    first = run_abi(Plain(), *case_inputs(c))
    # loss only, no keys, no mask, on the workspace the first call left behind: the same bits
    again = run_abi(Plain(), *case_inputs(c), grads=False, want_keys=False, want_kept=False, ws=first["ws"])
    assert again["grad_main"] is None and again["pred_ds"] is None
    for k in ("threshold", "loss", "n_kept"):
        assert torch.equal(again[k], first[k]), k
    assert again["num_valid"] == first["num_valid"]
    # everything again with gradients on that workspace: bit-equal results
    third = run_abi(Plain(), *case_inputs(c), ws=first["ws"])
    for k in ("threshold", "loss", "n_kept", "pred_ds", "kept", "grad_main", "grad_dsn"):
        assert torch.equal(third[k], first[k]), k
    # main gradient only
    lib = _lib.load()
    lm, ld, tg, thresh, min_kept, factor = case_inputs(c)
    B, Cc, h, w = lm.shape
    H, W = tg.shape[1:]
    lmg, ldg, tgg = lm.to(DEV), ld.to(DEV), tg.to(DEV)
    thr, loss, gm = first["threshold"].to(DEV), _filled((1,), torch.float32), _filled(lm.shape, torch.float32)
    assert lib.skd_ce_ohem_dsn_forward(B, Cc, h, w, H, W, P(lmg), P(ldg), P(tgg), 255, 0.4, P(thr), P(loss), None, None, P(gm), None,
                                       P(first["ws"]), None) == 1
    assert torch.equal(loss.cpu(), first["loss"]) and torch.equal(gm.cpu(), first["grad_main"])
    # every pixel ignored: num_valid 0 -> threshold 1.0, no kept pixel -> 0 / 0 = NaN like CrossEntropyLoss
    none = run_abi(Plain(), lm, ld, torch.full_like(tg, 255), thresh, min_kept, factor)
    assert none["num_valid"] == 0 and float(none["threshold"]) == 1.0 and float(none["n_kept"]) == 0
    assert bool((none["pred_ds"] == -1).all()) and not bool(none["kept"].any())
    assert bool(torch.isnan(none["loss"]).all()) and bool(torch.isnan(none["grad_main"]).all())
    # a label outside [0, C) that is not the ignore value: NaN loss, NaN kept count, NaN gradients
    bad = tg.clone()
    bad[0, H - 1, W // 2] = Cc + 3
    out = run_abi(Plain(), lm, ld, bad, thresh, min_kept, factor)
    assert bool(torch.isnan(out["loss"]).all()) and bool(torch.isnan(out["n_kept"]).all())
    assert bool(torch.isnan(out["grad_main"]).all()) and bool(torch.isnan(out["grad_dsn"]).all())
    assert not bool(torch.isnan(out["threshold"]).any())
    torch.cuda.synchronize()
    assert _lib.device_status() == [0] * lib.skd_status_words()


# ---- 2. guard bands --------------------------------------------------------------------------------------------------------

GUARD_CASES = {
    "half_even-two-heads": (("skd_ohem_threshold", "skd_ce_ohem_dsn_forward"), "half_even"),
    "zero_lines-two-heads": (("skd_ohem_threshold", "skd_ce_ohem_dsn_forward"), "zero_lines"),
    "single-head": (("skd_ohem_threshold", "skd_ce_ohem_dsn_forward"), "single_head"),
}


@pytest.mark.parametrize("name", list(GUARD_CASES))
def test_entries_stay_inside_their_buffers(name):
    """Inputs, outputs and a workspace of exactly the queried size between 0xFF guard bands, outputs and workspace pre-filled
    with 0xFF: no guard byte changes, no output element is left unwritten, values as in the restatement."""
    G = CPU.gold()
    c = G["by_name"][GUARD_CASES[name][1]]
    lib = _lib.load()
    got = run_abi(BC.Arena("cuda"), *case_inputs(c))
    check_case(c, got, G)
    for k in ("grad_main", "grad_dsn", "loss", "n_kept", "threshold"):
        assert got[k] is None or not bool(torch.isnan(got[k]).any()), k
    torch.cuda.synchronize()
    assert _lib.device_status() == [0] * lib.skd_status_words()


def test_every_pointer_taking_ohem_entry_has_a_guard_band_case():
    covered = {e for entries, _ in GUARD_CASES.values() for e in entries}
    pointer_taking = {n for n, (_, args) in _lib.ABI["skd_ohem.h"].items() if _lib.ctypes.c_void_p in args}
    assert covered == pointer_taking == {"skd_ohem_threshold", "skd_ce_ohem_dsn_forward"}


# ---- 3. the modules ----------------------------------------------------------------------------------------------------------

def module_case(c):
    lm = c["logits_main"].to(DEV).requires_grad_(True)
    ld = c["logits_dsn"].to(DEV).requires_grad_(True)
    crit = CR.CriterionOhemDSN(thresh=c["thresh"], min_kept=c["min_kept"]).to(DEV)
    return crit, lm, ld, c["target64"].to(DEV)


def test_criterion_ohem_dsn_module_forward_backward():
    G = CPU.gold()
    c = G["by_name"]["kth"]
    crit, lm, ld, tg = module_case(c)
    loss = crit([lm, ld], tg)
    (loss * 2.0).backward()
    assert loss.dim() == 0 and crit.criterion1.last_threshold.is_cuda and crit.criterion1.last_kept.dim() == 0
    assert abs(float(crit.criterion1.last_threshold) - c["threshold"]) <= G["tau"]
    n_kept = float(crit.criterion1.last_kept)
    assert abs(n_kept - c["n_kept"]) <= c["near"]
    # the module gives no mask: take the one the C ABI gives on the same inputs (the same kernels: the kept counts must agree)
    abi = run_abi(Plain(), *case_inputs(c))
    assert float(abi["n_kept"]) == n_kept and torch.equal(abi["loss"].reshape(()), loss.detach().cpu())
    kept = abi["kept"].numpy().astype(bool)
    if np.array_equal(kept, c["kept"]):                    # the reference's own mask: the reference's own numbers
        assert abs(float(loss.detach()) - c["loss"]) <= PARITY * abs(c["loss"])
        close(lm.grad, 2.0 * c["grad_main"], GRAD_TOL, "module grad main vs reference")
        close(ld.grad, 2.0 * c["grad_dsn"], GRAD_TOL, "module grad dsn vs reference")
    own = CPU.restate(c)
    on = own if np.array_equal(kept, own.own_kept) else CPU.restate(c, kept=kept)      # always: the restatement on that mask
    close(loss.reshape(1), [on.loss], LOSS_TOL, "module loss")
    close(lm.grad, 2.0 * on.grad_main, GRAD_TOL, "module grad main")
    close(ld.grad, 2.0 * on.grad_dsn, GRAD_TOL, "module grad dsn")
    # the single-head class, and find_threshold (which may synchronise)
    s = G["by_name"]["single_head"]
    one = CR.OhemCrossEntropy2d(thresh=s["thresh"], min_kept=s["min_kept"], factor=s["factor"])
    x = s["logits_main"].to(DEV).requires_grad_(True)
    l1 = one(x, s["target64"].to(DEV))
    l1.backward()
    assert abs(float(l1.detach()) - s["loss"]) <= PARITY * abs(s["loss"])
    close(x.grad, s["grad_main"], GRAD_TOL, "single-head grad vs reference")
    th = one.find_threshold(s["logits_main"].numpy(), s["target64"].numpy())
    assert isinstance(th, float) and abs(th - s["threshold"]) <= G["tau"]
    # the reference's calling convention: the softmax as a numpy array (recognised as probabilities, not soft-maxed again)
    th_p = one.find_threshold(torch.softmax(s["logits_main"], 1).numpy(), s["target64"].numpy())
    assert isinstance(th_p, float) and abs(th_p - s["threshold"]) <= G["tau"]
    # no gradient wanted: loss only
    with torch.no_grad():
        assert float(crit([lm, ld], tg)) == float(loss.detach())


def test_training_path_does_not_synchronise():
    """criterion(preds, target).backward() with torch's synchronisation debug mode set to "error": any host read of a device
    value (an .item(), a .cpu(), a blocking copy) raises."""
    c = CPU.gold()["by_name"]["kth"]
    crit, lm, ld, tg = module_case(c)
    crit([lm, ld], tg).backward()                          # warm-up: module load, allocator
    lm.grad = ld.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = crit([lm, ld], tg)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(loss)) and lm.grad is not None and ld.grad is not None


# ---- 4. full size ----------------------------------------------------------------------------------------------------------

def test_full_size_vs_torch_composition():
    """(8, 19, 65, 65) -> (512, 512), defaults: the tile walk and the XCD order only exist at this size.  The yardstick is a torch
    composition on the same GPU: float64 up-sampling with the fp32 bilinear weights, float64 softmax rounded once to fp32, the
    zoom rules of tests/ohem_ref.py as gathers, torch.kthvalue; the kink rule as above."""
    G = CPU.gold()
    tau = G["tau"]
    B, C, h, w, H, W, factor, thresh, min_kept = 8, 19, 65, 65, 512, 512, 8, 0.7, 100000
    lm0, ld0, tg0 = CPU.gen().make_inputs((B, C, h, w), (H, W), 21)
    got = run_abi(Plain(), lm0, ld0, tg0, thresh, min_kept, factor)
    lm, ld, tg = lm0.to(DEV).double().requires_grad_(True), ld0.to(DEV).double().requires_grad_(True), tg0.to(DEV)
    My, Mx = R.upsample_matrix(h, H).to(DEV), R.upsample_matrix(w, W).to(DEV)
    up = lambda x: torch.log_softmax(torch.einsum("Yy,bcyx,Xx->bcYX", My, x, Mx), dim=1)
    logp = up(lm)
    valid = tg != 255
    idx = torch.where(valid, tg, torch.zeros_like(tg))
    p_label = logp.detach().gather(1, idx[:, None])[:, 0].exp()
    # the threshold at 1 / factor resolution
    Hd, Wd = R.zoom_size(H, factor), R.zoom_size(W, factor)
    y0, y1, wy0, wy1, ny, iny = [torch.from_numpy(np.asarray(a)).to(DEV) for a in R.zoom_axis(H, Hd)]
    x0, x1, wx0, wx1, nx, inx = [torch.from_numpy(np.asarray(a)).to(DEV) for a in R.zoom_axis(W, Wd)]
    inside = iny[:, None] & inx[None, :]
    label_ds = torch.where(inside, tg[:, ny][:, :, nx], torch.zeros((), dtype=tg.dtype, device=DEV))
    valid_ds = label_ds != 255
    cls = torch.where(valid_ds, label_ds, torch.zeros_like(label_ds))
    prob32 = logp.detach().exp().float()

    def at(ys, xs):
        return prob32[:, :, ys][:, :, :, xs].gather(1, cls[:, None])[:, 0].double()
    keys = (at(y0, x0) * wy0[:, None] * wx0[None, :] + at(y0, x1) * wy0[:, None] * wx1[None, :]
            + at(y1, x0) * wy1[:, None] * wx0[None, :] + at(y1, x1) * wy1[:, None] * wx1[None, :])
    keys = torch.where(inside, keys, torch.zeros_like(keys)).float()
    num_valid, mk = int(valid_ds.sum()), min_kept // (factor * factor)
    assert got["num_valid"] == num_valid and 0 < mk < num_valid
    kth = float(torch.kthvalue(keys[valid_ds], mk).values)
    want_keys = torch.where(valid_ds, keys, torch.full_like(keys, -1.0)).cpu()
    assert torch.equal(got["pred_ds"] == -1, want_keys == -1)
    kerr = float((got["pred_ds"].double() - want_keys.double()).abs().max())
    th_gpu = float(got["threshold"])
    print("full size: keys max err %.3e, k-th %.9g, threshold %.9g" % (kerr, kth, th_gpu))
    assert kerr <= tau
    if kth > float(np.float32(thresh)) + tau:
        assert abs(th_gpu - kth) <= tau
        th = kth
    else:
        assert kth < float(np.float32(thresh)) - tau, "the k-th key lies within tau of thresh: choose another seed"
        assert th_gpu == float(np.float32(thresh))
        th = th_gpu
    # the mask, with the kink rule
    near = valid & ((p_label - th).abs() <= tau)
    want_kept = valid & (p_label.float() <= np.float32(th))
    kept = got["kept"].to(DEV).bool()
    assert int(near.sum()) <= 1e-3 * int(valid.sum())
    assert torch.equal(kept[~near], want_kept[~near]) and int((kept != want_kept).sum()) <= int(near.sum())
    assert float(got["n_kept"]) == int(kept.sum()) and 0 < int(kept.sum()) < int(valid.sum())
    # loss and gradients on the kernel's mask
    nll = -logp.gather(1, idx[:, None])[:, 0]
    nll_d = -up(ld).gather(1, idx[:, None])[:, 0]
    loss = (nll * kept).sum() / kept.sum() + 0.4 * (nll_d * valid).sum() / valid.sum()
    loss.backward()
    close(got["loss"], loss.detach().reshape(1), LOSS_TOL, "full size loss")
    close(got["grad_main"], lm.grad, GRAD_TOL, "full size grad main")
    close(got["grad_dsn"], ld.grad, GRAD_TOL, "full size grad dsn")
