"""-m gpu: every row of tests/regime_cases.py against libskd_hip.so -- each kernel instantiation and in-kernel regime the
table names is launched through its public entry with the library's own geometry choice, every buffer between 0xFF guard
bands, workspaces at exactly the queried size and dirty, workspace entries twice on the same buffers; every output must meet
the tolerance of its entry's value test against the row's float64 expectation, and no device status word may be raised."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import bounds_cases as BC  # noqa: E402
import ohem_ref as R  # noqa: E402
import regime_cases as RC  # noqa: E402
import test_ohem_cpu as OC  # noqa: E402  (gold(): tau; gen(): the fixture generator's inputs)
import test_ohem_gpu as OG  # noqa: E402  (run_abi, close and the bounds of the OHEM value test)

from structure_knowledge_distillation_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
KERNEL_ROWS = [n for n, r in RC.REGIMES.items() if r.case is not None]
OHEM_ROWS = [n for n, r in RC.REGIMES.items() if r.ohem is not None]


@pytest.fixture(scope="module")
def hip():
    return _lib.load()


@pytest.mark.parametrize("name", KERNEL_ROWS)
def test_kernel_in_its_regime(hip, name):
    r = RC.REGIMES[name]
    assert r.predicate() is True
    got, tols, want = BC.run_case(r.case, hip, BC.Arena("cuda"))
    torch.cuda.synchronize()
    for k, g in enumerate(got):
        what = "%s, call %d%s" % (name, k + 1, " (on the workspace the first call left)" if k else "")
        if r.nan:
            assert all(bool(torch.isnan(g[o]).all()) for o in tols), what + ": not every output is NaN"
        else:
            BC.compare(g, want, tols, what)
        if r.post is not None:
            r.post(g, *r.case.args)
    if r.case.ws and r.case.bit:
        for out in tols:
            assert BC.same_bits(got[0][out], got[1][out]), "%s: %s is not bit-reproducible on a used workspace" % (name, out)
    assert _lib.device_status() == [0] * hip.skd_status_words()


def check_ohem(name, got, own, target, tau):
    """check_case() of tests/test_ohem_gpu.py without the parts that need the reference's recording: keys and a k-th threshold
    within tau of the float64 restatement's, a thresh / 1.0 threshold the same bits, the mask equal wherever the label probability
    is farther than tau from the threshold, loss and gradients against the restatement on the mask the kernel chose."""
    keys = got["pred_ds"].numpy()
    assert not np.isnan(keys).any(), "a key was left unwritten"
    assert np.array_equal(keys == -1, own.pred_ds == -1)
    kerr = float(np.abs(keys.astype(np.float64) - own.pred_ds.astype(np.float64)).max())
    th_gpu, th_own = float(got["threshold"]), float(own.threshold)
    print("%s: keys max err %.3e (tau %.3e), threshold gpu %.9g restatement %.9g" % (name, kerr, tau, th_gpu, th_own))
    assert kerr <= tau and got["num_valid"] == own.num_valid
    assert abs(th_gpu - th_own) <= tau
    valid = target.numpy() != 255
    near = valid & (np.abs(own.p_label - th_own) <= tau)
    kept = got["kept"].numpy()
    assert set(np.unique(kept)) <= {0, 1}, "a mask byte was left unwritten"
    kept = kept.astype(bool)
    assert not kept[~valid].any() and np.array_equal(kept[~near], own.own_kept[~near])
    assert int(near.sum()) <= 1e-3 * int(valid.sum()) and float(got["n_kept"]) == kept.sum() and 0 < kept.sum()
    return kept


@pytest.mark.parametrize("name", OHEM_ROWS)
def test_ohem_in_its_regime(hip, name):
    r = RC.REGIMES[name]
    assert r.predicate() is True
    o = r.ohem
    tau = OC.gold()["tau"]
    lm, ld, tg = OC.gen().make_inputs(o["shape"], o["size"], o["seed"])
    if not o["two"]:
        ld = None
    own = R.ohem(lm.numpy(), None if ld is None else ld.numpy(), tg.numpy(), 255, o["thresh"], o["min_kept"], o["factor"], 0.4)
    assert 0 < o["min_kept"] // o["factor"] ** 2 < own.num_valid                      # the k-th key is looked for
    A1 = BC.Arena("cuda")
    first = OG.run_abi(A1, lm, ld, tg, o["thresh"], o["min_kept"], o["factor"])
    again = OG.run_abi(BC.Arena("cuda"), lm, ld, tg, o["thresh"], o["min_kept"], o["factor"], ws=first["ws"])     # the used workspace
    A1.check()                                                                         # (the workspace's guards live in the first arena)
    for k, got in enumerate((first, again)):
        kept = check_ohem("%s, call %d" % (name, k + 1), got, own, tg, tau)
        on = own if np.array_equal(kept, own.own_kept) else R.ohem(lm.numpy(), None if ld is None else ld.numpy(), tg.numpy(), 255, o["thresh"],
                                                                    o["min_kept"], o["factor"], 0.4, kept=kept)
        OG.close(got["loss"], [on.loss], OG.LOSS_TOL, name + " loss")
        OG.close(got["grad_main"], on.grad_main, OG.GRAD_TOL, name + " grad main")
        if ld is not None:
            OG.close(got["grad_dsn"], on.grad_dsn, OG.GRAD_TOL, name + " grad dsn")
    for k in ("threshold", "loss", "n_kept", "pred_ds", "kept", "grad_main", "grad_dsn"):
        assert (first[k] is None and again[k] is None) or torch.equal(first[k], again[k]), "%s: %s is not bit-reproducible on a used workspace" % (name, k)
    torch.cuda.synchronize()
    assert _lib.device_status() == [0] * hip.skd_status_words()
