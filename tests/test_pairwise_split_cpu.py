"""The pair-wise loss on the split core, the parts that need no GPU: the C ABI of include/skd_pairwise_split.h (the pinned names and argument lists; header <-> table <-> library is
tests/test_abi.py, the workspace queries on a host without a device), the routing of ``pair_wise_loss(..., split=True)`` under
a recording double of the four entries, the wiring under a torch-implemented double of the two split entries (on raw HOST
addresses, on top of the plain-C double), NetModel's ``split_pairwise`` switch and the documents."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import cref
from structure_knowledge_distillation_amd import _lib, functional as SF
from structure_knowledge_distillation_amd.utils.criterion import CriterionPairWiseforWholeFeatAfterPool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["skd_pairwise_split_workspace_floats", "skd_pairwise_split_gram_loss", "skd_pairwise_split_backward_workspace_floats",
         "skd_pairwise_split_backward"]
FOUR = ("skd_pairwise_gram_loss", "skd_pairwise_backward", "skd_pairwise_split_gram_loss", "skd_pairwise_split_backward")


def _host(addr, shape):
    n = int(np.prod(shape))
    return np.ctypeslib.as_array(ctypes.cast(ctypes.c_void_p(addr), ctypes.POINTER(ctypes.c_float)), shape=(n,)).reshape(shape)


def _addr(p):
    return p.value if isinstance(p, ctypes.c_void_p) else p


class CoreDouble:
    """The plain-C double (the core ABI only: no split entries) with every call logged as (name, leading integer arguments), and
    the operands of the two fp32 pair-wise products kept as copies."""

    def __init__(self):
        self._core = cref.load(_lib.SIGNATURES)
        self.log, self.operands = [], []

    def __getattr__(self, name):
        fn = getattr(self._core, name)          # AttributeError for an entry the core does not have

        def logged(*args):
            ints = []
            for a in args:
                if not isinstance(a, int) or isinstance(a, bool) or abs(a) > 1 << 20:
                    break
                ints.append(a)
            self.log.append((name,) + tuple(ints))
            if name in FOUR:
                self._keep(name, args)
            return fn(*args)
        return logged

    def _keep(self, name, args):
        if name.endswith("gram_loss"):
            b, cs, ct, m, ldm, fs, ft = args[:7]
            self.operands.append((name, _host(_addr(fs), (b, cs, ldm)).copy(), _host(_addr(ft), (b, ct, ldm)).copy()))
        else:
            b, cs, m, ldm, fs, g, nrm, gl = args[:8]
            self.operands.append((name, _host(_addr(fs), (b, cs, ldm)).copy(), _host(_addr(g), (b, ldm, ldm)).copy(),
                                  _host(_addr(nrm), (b, m)).copy(), _host(_addr(gl), (1,)).copy()))


class SplitDouble(CoreDouble):
    """... + the four entries of skd_pairwise_split.h.  ``compute`` False: the two products are the core's own fp32 entries on a
    workspace of their own (a recording double: the outputs are today's bits); True: computed with torch in float64 from the raw
    host buffers (a second implementation: the comparison with the unsplit path sees the wiring)."""

    def __init__(self, compute=False):
        super().__init__()
        self.compute = compute

    def skd_pairwise_split_workspace_floats(self, b, cs, ct, m):
        self.log.append(("skd_pairwise_split_workspace_floats", b, cs, ct, m))
        return 3

    def skd_pairwise_split_backward_workspace_floats(self, b, cs, m):
        self.log.append(("skd_pairwise_split_backward_workspace_floats", b, cs, m))
        return 5

    def skd_pairwise_split_gram_loss(self, b, cs, ct, m, ldm, fs, ft, g, loss, ws, stream):
        args = (b, cs, ct, m, ldm, fs, ft, g, loss, ws, stream)
        self.log.append(("skd_pairwise_split_gram_loss", b, cs, ct, m, ldm))
        self._keep("skd_pairwise_split_gram_loss", args)
        assert fs and ft and loss and ws and ldm == self._core.skd_pairwise_ldm(m)
        if not self.compute:
            own = torch.empty(max(1, self._core.skd_pairwise_workspace_floats(b, m)))
            return self._core.skd_pairwise_gram_loss(b, cs, ct, m, ldm, fs, ft, g, loss, own.data_ptr(), None)
        s, t = torch.from_numpy(_host(fs, (b, cs, ldm))).double(), torch.from_numpy(_host(ft, (b, ct, ldm))).double()
        gram = torch.einsum("icm,icn->imn", t, t) - torch.einsum("icm,icn->imn", s, s)
        if g:
            _host(g, (b, ldm, ldm))[...] = gram.float().numpy()
        _host(loss, (1,))[0] = float((gram ** 2).sum() / m ** 2 / b)
        return 1

    def skd_pairwise_split_backward(self, b, cs, m, ldm, fs, g, nrm, gl, dp, ws, stream):
        args = (b, cs, m, ldm, fs, g, nrm, gl, dp, ws, stream)
        self.log.append(("skd_pairwise_split_backward", b, cs, m, ldm))
        self._keep("skd_pairwise_split_backward", args)
        assert fs and g and nrm and gl and dp and ws
        if not self.compute:
            own = torch.empty(max(1, self._core.skd_pairwise_backward_workspace_floats(b, cs, m)))
            return self._core.skd_pairwise_backward(b, cs, m, ldm, fs, g, nrm, gl, dp, own.data_ptr(), None)
        s, gram = torch.from_numpy(_host(fs, (b, cs, ldm))).double(), torch.from_numpy(_host(g, (b, ldm, ldm))).double()
        n, up = torch.from_numpy(_host(nrm, (b, m))).double(), float(_host(gl, (1,))[0])
        out = torch.zeros(b, cs, ldm, dtype=torch.float64)
        out[:, :, :m] = (-4.0 / (m * m * b)) * up * torch.einsum("bcn,bmn->bcm", s, gram)[:, :, :m] / n[:, None, :]
        _host(dp, (b, cs, ldm))[...] = out.float().numpy()
        return 1


@pytest.fixture
def backend():
    def install(double):
        _lib.install_test_backend(double)
        return double
    yield install
    _lib.install_test_backend(None)


def features(cs=8, ct=12, hw=18, nhwc=False, seed=5):
    g = torch.Generator().manual_seed(seed)
    fs, ft = torch.randn(2, cs, hw, hw, generator=g), torch.randn(2, ct, hw, hw, generator=g)
    if nhwc:
        fs, ft = fs.contiguous(memory_format=torch.channels_last), ft.contiguous(memory_format=torch.channels_last)
    return fs, ft


def step(fs, ft, k, split, between=None):
    x = fs.clone(memory_format=torch.preserve_format).requires_grad_(True)
    loss = SF.pair_wise_loss(x, ft, k, k, split=split)
    if between is not None:
        between()
    (loss * 0.75).backward()
    return loss.detach(), x.grad


def pairwise_calls(double):
    return [c[0] for c in double.log if c[0] in FOUR]


# ---- 1. the C ABI ------------------------------------------------------------------------------------------------------------------

def test_header_table_and_library_agree():
    """What is particular to skd_pairwise_split.h; header <-> table <-> library <-> build digest: tests/test_abi.py, for every header."""
    assert sorted(_lib.ABI["skd_pairwise_split.h"]) == sorted(NAMES) and len(NAMES) == 4
    # the argument lists are the fp32 twins': a caller can hand both the same buffers
    for twin, name in (("skd_pairwise_gram_loss", "skd_pairwise_split_gram_loss"), ("skd_pairwise_backward", "skd_pairwise_split_backward"),
                       ("skd_pairwise_backward_workspace_floats", "skd_pairwise_split_backward_workspace_floats")):
        assert _lib.SIGNATURES[twin] == _lib.signature(name)


def test_workspace_queries_need_no_device_and_grow():
    lib = _lib.load()
    gram, bwd = lib.skd_pairwise_split_workspace_floats, lib.skd_pairwise_split_backward_workspace_floats
    for args in ((0, 8, 8, 65), (1, 0, 8, 65), (1, 8, 0, 65), (1, 8, 8, 0), (-1, 8, 8, 65)):
        assert gram(*args) == 1
    for args in ((0, 8, 65), (1, 0, 65), (1, 8, 0)):
        assert bwd(*args) == 1
    sizes = (65, 128, 129, 289, 1089, 4225)
    for cs, ct in ((1, 1), (12, 20), (130, 70), (128, 512)):
        kp = -(-cs // 16) * 16 + -(-ct // 16) * 16
        for b in (1, 2, 3, 8):
            for m in sizes:
                ldm, nt = lib.skd_pairwise_ldm(m), lib.skd_pairwise_ldm(m) // 128
                # the node-major copy of both panels + one partial per 64-row half of every upper-triangle tile
                assert gram(b, cs, ct, m) == b * ldm * kp + nt * (nt + 1) * b, (b, cs, ct, m)
                assert bwd(b, cs, m) >= 1
        for m in sizes:       # monotone in B ...
            assert [gram(b, cs, ct, m) for b in (1, 2, 3, 8)] == sorted(gram(b, cs, ct, m) for b in (1, 2, 3, 8))
        for b in (1, 2, 8):   # ... and in M
            assert [gram(b, cs, ct, m) for m in sizes] == sorted(gram(b, cs, ct, m) for m in sizes)
    # the backward's workspace: S slices of raw 64 x 128 tiles per output tile, S > 1 only while the tiles do not fill the chip
    for b, cs, m in ((8, 128, 289), (8, 128, 1089), (1, 128, 1089), (2, 130, 289)):
        n = bwd(b, cs, m)
        ldm = lib.skd_pairwise_ldm(m)
        tiles = b * (ldm // 128) * -(-cs // 64)
        assert n % (tiles * 64 * 128) == 0 and 2 <= n // (tiles * 64 * 128) <= ldm // 16 // 8, (b, cs, m, n)
    assert bwd(8, 128, 4225) == 1 and bwd(2, 12, 65) == 1
    # the launch entries refuse on the host, before any device call
    z = ctypes.c_void_p(0)
    assert lib.skd_pairwise_split_gram_loss(2, 8, 8, 65, 128, z, z, z, z, z, None) == 0
    assert lib.skd_pairwise_split_backward(2, 8, 65, 128, z, z, z, z, z, z, None) == 0


# ---- 2. routing under the recording double -------------------------------------------------------------------------------------------

def test_split_false_small_excluded_or_no_entries_make_todays_calls(backend, monkeypatch):
    fs, ft = features()
    plain = backend(CoreDouble())
    today = {k: step(fs, ft, k, False) for k in (2, 3)}        # 18 x 18 features: kernel 2 -> 81 nodes, kernel 3 -> 36
    logs = {}
    for k in (2, 3):
        plain.log.clear()
        step(fs, ft, k, False)
        logs[k] = list(plain.log)
    assert pairwise_calls(plain) == [] and any(c[0] == "skd_pairwise_small" for c in logs[3])
    assert [c[0] for c in logs[2] if c[0] in FOUR] == list(FOUR[:2])

    def same(double, k, split):
        double.log.clear()
        loss, grad = step(fs, ft, k, split)
        assert double.log == logs[k], (k, split)
        assert torch.equal(loss, today[k][0]) and torch.equal(grad, today[k][1])
    # a back-end without the entries, whatever the flag says
    assert not SF.pairwise_split_supported()
    same(plain, 2, True)
    same(plain, 3, True)
    # a back-end with them: split=False, and m <= 64 whatever the flag says
    rec = backend(SplitDouble())
    assert SF.pairwise_split_supported()
    same(rec, 2, False)
    same(rec, 3, False)
    same(rec, 3, True)
    # an excluded shape
    monkeypatch.setattr(SF, "PAIRWISE_SPLIT_ROUTING_EXCLUDED", frozenset({(8, 12, 81)}))
    same(rec, 2, True)


def test_split_entries_get_todays_buffers(backend, monkeypatch):
    monkeypatch.setattr(SF, "PAIRWISE_SPLIT_ROUTING_EXCLUDED", frozenset())
    for nhwc in (False, True):
        fs, ft = features(nhwc=nhwc)
        rec = backend(SplitDouble())
        l0, g0 = step(fs, ft, 2, False)
        log0, ops0 = list(rec.log), list(rec.operands)
        rec.log.clear()
        rec.operands.clear()
        l1, g1 = step(fs, ft, 2, True)
        assert pairwise_calls(rec) == list(FOUR[2:])
        # the same calls in the same order, but for the two products and their workspace queries
        swap = {"skd_pairwise_gram_loss": "skd_pairwise_split_gram_loss", "skd_pairwise_backward": "skd_pairwise_split_backward"}
        want = []
        for c in log0:
            if c[0] == "skd_pairwise_workspace_floats":
                want.append(("skd_pairwise_split_workspace_floats", 2, 8, 12, 81))
            elif c[0] == "skd_pairwise_backward_workspace_floats":
                want.append(("skd_pairwise_split_backward_workspace_floats",) + c[1:])
            else:
                want.append((swap.get(c[0], c[0]),) + c[1:])
        assert rec.log == want
        # the operands the split entries were handed are today's, bit for bit
        assert len(ops0) == len(rec.operands) == 2
        for a, b in zip(ops0, rec.operands):
            assert swap[a[0]] == b[0] and len(a) == len(b)
            for x, y in zip(a[1:], b[1:]):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        # the recording double computes with the core's own kernels: today's bits, in today's layout
        assert torch.equal(l0, l1) and torch.equal(g0, g1) and g0.stride() == g1.stride()


def test_backward_follows_the_forwards_decision(backend, monkeypatch):
    fs, ft = features()
    rec = backend(SplitDouble())
    monkeypatch.setattr(SF, "PAIRWISE_SPLIT_ROUTING_EXCLUDED", frozenset())
    # split in the forward; the set gains the shape before the backward
    exclude = lambda: monkeypatch.setattr(SF, "PAIRWISE_SPLIT_ROUTING_EXCLUDED", frozenset({(8, 12, 81)}))
    step(fs, ft, 2, True, between=exclude)
    assert pairwise_calls(rec) == list(FOUR[2:])
    # fp32 in the forward (excluded); the set is emptied before the backward
    rec.log.clear()
    step(fs, ft, 2, True, between=lambda: monkeypatch.setattr(SF, "PAIRWISE_SPLIT_ROUTING_EXCLUDED", frozenset()))
    assert pairwise_calls(rec) == list(FOUR[:2])
    # fp32 in the forward (flag off); nothing the caller does afterwards turns the backward
    rec.log.clear()
    step(fs, ft, 2, False, between=lambda: None)
    assert pairwise_calls(rec) == list(FOUR[:2])
    # no gradient wanted: the loss alone, G = NULL
    rec.log.clear()
    rec.operands.clear()
    with torch.no_grad():
        SF.pair_wise_loss(fs, ft, 2, 2, split=True)
    assert pairwise_calls(rec) == ["skd_pairwise_split_gram_loss"]


# ---- 3. wiring under the torch-implemented double -------------------------------------------------------------------------------------

@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "channels_last"])
@pytest.mark.parametrize("k,cs,ct", [(2, 8, 12), (1, 4, 20)])
def test_split_path_equals_the_unsplit_path(backend, monkeypatch, nhwc, k, cs, ct):
    monkeypatch.setattr(SF, "PAIRWISE_SPLIT_ROUTING_EXCLUDED", frozenset())
    fs, ft = features(cs, ct, 18 if k == 2 else 9, nhwc)
    backend(CoreDouble())
    l0, g0 = step(fs, ft, k, False)
    rec = backend(SplitDouble(compute=True))
    l1, g1 = step(fs, ft, k, True)
    assert pairwise_calls(rec) == list(FOUR[2:])
    assert g1.shape == g0.shape and g1.stride() == g0.stride()
    assert abs(float(l1) - float(l0)) <= 1e-6 * abs(float(l0))
    assert float((g1 - g0).abs().max()) <= 1e-6 * float(g0.abs().max()) and float(g0.abs().max()) > 0


# ---- 4. the switch -----------------------------------------------------------------------------------------------------------------

def _criterion(model):
    found = [m for m in model.criterion_pair_wise_for_interfeat.modules() if isinstance(m, CriterionPairWiseforWholeFeatAfterPool)]
    assert len(found) == 1
    return found[0]


def test_netmodel_split_pairwise_switch(backend, monkeypatch):
    from structure_knowledge_distillation_amd.networks import kd_model
    from structure_knowledge_distillation_amd.networks.kd_model import NetModel, default_args
    assert kd_model.SWITCHES[8] == ("split_pairwise", "SKD_SPLIT_PAIRWISE", ()) and len(kd_model.SWITCHES) == 9
    monkeypatch.delenv("SKD_SPLIT_PAIRWISE", raising=False)
    assert default_args().split_pairwise is False
    assert default_args(split_pairwise=True).split_pairwise is True
    monkeypatch.setenv("SKD_SPLIT_PAIRWISE", "1")
    assert default_args().split_pairwise is True and default_args(split_pairwise=False).split_pairwise is False
    monkeypatch.setenv("SKD_SPLIT_PAIRWISE", "0")
    assert default_args().split_pairwise is False
    # the reference's positional signature stands; the keyword is extra
    assert CriterionPairWiseforWholeFeatAfterPool(0.5, -5).split is False
    assert CriterionPairWiseforWholeFeatAfterPool(0.5, -5, split=True).split is True
    kw = dict(device=torch.device("cpu"), batch_size=2, ho=False)
    backend(SplitDouble())
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        model = NetModel(default_args(**kw))
        assert model.split_pairwise is False and _criterion(model).split is False
        model = NetModel(default_args(split_pairwise=True, **kw))
        assert model.split_pairwise is True and _criterion(model).split is True
        monkeypatch.setenv("SKD_SPLIT_PAIRWISE", "1")
        assert _criterion(NetModel(default_args(**kw))).split is True
        monkeypatch.setenv("SKD_SPLIT_PAIRWISE", "0")
    assert not [w for w in seen if "skd_pairwise_split.h" in str(w.message)]
    # a back-end without the entries: one warning, the fp32 kernels
    backend(CoreDouble())
    with pytest.warns(RuntimeWarning, match="skd_pairwise_split.h") as seen:
        model = NetModel(default_args(split_pairwise=True, **kw))
    assert len([w for w in seen if "skd_pairwise_split.h" in str(w.message)]) == 1
    assert model.split_pairwise is False and _criterion(model).split is False
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        assert _criterion(NetModel(default_args(**kw))).split is False      # switch off: nothing to warn about
    assert not [w for w in seen if "skd_pairwise_split.h" in str(w.message)]


def test_criterion_hands_the_flag_to_the_op(backend, monkeypatch):
    monkeypatch.setattr(SF, "PAIRWISE_SPLIT_ROUTING_EXCLUDED", frozenset())
    rec = backend(SplitDouble())
    fs, ft = features()
    for split, want in ((False, FOUR[:2]), (True, FOUR[2:])):
        rec.log.clear()
        x = fs.clone().requires_grad_(True)
        CriterionPairWiseforWholeFeatAfterPool(0.12, -5, split=split)([x] * 5, [ft] * 5).backward()      # int(18 * 0.12) = 2
        assert pairwise_calls(rec) == list(want)


# ---- 5. the documents ----------------------------------------------------------------------------------------------------------------

def test_documents_name_the_switch_the_header_and_the_section():
    read = lambda name: open(os.path.join(ROOT, name)).read()
    design, readme, integration = read("DESIGN.md"), read("README.md"), read("INTEGRATION.md")
    assert "7.13" in design and "skd_pairwise_split.h" in design and "SKD_SPLIT_PAIRWISE" in design
    assert "PAIRWISE_SPLIT_ROUTING_EXCLUDED" in design and "pairwise_split.hip" in design
    assert "SKD_SPLIT_PAIRWISE" in readme and "7.13" in readme
    assert "SKD_SPLIT_PAIRWISE" in integration and "split_pairwise" in integration
    assert "skd_pairwise_split.h" in SF.pair_wise_loss.__doc__ and "skd_pairwise_split.h" in SF.pairwise_split_supported.__doc__
    with open(os.path.join(ROOT, "structure_knowledge_distillation_amd", "csrc", "pairwise.hip")) as fh:
        head = fh.read(4000)
    assert "pairwise_split.hip" in head and "bf16 would break" not in head
    # the shipped exclusion set holds shapes of the measured sweep only
    assert SF.PAIRWISE_SPLIT_ROUTING_EXCLUDED <= {(128, 512, 289), (128, 512, 1089), (128, 512, 4225)}
