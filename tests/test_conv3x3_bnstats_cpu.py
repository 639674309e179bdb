"""Batch-norm statistics from the epilogue of the split-core 3x3 convolution (include/skd_bnstats.h), the parts that need no GPU:
the numpy restatement of the record and of the fixed-order combine (tests/bnstats_ref.py) against float64 at the project's
statistics bounds, the C ABI (the pinned names and argument lists, host-side refusals), the wiring of a student flagged with
``bnstats=True`` (a double of the four entries on raw HOST addresses, computed by the restatement, on top of the training form's
torch-implemented double), the plain-C double (no entry: nothing changes, bit for bit) and NetModel's ``split_bnstats`` switch."""
import copy

import numpy as np
import pytest
import torch

import bnstats_ref as R
import structure_knowledge_distillation_amd.networks.pspnet_combine as PC
from oracle import cref
from structure_knowledge_distillation_amd import _lib, functional as SF
from structure_knowledge_distillation_amd import networks
from test_conv3x3_train_cpu import TrainDouble, _input, _step, _student
from test_student_infer_cpu import _host

NAMES = ["skd_conv3x3_bnstats_floats", "skd_conv3x3_split_stats_nhwc", "skd_conv3x3_narrow_stats_nhwc",
         "skd_abn_stats_from_partials_nhwc"]
# (Cin, Cout, dilation) of the BasicBlock convolutions the training form routes, in the order of the forward
BLOCK_ROUTED = [(128, 128, 1)] * 3 + [(128, 256, 2)] + [(256, 256, 2)] * 3 + [(256, 512, 4)] + [(512, 512, 4)] * 3


# ---- 1. the restatement against float64 ------------------------------------------------------------------------------------------

def _data(m, c, seed, offset=0.0):
    g = np.random.default_rng(seed)
    sigma = 3.0
    y = (g.standard_normal((m, c)) * sigma + g.standard_normal((1, c)) * 5.0 + offset * sigma).astype(np.float32)
    return y, g.standard_normal(c).astype(np.float32), (g.random(c) + 0.5).astype(np.float32)


@pytest.mark.parametrize("m,c", [(286, 128), (33, 64), (9, 64), (32, 16), (2079, 16)])
@pytest.mark.parametrize("offset", [0.0, 1e3], ids=["random", "offset-1e3-sigma"])
def test_restatement_within_the_statistics_bounds(m, c, offset):
    y, rm, rv = _data(m, c, seed=m + c, offset=offset)
    rec = R.block_records(y)
    assert rec.shape == (-(-m // 32), c, 2) and rec.size == R.workspace_floats(m, c)
    got = R.combine(rec, m, rm, rv, 0.1)
    want = R.float64_stats(y, rm, rv, 0.1)
    keys = ("mean", "var", "running_mean", "running_var") if offset == 0.0 else ("mean", "var")
    for k, a, b in zip(("mean", "var", "running_mean", "running_var"), got, want):
        err = R.rel_err(a, b)
        print("M %d C %d offset %g %s: %.3e (bound %.1e)" % (m, c, offset, k, err, R.BOUNDS[k]))
        if k in keys:
            assert err <= R.BOUNDS[k], (k, err)
    again = R.combine(R.block_records(y), m, rm, rv, 0.1)
    assert all(np.array_equal(a, b) for a, b in zip(got, again))


def test_restatement_is_exact_on_a_constant_channel_and_on_a_single_row():
    y, _, _ = _data(286, 8, seed=1)
    y[:, 3] = 7.25
    mean, var = R.combine(R.block_records(y), 286)
    assert mean[3] == np.float32(7.25) and var[3] == 0.0
    rec = R.block_records(y[:33])
    assert np.array_equal(rec[1, :, 0], y[32]) and not rec[1, :, 1].any(), "a block of one row: its value, M2 = 0"
    one = R.combine(R.block_records(y[:1]), 1, np.zeros(8, np.float32), np.ones(8, np.float32))
    assert np.array_equal(one[0], y[0]) and not one[1].any() and np.array_equal(one[3], np.full(8, 0.9, np.float32))


# ---- 2. the C ABI ------------------------------------------------------------------------------------------------------------

def test_bnstats_header_table_and_library_agree():
    """What is particular to skd_bnstats.h; header <-> table <-> library <-> build digest: tests/test_abi.py, for every header."""
    assert sorted(_lib.ABI["skd_bnstats.h"]) == sorted(NAMES) and len(NAMES) == 4
    # the two convolution entries take the same list: the training forward's arguments, then the workspace
    assert _lib.signature("skd_conv3x3_split_stats_nhwc") == _lib.signature("skd_conv3x3_narrow_stats_nhwc")


def test_workspace_size_and_host_side_refusals():
    """Every refusal is decided on the host, in front of the launch: no device is touched (the pointers are never followed)."""
    lib = _lib.load()
    for m, c in ((286, 128), (33, 64), (9, 256), (1, 64), (32, 64), (33800, 512), (2 ** 31 + 5, 128)):
        assert lib.skd_conv3x3_bnstats_floats(m, c) == R.workspace_floats(m, c), (m, c)
    for m, c in ((0, 128), (-1, 128), (10, 0), (10, 32), (10, 96), (10, -64)):
        assert lib.skd_conv3x3_bnstats_floats(m, c) == 0, (m, c)
    X, OUT, PK, ST = 0x10000, 0x4000000, 0x8000000, 0xA000000
    n = R.workspace_floats(2 * 13 * 11, 128)
    ok = dict(B=2, H=13, W=11, cin=128, cout=128, d=1, x=X, pk=PK, out=OUT, geo=0, st=ST, n=n)
    bads = [dict(st=None), dict(st=ST + 4), dict(n=n - 1), dict(n=0), dict(n=-1), dict(x=None), dict(pk=None), dict(out=None),
            dict(x=X + 4), dict(x=X + 8), dict(pk=PK + 4), dict(B=0), dict(H=0), dict(W=-1), dict(cin=24), dict(cin=0), dict(cout=0),
            dict(d=0), dict(d=-1), dict(geo=-1)]
    for entry, more in ((lib.skd_conv3x3_split_stats_nhwc, [dict(cout=64), dict(cout=192), dict(geo=4)]),
                        (lib.skd_conv3x3_narrow_stats_nhwc, [dict(cout=32), dict(cout=96), dict(geo=2), dict(geo=3)])):
        for bad in bads + more:
            v = dict(ok, **bad)
            assert entry(v["B"], v["H"], v["W"], v["cin"], v["cout"], v["d"], v["x"], v["pk"], v["out"], None, v["geo"], v["st"],
                         v["n"], None) == 0, bad
    ok = dict(rows=286, C=128, st=ST, n=n, mean=OUT, var=OUT + 4096)
    for bad in (dict(rows=0), dict(rows=-1), dict(C=8), dict(C=24), dict(C=0), dict(C=-16), dict(st=None), dict(st=ST + 4),
                dict(n=n - 1), dict(n=0), dict(mean=None), dict(var=None), dict(rows=289), dict(C=256)):
        v = dict(ok, **bad)
        assert lib.skd_abn_stats_from_partials_nhwc(v["rows"], v["C"], v["st"], v["n"], v["mean"], v["var"], None, None, 0.1,
                                                    None) == 0, bad


# ---- 3. wiring -----------------------------------------------------------------------------------------------------------------

class StatsDouble(TrainDouble):
    """TrainDouble + the entries of skd_bnstats.h on raw HOST addresses: the convolution entry is the plain one followed by the
    restatement's records of its output, the finalize is the restatement's combine.  Every call is recorded."""

    def __init__(self, core):
        super().__init__(core, compute=True)
        self.stats, self.finals = [], []

    def skd_conv3x3_bnstats_floats(self, m, cout):
        return R.workspace_floats(m, cout) if m > 0 and cout > 0 and cout % 64 == 0 else 0

    def skd_conv3x3_split_stats_nhwc(self, B, H, W, cin, cout, dil, x, pack, out, cbias, geometry, stats, stats_floats, stream):
        m = B * H * W
        assert stats and stats_floats == R.workspace_floats(m, cout) and geometry == 0
        if not self.skd_conv3x3_split_nhwc(B, H, W, cin, cout, dil, x, pack, out, cbias, None, None, None, None, 0.0, 0, 0.01, 0, stream):
            return 0
        _host(stats, (stats_floats,))[...] = R.block_records(_host(out, (m, cout))).reshape(-1)
        self.stats.append(dict(cin=cin, cout=cout, dilation=dil, out=out, stats=stats))
        return 1

    def skd_conv3x3_narrow_stats_nhwc(self, *args):
        raise AssertionError("no 64-channel convolution is routed without ``narrow``")

    def skd_abn_stats_from_partials_nhwc(self, rows, c, stats, stats_floats, mean, var, running_mean, running_var, momentum, stream):
        assert stats_floats == R.workspace_floats(rows, c) and mean and var
        rec = _host(stats, (stats_floats,)).reshape(-1, c, 2)
        if running_mean:
            rm, rv = _host(running_mean, (c,)), _host(running_var, (c,))
            m, v, rm[...], rv[...] = R.combine(rec, rows, rm.copy(), rv.copy(), momentum)
        else:
            m, v = R.combine(rec, rows)
        _host(mean, (c,))[...], _host(var, (c,))[...] = m, v
        self.finals.append(dict(rows=rows, c=c, stats=stats, running=bool(running_mean)))
        return 1


@pytest.fixture
def double():
    d = StatsDouble(cref.load(_lib.SIGNATURES))
    _lib.install_test_backend(d)
    yield d
    _lib.install_test_backend(None)


def _marks(net):
    return [getattr(m, "_skd_train_bnstats", False) for m in net.modules() if isinstance(m, PC.BasicBlock)]


def _running(net):
    return {k: v.clone() for k, v in net.named_buffers() if "running" in k}


def test_flagged_student_takes_its_statistics_from_the_epilogue(double, monkeypatch):
    # the policy lists shapes of the step alone: the wide ones above, layer1's two with ``narrow``
    assert isinstance(PC.BNSTATS_ROUTING_EXCLUDED, frozenset)
    assert all(e in BLOCK_ROUTED + [(128, 64, 1), (64, 64, 1)] for e in PC.BNSTATS_ROUTING_EXCLUDED)
    monkeypatch.setattr(PC, "BNSTATS_ROUTING_EXCLUDED", frozenset())            # the mechanism; the policy is below
    assert SF.conv3x3_bnstats_supported()
    net, x = _student(), _input()
    routed = networks.route_training_convs(copy.deepcopy(net))
    flagged = networks.route_training_convs(copy.deepcopy(net), bnstats=True)
    assert _marks(routed) == [False] * 8 and _marks(flagged) == [True] * 8
    assert not any(hasattr(m, "_skd_train_bnstats") for m in flagged.modules() if not isinstance(m, PC.BasicBlock))
    want_out, want = _step(routed, x)
    assert double.stats == [] and double.finals == []
    n_plain = len(double.calls)
    got_out, got = _step(flagged, x)
    assert [(c["cin"], c["cout"], c["dilation"]) for c in double.stats] == BLOCK_ROUTED
    # every record buffer went to exactly one finalize, in order, with the running pointers; dsn[0] and the PSP half: plain calls
    assert [f["stats"] for f in double.finals] == [c["stats"] for c in double.stats] and all(f["running"] for f in double.finals)
    assert len(double.calls) == 2 * n_plain, "the same launches: 13 forward (11 of them inside the statistics entry), 13 data gradients"
    assert len(got_out) == len(want_out)
    rel = lambda a, b: float((a.detach() - b.detach()).abs().max() / b.detach().abs().max())
    for a, b in zip(got_out, want_out):
        assert rel(a, b) <= 1e-5, rel(a, b)
    assert set(got) == set(want) and all(g is not None for g in got.values())
    # The statistics move by about 1e-7 of themselves (another summation order), and the network carries that on: the 1 x 1 stage
    # of the pyramid normalises over two samples, and the bias of dsn[0] sits in front of a batch norm, so its gradient is a
    # cancellation residue.  Hence: all gradients together within 1e-4 of their norm, each within 1e-3 of its largest element --
    # or, for a residue, of 1e-3 of the largest gradient element anywhere.  A wiring mistake (the wrong records, a stale mean)
    # moves the gradients by their own size.
    top = max(float(v.abs().max()) for v in want.values())
    total = sum(float((got[k] - want[k]).norm()) ** 2 for k in want) ** 0.5 / sum(float(want[k].norm()) ** 2 for k in want) ** 0.5
    print("all gradients: %.3e of their norm" % total)
    assert total <= 1e-4, total
    for k in want:
        err = float((got[k] - want[k]).abs().max()) / max(float(want[k].abs().max()), 1e-3 * top)
        assert err <= 1e-3, (k, err)
    ra, rb = _running(flagged), _running(routed)
    for k in rb:
        assert rel(ra[k], rb[k]) <= 1e-5, k
    # eval mode, no_grad: nothing is asked for statistics
    double.stats.clear()
    flagged.eval()
    flagged(x)
    flagged.train()
    with torch.no_grad():
        flagged(x)
    assert double.stats == []
    # the policy: an excluded shape keeps the pair it had
    monkeypatch.setattr(PC, "BNSTATS_ROUTING_EXCLUDED", frozenset({(128, 128, 1), (512, 512, 4)}))
    flagged(x)
    assert [(c["cin"], c["cout"], c["dilation"]) for c in double.stats] == [s for s in BLOCK_ROUTED
                                                                             if s not in PC.BNSTATS_ROUTING_EXCLUDED]
    # the flag cleared
    double.stats.clear()
    networks.route_training_convs(flagged)
    flagged(x)
    assert double.stats == [] and _marks(flagged) == [False] * 8
    networks.route_training_convs(flagged, enable=False, bnstats=True)
    assert _marks(flagged) == [False] * 8


def test_replicated_normalisation_is_not_asked(double, monkeypatch):
    """A synchronised (replicated) call ignores the opt-in: the convolution is then not asked for statistics."""
    import structure_knowledge_distillation_amd.libs.modules as M
    net, x = _student(), _input()
    flagged = networks.route_training_convs(copy.deepcopy(net), bnstats=True)
    assert flagged.layer2[1].bn1.takes_partials()
    monkeypatch.setattr(M, "abn_relu_replicated", lambda group, sync: True)
    assert not flagged.layer2[1].bn1.takes_partials()
    conv, bn = flagged.layer2[1].conv1, flagged.layer2[1].bn1
    h = torch.randn(2, 128, 7, 8).contiguous(memory_format=torch.channels_last)
    y, partials = PC._train_conv(flagged.layer2[1], conv, h, bn)
    assert partials is None and double.stats == [] and len(double.calls) == 1


def test_op_returns_the_pair_and_the_plain_backward(double):
    torch.manual_seed(3)
    conv = torch.nn.Conv2d(128, 128, 3, 1, 2, 2, bias=True)
    x = torch.randn(2, 128, 5, 6).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    plain = SF.conv3x3_split_train(x, conv.weight, 2, conv.bias, owner=conv)
    y, partials = SF.conv3x3_split_train(x, conv.weight, 2, conv.bias, owner=conv, stats=True)
    assert torch.equal(y, plain) and y.requires_grad and not partials.requires_grad
    assert partials.dtype == torch.float32 and partials.numel() == R.workspace_floats(60, 128)
    assert np.array_equal(partials.numpy().reshape(-1, 128, 2), R.block_records(y.detach().permute(0, 2, 3, 1).reshape(60, 128).numpy()))
    go = torch.randn(y.shape, generator=torch.Generator().manual_seed(4))
    want = torch.autograd.grad(plain, (x, conv.weight, conv.bias), go)
    got = torch.autograd.grad(y, (x, conv.weight, conv.bias), go)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # through the normalisation: mean and var from the records, the backward untouched
    bn = PC.BatchNorm2d(128).train()
    out_a = bn.forward_relu(y.detach().clone(), partials=partials)
    bn_b = PC.BatchNorm2d(128).train()
    out_b = bn_b.forward_relu(y.detach().clone())
    assert float((out_a - out_b).detach().abs().max()) <= 1e-5 * float(out_b.detach().abs().max())
    assert float((bn.running_var - bn_b.running_var).abs().max()) <= 1e-5 * float(bn_b.running_var.abs().max())


def test_plain_c_double_changes_no_bit():
    """A back-end without the entries (the plain-C double): the flag is set and a training forward is what it was, bit for bit."""
    _lib.install_test_backend(cref.load(_lib.SIGNATURES))
    try:
        assert not any(_lib.has_entry(n) for n in NAMES) and not SF.conv3x3_bnstats_supported()
        net, x = _student(), _input()
        flagged = networks.route_training_convs(copy.deepcopy(net), bnstats=True)
        assert _marks(flagged) == [True] * 8
        (want_out, want), (got_out, got) = _step(net, x), _step(flagged, x)
        assert all(torch.equal(a, b) for a, b in zip(got_out, want_out)) and all(torch.equal(got[k], want[k]) for k in want)
        ra, rb = _running(flagged), _running(net)
        assert all(torch.equal(ra[k], rb[k]) for k in rb)
        with pytest.raises(NotImplementedError, match="skd_bnstats.h"):
            SF.conv3x3_split_train(torch.zeros(1, 128, 2, 2).contiguous(memory_format=torch.channels_last),
                                   torch.zeros(128, 128, 3, 3, requires_grad=True), 1, stats=True)
    finally:
        _lib.install_test_backend(None)


# ---- 4. the switch ---------------------------------------------------------------------------------------------------------------

def test_netmodel_split_bnstats_switch(monkeypatch):
    from structure_knowledge_distillation_amd.networks.kd_model import NetModel, default_args
    for name in ("SKD_SPLIT_TRAIN", "SKD_SPLIT_WGRAD", "SKD_SPLIT_NARROW", "SKD_SPLIT_NARROW_WGRAD", "SKD_SPLIT_SHORTCUT",
                 "SKD_SPLIT_BNSTATS"):
        monkeypatch.delenv(name, raising=False)
    assert default_args().split_bnstats is False
    monkeypatch.setenv("SKD_SPLIT_BNSTATS", "1")
    assert default_args().split_bnstats is True and default_args(split_bnstats=False).split_bnstats is False
    assert default_args().split_train is False and default_args().split_shortcut is False and default_args().split_wgrad is False
    for off in ("0", "", "true", "yes", "2"):                       # parsed like its siblings: "1" alone switches it on
        monkeypatch.setenv("SKD_SPLIT_BNSTATS", off)
        assert default_args().split_bnstats is False and default_args(split_bnstats=True).split_bnstats is True
    _lib.install_test_backend(cref.load(_lib.SIGNATURES))
    try:
        kw = dict(device=torch.device("cpu"), batch_size=2, ho=False)
        model = NetModel(default_args(**kw))
        assert _marks(model.student) == [False] * 8 and model.split_bnstats is False
        for pre in (dict(), dict(split_narrow=True), dict(split_shortcut=True)):     # without split_train it routes nothing
            model = NetModel(default_args(split_bnstats=True, **pre, **kw))
            assert not model.split_bnstats and not any(_marks(model.student)), pre
        model = NetModel(default_args(split_train=True, **kw))
        assert _marks(model.student) == [False] * 8 and not model.split_bnstats
        model = NetModel(default_args(split_train=True, split_bnstats=True, **kw))
        assert _marks(model.student) == [True] * 8 and model.split_bnstats and not model.split_wgrad and not model.split_shortcut
        assert not any(getattr(m, "_skd_train_bnstats", False) for m in model.teacher.modules())
        # under the plain-C double the flagged student's training forward is the unflagged one's, bit for bit
        torch.manual_seed(0)
        plain = NetModel(default_args(split_train=True, **kw)).student.train()
        for m in plain.modules():
            if isinstance(m, torch.nn.Dropout2d):
                m.p = 0.0
        flagged = networks.route_training_convs(copy.deepcopy(plain), bnstats=True)
        x = torch.randn(2, 3, 33, 33, generator=torch.Generator().manual_seed(2))
        assert all(torch.equal(a, b) for a, b in zip(plain(x), flagged(x)))
        model = NetModel(default_args(split_train=True, split_wgrad=True, split_narrow=True, split_shortcut=True,
                                      split_bnstats=True, **kw))
        assert _marks(model.student) == [True] * 8 and model.split_wgrad and model.split_narrow and model.split_shortcut
        monkeypatch.setenv("SKD_SPLIT_BNSTATS", "1")
        assert _marks(NetModel(default_args(**kw)).student) == [False] * 8
        monkeypatch.setenv("SKD_SPLIT_TRAIN", "1")
        assert _marks(NetModel(default_args(**kw)).student) == [True] * 8
    finally:
        _lib.install_test_backend(None)


def test_docs_name_the_statistics_form():
    assert "skd_bnstats.h" in SF.conv3x3_split_train.__doc__ and "BNSTATS_ROUTING_EXCLUDED" in PC.route_training_convs.__doc__
    with open(_lib.header_path("skd_bnstats.h")) as fh:
        text = fh.read()
    for phrase in ("32-row", "M2", "no pivot", "same bits on every call", "not 8-byte aligned"):
        assert phrase in text, phrase
