"""Guard-banded buffers and the one table of bounds cases (test infrastructure, shared by tests/test_bounds_cpu.py and
tests/test_bounds_gpu.py; a plain module like tests/kinks.py and tests/sliding_ref.py).

The value tests of the suite allocate every output and workspace at its logical size and look at the payload only, so a
kernel that writes one row / float4 / tile past a buffer, writes past what its ``*_workspace_floats()`` query reported, or
reads past an input and multiplies what it read by zero, passes them.  Here every buffer a C-ABI entry is handed lives
inside a larger byte buffer:

    [ front guard | payload | back guard ]        one torch.uint8 allocation per buffer

  * guard length per side: max(64 KiB, 160 x row_bytes) rounded up to a multiple of 256 bytes (so the payload keeps the
    alignment of a plain allocation); row_bytes = the buffer's innermost logical row (C floats channels-last, ldm floats
    for the pair-wise panels, N floats for a GEMM output); 160 rows = "more than one tile of rows", the figure of the
    split-GEMM tests;
  * every guard byte is 0xFF (NaN as fp32, -1 as a signed integer, 255 as uint8); the payloads of pure outputs and of
    workspaces are 0xFF too, so an element a kernel should have written and did not is NaN against the expectation, and a
    kernel that reads a stray guard element and does anything but multiply it away produces NaN;
  * workspaces have exactly the size the library under test reports (``max(1, n)`` only where the entry's own value test
    does the same);
  * ``Arena.check()`` asserts that every guard byte is still 0xFF and names buffer, side and byte offsets otherwise.

A CASE is ``fn(lib, arena, *args) -> (call, outputs[, want])``: it allocates through the arena, runs whatever earlier
stage it needs, and returns ``call`` (one C-ABI call of the entry under test, returning the entry's status) and
``outputs`` = {name: (tensor or callable giving one, tolerance, floor)} in the ``close()`` form of
tests/test_kernels_gpu.py (tolerance EXACT: same bits).  ``want`` -- {name: float64 / exact tensor} -- is given by the
cases the plain-C oracle does not implement; every other case runs unchanged against the oracle on the CPU and against
libskd_hip.so on the GPU, and the oracle's outputs are the expectation.  ``run_case`` makes the call, checks the guards
and snapshots the outputs; cases with a workspace (``ws=True``) are then called a SECOND time on the same buffers -- inputs
of in-place entries restored, pure outputs re-filled with 0xFF, the workspace left as the first call left it -- because
include/skd.h promises that a workspace needs no initialisation and is owned by the caller.  ``bit=True``: the entry is
documented (and tested elsewhere) as bit-reproducible, the two results must have the same bits.

Shapes: per entry (a) the smallest ragged shapes of the entry's own parametrisation in the value tests and (b) the smallest
shape that takes each launch-form branch of its host function (the row's comment names the branch and the line that
decides it), (c) the pair-wise backward at TI = 128 with several images and channel tiles.  Tolerances are the ones of the
entry's value test, named in the comment next to them.
"""
import ctypes
import math

import torch

from structure_knowledge_distillation_amd import _lib

EXACT = 0.0            # tolerance marker: the same bits
GUARD_MIN = 64 * 1024
GUARD_ROWS = 160
FILL = 0xFF


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def guard_bytes(row_bytes):
    return -(-max(GUARD_MIN, GUARD_ROWS * int(row_bytes)) // 256) * 256


class GuardError(AssertionError):
    pass


class Arena:
    """Hands out tensors that live between two 0xFF guard bands (``guarded=False``: plain buffers, same fills)."""

    def __init__(self, device="cpu", guarded=True):
        self.device, self.guarded = torch.device(device), guarded
        self.buffers = []          # dicts: name, raw, guard, nbytes, view, kind, data

    def _new(self, name, shape, dtype, row, data, kind):
        shape = (int(shape),) if isinstance(shape, int) else tuple(int(s) for s in shape)
        item = torch.empty(0, dtype=dtype).element_size()
        nbytes = int(math.prod(shape)) * item
        g = guard_bytes((row if row else (shape[-1] if shape else 1)) * item) if self.guarded else 0
        raw = torch.full((2 * g + nbytes,), FILL, dtype=torch.uint8, device=self.device)
        view = raw[g:g + nbytes].view(dtype).view(shape)
        if data is not None:
            assert tuple(data.shape) == shape and data.dtype == dtype, (name, tuple(data.shape), shape, data.dtype, dtype)
            data = data.detach().cpu().clone()
            view.copy_(data)
        names = {b["name"] for b in self.buffers}
        base, k = name, 1
        while name in names:
            k += 1
            name = "%s#%d" % (base, k)
        self.buffers.append(dict(name=name, raw=raw, guard=g, nbytes=nbytes, view=view, kind=kind, data=data))
        return view

    def inp(self, name, data, row=None):
        """A read-only input holding ``data``."""
        return None if data is None else self._new(name, data.shape, data.dtype, row, data, "in")

    def io(self, name, data, row=None):
        """An argument the entry reads AND writes (in-place entries, accumulated gradients): restored by ``reset()``."""
        return None if data is None else self._new(name, data.shape, data.dtype, row, data, "io")

    def out(self, name, shape, dtype=torch.float32, row=None):
        """A pure output: payload 0xFF, re-filled by ``reset()``."""
        return self._new(name, shape, dtype, row, None, "out")

    def ws(self, name, nfloats):
        """A workspace of exactly ``nfloats`` floats: payload 0xFF before the first call, never touched again by the arena."""
        return self._new(name, (int(nfloats),), torch.float32, None, None, "ws")

    def reset(self):
        for b in self.buffers:
            if b["kind"] == "io":
                b["view"].copy_(b["data"])
            elif b["kind"] == "out":
                b["raw"][b["guard"]:b["guard"] + b["nbytes"]].fill_(FILL)

    def sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def check(self):
        """Every guard byte of every buffer is still 0xFF."""
        if not self.guarded:
            return
        self.sync()
        sides = []
        for b in self.buffers:
            g, n = b["guard"], b["nbytes"]
            sides.append((b, "front", b["raw"][:g], -g))
            sides.append((b, "back", b["raw"][g + n:], n))
        clean = torch.stack([(s[2] == FILL).all() for s in sides]).cpu().tolist()
        bad = []
        for ok, (b, side, band, off0) in zip(clean, sides):
            if not ok:
                idx = (band != FILL).nonzero().flatten().cpu()
                bad.append("buffer '%s' (%s, %d payload bytes): %s guard overwritten, %d byte(s), first at payload offset %d, last at %d"
                           % (b["name"], b["kind"], b["nbytes"], side, idx.numel(), int(idx[0]) + off0, int(idx[-1]) + off0))
        if bad:
            raise GuardError("; ".join(bad))


class Case:
    def __init__(self, name, fn, entries, args, ws, bit, oracle, fused):
        self.name, self.fn, self.entries, self.args = name, fn, entries, args
        self.ws, self.bit, self.oracle, self.fused = ws, bit, oracle, fused


CASES = {}


def add(name, fn, entries, *args, ws=False, bit=False, oracle=True, fused=None):
    """``entries``: the C-ABI entry (or the few entries of one pipeline) whose bounds the case covers.  ``fused``: value of
    skd_abn_set_fused() during the calls (restored to -1, the environment's default, afterwards)."""
    assert name not in CASES, name
    CASES[name] = Case(name, fn, (entries,) if isinstance(entries, str) else tuple(entries), args, ws, bit, oracle, fused)


def _snapshot(outs):
    res = {}
    for k, v in outs.items():
        t = v[0]() if callable(v[0]) else v[0]
        res[k] = t.detach().cpu().clone()
    return res


def run_case(case, lib, arena):
    """[{name: tensor on the CPU} per call], {name: (tolerance, floor)}, want or None.  Guards are checked after each call."""
    if case.fused is not None:
        assert lib.skd_abn_set_fused(case.fused) and lib.skd_abn_get_fused() == case.fused
    try:
        made = case.fn(lib, arena, *case.args)
        call, outs = made[0], made[1]
        want = made[2] if len(made) > 2 else None
        results = []
        for k in range(2 if case.ws else 1):
            if k:
                arena.reset()
            assert call() == 1, "%s: the entry refused the call" % case.name
            arena.check()
            results.append(_snapshot(outs))
    finally:
        if case.fused is not None:
            lib.skd_abn_set_fused(-1)
    return results, {k: (v[1], v[2] if len(v) > 2 else 0.0) for k, v in outs.items()}, want


def same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def compare(got, want, tols, what):
    """``close()`` of tests/test_kernels_gpu.py per output: max |got - want| <= tol * max(max |want|, floor); EXACT: same bits
    (against a float64 expectation: same values)."""
    assert set(got) == set(tols) and set(got) <= set(want), (what, sorted(got), sorted(want))
    for k, (tol, floor) in tols.items():
        g, w = got[k], want[k]
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        if tol == EXACT:
            ok = same_bits(g, w) if g.dtype == w.dtype else torch.equal(g.double(), w.double())
            assert ok, "%s: %s differs from the expectation in %d of %d elements" % (what, k, int((g.double() != w.double()).sum()), g.numel())
            continue
        g, w = g.double(), w.double()
        scale = max(float(w.abs().max()) if w.numel() else 0.0, floor, 1e-30)
        err = float((g - w).abs().max()) / scale if w.numel() else 0.0
        assert err <= tol, "%s: %s max err %.3e (rel to %.3e) > %.1e" % (what, k, err, scale, tol)      # NaN fails


def pointer_entries():
    """Every entry of the two signature tables that takes at least one pointer."""
    out = []
    for table in (_lib.SIGNATURES, _lib.ABI["skd_eval.h"]):
        out += [n for n, (_, args) in table.items() if ctypes.c_void_p in args]
    return out


# Entries without a bounds case, and why.  Nothing else may be listed (tests/test_bounds_cpu.py holds the list).
_MAILBOX = "needs a mailbox context and peer ranks: tests/test_distributed_gpu.py owns it"
_HOST = "its only pointer is a host array"
EXEMPT = {
    "skd_sync_create": _MAILBOX, "skd_sync_connect": _MAILBOX, "skd_sync_destroy": _MAILBOX, "skd_sync_all_gather": _MAILBOX,
    "skd_sync_set_timeout": _MAILBOX, "skd_abn_sync_stats": _MAILBOX, "skd_abn_sync_grad_stats": _MAILBOX,
    "skd_abn_forward_train_nhwc_sync": _MAILBOX, "skd_abn_backward_nhwc_sync": _MAILBOX, "skd_abn_relu_backward_nhwc_sync": _MAILBOX,
    "skd_status_read": _HOST, "skd_abn_sync_form_counts": _HOST, "skd_conv1x1_abn_geometry": _HOST, "skd_conv1x1_abn_tile_of": _HOST,
    "skd_ppm_pooled_floats": _HOST, "skd_ppm_nhwc_workspace_floats": _HOST, "skd_ppm_fold_nhwc_workspace_floats": _HOST,
}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(values):
    return (ctypes.c_int * len(values))(*[int(v) for v in values])


def _ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


ACT_NONE, ACT_LEAKY, ACT_ELU, ACT_RELU = 0, 1, 2, 3
EPS, SLOPE, MOM = 1e-5, 0.01, 0.1


def _act(y, act):
    if act == ACT_LEAKY:
        return torch.where(y < 0, y * SLOPE, y)
    if act == ACT_RELU:
        return torch.relu(y)
    return y


# =====================================================================================================================
# 1. InPlace-ABN, planar (N, C, S).  Shapes (a): (2, 3, 1), (1, 5, 7), (5, 130, 9) of ABN_SHAPES.  Tolerances:
#    test_abn_train_forward_backward / test_abn_relu_training_fusion / test_abn_legacy_entries of tests/test_kernels_gpu.py.
# =====================================================================================================================
# (b) the three cuts of make_plan(), csrc/abn.hip:35-55 (P partial slots per channel in the workspace): S small and one group of
# rows per channel (the three shapes of (a)); S small and several groups, the last one ragged ((3, 2, 2731): 2 rows per item, 3 rows);
# 2 S >= kChunk: rows cut into pieces, the last one ragged ((2, 7, 8193) of ABN_SHAPES there: pieces of 4100 and 4093)
ABN_SHAPES = [(2, 3, 1), (1, 5, 7), (5, 130, 9), (3, 2, 2731), (2, 7, 8193)]


def _abn_data(N, C, S, seed):
    """The recipe of test_kernels_gpu._abn_inputs plus everything a backward entry reads, all seeded and computed on the CPU
    so that both libraries get the same bits: z (a saved leaky-ReLU output), dz, batch statistics, a ReLU output, edz / eydz."""
    g = _gen(seed)
    d = {}
    d["x"] = torch.randn(N, C, S, generator=g) * 3.0 + torch.randn(1, C, 1, generator=g) * 5.0
    d["w"], d["b"] = torch.randn(C, generator=g), torch.randn(C, generator=g)
    if C >= 3:
        d["w"][0] = 0.0
        d["w"][1] = -abs(d["w"][1])
    d["rm"], d["rv"] = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    d["r"], d["dz"] = torch.randn(N, C, S, generator=g), torch.randn(N, C, S, generator=g)
    xd = d["x"].double()
    d["mean"] = xd.mean((0, 2)).float()
    d["var"] = (xd.var((0, 2), unbiased=False).float() + 0.01)         # (+ 0.01: S = 1, N = 1 would give var 0)
    v = lambda t: t.view(1, C, 1)
    y = (d["x"] - v(d["mean"])) / torch.sqrt(v(d["var"]) + EPS) * (v(d["w"]).abs() + EPS) + v(d["b"])
    d["z"] = _act(y, ACT_LEAKY)
    d["out"], d["out_r"] = torch.relu(y), torch.relu(y + d["r"])
    d["edz"], d["eydz"] = torch.randn(C, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1
    d["mul"] = float(((d["w"].abs() + EPS) / torch.sqrt(d["var"] + EPS)).max())
    d["dzmax"] = float(d["dz"].abs().max())
    return d


def abn_forward_train(lib, A, N, C, S, act):
    d = _abn_data(N, C, S, N * 1000 + C + S)
    x, w, b, rm, rv = A.io("x", d["x"]), A.inp("weight", d["w"]), A.inp("bias", d["b"]), A.io("running_mean", d["rm"]), A.io("running_var", d["rv"])
    m, v = A.out("mean", C), A.out("var", C)
    ws = A.ws("workspace", max(1, lib.skd_abn_workspace_floats(N, C, S)))
    call = lambda: lib.skd_abn_forward_train(N, C, S, P(x), P(w), P(b), P(rm), P(rv), P(m), P(v), MOM, EPS, act, SLOPE, P(ws), None)
    return call, {"mean": (m, 2e-5), "var": (v, 5e-5), "running_mean": (rm, 2e-6), "running_var": (rv, 1e-5), "z": (x, 3e-5)}


def abn_stats(lib, A, N, C, S):
    d = _abn_data(N, C, S, 7 + S)
    x, m, v = A.inp("x", d["x"]), A.out("mean", C), A.out("var", C)
    ws = A.ws("workspace", max(1, lib.skd_abn_workspace_floats(N, C, S)))
    return (lambda: lib.skd_abn_stats(N, C, S, P(x), P(m), P(v), P(ws), None)), {"mean": (m, 2e-5), "var": (v, 5e-5)}


def abn_apply(lib, A, N, C, S, act, residual):
    """skd_abn_apply / skd_abn_apply_residual, in place (test_abn_fused_relu_and_residual: 2e-5)."""
    d = _abn_data(N, C, S, S)
    x, rm, rv, w, b = A.io("x", d["x"]), A.inp("mean", d["rm"]), A.inp("var", d["rv"]), A.inp("weight", d["w"]), A.inp("bias", d["b"])
    if residual:
        r = A.inp("residual", d["r"])
        call = lambda: lib.skd_abn_apply_residual(N, C, S, P(x), P(r), P(rm), P(rv), P(w), P(b), EPS, act, SLOPE, None)
    else:
        call = lambda: lib.skd_abn_apply(N, C, S, P(x), P(rm), P(rv), P(w), P(b), EPS, act, SLOPE, None)
    return call, {"z": (x, 2e-5)}


def abn_apply_to(lib, A, N, C, S, residual):
    d = _abn_data(N, C, S, S + 7)
    x, r, out = A.inp("x", d["x"]), A.inp("residual", d["r"] if residual else None), A.out("out", (N, C, S))
    m, v, w, b = A.inp("mean", d["mean"]), A.inp("var", d["var"]), A.inp("weight", d["w"]), A.inp("bias", d["b"])
    call = lambda: lib.skd_abn_apply_to(N, C, S, P(x), P(r), P(out), P(m), P(v), P(w), P(b), EPS, ACT_RELU, 0.0, None)
    return call, {"out": (out, 3e-5)}


def abn_forward_train_to(lib, A, N, C, S, residual):
    d = _abn_data(N, C, S, S + 7)
    x, r, out = A.inp("x", d["x"]), A.inp("residual", d["r"] if residual else None), A.out("out", (N, C, S))
    w, b, rm, rv = A.inp("weight", d["w"]), A.inp("bias", d["b"]), A.io("running_mean", d["rm"]), A.io("running_var", d["rv"])
    m, v = A.out("mean", C), A.out("var", C)
    ws = A.ws("workspace", max(1, lib.skd_abn_workspace_floats(N, C, S)))
    call = lambda: lib.skd_abn_forward_train_to(N, C, S, P(x), P(r), P(out), P(w), P(b), P(rm), P(rv), P(m), P(v), MOM, EPS, ACT_RELU, 0.0, P(ws), None)
    return call, {"mean": (m, 2e-5), "var": (v, 5e-5), "running_mean": (rm, 2e-6), "running_var": (rv, 1e-5), "out": (out, 3e-5)}


def abn_relu_backward_reduce(lib, A, N, C, S):
    d = _abn_data(N, C, S, S + 7)
    x, o, dz, m, v = A.inp("x", d["x"]), A.inp("out", d["out"]), A.inp("dout", d["dz"]), A.inp("mean", d["mean"]), A.inp("var", d["var"])
    e, ey = A.out("edz", C), A.out("eydz", C)
    ws = A.ws("workspace", max(1, lib.skd_abn_workspace_floats(N, C, S)))
    call = lambda: lib.skd_abn_relu_backward_reduce(N, C, S, P(x), P(o), P(dz), P(m), P(v), P(e), P(ey), EPS, P(ws), None)
    return call, {"edz": (e, 5e-5), "eydz": (ey, 5e-5)}


def abn_relu_backward_dx(lib, A, N, C, S, residual):
    d = _abn_data(N, C, S, S + 7)
    x, o, dz = A.inp("x", d["x"]), A.inp("out", d["out_r"] if residual else d["out"]), A.inp("dout", d["dz"])
    m, v, w, e, ey = A.inp("mean", d["mean"]), A.inp("var", d["var"]), A.inp("weight", d["w"]), A.inp("edz", d["edz"]), A.inp("eydz", d["eydz"])
    dx, dres = A.out("dx", (N, C, S)), (A.out("dres", (N, C, S)) if residual else None)
    dw, db = A.io("dweight", torch.zeros(C)), A.io("dbias", torch.zeros(C))
    call = lambda: lib.skd_abn_relu_backward_dx(N, C, S, P(x), P(o), P(dz), P(m), P(v), P(w), P(e), P(ey), P(dx), P(dres), P(dw), P(db), EPS, 1, None)
    outs = {"dx": (dx, 1e-4, d["dzmax"] * d["mul"]), "dweight": (dw, 5e-5, 1e-6), "dbias": (db, 5e-5, 1e-6)}
    if residual:
        outs["dres"] = (dres, EXACT)                                   # dres = dout * (out > 0), exact
    return call, outs


def abn_backward_reduce(lib, A, N, C, S):
    d = _abn_data(N, C, S, 99 + S)
    z, dz, w, b, e, ey = A.inp("z", d["z"]), A.inp("dz", d["dz"]), A.inp("weight", d["w"]), A.inp("bias", d["b"]), A.out("edz", C), A.out("eydz", C)
    ws = A.ws("workspace", max(1, lib.skd_abn_workspace_floats(N, C, S)))
    call = lambda: lib.skd_abn_backward_reduce(N, C, S, P(z), P(dz), P(w), P(b), P(e), P(ey), EPS, ACT_LEAKY, SLOPE, P(ws), None)
    return call, {"edz": (e, 5e-5), "eydz": (ey, 5e-5)}


def abn_backward_dx(lib, A, N, C, S):
    d = _abn_data(N, C, S, 99 + S)
    z, dz, v, w, b = A.inp("z", d["z"]), A.inp("dz", d["dz"]), A.inp("var", d["var"]), A.inp("weight", d["w"]), A.inp("bias", d["b"])
    e, ey, dx = A.inp("edz", d["edz"]), A.inp("eydz", d["eydz"]), A.out("dx", (N, C, S))
    dw, db = A.io("dweight", torch.zeros(C)), A.io("dbias", torch.zeros(C))
    call = lambda: lib.skd_abn_backward_dx(N, C, S, P(z), P(dz), P(v), P(w), P(b), P(e), P(ey), P(dx), P(dw), P(db), EPS, ACT_LEAKY, SLOPE, None)
    return call, {"dx": (dx, 1e-4, d["dzmax"] * d["mul"]), "dweight": (dw, 5e-5, 1e-6), "dbias": (db, 5e-5, 1e-6)}


def abn_backward(lib, A, N, C, S):
    d = _abn_data(N, C, S, 99 + S)
    z, dz, v, w, b = A.inp("z", d["z"]), A.inp("dz", d["dz"]), A.inp("var", d["var"]), A.inp("weight", d["w"]), A.inp("bias", d["b"])
    e, ey, dx = A.out("edz", C), A.out("eydz", C), A.out("dx", (N, C, S))
    dw, db = A.io("dweight", torch.zeros(C)), A.io("dbias", torch.zeros(C))
    ws = A.ws("workspace", max(1, lib.skd_abn_workspace_floats(N, C, S)))
    call = lambda: lib.skd_abn_backward(N, C, S, P(z), P(dz), P(v), P(w), P(b), P(e), P(ey), P(dx), P(dw), P(db), EPS, ACT_LEAKY, SLOPE, 1, P(ws), None)
    return call, {"edz": (e, 5e-5), "eydz": (ey, 5e-5), "dx": (dx, 1e-4, d["dzmax"] * d["mul"]), "dweight": (dw, 5e-5, 1e-6), "dbias": (db, 5e-5, 1e-6)}


def bn_legacy(lib, A, N, C, S, which):
    """The reference's original exports (test_abn_legacy_entries)."""
    d = _abn_data(N, C, S, 11)
    if which == "mean_var":
        x, m, v = A.inp("x", d["x"]), A.out("mean", C), A.out("var", C)
        return (lambda: lib.skd_bn_mean_var(N, C, S, P(x), P(m), P(v), None)), {"mean": (m, 2e-5), "var": (v, 5e-5)}
    if which == "forward":
        x, m, v, w, b = A.inp("x", d["x"]), A.inp("mean", d["mean"]), A.inp("var", d["var"]), A.inp("weight", d["w"]), A.inp("bias", d["b"])
        y, z = A.out("y", (N, C, S)), A.out("z", (N, C, S))
        return (lambda: lib.skd_bn_forward(N, C, S, P(x), P(m), P(v), P(w), P(b), P(y), P(z), EPS, None)), {"y": (y, 2e-5), "z": (z, 2e-5)}
    z, dz, w, b = A.inp("z", d["z"]), A.inp("dz", d["dz"]), A.inp("weight", d["w"]), A.inp("bias", d["b"])
    if which == "edz_eydz":
        e, ey = A.out("edz", C), A.out("eydz", C)
        return (lambda: lib.skd_bn_edz_eydz(N, C, S, P(z), P(dz), P(w), P(b), P(e), P(ey), EPS, None)), {"edz": (e, 5e-5), "eydz": (ey, 5e-5)}
    v, e, ey, dx = A.inp("var", d["var"]), A.inp("edz", d["edz"]), A.inp("eydz", d["eydz"]), A.out("dx", (N, C, S))
    dw, db = A.io("dweight", torch.ones(C)), A.io("dbias", torch.ones(C))                      # accumulated (+=) into ones
    call = lambda: lib.skd_bn_backward(N, C, S, P(dz), P(z), P(v), P(w), P(b), P(e), P(ey), P(dx), P(dw), P(db), EPS, None)
    return call, {"dx": (dx, 5e-5), "dweight": (dw, 5e-5), "dbias": (db, 5e-5)}


def elementwise(lib, A, n, name):
    """skd_leaky_relu / skd_elu / skd_elu_inv and the two backward forms on a flat buffer (test_abn_legacy_entries: 1e-5)."""
    g = _gen(n)
    a = (torch.rand(n, generator=g) - 0.7) if name == "skd_elu_inv" else torch.randn(n, generator=g)
    extra = (SLOPE,) if "leaky" in name else ()
    if name.endswith("backward"):
        x, dz = A.inp("x", a), A.io("dz", torch.randn(n, generator=g))
        return (lambda: getattr(lib, name)(n, P(x), P(dz), *extra, None)), {"dz": (dz, 1e-5)}
    x = A.io("x", a)
    return (lambda: getattr(lib, name)(n, P(x), *extra, None)), {"x": (x, 1e-5)}


def abn_combine_stats(lib, A, G, C, weighted):
    """test_abn_combine_stats: 1e-6."""
    g = _gen(G * C)
    gathered = torch.cat([torch.randn(G, 1, C, generator=g), torch.rand(G, 1, C, generator=g) + 0.1], 1).contiguous()
    counts = torch.arange(1, G + 1, dtype=torch.float64) * 7
    wts = A.inp("weights", (counts / counts.sum()).float()) if weighted else None
    ga, m, v = A.inp("gathered", gathered), A.out("mean", C), A.out("var", C)
    rm, rv = A.io("running_mean", torch.randn(C, generator=g)), A.io("running_var", torch.rand(C, generator=g) + 0.5)
    n = float(counts[G - 1]) if weighted else float(4225 * 8 * G)
    call = lambda: lib.skd_abn_combine_stats(G, C, P(ga), P(wts), G - 1 if weighted else 0, P(m), P(v), P(rm), P(rv), MOM, n, None)
    return call, {"mean": (m, 1e-6), "var": (v, 1e-6), "running_mean": (rm, 1e-6), "running_var": (rv, 1e-6)}


def abn_update_running(lib, A, C):
    """No value test of its own: the running-statistics bound of the module docstring of test_kernels_gpu.py (1e-6)."""
    g = _gen(C)
    rm, rv = A.io("running_mean", torch.randn(C, generator=g)), A.io("running_var", torch.rand(C, generator=g) + 0.5)
    m, v = A.inp("mean", torch.randn(C, generator=g)), A.inp("var", torch.rand(C, generator=g) + 0.1)
    call = lambda: lib.skd_abn_update_running(C, P(rm), P(rv), P(m), P(v), MOM, 33800.0, None)
    return call, {"running_mean": (rm, 1e-6), "running_var": (rv, 1e-6)}


for _s in ABN_SHAPES:
    _t = "%dx%dx%d" % _s
    add("abn_forward_train-" + _t, abn_forward_train, "skd_abn_forward_train", *_s, ACT_LEAKY, ws=True)
    add("abn_stats-" + _t, abn_stats, "skd_abn_stats", *_s, ws=True)
    add("abn_apply-" + _t, abn_apply, "skd_abn_apply", *_s, ACT_LEAKY, False)
    add("abn_apply_residual-" + _t, abn_apply, "skd_abn_apply_residual", *_s, ACT_RELU, True)
    add("abn_apply_to-" + _t, abn_apply_to, "skd_abn_apply_to", *_s, True)
    add("abn_forward_train_to-" + _t, abn_forward_train_to, "skd_abn_forward_train_to", *_s, _s[1] != 5, ws=True)
    add("abn_relu_backward_reduce-" + _t, abn_relu_backward_reduce, "skd_abn_relu_backward_reduce", *_s, ws=True)
    add("abn_relu_backward_dx-" + _t, abn_relu_backward_dx, "skd_abn_relu_backward_dx", *_s, _s[1] != 5)
    add("abn_backward_reduce-" + _t, abn_backward_reduce, "skd_abn_backward_reduce", *_s, ws=True)
    add("abn_backward_dx-" + _t, abn_backward_dx, "skd_abn_backward_dx", *_s)
    add("abn_backward-" + _t, abn_backward, "skd_abn_backward", *_s, ws=True)
add("abn_forward_train-none-1x5x7", abn_forward_train, "skd_abn_forward_train", 1, 5, 7, ACT_NONE, ws=True)
for _w in ("mean_var", "forward", "edz_eydz", "backward"):
    for _s in ((2, 3, 1), (5, 130, 9)):
        add("bn_%s-%dx%dx%d" % ((_w,) + _s), bn_legacy, "skd_bn_" + _w, *_s, _w)
for _n in ("skd_leaky_relu", "skd_elu", "skd_elu_inv", "skd_leaky_relu_backward", "skd_elu_backward"):
    add(_n[4:] + "-1", elementwise, _n, 1, _n)
    add(_n[4:] + "-4629", elementwise, _n, 4629, _n)                   # 3 * 6 * 257 + 3: several workgroups, a ragged float4 tail
add("abn_combine_stats-2x6", abn_combine_stats, "skd_abn_combine_stats", 2, 6, False)
add("abn_combine_stats-weighted-3x1000", abn_combine_stats, "skd_abn_combine_stats", 3, 1000, True)
add("abn_update_running-6", abn_update_running, "skd_abn_update_running", 6)
add("abn_update_running-1000", abn_update_running, "skd_abn_update_running", 1000)


# =====================================================================================================================
# 2. InPlace-ABN, channels-last (rows, C).  Shapes (a): (35, 8) and (7, 20) of test_abn_apply_nhwc, (50, 4) of
#    test_abn_nhwc_training (the training entries need C a power of two), and (3000, 256) of
#    test_abn_nhwc_reduction_handoff_stress: several channel blocks and row groups, i.e. several partial slots and ticket
#    counters.  (b): the three entries that consult the switch -- skd_abn_forward_train_nhwc, skd_abn_backward_nhwc and
#    skd_abn_relu_backward_nhwc, through fwd_fused_geom / bwd_fused_geom, csrc/abn_fused.hip:491-498 -- run with
#    skd_abn_set_fused(1) and (0): the register-resident one-launch pass against the separate statistics / reduce and apply
#    launches.  make_fuse_geom() (:67) fits all three shapes on a whole device (one row per thread; (3000, 256): 4 channel
#    blocks x 47 row groups = 188 workgroups, more rows per thread under a lower cap); each fused-1 case asserts on the host that it
#    fits under the cap of the library it is about to call (_pin_launch_form), so it cannot quietly take the other branch.
#    The reductions (stats, backward_reduce, the two relu_backward_reduce forms) have one launch form and run once.
#    Tolerances: test_abn_nhwc_training and test_abn_nhwc_one_call_backward of tests/test_kernels_gpu.py.
# =====================================================================================================================
def _nhwc_data(rows, C, seed):
    d = _abn_data(rows, C, 1, seed)
    for k in ("x", "r", "dz", "z", "out", "out_r"):
        d[k] = d[k].reshape(rows, C).contiguous()
    return d


FUSE_FWD_MAX_NR, FUSE_BWD_MAX_NR = 17, 9       # kFuseFwdMaxNR / kFuseBwdMaxNR, csrc/abn_fused.hip:335


def one_launch_fits(rows, C, nr_max, max_wg):
    """make_fuse_geom() of csrc/abn_fused.hip:67-78 (on make_red_geom(), csrc/abn_dev.hpp:186-201) restated on the host: does the
    register-resident one-launch pass take a (rows, C) tensor with at most ``max_wg`` co-resident 1024-thread workgroups?"""
    if max_wg < 4 or rows <= 0 or C < 4 or C > 1024 or C & (C - 1):
        return False
    CB = 4 if C >= 256 else (2 if C >= 128 else 1)
    rpp = 1024 // (C // 4 // CB)
    RG = min(-(-rows // rpp), max_wg // CB)
    return -(-rows // (RG * rpp)) <= nr_max


def _pin_launch_form(lib, rows, C, nr_max):
    """With skd_abn_set_fused(1) the case must really take the one-launch pass: the geometry has to fit under the workgroup cap
    of the library under test (the device's compute-unit count, or what a caller lowered it to)."""
    if lib.skd_abn_get_fused() == 1:
        cap = lib.skd_abn_set_fused_max_workgroups(-1)              # a query: a negative value changes nothing
        assert one_launch_fits(rows, C, nr_max, cap), "(%d, %d) does not fit the one-launch form under a cap of %d workgroups" % (rows, C, cap)


def _nhwc_ws(lib, A, rows, C):
    return A.ws("workspace", max(1, lib.skd_abn_nhwc_workspace_floats(rows, C)))


def abn_apply_nhwc(lib, A, rows, C, act, residual, to):
    """skd_abn_apply_nhwc (in place) / skd_abn_apply_nhwc_to (test_abn_apply_nhwc: 2e-5; apply_to: 3e-5)."""
    d = _nhwc_data(rows, C, rows + C)
    r, m, v, w, b = A.inp("residual", d["r"] if residual else None), A.inp("mean", d["rm"]), A.inp("var", d["rv"]), A.inp("weight", d["w"]), A.inp("bias", d["b"])
    if to:
        x, out = A.inp("x", d["x"]), A.out("out", (rows, C))
        call = lambda: lib.skd_abn_apply_nhwc_to(rows, C, P(x), P(r), P(out), P(m), P(v), P(w), P(b), EPS, act, SLOPE, None)
        return call, {"out": (out, 3e-5)}
    x = A.io("x", d["x"])
    return (lambda: lib.skd_abn_apply_nhwc(rows, C, P(x), P(r), P(m), P(v), P(w), P(b), EPS, act, SLOPE, None)), {"z": (x, 2e-5)}


def abn_stats_nhwc(lib, A, rows, C):
    d = _nhwc_data(rows, C, rows + C)
    x, m, v, ws = A.inp("x", d["x"]), A.out("mean", C), A.out("var", C), _nhwc_ws(lib, A, rows, C)
    return (lambda: lib.skd_abn_stats_nhwc(rows, C, P(x), P(m), P(v), P(ws), None)), {"mean": (m, 2e-5), "var": (v, 5e-5)}


def abn_forward_train_nhwc(lib, A, rows, C, act, residual):
    """act none / leaky: in place (out == x, the same guarded view passed twice); ReLU: out of place, optional residual."""
    _pin_launch_form(lib, rows, C, FUSE_FWD_MAX_NR)
    d = _nhwc_data(rows, C, rows + C)
    w, b, rm, rv = A.inp("weight", d["w"]), A.inp("bias", d["b"]), A.io("running_mean", d["rm"]), A.io("running_var", d["rv"])
    m, v, ws = A.out("mean", C), A.out("var", C), _nhwc_ws(lib, A, rows, C)
    if act == ACT_RELU:
        x, r, out = A.inp("x", d["x"]), A.inp("residual", d["r"] if residual else None), A.out("out", (rows, C))
    else:
        x = out = A.io("x", d["x"])
        r = None
    call = lambda: lib.skd_abn_forward_train_nhwc(rows, C, P(x), P(r), P(out), P(w), P(b), P(rm), P(rv), P(m), P(v), MOM, EPS, act, SLOPE if act != ACT_RELU else 0.0, P(ws), None)
    return call, {"mean": (m, 2e-5), "var": (v, 5e-5), "running_mean": (rm, 2e-6), "running_var": (rv, 1e-5), "out": (out, 3e-5)}


def abn_backward_reduce_nhwc(lib, A, rows, C):
    d = _nhwc_data(rows, C, rows + C)
    z, dz, w, b, e, ey, ws = A.inp("z", d["z"]), A.inp("dz", d["dz"]), A.inp("weight", d["w"]), A.inp("bias", d["b"]), A.out("edz", C), A.out("eydz", C), _nhwc_ws(lib, A, rows, C)
    call = lambda: lib.skd_abn_backward_reduce_nhwc(rows, C, P(z), P(dz), P(w), P(b), P(e), P(ey), EPS, ACT_LEAKY, SLOPE, P(ws), None)
    return call, {"edz": (e, 5e-5), "eydz": (ey, 5e-5)}


def abn_backward_dx_nhwc(lib, A, rows, C):
    d = _nhwc_data(rows, C, rows + C)
    z, dz, v, w, b = A.inp("z", d["z"]), A.inp("dz", d["dz"]), A.inp("var", d["var"]), A.inp("weight", d["w"]), A.inp("bias", d["b"])
    e, ey, dx = A.inp("edz", d["edz"]), A.inp("eydz", d["eydz"]), A.out("dx", (rows, C))
    dw, db = A.io("dweight", torch.zeros(C)), A.io("dbias", torch.zeros(C))
    call = lambda: lib.skd_abn_backward_dx_nhwc(rows, C, P(z), P(dz), P(v), P(w), P(b), P(e), P(ey), P(dx), P(dw), P(db), EPS, ACT_LEAKY, SLOPE, 1, None)
    return call, {"dx": (dx, 1e-4, d["dzmax"] * d["mul"]), "dweight": (dw, 5e-5, 1e-6), "dbias": (db, 5e-5, 1e-6)}


def abn_backward_nhwc(lib, A, rows, C):
    """One call, reduce + dx; dweight / dbias WRITTEN (accumulate = 0) into 0xFF payloads (test_abn_nhwc_one_call_backward)."""
    _pin_launch_form(lib, rows, C, FUSE_BWD_MAX_NR)
    d = _nhwc_data(rows, C, rows * 3 + C)
    z, dz, v, w, b = A.inp("z", d["z"]), A.inp("dz", d["dz"]), A.inp("var", d["var"]), A.inp("weight", d["w"]), A.inp("bias", d["b"])
    e, ey, dx, dw, db, ws = A.out("edz", C), A.out("eydz", C), A.out("dx", (rows, C)), A.out("dweight", C), A.out("dbias", C), _nhwc_ws(lib, A, rows, C)
    call = lambda: lib.skd_abn_backward_nhwc(rows, C, P(z), P(dz), P(v), P(w), P(b), P(e), P(ey), P(dx), P(dw), P(db), EPS, ACT_LEAKY, SLOPE, 0, P(ws), None)
    return call, {"edz": (e, 5e-5), "eydz": (ey, 5e-5), "dx": (dx, 1e-4, d["dzmax"] * d["mul"]), "dweight": (dw, 5e-5, 1e-6), "dbias": (db, 5e-5, 1e-6)}


def abn_relu_backward_reduce_nhwc(lib, A, rows, C, from_x):
    d = _nhwc_data(rows, C, rows + C)
    x, dz, m, v, e, ey, ws = A.inp("x", d["x"]), A.inp("dz", d["dz"]), A.inp("mean", d["mean"]), A.inp("var", d["var"]), A.out("edz", C), A.out("eydz", C), _nhwc_ws(lib, A, rows, C)
    if from_x:
        w, b = A.inp("weight", d["w"]), A.inp("bias", d["b"])
        call = lambda: lib.skd_abn_relu_backward_reduce_nhwc_x(rows, C, P(x), P(dz), P(m), P(v), P(w), P(b), P(e), P(ey), EPS, P(ws), None)
    else:
        o = A.inp("out", d["out"])
        call = lambda: lib.skd_abn_relu_backward_reduce_nhwc(rows, C, P(x), P(o), P(dz), P(m), P(v), P(e), P(ey), EPS, P(ws), None)
    return call, {"edz": (e, 5e-5), "eydz": (ey, 5e-5)}


def abn_relu_backward_dx_nhwc(lib, A, rows, C, from_x, residual):
    d = _nhwc_data(rows, C, rows + C)
    x, dz, m, v, w = A.inp("x", d["x"]), A.inp("dz", d["dz"]), A.inp("mean", d["mean"]), A.inp("var", d["var"]), A.inp("weight", d["w"])
    e, ey, dx = A.inp("edz", d["edz"]), A.inp("eydz", d["eydz"]), A.out("dx", (rows, C))
    dw, db = A.io("dweight", torch.zeros(C)), A.io("dbias", torch.zeros(C))
    outs = {"dx": (dx, 1e-4, d["dzmax"] * d["mul"]), "dweight": (dw, 5e-5, 1e-6), "dbias": (db, 5e-5, 1e-6)}
    if from_x:
        b = A.inp("bias", d["b"])
        call = lambda: lib.skd_abn_relu_backward_dx_nhwc_x(rows, C, P(x), P(dz), P(m), P(v), P(w), P(b), P(e), P(ey), P(dx), P(dw), P(db), EPS, 1, None)
    else:
        o, dres = A.inp("out", d["out_r"] if residual else d["out"]), (A.out("dres", (rows, C)) if residual else None)
        call = lambda: lib.skd_abn_relu_backward_dx_nhwc(rows, C, P(x), P(o), P(dz), P(m), P(v), P(w), P(e), P(ey), P(dx), P(dres), P(dw), P(db), EPS, 1, None)
        if residual:
            outs["dres"] = (dres, EXACT)
    return call, outs


def abn_relu_backward_nhwc(lib, A, rows, C, residual):
    _pin_launch_form(lib, rows, C, FUSE_BWD_MAX_NR)
    d = _nhwc_data(rows, C, rows * 3 + C)
    x, o, dz = A.inp("x", d["x"]), A.inp("out", d["out_r"] if residual else d["out"]), A.inp("dz", d["dz"])
    m, v, w, b = A.inp("mean", d["mean"]), A.inp("var", d["var"]), A.inp("weight", d["w"]), A.inp("bias", d["b"])
    e, ey, dx, dres = A.out("edz", C), A.out("eydz", C), A.out("dx", (rows, C)), (A.out("dres", (rows, C)) if residual else None)
    dw, db, ws = A.out("dweight", C), A.out("dbias", C), _nhwc_ws(lib, A, rows, C)
    call = lambda: lib.skd_abn_relu_backward_nhwc(rows, C, P(x), P(o), P(dz), P(m), P(v), P(w), P(b), P(e), P(ey), P(dx), P(dres), P(dw), P(db), EPS, 0, P(ws), None)
    outs = {"edz": (e, 5e-5), "eydz": (ey, 5e-5), "dx": (dx, 1e-4, d["dzmax"] * d["mul"]), "dweight": (dw, 5e-5, 1e-6), "dbias": (db, 5e-5, 1e-6)}
    if residual:
        outs["dres"] = (dres, EXACT)
    return call, outs


for _rows, _C in ((35, 8), (7, 20), (50, 4)):
    _t = "%dx%d" % (_rows, _C)
    add("abn_apply_nhwc-" + _t, abn_apply_nhwc, "skd_abn_apply_nhwc", _rows, _C, ACT_LEAKY, _C != 8, False)
    if _C != 20:                                                       # the `_to` form shares the training geometry: C a power of two
        add("abn_apply_nhwc_to-" + _t, abn_apply_nhwc, "skd_abn_apply_nhwc_to", _rows, _C, ACT_RELU, _C == 8, True)
for _rows, _C in ((35, 8), (50, 4), (3000, 256)):
    _t = "%dx%d" % (_rows, _C)
    add("abn_backward_dx_nhwc-" + _t, abn_backward_dx_nhwc, "skd_abn_backward_dx_nhwc", _rows, _C)
    add("abn_relu_backward_dx_nhwc-" + _t, abn_relu_backward_dx_nhwc, "skd_abn_relu_backward_dx_nhwc", _rows, _C, False, _C == 8)
    add("abn_relu_backward_dx_nhwc_x-" + _t, abn_relu_backward_dx_nhwc, "skd_abn_relu_backward_dx_nhwc_x", _rows, _C, True, False)
    add("abn_stats_nhwc-" + _t, abn_stats_nhwc, "skd_abn_stats_nhwc", _rows, _C, ws=True, bit=True)
    add("abn_backward_reduce_nhwc-" + _t, abn_backward_reduce_nhwc, "skd_abn_backward_reduce_nhwc", _rows, _C, ws=True, bit=True)
    add("abn_relu_backward_reduce_nhwc-" + _t, abn_relu_backward_reduce_nhwc, "skd_abn_relu_backward_reduce_nhwc", _rows, _C, False, ws=True, bit=True)
    add("abn_relu_backward_reduce_nhwc_x-" + _t, abn_relu_backward_reduce_nhwc, "skd_abn_relu_backward_reduce_nhwc_x", _rows, _C, True, ws=True, bit=True)
    for _f in (1, 0):                                                  # one-launch / separate launches, csrc/abn_fused.hip:491-498
        _u = _t + ("-fused1" if _f else "-fused0")
        add("abn_forward_train_nhwc-leaky-" + _u, abn_forward_train_nhwc, "skd_abn_forward_train_nhwc", _rows, _C, ACT_LEAKY, False, ws=True, fused=_f)
        add("abn_forward_train_nhwc-relu-" + _u, abn_forward_train_nhwc, "skd_abn_forward_train_nhwc", _rows, _C, ACT_RELU, _C == 8, ws=True, fused=_f)
        add("abn_backward_nhwc-" + _u, abn_backward_nhwc, "skd_abn_backward_nhwc", _rows, _C, ws=True, fused=_f)
        add("abn_relu_backward_nhwc-" + _u, abn_relu_backward_nhwc, "skd_abn_relu_backward_nhwc", _rows, _C, _C == 4, ws=True, fused=_f)


# =====================================================================================================================
# 3. The fused training stem and the stem max-pool, channels-last (B, C, H, W).  Shapes (a): (1, 4, 9, 12) and
#    (3, 16, 1, 2) of test_maxpool3x3s2_nhwc / test_abn_relu_maxpool_stem.  Tolerances: those two tests.
# =====================================================================================================================
STEM_SHAPES = [(1, 4, 9, 12), (3, 16, 1, 2)]


def _pool_out(n):
    """MaxPool2d(3, 2, 1, ceil_mode=True) (functional._pool_out)."""
    o = -(-(n + 2 - 3) // 2) + 1
    return o - 1 if (o - 1) * 2 >= n + 1 else o


def _arg_codes(y):
    """(B, H, W, C) values -> (pooled, window code 3 * dy + dx as uint8) of the 3x3 / stride 2 / pad 1 ceil-mode pool, by torch."""
    B, H, W, C = y.shape
    p, idx = torch.nn.functional.max_pool2d(y.permute(0, 3, 1, 2), 3, 2, 1, ceil_mode=True, return_indices=True)
    OH, OW = p.shape[2:]
    oy, ox = torch.arange(OH).view(1, 1, OH, 1), torch.arange(OW).view(1, 1, 1, OW)
    code = (idx // W - (2 * oy - 1)) * 3 + (idx % W - (2 * ox - 1))
    return p.permute(0, 2, 3, 1).contiguous(), code.permute(0, 2, 3, 1).contiguous().to(torch.uint8)


def _stem_data(B, C, H, W):
    g = _gen(H * 3 + W + C)
    d = {}
    d["x"] = torch.randn(B, H, W, C, generator=g) * 2.0 + torch.randn(1, 1, 1, C, generator=g)
    d["x"][torch.rand(B, H, W, C, generator=g) < 0.05] = 0.75
    d["w"], d["b"] = torch.randn(C, generator=g), torch.randn(C, generator=g) * 0.5
    d["w"][0], d["w"][1] = 0.0, -abs(d["w"][1])
    xd = d["x"].double().reshape(-1, C)
    d["mean"], d["var"] = xd.mean(0).float(), xd.var(0, unbiased=False).float() + 0.01
    d["y"] = torch.relu((d["x"] - d["mean"]) / torch.sqrt(d["var"] + EPS) * (d["w"].abs() + EPS) + d["b"])
    d["pooled"], d["arg"] = _arg_codes(d["y"])
    OH, OW = d["arg"].shape[1:3]
    assert (OH, OW) == (_pool_out(H), _pool_out(W))
    d["gp"] = torch.randn(B, OH, OW, C, generator=g)
    d["edz"], d["eydz"] = torch.randn(C, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1
    d["OH"], d["OW"] = OH, OW
    return d


def maxpool3x3s2(lib, A, B, C, H, W):
    """Values and argmax codes bit-exact (test_maxpool3x3s2_nhwc); -inf and ties as there."""
    d = _stem_data(B, C, H, W)
    x0 = d["x"].clone()
    x0[torch.rand(x0.shape, generator=_gen(1)) < 0.3] = 1.0
    x0.view(-1)[::97] = float("-inf")
    OH, OW = d["OH"], d["OW"]
    x, y, a = A.inp("x", x0), A.out("y", (B, OH, OW, C)), A.out("arg", (B, OH, OW, C), torch.uint8)
    return (lambda: lib.skd_maxpool3x3s2_nhwc(B, C, H, W, OH, OW, P(x), P(y), P(a), None)), {"y": (y, EXACT), "arg": (a, EXACT)}


def maxpool3x3s2_backward(lib, A, B, C, H, W):
    d = _stem_data(B, C, H, W)
    OH, OW = d["OH"], d["OW"]
    gy, a, dx = A.inp("gy", d["gp"]), A.inp("arg", d["arg"]), A.out("dx", (B, H, W, C))
    call = lambda: lib.skd_maxpool3x3s2_backward_nhwc(B, C, H, W, OH, OW, P(gy), P(a), P(dx), None)
    return call, {"dx": (dx, 1e-6, float(d["gp"].abs().max()))}


def stem_forward(lib, A, B, C, H, W):
    """pooled <= 2e-5 vs the oracle; the argmax bytes may differ from the oracle's on at most 1e-3 of the positions there (two
    window positions within rounding of each other): fewer than one position at these shapes, so they are compared exactly."""
    d = _stem_data(B, C, H, W)
    OH, OW = d["OH"], d["OW"]
    x, m, v, w, b = A.inp("x", d["x"]), A.inp("mean", d["mean"]), A.inp("var", d["var"]), A.inp("weight", d["w"]), A.inp("bias", d["b"])
    p, a = A.out("pooled", (B, OH, OW, C)), A.out("arg", (B, OH, OW, C), torch.uint8)
    call = lambda: lib.skd_abn_relu_maxpool3x3s2_nhwc(B, C, H, W, OH, OW, P(x), P(m), P(v), P(w), P(b), EPS, P(p), P(a), None)
    return call, {"pooled": (p, 2e-5), "arg": (a, EXACT)}


def stem_backward_reduce(lib, A, B, C, H, W):
    d = _stem_data(B, C, H, W)
    OH, OW = d["OH"], d["OW"]
    x, gp, a = A.inp("x", d["x"]), A.inp("gpooled", d["gp"]), A.inp("arg", d["arg"])
    m, v, w, b = A.inp("mean", d["mean"]), A.inp("var", d["var"]), A.inp("weight", d["w"]), A.inp("bias", d["b"])
    e, ey, ws = A.out("edz", C), A.out("eydz", C), _nhwc_ws(lib, A, B * H * W, C)
    call = lambda: lib.skd_abn_relu_maxpool3x3s2_backward_reduce_nhwc(B, C, H, W, OH, OW, P(x), P(gp), P(a), P(m), P(v), P(w), P(b), P(e), P(ey), EPS, P(ws), None)
    # that test's floor: the mean magnitude of the un-pooled gradient (every pooled position lands on one input position)
    scale = float(d["gp"].abs().sum()) / (B * H * W * C) + 1e-12
    return call, {"edz": (e, 2e-5, scale), "eydz": (ey, 2e-5, scale)}


def stem_backward_dx(lib, A, B, C, H, W):
    d = _stem_data(B, C, H, W)
    OH, OW = d["OH"], d["OW"]
    x, gp, a = A.inp("x", d["x"]), A.inp("gpooled", d["gp"]), A.inp("arg", d["arg"])
    m, v, w, b = A.inp("mean", d["mean"]), A.inp("var", d["var"]), A.inp("weight", d["w"]), A.inp("bias", d["b"])
    e, ey, dx = A.inp("edz", d["edz"]), A.inp("eydz", d["eydz"]), A.out("dx", (B, H, W, C))
    dw, db = A.io("dweight", torch.zeros(C)), A.io("dbias", torch.zeros(C))          # accumulate = 1 onto zeros
    call = lambda: lib.skd_abn_relu_maxpool3x3s2_backward_dx_nhwc(B, C, H, W, OH, OW, P(x), P(gp), P(a), P(m), P(v), P(w), P(b), P(e), P(ey), P(dx), P(dw), P(db), EPS, 1, None)
    floor = float(d["gp"].abs().max()) * float((d["w"].abs() / (d["var"] + EPS).sqrt()).max())
    # dx: "fused stem dx vs oracle" of test_abn_relu_maxpool_stem; dweight / dbias: that test compares them with the un-fused GPU
    # sequence only, so the bound of the same sums in test_abn_nhwc_training ("relu dweight") is used
    return call, {"dx": (dx, 5e-5, floor), "dweight": (dw, 5e-5, 1e-6), "dbias": (db, 5e-5, 1e-6)}


for _s in STEM_SHAPES:
    _t = "%dx%dx%dx%d" % _s
    add("maxpool3x3s2-" + _t, maxpool3x3s2, "skd_maxpool3x3s2_nhwc", *_s)
    add("maxpool3x3s2_backward-" + _t, maxpool3x3s2_backward, "skd_maxpool3x3s2_backward_nhwc", *_s)
    add("stem_forward-" + _t, stem_forward, "skd_abn_relu_maxpool3x3s2_nhwc", *_s)
    add("stem_backward_reduce-" + _t, stem_backward_reduce, "skd_abn_relu_maxpool3x3s2_backward_reduce_nhwc", *_s, ws=True, bit=True)
    add("stem_backward_dx-" + _t, stem_backward_dx, "skd_abn_relu_maxpool3x3s2_backward_dx_nhwc", *_s)


# =====================================================================================================================
# 4. Classifier head (test_head1x1): (B, HW, K, C) = (1, 7, 128, 3), and (3, 100, 128, 20) for more than one row block.
# =====================================================================================================================
def head_forward(lib, A, B, HW, K, C):
    g = _gen(B * HW + K + C)
    M = B * HW
    x, w, b = A.inp("x", torch.randn(M, K, generator=g)), A.inp("w", torch.randn(C, K, generator=g) / K ** 0.5), A.inp("bias", torch.randn(C, generator=g))
    o = A.out("logits", (B, C, HW))
    return (lambda: lib.skd_head1x1_forward_nhwc(B, HW, K, C, P(x), P(w), P(b), P(o), None)), {"logits": (o, 2e-5)}


def head_backward(lib, A, B, HW, K, C):
    """dW / db are written in a fixed order: bit-reproducible (test_head1x1)."""
    g = _gen(B * HW + K + C)
    M = B * HW
    x, w = A.inp("x", torch.randn(M, K, generator=g)), A.inp("w", torch.randn(C, K, generator=g) / K ** 0.5)
    go = A.inp("gout", torch.randn(B, C, HW, generator=g))
    gx, gw, gb = A.out("gx", (M, K)), A.out("gw", (C, K)), A.out("gb", C)
    ws = A.ws("workspace", max(1, lib.skd_head1x1_backward_workspace_floats(B, HW, K, C)))
    call = lambda: lib.skd_head1x1_backward_nhwc(B, HW, K, C, P(x), P(w), P(go), P(gx), P(gw), P(gb), P(ws), None)
    return call, {"gx": (gx, 2e-5), "gw": (gw, 3e-5, float(M ** 0.5)), "gb": (gb, 3e-5, float(M ** 0.5))}


add("head1x1_forward-2x50x1024x11", head_forward, "skd_head1x1_forward_nhwc", 2, 50, 1024, 11)      # the widest K the forward takes
for _s in ((1, 7, 128, 3), (3, 100, 128, 20)):
    add("head1x1_forward-%dx%dx%dx%d" % _s, head_forward, "skd_head1x1_forward_nhwc", *_s)
    add("head1x1_backward-%dx%dx%dx%d" % _s, head_backward, "skd_head1x1_backward_nhwc", *_s, ws=True, bit=True)


# =====================================================================================================================
# 5. Losses: pixel-wise, CE with deep supervision, spectral norm, the deterministic sum, the evaluation tail.
# =====================================================================================================================
def pixelwise(lib, A, N, C, HW):
    """test_pixelwise: loss 1e-5, gradient 2e-5; the loss is bit-reproducible."""
    g = _gen(C)
    s, t = A.inp("logits_s", torch.randn(N, C, HW, generator=g) * 4), A.inp("logits_t", torch.randn(N, C, HW, generator=g) * 4)
    loss, grad = A.out("loss", 1), A.out("grad", (N, C, HW))
    ws = A.ws("workspace", max(1, lib.skd_pixelwise_workspace_floats(N, HW)))
    return (lambda: lib.skd_pixelwise_loss(N, C, HW, P(s), P(t), P(loss), P(grad), P(ws), None)), {"loss": (loss, 1e-5), "grad": (grad, 2e-5)}


add("pixelwise-1x1x1", pixelwise, "skd_pixelwise_loss", 1, 1, 1, ws=True, bit=True)
add("pixelwise-3x11x2806", pixelwise, "skd_pixelwise_loss", 3, 11, 46 * 61, ws=True, bit=True)
add("pixelwise-generic-2x40x100", pixelwise, "skd_pixelwise_loss", 2, 40, 100, ws=True, bit=True)      # C > 32: pixelwise_generic_kernel, csrc/pixelwise.hip:124


def ce_dsn(lib, A, B, C, h, w, H, W):
    """test_ce_dsn: loss 1e-5, gradients 5e-5; the workspace has exactly the queried size (no max(1, .) there)."""
    g = _gen(H + C)
    lm, ld = A.inp("logits_main", torch.randn(B, C, h, w, generator=g) * 3), A.inp("logits_dsn", torch.randn(B, C, h, w, generator=g) * 3)
    y = torch.randint(0, C, (B, H, W), generator=g)
    y[0, : max(1, H // 16)] = 255
    y[-1, -1, -1] = 255
    yt, loss, gm, gd = A.inp("target", y), A.out("loss", 1), A.out("grad_main", (B, C, h, w)), A.out("grad_dsn", (B, C, h, w))
    ws = A.ws("workspace", lib.skd_ce_dsn_workspace_floats(B, C, h, w, H, W))
    call = lambda: lib.skd_ce_dsn_forward(B, C, h, w, H, W, P(lm), P(ld), P(yt), 255, 0.4, P(loss), P(gm), P(gd), P(ws), None)
    return call, {"loss": (loss, 1e-5), "grad_main": (gm, 5e-5), "grad_dsn": (gd, 5e-5)}


# the class-count templates of ce_cmax(), csrc/ce_dsn.hip:462-467: C = 3 -> 12, 19 -> 19, 21 -> 24, 40 -> 64
for _s in ((1, 3, 1, 1, 4, 4), (2, 21, 17, 9, 100, 3), (2, 19, 9, 9, 65, 65), (1, 40, 5, 7, 5, 7)):
    add("ce_dsn-%dx%dx%dx%dx%dx%d" % _s, ce_dsn, "skd_ce_dsn_forward", *_s, ws=True, bit=True)


def _sn_data(h, w, g):
    W = torch.randn(h, w, generator=g) * 0.05
    u, v = torch.randn(h, generator=g), torch.randn(w, generator=g)
    return W, u / u.norm(), v / v.norm(), torch.randn(h, w, generator=g)


def spectral_forward(lib, A, h, w):
    """test_spectral_norm: 2e-5; u and v persist (in / out)."""
    W0, u0, v0, _ = _sn_data(h, w, _gen(h))
    W, u, v, s, o = A.inp("w_bar", W0), A.io("u", u0), A.io("v", v0), A.out("sigma", 1), A.out("w", (h, w))
    ws = A.ws("workspace", max(1, lib.skd_spectral_workspace_floats(h, w)))
    call = lambda: lib.skd_spectral_norm_forward(h, w, P(W), P(u), P(v), P(s), P(o), P(ws), None)
    return call, {"u": (u, 2e-5), "v": (v, 2e-5), "sigma": (s, 2e-5), "w": (o, 2e-5)}


def spectral_backward(lib, A, h, w):
    """test_spectral_norm: 5e-5."""
    W0, u0, v0, gw0 = _sn_data(h, w, _gen(h))
    sig = (u0.double() @ W0.double() @ v0.double()).abs().float().reshape(1) + 0.1
    W, u, v, s, gw, o = A.inp("w_bar", W0), A.inp("u", u0), A.inp("v", v0), A.inp("sigma", sig), A.inp("grad_w", gw0), A.out("grad_w_bar", (h, w))
    ws = A.ws("workspace", max(1, lib.skd_spectral_workspace_floats(h, w)))
    call = lambda: lib.skd_spectral_norm_backward(h, w, P(W), P(u), P(v), P(s), P(gw), P(o), P(ws), None)
    return call, {"grad_w_bar": (o, 5e-5)}


def spectral_multi(lib, A, shapes, backward):
    """All layers in one call: host arrays of device pointers, each pointing at its own guarded buffer; per layer the arithmetic of
    the single-layer entries (test_spectral_norm_multi_is_bit_identical...), hence their tolerances."""
    L = len(shapes)
    g = _gen(L * 100 + shapes[0][0])
    data = [_sn_data(h, w, g) for h, w in shapes]
    Ws = [A.inp("w_bar%d" % k, d[0]) for k, d in enumerate(data)]
    mk = A.inp if backward else A.io
    us, vs = [mk("u%d" % k, d[1]) for k, d in enumerate(data)], [mk("v%d" % k, d[2]) for k, d in enumerate(data)]
    hs, ws_ = _ints([h for h, _ in shapes]), _ints([w for _, w in shapes])
    work = A.ws("workspace", sum(max(1, lib.skd_spectral_workspace_floats(h, w)) for h, w in shapes))
    outs = {}
    if backward:
        sig = [A.inp("sigma%d" % k, (d[1].double() @ d[0].double() @ d[2].double()).abs().float().reshape(1) + 0.1) for k, d in enumerate(data)]
        gws = [A.inp("grad_w%d" % k, d[3]) for k, d in enumerate(data)]
        gb = [A.out("grad_w_bar%d" % k, s) for k, s in enumerate(shapes)]
        keep = (hs, ws_, _ptrs(Ws), _ptrs(us), _ptrs(vs), _ptrs(sig), _ptrs(gws), _ptrs(gb))
        call = lambda: lib.skd_spectral_norm_backward_multi(L, *keep, P(work), None)
        for k in range(L):
            outs["grad_w_bar%d" % k] = (gb[k], 5e-5)
    else:
        sig, wo = [A.out("sigma%d" % k, 1) for k in range(L)], [A.out("w%d" % k, s) for k, s in enumerate(shapes)]
        keep = (hs, ws_, _ptrs(Ws), _ptrs(us), _ptrs(vs), _ptrs(sig), _ptrs(wo))
        call = lambda: lib.skd_spectral_norm_forward_multi(L, *keep, P(work), None)
        for k in range(L):
            outs.update({"u%d" % k: (us[k], 2e-5), "v%d" % k: (vs[k], 2e-5), "sigma%d" % k: (sig[k], 2e-5), "w%d" % k: (wo[k], 2e-5)})
    return call, outs


for _s in ((7, 5), (1, 1), (33, 1000)):
    add("spectral_forward-%dx%d" % _s, spectral_forward, "skd_spectral_norm_forward", *_s, ws=True)
    add("spectral_backward-%dx%d" % _s, spectral_backward, "skd_spectral_norm_backward", *_s, ws=True)
for _k, _shapes in enumerate(([(7, 5), (1, 1)], [(33, 1000), (64, 304), (5, 3)])):
    add("spectral_forward_multi-%d" % _k, spectral_multi, "skd_spectral_norm_forward_multi", _shapes, False, ws=True)
    add("spectral_backward_multi-%d" % _k, spectral_multi, "skd_spectral_norm_backward_multi", _shapes, True, ws=True)


def sum_f32(lib, A, n):
    """test_sum_f32: |err| <= 1e-6 max(1, sum |x|); a 2048-float workspace as there; deterministic two-stage sum."""
    x0 = torch.randn(n, generator=_gen(n))
    x, o, ws = A.inp("x", x0), A.out("out", 1), A.ws("workspace", 2048)
    return (lambda: lib.skd_sum_f32(n, P(x), P(o), 0.5, P(ws), None)), {"out": (o, 1e-6, max(1.0, float(x0.double().abs().sum())))}


add("sum_f32-1", sum_f32, "skd_sum_f32", 1, ws=True, bit=True)
add("sum_f32-4097", sum_f32, "skd_sum_f32", 4097, ws=True, bit=True)


def seg_confusion(lib, A, B, C, h, w, H, W):
    """test_seg_confusion_bit_exact: predictions and the (accumulated) int64 counts bit-exact."""
    g = _gen(H + W + C)
    lg = torch.randn(B, C, h, w, generator=g) * 4
    lg[0, :, 0, 0] = 1.5
    y = torch.randint(0, C, (B, H, W), generator=g)
    y[0, : max(1, H // 16)] = 255
    l, t, p, c = A.inp("logits", lg), A.inp("target", y), A.out("pred", (B, H, W), torch.uint8), A.io("confusion", torch.ones(C, C, dtype=torch.int64))
    return (lambda: lib.skd_seg_confusion(B, C, h, w, H, W, P(l), P(t), 255, P(p), P(c), None)), {"pred": (p, EXACT), "confusion": (c, EXACT)}


add("seg_confusion-1x3x1x1x4x4", seg_confusion, "skd_seg_confusion", 1, 3, 1, 1, 4, 4)
add("seg_confusion-3x64x5x7x33x20", seg_confusion, "skd_seg_confusion", 3, 64, 5, 7, 33, 20)


# =====================================================================================================================
# 6. Pyramid pooling (test_ppm, test_ppm_fold).  Shapes (a): (1, 2, 7, 9, 2) (planar only: C % 4) and (2, 8, 33, 47, 4).
# =====================================================================================================================
PPM_SIZES = (1, 2, 3, 6)


def _split_levels(flat, B, C, sizes, to_nhwc):
    out, off = [], 0
    for s in sizes:
        n = B * C * s * s
        t = flat[off:off + n].view(B, C, s, s)
        out.append(t.permute(0, 2, 3, 1).contiguous().reshape(-1) if to_nhwc else t)
        off += n
    return out


def ppm_planar(lib, A, B, C, H, W, Cout, which):
    """test_ppm: pooled / pool backward / concat 1e-5, concat backward 2e-5."""
    arr = _ints(PPM_SIZES)
    g = _gen(C + H)
    x0 = torch.randn(B, C, H, W, generator=g)
    total = lib.skd_ppm_pooled_floats(B * C, 4, arr)
    assert total == B * C * 50
    if which == "pool":
        x, p = A.inp("x", x0), A.out("pooled", total)
        return (lambda: lib.skd_ppm_pool(B * C, H, W, 4, arr, P(x), P(p), None)), {"pooled": (p, 1e-5)}
    if which == "pool_backward":
        gp, dx = A.inp("gpooled", torch.randn(total, generator=g)), A.out("dx", (B, C, H, W))
        return (lambda: lib.skd_ppm_pool_backward(B * C, H, W, 4, arr, P(gp), P(dx), None)), {"dx": (dx, 1e-5)}
    if which == "concat":
        pri = [A.inp("prior%d" % s, torch.randn(B, Cout, s, s, generator=g)) for s in PPM_SIZES]
        x, cat = A.inp("x", x0), A.out("cat", (B, 4 * Cout + C, H, W))
        pp = _ptrs(pri)
        return (lambda: lib.skd_ppm_concat(B, Cout, C, H, W, 4, arr, pp, P(x), P(cat), None)), {"cat": (cat, 1e-5)}
    gc = A.inp("gcat", torch.randn(B, 4 * Cout + C, H, W, generator=g))
    gr = [A.out("gprior%d" % s, (B, Cout, s, s)) for s in PPM_SIZES]
    pp = _ptrs(gr)
    return (lambda: lib.skd_ppm_concat_backward(B, Cout, C, H, W, 4, arr, P(gc), pp, None)), {"gprior%d" % s: (t, 2e-5) for s, t in zip(PPM_SIZES, gr)}


def ppm_nhwc(lib, A, B, C, H, W, Cout, which):
    """The channels-last forms at the planar tolerances (test_ppm compares them with the planar oracle results at those)."""
    arr = _ints(PPM_SIZES)
    g = _gen(C + H)
    x0 = torch.randn(B, H, W, C, generator=g)
    total = B * C * 50
    nws = max(1, lib.skd_ppm_nhwc_workspace_floats(B, C, Cout, H, W, 4, arr))
    if which == "pool":
        x, p, ws = A.inp("x", x0), A.out("pooled", total, row=C), A.ws("workspace", nws)
        return (lambda: lib.skd_ppm_pool_nhwc(B, C, H, W, 4, arr, P(x), P(p), P(ws), None)), {"pooled": (p, 1e-5)}
    if which == "pool_backward":
        gp, dx = A.inp("gpooled", torch.randn(total, generator=g), row=C), A.out("dx", (B, H, W, C))
        return (lambda: lib.skd_ppm_pool_backward_nhwc(B, C, H, W, 4, arr, P(gp), P(dx), None)), {"dx": (dx, 1e-5)}
    if which == "concat":
        pri = [A.inp("prior%d" % s, torch.randn(B, s, s, Cout, generator=g)) for s in PPM_SIZES]
        x, cat = A.inp("x", x0), A.out("cat", (B, H, W, 4 * Cout + C))
        pp = _ptrs(pri)
        return (lambda: lib.skd_ppm_concat_nhwc(B, Cout, C, H, W, 4, arr, pp, P(x), P(cat), None)), {"cat": (cat, 1e-5)}
    gc = A.inp("gcat", torch.randn(B, H, W, 4 * Cout + C, generator=g))
    gr = [A.out("gprior%d" % s, (B, s, s, Cout)) for s in PPM_SIZES]
    gf, ws = A.out("gfeat", (B, H, W, C)), A.ws("workspace", nws)
    pp = _ptrs(gr)
    outs = {"gprior%d" % s: (t, 2e-5) for s, t in zip(PPM_SIZES, gr)}
    outs["gfeat"] = (gf, EXACT)                           # the gradient of the feature map is its slice of gcat
    return (lambda: lib.skd_ppm_concat_backward_nhwc(B, Cout, C, H, W, 4, arr, P(gc), pp, P(gf), P(ws), None)), outs


for _w in ("pool", "pool_backward", "concat", "concat_backward"):
    for _s in ((1, 2, 7, 9, 2), (2, 8, 33, 47, 4)):
        add("ppm_%s-%dx%dx%dx%dx%d" % ((_w,) + _s), ppm_planar, "skd_ppm_" + _w, *_s, _w)
    for _s in ((1, 4, 7, 9, 4), (2, 8, 33, 47, 4)):
        add("ppm_%s_nhwc-%dx%dx%dx%dx%d" % ((_w,) + _s), ppm_nhwc, "skd_ppm_%s_nhwc" % _w, *_s, _w, ws=_w in ("pool", "concat_backward"))


def ppm_fold(lib, A, B, Cout, H, W, sizes, backward):
    """test_ppm_fold: forward 2e-5 (out is accumulated into), backward 2e-5 with floor max |gout|; the backward's workspace at exactly
    the queried size, as there."""
    L = len(sizes)
    arr = _ints(sizes)
    LD = 9 * Cout
    g = _gen(Cout + H + W)
    zs = [torch.randn(B * s * s, LD, generator=g) for s in sizes]
    base = torch.randn(B, H, W, Cout, generator=g)
    if not backward:
        z, out = [A.inp("z%d" % s, t) for s, t in zip(sizes, zs)], A.io("out", base)
        pp = _ptrs(z)
        return (lambda: lib.skd_ppm_fold_nhwc(B, Cout, H, W, L, arr, pp, LD, P(out), None)), {"out": (out, 2e-5)}
    gout0 = torch.randn(B, H, W, Cout, generator=g)
    gout, gz = A.inp("gout", gout0), [A.out("gz%d" % s, t.shape) for s, t in zip(sizes, zs)]
    ws = A.ws("workspace", lib.skd_ppm_fold_nhwc_workspace_floats(B, Cout, H, W, L, arr))
    pp = _ptrs(gz)
    call = lambda: lib.skd_ppm_fold_backward_nhwc(B, Cout, H, W, L, arr, P(gout), pp, LD, P(ws), None)
    return call, {"gz%d" % s: (t, 2e-5, float(gout0.abs().max())) for s, t in zip(sizes, gz)}


# (1, 4, 1, 5, (1,)): one level, one row; (3, 4, 7, 9): all four levels, i.e. the two launches over {1, 2, 3} and {6} of csrc/ppm.hip:903-911;
# (1, 16, 3, 2, (1, 2)): fewer columns than levels' bins
for _s in ((1, 4, 1, 5, (1,)), (3, 4, 7, 9, (1, 2, 3, 6)), (1, 16, 3, 2, (1, 2))):
    _t = "%dx%dx%dx%d-L%d" % (_s[:4] + (len(_s[4]),))
    add("ppm_fold-" + _t, ppm_fold, "skd_ppm_fold_nhwc", *_s, False)
    add("ppm_fold_backward-" + _t, ppm_fold, "skd_ppm_fold_backward_nhwc", *_s, True, ws=True)


# =====================================================================================================================
# 7. Pair-wise distillation: max-pool / un-pool, normalise, Gram + loss, backward, the one-launch small-graph entry.
#    Tolerances: test_maxpool_argmax_bit_exact, test_maxpool_argmax_channels_last_bit_exact, test_pairwise_stages,
#    test_pairwise_small_m_fused.
# =====================================================================================================================
def _pool_index(x, kh, kw):
    """(planes, H, W) -> flat argmax indices (planes, OH * OW) int32 of the ceil-mode kh x kw pool, by torch."""
    _, idx = torch.nn.functional.max_pool2d(x[None], (kh, kw), (kh, kw), 0, ceil_mode=True, return_indices=True)
    return idx[0].reshape(x.shape[0], -1).int().contiguous()


def maxpool_argmax(lib, A, planes, H, W, kh, kw):
    g = _gen(H * W)
    x0 = torch.randn(planes, H, W, generator=g)
    x0[0] = torch.randint(0, 3, (H, W), generator=g).float()           # many ties: the first maximum wins
    OH, OW = -(-H // kh), -(-W // kw)
    x, p, i = A.inp("x", x0), A.out("pooled", (planes, OH * OW)), A.out("index", (planes, OH * OW), torch.int32)
    return (lambda: lib.skd_maxpool_argmax(planes, H, W, kh, kw, P(x), P(p), P(i), None)), {"pooled": (p, EXACT), "index": (i, EXACT)}


def maxunpool_scatter(lib, A, planes, H, W, kh, kw):
    g = _gen(H * W)
    OH, OW = -(-H // kh), -(-W // kw)
    ldp = OH * OW + 5                                                  # strided rows, as in the value test
    idx = _pool_index(torch.randn(planes, H, W, generator=g), kh, kw)
    dp, i, dx = A.inp("dpooled", torch.randn(planes, ldp, generator=g)), A.inp("index", idx), A.out("dx", (planes, H, W))
    return (lambda: lib.skd_maxunpool_scatter(planes, H, W, kh, kw, P(dp), ldp, P(i), P(dx), None)), {"dx": (dx, EXACT)}


def maxpool_argmax_nhwc(lib, A, B, C, H, W, kh, kw):
    g = _gen(H * W + C)
    x0 = torch.randn(B, H, W, C, generator=g)
    x0[0, :, :, 0] = torch.randint(0, 3, (H, W), generator=g).float()
    x0[0, :, :, 1] = 1.0
    x0[-1, :, :, 3] = float("-inf")
    M = -(-H // kh) * -(-W // kw)
    x, p, i = A.inp("x", x0), A.out("pooled", (B * C, M)), A.out("index", (B * C, M), torch.int32)
    return (lambda: lib.skd_maxpool_argmax_nhwc(B, C, H, W, kh, kw, P(x), P(p), P(i), None)), {"pooled": (p, EXACT), "index": (i, EXACT)}


def maxunpool_scatter_nhwc(lib, A, B, C, H, W, kh, kw):
    g = _gen(H * W + C)
    M = -(-H // kh) * -(-W // kw)
    idx = _pool_index(torch.randn(B * C, H, W, generator=g), kh, kw)
    dp, i, dx = A.inp("dpooled", torch.randn(B * C, M + 5, generator=g)), A.inp("index", idx), A.out("dx", (B, H, W, C))
    return (lambda: lib.skd_maxunpool_scatter_nhwc(B, C, H, W, kh, kw, P(dp), M + 5, P(i), P(dx), None)), {"dx": (dx, EXACT)}


# planar: W <= kPoolMaxW = 1024 -> maxpool_band_kernel, else maxpool_cell_kernel (csrc/pairwise.hip:855)
add("maxpool_argmax-band-2x7x130-3x64", maxpool_argmax, "skd_maxpool_argmax", 2, 7, 130, 3, 64)
add("maxpool_argmax-band-5x46x61-23x30", maxpool_argmax, "skd_maxpool_argmax", 5, 46, 61, 23, 30)
add("maxpool_argmax-cell-1x3x1500-2x7", maxpool_argmax, "skd_maxpool_argmax", 1, 3, 1500, 2, 7)
add("maxunpool_scatter-2x7x130-3x64", maxunpool_scatter, "skd_maxunpool_scatter", 2, 7, 130, 3, 64)
add("maxunpool_scatter-1x3x1500-2x7", maxunpool_scatter, "skd_maxunpool_scatter", 1, 3, 1500, 2, 7)
# channels-last: window of >= 64 positions -> maxpool_window_nhwc_kernel, else maxpool_cell_nhwc_kernel (csrc/pairwise.hip:905)
add("maxpool_argmax_nhwc-window-1x8x7x130-3x64", maxpool_argmax_nhwc, "skd_maxpool_argmax_nhwc", 1, 8, 7, 130, 3, 64)
add("maxpool_argmax_nhwc-window-3x20x46x61-23x30", maxpool_argmax_nhwc, "skd_maxpool_argmax_nhwc", 3, 20, 46, 61, 23, 30)
add("maxpool_argmax_nhwc-cell-1x16x65x65-4x4", maxpool_argmax_nhwc, "skd_maxpool_argmax_nhwc", 1, 16, 65, 65, 4, 4)
add("maxunpool_scatter_nhwc-1x8x7x130-3x64", maxunpool_scatter_nhwc, "skd_maxunpool_scatter_nhwc", 1, 8, 7, 130, 3, 64)
add("maxunpool_scatter_nhwc-1x16x65x65-4x4", maxunpool_scatter_nhwc, "skd_maxunpool_scatter_nhwc", 1, 16, 65, 65, 4, 4)


def _pair_data(B, Cs, Ct, M, ldm):
    """Pooled features and, computed in fp32 by torch so that both libraries read the same bits, everything a later stage reads:
    the zero-padded normalised panels, the norms, G = A_T - A_S."""
    g = _gen(M + Cs)
    d = {"ps": torch.randn(B, Cs, M, generator=g), "pt": torch.randn(B, Ct, M, generator=g)}
    d["norm"] = (d["ps"] ** 2).sum(1).sqrt() + 1e-8
    pad = lambda t: torch.nn.functional.pad(t, (0, ldm - M)).contiguous()
    d["fs"] = pad(d["ps"] / d["norm"][:, None])
    d["ft"] = pad(d["pt"] / ((d["pt"] ** 2).sum(1, keepdim=True).sqrt() + 1e-8))
    d["G"] = (torch.einsum("icm,icn->imn", d["ft"], d["ft"]) - torch.einsum("icm,icn->imn", d["fs"], d["fs"])).contiguous()
    return d


def l2_normalise(lib, A, B, C, M, transposed):
    """Padding columns are written (zeros) by both libraries: the whole panels are compared (1e-6)."""
    ldm = lib.skd_pairwise_ldm(M)
    ldc = -(-C // 128) * 128
    p, f = A.inp("pooled", _pair_data(B, C, 3, M, ldm)["ps"]), A.out("fhat", (B, C, ldm))
    if not transposed:
        return (lambda: lib.skd_channel_l2_normalise(B, C, M, P(p), P(f), ldm, None, 0, None, None)), {"fhat": (f, 1e-6)}
    ft, n = A.out("fhat_t", (B, ldm, ldc)), A.out("norm", (B, M))
    call = lambda: lib.skd_channel_l2_normalise(B, C, M, P(p), P(f), ldm, P(ft), ldc, P(n), None)
    return call, {"fhat": (f, 1e-6), "fhat_t": (ft, 1e-6), "norm": (n, 1e-6)}


def gram_loss(lib, A, B, Cs, Ct, M):
    ldm = lib.skd_pairwise_ldm(M)
    d = _pair_data(B, Cs, Ct, M, ldm)
    fs, ft, G, loss = A.inp("fhat_s", d["fs"]), A.inp("fhat_t", d["ft"]), A.out("G", (B, ldm, ldm)), A.out("loss", 1)
    ws = A.ws("workspace", max(1, lib.skd_pairwise_workspace_floats(B, M)))
    call = lambda: lib.skd_pairwise_gram_loss(B, Cs, Ct, M, ldm, P(fs), P(ft), P(G), P(loss), P(ws), None)
    # G = A_T - A_S: a difference of Gram entries of magnitude <= 1; every padding entry is an exact zero
    return call, {"G": (lambda: G[..., :M], 2e-5, 1.0), "G_padding": (lambda: G[..., M:], EXACT), "loss": (loss, 1e-5, 1e-6)}


def pairwise_backward(lib, A, B, Cs, M):
    ldm = lib.skd_pairwise_ldm(M)
    d = _pair_data(B, Cs, 3, M, ldm)
    fs, G, n, gl = A.inp("fhat_s", d["fs"]), A.inp("G", d["G"]), A.inp("norm", d["norm"]), A.inp("grad_loss", torch.tensor([0.5]))
    dp = A.out("dpooled", (B, Cs, ldm))
    ws = A.ws("workspace", max(1, lib.skd_pairwise_backward_workspace_floats(B, Cs, M)))
    call = lambda: lib.skd_pairwise_backward(B, Cs, M, ldm, P(fs), P(G), P(n), P(gl), P(dp), P(ws), None)
    return call, {"dpooled": (lambda: dp[..., :M], 5e-5, 1.0 if M == 1 else 0.0), "dpooled_padding": (lambda: dp[..., M:], EXACT)}


def pairwise_small(lib, A, B, Cs, Ct, M):
    g = _gen(M * 7 + Cs)
    ps, pt = A.inp("pooled_s", torch.randn(B, Cs, M, generator=g)), A.inp("pooled_t", torch.randn(B, Ct, M, generator=g))
    loss, dp, ws = A.out("loss", 1), A.out("dpooled", (B, Cs, M)), A.ws("workspace", B)
    call = lambda: lib.skd_pairwise_small(B, Cs, Ct, M, P(ps), P(pt), P(loss), P(dp), P(ws), None)
    return call, {"loss": (loss, 1e-5, 1e-6), "dpooled": (dp, 5e-5, 1.0 if M == 1 else 1e-6)}


# M = 1: pure padding; M = 65: the first graph past skd_pairwise_small (M > kSmallM = 64: the MFMA path); M = 129: two tiles
for _B, _Cs, _Ct, _M in ((1, 5, 3, 1), (2, 16, 40, 65), (2, 12, 20, 129)):
    _t = "%dx%dx%d" % (_B, _Cs, _M)
    add("l2_normalise-student-" + _t, l2_normalise, "skd_channel_l2_normalise", _B, _Cs, _M, True)
    add("l2_normalise-teacher-%dx%dx%d" % (_B, _Ct, _M), l2_normalise, "skd_channel_l2_normalise", _B, _Ct, _M, False)
    # fewer than 1024 tiles: gram_loss_kernel<64> (csrc/pairwise.hip:982); fewer than 8 * 512 units: pairwise_bwd_kernel<64> (:1001)
    add("gram_loss-64-" + _t, gram_loss, "skd_pairwise_gram_loss", _B, _Cs, _Ct, _M, ws=True)
    add("pairwise_backward-64-" + _t, pairwise_backward, "skd_pairwise_backward", _B, _Cs, _M, ws=True, bit=True)
# 1024 images of one tile each: ntri * B = 1024 -> gram_loss_kernel<128> (csrc/pairwise.hip:982), the smallest such problem (G: 64 MiB)
add("gram_loss-128-1024x5x65", gram_loss, "skd_pairwise_gram_loss", 1024, 5, 3, 65, ws=True)
add("pairwise_small-1x5x1", pairwise_small, "skd_pairwise_small", 1, 5, 3, 1, ws=True, bit=True)
add("pairwise_small-2x130x25", pairwise_small, "skd_pairwise_small", 2, 130, 70, 25, ws=True, bit=True)
add("pairwise_small-3x128x64", pairwise_small, "skd_pairwise_small", 3, 128, 512, 64, ws=True, bit=True)   # M = kSmallM, the largest it takes


def pairwise_named(lib, A, B, Cs, Ct, M):
    """pairwise_bwd_kernel<128> with several images and two channel tiles (b = t / tiles_per_image and tc = rem / ntm both non-zero):
    the whole staged chain on one set of guarded buffers.  ldm = 1152, 36 K-tiles, 9 * 2 * 7 * 36 = 4536 units >= 8 * 512, hence
    TI = 128 and 512 workgroups of 8 or 9 units: every output tile is shared by four or five of them.  Expectation: float64 einsum and
    autograd of the reference formula (utils.py:170-183), as test_pairwise_stages does; its tolerances."""
    ldm = lib.skd_pairwise_ldm(M)
    ldc = -(-Cs // 128) * 128
    assert ldm == 1152
    nws = lib.skd_pairwise_backward_workspace_floats(B, Cs, M)
    assert nws == 7 * 1152 * 256 + 512 * 2 * 128 * 128, nws                # TI = 128: one round of 512 workgroups, two slots each
    g = _gen(M + Cs)
    ps0, pt0 = torch.randn(B, Cs, M, generator=g), torch.randn(B, Ct, M, generator=g)
    ps, pt = A.inp("pooled_s", ps0), A.inp("pooled_t", pt0)
    fs, ft = A.out("fhat_s", (B, Cs, ldm)), A.out("fhat_t", (B, Ct, ldm))
    fst, nrm = A.out("fhat_s_t", (B, ldm, ldc)), A.out("norm", (B, M))
    G, loss, dp = A.out("G", (B, ldm, ldm)), A.out("loss", 1), A.out("dpooled", (B, Cs, ldm))
    gl = A.inp("grad_loss", torch.tensor([0.5]))
    ws, bws = A.ws("gram workspace", max(1, lib.skd_pairwise_workspace_floats(B, M))), A.ws("backward workspace", nws)

    def call():
        return int(lib.skd_channel_l2_normalise(B, Cs, M, P(ps), P(fs), ldm, P(fst), ldc, P(nrm), None) == 1
                   and lib.skd_channel_l2_normalise(B, Ct, M, P(pt), P(ft), ldm, None, 0, None, None) == 1
                   and lib.skd_pairwise_gram_loss(B, Cs, Ct, M, ldm, P(fs), P(ft), P(G), P(loss), P(ws), None) == 1
                   and lib.skd_pairwise_backward(B, Cs, M, ldm, P(fs), P(G), P(nrm), P(gl), P(dp), P(bws), None) == 1)

    x = ps0.double().requires_grad_(True)
    fh = x / ((x ** 2).sum(1, keepdim=True).sqrt() + 1e-8).detach()
    th = pt0.double() / ((pt0.double() ** 2).sum(1, keepdim=True).sqrt() + 1e-8)
    Gd = torch.einsum("icm,icn->imn", th, th) - torch.einsum("icm,icn->imn", fh, fh)
    L = (Gd ** 2).sum() / M ** 2 / B
    L.backward()
    Gpad = torch.nn.functional.pad(Gd.detach(), (0, 0, 0, ldm - M))    # the padding ROWS are zeros too, as in test_pairwise_stages
    want = {"G": Gpad, "G_padding": torch.zeros(B, ldm, ldm - M), "loss": L.detach().reshape(1), "dpooled": 0.5 * x.grad,
            "dpooled_padding": torch.zeros(B, Cs, ldm - M)}
    outs = {"G": (lambda: G[..., :M], 2e-5, 1.0), "G_padding": (lambda: G[..., M:], EXACT), "loss": (loss, 1e-5, 1e-6),
            "dpooled": (lambda: dp[..., :M], 5e-5, 1e-6), "dpooled_padding": (lambda: dp[..., M:], EXACT)}
    return call, outs, want


add("pairwise_backward-128-7x256x1025", pairwise_named, ("skd_channel_l2_normalise", "skd_pairwise_gram_loss", "skd_pairwise_backward"),
    7, 256, 64, 1025, ws=True, bit=True, oracle=False)


# =====================================================================================================================
# 8. The frozen teacher's GEMMs.  1x1 (+ eval ABN, residual, activation): the smallest ragged shapes of test_conv1x1_abn_gemm
#    and test_conv1x1_abn_gemm_with_bn_relu_prologue against the oracle (2e-5 / 3e-5), and -- GPU only, float64 truth, the
#    bound of tests/test_conv1x1_split_gpu.py -- one routed shape per geometry class of the split kernel.  3x3: the ragged
#    B = 2 cases of tests/test_conv3x3_split_gpu.py at the teacher's dilations 1, 2, 4 (float64 truth, that file's bound), so
#    rows -1 and H of the first and of the last image are read.
# =====================================================================================================================
def conv1x1_abn(lib, A, M, K, N, prologue):
    g = _gen(M + K + N + int(prologue))
    x0, w0 = torch.randn(M, K, generator=g) * (2 if prologue else 1), torch.randn(N, K, generator=g) / K ** 0.5
    x, w, r, o = A.inp("x", x0), A.inp("w", w0), A.inp("residual", torch.randn(M, N, generator=g)), A.out("out", (M, N))
    m, v = A.inp("mean", torch.randn(N, generator=g) * 0.3), A.inp("var", torch.rand(N, generator=g) + 0.5)
    ga, be = A.inp("weight", torch.randn(N, generator=g)), A.inp("bias", torch.randn(N, generator=g))
    if not prologue:
        call = lambda: lib.skd_conv1x1_abn_nhwc(M, K, N, P(x), P(w), P(r), P(o), P(m), P(v), P(ga), P(be), EPS, ACT_RELU, SLOPE, None)
        return call, {"out": (o, 2e-5)}
    pk = A.out("ppack", (4, K))
    src = [A.inp(n, t) for n, t in (("pmean", torch.randn(K, generator=g) * 0.5), ("pvar", torch.rand(K, generator=g) + 0.5),
                                    ("pweight", torch.randn(K, generator=g)), ("pbias", torch.randn(K, generator=g) * 0.5))]

    def call():
        return int(lib.skd_abn_pack_eval_params(K, P(src[0]), P(src[1]), P(src[2]), P(src[3]), EPS, P(pk), None) == 1
                   and lib.skd_conv1x1_abn_pro_nhwc(M, K, N, P(x), P(w), P(r), P(o), P(m), P(v), P(ga), P(be), EPS, P(pk), ACT_RELU, SLOPE, None) == 1)
    return call, {"ppack": (pk, EXACT), "out": (o, 3e-5)}          # the pack: correctly rounded sqrt / divide on both sides


add("conv1x1_abn-1000x64x128", conv1x1_abn, "skd_conv1x1_abn_nhwc", 1000, 64, 128, False)
add("conv1x1_abn-129x2048x512", conv1x1_abn, "skd_conv1x1_abn_nhwc", 129, 2048, 512, False)
add("conv1x1_abn_pro-1000x64x128", conv1x1_abn, ("skd_abn_pack_eval_params", "skd_conv1x1_abn_pro_nhwc"), 1000, 64, 128, True)
add("conv1x1_abn_pro-777x96x256", conv1x1_abn, ("skd_abn_pack_eval_params", "skd_conv1x1_abn_pro_nhwc"), 777, 96, 256, True)


def conv1x1_split_class(lib, A, name):
    """A routed shape of tests/test_conv1x1_split_gpu.py (its inputs, its float64 truth, its bound min(4 x parent, 2e-6)), after
    asserting through skd_conv1x1_abn_geometry that the problem is of the class the row means."""
    import test_conv1x1_split_gpu as S
    _, K, N, act, M, cls = S.ROUTED_CASE[name]
    S.assert_geometry(lib, M, K, N, cls)
    x0, w0, bn = S.routed_inputs(name, M, K, N)
    mean, var, ga, be, eps = bn
    x, w, o = A.inp("x", x0), A.inp("w", w0), A.out("out", (M, N))
    m, v, g_, b_ = A.inp("mean", mean), A.inp("var", var), A.inp("weight", ga), A.inp("bias", be)
    call = lambda: lib.skd_conv1x1_abn_nhwc(M, K, N, P(x), P(w), None, P(o), P(m), P(v), P(g_), P(b_), eps, act, SLOPE, None)
    return call, {"out": (o, min(S.RATIO * S.PARENT_ERR[name], S.ROUTED_CAP))}, {"out": S.routed_want(x0, w0, bn, act)}


# nt = 0: every column tile of a panel in one workgroup row (ct == tiles_n); nt = 1: column chunks (ct < tiles_n) with padding workgroups
add("conv1x1_split-class-nt0-reduce-K512-N256", conv1x1_split_class, "skd_conv1x1_abn_nhwc", "reduce-K512-N256", oracle=False)
add("conv1x1_split-class-nt1-reduce-K2048-N512", conv1x1_split_class, "skd_conv1x1_abn_nhwc", "reduce-K2048-N512", oracle=False)


def conv3x3_split(lib, A, name, geometry=0):
    """``geometry`` 1 .. 3 force the kernel's tile heights (0: the library's choice); every one gives the same bits
    (test_every_geometry_gives_the_same_bits), hence the same bound."""
    import test_conv3x3_split_gpu as S
    _, B, cin, cout, H, W, d, _ = S.CASE[name]
    x0, wt0, p = S.case_inputs(name)
    x = A.inp("x", x0.permute(0, 2, 3, 1).contiguous())              # (B, H, W, Cin) memory
    wt = A.inp("weight", wt0, row=9 * cin)
    nbytes = lib.skd_conv3x3_split_pack_bytes(cin, cout)
    assert nbytes == cout * cin * 54
    pk, out = A.out("pack", nbytes, torch.uint8, row=6 * cin), A.out("out", (B * H * W, cout))
    ep = {k: A.inp(k, p[k]) for k in ("cbias", "mean", "var", "gamma", "beta")}
    sn, sc, sy, sx = wt0.stride()

    def call():
        return int(lib.skd_conv3x3_split_pack_weights(cin, cout, P(wt), sn, sc, sy, sx, P(pk), nbytes, None) == 1
                   and lib.skd_conv3x3_split_nhwc(B, H, W, cin, cout, d, P(x), P(pk), P(out), P(ep["cbias"]), P(ep["mean"]), P(ep["var"]),
                                                  P(ep["gamma"]), P(ep["beta"]), p["eps"], S.ACT[p["act"]], SLOPE, geometry, None) == 1)
    want = S.want_of(name).permute(0, 2, 3, 1).reshape(B * H * W, cout)
    return call, {"out": (out, min(S.RATIO * S.PARENT_ERR[name], S.CAP))}, {"out": want}


for _n in ("ragged-13x11-d1", "ragged-13x11-d2", "ragged-13x11-d4", "ragged-13x11-d2-bias-abn-leaky"):
    add("conv3x3_split-" + _n, conv3x3_split, ("skd_conv3x3_split_pack_weights", "skd_conv3x3_split_nhwc"), _n, oracle=False)
for _g in (1, 2, 3):
    add("conv3x3_split-ragged-13x11-d2-geometry%d" % _g, conv3x3_split, ("skd_conv3x3_split_pack_weights", "skd_conv3x3_split_nhwc"),
        "ragged-13x11-d2", _g, oracle=False)


# =====================================================================================================================
# 9. Input pipeline and the sliding-window evaluation tail (bit-exact: test_transform_bit_exact,
#    test_seg_sliding_kernel_full_size_18_tiles_vs_restatement).
# =====================================================================================================================
def cs_transform(lib, A, B, H0, W0, ch, cw, channels_last):
    """Scale 0.7 (the scaled image is smaller than the crop: bottom / right padding), 1.0 with an offset, 2.1 cropped at the far
    corner; both mirror states.  ``mean`` is a host array."""
    from structure_knowledge_distillation_amd.dataset import datasets as D
    g = _gen(H0 + W0)
    img = A.inp("images", torch.randint(0, 256, (B, H0, W0, 3), generator=g, dtype=torch.uint8), row=W0 * 3)
    lab0 = torch.randint(0, 34, (B, H0, W0), generator=g, dtype=torch.uint8)
    lab0[:, :3] = 255
    lab, lut = A.inp("labels", lab0), A.inp("lut", torch.from_numpy(D.trainid_lut()))
    r = lambda v: int(round(v))
    params = [(0.7, r(H0 * 0.7), r(W0 * 0.7), 0, 0, -1), (1.0, H0, W0, max(H0, ch) - ch, max(W0, cw) - cw, 1),
              (2.1, r(H0 * 2.1), r(W0 * 2.1), max(r(H0 * 2.1), ch) - ch, max(r(W0 * 2.1), cw) - cw, -1)][:B]
    f = A.inp("scale", torch.tensor([q[0] for q in params], dtype=torch.float64))
    ints = [A.inp(n, torch.tensor([q[k] for q in params], dtype=torch.int32)) for k, n in enumerate(("dst_h", "dst_w", "h_off", "w_off", "flip"), 1)]
    out = A.out("out_image", (B, ch, cw, 3) if channels_last else (B, 3, ch, cw), row=cw * 3 if channels_last else cw)
    ol = A.out("out_label", (B, ch, cw), torch.int64)
    mean = (ctypes.c_float * 3)(104.00698793, 116.66876762, 122.67891434)
    call = lambda: lib.skd_cs_transform(B, H0, W0, P(img), P(lab), P(lut), P(f), *[P(t) for t in ints], ch, cw, mean, 255, P(out), channels_last, P(ol), None)
    return call, {"image": (out, EXACT), "label": (ol, EXACT)}


add("cs_transform-planar-3x37x53-48x40", cs_transform, "skd_cs_transform", 3, 37, 53, 48, 40, 0)
add("cs_transform-nhwc-3x97x131-64x80", cs_transform, "skd_cs_transform", 3, 97, 131, 64, 80, 1)


def seg_sliding(lib, A, T, C, h, w, tile, H, W):
    """Target and remap given, probabilities wanted: every output of the entry, against the numpy restatement, bit for bit."""
    import numpy as np
    import sliding_ref as R
    tiles = R.tiles_of(H, W, tile)
    assert len(tiles) == T
    rng = np.random.RandomState(17 + C)
    lg0 = (rng.randn(T, C, h, w) * 16).astype(np.float32)
    tg0 = rng.randint(0, C, size=(H, W)).astype(np.int64)
    tg0[rng.rand(H, W) < 0.1] = 255
    remap0 = np.random.RandomState(3).permutation(256).astype(np.uint8)
    lg, tl = A.inp("logits", torch.from_numpy(lg0), row=w), A.inp("tiles", torch.tensor(tiles, dtype=torch.int32))
    tg, rm = A.inp("target", torch.from_numpy(tg0)), A.inp("remap", torch.from_numpy(remap0))
    pred, probs = A.out("pred", (H, W), torch.uint8), A.out("probs", (H, W, C), torch.float64)
    conf = A.io("confusion", torch.ones(C, C, dtype=torch.int64))
    call = lambda: lib.skd_seg_sliding(T, C, h, w, tile[0], tile[1], H, W, P(lg), P(tl), P(tg), 255, P(rm), P(pred), P(probs), P(conf), None)
    want_probs, want_pred = R.sliding(lg0, tiles, tile, (H, W))
    want = {"pred": torch.from_numpy(remap0[want_pred]), "probs": torch.from_numpy(want_probs),
            "confusion": torch.from_numpy(R.confusion(tg0, want_pred, C) + 1)}
    return call, {"pred": (pred, EXACT), "probs": (probs, EXACT), "confusion": (conf, EXACT)}, want


# 12 overlapping tiles of 64 x 96 over 129 x 193 (ragged last row and column of tiles); class counts 1, 17 and 32 (the kernel's bounds)
for _C in (1, 17, 32):
    add("seg_sliding-12x%dx9x13" % _C, seg_sliding, "skd_seg_sliding", 12, _C, 9, 13, (64, 96), 129, 193, oracle=False)
