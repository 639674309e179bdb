"""The bounds table of tests/bounds_cases.py on the CPU: the guard-band helper itself, the partition of the C ABI into
"has a bounds case" and "exempt by name", and every oracle-backed case against the plain-C oracle inside guard bands.

The oracle judges every kernel test and has never been bounds-checked itself; running the table against it also proves
each case's shapes, sizes and argument order before a GPU sees them."""
import ctypes
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import bounds_cases as BC  # noqa: E402

from oracle import cref  # noqa: E402
from structure_knowledge_distillation_amd import _lib  # noqa: E402

ALLOWED_EXEMPT = {
    "skd_sync_create", "skd_sync_connect", "skd_sync_destroy", "skd_sync_all_gather", "skd_sync_set_timeout",
    "skd_abn_sync_stats", "skd_abn_sync_grad_stats",
    "skd_abn_forward_train_nhwc_sync", "skd_abn_backward_nhwc_sync", "skd_abn_relu_backward_nhwc_sync",
    "skd_status_read", "skd_abn_sync_form_counts", "skd_conv1x1_abn_geometry", "skd_conv1x1_abn_tile_of",
    "skd_ppm_pooled_floats", "skd_ppm_nhwc_workspace_floats", "skd_ppm_fold_nhwc_workspace_floats",
}
ORACLE_CASES = [n for n, c in BC.CASES.items() if c.oracle]


@pytest.fixture(scope="module")
def ref():
    return cref.load(_lib.SIGNATURES)


def test_every_pointer_taking_entry_has_a_bounds_case_or_is_exempt_by_name():
    entries = set(BC.pointer_entries())
    covered = set()
    for c in BC.CASES.values():
        covered.update(c.entries)
    exempt = set(BC.EXEMPT)
    assert not covered - entries, "cases name entries that do not exist or take no pointer: %s" % sorted(covered - entries)
    assert not exempt - entries, "exempt names that do not exist or take no pointer: %s" % sorted(exempt - entries)
    assert not covered & exempt, "both covered and exempt: %s" % sorted(covered & exempt)
    assert not entries - covered - exempt, "entries with neither a bounds case nor an exemption: %s" % sorted(entries - covered - exempt)
    allowed = {n for n in ALLOWED_EXEMPT if n in entries} | {n for n in entries if n.startswith("skd_sync_")}
    assert exempt <= allowed, "exempt beyond the mailbox family and the host-only pointers: %s" % sorted(exempt - allowed)
    assert all(isinstance(r, str) and r for r in BC.EXEMPT.values())
    for c in BC.CASES.values():                       # a case judged by the oracle names only entries the oracle has
        assert not c.oracle or all(e in _lib.SIGNATURES for e in c.entries), c.name


def test_arena_layout_fill_and_alignment():
    A = BC.Arena("cpu")
    x = A.inp("x", torch.arange(6, dtype=torch.float32).view(2, 3))
    o = A.out("o", (5, 7), torch.int32)
    w = A.ws("w", 3)
    big = A.out("big", (2, 1152), row=1152)
    for t, q in zip((x, o, w, big), A.buffers):      # a guard is whole 256-byte blocks: the payload is aligned like the allocation
        assert (t.data_ptr() - q["raw"].data_ptr()) % 256 == 0 and t.data_ptr() % 16 == 0
    b = {q["name"]: q for q in A.buffers}
    assert b["x"]["guard"] == 64 * 1024 and b["big"]["guard"] == 160 * 1152 * 4 and b["big"]["guard"] % 256 == 0
    assert BC.guard_bytes(1) == 65536 and BC.guard_bytes(410) == 65792 and BC.guard_bytes(410) % 256 == 0
    assert torch.equal(x, torch.arange(6, dtype=torch.float32).view(2, 3))
    assert bool((o == -1).all()) and bool(torch.isnan(w).all()) and bool(torch.isnan(big).all())
    assert all(bool((q["raw"][:q["guard"]] == 255).all()) and bool((q["raw"][q["guard"] + q["nbytes"]:] == 255).all()) for q in A.buffers)
    A.check()
    o.zero_()
    x.add_(1.0)
    A.reset()                                         # inputs are kept, pure outputs are 0xFF again
    assert bool((o == -1).all()) and float(x[0, 0]) == 1.0
    A.check()


def test_one_launch_geometry_restatement():
    """BC.one_launch_fits against the figures the value tests state for make_fuse_geom (test_fused_abn_grid_cap_and_device_status_words:
    16 workgroups x 1024 threads x 17 rows cannot hold 33800 x 256; a whole device holds it) and the table's own shapes."""
    assert BC.one_launch_fits(33800, 256, BC.FUSE_FWD_MAX_NR, 256) and BC.one_launch_fits(33800, 256, BC.FUSE_BWD_MAX_NR, 256)
    assert not BC.one_launch_fits(33800, 256, BC.FUSE_FWD_MAX_NR, 16) and not BC.one_launch_fits(33800, 256, BC.FUSE_BWD_MAX_NR, 16)
    assert not BC.one_launch_fits(4 * 256 * 256, 64, BC.FUSE_BWD_MAX_NR, 256)          # "the last two shapes ... fall back to two launches"
    assert not BC.one_launch_fits(100, 48, BC.FUSE_FWD_MAX_NR, 256) and not BC.one_launch_fits(100, 64, BC.FUSE_FWD_MAX_NR, 3)
    for rows, C in ((35, 8), (50, 4), (3000, 256)):
        assert BC.one_launch_fits(rows, C, BC.FUSE_BWD_MAX_NR, 32)


def test_arena_reports_a_one_byte_write_before_and_behind_the_payload():
    A = BC.Arena("cpu")
    A.out("first", (4, 4))
    t = A.out("victim", (3, 5))
    A.ws("last", 9)
    n = 3 * 5 * 4
    raw = next(q for q in A.buffers if q["name"] == "victim")
    base = t.data_ptr()
    assert raw["raw"].data_ptr() + raw["guard"] == base
    ctypes.memset(base - 1, 0, 1)                     # payload - 1
    with pytest.raises(BC.GuardError) as e:
        A.check()
    msg = str(e.value)
    assert "'victim'" in msg and "front guard" in msg and "first at payload offset -1, last at -1" in msg and "'first'" not in msg and "'last'" not in msg
    ctypes.memset(base - 1, 0xFF, 1)
    A.check()
    ctypes.memset(base + n, 7, 1)                     # payload + n
    with pytest.raises(BC.GuardError) as e:
        A.check()
    msg = str(e.value)
    assert "'victim'" in msg and "back guard" in msg and "first at payload offset %d, last at %d" % (n, n) in msg and "front" not in msg
    ctypes.memset(base + n + 300, 7, 1)
    with pytest.raises(BC.GuardError) as e:
        A.check()
    assert "2 byte(s), first at payload offset %d, last at %d" % (n, n + 300) in str(e.value)


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_oracle_stays_inside_its_buffers(ref, name):
    case = BC.CASES[name]
    guarded, tols, want = BC.run_case(case, ref, BC.Arena("cpu"))
    plain, _, _ = BC.run_case(case, ref, BC.Arena("cpu", guarded=False))
    assert want is None
    for k, (g, p) in enumerate(zip(guarded, plain)):
        for out in tols:
            assert not (g[out].is_floating_point() and bool(torch.isnan(g[out]).any())), "%s, call %d: %s has NaN (an element was not written)" % (name, k + 1, out)
            assert BC.same_bits(g[out], p[out]), "%s, call %d: %s differs between the guarded and the plain run" % (name, k + 1, out)
    if case.ws:                                       # the oracle is sequential: a dirty workspace never changes its bits
        for out in tols:
            assert BC.same_bits(guarded[0][out], guarded[1][out]), "%s: %s depends on what the workspace held" % (name, out)
