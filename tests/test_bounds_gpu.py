"""-m gpu: every case of tests/bounds_cases.py against libskd_hip.so with every buffer between 0xFF guard bands, workspaces
at exactly the queried size and dirty: no guard byte may change, every output must meet the tolerance of its entry's value
test against the plain-C oracle (or the float64 / restatement expectation the case carries), the second call on the used
workspace must do so again (with the same bits where the entry is documented as bit-reproducible), and no device status
word may be raised."""
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

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    return _lib.load()


@pytest.fixture(scope="module")
def ref():
    return cref.load(_lib.SIGNATURES)


def test_arena_reports_a_write_into_a_guard_on_the_device():
    """The helper on device memory: one byte of a guard set from torch (inside the arena's own allocation; no kernel is made to
    overrun) is reported with buffer, side and offset."""
    A = BC.Arena("cuda")
    A.out("first", (4, 4))
    t = A.out("victim", (3, 5))
    A.check()
    q = next(b for b in A.buffers if b["name"] == "victim")
    assert t.is_cuda and t.data_ptr() == q["raw"].data_ptr() + q["guard"] and t.data_ptr() % 256 == 0 and bool(torch.isnan(t).all())
    q["raw"][q["guard"] + q["nbytes"] + 2] = 0
    with pytest.raises(BC.GuardError) as e:
        A.check()
    assert "'victim'" in str(e.value) and "back guard" in str(e.value) and "first at payload offset 62, last at 62" in str(e.value)
    q["raw"][q["guard"] + q["nbytes"] + 2] = 0xFF
    q["raw"][q["guard"] - 4] = 1
    with pytest.raises(BC.GuardError) as e:
        A.check()
    assert "'victim'" in str(e.value) and "front guard" in str(e.value) and "first at payload offset -4, last at -4" in str(e.value)


@pytest.mark.parametrize("name", list(BC.CASES))
def test_kernel_stays_inside_its_buffers(hip, ref, name):
    case = BC.CASES[name]
    got, tols, want = BC.run_case(case, hip, BC.Arena("cuda"))
    torch.cuda.synchronize()
    if case.oracle:
        assert want is None
        want = BC.run_case(case, ref, BC.Arena("cpu", guarded=False))[0][0]
    else:
        assert want is not None
    for k, g in enumerate(got):
        BC.compare(g, want, tols, "%s, call %d%s" % (name, k + 1, " (on the workspace the first call left)" if k else ""))
    if case.ws and case.bit:
        for out in tols:
            assert BC.same_bits(got[0][out], got[1][out]), "%s: %s is not bit-reproducible on a used workspace" % (name, out)
    assert _lib.device_status() == [0] * hip.skd_status_words()
