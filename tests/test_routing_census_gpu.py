"""-m gpu: the call census of networks/pspnet_combine.py against tests/golden/routing_census.json.  Every configuration of
tests/golden/make_golden_routing_census.py -- the student's training forward and backward under each opt-in of
route_training_convs, its frozen forward under each of fuse_for_inference, the frozen teacher under set_teacher_pieces and
route_teacher_early, patched exclusion sets, and each opt-in enabled and disabled again -- is replayed on the real library, and
the sequence of ``functional`` ops and library convolutions, with the arguments the ops see, must be the recorded one.  Call
sequences only: output bits are not compared (the kernels promise no reproducibility across processes)."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(HERE, "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)
import make_golden_routing_census as G  # noqa: E402

pytestmark = pytest.mark.gpu
_FX = {}


def _fixture():
    if not _FX:
        _FX.update(json.load(open(G.OUT)))
        assert os.path.getsize(G.OUT) <= 400 * 1024 and len(_FX["recorded_on"]) == 40 and sorted(_FX) == sorted(G.NAMES + ["recorded_on"])
    return _FX


def test_fixture_has_the_documented_counts():
    G.check_counts(_fixture())


@pytest.mark.parametrize("name", G.NAMES)
def test_call_sequence_is_the_recorded_one(name):
    want, got = _fixture()[name], G.run(name)
    moved = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not moved, "call %d of %r is %s, recorded %s" % (moved[0], name, got[moved[0]], want[moved[0]])
    assert len(got) == len(want), (name, len(got), len(want))
