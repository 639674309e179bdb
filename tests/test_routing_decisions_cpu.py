"""The routing decisions of networks/pspnet_combine.py against tests/golden/routing_decisions.json: for every recorded
combination of flags, module state, grad mode and convolution geometry -- geometries of no network included -- _frozen_form,
_train_form and _wgrad_routed give the answer the one-predicate-per-opt-in helpers gave on the commit the fixture names
(True reads "wide", False reads None; nothing else is mapped).  tests/golden/make_golden_routing_decisions.py has the cases,
the restated geometry rules and the encoding; no library is loaded."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(HERE, "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)
import make_golden_routing_decisions as G  # noqa: E402
from structure_knowledge_distillation_amd import _lib, functional as SF  # noqa: E402
from structure_knowledge_distillation_amd.networks import pspnet_combine as PC  # noqa: E402

SECTIONS = {"block": 3840, "bottle": 1024, "dsn": 512, "stem": 2048, "train": 6656}


@pytest.fixture(scope="module")
def answers():
    before = (SF._conv3x3_ok, _lib.has_entry, _lib.get, {name: getattr(PC, name) for name in G.EXCLUSION_SETS})
    got = G.sections()
    assert before == (SF._conv3x3_ok, _lib.has_entry, _lib.get, {name: getattr(PC, name) for name in G.EXCLUSION_SETS})
    return got


def test_fixture_is_small_and_complete():
    fx = json.load(open(G.OUT))
    smallest = min(os.path.getsize(os.path.join(os.path.dirname(G.OUT), f)) for f in os.listdir(os.path.dirname(G.OUT)) if f.endswith(".pt"))
    assert os.path.getsize(G.OUT) < smallest
    assert len(fx["recorded_on"]) == 40 and {k: len(v) for k, v in fx.items() if k != "recorded_on"} == SECTIONS
    for name in ("block", "bottle", "stem"):
        assert set(fx[name]) == set("-wns"), name      # every form is decided somewhere, and refused somewhere
    assert set(fx["dsn"]) == set("-w") and len(set(fx["train"])) >= 12


@pytest.mark.parametrize("section", list(SECTIONS))
def test_decisions_are_the_recorded_ones(answers, section):
    want, got = json.load(open(G.OUT))[section], answers[section]
    assert len(got) == len(want)
    moved = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not moved, "%d of %d cases of %r moved, the first at %d: %r, recorded %r" % (len(moved), len(want), section, moved[0],
                                                                                      got[moved[0]], want[moved[0]])
