"""Generates tests/golden/routing_decisions.json: which split-core form networks/pspnet_combine.py decides on, one character per
case, over flags x module state x grad mode x convolution geometry -- geometries of no network included.  Pure Python on the CPU:

    python tests/golden/make_golden_routing_decisions.py          (a second behind the imports)

The fixture was recorded on the commit named in it (the last one with one predicate per opt-in: _conv3x3_split,
BasicBlock._routed, _narrow_infer_routed, _early_routed, _train_routed, _narrow_train_routed, _wgrad_routed, _bnstats_routed and
the narrow-wgrad expression inside _train_conv); the LEGACY branches below are how those helpers were combined into one answer, in
the order of precedence their callers had, and the other branches ask the functions that replaced them (_frozen_form, _train_form).
Run on either kind of tree it writes the same bytes.  tests/test_routing_decisions_cpu.py imports this file, so the cases and
the patched geometry rules exist once.

The library is not loaded: ``_lib.has_entry`` answers True, ``SF._conv3x3_ok`` is a restatement of the entries' geometry rules
keyed by ``query`` (RULES), and ``_lib.get()`` hands the one rule conv3x3_narrow_train_supported asks directly.

Sections (the characters of a section are its cases in the order of its loops):
  block    a BasicBlock, _skd_infer_min_cin x _skd_infer_narrow x _skd_infer_stride2, frozen; one fully flagged state in the other modes
  bottle   a Bottleneck with and without _skd_teacher_early, every mode
  dsn      the convolution no opt-in is about (ResNet.dsn[0]: CONV3X3_SPLIT alone), every mode
  stem     the ResNet's stem gate and predicate, _skd_infer_narrow x _skd_teacher_early, every mode
  train    a BasicBlock, _skd_train_min_cin x narrow x wgrad x narrow_wgrad x bnstats, committed and emptied exclusion sets,
           training with grad; the fully flagged state with biased convolutions, and in the other modes
Frozen answers: "-" none, "w" wide, "n" narrow (64-column), "s" stride 2.  Training answers: one letter, TRAIN_CODE[form, weight
gradient on the core, statistics from the epilogue, _wgrad_routed of the shape].
"""
import contextlib
import itertools
import json
import os
import string
import subprocess
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from structure_knowledge_distillation_amd import _lib, functional as SF  # noqa: E402
from structure_knowledge_distillation_amd.networks import pspnet_combine as PC  # noqa: E402

OUT = os.path.join(HERE, "routing_decisions.json")
EXCLUSION_SETS = ("INFER_ROUTING_EXCLUDED", "TRAIN_ROUTING_EXCLUDED", "WGRAD_ROUTING_EXCLUDED", "NARROW_ROUTING_EXCLUDED",
                  "NARROW_WGRAD_ROUTING_EXCLUDED", "BNSTATS_ROUTING_EXCLUDED", "TEACHER_EARLY_ROUTING_EXCLUDED",
                  "STRIDE2_ROUTING_EXCLUDED")
MODES = [(False, False), (False, True), (True, False), (True, True)]      # (module.training, grad enabled); the first is frozen
FROZEN_CODE = {None: "-", False: "-", True: "w", "wide": "w", "narrow": "n", "s2": "s"}
TRAIN_CODE = dict(zip(itertools.product((None, "wide", "narrow"), (False, True), (False, True), (False, True)), string.ascii_letters))


def _plain(stride, cin, cout, s, p, d, g, cout_multiple, cin_multiple=16):
    return s == stride and g == 1 and cin % cin_multiple == 0 and cout % cout_multiple == 0 and (p == d if stride == 1 else p == d == 1)


RULES = {
    "skd_conv3x3_split_supported": lambda cin, cout, s, p, d, g: _plain(1, cin, cout, s, p, d, g, 128),
    "skd_conv3x3_narrow_supported": lambda cin, cout, s, p, d, g: _plain(1, cin, cout, s, p, d, g, 64),
    "skd_conv3x3_split_s2_supported": lambda cin, cout, s, p, d, g: _plain(2, cin, cout, s, p, d, g, 128),
    "skd_conv3x3_split_train_supported": lambda cin, cout, s, p, d, g: _plain(1, cin, cout, s, p, d, g, 128, 128),
}


def _ok(x, weight, stride, padding, dilation, groups, grad, entries, query, host_ok):
    """SF._conv3x3_ok with the back-end's answer restated; a host map passes (there is no device here)."""
    if torch.is_grad_enabled() != grad or not (x.dtype == torch.float32 and x.dim() == 4
                                               and x.is_contiguous(memory_format=torch.channels_last)):
        return False
    return x.shape[1] == weight.shape[1] * groups and RULES[query](weight.shape[1], weight.shape[0], stride, padding, dilation, groups)


@contextlib.contextmanager
def patched(emptied=False):
    """The library's answers restated (above); ``emptied``: every *_ROUTING_EXCLUDED of the module empty."""
    saved = [(SF, "_conv3x3_ok", SF._conv3x3_ok), (_lib, "has_entry", _lib.has_entry), (_lib, "get", _lib.get)]
    saved += [(PC, name, getattr(PC, name)) for name in EXCLUSION_SETS] if emptied else []
    back_end = types.SimpleNamespace(skd_conv3x3_narrow_supported=RULES["skd_conv3x3_narrow_supported"])
    try:
        SF._conv3x3_ok, _lib.has_entry, _lib.get = _ok, (lambda name: True), (lambda: back_end)
        for name in EXCLUSION_SETS if emptied else ():
            setattr(PC, name, frozenset())
        yield
    finally:
        for owner, name, value in saved:
            setattr(owner, name, value)


def convs(biases=(False, True)):
    """Cin x Cout x stride x dilation (padding == dilation) x bias, with a channels-last map of the right width each."""
    maps = {cin: torch.zeros(1, cin, 2, 2).contiguous(memory_format=torch.channels_last) for cin in (48, 64, 128, 256)}
    out = []
    for cin, cout, stride, d, bias in itertools.product((48, 64, 128, 256), (64, 128, 192, 256), (1, 2), (1, 2), biases):
        out.append((torch.nn.Conv2d(cin, cout, 3, stride, d, d, bias=bias), maps[cin]))
    return out


@contextlib.contextmanager
def mode(module, conv, training, grad):
    if module is not None and module.training != training:      # (a ResNet has 150 modules to tell)
        module.train(training)
    conv.training = training
    with torch.set_grad_enabled(grad):
        yield


# ---- the questions, as the commit the fixture was recorded on answered them and as the tree answers them now ----------------------

LEGACY = hasattr(PC, "_conv3x3_split")


def block_form(block, x, conv, residual):
    if not block._infer_form(x):
        return None
    return block._routed(x, conv, residual) if LEGACY else PC._frozen_form(block, x, conv, residual)


def bottleneck_form(block, x, conv):
    if LEGACY:
        return "wide" if PC._conv3x3_split(x, conv) else PC._early_routed(block, x, conv)
    return PC._frozen_form(block, x, conv)


def dsn_form(x, conv):
    return bool(PC._conv3x3_split(x, conv)) if LEGACY else PC._frozen_form(None, x, conv)


def stem_form(net, x, conv):
    if LEGACY:
        if net._stem_narrow(x):
            return PC._narrow_infer_routed(net, x, conv)
        return PC._early_routed(net, x, conv) if net._stem_early(x) else None
    return PC._frozen_form(net, x, conv) if net._stem_routed(x) else None


def train_form(block, x, conv, bn):
    cin, cout, d = conv.in_channels, conv.out_channels, conv.dilation[0]
    raw = bool(PC._wgrad_routed(block, cin, cout, d))
    if LEGACY:
        form = "wide" if PC._train_routed(block, x, conv) else "narrow" if PC._narrow_train_routed(block, x, conv) else None
        narrow_wgrad = bool(getattr(block, "_skd_train_narrow_wgrad", False) and (cin, cout, d) not in PC.NARROW_WGRAD_ROUTING_EXCLUDED)
        wgrad = form is not None and (raw if form == "wide" else narrow_wgrad)
        stats = form is not None and bool(PC._bnstats_routed(block, conv, bn))
    else:
        form, wgrad, stats = PC._train_form(block, x, conv, bn)
    return TRAIN_CODE[form, bool(wgrad), bool(stats), raw]


def sections():
    out = {}
    both, plain = convs(), convs((False,))
    block, bottle = PC.BasicBlock(64, 64), PC.Bottleneck(128, 64)
    net = PC.Res_pspnet(PC.BasicBlock, [2, 2, 2, 2], 19)

    def flag_block(min_cin, narrow, stride2):
        block._skd_infer_min_cin, block._skd_infer_narrow, block._skd_infer_stride2 = min_cin, narrow, stride2

    def flag_train(min_cin, narrow, wgrad, narrow_wgrad, bnstats):
        (block._skd_train_min_cin, block._skd_train_narrow, block._skd_train_wgrad, block._skd_train_narrow_wgrad,
         block._skd_train_bnstats) = min_cin, narrow, wgrad, narrow_wgrad, bnstats

    with patched():
        chars = []
        states = [(s, MODES[0]) for s in itertools.product((None, 128, 256), (False, True), (False, True))]
        for (state, (training, grad)) in states + [((128, True, True), m) for m in MODES[1:]]:
            flag_block(*state)
            for (conv, x), residual in itertools.product(both, (False, True)):
                with mode(block, conv, training, grad):
                    chars.append(FROZEN_CODE[block_form(block, x, conv, residual)])
        flag_block(None, False, False)
        out["block"] = "".join(chars)

        chars = []
        for early, (training, grad), (conv, x) in itertools.product((False, True), MODES, both):
            bottle._skd_teacher_early = early
            with mode(bottle, conv, training, grad):
                chars.append(FROZEN_CODE[bottleneck_form(bottle, x, conv)])
        out["bottle"] = "".join(chars)

        chars = []
        for (training, grad), (conv, x) in itertools.product(MODES, both):
            with mode(None, conv, training, grad):
                chars.append(FROZEN_CODE[dsn_form(x, conv)])
        out["dsn"] = "".join(chars)

        chars = []
        for narrow, early, (training, grad), (conv, x) in itertools.product((False, True), (False, True), MODES, both):
            net._skd_infer_narrow, net._skd_teacher_early = narrow, early
            with mode(net, conv, training, grad):
                chars.append(FROZEN_CODE[stem_form(net, x, conv)])
        out["stem"] = "".join(chars)

    chars = []
    flags = list(itertools.product((None, 128, 256), (False, True), (False, True), (False, True), (False, True)))
    everything = (128, True, True, True, True)
    for emptied in (False, True):
        with patched(emptied):
            runs = [(f, MODES[3], plain) for f in flags] + [(everything, MODES[3], convs((True,)))]
            runs += [(everything, m, plain) for m in MODES[:3]]
            for state, (training, grad), some in runs:
                flag_train(*state)
                for conv, x in some:
                    with mode(block, conv, training, grad):
                        chars.append(train_form(block, x, conv, block.bn1))
    out["train"] = "".join(chars)
    return out


def commit():
    return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()


def main():
    assert LEGACY or os.path.exists(OUT), "record on the commit with the old helpers first"
    fx = {"recorded_on": commit() if LEGACY else json.load(open(OUT))["recorded_on"], **sections()}
    with open(OUT, "w") as fh:
        json.dump(fx, fh, indent=0)
        fh.write("\n")
    print("wrote %s: %d bytes; %s" % (OUT, os.path.getsize(OUT), {k: len(v) for k, v in fx.items() if k != "recorded_on"}))


if __name__ == "__main__":
    main()
