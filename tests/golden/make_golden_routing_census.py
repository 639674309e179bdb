"""Generates tests/golden/routing_census.json: which op of ``functional`` each convolution of the two networks is handed to, per
opt-in, with the arguments the op sees -- the call sequence networks/pspnet_combine.py produces on the real library.  On an MI355X:

    python tests/golden/make_golden_routing_census.py --recorded-on COMMIT [--out FILE] [--hashes FILE]          (about a minute)

Every public function of ``functional`` named conv3x3_* / conv1x1_* / ppm_fold_bottleneck (the *_supported predicates excluded) is
wrapped by one generic wrapper: it binds the call to the op's signature, fills the defaults in -- so ``f(x)`` and ``f(x, pieces=3)``
log alike, and only what the op is told counts -- and logs the name with tensors as shapes, modules as type and channels,
caches as "cache", everything else by ``repr``.  A forward hook on every nn.Conv2d logs ``library(qualified name)``: a convolution
the network calls appears once per forward, as the one or the other.  The calls of the enabling function (the pre-packing of
fuse_for_inference / route_teacher_early) are part of a configuration's log, and so is the backward of a training configuration.

Input: 2 x 3 x 49 x 49 channels-last (maps of 25, 13 and 7 pixels: the PSP fold's min(H, W) >= 6 holds).  The weights are those of
oracle.step_torch.pspnet_init; only call sequences are recorded, never output bits (--hashes writes a SHA-256 of each no-grad
configuration's outputs for a comparison of two trees in one session; it is no fixture).  A ``toggle_*`` configuration enables an
opt-in, runs, disables it and runs again: that last log must be the unflagged one, and the network must then carry the weight packs
an unflagged network carries and no other.  main() asserts the documented counts before it writes.
"""
import contextlib
import copy
import functools
import hashlib
import inspect
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import step_torch as O  # noqa: E402
from structure_knowledge_distillation_amd import functional as SF  # noqa: E402
from structure_knowledge_distillation_amd.networks import pspnet_combine as PC  # noqa: E402

OUT = os.path.join(HERE, "routing_census.json")
SIZE = (2, 3, 49, 49)
SEEDS = {"student": 2811, "teacher": 2812, "x": 2813}
ALL = dict(wgrad=True, narrow=True, narrow_wgrad=True, shortcut=True, bnstats=True)
EMPTIED = {name: frozenset() for name in dir(PC) if name.endswith("_ROUTING_EXCLUDED")}
TEACHER_EXCLUDED = dict(SPLIT2_ROUTING_EXCLUDED=frozenset({("1x1", 512, 1024), ("3x3", 128, 128, 1)}),
                        TEACHER_EARLY_ROUTING_EXCLUDED=frozenset({(128, 128, 2, 1)}))
HASHES = {}
_NETS = {}


def _describe(v):
    if isinstance(v, torch.Tensor):
        return "T" + "x".join(str(n) for n in v.shape)
    if isinstance(v, torch.nn.Conv2d):
        return "%s:%d>%d" % (type(v).__name__, v.in_channels, v.out_channels)
    if isinstance(v, torch.nn.Module):
        return "%s:%s" % (type(v).__name__, getattr(v, "num_features", "-"))
    if isinstance(v, dict):
        return "cache"
    if isinstance(v, (list, tuple)):
        return "(%s)" % ",".join(_describe(i) for i in v)
    return repr(v)


def wrapped_names():
    return [n for n in sorted(vars(SF)) if (n.startswith(("conv3x3_", "conv1x1_")) or n == "ppm_fold_bottleneck")
            and not n.endswith("_supported") and inspect.isfunction(getattr(SF, n))]


@contextlib.contextmanager
def census(model, log):
    """Log into ``log`` every wrapped op (looked up on ``functional`` at call time, by the networks and by the ops themselves) and
    every nn.Conv2d of ``model`` that is called."""
    def wrap(name, real):
        signature = inspect.signature(real)

        @functools.wraps(real)
        def op(*args, **kwargs):
            bound = signature.bind(*args, **kwargs)
            bound.apply_defaults()
            log.append("%s(%s)" % (name, ",".join(_describe(v) for v in bound.arguments.values())))
            return real(*args, **kwargs)
        return op
    saved = {n: getattr(SF, n) for n in wrapped_names()}
    hooks = [m.register_forward_hook(lambda mod, args, out, q=q: log.append("library(%s)" % q))
             for q, m in model.named_modules() if isinstance(m, torch.nn.Conv2d)]
    try:
        for n, real in saved.items():
            setattr(SF, n, wrap(n, real))
        yield log
    finally:
        for n, real in saved.items():
            setattr(SF, n, real)
        for h in hooks:
            h.remove()


@contextlib.contextmanager
def excluded(sets):
    saved = {name: getattr(PC, name) for name in sets}
    try:
        for name, value in sets.items():
            setattr(PC, name, value)
        yield
    finally:
        for name, value in saved.items():
            setattr(PC, name, value)


def nets():
    """The seeded student and frozen teacher on the device, channels-last, and the input (made once; configurations copy them)."""
    if not _NETS:
        dev = torch.device("cuda", 0)
        student = PC.Res_pspnet(PC.BasicBlock, [2, 2, 2, 2], 19)
        student.load_state_dict(O.pspnet_init(O.STUDENT, 19, seed=SEEDS["student"]))
        teacher = PC.Res_pspnet(PC.Bottleneck, [3, 4, 23, 3], 19)
        teacher.load_state_dict(O.pspnet_init(O.TEACHER, 19, seed=SEEDS["teacher"]))
        for p in teacher.parameters():
            p.requires_grad_(False)
        x = torch.randn(SIZE, generator=torch.Generator().manual_seed(SEEDS["x"]))
        _NETS.update(student=student.to(dev).to(memory_format=torch.channels_last),
                     teacher=teacher.eval().to(dev).to(memory_format=torch.channels_last),
                     x=x.to(dev).contiguous(memory_format=torch.channels_last))
    return _NETS


def packs(model):
    """Every weight pack of the split-core 3x3 forms ``model`` carries: (module, attribute or fold-cache key)."""
    found = []
    for q, m in model.named_modules():
        found += [(q, a) for a in vars(m) if a.startswith("_skd_conv3x3") and "pack" in a]
        found += [(q, a) for a in getattr(m, "_fold_cache", {}) if "pack3x3" in a]
    return sorted(found)


def forward(model, x, train, name=None):
    """One training forward + backward of the summed outputs, or one eval-mode forward under no_grad."""
    model.train(train)
    if train:
        sum(o.sum() for o in model(x) if o is not None).backward()
        return
    with torch.no_grad():
        outs = model(x)
    torch.cuda.synchronize()
    if name is not None:
        HASHES[name] = hashlib.sha256(b"".join(o.float().cpu().numpy().tobytes() for o in outs if o is not None)).hexdigest()


def _plain(model):
    return model


# name: (network, training forward?, exclusion sets patched, what enables the opt-in)
CONFIGURATIONS = {
    "student_train": ("student", True, {}, _plain),
    "student_train_split": ("student", True, {}, lambda m: PC.route_training_convs(m)),
    "student_train_wgrad": ("student", True, {}, lambda m: PC.route_training_convs(m, wgrad=True)),
    "student_train_narrow": ("student", True, {}, lambda m: PC.route_training_convs(m, narrow=True)),
    "student_train_narrow_wgrad": ("student", True, {}, lambda m: PC.route_training_convs(m, narrow=True, narrow_wgrad=True)),
    "student_train_shortcut": ("student", True, {}, lambda m: PC.route_training_convs(m, shortcut=True)),
    "student_train_bnstats": ("student", True, {}, lambda m: PC.route_training_convs(m, bnstats=True)),
    "student_train_all": ("student", True, {}, lambda m: PC.route_training_convs(m, **ALL)),
    "student_train_all_emptied": ("student", True, EMPTIED, lambda m: PC.route_training_convs(m, **ALL)),
    "student_train_fused": ("student", True, {}, lambda m: PC.fuse_for_inference(m, narrow=True, stride2=True)),
    "student_eval": ("student", False, {}, _plain),
    "student_eval_fused": ("student", False, {}, lambda m: PC.fuse_for_inference(m)),
    "student_eval_fused_narrow": ("student", False, {}, lambda m: PC.fuse_for_inference(m, narrow=True)),
    "student_eval_fused_stride2": ("student", False, {}, lambda m: PC.fuse_for_inference(m, stride2=True)),
    "student_eval_fused_both": ("student", False, {}, lambda m: PC.fuse_for_inference(m, narrow=True, stride2=True)),
    "student_eval_train_flagged": ("student", False, {}, lambda m: PC.route_training_convs(m, **ALL)),
    "teacher": ("teacher", False, {}, _plain),
    "teacher_pieces2": ("teacher", False, {}, lambda m: PC.set_teacher_pieces(m, 2)),
    "teacher_early": ("teacher", False, {}, lambda m: PC.route_teacher_early(m)),
    "teacher_both": ("teacher", False, {}, lambda m: PC.route_teacher_early(PC.set_teacher_pieces(m, 2))),
    "teacher_both_excluded": ("teacher", False, TEACHER_EXCLUDED, lambda m: PC.route_teacher_early(PC.set_teacher_pieces(m, 2))),
}
# name: (the unflagged configuration its last log must equal, what enables, what disables)
TOGGLES = {
    "toggle_fuse_for_inference": ("student_eval", lambda m: PC.fuse_for_inference(m, narrow=True, stride2=True),
                                  lambda m: PC.fuse_for_inference(m, enable=False)),
    "toggle_route_training_convs": ("student_train", lambda m: PC.route_training_convs(m, **ALL),
                                    lambda m: PC.route_training_convs(m, enable=False)),
    "toggle_route_teacher_early": ("teacher", lambda m: PC.route_teacher_early(m), lambda m: PC.route_teacher_early(m, enable=False)),
    "toggle_set_teacher_pieces": ("teacher", lambda m: PC.set_teacher_pieces(m, 2), lambda m: PC.set_teacher_pieces(m, pieces=3)),
}
NAMES = list(CONFIGURATIONS) + list(TOGGLES)


def run(name):
    """The log of configuration ``name`` on a fresh copy of its network."""
    base = nets()
    log = []
    if name in CONFIGURATIONS:
        which, train, sets, enable = CONFIGURATIONS[name]
        model = copy.deepcopy(base[which])
        with excluded(sets), census(model, log):
            assert enable(model) is model
            forward(model, base["x"], train, name)
        return log
    plain_name, enable, disable = TOGGLES[name]
    which, train, _, _ = CONFIGURATIONS[plain_name]
    model, plain = copy.deepcopy(base[which]), copy.deepcopy(base[which])
    assert enable(model) is model
    forward(model, base["x"], train)
    assert disable(model) is model
    model.zero_grad(set_to_none=True)
    with census(model, log):
        forward(model, base["x"], train)
    forward(plain, base["x"], train)
    assert packs(model) == packs(plain), (name, packs(model), packs(plain))
    return log


def count(log, op, *having):
    return sum(1 for c in log if c.startswith(op + "(") and all(h in c for h in having))


def check_counts(fx):
    """What the documentation of the opt-ins says they route, at this size."""
    ends = lambda name, ops, tail: sum(1 for c in fx[name] if c.startswith(ops) and c.endswith(tail))
    stats = lambda name: ends(name, "conv3x3_split_train(", ",True)")
    two = lambda name: ends(name, ("conv3x3_split_eval(", "conv3x3_s2_eval("), ",2)")
    got = {
        "split_train": [count(fx[n], "conv3x3_split_train") for n in ("student_train", "student_train_split", "student_train_narrow")],
        "narrow form": count(fx["student_train_narrow"], "conv3x3_split_train", "True"),
        "shortcut": count(fx["student_train_shortcut"], "conv1x1_split_train"),
        "wgrad": [count(fx[n], "conv3x3_split_wgrad") for n in ("student_train_split", "student_train_wgrad")],
        "narrow wgrad": [count(fx[n], "conv3x3_narrow_wgrad") for n in ("student_train_all", "student_train_all_emptied")],
        "stats": [stats(n) for n in ("student_train_bnstats", "student_train_all", "student_train_all_emptied")],
        "fused narrow": [count(fx[n], "conv3x3_narrow_eval") for n in ("student_eval", "student_eval_fused", "student_eval_fused_narrow",
                                                                       "student_eval_fused_both")],
        "fused s2": [count(fx[n], "conv3x3_s2_eval") for n in ("student_eval", "student_eval_fused", "student_eval_fused_stride2",
                                                               "student_eval_fused_both")],
        "fused residual": count(fx["student_eval_fused"], "conv3x3_split_res_eval"),
        "early narrow": [count(fx[n], "conv3x3_narrow_eval") for n in ("teacher", "teacher_early", "teacher_both")],
        "early s2": [count(fx[n], "conv3x3_s2_eval") for n in ("teacher", "teacher_early", "teacher_both", "teacher_both_excluded")],
        "early wide": count(fx["teacher_early"], "conv3x3_split_eval") - count(fx["teacher"], "conv3x3_split_eval"),
        "two pieces": [two("teacher"), two("teacher_early"), two("teacher_both") - two("teacher_pieces2")],
    }
    want = {"split_train": [0, 13, 19], "narrow form": 6, "shortcut": 4, "wgrad": [0, 13], "narrow wgrad": [0, 6], "stats": [0, 0, 15],
            "fused narrow": [0, 0, 5, 5], "fused s2": [0, 0, 1, 1], "fused residual": 6, "early narrow": [0, 4, 4],
            "early s2": [0, 1, 1, 0], "early wide": 4, "two pieces": [0, 0, 5]}
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert two("teacher_both_excluded") < two("teacher_both")
    assert [c for c in fx["student_train_fused"] if "pack_weights(" not in c] == fx["student_train"]      # but for the pre-packing
    for name, (plain_name, _, _) in TOGGLES.items():
        assert fx[name] == fx[plain_name], name


def main():
    """--recorded-on COMMIT names the commit of the tree this runs on (a tree without its history cannot tell); without it the
    name in the existing fixture stays."""
    arg = lambda flag, default=None: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else default
    fx = {name: run(name) for name in NAMES}
    check_counts(fx)
    if arg("--hashes"):
        with open(arg("--hashes"), "w") as fh:
            json.dump(HASHES, fh, indent=1, sort_keys=True)
    recorded_on = arg("--recorded-on") or json.load(open(OUT))["recorded_on"]
    out = arg("--out", OUT)
    with open(out, "w") as fh:
        json.dump({"recorded_on": recorded_on, **fx}, fh, indent=0)
        fh.write("\n")
    print("wrote %s: %d bytes; %d configurations, %d calls" % (out, os.path.getsize(out), len(NAMES), sum(len(fx[n]) for n in NAMES)))


if __name__ == "__main__":
    main()
