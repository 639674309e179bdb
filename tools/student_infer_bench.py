"""Times the student's fused inference form (networks.fuse_for_inference) against the path it replaces, on one MI355X, in one
process, with tools/_timing.warm_timed (GPU warmed up in front of every figure) and interleaved A/B rounds: parent, fused, parent,
fused, ... so that both sides see the same clocks, and the spread of a side's repeated identical runs is in the table next to
the difference between the sides.

Per launch -- every BasicBlock convolution shape of the student at the 1024 x 2048 evaluation sizes (batch 1) plus the 128-wide
candidates.  Parent: what an unflagged block runs for the same work, the MIOpen convolution followed by the in-place eval-mode
InPlace-ABN pass (``bn.forward_relu(conv(x)[, residual])``: BN + ReLU, or BN + residual + ReLU, one pass).  Fused: one launch of
csrc/conv3x3.hip with that epilogue (``conv3x3_split_eval`` / ``conv3x3_split_res_eval``).

Whole forward -- the seeded student, batch 1 at 1024 x 2048, and the five-scale flip set of tools/multiscale_eval_bench.py (five
batches of 2), each without ``fuse_for_inference`` and with it at every ``--min-cin`` (default: the frozen teacher's 256 and the
shipped FUSED_EVAL_MIN_CIN), and with ``narrow=True`` on top of the shipped policy (the row "fused, narrow": the stem and layer1 on
the split core too, the 64-column form of csrc/conv3x3.hip).

    python tools/student_infer_bench.py [--rounds 3] [--min-cin 256 128] [--skip-launches] [--out FILE]

Prints one JSON line and writes the tables to ``--out`` (default profiles/r17_student_infer.md).
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import structure_knowledge_distillation_amd as S  # noqa: E402
from structure_knowledge_distillation_amd import functional as SF  # noqa: E402
from _timing import warm_timed  # noqa: E402

SCALES = (0.75, 1.0, 1.25, 1.5, 1.75)
# (label, Cin, Cout, dilation, H, W, residual form too?)
LAUNCHES = [
    ("layer3 256->256 d2", 256, 256, 2, 129, 257, True),
    ("layer4 512->512 d4", 512, 512, 4, 129, 257, True),
    ("layer3.0.conv1 128->256 d2", 128, 256, 2, 129, 257, False),
    ("layer4.0.conv1 256->512 d4", 256, 512, 4, 129, 257, False),
    ("layer2 128->128 d1 (candidate)", 128, 128, 1, 129, 257, True),
    ("stem conv3 64->128 d1 (candidate)", 64, 128, 1, 512, 1024, False),
]


def stats(v):
    s = sorted(v)
    med = s[len(s) // 2]
    return {"runs_ms": v, "median_ms": med, "spread": (s[-1] - s[0]) / med}


def ab(parent, fused, rounds, **kw):
    a, b = [], []
    for _ in range(rounds):
        a.append(warm_timed(parent, **kw))
        b.append(warm_timed(fused, **kw))
    a, b = stats(a), stats(b)
    ratio = a["median_ms"] / b["median_ms"]
    noise = max(a["spread"], b["spread"])
    verdict = "ahead" if ratio > 1.0 + noise else ("behind" if ratio < 1.0 - noise else "within the spread")
    return {"parent": a, "fused": b, "parent_over_fused": ratio, "verdict": verdict}


def launch_case(cin, cout, dil, h, w, residual, dev, rounds):
    from structure_knowledge_distillation_amd.networks import pspnet_combine as PC
    g = torch.Generator().manual_seed(cin + cout + dil)
    conv = torch.nn.Conv2d(cin, cout, 3, 1, dil, dil, bias=False)
    bn = PC.BatchNorm2d(cout)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(cout, generator=g) * 0.3)
        bn.running_var.copy_(torch.rand(cout, generator=g) + 0.5)
    conv, bn = conv.to(dev).to(memory_format=torch.channels_last).eval(), bn.to(dev).eval()
    x = torch.relu(torch.randn(1, cin, h, w, generator=g)).to(dev).contiguous(memory_format=torch.channels_last)
    r = torch.randn(1, cout, h, w, generator=g).to(dev).contiguous(memory_format=torch.channels_last) if residual else None
    pack = SF.conv3x3_pack_weights(conv)
    if residual:
        parent = lambda: bn.forward_relu(conv(x), r)
        fused = lambda: SF.conv3x3_split_res_eval(x, pack, cout, dil, r, bn, "relu")
    else:
        parent = lambda: bn.forward_relu(conv(x))
        fused = lambda: SF.conv3x3_split_eval(x, pack, cout, dil, None, bn, "relu")
    diff = float((parent() - fused()).abs().max())
    res = ab(parent, fused, rounds, reps=10, warm_ms=30.0, groups=5)
    res["max_abs_difference"] = diff
    return res


def fmt_runs(s):
    return " / ".join("%.3f" % v for v in s["runs_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-cin", type=int, nargs="+", default=None, help="fuse_for_inference policies of the whole-forward rows")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_student_infer.md"))
    ap.add_argument("--skip-multiscale", action="store_true")
    ap.add_argument("--skip-launches", action="store_true", help="the whole-forward tables only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("student_infer_bench needs an MI355X: there is no CPU timing")
    S.configure_miopen()
    from structure_knowledge_distillation_amd.networks import fuse_for_inference, pspnet_combine as PC
    min_cins = sorted({PC.CONV3X3_SPLIT_MIN_CIN, PC.FUSED_EVAL_MIN_CIN}, reverse=True) if args.min_cin is None else args.min_cin
    dev = torch.device("cuda", 0)
    out = {"rounds": args.rounds, "min_cins": min_cins, "launches": {}, "forwards": {}}
    with torch.no_grad():
        for label, cin, cout, dil, h, w, both in ([] if args.skip_launches else LAUNCHES):
            for residual in ((False, True) if both else (False,)):
                key = label + (" + residual" if residual else "")
                out["launches"][key] = launch_case(cin, cout, dil, h, w, residual, dev, args.rounds)
                print(key, json.dumps(out["launches"][key]), flush=True)

        H, W = 1024, 2048
        g = torch.Generator().manual_seed(3)
        image = (torch.randn(1, 3, H, W, generator=g) * 57.0).to(dev)
        torch.manual_seed(1)
        net = PC.Res_pspnet(PC.BasicBlock, [2, 2, 2, 2], 19).to(dev).to(memory_format=torch.channels_last).eval()
        sets = {"batch 1 at 1024 x 2048": [image.contiguous(memory_format=torch.channels_last)]}
        if not args.skip_multiscale:
            sets["five scales with flip (5 batches of 2)"] = [SF.zoom_linear(image, s, mirror=True, channels_last=True) for s in SCALES]
        for name, batches in sets.items():
            run = lambda: [net(b) for b in batches]
            fuse_for_inference(net, enable=False)
            plain = [o[0].clone() for o in run()]
            sides = [("plain", None)] + [("fused, min_cin %d" % m, m) for m in min_cins] + [("fused, narrow", "narrow")]
            runs, diff = {k: [] for k, _ in sides}, {}
            for _ in range(args.rounds):
                for k, m in sides:
                    fuse_for_inference(net, enable=False)
                    if m == "narrow":
                        fuse_for_inference(net, narrow=True)
                    elif m is not None:
                        fuse_for_inference(net, min_cin=m)
                    runs[k].append(warm_timed(run, reps=2, warm_ms=200.0, groups=3))
                    diff[k] = max(float((p - o[0]).abs().max() / p.abs().max()) for p, o in zip(plain, run()))
            res = {k: dict(stats(v), logits_max_rel_difference=diff[k]) for k, v in runs.items()}
            for k in res:
                res[k]["plain_over_this"] = res["plain"]["median_ms"] / res[k]["median_ms"]
            out["forwards"][name] = res
            print(name, json.dumps(res), flush=True)
    print(json.dumps(out))

    lines = [
        "# The student's fused inference form on one MI355X: per launch and per forward",
        "",
        "Written by `python tools/student_infer_bench.py --rounds %d` (one process; `tools/_timing.warm_timed`: >= 30 ms of the same" % args.rounds,
        "launches as warm-up, then the median of 5 groups of 10 back-to-back launches; the forwards: >= 200 ms warm-up, median of 3",
        "groups of 2).  Every row is %d interleaved rounds parent, fused, parent, fused, ...; the runs column lists each round, **spread**" % args.rounds,
        "is (max - min) / median of one side's repeated identical runs, the larger of the two sides.",
        "",
    ]
    if not args.skip_launches:
        lines += [
            "## Per launch, batch 1",
            "",
            "Parent: the MIOpen fp32 convolution (channels-last) + the in-place eval-mode InPlace-ABN pass with ReLU, which also adds the",
            "residual where there is one (`bn.forward_relu(conv(x)[, residual])`, what an unflagged BasicBlock runs).  Fused: one launch of",
            "`csrc/conv3x3.hip` with BN + ReLU (`skd_conv3x3_split_nhwc`) or BN + residual + ReLU (`skd_conv3x3_split_res_nhwc`) in the epilogue.",
            "",
            "| convolution | map | parent ms (runs) | fused ms (runs) | parent median | fused median | parent / fused | spread | verdict |",
            "|---|---|---|---|---|---|---|---|---|",
        ]
    for label, cin, cout, dil, h, w, both in ([] if args.skip_launches else LAUNCHES):
        for residual in ((False, True) if both else (False,)):
            key = label + (" + residual" if residual else "")
            r = out["launches"][key]
            lines.append("| %s | %d x %d | %s | %s | %.3f | %.3f | %.2f | %.1f %% | %s |" % (
                key, h, w, fmt_runs(r["parent"]), fmt_runs(r["fused"]), r["parent"]["median_ms"], r["fused"]["median_ms"],
                r["parent_over_fused"], 100 * max(r["parent"]["spread"], r["fused"]["spread"]), r["verdict"]))
    lines += ["", "## Whole forward (Res_pspnet BasicBlock [2, 2, 2, 2], seeded, eval, channels-last)", "",
              "Interleaved per round: plain, then `fuse_for_inference(net, min_cin=m)` for every m listed, then",
              "`fuse_for_inference(net, narrow=True)` (\"fused, narrow\": the shipped min_cin plus the stem and layer1).", "",
              "| input | forward | ms (runs) | median ms | plain / this | spread | logits: max difference from plain / max |", "|---|---|---|---|---|---|---|"]
    for name, res in out["forwards"].items():
        for k, r in res.items():
            lines.append("| %s | %s | %s | %.2f | %.3f | %.1f %% | %.1e |" % (name, k, fmt_runs(r), r["median_ms"], r["plain_over_this"],
                                                                          100 * r["spread"], r["logits_max_rel_difference"]))
    lines += ["", "The parent's convolutions are MIOpen's with the find-db shipped in `miopen_db/`, which was tuned for the 512 x 512 training",
              "shapes only: at these map sizes MIOpen runs whatever its heuristics pick.  That is the path an unflagged student takes today, so it",
              "is the baseline here; it is not MIOpen at its best."]
    lines += ["", "Not measured: other batch sizes or image sizes, a counter profile of the new instantiations.  The 64-column shapes of the stem",
              "and layer1, isolated: profiles/r21_conv3x3_narrow_isolated.md (tools/conv3x3_narrow_bench.py).", ""]
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
