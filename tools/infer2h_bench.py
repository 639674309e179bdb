"""Times the student's fused inference form on two FP16 pieces (fuse_for_inference(piece_format="fp16"), include/skd_infer2h.h)
against the same form on three bf16 pieces, on one MI355X, in one process, by the convention of tools/student_infer_bench.py (whose
helpers it uses): tools/_timing.warm_timed in front of every figure, interleaved A/B rounds, spread = (max - min) / median of one
side's repeated identical runs, the medians reported.

Per launch -- every routed shape of the student at the 1024 x 2048 evaluation sizes, batch 1 and 2: 129 x 257 for layer2 - 4,
257 x 513 for the stem's shapes, layer1 and the stride-2 input (and the stem's two convolutions at the 512 x 1024 they really run at).
A: the three-piece op of the form; B: its fp16 twin; both with eval-mode BN + ReLU (+ residual) in the epilogue, the stem's conv3 raw.
A shape is "ahead" when A / B exceeds 1 + the larger side's spread; pspnet_combine.INFER2H_ROUTING_EXCLUDED lists the shapes that
are not ahead at both batch sizes.

Whole forward -- the seeded student, batch 1 at 1024 x 2048, and the five-scale flip set of tools/multiscale_eval_bench.py: plain,
``fuse_for_inference(narrow=True, stride2=True)``, and the same with ``piece_format="fp16"`` (with the shipped exclusion set and with
the set emptied), with the logits' largest difference from plain.

    python tools/infer2h_bench.py [--rounds 3] [--skip-launches] [--skip-forwards] [--out-launches FILE] [--out-forwards FILE]

Prints one JSON line and writes the tables (default profiles/r34_infer2h_isolated.md, profiles/r34_student_infer.md).
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
from student_infer_bench import SCALES, ab, fmt_runs, stats  # noqa: E402
from _timing import warm_timed  # noqa: E402

# (label, form, Cin, Cout, dilation, H, W): form as in pspnet_combine.INFER2H_ROUTING_EXCLUDED
LAUNCHES = [
    ("layer2 conv1 128->128", "wide", 128, 128, 1, 129, 257),
    ("layer2 conv2 128->128", "wide+res", 128, 128, 1, 129, 257),
    ("layer3.0.conv1 128->256 d2", "wide", 128, 256, 2, 129, 257),
    ("layer3 conv1 256->256 d2", "wide", 256, 256, 2, 129, 257),
    ("layer3 conv2 256->256 d2", "wide+res", 256, 256, 2, 129, 257),
    ("layer4.0.conv1 256->512 d4", "wide", 256, 512, 4, 129, 257),
    ("layer4 conv1 512->512 d4", "wide", 512, 512, 4, 129, 257),
    ("layer4 conv2 512->512 d4", "wide+res", 512, 512, 4, 129, 257),
    ("stem conv2 64->64", "narrow", 64, 64, 1, 257, 513),
    ("stem conv3 64->128 (raw)", "wide", 64, 128, 1, 257, 513),
    ("layer1.0.conv1 128->64", "narrow", 128, 64, 1, 257, 513),
    ("layer1 conv1 64->64", "narrow", 64, 64, 1, 257, 513),
    ("layer1 conv2 64->64", "narrow+res", 64, 64, 1, 257, 513),
    ("layer2.0.conv1 64->128 stride 2", "s2", 64, 128, 1, 257, 513),
    ("stem conv2 64->64 at its own size", "narrow", 64, 64, 1, 512, 1024),
    ("stem conv3 64->128 (raw) at its own size", "wide", 64, 128, 1, 512, 1024),
]


def launch_case(form, cin, cout, dil, h, w, batch, raw, dev, rounds):
    from structure_knowledge_distillation_amd.networks import pspnet_combine as PC
    g = torch.Generator().manual_seed(cin + cout + dil + batch)
    stride = 2 if form == "s2" else 1
    conv = torch.nn.Conv2d(cin, cout, 3, stride, dil, dil, bias=False)
    bn = PC.BatchNorm2d(cout)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(cout, generator=g) * 0.3)
        bn.running_var.copy_(torch.rand(cout, generator=g) + 0.5)
    conv, bn = conv.to(dev).to(memory_format=torch.channels_last).eval(), bn.to(dev).eval()
    x = torch.relu(torch.randn(batch, cin, h, w, generator=g)).to(dev).contiguous(memory_format=torch.channels_last)
    r = None
    if form.endswith("+res"):
        r = torch.randn(batch, cout, h, w, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    epi = (None, "none") if raw else (bn, "relu")
    if form.startswith("narrow"):
        p3, ph = SF.conv3x3_narrow_pack_weights(conv), SF.conv3x3_narrow_pack_weights_fp16(conv)
        three = lambda: SF.conv3x3_narrow_eval(x, p3, cout, dil, r, None, *epi)
        half = lambda: SF.conv3x3_narrow_eval_fp16(x, ph, cout, dil, r, None, *epi)
    else:
        p3, ph = SF.conv3x3_pack_weights(conv), SF.conv3x3_pack_weights_fp16(conv)
        if form == "s2":
            three = lambda: SF.conv3x3_s2_eval(x, p3, cout, None, *epi)
            half = lambda: SF.conv3x3_s2_eval_fp16(x, ph, cout, None, *epi)
        elif r is not None:
            three = lambda: SF.conv3x3_split_res_eval(x, p3, cout, dil, r, *epi)
            half = lambda: SF.conv3x3_split_res_eval_fp16(x, ph, cout, dil, r, *epi)
        else:
            three = lambda: SF.conv3x3_split_eval(x, p3, cout, dil, None, *epi)
            half = lambda: SF.conv3x3_split_eval_fp16(x, ph, cout, dil, None, *epi)
    a, b = three(), half()
    diff = float((a - b).abs().max() / a.abs().max())
    res = ab(three, half, rounds, reps=10, warm_ms=30.0, groups=5)      # "parent" = three bf16 pieces, "fused" = two fp16 pieces
    res["max_rel_difference"] = diff
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out-launches", default=os.path.join(ROOT, "profiles", "r34_infer2h_isolated.md"))
    ap.add_argument("--out-forwards", default=os.path.join(ROOT, "profiles", "r34_student_infer.md"))
    ap.add_argument("--skip-launches", action="store_true")
    ap.add_argument("--skip-forwards", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("infer2h_bench needs an MI355X: there is no CPU timing")
    S.configure_miopen()
    from structure_knowledge_distillation_amd.networks import fuse_for_inference, pspnet_combine as PC
    if not SF.infer2h_supported():
        raise SystemExit("this back-end lacks the entries of include/skd_infer2h.h")
    dev = torch.device("cuda", 0)
    out = {"rounds": args.rounds, "launches": {}, "forwards": {}, "excluded": sorted(PC.INFER2H_ROUTING_EXCLUDED)}
    with torch.no_grad():
        if not args.skip_launches:
            for label, form, cin, cout, dil, h, w in LAUNCHES:
                for batch in (1, 2):
                    key = "%s | %s | %d x %d | batch %d" % (label, form, h, w, batch)
                    out["launches"][key] = launch_case(form, cin, cout, dil, h, w, batch, "(raw)" in label, dev, args.rounds)
                    print(key, json.dumps(out["launches"][key]), flush=True)
        if not args.skip_forwards:
            H, W = 1024, 2048
            g = torch.Generator().manual_seed(3)
            image = (torch.randn(1, 3, H, W, generator=g) * 57.0).to(dev)
            torch.manual_seed(1)
            net = PC.Res_pspnet(PC.BasicBlock, [2, 2, 2, 2], 19).to(dev).to(memory_format=torch.channels_last).eval()
            sets = {"batch 1 at 1024 x 2048": [image.contiguous(memory_format=torch.channels_last)],
                    "five scales with flip (5 batches of 2)": [SF.zoom_linear(image, s, mirror=True, channels_last=True) for s in SCALES]}
            shipped = PC.INFER2H_ROUTING_EXCLUDED
            sides = [("plain", None), ("fused, narrow, stride2", ("bf16", shipped)), ("fused, narrow, stride2, fp16", ("fp16", shipped))]
            if shipped:
                sides.append(("fused, narrow, stride2, fp16, exclusion set emptied", ("fp16", frozenset())))
            for name, batches in sets.items():
                run = lambda: [net(b) for b in batches]
                fuse_for_inference(net, enable=False)
                plain = [o[0].clone() for o in run()]
                runs, diff = {k: [] for k, _ in sides}, {}
                for _ in range(args.rounds):
                    for k, m in sides:
                        fuse_for_inference(net, enable=False)
                        if m is not None:
                            PC.INFER2H_ROUTING_EXCLUDED = m[1]
                            fuse_for_inference(net, narrow=True, stride2=True, piece_format=m[0])
                        runs[k].append(warm_timed(run, reps=2, warm_ms=200.0, groups=3))
                        diff[k] = max(float((p - o[0]).abs().max() / p.abs().max()) for p, o in zip(plain, run()))
                        PC.INFER2H_ROUTING_EXCLUDED = shipped
                res = {k: dict(stats(v), logits_max_rel_difference=diff[k]) for k, v in runs.items()}
                for k in res:
                    res[k]["plain_over_this"] = res["plain"]["median_ms"] / res[k]["median_ms"]
                    res[k]["three_over_this"] = res["fused, narrow, stride2"]["median_ms"] / res[k]["median_ms"]
                out["forwards"][name] = res
                print(name, json.dumps(res), flush=True)
    print(json.dumps(out))

    head = ["Written by `python tools/infer2h_bench.py --rounds %d` (one process; `tools/_timing.warm_timed`: >= 30 ms of the same" % args.rounds,
            "launches as warm-up, then the median of 5 groups of 10 back-to-back launches; the forwards: >= 200 ms warm-up, median of 3",
            "groups of 2).  Every row is %d interleaved rounds A, B, A, B, ...; the runs column lists each round, **spread** is" % args.rounds,
            "(max - min) / median of one side's repeated identical runs, the larger of the two sides.", ""]
    if not args.skip_launches:
        lines = ["# The student's inference shapes on two fp16 pieces against three bf16 pieces, per launch, on one MI355X", ""] + head + [
            "A: the three-piece op of the form (`conv3x3_split_eval`, `conv3x3_split_res_eval`, `conv3x3_narrow_eval`, `conv3x3_s2_eval`);",
            "B: its fp16 twin (include/skd_infer2h.h; the wide form without residual: skd_split2h.h).  Eval-mode BN + ReLU (+ residual) in",
            "the epilogue, the stem's conv3 raw.  **ahead**: A / B > 1 + spread.", "",
            "| convolution | form | map | batch | bf16 x 3 ms (runs) | fp16 x 2 ms (runs) | bf16 x 3 median | fp16 x 2 median | A / B | spread | verdict |",
            "|---|---|---|---|---|---|---|---|---|---|---|"]
        for key, r in out["launches"].items():
            label, form, hw, batch = key.split(" | ")
            lines.append("| %s | %s | %s | %s | %s | %s | %.3f | %.3f | %.2f | %.1f %% | %s |" % (
                label, form, hw, batch.split()[1], fmt_runs(r["parent"]), fmt_runs(r["fused"]), r["parent"]["median_ms"],
                r["fused"]["median_ms"], r["parent_over_fused"], 100 * max(r["parent"]["spread"], r["fused"]["spread"]), r["verdict"]))
        behind = sorted({(k.split(" | ")[1],) + tuple(c for c in LAUNCHES if c[0] == k.split(" | ")[0])[0][2:5]
                         for k, r in out["launches"].items() if r["verdict"] != "ahead"})
        lines += ["", "Shapes (form, Cin, Cout, dilation) that are not ahead at both batch sizes and every map measured: %s." % (behind or "none"),
                  "`pspnet_combine.INFER2H_ROUTING_EXCLUDED` when this was written: %s." % (out["excluded"] or "empty"), "",
                  "Not measured: other image sizes, a counter profile of the new instantiations.", ""]
        with open(args.out_launches, "w") as fh:
            fh.write("\n".join(lines))
    if not args.skip_forwards:
        lines = ["# The student's whole forward: plain, fused on three bf16 pieces, fused on two fp16 pieces, on one MI355X", ""] + head + [
            "Res_pspnet BasicBlock [2, 2, 2, 2], seeded, eval, channels-last.  Interleaved per round: plain, then",
            "`fuse_for_inference(net, narrow=True, stride2=True)`, then the same with `piece_format=\"fp16\"` under the shipped",
            "`INFER2H_ROUTING_EXCLUDED` (%s)%s." % (out["excluded"] or "empty", ", then with the set emptied" if out["excluded"] else ""), "",
            "| input | forward | ms (runs) | median ms | plain / this | three pieces / this | spread | logits: max difference from plain / max |",
            "|---|---|---|---|---|---|---|---|"]
        for name, res in out["forwards"].items():
            for k, r in res.items():
                lines.append("| %s | %s | %s | %.2f | %.3f | %.3f | %.1f %% | %.1e |" % (
                    name, k, fmt_runs(r), r["median_ms"], r["plain_over_this"], r["three_over_this"], 100 * r["spread"],
                    r["logits_max_rel_difference"]))
        lines += ["", "Not measured: other batch sizes or image sizes; the accuracy of the legs against float64 is in",
                  "profiles/r34_infer2h_accuracy.md.", ""]
        with open(args.out_forwards, "w") as fh:
            fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
