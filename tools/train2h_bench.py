"""Times the student's wide training convolutions on two FP16 pieces with a device-side gradient scale
(route_training_convs(pieces=2, piece_format="fp16"), include/skd_train2h.h) against the same convolutions on three bf16 pieces,
with the bf16 two-piece form (include/skd_train2.h) as a third column, on one MI355X, in one process: tools/_timing.warm_timed in
front of every figure (>= 30 ms of the same launches as warm-up, then the median of 5 groups of 10 back-to-back launches),
``--rounds`` interleaved rounds three, fp16, two, three, fp16, two, ...; spread = (max - min) / median of one side's per-round
sums, the largest of the sides; a shape is *ahead* when three / fp16 exceeds 1 + spread.  Every launch is the C-ABI entry on
pre-allocated buffers.

Per shape, the seven the routing puts on the split core, at ``--batch`` x ``--hw`` x ``--hw``:
  forward + data gradient + pack pair (+ the scale word of g, fp16 alone), and the weight gradient (both its launches) on the plan's
  slice count.  The scale word's own time is listed separately.  A shape that is not ahead in both groups belongs in
  pspnet_combine.STUDENT_FP16_ROUTING_EXCLUDED.

    python tools/train2h_bench.py [--rounds 3] [--batch 8] [--hw 65] [--out FILE]

Prints one JSON line and writes the tables (default profiles/r35_student_fp16_isolated.md).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from conv3x3_train_bench import PROBLEMS  # noqa: E402

SIDES = ("three", "fp16", "two")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--hw", type=int, default=65)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r35_student_fp16_isolated.md"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("train2h_bench needs an MI355X: there is no CPU timing")
    import structure_knowledge_distillation_amd as _skd
    _skd.configure_miopen()
    from structure_knowledge_distillation_amd import _lib, functional as SF
    from structure_knowledge_distillation_amd.networks import pspnet_combine as PC
    from _timing import warm_timed
    if not SF.train2h_supported():
        raise SystemExit("this back-end lacks the entries of include/skd_train2h.h")
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    B, hw = a.batch, a.hw
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    med = statistics.median
    out = {"rounds": a.rounds, "batch": B, "hw": hw, "cus": cus, "shapes": {}, "excluded": sorted(PC.STUDENT_FP16_ROUTING_EXCLUDED)}
    P = lambda t: None if t is None else t.data_ptr()
    with torch.no_grad():
        for name, cin, cout, d, bias, count in PROBLEMS:
            torch.manual_seed(cin + cout + d)
            x = torch.relu(torch.randn(B, cin, hw, hw, device=dev)).contiguous(memory_format=torch.channels_last)
            g = (torch.randn(B, cout, hw, hw, device=dev) * 1e-5).contiguous(memory_format=torch.channels_last)
            conv = torch.nn.Conv2d(cin, cout, 3, 1, d, d, bias=bias).to(dev).to(memory_format=torch.channels_last)
            w, bs = conv.weight.detach(), None if conv.bias is None else conv.bias.detach()
            st = _lib.stream_of(x)
            packs = {"three": SF.conv3x3_train_packs(w), "fp16": SF.conv3x3_train_packs_fp16(w), "two": SF.conv3x3_train_packs2(w)}
            y = torch.empty((B, cout, hw, hw), device=dev).contiguous(memory_format=torch.channels_last)
            dx = torch.empty((B, cin, hw, hw), device=dev).contiguous(memory_format=torch.channels_last)
            dw = torch.empty_like(w)
            word = SF.fp16_scale_word(g)
            wws = torch.empty(int(lib.skd_fp16_scale_word_workspace_bytes(g.numel())), dtype=torch.uint8, device=dev)
            plan = (ctypes.c_int64 * 3)()
            assert lib.skd_conv3x3_split2h_wgrad_plan(B, hw, hw, cin, cout, 0, cus, ctypes.cast(plan, ctypes.c_void_p)) == 1
            used, per_slice, nbytes = int(plan[0]), int(plan[1]), int(plan[2])
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            run = {"three": lib.skd_conv3x3_split_nhwc, "fp16": lib.skd_conv3x3_split2h_nhwc, "two": lib.skd_conv3x3_split2_nhwc}
            pair = {"three": lib.skd_conv3x3_split_pack_pair, "fp16": lib.skd_conv3x3_split2h_pack_pair, "two": lib.skd_conv3x3_split2_pack_pair}
            wgr = {"three": lib.skd_conv3x3_split_wgrad_nhwc, "two": lib.skd_conv3x3_split2_wgrad_nhwc}
            sn, sc, sy, sx = w.stride()

            def fwd(side):
                return lambda: run[side](B, hw, hw, cin, cout, d, P(x), P(packs[side][0]), P(y), P(bs), None, None, None, None, 0.0, 0, 0.01,
                                         0, st)

            def dgrad(side):
                if side == "fp16":
                    return lambda: lib.skd_conv3x3_split2h_scaled_nhwc(B, hw, hw, cout, cin, d, P(g), P(packs[side][1]), P(dx), P(word), 0, st)
                return lambda: run[side](B, hw, hw, cout, cin, d, P(g), P(packs[side][1]), P(dx), None, None, None, None, None, 0.0, 0, 0.01,
                                         0, st)

            def pack(side):
                pf, pb = packs[side]
                return lambda: pair[side](cin, cout, P(w), sn, sc, sy, sx, P(pf), pf.numel(), P(pb), pb.numel(), st)

            def wgrad(side):
                if side == "fp16":
                    return lambda: lib.skd_conv3x3_split2h_wgrad_nhwc(B, hw, hw, cin, cout, d, P(x), P(g), P(dw), *dw.stride(), P(ws), nbytes,
                                                                      P(word), used, st)
                return lambda: wgr[side](B, hw, hw, cin, cout, d, P(x), P(g), P(dw), *dw.stride(), P(ws), nbytes, used, st)

            scale = lambda: lib.skd_fp16_scale_word(g.numel(), P(g), P(wws), wws.numel(), P(word), st)
            for fn in [f(s) for f in (fwd, dgrad, pack, wgrad) for s in SIDES] + [scale]:
                assert fn() == 1
            runs = {(k, s): [] for k in ("fwd", "dgrad", "pack", "wgrad") for s in SIDES}
            runs[("word", "fp16")] = []
            for _ in range(a.rounds):
                for k, f in (("fwd", fwd), ("dgrad", dgrad), ("pack", pack)):
                    for s in SIDES:
                        runs[(k, s)].append(warm_timed(f(s)))
                runs[("word", "fp16")].append(warm_timed(scale))
                for s in SIDES:
                    runs[("wgrad", s)].append(warm_timed(wgrad(s)))
            group1 = {s: [f + b + p + (wd if s == "fp16" else 0.0) for f, b, p, wd in
                          zip(runs[("fwd", s)], runs[("dgrad", s)], runs[("pack", s)], runs[("word", "fp16")])] for s in SIDES}
            res = {"count": count, "slices": used, "per_slice": per_slice,
                   "runs_us": {"%s %s" % k: [1e3 * t for t in v] for k, v in runs.items()}}
            for label, sums in (("fwd+dgrad+pack+word", group1), ("wgrad", {s: runs[("wgrad", s)] for s in SIDES})):
                m = {s: med(v) for s, v in sums.items()}
                spread = max((max(v) - min(v)) / med(v) for v in sums.values())
                ratio = m["three"] / m["fp16"]
                res[label] = {"median_us": {s: 1e3 * t for s, t in m.items()}, "three_over_fp16": ratio, "three_over_two": m["three"] / m["two"],
                              "spread": spread, "verdict": "ahead" if ratio > 1 + spread else ("behind" if ratio < 1 - spread else "within the spread")}
            out["shapes"][name] = res
            print(name, json.dumps(res), flush=True)
    print(json.dumps(out))

    fmt = lambda v: " / ".join("%.1f" % t for t in v)
    lines = ["# The student's wide training convolutions on two fp16 pieces against three bf16 pieces, isolated, on one MI355X", "",
             "Written by `python tools/train2h_bench.py --rounds %d --batch %d --hw %d` (%d compute units; one process;" % (a.rounds, B, hw, cus),
             "`tools/_timing.warm_timed`: >= 30 ms of the same launches as warm-up, then the median of 5 groups of 10 back-to-back launches;",
             "%d interleaved rounds three, fp16, two, ...; every launch is the C-ABI entry on pre-allocated buffers).  **three**: three bf16" % a.rounds,
             "pieces, six products (the parent's launches); **fp16**: two fp16 pieces with the scale word (include/skd_train2h.h); **two**: two",
             "bf16 pieces (include/skd_train2.h, the accuracy trade: the ceiling).  Spread = (max - min) / median of one side's per-round sums,",
             "the largest of the three sides; **ahead**: three / fp16 > 1 + spread.  g is Gaussian x 1e-5.", "",
             "## Forward + data gradient + pack pair (+ scale word, fp16 alone)", "",
             "| convolution | per step | fwd three / fp16 / two us | dgrad three / fp16 / two us | pack three / fp16 / two us | word us (runs) "
             "| sum three | sum fp16 | sum two | three / fp16 | three / two | spread | verdict |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    tot = {k: {s: 0.0 for s in SIDES} for k in ("fwd+dgrad+pack+word", "wgrad")}
    word_total = 0.0
    for name, r in out["shapes"].items():
        ru, g1 = r["runs_us"], r["fwd+dgrad+pack+word"]
        trio = lambda k: " / ".join("%.1f" % med(ru["%s %s" % (k, s)]) for s in SIDES)
        lines.append("| %s | %d | %s | %s | %s | %s | %.1f | %.1f | %.1f | %.2f | %.2f | %.1f %% | %s |" % (
            name, r["count"], trio("fwd"), trio("dgrad"), trio("pack"), fmt(ru["word fp16"]), g1["median_us"]["three"], g1["median_us"]["fp16"],
            g1["median_us"]["two"], g1["three_over_fp16"], g1["three_over_two"], 100 * g1["spread"], g1["verdict"]))
        word_total += r["count"] * med(ru["word fp16"])
        for k in tot:
            for s in SIDES:
                tot[k][s] += r["count"] * r[k]["median_us"][s]
    lines += ["", "Per student step (the counts above): three %.2f ms, fp16 %.2f ms, two %.2f ms; the scale words alone %.3f ms of the fp16 figure."
              % (tot["fwd+dgrad+pack+word"]["three"] / 1e3, tot["fwd+dgrad+pack+word"]["fp16"] / 1e3, tot["fwd+dgrad+pack+word"]["two"] / 1e3,
                 word_total / 1e3), "",
              "## Weight gradient (both launches, the plan's slice count)", "",
              "| convolution | per step | slices (K-tiles each) | three us (runs) | fp16 us (runs) | two us (runs) | three / fp16 | three / two | spread | verdict |",
              "|---|---|---|---|---|---|---|---|---|---|"]
    for name, r in out["shapes"].items():
        ru, wg = r["runs_us"], r["wgrad"]
        lines.append("| %s | %d | %d (%d) | %s | %s | %s | %.2f | %.2f | %.1f %% | %s |" % (
            name, r["count"], r["slices"], r["per_slice"], fmt(ru["wgrad three"]), fmt(ru["wgrad fp16"]), fmt(ru["wgrad two"]),
            wg["three_over_fp16"], wg["three_over_two"], 100 * wg["spread"], wg["verdict"]))
    behind = sorted(n for n, r in out["shapes"].items() if r["fwd+dgrad+pack+word"]["verdict"] != "ahead" or r["wgrad"]["verdict"] != "ahead")
    lines += ["", "Per student step (the counts above): three %.2f ms, fp16 %.2f ms, two %.2f ms."
              % tuple(tot["wgrad"][s] / 1e3 for s in SIDES), "",
              "Shapes that are not ahead of three pieces in both groups: %s.  `pspnet_combine.STUDENT_FP16_ROUTING_EXCLUDED` when this was"
              % (", ".join(behind) or "none"), "written: %s." % (out["excluded"] or "empty"), "",
              "Not measured: other batch or map sizes, slice counts other than the plan's, a counter profile of the new instantiations.", ""]
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
