"""GPU tool: the training student's routed 3x3 convolutions at batch 8, 65 x 65, isolated -- writes the table of
profiles/r18_conv3x3_train_isolated.md.  Per shape: the forward (MIOpen's fp32 ``F.conv2d`` against one launch of the split core),
the data gradient (``aten.convolution_backward`` input-only against one launch of the split core on ``pack_bwd``) and the
``skd_conv3x3_split_pack_pair`` launch alone, which the training form pays once per step and weight.  ``tools/_timing.warm_timed``
(>= 30 ms of the same launches as warm-up, then the median of 5 groups of 10 back-to-back launches), ``--rounds`` interleaved
rounds parent, split, parent, split, ...; spread = (max - min) / median of one side's per-round sums (forward + data gradient
[+ pack]), the larger of the two sides.
``--pieces 2``: the table of profiles/r33_student_pieces_isolated.md instead -- the "parent" side is the THREE-piece split core
(forward + data gradient + its pack pair), the other side the two-piece form of include/skd_train2.h (skd_conv3x3_split2_nhwc in
both directions + skd_conv3x3_split2_pack_pair); the library is not timed.
    python tools/conv3x3_train_bench.py [--rounds 3] [--pieces 2]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("PYTORCH_MIOPEN_SUGGEST_NHWC", "1")
PROBLEMS = [  # (name, Cin, Cout, dilation, bias, convolutions of this shape per student step)
    ("layer2 128->128 d1", 128, 128, 1, False, 3),
    ("layer3.0.conv1 128->256 d2", 128, 256, 2, False, 1),
    ("layer3 256->256 d2", 256, 256, 2, False, 3),
    ("layer4.0.conv1 256->512 d4", 256, 512, 4, False, 1),
    ("layer4 512->512 d4", 512, 512, 4, False, 3),
    ("dsn[0] 256->128 d1 + bias", 256, 128, 1, True, 1),
    ("psp half 512->128 d1", 512, 128, 1, False, 1),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--hw", type=int, default=65)
    ap.add_argument("--pieces", type=int, default=3, choices=(2, 3))
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    import structure_knowledge_distillation_amd as _skd
    _skd.configure_miopen()
    from structure_knowledge_distillation_amd import _lib, functional as SF
    from _timing import warm_timed
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    B, hw = a.batch, a.hw
    med = statistics.median
    fmt = lambda runs: " / ".join("%.1f" % (1e3 * t) for t in runs)
    two = a.pieces == 2
    if two:
        print("| convolution | per step | fwd three us (runs) | fwd two us (runs) | dgrad three us (runs) | dgrad two us (runs) "
              "| pack three us (runs) | pack two us (runs) | three fwd + dgrad + pack | two fwd + dgrad + pack | three / two | spread | verdict |")
        print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    else:
        print("| convolution | per step | fwd parent us (runs) | fwd split us (runs) | dgrad parent us (runs) | dgrad split us (runs) "
              "| pack us (runs) | parent fwd + dgrad | split fwd + dgrad + pack | parent / split | spread | verdict |")
        print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    total_p = total_s = 0.0
    with torch.no_grad():
        for name, cin, cout, d, bias, count in PROBLEMS:
            torch.manual_seed(cin + cout + d)
            x = torch.relu(torch.randn(B, cin, hw, hw, device=dev)).contiguous(memory_format=torch.channels_last)
            g = torch.randn(B, cout, hw, hw, device=dev).contiguous(memory_format=torch.channels_last)
            conv = torch.nn.Conv2d(cin, cout, 3, 1, d, d, bias=bias).to(dev).to(memory_format=torch.channels_last)
            w, bs = conv.weight.detach(), None if conv.bias is None else conv.bias.detach()
            pf, pb = SF.conv3x3_train_packs(w)
            nbytes, (sn, sc, sy, sx), st = pf.numel(), w.stride(), _lib.stream_of(x)
            sides = {
                "fp": lambda: F.conv2d(x, w, bs, 1, d, d),
                "fs": lambda: SF._conv3x3_raw_launch(SF._WIDE3, x, pf, cout, d, bs),
                "bp": lambda: torch.ops.aten.convolution_backward(g, x, w, None, [1, 1], [d, d], [d, d], False, [0, 0], 1,
                                                                  (True, False, False)),
                "bs": lambda: SF._conv3x3_raw_launch(SF._WIDE3, g, pb, cin, d),
                "pk": lambda: lib.skd_conv3x3_split_pack_pair(cin, cout, w.data_ptr(), sn, sc, sy, sx, pf.data_ptr(), nbytes,
                                                              pb.data_ptr(), nbytes, st),
            }
            if two:
                # three pieces take the parent's place, pack pair included; two pieces the other side
                pf2, pb2 = SF.conv3x3_train_packs2(w)
                n2 = pf2.numel()
                sides = {
                    "fp": sides["fs"], "bp": sides["bs"], "pp": sides["pk"],
                    "fs": lambda: SF._conv3x3_raw_launch(SF._WIDE2, x, pf2, cout, d, bs),
                    "bs": lambda: SF._conv3x3_raw_launch(SF._WIDE2, g, pb2, cin, d),
                    "pk": lambda: lib.skd_conv3x3_split2_pack_pair(cin, cout, w.data_ptr(), sn, sc, sy, sx, pf2.data_ptr(), n2,
                                                                   pb2.data_ptr(), n2, st),
                }
            runs = {k: [] for k in sides}
            for _ in range(a.rounds):
                for k in (("fp", "fs", "bp", "bs", "pp", "pk") if two else ("fp", "fs", "bp", "bs", "pk")):
                    runs[k].append(warm_timed(sides[k]))
            m = {k: med(v) for k, v in runs.items()}
            if two:
                p_runs = [f + b + k for f, b, k in zip(runs["fp"], runs["bp"], runs["pp"])]
                s_runs = [f + b + k for f, b, k in zip(runs["fs"], runs["bs"], runs["pk"])]
                spread = max((max(v) - min(v)) / med(v) for v in (p_runs, s_runs))
                parent, split = m["fp"] + m["bp"] + m["pp"], m["fs"] + m["bs"] + m["pk"]
                gain = (parent - split) / parent
                verdict = "ahead" if gain > spread else ("behind" if -gain > spread else "within the spread")
                total_p += count * parent
                total_s += count * split
                print("| %s | %d | %s | %s | %s | %s | %s | %s | %.1f | %.1f | %.2f | %.1f %% | %s |" % (
                    name, count, fmt(runs["fp"]), fmt(runs["fs"]), fmt(runs["bp"]), fmt(runs["bs"]), fmt(runs["pp"]), fmt(runs["pk"]),
                    1e3 * parent, 1e3 * split, parent / split, 100 * spread, verdict), flush=True)
                continue
            # the two sides of the verdict, per round: what one convolution costs the step in each form
            p_runs = [f + b for f, b in zip(runs["fp"], runs["bp"])]
            s_runs = [f + b + k for f, b, k in zip(runs["fs"], runs["bs"], runs["pk"])]
            spread = max((max(v) - min(v)) / med(v) for v in (p_runs, s_runs))
            parent, split = m["fp"] + m["bp"], m["fs"] + m["bs"] + m["pk"]
            gain = (parent - split) / parent
            verdict = "ahead" if gain > spread else ("behind" if -gain > spread else "within the spread")
            total_p += count * parent
            total_s += count * split
            print("| %s | %d | %s | %s | %s | %s | %s | %.1f | %.1f | %.2f | %.1f %% | %s |" % (
                name, count, fmt(runs["fp"]), fmt(runs["fs"]), fmt(runs["bp"]), fmt(runs["bs"]), fmt(runs["pk"]),
                1e3 * parent, 1e3 * split, parent / split, 100 * spread, verdict), flush=True)
    print()
    print("Per student step (the counts above, forward + data gradient [+ pack]): %s %.2f ms, %s %.2f ms, difference %.2f ms."
          % ("three pieces" if two else "parent", total_p, "two pieces" if two else "split", total_s, total_p - total_s))


if __name__ == "__main__":
    main()
