"""GPU tool: the frozen teacher's conv1 -> bn1 -> relu -> conv2 link as bf16 piece planes (route_teacher_planes,
include/skd_planes.h), isolated -- writes the table of profiles/r31_planes_isolated.md.
The four (reduce GEMM, 3x3) pairs a teacher forward has at batch 8 on 65 x 65 maps (a 512 x 512 step): PARENT {reduce GEMM with
fp32 output + 3x3 on the fp32 map} against NEW {reduce GEMM with piece planes out + 3x3 on the planes}, the producer alone, the
consumer alone and the pair back to back (the consumer then finds its input where the producer left it, as in the network).
``tools/_timing.warm_timed`` (>= 30 ms of the same launches as warm-up, then the median of 5 groups of 10 back-to-back launches),
``--rounds`` interleaved rounds parent, new, parent, ...; spread = (max - min) / median of one side's per-round figures, the larger
of the two sides compared.  A pair is routed only where NEW is ahead of PARENT by more than that spread; every other pair belongs
in pspnet_combine.PLANES_ROUTING_EXCLUDED as (conv1 Cin, planes, dilation).
    python tools/conv_planes_bench.py [--rounds 3]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
PAIRS = [  # (name, blocks per forward, conv1 Cin, planes, dilation)
    ("layer3.0    512 -> 256, 3x3 256 -> 256 d2", 1, 512, 256, 2),
    ("layer3.1-22 1024 -> 256, 3x3 256 -> 256 d2", 22, 1024, 256, 2),
    ("layer4.0    1024 -> 512, 3x3 512 -> 512 d4", 1, 1024, 512, 4),
    ("layer4.1-2  2048 -> 512, 3x3 512 -> 512 d4", 2, 2048, 512, 4),
]


def verdict_of(p_runs, n_runs):
    med = statistics.median
    spread = max((max(v) - min(v)) / med(v) for v in (p_runs, n_runs))
    gain = (med(p_runs) - med(n_runs)) / med(p_runs)
    return spread, "ahead" if gain > spread else ("behind" if -gain > spread else "within the spread")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=65)
    a = ap.parse_args()
    import torch
    from structure_knowledge_distillation_amd import functional as SF
    from structure_knowledge_distillation_amd.libs import InPlaceABNSync
    from _timing import warm_timed
    dev = torch.device("cuda", 0)
    med = statistics.median
    fmt = lambda runs: " / ".join("%.1f" % (1e3 * t) for t in runs)
    print("Batch %d, %d x %d maps; microseconds per launch (per pair: both launches); runs in round order." % (a.batch, a.size, a.size))
    print()
    print("| pair | per forward | side | reduce GEMM us (runs) | 3x3 us (runs) | pair us (runs) | reduce | 3x3 | pair |")
    print("|---|---|---|---|---|---|---|---|---|")
    rows, saved = [], 0.0
    with torch.no_grad():
        for name, count, cin, planes, d in PAIRS:
            torch.manual_seed(cin + planes + d)
            x = torch.relu(torch.randn(a.batch, cin, a.size, a.size, device=dev)).contiguous(memory_format=torch.channels_last)
            c1 = torch.nn.Conv2d(cin, planes, 1, bias=False).to(dev).eval()
            c2 = torch.nn.Conv2d(planes, planes, 3, 1, d, d, bias=False).to(dev).to(memory_format=torch.channels_last).eval()
            bn = InPlaceABNSync(planes, activation="none").to(dev).eval()
            bn.running_var.uniform_(0.5, 1.5)
            pack = SF.conv3x3_pack_weights(c2)
            bn_args = (c1.weight, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.eps, "relu")
            reduce, reduce_planes = lambda: SF.conv1x1_abn_eval(x, *bn_args), lambda: SF.conv1x1_abn_planes_eval(x, *bn_args)
            fp32, pl = reduce(), reduce_planes()
            assert torch.equal(SF.conv3x3_split_eval(pl, pack, planes, d), SF.conv3x3_split_eval(fp32, pack, planes, d))
            sides = {
                ("parent", "reduce"): lambda: reduce(),
                ("parent", "3x3"): lambda: SF.conv3x3_split_eval(fp32, pack, planes, d),
                ("parent", "pair"): lambda: SF.conv3x3_split_eval(reduce(), pack, planes, d),
                ("new", "reduce"): lambda: reduce_planes(),
                ("new", "3x3"): lambda: SF.conv3x3_split_eval(pl, pack, planes, d),
                ("new", "pair"): lambda: SF.conv3x3_split_eval(reduce_planes(), pack, planes, d),
            }
            runs = {k: [] for k in sides}
            for _ in range(a.rounds):
                for what in ("reduce", "3x3", "pair"):
                    for side in ("parent", "new"):
                        runs[(side, what)].append(warm_timed(sides[(side, what)]))
            for side in ("parent", "new"):
                print("| %s | %d | %s | %s | %s | %s | %.1f | %.1f | %.1f |" % (
                    name, count, side, fmt(runs[(side, "reduce")]), fmt(runs[(side, "3x3")]), fmt(runs[(side, "pair")]),
                    1e3 * med(runs[(side, "reduce")]), 1e3 * med(runs[(side, "3x3")]), 1e3 * med(runs[(side, "pair")])), flush=True)
            cells = []
            for what in ("reduce", "3x3", "pair"):
                spread, verdict = verdict_of(runs[("parent", what)], runs[("new", what)])
                cells.append("%s parent / new %.3f, spread %.1f %%, %s" % (what, med(runs[("parent", what)]) / med(runs[("new", what)]),
                                                                         100 * spread, verdict))
            rows.append((name, count, (cin, planes, d), cells, verdict))
            if verdict == "ahead":
                saved += count * (med(runs[("parent", "pair")]) - med(runs[("new", "pair")]))
            del x, fp32, pl
    print()
    for name, count, key, cells, verdict in rows:
        print("* %s (x %d), %r: %s -> %s" % (name, count, key, "; ".join(cells), "ROUTED" if verdict == "ahead" else "EXCLUDED"))
    print()
    print("PLANES_ROUTING_EXCLUDED = %r" % (sorted(key for _, _, key, _, verdict in rows if verdict != "ahead"),))
    print("Per teacher forward, routed pairs x their counts: %.3f ms saved." % saved)


if __name__ == "__main__":
    main()
