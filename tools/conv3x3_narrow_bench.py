"""GPU tool: the student's 64-channel 3x3 convolutions, isolated -- writes the tables of profiles/r21_conv3x3_narrow_isolated.md.
Inference (batch 1, the shapes of a 1024 x 2048 forward): the MIOpen convolution followed by the library's eval-mode ABN pass (with
the residual where the block has one) against ONE launch of the split core with that epilogue -- csrc/conv3x3.hip's 64-column form for
Cout = 64, the existing kernel for the stem's conv3 (64 -> 128, raw).  Training (batch 8, the shapes of a 512 x 512 step): the
forward (``F.conv2d``) and the data gradient (``aten.convolution_backward``, input only) against one launch each of the entry
that direction's N chooses, plus the pack launches the training form pays once per step and weight.
``tools/_timing.warm_timed`` (>= 30 ms of the same launches as warm-up, then the median of 5 groups of 10 back-to-back launches),
``--rounds`` interleaved rounds parent, new, parent, new, ...; spread = (max - min) / median of one side's per-round sums, the
larger of the two sides.  A shape is routed only where it is ahead by more than the spread.
    python tools/conv3x3_narrow_bench.py [--rounds 3]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("PYTORCH_MIOPEN_SUGGEST_NHWC", "1")
INFER = [  # (name, H, W, Cin, Cout, residual, BN + ReLU epilogue)
    ("layer1.0 conv1 128->64 257x513 bn+relu", 257, 513, 128, 64, False, True),
    ("layer1 conv1 64->64 257x513 bn+relu", 257, 513, 64, 64, False, True),
    ("layer1 conv2 64->64 257x513 bn+res+relu", 257, 513, 64, 64, True, True),
    ("stem conv2 64->64 512x1024 bn+relu", 512, 1024, 64, 64, False, True),
    ("stem conv3 64->128 512x1024 raw (wide kernel)", 512, 1024, 64, 128, False, False),
]
TRAIN = [  # (name, H = W, Cin, Cout, convolutions of this shape per student step)
    ("stem conv2 64->64 256x256", 256, 64, 64, 1),
    ("layer1.0.conv1 128->64 129x129 (fwd narrow, dgrad wide)", 129, 128, 64, 1),
    ("layer1 64->64 129x129", 129, 64, 64, 3),
    ("stem conv3 64->128 256x256 (fwd wide, dgrad narrow)", 256, 64, 128, 1),
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
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    import structure_knowledge_distillation_amd as _skd
    _skd.configure_miopen()
    from structure_knowledge_distillation_amd import functional as SF
    from structure_knowledge_distillation_amd.libs import InPlaceABNSync
    from structure_knowledge_distillation_amd.libs.inplace_abn import abn_eval_fused
    from _timing import warm_timed
    dev = torch.device("cuda", 0)
    med = statistics.median
    fmt = lambda runs: " / ".join("%.1f" % (1e3 * t) for t in runs)
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)

    print("Inference, batch 1")
    print()
    print("| convolution | parent conv us (runs) | parent ABN pass us (runs) | one launch us (runs) | parent | new | parent / new | spread | verdict |")
    print("|---|---|---|---|---|---|---|---|---|")
    with torch.no_grad():
        for name, h, w, cin, cout, res, epi in INFER:
            torch.manual_seed(h + cin + cout)
            x = cl(torch.relu(torch.randn(1, cin, h, w, device=dev)))
            conv = torch.nn.Conv2d(cin, cout, 3, 1, 1, bias=False).to(dev).to(memory_format=torch.channels_last).eval()
            bn = InPlaceABNSync(cout, activation="none").to(dev).eval()
            bn.running_var.uniform_(0.5, 1.5)
            r = cl(torch.randn(1, cout, h, w, device=dev)) if res else None
            y = conv(x)
            if cout % 128:
                pack = SF.conv3x3_narrow_pack_weights(conv)
                new = lambda: SF.conv3x3_narrow_eval(x, pack, cout, 1, r, None, bn if epi else None, "relu" if epi else "none")
            else:
                pack = SF.conv3x3_pack_weights(conv)
                new = lambda: SF.conv3x3_split_eval(x, pack, cout, 1, None, bn if epi else None, "relu" if epi else "none")
            sides = {"pc": lambda: conv(x), "new": new}
            if epi:         # in place on the convolution's output, as forward_relu runs it: the values drift, the time does not
                sides["pa"] = lambda: abn_eval_fused(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, "relu", 0.01, r)
            runs = {k: [] for k in sides}
            for _ in range(a.rounds):
                for k in sides:
                    runs[k].append(warm_timed(sides[k]))
            p_runs = [c + (runs["pa"][i] if epi else 0.0) for i, c in enumerate(runs["pc"])]
            spread, verdict = verdict_of(p_runs, runs["new"])
            print("| %s | %s | %s | %s | %.1f | %.1f | %.2f | %.1f %% | %s |" % (
                name, fmt(runs["pc"]), fmt(runs["pa"]) if epi else "-", fmt(runs["new"]), 1e3 * med(p_runs), 1e3 * med(runs["new"]),
                med(p_runs) / med(runs["new"]), 100 * spread, verdict), flush=True)
            del x, y, r

    print()
    print("Training, batch %d" % a.batch)
    print()
    print("| convolution | per step | fwd parent us (runs) | fwd new us (runs) | dgrad parent us (runs) | dgrad new us (runs) "
          "| packs us (runs) | parent fwd + dgrad | new fwd + dgrad + packs | parent / new | spread | verdict |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    total_p = total_n = 0.0
    with torch.no_grad():
        for name, hw, cin, cout, count in TRAIN:
            torch.manual_seed(hw + cin + cout)
            x = cl(torch.relu(torch.randn(a.batch, cin, hw, hw, device=dev)))
            g = cl(torch.randn(a.batch, cout, hw, hw, device=dev))
            w = torch.nn.Conv2d(cin, cout, 3, 1, 1, bias=False).to(dev).to(memory_format=torch.channels_last).weight.detach()
            pf, pb, fwd_form, bwd_form = SF._conv3x3_narrow_train_packs(w, None)
            sides = {
                "fp": lambda: F.conv2d(x, w, None, 1, 1, 1),
                "fn": lambda: SF._conv3x3_raw_launch(fwd_form, x, pf, cout, 1),
                "bp": lambda: torch.ops.aten.convolution_backward(g, x, w, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1,
                                                                  (True, False, False)),
                "bn": lambda: SF._conv3x3_raw_launch(bwd_form, g, pb, cin, 1),
                "pk": lambda: SF._conv3x3_narrow_train_packs(w, None),        # no owner: no cache, every call packs
            }
            runs = {k: [] for k in sides}
            for _ in range(a.rounds):
                for k in ("fp", "fn", "bp", "bn", "pk"):
                    runs[k].append(warm_timed(sides[k]))
            p_runs = [f + b for f, b in zip(runs["fp"], runs["bp"])]
            n_runs = [f + b + k for f, b, k in zip(runs["fn"], runs["bn"], runs["pk"])]
            spread, verdict = verdict_of(p_runs, n_runs)
            total_p += count * med(p_runs)
            total_n += count * med(n_runs)
            print("| %s | %d | %s | %s | %s | %s | %s | %.1f | %.1f | %.2f | %.1f %% | %s |" % (
                name, count, fmt(runs["fp"]), fmt(runs["fn"]), fmt(runs["bp"]), fmt(runs["bn"]), fmt(runs["pk"]),
                1e3 * med(p_runs), 1e3 * med(n_runs), med(p_runs) / med(n_runs), 100 * spread, verdict), flush=True)
            del x, g
    print()
    print("Per student step (the counts above, forward + data gradient [+ packs]): parent %.2f ms, new %.2f ms, difference %.2f ms."
          % (total_p, total_n, total_p - total_n))


if __name__ == "__main__":
    main()
