"""GPU tool: the frozen teacher's nine early 3x3 convolutions (route_teacher_early) and the student's stride-2 one
(fuse_for_inference(stride2=True)), isolated -- writes the tables of profiles/r27_conv3x3_early_isolated.md.
Teacher (batch 8, the shapes of a 512 x 512 step): the library convolution each shape takes today -- for the stem's conv2 plus the
eval-mode ABN pass the split-core launch absorbs -- against ONE launch of the split core with three and with two pieces: the
64-column form (three pieces only) for Cout = 64, the wide kernel for the stem's conv3 and layer2's stride-1 conv2, the stride-2
form (include/skd_stride2.h) for layer2.0's conv2.  Student (batch 1, the shapes of a 1024 x 2048 forward): layer2.0's conv1
(64 -> 128, stride 2) followed by the eval-mode ABN pass against one launch of the stride-2 form with BN + ReLU in the epilogue.
``tools/_timing.warm_timed`` (>= 30 ms of the same launches as warm-up, then the median of 5 groups of 10 back-to-back launches),
``--rounds`` interleaved rounds library, three pieces, two pieces, library, ...; spread = (max - min) / median of one side's
per-round figures, the larger of the two sides compared.  A shape is routed only where it is ahead by more than the spread.
    python tools/conv3x3_early_bench.py [--rounds 3]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("PYTORCH_MIOPEN_SUGGEST_NHWC", "1")
TEACHER = [  # (name, calls per forward, H = W of the input, Cin, Cout, stride, BN + ReLU epilogue)
    ("stem conv2 64->64 256x256 bn+relu (64-column form)", 1, 256, 64, 64, 1, True),
    ("stem conv3 64->128 256x256 raw (wide kernel)", 1, 256, 64, 128, 1, False),
    ("layer1 conv2 64->64 129x129 raw (64-column form)", 3, 129, 64, 64, 1, False),
    ("layer2.0 conv2 128->128 stride 2 129x129 -> 65x65 raw (stride-2 form)", 1, 129, 128, 128, 2, False),
    ("layer2 conv2 128->128 65x65 raw (wide kernel)", 3, 65, 128, 128, 1, False),
]
STUDENT = [("student layer2.0 conv1 64->128 stride 2 257x513 -> 129x257 bn+relu (stride-2 form)", 1, (257, 513), 64, 128, 2, True)]


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
    import structure_knowledge_distillation_amd as _skd
    _skd.configure_miopen()
    from structure_knowledge_distillation_amd import functional as SF
    from structure_knowledge_distillation_amd.libs import InPlaceABNSync
    from structure_knowledge_distillation_amd.libs.inplace_abn import abn_eval_fused
    from _timing import warm_timed
    dev = torch.device("cuda", 0)
    med = statistics.median
    fmt = lambda runs: " / ".join("%.1f" % (1e3 * t) for t in runs) if runs else "-"
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)

    totals = {"p": 0.0, "3": 0.0, "2": 0.0}
    for title, batch, table in (("Teacher, batch %d" % a.batch, a.batch, TEACHER), ("Student inference, batch 1", 1, STUDENT)):
        print(title)
        print()
        print("| convolution | per forward | library conv us (runs) | library ABN pass us (runs) | three pieces us (runs) | two pieces us (runs) "
              "| library | three | two | library / three | spread | verdict | library / two | spread | verdict |")
        print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
        with torch.no_grad():
            for name, count, hw, cin, cout, stride, epi in table:
                h, w = hw if isinstance(hw, tuple) else (hw, hw)
                torch.manual_seed(h + cin + cout + stride)
                x = cl(torch.relu(torch.randn(batch, cin, h, w, device=dev)))
                conv = torch.nn.Conv2d(cin, cout, 3, stride, 1, bias=False).to(dev).to(memory_format=torch.channels_last).eval()
                bn = InPlaceABNSync(cout, activation="none").to(dev).eval()
                bn.running_var.uniform_(0.5, 1.5)
                y = conv(x)
                args = (bn, "relu") if epi else (None, "none")
                sides = {"pc": lambda: conv(x)}
                if epi:     # in place on the convolution's output, as forward_relu runs it: the values drift, the time does not
                    sides["pa"] = lambda: abn_eval_fused(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, "relu", 0.01, None)
                if cout % 128:
                    pack = SF.conv3x3_narrow_pack_weights(conv)
                    sides["3"] = lambda: SF.conv3x3_narrow_eval(x, pack, cout, 1, None, None, *args)
                elif stride == 2:
                    pack, pack2 = SF.conv3x3_pack_weights(conv), SF.conv3x3_pack_weights(conv, pieces=2)
                    sides["3"] = lambda: SF.conv3x3_s2_eval(x, pack, cout, None, *args)
                    sides["2"] = lambda: SF.conv3x3_s2_eval(x, pack2, cout, None, *args, pieces=2)
                else:
                    pack, pack2 = SF.conv3x3_pack_weights(conv), SF.conv3x3_pack_weights(conv, pieces=2)
                    sides["3"] = lambda: SF.conv3x3_split_eval(x, pack, cout, 1, None, *args)
                    sides["2"] = lambda: SF.conv3x3_split_eval(x, pack2, cout, 1, None, *args, pieces=2)
                runs = {k: [] for k in ("pc", "pa", "3", "2")}
                for _ in range(a.rounds):
                    for k in sides:
                        runs[k].append(warm_timed(sides[k]))
                p_runs = [c + (runs["pa"][i] if epi else 0.0) for i, c in enumerate(runs["pc"])]
                cells = []
                for k in ("3", "2"):
                    if runs[k]:
                        spread, verdict = verdict_of(p_runs, runs[k])
                        cells += ["%.2f" % (med(p_runs) / med(runs[k])), "%.1f %%" % (100 * spread), verdict]
                    else:
                        cells += ["-", "-", "three pieces only"]
                print("| %s | %d | %s | %s | %s | %s | %.1f | %.1f | %s | %s |" % (
                    name, count, fmt(runs["pc"]), fmt(runs["pa"]), fmt(runs["3"]), fmt(runs["2"]), 1e3 * med(p_runs), 1e3 * med(runs["3"]),
                    "%.1f" % (1e3 * med(runs["2"])) if runs["2"] else "-", " | ".join(cells)), flush=True)
                if table is TEACHER:
                    totals["p"] += count * med(p_runs)
                    totals["3"] += count * med(runs["3"])
                    totals["2"] += count * med(runs["2"] or runs["3"])
                del x, y
        print()
    print("Per teacher forward (the counts above): library %.3f ms, three pieces %.3f ms, two pieces (64-column calls on three) %.3f ms."
          % (totals["p"], totals["3"], totals["2"]))


if __name__ == "__main__":
    main()
