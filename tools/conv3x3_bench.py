"""GPU tool: the frozen teacher's wide 3x3 convolutions at batch 8, isolated -- MIOpen's fp32 ``F.conv2d`` (the shipped find-db)
against the split-core implicit GEMM of csrc/conv3x3.hip in each tile geometry (0 = shipped choice, 1 = 128-pixel tiles,
2 = 64-pixel tiles, 3 = 128 for the whole rounds + 64 for the rest).  HIP events around `reps` back-to-back calls after >= 30 ms
of warm-up launches, three repeats; one JSON line per problem.
    python tools/conv3x3_bench.py [reps] [--pieces {2,3}]     # --pieces 2: the split side on the two-piece core (include/skd_split2.h)
    python tools/conv3x3_bench.py pmc      # two launches of each path per problem and nothing else: for counter-only rocprofv3 --pmc runs
    python tools/conv3x3_bench.py pmc-summary <counter_collection.csv> [...]    # mean counter value per kernel and grid
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("PYTORCH_MIOPEN_SUGGEST_NHWC", "1")
PROBLEMS = [  # (name, Cin, Cout, HW, dilation, bias, launches per teacher forward)
    ("layer3 conv2", 256, 256, 65, 2, False, 23),
    ("psp bottleneck feats half", 2048, 512, 65, 1, False, 1),
    ("layer4 conv2", 512, 512, 65, 4, False, 3),
    ("dsn head", 1024, 512, 65, 1, True, 1),
    ("layer2 conv2 (not routed)", 128, 128, 65, 1, False, 3),
]


def main():
    import torch
    import torch.nn.functional as F
    import structure_knowledge_distillation_amd as _skd
    _skd.configure_miopen()
    from structure_knowledge_distillation_amd import _lib, functional as SF
    _lib.load()
    pieces = 3
    if "--pieces" in sys.argv:
        i = sys.argv.index("--pieces")
        pieces = int(sys.argv[i + 1])
        if pieces not in (2, 3):
            raise SystemExit("--pieces takes 2 or 3")
        del sys.argv[i:i + 2]
    pk = dict(pieces=2) if pieces == 2 else {}
    pmc = len(sys.argv) > 1 and sys.argv[1] == "pmc"
    reps = int(sys.argv[1]) if len(sys.argv) > 1 and not pmc else 20
    dev = torch.device("cuda", 0)
    B = 8

    def warm_up(fn, ms=30.0):
        w0, w1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        spent = 0.0
        for _ in range(400):
            w0.record()
            for _ in range(4):
                fn()
            w1.record()
            w1.synchronize()
            spent += w0.elapsed_time(w1)
            if spent >= ms:
                break

    def timed(fn):
        out = []
        for _ in range(3):
            warm_up(fn)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(round(e0.elapsed_time(e1) / reps * 1e3, 1))
        return out

    total = {"miopen_ms": 0.0, "split_ms": 0.0}
    with torch.no_grad():
        for name, cin, cout, hw, d, bias, count in PROBLEMS:
            torch.manual_seed(cin + cout + d)
            x = torch.relu(torch.randn(B, cin, hw, hw, device=dev)).contiguous(memory_format=torch.channels_last)
            conv = torch.nn.Conv2d(cin, cout, 3, 1, d, d, bias=bias).to(dev).to(memory_format=torch.channels_last).eval()
            flop = 2.0 * B * hw * hw * 9 * cin * cout
            row = {"problem": name, "pieces": pieces, "cin": cin, "cout": cout, "hw": hw, "dilation": d, "count": count, "gflop": round(flop / 1e9, 1)}
            if pmc:
                pack = SF.conv3x3_pack_weights(conv, **pk)
                for _ in range(2):
                    F.conv2d(x, conv.weight, conv.bias, 1, d, d)
                    SF.conv3x3_split_eval(x, pack, cout, d, conv.bias, **pk)
                torch.cuda.synchronize()
                row["algorithmic_mb"] = {"x": round(x.numel() * 4 / 1e6, 1), "w_fp32": round(conv.weight.numel() * 4 / 1e6, 1),
                                         "w_pack": round(conv.weight.numel() * 2 * pieces / 1e6, 1), "y": round(B * hw * hw * cout * 4 / 1e6, 1)}
                print(json.dumps(row), flush=True)
                continue
            row["miopen_us"] = timed(lambda: F.conv2d(x, conv.weight, conv.bias, 1, d, d))
            assert SF.conv3x3_split_supported(x, conv)
            pack = SF.conv3x3_pack_weights(conv, **pk)
            for g in (0, 1, 2, 3):
                row["split_g%d_us" % g] = timed(lambda: SF.conv3x3_split_eval(x, pack, cout, d, conv.bias, geometry=g, **pk))
            want = F.conv2d(x, conv.weight, conv.bias, 1, d, d)
            got = SF.conv3x3_split_eval(x, pack, cout, d, conv.bias, **pk)
            row["max_abs_diff_over_max"] = float((got - want).abs().max() / want.abs().max())
            t_m, t_s = min(row["miopen_us"]), min(row["split_g0_us"])
            row["split_tflops_algorithmic"] = round(flop / t_s / 1e6, 1)
            row["split_frac_of_%s_product_bound" % ("six" if pieces == 3 else "three")] = round(
                pieces * (pieces + 1) // 2 * flop / 2.5e15 / (t_s * 1e-6), 3)
            row["speedup"] = round(t_m / t_s, 3)
            if "not routed" not in name:
                total["miopen_ms"] += count * t_m / 1e3
                total["split_ms"] += count * t_s / 1e3
            print(json.dumps(row), flush=True)
    if pmc:
        return
    print(json.dumps({"per_teacher_forward": {k: round(v, 3) for k, v in total.items()}}), flush=True)


def pmc_summary(paths):
    """Mean Counter_Value per (counter, kernel, grid) over the launches in rocprofv3 counter_collection CSVs."""
    import collections
    import csv
    acc = collections.defaultdict(list)
    for path in paths:
        for r in csv.DictReader(open(path, newline="")):
            n = r["Kernel_Name"]
            if "conv3x3_split_kernel" in n or n.startswith("igemm_fwd"):
                acc[(r.get("Counter_Name", "?"), n.replace("void skd::(anonymous namespace)::", "")[:60], r.get("Grid_Size", "?"))].append(float(r["Counter_Value"]))
    print("| counter | kernel | grid | launches | mean value |\n|---|---|---|---|---|")
    for (c, n, g), v in sorted(acc.items()):
        print("| %s | `%s` | %s | %d | %.0f |" % (c, n, g, len(v), sum(v) / len(v)))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "pmc-summary":
        pmc_summary(sys.argv[2:])
    else:
        main()
