"""GPU tool: two pieces against three (include/skd_split2.h), isolated, at the frozen teacher's batch-8 shapes -- the four routed
3x3 shapes and the tail / reduce / down-sample 1x1 shapes.  Three interleaved rounds (three, two, three, two, ...) of
tools/_timing.warm_timed per shape on the same tensors; one JSON line per shape with the three rounds of each leg, the matrix-pipe
share each implies (6 or 3 bf16 products at 2.5 PFLOP/s) and whether the two sets overlap; profiles/r25_split2_isolated.md.
    python tools/split2_bench.py
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("PYTORCH_MIOPEN_SUGGEST_NHWC", "1")
from _timing import warm_timed  # noqa: E402
from structure_knowledge_distillation_amd import _lib, functional as SF  # noqa: E402

B = 8
C3 = [("layer3 conv2", 256, 256, 65, 2, False, 23), ("psp feats half", 2048, 512, 65, 1, False, 1),
      ("layer4 conv2", 512, 512, 65, 4, False, 3), ("dsn head", 1024, 512, 65, 1, True, 1)]
# (what, Cin, Cout, HW, count, residual, prologue)
C1 = [("tail l3", 256, 1024, 65, 23, True, True), ("tail l4", 512, 2048, 65, 3, True, True), ("tail l2", 128, 512, 65, 4, True, True),
      ("tail l1", 64, 256, 129, 3, True, True), ("reduce l3", 1024, 256, 65, 22, False, False), ("reduce l4", 2048, 512, 65, 2, False, False),
      ("reduce l4.0", 1024, 512, 65, 1, False, False), ("reduce l3.0", 512, 256, 65, 1, False, False),
      ("reduce l2.0", 256, 128, 129, 1, False, False), ("down l1.0", 128, 256, 129, 1, False, False),
      ("down l4.0", 1024, 2048, 65, 1, False, False), ("down l3.0", 512, 1024, 65, 1, False, False)]
PEAK = 2.5e15


def ab(fns, flop, tot, count):
    t = {2: [], 3: []}
    for _ in range(3):
        for p in (3, 2):
            t[p].append(warm_timed(fns[p], reps=10, warm_ms=30.0, groups=5))
    row = {}
    for p in (2, 3):
        row["us_%d" % p] = [round(v * 1e3, 1) for v in t[p]]
        row["mfma_share_%d" % p] = round((p * (p + 1) // 2) * flop / PEAK / (min(t[p]) * 1e-3), 3)
    row["speedup_min_over_min"] = round(min(t[3]) / min(t[2]), 3)
    row["sets_overlap"] = not (max(t[2]) < min(t[3]) or max(t[3]) < min(t[2]))
    tot[2] += count * min(t[2])
    tot[3] += count * min(t[3])
    return row


def main():
    _lib.load()
    dev = torch.device("cuda", 0)
    tot = {2: 0.0, 3: 0.0}
    with torch.no_grad():
        for name, cin, cout, hw, d, bias, count in C3:
            torch.manual_seed(cin + cout + d)
            x = torch.relu(torch.randn(B, cin, hw, hw, device=dev)).contiguous(memory_format=torch.channels_last)
            conv = torch.nn.Conv2d(cin, cout, 3, 1, d, d, bias=bias).to(dev).to(memory_format=torch.channels_last).eval()
            pk = {3: SF.conv3x3_pack_weights(conv), 2: SF.conv3x3_pack_weights(conv, pieces=2)}
            fns = {p: (lambda p=p: SF.conv3x3_split_eval(x, pk[p], cout, d, conv.bias, pieces=p)) for p in (2, 3)}
            row = ab(fns, 2.0 * B * hw * hw * 9 * cin * cout, tot, count)
            print(json.dumps(dict(kernel="3x3", shape=name, cin=cin, cout=cout, count=count, **row)), flush=True)
        for name, cin, cout, hw, count, has_res, pro in C1:
            torch.manual_seed(cin + cout)
            x = torch.relu(torch.randn(B, cin, hw, hw, device=dev)).contiguous(memory_format=torch.channels_last)
            res = torch.randn(B, cout, hw, hw, device=dev).contiguous(memory_format=torch.channels_last) if has_res else None
            w = torch.randn(cout, cin, 1, 1, device=dev) * 0.05
            rm, rv = torch.randn(cout, device=dev) * 0.1, torch.rand(cout, device=dev) + 0.5
            ga, be = torch.rand(cout, device=dev) + 0.5, torch.randn(cout, device=dev)
            table = None
            if pro:
                table = torch.stack([torch.randn(cin, device=dev) * 0.1, torch.rand(cin, device=dev) + 0.5, torch.rand(cin, device=dev) + 0.5,
                                     torch.randn(cin, device=dev) * 0.1]).contiguous()
            fns = {p: (lambda p=p: SF.conv1x1_abn_eval(x, w, rm, rv, ga, be, 1e-5, "relu", 0.01, res, table, pieces=p)) for p in (2, 3)}
            row = ab(fns, 2.0 * B * hw * hw * cin * cout, tot, count)
            print(json.dumps(dict(kernel="1x1", shape=name, cin=cin, cout=cout, count=count, **row)), flush=True)
    print(json.dumps({"per_teacher_forward_ms": {"two": round(tot[2], 3), "three": round(tot[3], 3)}}), flush=True)


if __name__ == "__main__":
    main()
