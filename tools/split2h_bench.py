"""GPU tool: two fp16 pieces with a scaled residual (include/skd_split2h.h) against three bf16 pieces and against two bf16
pieces (include/skd_split2.h), isolated, at the frozen teacher's batch-8 shapes of tools/split2_bench.py.  Three interleaved rounds
(three, fp16 two, bf16 two, three, ...) of tools/_timing.warm_timed per shape on the same tensors; one JSON line per shape with the
three rounds of each leg, the speed-ups (fastest round over fastest round) and whether the fp16 leg's rounds overlap the three-piece
leg's -- a shape that is not ahead by more than the spread belongs in SPLIT2H_ROUTING_EXCLUDED; profiles/r32_split2h_isolated.md.
    python tools/split2h_bench.py
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
from split2_bench import B, C1, C3  # noqa: E402
from structure_knowledge_distillation_amd import _lib, functional as SF  # noqa: E402

# leg -> (suffix of the op's name, its piece keyword)
LEGS = {"bf16x3": ("", dict(pieces=3)), "fp16x2": ("_fp16", {}), "bf16x2": ("", dict(pieces=2))}
op = lambda name, leg: getattr(SF, name + LEGS[leg][0])


def abc(fns, tot, count):
    t = {leg: [] for leg in LEGS}
    for _ in range(3):
        for leg in LEGS:
            t[leg].append(warm_timed(fns[leg], reps=10, warm_ms=30.0, groups=5))
    row = {"us_" + leg: [round(v * 1e3, 1) for v in t[leg]] for leg in LEGS}
    row["fp16x2_over_bf16x3"] = round(min(t["bf16x3"]) / min(t["fp16x2"]), 3)
    row["fp16x2_over_bf16x2"] = round(min(t["bf16x2"]) / min(t["fp16x2"]), 3)
    row["ahead_of_three_beyond_the_spread"] = max(t["fp16x2"]) < min(t["bf16x3"])
    for leg in LEGS:
        tot[leg] += count * min(t[leg])
    return row


def main():
    _lib.load()
    dev = torch.device("cuda", 0)
    tot = {leg: 0.0 for leg in LEGS}
    with torch.no_grad():
        for name, cin, cout, hw, d, bias, count in C3:
            torch.manual_seed(cin + cout + d)
            x = torch.relu(torch.randn(B, cin, hw, hw, device=dev)).contiguous(memory_format=torch.channels_last)
            conv = torch.nn.Conv2d(cin, cout, 3, 1, d, d, bias=bias).to(dev).to(memory_format=torch.channels_last).eval()
            pk = {leg: op("conv3x3_pack_weights", leg)(conv, **kw) for leg, (_, kw) in LEGS.items()}
            fns = {leg: (lambda leg=leg, kw=kw: op("conv3x3_split_eval", leg)(x, pk[leg], cout, d, conv.bias, **kw)) for leg, (_, kw) in LEGS.items()}
            print(json.dumps(dict(kernel="3x3", shape=name, cin=cin, cout=cout, dilation=d, count=count, **abc(fns, tot, count))), flush=True)
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
            fns = {leg: (lambda leg=leg, kw=kw: op("conv1x1_abn_eval", leg)(x, w, rm, rv, ga, be, 1e-5, "relu", 0.01, res, table, **kw))
                   for leg, (_, kw) in LEGS.items()}
            print(json.dumps(dict(kernel="1x1", shape=name, cin=cin, cout=cout, count=count, **abc(fns, tot, count))), flush=True)
    print(json.dumps({"per_teacher_forward_ms": {leg: round(v, 3) for leg, v in tot.items()}}), flush=True)


if __name__ == "__main__":
    main()
