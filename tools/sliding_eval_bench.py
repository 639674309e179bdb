"""Times the fused sliding-window evaluation tail (csrc/evaluate_sliding.hip) for one 1024 x 2048 image, 18 tiles of 512^2,
19 x 65 x 65 logits per tile, against the straightforward torch composition of the reference recipe on the same GPU
(networks/evaluate.py:70-104, 187-198: F.interpolate per tile, float64 ``+=`` into (H, W, C) sums and counts, divide, argmax,
bincount), and the 18-tile student forward that precedes the tail.  Median of per-repetition HIP-event times after warm-up,
one process.  Prints one JSON line; writes nothing.  The results are recorded in profiles/sliding_eval.md.

    python tools/sliding_eval_bench.py [--reps 30] [--no-student]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import structure_knowledge_distillation_amd as S  # noqa: E402
from structure_knowledge_distillation_amd import functional as SF  # noqa: E402
from structure_knowledge_distillation_amd.networks import evaluate as E  # noqa: E402


def timed(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "reps": reps}


def torch_composition(logits, tiles, tile, H, W, target, C):
    """The reference recipe with every array kept on the GPU (the reference itself copies each tile to the host)."""
    total = torch.zeros((H, W, C), dtype=torch.float64, device=logits.device)
    count = torch.zeros((H, W, C), dtype=torch.float64, device=logits.device)
    for t, (y1, x1, y2, x2) in enumerate(tiles):
        up = F.interpolate(logits[t:t + 1], size=tile, mode="bilinear", align_corners=True)[0].permute(1, 2, 0)
        count[y1:y2, x1:x2] += 1
        total[y1:y2, x1:x2] += up[:y2 - y1, :x2 - x1]
    total /= count
    pred = total.argmax(2).to(torch.uint8)
    keep = target != 255
    cm = torch.bincount(target[keep] * C + pred[keep].long(), minlength=C * C).reshape(C, C)
    return pred, cm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--no-student", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sliding_eval_bench needs an MI355X: there is no CPU timing")
    S.configure_miopen()
    dev = torch.device("cuda", 0)
    H, W, tile, C = 1024, 2048, (512, 512), 19
    tiles = E.sliding_tiles(H, W, tile)
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(len(tiles), C, 65, 65, generator=g) * 16).to(dev)
    target = torch.randint(0, C, (H, W), generator=g).to(dev)
    target[:100, :500] = 255
    tl = torch.tensor(tiles, dtype=torch.int32, device=dev)
    cm = torch.zeros((C, C), dtype=torch.int64, device=dev)
    out = {"image": [H, W], "tile": list(tile), "tiles": len(tiles), "classes": C, "logits_hw": [65, 65]}
    out["fused_confusion_only"] = timed(lambda: SF.seg_sliding(logits, tl, tile, (H, W), target=target, confusion=cm, want_pred=False), args.reps)
    out["fused_pred_and_confusion"] = timed(lambda: SF.seg_sliding(logits, tl, tile, (H, W), target=target, confusion=cm), args.reps)
    out["fused_with_probs"] = timed(lambda: SF.seg_sliding(logits, tl, tile, (H, W), target=target, confusion=cm, want_probs=True), args.reps)
    out["torch_composition"] = timed(lambda: torch_composition(logits, tiles, tile, H, W, target, C), args.reps)
    # same inputs, same answer (the composition's interpolate may round the last bit differently: count, do not assert zero)
    pred, _, cm1 = SF.seg_sliding(logits, tl, tile, (H, W), target=target)
    pred2, cm2 = torch_composition(logits, tiles, tile, H, W, target, C)
    out["pixels_differing_from_composition"] = int((pred != pred2).sum())
    out["confusion_total"] = [int(cm1.sum()), int(cm2.sum())]
    out["speedup_pred_and_confusion"] = out["torch_composition"]["median_ms"] / out["fused_pred_and_confusion"]["median_ms"]
    out["gather_bytes_model"] = int(logits.numel() * 4 + H * W * 9)
    if not args.no_student:
        from structure_knowledge_distillation_amd.networks import pspnet_combine
        torch.manual_seed(1)
        net = pspnet_combine.Res_pspnet(pspnet_combine.BasicBlock, [2, 2, 2, 2], C).to(dev).to(memory_format=torch.channels_last).eval()
        batch = (torch.randn(len(tiles), 3, 512, 512, generator=g) * 57).to(dev).contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            out["student_forward_18_tiles"] = timed(lambda: net(batch), max(args.reps // 3, 5), warm=3)
        whole = out["student_forward_18_tiles"]["median_ms"] + out["fused_confusion_only"]["median_ms"]
        out["tail_share_of_image"] = out["fused_confusion_only"]["median_ms"] / whole
    print(json.dumps(out))


if __name__ == "__main__":
    main()
