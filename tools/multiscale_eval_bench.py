"""Times multi-scale / flip evaluation of one seeded 1024 x 2048 image with the real student (Res_pspnet BasicBlock [2, 2, 2, 2],
eval, channels-last), scales (0.75, 1.0, 1.25, 1.5, 1.75) with flip: the five resize kernels (skd_zoom_linear), the five
forwards of batch 2 and the fused tail (skd_seg_multiscale) separately, and the tail next to the straightforward torch
composition of the reference recipe on the same GPU and the same logits (networks/evaluate.py:115-134, 187-198: F.interpolate
per map, fp32 flip average, float64 ``+=``, divide, argmax, bincount).  Median of per-repetition HIP-event times after warm-up
of every shape, one process.  Prints one JSON line and writes the table to profiles/<next round>_multiscale_eval.md (``--out``).

    python tools/multiscale_eval_bench.py [--reps 20] [--out FILE]
"""
import argparse
import json
import os
import re
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import structure_knowledge_distillation_amd as S  # noqa: E402
from structure_knowledge_distillation_amd import functional as SF  # noqa: E402

SCALES = (0.75, 1.0, 1.25, 1.5, 1.75)


def timed(fn, reps, warm=3):
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


def torch_composition(logits, H, W, target, C):
    """The reference recipe with every array kept on the GPU (the reference itself copies each up-sampled map to the host)."""
    total = torch.zeros((H, W, C), dtype=torch.float64, device=target.device)
    for lg in logits:
        up = F.interpolate(lg, size=(H, W), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
        total += 0.5 * (up[0] + up[1].flip(1))
    total /= len(logits)
    pred = total.argmax(2).to(torch.uint8)
    keep = target != 255
    cm = torch.bincount(target[keep] * C + pred[keep].long(), minlength=C * C).reshape(C, C)
    return pred, cm


def next_round_path():
    prof = os.path.join(ROOT, "profiles")
    rounds = [int(m.group(1)) for f in os.listdir(prof) if not f.endswith("_multiscale_eval.md") for m in [re.match(r"r(\d+)", f)] if m]
    return os.path.join(prof, "r%02d_multiscale_eval.md" % (max(rounds, default=0) + 1))


def row(label, t):
    return "| %s | %.3f | %.3f … %.3f |" % (label, t["median_ms"], t["min_ms"], t["max_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multiscale_eval_bench needs an MI355X: there is no CPU timing")
    S.configure_miopen()
    from structure_knowledge_distillation_amd.networks import pspnet_combine
    dev = torch.device("cuda", 0)
    H, W, C = 1024, 2048, 19
    g = torch.Generator().manual_seed(3)
    image = (torch.randn(1, 3, H, W, generator=g) * 57.0).to(dev)
    target = torch.randint(0, C, (H, W), generator=g).to(dev)
    target[:100, :500] = 255
    torch.manual_seed(1)
    net = pspnet_combine.Res_pspnet(pspnet_combine.BasicBlock, [2, 2, 2, 2], C).to(dev).to(memory_format=torch.channels_last).eval()
    cm = torch.zeros((C, C), dtype=torch.int64, device=dev)
    out = {"image": [H, W], "classes": C, "scales": list(SCALES), "flip": True}
    with torch.no_grad():
        batches = [SF.zoom_linear(image, s, mirror=True, channels_last=True) for s in SCALES]
        out["scaled_sizes"] = [list(b.shape[2:]) for b in batches]
        out["resize_5_scales"] = timed(lambda: [SF.zoom_linear(image, s, mirror=True, channels_last=True) for s in SCALES], args.reps)
        out["forwards_5_scales_batch_2"] = timed(lambda: [net(b) for b in batches], max(args.reps // 4, 5), warm=2)
        logits = [net(b)[0].float().contiguous() for b in batches]
    out["logit_sizes"] = [list(lg.shape[2:]) for lg in logits]
    out["fused_confusion_only"] = timed(lambda: SF.seg_multiscale(logits, (H, W), target=target, confusion=cm, want_pred=False), args.reps)
    out["fused_pred_and_confusion"] = timed(lambda: SF.seg_multiscale(logits, (H, W), target=target, confusion=cm), args.reps)
    out["fused_with_probs"] = timed(lambda: SF.seg_multiscale(logits, (H, W), target=target, confusion=cm, want_probs=True), args.reps)
    out["torch_composition"] = timed(lambda: torch_composition(logits, H, W, target, C), args.reps)
    # same inputs, same answer (the composition's interpolate may round the last bit differently: count, do not assert zero)
    pred, _, cm1 = SF.seg_multiscale(logits, (H, W), target=target)
    pred2, cm2 = torch_composition(logits, H, W, target, C)
    out["pixels_differing_from_composition"] = int((pred != pred2).sum())
    out["confusion_total"] = [int(cm1.sum()), int(cm2.sum())]
    ratio = out["torch_composition"]["median_ms"] / out["fused_pred_and_confusion"]["median_ms"]
    out["composition_over_fused"] = ratio
    whole = out["resize_5_scales"]["median_ms"] + out["forwards_5_scales_batch_2"]["median_ms"] + out["fused_confusion_only"]["median_ms"]
    out["ms_per_image"] = whole
    print(json.dumps(out))

    verdict = ("The fused tail is **%.1f x faster** than the composition" % ratio) if ratio > 1.0 else \
        ("The fused tail is **NOT faster** than the composition: %.2f x its time" % (1.0 / ratio))
    lines = [
        "# Multi-scale / flip evaluation of one image on one MI355X",
        "",
        "Written by `python tools/multiscale_eval_bench.py --reps %d` (one process, HIP events around every repetition, every shape" % args.reps,
        "warmed up first, median of %d; the forwards: 2 warm-up, median of %d).  Input: one seeded 1024 × 2048 image, the real student" % (args.reps, max(args.reps // 4, 5)),
        "(Res_pspnet BasicBlock [2, 2, 2, 2], seeded, eval, channels-last), scales %s with flip, 19 classes, int64 label with an" % (list(SCALES),),
        "ignore region.  Scaled sizes %s, logit maps %s.  Same process, same tensors for every variant." % (out["scaled_sizes"], out["logit_sizes"]),
        "",
        "| part of one image | median ms | min … max ms |",
        "|---|---|---|",
        row("resize, 5 launches of `skd_zoom_linear` (image + mirrored copy, channels-last)", out["resize_5_scales"]),
        row("student forwards, 5 batches of 2", out["forwards_5_scales_batch_2"]),
        row("fused tail (`skd_seg_multiscale`), confusion matrix only (what `evaluate_main` runs)", out["fused_confusion_only"]),
        row("fused tail, uint8 prediction + confusion matrix", out["fused_pred_and_confusion"]),
        row("fused tail, + float64 probabilities (H, W, C) (what `predict_multiscale` runs)", out["fused_with_probs"]),
        row("torch composition of the reference recipe on the same GPU and logits: per scale `F.interpolate` (bilinear, align_corners) "
            "of both maps, fp32 flip average, float64 `+=` into (H, W, C), divide, argmax, `bincount`", out["torch_composition"]),
        "",
        "* %s (prediction + confusion matrix against the composition's prediction + confusion matrix).  %d of %d predictions differ"
        % (verdict, out["pixels_differing_from_composition"], H * W),
        "  between the two; the matrices hold %d and %d scored pixels." % tuple(out["confusion_total"]),
        "* One image takes %.2f ms (resize + forwards + confusion-only tail); the tail is %.1f %% of it, the resize %.1f %%."
        % (whole, 100 * out["fused_confusion_only"]["median_ms"] / whole, 100 * out["resize_5_scales"]["median_ms"] / whole),
        "",
        "Not measured: other image sizes or scale sets, the host-side loader, a counter profile of either kernel.",
        "",
    ]
    path = args.out or next_round_path()
    with open(path, "w") as fh:
        fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
