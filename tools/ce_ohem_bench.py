"""Times the fused OHEM criterion (csrc/ce_ohem.hip) at (8, 19, 65, 65) -> (512, 512), thresh 0.7, min_kept 100000, factor 8,
forward + gradient, on a warm GPU (tools/_timing.py), next to its two yardsticks on the same inputs:

  1. the fused OHEM criterion: ``skd_ohem_threshold`` + ``skd_ce_ohem_dsn_forward`` (and each of the two alone: the split
     between the threshold pre-pass and the main pass);
  2. ``skd_ce_dsn_forward``, the plain criterion (what "cheap enough" is measured against);
  3. the reference recipe composed from torch + scipy on the same GPU, its host copies included: up-sample, softmax, copy to the
     host, ``scipy.ndimage.zoom`` twice, ``np.partition``, a new target built on the host and copied back, two cross-entropies,
     backward.  Wall-clock around a synchronised repetition (the recipe synchronises by itself).

Prints one JSON line and writes the table to ``--out`` (default profiles/r16_ce_ohem.md).

    python tools/ce_ohem_bench.py [--reps 10] [--recipe-reps 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from structure_knowledge_distillation_amd import _lib  # noqa: E402
from structure_knowledge_distillation_amd.functional import zoom_size  # noqa: E402
from _timing import warm_timed  # noqa: E402

B, C, h, w, H, W = 8, 19, 65, 65, 512, 512
THRESH, MIN_KEPT, FACTOR, IGNORE = 0.7, 100000, 8, 255


def make_inputs(dev):
    """A label field with confident logits on it, 2 % flipped labels and an ignored band (the recipe of the test fixture)."""
    g = torch.Generator().manual_seed(21)
    field = torch.randint(0, C, (B, h, w), generator=g)
    margin = 8.0 + 2.0 * torch.rand((B, 1, h, w), generator=g)
    onehot = F.one_hot(field, C).permute(0, 3, 1, 2).float()
    lm = torch.randn((B, C, h, w), generator=g) * 2.0 + margin * onehot
    ld = torch.randn((B, C, h, w), generator=g) * 2.0 + margin * onehot
    target = F.interpolate(field[:, None].float(), size=(H, W), mode="nearest")[:, 0].long()
    flip = torch.rand((B, H, W), generator=g) < 0.02
    target = torch.where(flip, torch.randint(0, C, (B, H, W), generator=g), target)
    target[:, H // 3:H // 3 + H // 10, :] = IGNORE
    return lm.contiguous().to(dev), ld.contiguous().to(dev), target.contiguous().to(dev)


def reference_recipe(lm, ld, target):
    """OHEM as the reference composes it (host round trip included); returns (loss, threshold, kept pixels)."""
    import scipy.ndimage as nd
    lm = lm.detach().requires_grad_(True)
    ld = ld.detach().requires_grad_(True)
    up = F.interpolate(lm, size=(H, W), mode="bilinear", align_corners=True)
    prob = F.softmax(up, 1).detach().cpu().numpy()
    tg = target.cpu().numpy()
    small_p = nd.zoom(prob, (1.0, 1.0, 1.0 / FACTOR, 1.0 / FACTOR), order=1)
    small_t = nd.zoom(tg, (1.0, 1.0 / FACTOR, 1.0 / FACTOR), order=0).ravel().astype(np.int32)
    mk = MIN_KEPT // (FACTOR * FACTOR)
    ok = small_t != IGNORE
    threshold = 1.0
    if mk < ok.sum():
        pred = np.moveaxis(small_p, 1, 0).reshape(C, -1)[:, ok][small_t[ok], np.arange(int(ok.sum()))]
        threshold = THRESH
        if mk > 0:
            kth = np.partition(pred, mk - 1)[mk - 1]
            threshold = kth if kth > THRESH else THRESH
    flat = tg.ravel()
    valid = flat != IGNORE
    p_label = np.moveaxis(prob, 1, 0).reshape(C, -1)[np.where(valid, flat, 0), np.arange(flat.size)]
    keep = valid & (p_label <= threshold)
    new_target = torch.from_numpy(np.where(keep, flat, IGNORE).reshape(tg.shape)).long().to(target.device)
    loss = F.cross_entropy(up, new_target, ignore_index=IGNORE) + 0.4 * F.cross_entropy(
        F.interpolate(ld, size=(H, W), mode="bilinear", align_corners=True), target, ignore_index=IGNORE)
    loss.backward()
    return float(loss.detach()), float(threshold), int(keep.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--recipe-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_ce_ohem.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ce_ohem_bench needs an MI355X: there is no CPU timing")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    lm, ld, tg = make_inputs(dev)
    P = lambda t: None if t is None else t.data_ptr()
    new = lambda *s: torch.empty(s, device=dev)
    thr, nv = new(1), torch.empty(1, dtype=torch.int32, device=dev)
    loss, nk, gm, gd = new(1), new(1), torch.empty_like(lm), torch.empty_like(ld)
    ws = new(lib.skd_ce_ohem_workspace_floats(B, C, h, w, H, W, FACTOR))
    ws_plain = new(lib.skd_ce_dsn_workspace_floats(B, C, h, w, H, W))

    def threshold(min_kept=MIN_KEPT):
        assert lib.skd_ohem_threshold(B, C, h, w, H, W, P(lm), P(tg), IGNORE, THRESH, min_kept, FACTOR, P(thr), P(nv), None, P(ws), None)

    def main_pass():
        assert lib.skd_ce_ohem_dsn_forward(B, C, h, w, H, W, P(lm), P(ld), P(tg), IGNORE, 0.4, P(thr), P(loss), P(nk), None, P(gm),
                                           P(gd), P(ws), None)

    def fused():
        threshold()
        main_pass()

    def plain():
        assert lib.skd_ce_dsn_forward(B, C, h, w, H, W, P(lm), P(ld), P(tg), IGNORE, 0.4, P(loss), P(gm), P(gd), P(ws_plain), None)

    out = {"shape": [B, C, h, w, H, W], "thresh": THRESH, "min_kept": MIN_KEPT, "factor": FACTOR,
           "keys": B * zoom_size(H, 1.0 / FACTOR) * zoom_size(W, 1.0 / FACTOR)}
    out["fused_ohem_ms"] = warm_timed(fused, reps=args.reps)
    out["threshold_pass_ms"] = warm_timed(threshold, reps=args.reps)
    # min_kept 0: the selection stops after its first histogram (which counts the valid keys): keys kernel + one of four passes
    out["threshold_pass_no_select_ms"] = warm_timed(lambda: threshold(0), reps=args.reps)
    out["main_pass_ms"] = warm_timed(main_pass, reps=args.reps)
    out["plain_ce_dsn_ms"] = warm_timed(plain, reps=args.reps)
    fused()
    torch.cuda.synchronize()
    out["threshold"], out["num_valid"], out["n_kept"], out["loss"] = float(thr), int(nv), float(nk), float(loss)
    recipe = []
    for _ in range(1 + args.recipe_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = reference_recipe(lm, ld, tg)
        torch.cuda.synchronize()
        recipe.append(1e3 * (time.perf_counter() - t0))
    recipe = sorted(recipe[1:])
    out["reference_recipe_ms"] = recipe[len(recipe) // 2]
    out["recipe_loss"], out["recipe_threshold"], out["recipe_kept"] = res
    out["fused_over_plain"] = out["fused_ohem_ms"] / out["plain_ce_dsn_ms"]
    print(json.dumps(out))

    over = out["fused_over_plain"]
    lines = [
        "# OHEM criterion (CriterionOhemDSN) on one MI355X",
        "",
        "Written by `python tools/ce_ohem_bench.py --reps %d --recipe-reps %d` (one process, warm GPU: tools/_timing.py, median of 5" % (args.reps, args.recipe_reps),
        "groups of %d back-to-back calls; the recipe: wall-clock of a synchronised repetition, median of %d after one warm-up)." % (args.reps, args.recipe_reps),
        "Input: logits (%d, %d, %d, %d) -> target (%d, %d), thresh %.1f, min_kept %d, factor %d: %d down-sampled keys, %d valid;" % (
            B, C, h, w, H, W, THRESH, MIN_KEPT, FACTOR, out["keys"], out["num_valid"]),
        "threshold %.7f, %d pixels kept.  Forward + both gradients in every row." % (out["threshold"], int(out["n_kept"])),
        "",
        "| what | ms |",
        "|---|---|",
        "| 1. fused OHEM criterion: `skd_ohem_threshold` + `skd_ce_ohem_dsn_forward` | %.4f |" % out["fused_ohem_ms"],
        "| &nbsp;&nbsp; threshold pre-pass alone (keys kernel + one-workgroup radix select) | %.4f |" % out["threshold_pass_ms"],
        "| &nbsp;&nbsp; &nbsp;&nbsp; of it with `min_kept = 0` (keys kernel + the first of the select's four histogram passes) | %.4f |" % out["threshold_pass_no_select_ms"],
        "| &nbsp;&nbsp; main pass alone (cells, finalize, nodes) | %.4f |" % out["main_pass_ms"],
        "| 2. `skd_ce_dsn_forward`, the plain criterion, same inputs | %.4f |" % out["plain_ce_dsn_ms"],
        "| 3. reference recipe from torch + scipy on the same GPU, host copies included | %.1f |" % out["reference_recipe_ms"],
        "",
        "* (1) is %.2f x (2)%s." % (over, "" if over <= 1.25 else ": MORE than a quarter above it"),
        "* Where the time goes: the pre-pass is %.0f %% of (1) -- two launches of a few microseconds of work each, the second a single"
        % (100 * out["threshold_pass_ms"] / out["fused_ohem_ms"]),
        "  workgroup whose four dependent passes over the keys cannot overlap (%.4f ms of the pre-pass's %.4f lie after the first"
        % (out["threshold_pass_ms"] - out["threshold_pass_no_select_ms"], out["threshold_pass_ms"]),
        "  histogram); the OHEM main pass is %.2f x the plain criterion's whole time."
        % (out["main_pass_ms"] / out["plain_ce_dsn_ms"]),
        "* The recipe is %.0f x (1); it found threshold %.7f, kept %d pixels, loss %.6f (fused: %.6f)." % (
            out["reference_recipe_ms"] / out["fused_ohem_ms"], out["recipe_threshold"], out["recipe_kept"], out["recipe_loss"], out["loss"]),
        "",
        "Not measured: other shapes, class counts above 24 (the spilling instantiation), a counter profile of either kernel.",
        "",
    ]
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
