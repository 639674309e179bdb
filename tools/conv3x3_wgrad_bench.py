"""GPU tool: the weight gradients of the training student's routed 3x3 convolutions at batch 8, 65 x 65, isolated -- writes the
table of profiles/r20_conv3x3_wgrad_isolated.md.  Per shape: MIOpen's weight gradient (``aten.convolution_backward`` with mask
(False, True, False)) against the two launches of skd_conv3x3_split_wgrad_nhwc together, workspace and result allocated outside
the timed region on both sides.  ``tools/_timing.warm_timed`` (>= 30 ms of the same launches as warm-up, then the median of 5
groups of 10 back-to-back launches), ``--rounds`` interleaved rounds parent, split, parent, split, ...; spread = (max - min) /
median of one side's rounds, the larger of the two sides.  ``--slices a,b,c``: further slice counts timed beside the plan's own
(one extra column each, timed once) -- how the shipped rule of skd_conv3x3_split_wgrad_plan was chosen.  ``--lib PATH``: another
build of the library (say, one compiled with -DSKD_WGRAD_GRID_ORDER=1) timed in the same rounds, one more column.
``--narrow``: the six 64-channel convolutions of the stem (256 x 256) and layer1 (129 x 129) on skd_conv3x3_narrow_wgrad_nhwc
instead -- the table of profiles/r23_conv3x3_narrow_wgrad_isolated.md; ``--hw`` is ignored.
``--pieces 2``: the table of profiles/r33_student_pieces_wgrad_isolated.md instead -- the "parent" side is the THREE-piece
skd_conv3x3_split_wgrad_nhwc, the other side skd_conv3x3_split2_wgrad_nhwc (include/skd_train2.h) on the same plan; the library is
not timed.  Not with ``--narrow``, which has no two-piece form.
    python tools/conv3x3_wgrad_bench.py [--rounds 3] [--slices 1,2,4,8] [--lib other/libskd_hip.so] [--narrow] [--pieces 2]
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("PYTORCH_MIOPEN_SUGGEST_NHWC", "1")
PROBLEMS = [  # (name, Cin, Cout, dilation, convolutions of this shape per student step)
    ("layer2 128->128 d1", 128, 128, 1, 3),
    ("layer3.0.conv1 128->256 d2", 128, 256, 2, 1),
    ("layer3 256->256 d2", 256, 256, 2, 3),
    ("layer4.0.conv1 256->512 d4", 256, 512, 4, 1),
    ("layer4 512->512 d4", 512, 512, 4, 3),
    ("dsn[0] 256->128 d1", 256, 128, 1, 1),
    ("psp half 512->128 d1", 512, 128, 1, 1),
]
NARROW_PROBLEMS = [  # (name, Cin, Cout, dilation, convolutions of this shape per student step, map size)
    ("stem conv2 64->64 d1 256x256", 64, 64, 1, 1, 256),
    ("stem conv3 64->128 d1 256x256", 64, 128, 1, 1, 256),
    ("layer1.0.conv1 128->64 d1 129x129", 128, 64, 1, 1, 129),
    ("layer1 64->64 d1 129x129", 64, 64, 1, 3, 129),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--hw", type=int, default=65)
    ap.add_argument("--slices", default="")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--narrow", action="store_true")
    ap.add_argument("--pieces", type=int, default=3, choices=(2, 3))
    a = ap.parse_args()
    if a.pieces == 2 and a.narrow:
        ap.error("--pieces 2: the 128 x 64 form has no two-piece twin")
    import torch
    import structure_knowledge_distillation_amd as _skd
    _skd.configure_miopen()
    from structure_knowledge_distillation_amd import _lib
    from _timing import warm_timed
    lib = _lib.load()
    other = _lib.load(a.lib) if a.lib else None
    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    B, hw = a.batch, a.hw
    extra = [int(s) for s in a.slices.split(",") if s]
    med = statistics.median
    fmt = lambda runs: " / ".join("%.1f" % (1e3 * t) for t in runs)
    form = "narrow" if a.narrow else "split2" if a.pieces == 2 else "split"
    sides = ("three pieces", "two pieces") if a.pieces == 2 else ("parent", "split")
    print("%d compute units; batch %d, %s" % (cus, B, "the step's map sizes" if a.narrow else "%d x %d" % (hw, hw)))
    print()
    print("| convolution | per step | slices (K-tiles each) | %s us (runs) | %s us (runs) | %s / %s | spread | verdict |" % (sides + sides)
          + (" --lib us (runs) |" if other else "") + "".join(" %d slices us |" % s for s in extra))
    print("|---|---|---|---|---|---|---|---|" + "---|" * (len(extra) + bool(other)))
    total_p = total_s = 0.0
    plan = (ctypes.c_int64 * 3)()
    with torch.no_grad():
        for name, cin, cout, d, count, *size in (NARROW_PROBLEMS if a.narrow else PROBLEMS):
            hw = size[0] if size else a.hw
            torch.manual_seed(cin + cout + d)
            x = torch.relu(torch.randn(B, cin, hw, hw, device=dev)).contiguous(memory_format=torch.channels_last)
            g = torch.randn(B, cout, hw, hw, device=dev).contiguous(memory_format=torch.channels_last)
            w = torch.zeros(cout, cin, 3, 3, device=dev).contiguous(memory_format=torch.channels_last)
            dw = torch.empty_like(w)
            st = _lib.stream_of(x)

            def split_side(slices, lib=lib, form=form):
                assert getattr(lib, "skd_conv3x3_%s_wgrad_plan" % form)(B, hw, hw, cin, cout, slices, cus, ctypes.cast(plan, ctypes.c_void_p))
                used, per_slice, nbytes = int(plan[0]), int(plan[1]), int(plan[2])
                ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

                def run():
                    assert getattr(lib, "skd_conv3x3_%s_wgrad_nhwc" % form)(B, hw, hw, cin, cout, d, x.data_ptr(), g.data_ptr(),
                                                                            dw.data_ptr(), *dw.stride(), ws.data_ptr(), nbytes, used, st)
                return run, used, per_slice
            run_s, used, per_slice = split_side(0)
            run_p = lambda: torch.ops.aten.convolution_backward(g, x, w, None, [1, 1], [d, d], [d, d], False, [0, 0], 1,
                                                                (False, True, False))
            if a.pieces == 2:
                run_p = split_side(0, lib, "split")[0]
            run_o = split_side(0, other)[0] if other else None
            runs = {"p": [], "s": [], "o": []}
            for _ in range(a.rounds):
                runs["p"].append(warm_timed(run_p))
                runs["s"].append(warm_timed(run_s))
                if other:
                    runs["o"].append(warm_timed(run_o))
            parent, split = med(runs["p"]), med(runs["s"])
            spread = max((max(v) - min(v)) / med(v) for v in (runs["p"], runs["s"]))
            gain = (parent - split) / parent
            verdict = "ahead" if gain > spread else ("behind" if -gain > spread else "within the spread")
            total_p += count * parent
            total_s += count * split
            cols = " %s |" % fmt(runs["o"]) if other else ""
            for s in extra:
                run_e, used_e, _ = split_side(s)
                cols += " %.1f (%d) |" % (1e3 * warm_timed(run_e), used_e)
            print("| %s | %d | %d (%d) | %s | %s | %.2f | %.1f %% | %s |%s" % (
                name, count, used, per_slice, fmt(runs["p"]), fmt(runs["s"]), parent / split, 100 * spread, verdict, cols), flush=True)
    print()
    print("Per student step (the counts above): %s %.2f ms, %s %.2f ms, difference %.2f ms." % (sides[0], total_p, sides[1], total_s,
                                                                                            total_p - total_s))


if __name__ == "__main__":
    main()
