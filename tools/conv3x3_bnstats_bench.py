"""GPU tool: batch-norm statistics from the convolution's epilogue, isolated -- writes the table of
profiles/r26_conv3x3_bnstats_isolated.md.  For every BasicBlock convolution the opt-in is about (the 11 wide ones of layer2-4 at
65 x 65, layer1's four at 129 x 129, batch 8), with and without the residual of a block's second convolution, on ONE set of buffers:
    new     skd_conv3x3_{split,narrow}_stats_nhwc  +  skd_abn_stats_from_partials_nhwc  +  skd_abn_apply_nhwc_to
    parent  skd_conv3x3_{split,narrow}_nhwc        +  skd_abn_forward_train_nhwc (the one-launch register-resident form)
and, for information, the two convolution launches and the finalize on their own.  ``tools/_timing.warm_timed`` (>= 30 ms of the
same launches as warm-up, then the median of 5 groups of 10 back-to-back launches), ``--rounds`` interleaved rounds parent, new,
parent, new, ...; spread = (max - min) / median of one side's rounds, the larger of the two sides.  A shape is ahead only where it
is ahead by more than the spread; one that is not belongs in pspnet_combine.BNSTATS_ROUTING_EXCLUDED.
    python tools/conv3x3_bnstats_bench.py [--rounds 3]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
SHAPES = [  # (name, H = W, Cin, Cout, dilation, convolutions of this shape per student step: without / with residual)
    ("layer2 128->128 65x65 d1", 65, 128, 128, 1, (1, 2)),
    ("layer3.0.conv1 128->256 65x65 d2", 65, 128, 256, 2, (1, 0)),
    ("layer3 256->256 65x65 d2", 65, 256, 256, 2, (1, 2)),
    ("layer4.0.conv1 256->512 65x65 d4", 65, 256, 512, 4, (1, 0)),
    ("layer4 512->512 65x65 d4", 65, 512, 512, 4, (1, 2)),
    ("layer1.0.conv1 128->64 129x129 d1 (narrow)", 129, 128, 64, 1, (1, 0)),
    ("layer1 64->64 129x129 d1 (narrow)", 129, 64, 64, 1, (1, 2)),
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
    from structure_knowledge_distillation_amd import _lib
    from _timing import warm_timed
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    med = statistics.median
    fmt = lambda runs: " / ".join("%.1f" % (1e3 * t) for t in runs)
    P = lambda t: None if t is None else t.data_ptr()
    print("Batch %d; microseconds; runs = the %d interleaved rounds" % (a.batch, a.rounds))
    print()
    print("| convolution | residual | per step | conv (runs) | conv + stats (runs) | finalize (runs) | parent: conv + one-launch ABN (runs) "
          "| new: conv with stats + finalize + apply (runs) | parent | new | parent / new | spread | verdict |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    total_p = total_n = 0.0
    for name, hw, cin, cout, d, counts in SHAPES:
        torch.manual_seed(hw + cin + cout)
        b, m = a.batch, a.batch * hw * hw
        narrow = cout % 128 != 0
        x = torch.relu(torch.randn(b, hw, hw, cin, device=dev))
        w = torch.randn(cout, cin, 3, 3, device=dev) * (2.0 / (9 * cin)) ** 0.5
        nbytes = cout * cin * 54
        pack = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        pack_pair = lib.skd_conv3x3_narrow_pack_pair if narrow else lib.skd_conv3x3_split_pack_pair
        assert pack_pair(cin, cout, P(w), *w.stride(), P(pack), nbytes, None, 0, st)
        y, out, res = (torch.empty(m, cout, device=dev) for _ in range(3))
        res.normal_()
        n = lib.skd_conv3x3_bnstats_floats(m, cout)
        stats = torch.empty(n, device=dev)
        ws = torch.empty(max(1, lib.skd_abn_nhwc_workspace_floats(m, cout)), device=dev)
        mean, var, gamma, beta, rm = (torch.zeros(cout, device=dev) for _ in range(5))
        gamma.fill_(1.0)
        rv = torch.ones(cout, device=dev)

        def conv_plain():
            if narrow:
                assert lib.skd_conv3x3_narrow_nhwc(b, hw, hw, cin, cout, d, P(x), P(pack), P(y), None, None, None, None, None, None, 0.0,
                                                   0, 0.01, 0, st)
            else:
                assert lib.skd_conv3x3_split_nhwc(b, hw, hw, cin, cout, d, P(x), P(pack), P(y), None, None, None, None, None, 0.0, 0,
                                                  0.01, 0, st)

        def conv_stats():
            entry = lib.skd_conv3x3_narrow_stats_nhwc if narrow else lib.skd_conv3x3_split_stats_nhwc
            assert entry(b, hw, hw, cin, cout, d, P(x), P(pack), P(y), None, 0, P(stats), n, st)

        def finalize():
            assert lib.skd_abn_stats_from_partials_nhwc(m, cout, P(stats), n, P(mean), P(var), P(rm), P(rv), 0.1, st)

        for with_res, count in zip((False, True), counts):
            if count == 0:
                continue
            r = res if with_res else None

            def parent():
                conv_plain()
                assert lib.skd_abn_forward_train_nhwc(m, cout, P(y), P(r), P(out), P(gamma), P(beta), P(rm), P(rv), P(mean), P(var), 0.1,
                                                      1e-5, 3, 0.0, P(ws), st)

            def new():
                conv_stats()
                finalize()
                assert lib.skd_abn_apply_nhwc_to(m, cout, P(y), P(r), P(out), P(mean), P(var), P(gamma), P(beta), 1e-5, 3, 0.0, st)
            sides = {"c": conv_plain, "cs": conv_stats, "f": finalize, "p": parent, "n": new}
            runs = {k: [] for k in sides}
            for _ in range(a.rounds):
                for k in ("c", "cs", "f", "p", "n"):
                    runs[k].append(warm_timed(sides[k]))
            spread, verdict = verdict_of(runs["p"], runs["n"])
            total_p += count * med(runs["p"])
            total_n += count * med(runs["n"])
            print("| %s | %s | %d | %s | %s | %s | %s | %s | %.1f | %.1f | %.2f | %.1f %% | %s |" % (
                name, "yes" if with_res else "no", count, fmt(runs["c"]), fmt(runs["cs"]), fmt(runs["f"]), fmt(runs["p"]),
                fmt(runs["n"]), 1e3 * med(runs["p"]), 1e3 * med(runs["n"]), med(runs["p"]) / med(runs["n"]), 100 * spread, verdict),
                flush=True)
        del x, y, out, res, stats, ws
    print()
    print("Per student step (the counts above, forward only): parent %.3f ms, new %.3f ms, difference %.3f ms."
          % (total_p, total_n, total_p - total_n))


if __name__ == "__main__":
    main()
