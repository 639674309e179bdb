"""GPU tool: the split-operand core's timed shapes (the four bottleneck-tail GEMMs, the nine reduce / down-sample GEMMs, the
3x3 convolutions of tools/conv3x3_bench.py, all at batch 8; in the conv3x3 set also one of those with BN + residual + ReLU, the
64-column form at the five batch-1 inference shapes of tools/conv3x3_narrow_bench.py with their epilogues, and the weight images
of both pack_pair entries) through the C ABI of one or more builds of libskd_hip.so, on the same
seeded inputs: one SHA-256 of the output buffer per (shape, library) -- a change of the K loop's schedule must not move one --
and, with --ms, HIP-event timings, the libraries taking turns inside every repeat.

    python tools/split_core_ab.py --lib A.so [--lib B.so ...] [--ms 60] [--only tail|reduce|conv3x3] [--match TEXT]

Without --ms every library launches every selected shape exactly once, in the order given: that is the form for a counter-only
`rocprofv3 --pmc` pass (the libraries' kernels carry the same names; the dispatch order tells them apart).

One JSON line per shape: {"shape", "digest": [per lib], "equal", "us": [[three repeats] per lib]}.  A timed repeat is >= 30 ms of
warm-up launches, then back-to-back calls for about --ms milliseconds between two events.
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RELU = 3
TAIL = [(256, 1024, 33800), (512, 2048, 33800), (128, 512, 33800), (64, 256, 133128)]                 # (K, N, M): prologue + residual + ReLU
REDUCE = [(1024, 256, 33800), (2048, 512, 33800), (512, 128, 33800), (1024, 512, 33800), (512, 256, 33800), (256, 128, 133128),
          (128, 256, 133128), (1024, 2048, 33800), (512, 1024, 33800)]                                # BN + ReLU epilogue, no residual
CONV3 = [(256, 256, 65, 2, False), (2048, 512, 65, 1, False), (512, 512, 65, 4, False), (1024, 512, 65, 1, True),
         (128, 128, 65, 1, False)]                                                                     # (Cin, Cout, HW, dilation, bias)
B = 8
SPLIT, SPLIT_RES, NARROW = "skd_conv3x3_split", "skd_conv3x3_split_res", "skd_conv3x3_narrow"          # entry families
# (entry, batch, H, W, Cin, Cout, dilation, epilogue): epilogue "bn" = BN + ReLU, "res" = BN + residual + ReLU, "raw" = none
CONV3_EPI = [(SPLIT_RES, B, 65, 65, 256, 256, 2, "res"),
             (NARROW, 1, 257, 513, 128, 64, 1, "bn"), (NARROW, 1, 257, 513, 64, 64, 1, "bn"), (NARROW, 1, 257, 513, 64, 64, 1, "res"),
             (NARROW, 1, 512, 1024, 64, 64, 1, "bn"), (NARROW, 1, 512, 1024, 64, 128, 1, "raw")]
PACKS = [(SPLIT, 128, 128), (SPLIT, 512, 256), (NARROW, 64, 64), (NARROW, 64, 128), (NARROW, 128, 64)]    # (entry, Cin, Cout): both images


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", required=True)
    ap.add_argument("--ms", type=float, default=0.0)
    ap.add_argument("--only", default="")
    ap.add_argument("--match", action="append", default=[], help="only the shapes whose name contains this text (repeatable)")
    args = ap.parse_args()
    import torch
    from structure_knowledge_distillation_amd import _lib
    libs = [_lib.load(os.path.abspath(p)) for p in args.lib]
    dev = torch.device("cuda", 0)
    p = lambda t: None if t is None else t.data_ptr()
    rnd = lambda *s: torch.randn(*s, device=dev)

    def measure(name, calls, out):
        """calls[i]() launches the shape on library i into `out`."""
        if args.match and not any(t in name for t in args.match):
            return
        row = {"shape": name, "digest": [], "us": []}
        for call in calls:
            out.fill_(7.0)
            call()
            torch.cuda.synchronize()
            row["digest"].append(hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()[:16])
        row["equal"] = len(set(row["digest"])) == 1
        if args.ms > 0:
            ev = lambda: torch.cuda.Event(enable_timing=True)
            row["us"] = [[] for _ in calls]
            for _ in range(3):
                for i, call in enumerate(calls):
                    e0, e1, spent, n = ev(), ev(), 0.0, 0
                    while spent < 30.0:                   # warm-up, and the time of one call
                        e0.record()
                        for _ in range(8):
                            call()
                        e1.record()
                        e1.synchronize()
                        spent, n = spent + e0.elapsed_time(e1), n + 8
                    reps = max(20, int(args.ms / (spent / n)))
                    e0.record()
                    for _ in range(reps):
                        call()
                    e1.record()
                    e1.synchronize()
                    row["us"][i].append(round(e0.elapsed_time(e1) / reps * 1e3, 1))
        print(json.dumps(row), flush=True)

    def gemm(k, n, m, tail):
        torch.manual_seed(k * 7 + n)
        w = rnd(n, k) * 0.05
        mean, var, ga, be = rnd(n) * 0.3, torch.rand(n, device=dev) + 0.5, rnd(n), rnd(n)
        out = torch.empty(m, n, device=dev)
        if tail:
            x, r = rnd(m, k) * 2 + rnd(1, k), torch.relu(rnd(m, n))
            pk, src = torch.empty(4, k, device=dev), (rnd(k) * 0.5, torch.rand(k, device=dev) * 4 + 2, rnd(k), rnd(k) * 0.5)
            assert libs[0].skd_abn_pack_eval_params(k, p(src[0]), p(src[1]), p(src[2]), p(src[3]), 1e-5, p(pk), None)
            mk = lambda lib: lambda: lib.skd_conv1x1_abn_pro_nhwc(m, k, n, p(x), p(w), p(r), p(out), p(mean), p(var), p(ga), p(be), 1e-5,
                                                                  p(pk), RELU, 0.01, None) or sys.exit("launch refused")
        else:
            x = torch.relu(rnd(m, k) + rnd(1, k) * 0.5)
            mk = lambda lib: lambda: lib.skd_conv1x1_abn_nhwc(m, k, n, p(x), p(w), None, p(out), p(mean), p(var), p(ga), p(be), 1e-5,
                                                              RELU, 0.01, None) or sys.exit("launch refused")
        measure("%s K%d N%d M%d" % ("tail" if tail else "reduce", k, n, m), [mk(lib) for lib in libs], out)

    def conv3(cin, cout, hw, d, bias):
        torch.manual_seed(cin + cout + d)
        x = torch.relu(rnd(B, hw, hw, cin))                                 # channels-last
        wt = rnd(cout, cin, 3, 3) * (2.0 / (9 * cin)) ** 0.5
        cb = rnd(cout) * 0.2 if bias else None
        out = torch.empty(B * hw * hw, cout, device=dev)
        calls, keep = [], []
        for lib in libs:                                                    # every library packs for itself
            nbytes = lib.skd_conv3x3_split_pack_bytes(cin, cout)
            pk = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            assert lib.skd_conv3x3_split_pack_weights(cin, cout, p(wt), *wt.stride(), p(pk), nbytes, None)
            keep.append(pk)
            calls.append(lambda lib=lib, pk=pk: lib.skd_conv3x3_split_nhwc(B, hw, hw, cin, cout, d, p(x), p(pk), p(out), p(cb), None, None,
                                                                          None, None, 0.0, 0, 0.01, 0, None) or sys.exit("launch refused"))
        measure("conv3x3 %d->%d %dx%d d%d%s" % (cin, cout, hw, hw, d, " bias" if bias else ""), calls, out)

    def conv3_epi(entry, b, h, w, cin, cout, d, epi):
        """The entries that take the residual pointer (None unless epi == "res"), with the epilogue `epi`."""
        torch.manual_seed(h + cin + cout + d)
        x = torch.relu(rnd(b, h, w, cin))                                   # channels-last
        wt = rnd(cout, cin, 3, 3) * (2.0 / (9 * cin)) ** 0.5
        bn = [None] * 4 if epi == "raw" else [rnd(cout) * 0.3, torch.rand(cout, device=dev) + 0.5, rnd(cout), rnd(cout)]
        r = rnd(b * h * w, cout) if epi == "res" else None
        out = torch.empty(b * h * w, cout, device=dev)
        calls, keep = [], []
        for lib in libs:                                                    # every library packs for itself
            nbytes = getattr(lib, entry.replace("_res", "") + "_pack_bytes")(cin, cout)
            pk = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            assert getattr(lib, entry.replace("_res", "") + "_pack_pair")(cin, cout, p(wt), *wt.stride(), p(pk), nbytes, None, 0, None)
            keep.append(pk)
            calls.append(lambda run=getattr(lib, entry + "_nhwc"), pk=pk: run(
                b, h, w, cin, cout, d, p(x), p(pk), p(out), p(r), None, *(p(t) for t in bn), 1e-5, 0 if epi == "raw" else RELU, 0.01, 0,
                None) or sys.exit("launch refused"))
        measure("%s %d->%d %dx%dx%d d%d %s" % (entry[4:], cin, cout, b, h, w, d, epi), calls, out)

    def packs(entry, cin, cout):
        """Both weight images of one pack_pair launch, forward image first, in one buffer."""
        torch.manual_seed(cin * 3 + cout)
        wt = rnd(cout, cin, 3, 3)
        nf, nb = (getattr(libs[0], entry + "_pack_bytes")(*dims) for dims in ((cin, cout), (cout, cin)))
        assert nf > 0 and nb > 0 and nf % 16 == 0
        out = torch.empty(nf + nb, dtype=torch.uint8, device=dev)
        mk = lambda lib: lambda: getattr(lib, entry + "_pack_pair")(cin, cout, p(wt), *wt.stride(), p(out), nf, p(out) + nf, nb,
                                                                      None) or sys.exit("launch refused")
        measure("%s_pack_pair %d->%d" % (entry[4:], cin, cout), [mk(lib) for lib in libs], out)

    for k, n, m in TAIL if args.only in ("", "tail") else []:
        gemm(k, n, m, True)
    for k, n, m in REDUCE if args.only in ("", "reduce") else []:
        gemm(k, n, m, False)
    for c in CONV3 if args.only in ("", "conv3x3") else []:
        conv3(*c)
    for c in CONV3_EPI if args.only in ("", "conv3x3") else []:
        conv3_epi(*c)
    for c in PACKS if args.only in ("", "conv3x3") else []:
        packs(*c)


if __name__ == "__main__":
    main()
