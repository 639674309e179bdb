"""GPU tool: the pair-wise loss's two matrix products on the split core against their fp32 twins, isolated, at B = 8, Cs = 128,
Ct = 512 and M in {289, 1089, 4225} (bench.py's sweep sizes above 64) -- writes the tables of
profiles/r29_pairwise_split_isolated.md:
  (a) skd_pairwise_split_gram_loss against skd_pairwise_gram_loss (G wanted, as in a training step);
  (b) skd_pairwise_split_backward against skd_pairwise_backward;
  (c) functional.pair_wise_loss forward + backward on (8, 128 | 512, 65, 65) features with kernel 2 x 2 (M = 1089) and 1 x 1
      (M = 4225), split=True against split=False;
  (d) the two Gram entries with G = NULL (the loss alone): what of (a) is not the writing of G.
The only GPU use is timing.  Every timed step runs in a child process of its own under a time limit (--limit seconds); the first
child that fails or runs out of time ends the tool, nothing more is started.  A step warms the GPU with >= --warm-ms of the very
launches it times, then runs --rounds interleaved rounds, split and parent alternating, each round one HIP-event bracket around
--reps back-to-back launches; min / median / max over the rounds are printed per side.
A shape is AHEAD when the split side's median is lower and the two sets of rounds do not overlap (max split < min parent);
functional.PAIRWISE_SPLIT_ROUTING_EXCLUDED holds every measured (Cs, Ct, M) whose forward + backward (a) + (b) together are not.
    python tools/pairwise_split_bench.py [--rounds 5] [--reps 10]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, CS, CT = 8, 128, 512
SIZES = (289, 1089, 4225)
KERNELS = ((2, 1089), (1, 4225))           # (pool kernel, M) on 65 x 65 features
STEPS = (["gram:%d" % m for m in SIZES] + ["bwd:%d" % m for m in SIZES] + ["e2e:%d" % k for k, _ in KERNELS]
         + ["loss:%d" % m for m in SIZES])


def sides_of(step):
    """{"split": fn, "parent": fn} of one step, buffers allocated and filled once."""
    import torch
    from structure_knowledge_distillation_amd import _lib, functional as SF
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    kind, n = step.split(":")
    n = int(n)
    torch.manual_seed(n)
    if kind == "e2e":
        SF.PAIRWISE_SPLIT_ROUTING_EXCLUDED = frozenset()      # time the split path whatever the shipped set holds
        fs = torch.randn(B, CS, 65, 65, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        ft = torch.randn(B, CT, 65, 65, device=dev).contiguous(memory_format=torch.channels_last)

        def both(split):
            fs.grad = None
            SF.pair_wise_loss(fs, ft, n, n, split=split).backward()
        return {"split": lambda: both(True), "parent": lambda: both(False)}
    M = n
    ldm = lib.skd_pairwise_ldm(M)
    ps, pt = torch.randn(B, CS, M, device=dev), torch.randn(B, CT, M, device=dev)
    fhs, fht, nrm = torch.empty(B, CS, ldm, device=dev), torch.empty(B, CT, ldm, device=dev), torch.empty(B, M, device=dev)
    assert lib.skd_channel_l2_normalise(B, CS, M, ps.data_ptr(), fhs.data_ptr(), ldm, None, 0, nrm.data_ptr(), None)
    assert lib.skd_channel_l2_normalise(B, CT, M, pt.data_ptr(), fht.data_ptr(), ldm, None, 0, None, None)
    G, loss = torch.empty(B, ldm, ldm, device=dev), torch.empty(1, device=dev)
    ws0 = torch.empty(max(1, lib.skd_pairwise_workspace_floats(B, M)), device=dev)
    ws1 = torch.empty(max(1, lib.skd_pairwise_split_workspace_floats(B, CS, CT, M)), device=dev)
    args = (B, CS, CT, M, ldm, fhs.data_ptr(), fht.data_ptr(), G.data_ptr(), loss.data_ptr())
    assert lib.skd_pairwise_gram_loss(*args, ws0.data_ptr(), None)
    if kind == "gram":
        return {"split": lambda: lib.skd_pairwise_split_gram_loss(*args, ws1.data_ptr(), None),
                "parent": lambda: lib.skd_pairwise_gram_loss(*args, ws0.data_ptr(), None)}
    if kind == "loss":
        args = args[:7] + (None, loss.data_ptr())
        return {"split": lambda: lib.skd_pairwise_split_gram_loss(*args, ws1.data_ptr(), None),
                "parent": lambda: lib.skd_pairwise_gram_loss(*args, ws0.data_ptr(), None)}
    gl, dp = torch.ones(1, device=dev), torch.empty(B, CS, ldm, device=dev)
    bw0 = torch.empty(max(1, lib.skd_pairwise_backward_workspace_floats(B, CS, M)), device=dev)
    bw1 = torch.empty(max(1, lib.skd_pairwise_split_backward_workspace_floats(B, CS, M)), device=dev)
    args = (B, CS, M, ldm, fhs.data_ptr(), G.data_ptr(), nrm.data_ptr(), gl.data_ptr(), dp.data_ptr())
    return {"split": lambda: lib.skd_pairwise_split_backward(*args, bw1.data_ptr(), None),
            "parent": lambda: lib.skd_pairwise_backward(*args, bw0.data_ptr(), None)}


def child(step, rounds, reps, warm_ms):
    import torch
    sides = sides_of(step)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def bracket(fn, n):
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    spent = 0.0
    while spent < warm_ms:                     # both sides, so that neither is timed cold
        spent += bracket(sides["split"], 2) + bracket(sides["parent"], 2)
    runs = {"split": [], "parent": []}
    for _ in range(rounds):
        for side in ("split", "parent"):
            runs[side].append(1e3 * bracket(sides[side], reps) / reps)       # microseconds per launch
    print(json.dumps({"step": step, "split": runs["split"], "parent": runs["parent"]}), flush=True)


def fmt(v):
    return "%.1f / %.1f / %.1f" % (min(v), statistics.median(v), max(v))


def verdict(split, parent):
    if statistics.median(split) < statistics.median(parent) and max(split) < min(parent):
        return "ahead"
    if statistics.median(parent) < statistics.median(split) and max(parent) < min(split):
        return "behind"
    return "overlap"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm-ms", type=float, default=300.0)
    ap.add_argument("--limit", type=int, default=120, help="seconds a timed step may take")
    ap.add_argument("--step", default=None, help="(internal) run this one step in this process")
    a = ap.parse_args()
    if a.step is not None:
        return child(a.step, a.rounds, a.reps, a.warm_ms)
    got = {}
    for step in STEPS:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--step", step, "--rounds", str(a.rounds),
               "--reps", str(a.reps), "--warm-ms", str(a.warm_ms)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
        if res.returncode != 0 or not lines:
            sys.exit("step %s ended with status %d: nothing more is started" % (step, res.returncode))
        got[step] = json.loads(lines[-1])
        print("# %s done" % step, file=sys.stderr, flush=True)
    head = "| %s | split us (min / median / max) | fp32 us (min / median / max) | fp32 / split | verdict |\n|---|---|---|---|---|"
    for title, kind, keys in (("(a) Gram + loss", "gram", SIZES), ("(b) backward", "bwd", SIZES)):
        print("\n%s, B = %d, Cs = %d, Ct = %d\n" % (title, B, CS, CT))
        print(head % "M")
        for m in keys:
            r = got["%s:%d" % (kind, m)]
            print("| %d | %s | %s | %.2f | %s |" % (m, fmt(r["split"]), fmt(r["parent"]),
                                                    statistics.median(r["parent"]) / statistics.median(r["split"]),
                                                    verdict(r["split"], r["parent"])))
    print("\nForward + backward of one shape: the sums of (a) and (b), round by round\n")
    print(head % "M")
    excluded = []
    for m in SIZES:
        s = [x + y for x, y in zip(got["gram:%d" % m]["split"], got["bwd:%d" % m]["split"])]
        p = [x + y for x, y in zip(got["gram:%d" % m]["parent"], got["bwd:%d" % m]["parent"])]
        v = verdict(s, p)
        if v != "ahead":
            excluded.append((CS, CT, m))
        print("| %d | %s | %s | %.2f | %s |" % (m, fmt(s), fmt(p), statistics.median(p) / statistics.median(s), v))
    print("\n(c) pair_wise_loss forward + backward, (%d, %d | %d, 65, 65) channels-last features\n" % (B, CS, CT))
    print(head % "kernel (M)")
    for k, m in KERNELS:
        r = got["e2e:%d" % k]
        print("| %d x %d (%d) | %s | %s | %.2f | %s |" % (k, k, m, fmt(r["split"]), fmt(r["parent"]),
                                                         statistics.median(r["parent"]) / statistics.median(r["split"]),
                                                         verdict(r["split"], r["parent"])))
    print("\n(d) Gram + loss with G = NULL, B = %d, Cs = %d, Ct = %d\n" % (B, CS, CT))
    print(head % "M")
    for m in SIZES:
        r = got["loss:%d" % m]
        print("| %d | %s | %s | %.2f | %s |" % (m, fmt(r["split"]), fmt(r["parent"]),
                                                statistics.median(r["parent"]) / statistics.median(r["split"]),
                                                verdict(r["split"], r["parent"])))
    print("\nPAIRWISE_SPLIT_ROUTING_EXCLUDED = frozenset(%r)" % (excluded,))


if __name__ == "__main__":
    main()
