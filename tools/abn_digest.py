"""GPU tool: one SHA-256 per (InPlace-ABN entry, case) over the raw bytes of every output buffer, for comparing two builds of
libskd_hip.so bit for bit (a refactor of csrc/abn*.hip must not move a single digest: the expressions are unchanged and every
reduction is fixed-order).

    python tools/abn_digest.py --lib PATH > digests.txt         (run it once per library, then diff the two files)

Covers every non-synchronised entry: the planar NCHW ones and the legacy drop-ins (a shape on each side of the 2*S >= kChunk
split and one whose tensors start 4 bytes off a 16-byte boundary), the channels-last ones (tools/kernel_microbench.py's student
layers at batch 8 in the main configuration; one ragged row count per channel width with every activation an entry accepts, with
and without residual, affine and not; the one-call forms with skd_abn_set_fused 1 and 0) and the three stem entries.  The
synchronised (`_sync`) forms need peer ranks: tests/test_distributed_gpu.py.
"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kernel_microbench import STUDENT  # noqa: E402

NONE, LEAKY, ELU, RELU = 0, 1, 2, 3
RAGGED = [(8 * 33 * 33 + 5, 64), (4 * 65 * 65 + 3, 128), (2 * 65 * 65 + 1, 256), (1037, 512)]
NCHW = [(2, 5, 65 * 65, 0), (3, 7, 33 * 33, 0), (2, 6, 4099, 1)]       # (N, C, S, floats off alignment): 2*S >= 8192, below it, misaligned


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    import torch
    from structure_knowledge_distillation_amd import _lib
    lib = _lib.load(os.path.abspath(ap.parse_args().lib))
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: None if t is None else t.data_ptr()
    rnd = lambda *s: torch.randn(*s, device=dev)
    new = lambda *s: torch.zeros(*s, device=dev)

    def emit(name, case, ok, *outs):
        assert ok, (name, case)
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in outs:
            h.update(t.detach().contiguous().cpu().numpy().tobytes())
        print("%s  %-46s %s" % (h.hexdigest(), name, case), flush=True)

    def nhwc(rows, C, full):
        torch.manual_seed(rows * 131 + C)
        x, r, dz = rnd(rows, C) * 2 + 0.5, rnd(rows, C), rnd(rows, C)
        ws = new(lib.skd_abn_nhwc_workspace_floats(rows, C))
        for affine in (True, False) if full else (True,):
            w, b = (rnd(C), rnd(C)) if affine else (None, None)
            case = "rows=%d C=%d affine=%d" % (rows, C, affine)
            m, v, e, ey, dw, db = (new(C) for _ in range(6))
            emit("stats_nhwc", case, lib.skd_abn_stats_nhwc(rows, C, p(x), p(m), p(v), p(ws), st), m, v)
            zs = {}
            for act in (NONE, LEAKY, ELU, RELU) if full else (LEAKY, RELU):
                for res in (None, r):
                    c2 = "%s act=%d res=%d" % (case, act, res is not None)
                    out = torch.empty_like(x)
                    emit("apply_nhwc_to", c2, lib.skd_abn_apply_nhwc_to(rows, C, p(x), p(res), p(out), p(m), p(v), p(w), p(b), 1e-5, act, 0.01, st), out)
                    if act != ELU:
                        y = x.clone()
                        emit("apply_nhwc", c2, lib.skd_abn_apply_nhwc(rows, C, p(y), p(res), p(m), p(v), p(w), p(b), 1e-5, act, 0.01, st), y)
                    for fused in (1, 0):
                        lib.skd_abn_set_fused(fused)
                        rm, rv, mm, vv = new(C), new(C) + 1, new(C), new(C)
                        emit("forward_train_nhwc", "%s fused=%d" % (c2, fused), lib.skd_abn_forward_train_nhwc(
                            rows, C, p(x), p(res), p(out), p(w), p(b), p(rm), p(rv), p(mm), p(vv), 0.1, 1e-5, act, 0.01, p(ws), st), out, rm, rv, mm, vv)
                    if res is None:
                        zs[act] = out
            dx, dres = torch.zeros_like(x), torch.zeros_like(x)
            for act in (NONE, LEAKY, ELU) if full else (LEAKY,):
                c2, z = "%s act=%d" % (case, act), zs[act]
                emit("backward_reduce_nhwc", c2, lib.skd_abn_backward_reduce_nhwc(rows, C, p(z), p(dz), p(w), p(b), p(e), p(ey), 1e-5, act, 0.01, p(ws), st), e, ey)
                for acc in (0, 1):
                    emit("backward_dx_nhwc", "%s acc=%d" % (c2, acc), lib.skd_abn_backward_dx_nhwc(
                        rows, C, p(z), p(dz), p(v), p(w), p(b), p(e), p(ey), p(dx), p(dw) if affine else None, p(db), 1e-5, act, 0.01, acc, st), dx, dw, db)
                for fused in (1, 0):
                    lib.skd_abn_set_fused(fused)
                    emit("backward_nhwc", "%s fused=%d" % (c2, fused), lib.skd_abn_backward_nhwc(
                        rows, C, p(z), p(dz), p(v), p(w), p(b), p(e), p(ey), p(dx), p(dw) if affine else None, p(db), 1e-5, act, 0.01, 0, p(ws), st), e, ey, dx, dw, db)
            out, pdw = zs[RELU], (p(dw) if affine else None)
            emit("relu_backward_reduce_nhwc", case, lib.skd_abn_relu_backward_reduce_nhwc(rows, C, p(x), p(out), p(dz), p(m), p(v), p(e), p(ey), 1e-5, p(ws), st), e, ey)
            for rs in (None, dres):
                emit("relu_backward_dx_nhwc", "%s dres=%d" % (case, rs is not None), lib.skd_abn_relu_backward_dx_nhwc(
                    rows, C, p(x), p(out), p(dz), p(m), p(v), p(w), p(e), p(ey), p(dx), p(rs), pdw, p(db), 1e-5, 0, st), dx, dres, dw, db)
            emit("relu_backward_reduce_nhwc_x", case, lib.skd_abn_relu_backward_reduce_nhwc_x(rows, C, p(x), p(dz), p(m), p(v), p(w), p(b), p(e), p(ey), 1e-5, p(ws), st), e, ey)
            emit("relu_backward_dx_nhwc_x", case, lib.skd_abn_relu_backward_dx_nhwc_x(rows, C, p(x), p(dz), p(m), p(v), p(w), p(b), p(e), p(ey), p(dx), pdw, p(db), 1e-5, 1, st), dx, dw, db)
            for fused in (1, 0):
                lib.skd_abn_set_fused(fused)
                for o, rs in ((None, None), (out, None), (out, dres)):
                    emit("relu_backward_nhwc", "%s out=%d dres=%d fused=%d" % (case, o is not None, rs is not None, fused), lib.skd_abn_relu_backward_nhwc(
                        rows, C, p(x), p(o), p(dz), p(m), p(v), p(w), p(b), p(e), p(ey), p(dx), p(rs), pdw, p(db), 1e-5, 0, p(ws), st), e, ey, dx, dres, dw, db)
        lib.skd_abn_set_fused(-1)

    def stem(B, C, H, W):
        torch.manual_seed(B * H + W + C)
        OH, OW, case = H // 2 + 1, W // 2 + 1, "B=%d C=%d H=%d W=%d" % (B, C, H, W)
        x, w, b, m, v = rnd(B, H, W, C), rnd(C), rnd(C), rnd(C) * 0.1, torch.rand(C, device=dev) + 0.5
        pooled, arg, dy = new(B, OH, OW, C), torch.zeros(B, OH, OW, C, dtype=torch.uint8, device=dev), rnd(B, OH, OW, C)
        e, ey, dw, db, dx, ws = new(C), new(C), new(C), new(C), torch.zeros_like(x), new(lib.skd_abn_nhwc_workspace_floats(B * H * W, C))
        emit("relu_maxpool3x3s2_nhwc", case, lib.skd_abn_relu_maxpool3x3s2_nhwc(B, C, H, W, OH, OW, p(x), p(m), p(v), p(w), p(b), 1e-5, p(pooled), p(arg), st), pooled, arg)
        emit("relu_maxpool3x3s2_backward_reduce_nhwc", case, lib.skd_abn_relu_maxpool3x3s2_backward_reduce_nhwc(
            B, C, H, W, OH, OW, p(x), p(dy), p(arg), p(m), p(v), p(w), p(b), p(e), p(ey), 1e-5, p(ws), st), e, ey)
        for acc in (0, 1):
            emit("relu_maxpool3x3s2_backward_dx_nhwc", "%s acc=%d" % (case, acc), lib.skd_abn_relu_maxpool3x3s2_backward_dx_nhwc(
                B, C, H, W, OH, OW, p(x), p(dy), p(arg), p(m), p(v), p(w), p(b), p(e), p(ey), p(dx), p(dw), p(db), 1e-5, acc, st), dx, dw, db)

    def nchw(N, C, S, off):
        torch.manual_seed(N * 1000 + C * 10 + off)
        n = N * C * S
        buf = lambda fill=None: (rnd(n + 4) if fill is None else new(n + 4))[off:off + n]       # every tensor shares the 16-byte phase
        x, r, dz, out, y, dx, dres = buf(), buf(), buf(), buf(0), buf(0), buf(0), buf(0)
        dup = lambda t: buf(0).copy_(t)
        ws = new(lib.skd_abn_workspace_floats(N, C, S))
        for affine in (True, False):
            w, b = (rnd(C), rnd(C)) if affine else (None, None)
            case = "N=%d C=%d S=%d off=%d affine=%d" % (N, C, S, off, affine)
            m, v, e, ey, dw, db = (new(C) for _ in range(6))
            pdw = p(dw) if affine else None
            emit("stats", case, lib.skd_abn_stats(N, C, S, p(x), p(m), p(v), p(ws), st), m, v)
            emit("bn_mean_var", case, lib.skd_bn_mean_var(N, C, S, p(x), p(m), p(v), st), m, v)
            emit("bn_forward(y, z)", case, lib.skd_bn_forward(N, C, S, p(x), p(m), p(v), p(w), p(b), p(y), p(out), 1e-5, st), y, out)
            zs = {}
            for act in (NONE, LEAKY, ELU, RELU):
                c2, t = "%s act=%d" % (case, act), dup(x)
                emit("apply", c2, lib.skd_abn_apply(N, C, S, p(t), p(m), p(v), p(w), p(b), 1e-5, act, 0.01, st), t)
                rm, rv, t = new(C), new(C) + 1, dup(x)
                emit("forward_train", c2, lib.skd_abn_forward_train(N, C, S, p(t), p(w), p(b), p(rm), p(rv), p(m), p(v), 0.1, 1e-5, act, 0.01, p(ws), st), t, rm, rv, m, v)
                zs[act] = t
                for res in (None, r) if act != ELU else (None,):
                    c3 = "%s res=%d" % (c2, res is not None)
                    emit("apply_to", c3, lib.skd_abn_apply_to(N, C, S, p(x), p(res), p(out), p(m), p(v), p(w), p(b), 1e-5, act, 0.01, st), out)
                    emit("forward_train_to", c3, lib.skd_abn_forward_train_to(
                        N, C, S, p(x), p(res), p(out), p(w), p(b), p(rm), p(rv), p(m), p(v), 0.1, 1e-5, act, 0.01, p(ws), st), out, rm, rv, m, v)
                    if res is not None:
                        t = dup(x)
                        emit("apply_residual", c3, lib.skd_abn_apply_residual(N, C, S, p(t), p(res), p(m), p(v), p(w), p(b), 1e-5, act, 0.01, st), t)
            for act in (NONE, LEAKY, ELU):
                c2, z = "%s act=%d" % (case, act), zs[act]
                emit("backward_reduce", c2, lib.skd_abn_backward_reduce(N, C, S, p(z), p(dz), p(w), p(b), p(e), p(ey), 1e-5, act, 0.01, p(ws), st), e, ey)
                emit("backward_dx", c2, lib.skd_abn_backward_dx(N, C, S, p(z), p(dz), p(v), p(w), p(b), p(e), p(ey), p(dx), pdw, p(db), 1e-5, act, 0.01, st), dx, dw, db)
                for tr in (1, 0):
                    emit("backward", "%s training=%d" % (c2, tr), lib.skd_abn_backward(
                        N, C, S, p(z), p(dz), p(v), p(w), p(b), p(e), p(ey), p(dx), pdw, p(db), 1e-5, act, 0.01, tr, p(ws), st), e, ey, dx, dw, db)
            z = zs[NONE]
            emit("bn_edz_eydz", case, lib.skd_bn_edz_eydz(N, C, S, p(z), p(dz), p(w), p(b), p(e), p(ey), 1e-5, st), e, ey)
            emit("bn_backward", case, lib.skd_bn_backward(N, C, S, p(dz), p(z), p(v), p(w), p(b), p(e), p(ey), p(dx), pdw, p(db), 1e-5, st), dx, dw, db)
            o = zs[RELU]
            emit("relu_backward_reduce", case, lib.skd_abn_relu_backward_reduce(N, C, S, p(x), p(o), p(dz), p(m), p(v), p(e), p(ey), 1e-5, p(ws), st), e, ey)
            for rs in (None, dres):
                emit("relu_backward_dx", "%s dres=%d" % (case, rs is not None), lib.skd_abn_relu_backward_dx(
                    N, C, S, p(x), p(o), p(dz), p(m), p(v), p(w), p(e), p(ey), p(dx), p(rs), pdw, p(db), 1e-5, st), dx, dres, dw, db)
        a, g = dup(x), dup(dz)
        emit("leaky_relu_backward", case, lib.skd_leaky_relu_backward(n, p(a), p(g), 0.01, st), g)
        emit("leaky_relu", case, lib.skd_leaky_relu(n, p(a), 0.01, st), a)
        a, g = dup(x), dup(dz)
        emit("elu", case, lib.skd_elu(n, p(a), st), a)
        emit("elu_backward", case, lib.skd_elu_backward(n, p(a), p(g), st), g)
        emit("elu_inv", case, lib.skd_elu_inv(n, p(a), st), a)

    for N, C, S, off in NCHW:
        nchw(N, C, S, off)
    for rows, C in RAGGED:
        nhwc(rows, C, True)
    for rows, C in STUDENT:
        nhwc(rows, C, False)
    stem(2, 64, 17, 19)
    stem(2, 128, 32, 32)


if __name__ == "__main__":
    main()
