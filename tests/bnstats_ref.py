"""numpy restatement of the batch-norm statistics a split-core 3x3 convolution emits from its epilogue (include/skd_bnstats.h):
the per-block record of csrc/conv3x3.hip (block_stats) and the fixed-order combine of csrc/abn_nhwc.hip
(abn_stats_from_partials_kernel), operation for operation, in the kernels' precisions -- fp32 records, a double-precision
combine.  (The one liberty: the fused multiply-add of the squared deviations is a float64 product and sum rounded to fp32 once,
which differs from a true fma only where the float64 sum itself rounds.)"""
import numpy as np

BLOCK = 32
RUNS = 128
# the row of accumulator register q in the lower lane half; the upper half holds the rows four below (store_block's map)
LOW_ROWS = np.array([(q & 3) + 8 * (q >> 2) for q in range(16)])


def workspace_floats(m, cout):
    return -(-m // BLOCK) * cout * 2


def block_records(y):
    """``y`` (M, C) fp32 -> records (ceil(M / 32), C, 2) fp32: (mean, M2) of every 32-row block and channel."""
    y = np.asarray(y, dtype=np.float32)
    m, c = y.shape
    nb = -(-m // BLOCK)
    out = np.zeros((nb, c, 2), dtype=np.float32)
    for b in range(nb):
        left = min(BLOCK, m - BLOCK * b)
        blk = np.zeros((BLOCK, c), dtype=np.float32)
        blk[:left] = y[BLOCK * b:BLOCK * b + left]
        live = np.arange(BLOCK) < left
        halves = []
        for rows in (LOW_ROWS, LOW_ROWS + 4):
            s = np.zeros(c, dtype=np.float32)
            for r in rows:                                    # one chain per lane, rows beyond M add zero
                s = (s + (blk[r] if live[r] else np.float32(0))).astype(np.float32)
            halves.append(s)
        mean = ((halves[0] + halves[1]).astype(np.float32) / np.float32(left)).astype(np.float32)
        parts = []
        for rows in (LOW_ROWS, LOW_ROWS + 4):
            q = np.zeros(c, dtype=np.float32)
            for r in rows:
                d = (blk[r] - mean).astype(np.float32) if live[r] else np.zeros(c, dtype=np.float32)
                q = (d.astype(np.float64) * d.astype(np.float64) + q.astype(np.float64)).astype(np.float32)
            parts.append(q)
        out[b, :, 0] = mean
        out[b, :, 1] = (parts[0] + parts[1]).astype(np.float32)
    return out


def combine(records, rows, running_mean=None, running_var=None, momentum=0.1):
    """records (nb, C, 2) fp32 of a tensor of ``rows`` rows -> (mean, biased var[, running_mean, running_var]) fp32: float64 sums
    shifted by the pivot K = block 0's mean over 128 interleaved runs of blocks (run r: blocks r, r + 128, ...), the 8 runs of a
    wave added as a balanced tree, the 16 waves in turn."""
    rec = np.asarray(records, dtype=np.float32).astype(np.float64)
    nb, c, _ = rec.shape
    assert nb == -(-rows // BLOCK)
    counts = np.full(nb, float(BLOCK))
    counts[-1] = rows - BLOCK * (nb - 1)
    pivot = rec[0, :, 0]
    a1, a2 = np.zeros((RUNS, c)), np.zeros((RUNS, c))
    for r in range(RUNS):
        for b in range(r, nb, RUNS):
            d = rec[b, :, 0] - pivot
            a1[r] = a1[r] + counts[b] * d
            a2[r] = a2[r] + (rec[b, :, 1] + counts[b] * d * d)
    s1, s2 = np.zeros(c), np.zeros(c)
    for w in range(RUNS // 8):
        t1, t2 = a1[8 * w:8 * w + 8].copy(), a2[8 * w:8 * w + 8].copy()
        for stride in (1, 2, 4):
            for j in range(0, 8, 2 * stride):
                t1[j], t2[j] = t1[j] + t1[j + stride], t2[j] + t2[j + stride]
        s1, s2 = s1 + t1[0], s2 + t2[0]
    d = s1 / float(rows)
    mean = (pivot + d).astype(np.float32)
    var = np.maximum((s2 - s1 * d) / float(rows), 0.0).astype(np.float32)
    if running_mean is None:
        return mean, var
    mom, one = np.float32(momentum), np.float32(1)
    nf = np.float32(rows)
    unbiased = (var * nf / (nf - one)).astype(np.float32) if rows > 1 else var
    rm = (np.asarray(running_mean, np.float32) * (one - mom) + mom * mean).astype(np.float32)
    rv = (np.asarray(running_var, np.float32) * (one - mom) + mom * unbiased).astype(np.float32)
    return mean, var, rm, rv


def float64_stats(y, running_mean=None, running_var=None, momentum=0.1):
    """The float64 statistics of ``y`` (M, C) the kernels are checked against: mean, biased var and the running update."""
    y = np.asarray(y, dtype=np.float64)
    rows = y.shape[0]
    mean, var = y.mean(0), y.var(0)
    if running_mean is None:
        return mean, var
    unbiased = var * rows / (rows - 1) if rows > 1 else var
    return (mean, var, np.asarray(running_mean, np.float64) * (1 - momentum) + momentum * mean,
            np.asarray(running_var, np.float64) * (1 - momentum) + momentum * unbiased)


# the project's bounds for its statistics kernels (tests/test_kernels_gpu.py), each relative to max|want|
BOUNDS = dict(mean=2e-5, var=5e-5, running_mean=2e-6, running_var=1e-5)


def rel_err(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / max(float(np.abs(want).max()), 1e-300))
