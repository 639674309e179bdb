"""Numpy restatement of the sliding-window evaluation tail (reference networks/evaluate.py:70-104, 187-198), written from
the arithmetic alone: fp32 bilinear align_corners upsample with individually rounded mul / add (no FMA), float64 sums in
tile order, float64 divide by the cover count, first-maximum argmax.  Used by tests/golden/make_golden_sliding.py (to
check a fixture before it is written), by the CPU tests (against the reference's recorded outputs) and by the GPU tests
(bit-exact yardstick of csrc/evaluate_sliding.hip).  ``SlidingDouble`` is the adapter that lets the restatement stand in
for ``skd_seg_sliding`` behind the C ABI (raw host addresses) next to the plain-C double of oracle/."""
import ctypes
from math import ceil

import numpy as np


def tiles_of(H, W, tile_size):
    """(y1, x1, y2, x2) windows, row-major; stride from the tile height for both axes; overhanging windows moved back."""
    th, tw = tile_size
    stride = ceil(th * (1 - 1 / 3))
    rows = int(ceil((H - th) / stride) + 1)
    cols = int(ceil((W - tw) / stride) + 1)
    out = []
    for r in range(rows):
        for c in range(cols):
            y2, x2 = min(r * stride + th, H), min(c * stride + tw, W)
            out.append((max(y2 - th, 0), max(x2 - tw, 0), y2, x2))
    return out


def cover_count(H, W, tiles):
    n = np.zeros((H, W), dtype=np.int64)
    for y1, x1, y2, x2 in tiles:
        n[y1:y2, x1:x2] += 1
    return n


def _axis(n_in, n_out):
    """Source indices and fp32 weights of one axis: scale = (in - 1) / (out - 1) in fp32, src = scale * dst."""
    f32 = np.float32
    scale = f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)
    src = scale * np.arange(n_out, dtype=np.float32)
    i0 = np.minimum(src.astype(np.int32), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(np.float32)
    l0 = f32(1) - l1
    assert src.dtype == l1.dtype == l0.dtype == np.float32
    return i0, i1, l0, l1


def upsample(logits, tile_size):
    """(C, h, w) fp32 -> (C, tile_h, tile_w) fp32:  ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d), each op rounded."""
    q = np.ascontiguousarray(logits, dtype=np.float32)
    y0, y1, ly0, ly1 = _axis(q.shape[1], tile_size[0])
    x0, x1, lx0, lx1 = _axis(q.shape[2], tile_size[1])
    ly0, ly1 = ly0[None, :, None], ly1[None, :, None]
    top = lx0 * q[:, y0][:, :, x0] + lx1 * q[:, y0][:, :, x1]
    bot = lx0 * q[:, y1][:, :, x0] + lx1 * q[:, y1][:, :, x1]
    out = ly0 * top + ly1 * bot
    assert out.dtype == np.float32
    return out


def sliding(logits, tiles, tile_size, out_size):
    """(T, C, h, w) fp32 logits -> (probs (H, W, C) float64, pred (H, W) uint8)."""
    H, W = out_size
    C = logits.shape[1]
    total = np.zeros((H, W, C), dtype=np.float64)
    for t, (y1, x1, y2, x2) in enumerate(tiles):
        up = upsample(logits[t], tile_size)[:, :y2 - y1, :x2 - x1]
        total[y1:y2, x1:x2] += up.transpose(1, 2, 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        probs = total / cover_count(H, W, tiles)[:, :, None].astype(np.float64)
    return probs, np.argmax(probs, axis=2).astype(np.uint8)


def confusion(target, pred, C, ignore_index=255):
    keep = (target != ignore_index) & (target >= 0) & (target < C)
    idx = target[keep].astype(np.int64) * C + pred[keep].astype(np.int64)
    return np.bincount(idx, minlength=C * C).reshape(C, C).astype(np.int64)


def _host(addr, ctype, shape):
    n = int(np.prod(shape))
    return np.ctypeslib.as_array(ctypes.cast(ctypes.c_void_p(addr), ctypes.POINTER(ctype)), shape=(n,)).reshape(shape)


class SlidingDouble:
    """The plain-C double of oracle/ for every core entry + the restatement above as ``skd_seg_sliding`` on raw HOST
    addresses (include/skd_eval.h), for ``_lib.install_test_backend``."""

    def __init__(self, core):
        self._core = core
        self.calls = 0

    def __getattr__(self, name):
        return getattr(self._core, name)

    def skd_seg_sliding(self, T, C, h, w, tile_h, tile_w, H, W, logits, tiles, target, ignore_index, remap, pred, probs, conf, stream):
        if T <= 0 or not 1 <= C <= 32 or not logits or not tiles or (target and not conf):
            return 0
        self.calls += 1
        lg = _host(logits, ctypes.c_float, (T, C, h, w))
        tl = [tuple(int(v) for v in row) for row in _host(tiles, ctypes.c_int32, (T, 4))]
        p, a = sliding(lg, tl, (tile_h, tile_w), (H, W))
        if pred:
            _host(pred, ctypes.c_uint8, (H, W))[...] = a if not remap else _host(remap, ctypes.c_uint8, (256,))[a]
        if probs:
            _host(probs, ctypes.c_double, (H, W, C))[...] = p
        if target:
            _host(conf, ctypes.c_int64, (C, C))[...] += confusion(_host(target, ctypes.c_int64, (H, W)), a, C, ignore_index)
        return 1
