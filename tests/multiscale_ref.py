"""Numpy restatement of multi-scale / flip evaluation (reference networks/evaluate.py:115-134, 187-198), written from the
arithmetic alone.

The resize is ``scipy.ndimage.zoom(order=1, prefilter=False)`` in its default ``mode='constant'``: the output length is
Python's ``round(n * scale)`` (half to even); output index k sits at ``k * ((n_in - 1) / (n_out - 1))`` in float64, and a
coordinate above ``n_in - 1`` is OUTSIDE (the whole line is zero, which happens to the LAST line of some sizes when the
product rounds up); weights ``t = cc - floor(cc)``, ``(1 - t, t)``; the float64 sum
``p00*wy0*wx0 + p01*wy0*wx1 + p10*wy1*wx0 + p11*wy1*wx1`` in that order, each product left to right; one cast to float32.

The tail: per scale the fp32 align-corners upsample of tests/sliding_ref.py (``upsample``), the fp32 flip average
``0.5 * (a + b[:, ::-1])``, float64 sum in scale order, float64 divide by the number of scales, first-maximum argmax.

Used by tests/golden/make_golden_multiscale.py (to check a fixture before it is written), by the CPU tests (against scipy
and the reference's recorded outputs) and by the GPU tests (bit-exact yardstick of csrc/evaluate_multiscale.hip).
``MultiscaleDouble`` serves ``skd_zoom_linear`` and ``skd_seg_multiscale`` (include/skd_eval_ms.h) on raw HOST addresses
behind ``_lib.install_test_backend``, composed over ``SlidingDouble`` and the plain-C double of oracle/."""
import ctypes

import numpy as np

from sliding_ref import SlidingDouble, _host, confusion, upsample  # noqa: F401  (confusion: re-exported for the tests)


def zoom_size(n, scale):
    return int(round(n * float(scale)))


def _zoom_axis(n_in, n_out):
    """float64 coordinates of one axis: (i0, i1, w0, w1, inside)."""
    step = np.float64(n_in - 1) / np.float64(n_out - 1)
    cc = np.arange(n_out, dtype=np.float64) * step
    inside = cc <= n_in - 1
    fl = np.floor(cc)
    t = cc - fl
    i0 = np.clip(fl.astype(np.int64), 0, n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, 1.0 - t, t, inside


def zoom_linear(img, Ho, Wo):
    """(C, H, W) fp32 -> (C, Ho, Wo) fp32; Ho, Wo >= 2."""
    p = np.ascontiguousarray(img, dtype=np.float32).astype(np.float64)
    assert p.ndim == 3 and Ho >= 2 and Wo >= 2
    y0, y1, wy0, wy1, iny = _zoom_axis(p.shape[1], Ho)
    x0, x1, wx0, wx1, inx = _zoom_axis(p.shape[2], Wo)
    wy0, wy1 = wy0[None, :, None], wy1[None, :, None]
    wx0, wx1 = wx0[None, None, :], wx1[None, None, :]
    out = (p[:, y0][:, :, x0] * wy0 * wx0 + p[:, y0][:, :, x1] * wy0 * wx1
           + p[:, y1][:, :, x0] * wy1 * wx0 + p[:, y1][:, :, x1] * wy1 * wx1)
    out = np.where(iny[None, :, None] & inx[None, None, :], out, 0.0)
    return out.astype(np.float32)


def zero_lines(n_in, n_out):
    """Whether the last line of an axis resized from n_in to n_out is outside the input (and therefore zero)."""
    return not bool(_zoom_axis(n_in, n_out)[4][-1])


def scale_value(logits, flip, out_size):
    """One scale's (H, W, C) fp32 contribution: ``logits`` (F, C, h, w), element 1 the forward of the mirrored image."""
    a = upsample(logits[0], out_size).transpose(1, 2, 0)
    if not flip:
        return a
    b = upsample(logits[1], out_size).transpose(1, 2, 0)
    v = np.float32(0.5) * (a + b[:, ::-1, :])
    assert v.dtype == np.float32
    return v


def multiscale(logits_per_scale, flip, out_size):
    """[(F, C, h_s, w_s) fp32 per scale] -> (probs (H, W, C) float64, pred (H, W) uint8)."""
    H, W = out_size
    C = logits_per_scale[0].shape[1]
    total = np.zeros((H, W, C), dtype=np.float64)
    for lg in logits_per_scale:
        lg = np.asarray(lg, dtype=np.float32)
        assert lg.shape[0] == (2 if flip else 1) and lg.shape[1] == C
        total += scale_value(lg, flip, (H, W))
    probs = total / np.float64(len(logits_per_scale))
    return probs, np.argmax(probs, axis=2).astype(np.uint8)


class MultiscaleDouble(SlidingDouble):
    """``SlidingDouble`` + the two entries of include/skd_eval_ms.h as the restatement above, on raw HOST addresses."""

    def __init__(self, core):
        super().__init__(core)
        self.zoom_calls = 0
        self.ms_calls = 0
        self.confusion_calls = 0

    def skd_seg_confusion(self, *args):
        self.confusion_calls += 1
        return self._core.skd_seg_confusion(*args)

    def skd_zoom_linear(self, C, H, W, Ho, Wo, image, out, mirror, channels_last, stream):
        if min(C, H, W) <= 0 or Ho < 2 or Wo < 2 or not image or not out:
            return 0
        self.zoom_calls += 1
        z = zoom_linear(_host(image, ctypes.c_float, (C, H, W)), Ho, Wo)
        both = [z, z[:, :, ::-1]] if mirror else [z]
        for f, m in enumerate(both):
            if channels_last:
                _host(out, ctypes.c_float, (len(both), Ho, Wo, C))[f] = m.transpose(1, 2, 0)
            else:
                _host(out, ctypes.c_float, (len(both), C, Ho, Wo))[f] = m
        return 1

    def skd_seg_multiscale(self, S, F, C, H, W, logits, table, target, ignore_index, remap, pred, probs, conf, stream):
        if S <= 0 or F not in (1, 2) or not 1 <= C <= 32 or min(H, W) <= 0 or not logits or not table or (target and not conf):
            return 0
        self.ms_calls += 1
        rows = [tuple(int(v) for v in r) for r in _host(table, ctypes.c_int64, (S, 3))]
        floats = max(off + F * C * h * w for off, h, w in rows)
        flat = _host(logits, ctypes.c_float, (floats,))
        maps = [flat[off:off + F * C * h * w].reshape(F, C, h, w) for off, h, w in rows]
        p, a = multiscale(maps, F == 2, (H, W))
        if pred:
            _host(pred, ctypes.c_uint8, (H, W))[...] = a if not remap else _host(remap, ctypes.c_uint8, (256,))[a]
        if probs:
            _host(probs, ctypes.c_double, (H, W, C))[...] = p
        if target:
            _host(conf, ctypes.c_int64, (C, C))[...] += confusion(_host(target, ctypes.c_int64, (H, W)), a, C, ignore_index)
        return 1
