"""Numpy / torch restatement of the OHEM criterion (reference utils/criterion.py:11-90, 190-209), written from the arithmetic
alone (test infrastructure: tests/golden/make_golden_ohem.py, tests/test_ohem_cpu.py, tests/test_ohem_gpu.py).

The threshold, at 1 / factor resolution (``scipy.ndimage.zoom`` in its default ``mode='constant'``):
  * output length ``round(n * (1.0 / factor))``, half to even; output index k sits at ``k * ((n_in - 1) / (n_out - 1))`` in
    float64; a coordinate ABOVE ``n_in - 1`` is outside the input and yields 0 in both orders (256 -> 32 zeroes the last line);
  * order 0 (the target): the element at ``floor(cc + 0.5)``, clamped to ``n_in - 1``;
  * order 1 (the softmax): weights ``t = cc - floor(cc)``, ``(1 - t, t)``, the float64 sum
    ``p00*wy0*wx0 + p01*wy0*wx1 + p10*wy1*wx0 + p11*wy1*wx1`` in that order, one cast to float32 (tests/multiscale_ref.py);
  * ``pred_ds`` = the zoomed probability of the zoomed label where that label is not ignored; ``mk = min_kept // factor**2``;
    threshold 1.0 when ``mk >= num_valid``, else ``thresh``, or the ``mk``-th smallest ``pred_ds`` when ``mk > 0`` and it is
    greater than ``thresh``.  Every comparison in float32.
The loss: a main-head pixel is kept iff it is valid and ``float32(p_label) <= threshold``; mean of ``-log p`` over the kept
pixels (main) + aux_weight * mean over the valid pixels (dsn); NaN when nothing is kept.

Where the reference is free to differ in float32 -- the up-sampling, the softmax, the logarithm -- this file works in float64
and rounds the label probability to float32 once (``label_probability``).  ``probs32`` replaces that probability by one
computed elsewhere (the generator passes the reference's own fp32 softmax, and must then reproduce the reference's threshold
and mask exactly); ``kept`` replaces the mask (the GPU tests evaluate the loss on the mask the kernel chose: a pixel whose
probability lies within rounding of the threshold may fall either way, tests/kinks.py).
"""
import types

import numpy as np
import torch
import torch.nn.functional as F


def zoom_size(n, factor):
    return int(round(int(n) * (1.0 / float(factor))))


def zoom_axis(n_in, n_out):
    """float64 coordinates of one axis: (i0, i1, w0, w1, nearest, inside)."""
    step = np.float64(n_in - 1) / np.float64(n_out - 1) if n_out > 1 else np.float64(0.0)
    cc = np.arange(n_out, dtype=np.float64) * step
    inside = cc <= n_in - 1
    fl = np.floor(cc)
    t = cc - fl
    i0 = np.clip(fl.astype(np.int64), 0, n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    near = np.clip(np.floor(cc + 0.5).astype(np.int64), 0, n_in - 1)
    return i0, i1, 1.0 - t, t, near, inside


def zoom_nearest(a, Ho, Wo):
    """(..., H, W) -> (..., Ho, Wo): scipy.ndimage.zoom(order=0) over the last two axes."""
    a = np.asarray(a)
    _, _, _, _, ny, iny = zoom_axis(a.shape[-2], Ho)
    _, _, _, _, nx, inx = zoom_axis(a.shape[-1], Wo)
    out = a[..., ny, :][..., nx]
    return np.where(iny[:, None] & inx[None, :], out, np.zeros((), dtype=a.dtype))


def zoom_linear(p, Ho, Wo):
    """(..., H, W) fp32 -> (..., Ho, Wo) fp32: scipy.ndimage.zoom(order=1) over the last two axes."""
    p = np.ascontiguousarray(p, dtype=np.float32).astype(np.float64)
    y0, y1, wy0, wy1, _, iny = zoom_axis(p.shape[-2], Ho)
    x0, x1, wx0, wx1, _, inx = zoom_axis(p.shape[-1], Wo)
    wy0, wy1 = wy0[:, None], wy1[:, None]
    wx0, wx1 = wx0[None, :], wx1[None, :]
    r0, r1 = p[..., y0, :], p[..., y1, :]
    out = r0[..., x0] * wy0 * wx0 + r0[..., x1] * wy0 * wx1 + r1[..., x0] * wy1 * wx0 + r1[..., x1] * wy1 * wx1
    return np.where(iny[:, None] & inx[None, :], out, 0.0).astype(np.float32)


def upsample_matrix(n_in, n_out):
    """(n_out, n_in) float64 matrix of the align-corners bilinear up-sampling of one axis with PyTorch's fp32 index / weight
    arithmetic (upsample_bilinear2d; ``tap_of`` of csrc/ce_dev.hpp): scale = (in - 1) / (out - 1), src = scale * dst,
    i0 = (int)src, l1 = src - i0, l0 = 1 - l1, every step in float32.  The weights are part of the function, not of its
    rounding: they are taken as fp32 values, the sums that use them are float64."""
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0.0)
    src = (scale * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    l0 = (np.float32(1.0) - l1).astype(np.float32)
    m = np.zeros((n_out, n_in), dtype=np.float64)
    rows = np.arange(n_out)
    np.add.at(m, (rows, i0), l0.astype(np.float64))
    np.add.at(m, (rows, i1), l1.astype(np.float64))
    return torch.from_numpy(m)


def upsampled_log_softmax(logits, size):
    """(B, C, h, w) -> float64 log-softmax of the align-corners bilinear up-sampling to ``size``, as a torch tensor that
    carries autograd when ``logits`` does."""
    lg = logits if torch.is_tensor(logits) else torch.from_numpy(np.asarray(logits))
    lg = lg.double()
    if tuple(lg.shape[2:]) != tuple(size):
        lg = torch.einsum("Yy,bcyx,Xx->bcYX", upsample_matrix(lg.shape[2], size[0]), lg, upsample_matrix(lg.shape[3], size[1]))
    return F.log_softmax(lg, dim=1)


def label_probability(logp, target, ignore_index):
    """float64 probability of each pixel's own label, (B, H, W); 0 where the label is ignored or no class."""
    C = logp.shape[1]
    t = torch.as_tensor(np.asarray(target)).long()
    ok = (t != ignore_index) & (t >= 0) & (t < C)
    idx = torch.where(ok, t, torch.zeros_like(t))
    p = logp.detach().exp().gather(1, idx[:, None])[:, 0]
    return torch.where(ok, p, torch.zeros_like(p)).numpy()


def find_threshold(prob_of, target, ignore_index, thresh, min_kept, factor):
    """``prob_of(label_ds)``: fp32 probabilities of class ``label_ds`` (B, Hd, Wd) zoomed to the down-sampled grid.
    Returns (threshold float32, num_valid, pred_ds (B, Hd, Wd) fp32 with -1 where ignored)."""
    target = np.asarray(target)
    B, H, W = target.shape
    Hd, Wd = zoom_size(H, factor), zoom_size(W, factor)
    assert Hd >= 1 and Wd >= 1 and not (Hd == 1 and H > 1) and not (Wd == 1 and W > 1)
    label_ds = zoom_nearest(target, Hd, Wd).astype(np.int64)
    valid = label_ds != ignore_index
    pred = prob_of(label_ds).astype(np.float32)
    pred_ds = np.where(valid, pred, np.float32(-1.0)).astype(np.float32)
    num_valid = int(valid.sum())
    mk = int(min_kept) // (int(factor) * int(factor))
    th32 = np.float32(thresh)
    if mk >= num_valid:
        return np.float32(1.0), num_valid, pred_ds
    threshold = th32
    if mk > 0:
        keys = np.sort(pred[valid])
        kth = keys[min(num_valid, mk) - 1]
        if kth > th32:
            threshold = np.float32(kth)
    return threshold, num_valid, pred_ds


def ohem(logits_main, logits_dsn, target, ignore_index=255, thresh=0.7, min_kept=100000, factor=8, aux_weight=0.4,
         kept=None, probs32=None, threshold=None):
    """The whole criterion.  logits (B, C, h, w) fp32 arrays / tensors (``logits_dsn`` None: single head), target (B, H, W).
    ``probs32``: (B, C, H, W) fp32 softmax to use for the threshold and the mask instead of this file's float64 one.
    ``kept``: (B, H, W) bool mask to use instead of this file's.  ``threshold``: use this threshold for the mask.
    Returns a namespace: threshold (np.float32), num_valid, pred_ds, p_label (B, H, W float64: the probability the mask was
    decided on), kept (bool), n_kept, loss, loss_main, loss_dsn (floats), grad_main, grad_dsn (float64 arrays or None)."""
    target = np.asarray(target).astype(np.int64)
    B, H, W = target.shape
    lm = torch.as_tensor(np.asarray(logits_main, dtype=np.float32)).double().requires_grad_(True)
    C = lm.shape[1]
    logp = upsampled_log_softmax(lm, (H, W))
    valid = target != ignore_index
    if probs32 is None:
        p_label = label_probability(logp, target, ignore_index)

        def prob_of(label_ds):
            # the zoom of the (B, C, H, W) softmax read at class label_ds: only the four pixels around each coordinate matter
            full = logp.detach().exp().numpy().astype(np.float32)
            z = zoom_linear(full, label_ds.shape[1], label_ds.shape[2])
            return np.take_along_axis(z, np.clip(label_ds, 0, C - 1)[:, None], axis=1)[:, 0]
    else:
        probs32 = np.asarray(probs32, dtype=np.float32)
        idx = np.where(valid, np.clip(target, 0, C - 1), 0)
        p_label = np.where(valid, np.take_along_axis(probs32, idx[:, None], axis=1)[:, 0], 0).astype(np.float64)

        def prob_of(label_ds):
            z = zoom_linear(probs32, label_ds.shape[1], label_ds.shape[2])
            return np.take_along_axis(z, np.clip(label_ds, 0, C - 1)[:, None], axis=1)[:, 0]
    th, num_valid, pred_ds = find_threshold(prob_of, target, ignore_index, thresh, min_kept, factor)
    if threshold is not None:
        th = np.float32(threshold)
    own = valid & (p_label.astype(np.float32) <= th)
    mask = own if kept is None else (np.asarray(kept).astype(bool) & valid)
    tt = torch.from_numpy(np.where(valid, np.clip(target, 0, C - 1), 0))
    nll = -logp.gather(1, tt[:, None])[:, 0]
    n_kept = int(mask.sum())
    loss_main = (nll * torch.from_numpy(mask)).sum() / n_kept if n_kept else nll.sum() * float("nan")
    total = loss_main
    ld = None
    loss_dsn = None
    if logits_dsn is not None:
        ld = torch.as_tensor(np.asarray(logits_dsn, dtype=np.float32)).double().requires_grad_(True)
        nll_d = -upsampled_log_softmax(ld, (H, W)).gather(1, tt[:, None])[:, 0]
        nv = int(valid.sum())
        loss_dsn = (nll_d * torch.from_numpy(valid)).sum() / nv if nv else nll_d.sum() * float("nan")
        total = loss_main + aux_weight * loss_dsn
    total.backward()
    return types.SimpleNamespace(
        threshold=th, num_valid=num_valid, pred_ds=pred_ds, p_label=p_label, kept=mask, own_kept=own, n_kept=n_kept,
        loss=float(total.detach()), loss_main=float(loss_main.detach()),
        loss_dsn=None if loss_dsn is None else float(loss_dsn.detach()),
        grad_main=lm.grad.numpy(), grad_dsn=None if ld is None else ld.grad.numpy())
