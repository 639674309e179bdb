"""Autograd front-ends of the loss / spectral-norm kernels in libskd_hip.so.

Each function here is the differentiable form of one reference computation, executed by the
hand-written gfx950 kernels behind the C ABI of include/skd.h (no eager fallback: CPU tensors
raise, see _lib.require_device):

    cross_entropy_dsn(m, d, y)   utils/criterion.py:179-188   csrc/ce_dsn.hip
    ce_ohem_dsn(m, d, y, ...)    utils/criterion.py:11-90, 200-209   csrc/ce_ohem.hip  (include/skd_ohem.h)
    ppm_pool / ppm_concat        networks/pspnet_combine.py:102-111   csrc/ppm.hip
    seg_confusion(logits, y)     networks/evaluate.py:106-113,186-198 csrc/evaluate.hip  (no autograd)
    pixel_wise_loss(S, T)        utils/criterion.py:219-226   csrc/pixelwise.hip
    max_pool_argmax(x, kh, kw)   nn.MaxPool2d(k=s, ceil_mode=True) of criterion.py:243   csrc/pairwise.hip
    sim_dis(f_S, f_T)            utils/utils.py:170-183 (L2, similarity, sim_dis_compute)  csrc/pairwise.hip
    spectral_normalize(W, u, v)  networks/spectral.py:23-35    csrc/spectral.hip

All are first-order only (``once_differentiable``), like the reference's native op
(libs/functions.py:112,230).  WGAN-GP's double backward (criterion.py:110-115) only needs second
derivatives of the discriminator's stock convolutions; the spectral-norm node is traversed once,
by the final ``d_loss.backward()``.
"""
import collections
import ctypes

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib


def _f32c(t, what):
    if t.dtype != torch.float32:
        raise TypeError("%s: fp32 tensors only (got %s)" % (what, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


_HEADER_OF = {name: header for header, table in _lib.ABI.items() for name in table}      # entry -> the header that declares it


def _has(*names):
    """Whether the active back-end provides every entry of ``names``."""
    return all(_lib.has_entry(n) for n in names)


def _need(*names):
    """The one refusal of an op whose back-end lacks an extension entry: NotImplementedError naming the first entry of ``names``
    that is missing and the header of include/ that declares it.  An op lists its entries in the order it uses them."""
    for name in names:
        if not _lib.has_entry(name):
            raise NotImplementedError("the active back-end does not provide %s (include/%s)" % (name, _HEADER_OF[name]))


class _PixelWise(Function):
    @staticmethod
    def forward(ctx, logits_s, logits_t):
        _lib.require_device(logits_s, logits_t)
        assert logits_s.shape == logits_t.shape, "the output dim of teacher and student differ"  # criterion.py:221
        s, t = _f32c(logits_s, "pixel_wise_loss"), _f32c(logits_t, "pixel_wise_loss")
        n, c = s.shape[0], s.shape[1]
        hw = s.numel() // max(1, n * c)
        lib, st = _lib.get(), _lib.stream_of(s)
        loss = s.new_empty(())
        need_grad = ctx.needs_input_grad[0]
        grad = torch.empty_like(s) if need_grad else None
        ws = s.new_empty((max(1, lib.skd_pixelwise_workspace_floats(n, hw)),))
        _lib.check(lib.skd_pixelwise_loss(n, c, hw, s.data_ptr(), t.data_ptr(), loss.data_ptr(),
                                          _lib.ptr(grad), ws.data_ptr(), st), "skd_pixelwise_loss")
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (grad * g if grad is not None else None), None


def pixel_wise_loss(logits_s, logits_t):
    """sum(-softmax(T) * log_softmax(S)) / W / H over the class dim of (N,C,W,H) logits; no grad to T."""
    return _PixelWise.apply(logits_s, logits_t.detach())


class _CrossEntropyDSN(Function):
    @staticmethod
    def forward(ctx, logits_main, logits_dsn, target, ignore_index, aux_weight):
        _lib.require_device(logits_main, logits_dsn, target)
        lm = _f32c(logits_main, "cross_entropy_dsn")
        ld = _f32c(logits_dsn, "cross_entropy_dsn") if logits_dsn is not None else None
        if target.dtype != torch.int64:
            raise TypeError("cross_entropy_dsn: int64 target expected (got %s)" % target.dtype)
        tg = target if target.is_contiguous() else target.contiguous()
        b, c, h, w = lm.shape
        if ld is not None and ld.shape != lm.shape:
            raise ValueError("main and dsn logits differ in shape")
        if tg.dim() != 3 or tg.shape[0] != b:
            raise ValueError("target must be (B, H, W)")
        H, W = tg.shape[1], tg.shape[2]
        lib, st = _lib.get(), _lib.stream_of(lm)
        need_m = ctx.needs_input_grad[0]
        need_d = ld is not None and ctx.needs_input_grad[1]
        loss = lm.new_empty(())
        gm = torch.empty_like(lm) if need_m else None
        gd = torch.empty_like(ld) if need_d else None
        ws = lm.new_empty((max(8, lib.skd_ce_dsn_workspace_floats(b, c, h, w, H, W)),))
        _lib.check(lib.skd_ce_dsn_forward(b, c, h, w, H, W, lm.data_ptr(), _lib.ptr(ld), tg.data_ptr(),
                                          int(ignore_index), float(aux_weight), loss.data_ptr(), _lib.ptr(gm),
                                          _lib.ptr(gd), ws.data_ptr(), st), "skd_ce_dsn_forward")
        ctx.save_for_backward(gm, gd)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        gm, gd = ctx.saved_tensors
        return (gm * g if gm is not None else None), (gd * g if gd is not None else None), None, None, None


def cross_entropy_dsn(logits_main, logits_dsn, target, ignore_index=255, aux_weight=0.4):
    """CE(up(main), target) + aux_weight * CE(up(dsn), target), up = bilinear align_corners upsample to the
    target's size, CE = mean over non-ignored pixels (utils/criterion.py:179-188) -- one fused kernel chain
    that never materialises a (B, C, H, W) tensor.  ``logits_dsn`` may be None (single CE)."""
    return _CrossEntropyDSN.apply(logits_main, logits_dsn, target, ignore_index, aux_weight)


def _ohem_inputs(logits_main, logits_dsn, target, factor, what):
    _lib.require_device(logits_main, logits_dsn, target)
    lm = _f32c(logits_main, what)
    ld = _f32c(logits_dsn, what) if logits_dsn is not None else None
    if target.dtype != torch.int64:
        raise TypeError("%s: int64 target expected (got %s)" % (what, target.dtype))
    tg = target if target.is_contiguous() else target.contiguous()
    if lm.dim() != 4 or not 1 <= lm.shape[1] <= 64:
        raise ValueError("%s: logits (B, C, h, w) with 1 <= C <= 64 expected (got %s)" % (what, tuple(lm.shape)))
    if ld is not None and ld.shape != lm.shape:
        raise ValueError("main and dsn logits differ in shape")
    if tg.dim() != 3 or tg.shape[0] != lm.shape[0]:
        raise ValueError("target must be (B, H, W)")
    factor = int(factor)
    if factor < 1:
        raise ValueError("%s: factor >= 1 expected (got %d)" % (what, factor))
    for n in tg.shape[1:]:
        nd = zoom_size(n, 1.0 / factor)
        if nd < 1 or (nd == 1 and n > 1):
            raise ValueError("%s: an axis of %d down-samples to %d at factor %d: scipy's zoom step is undefined there"
                             % (what, n, nd, factor))
    return lm, ld, tg, factor


def _ohem_threshold(lib, lm, tg, ignore_index, thresh, min_kept, factor, ws, pred_ds=None):
    """Launches skd_ohem_threshold; returns the (threshold fp32 [], num_valid int32 []) DEVICE tensors."""
    b, c, h, w = lm.shape
    threshold = lm.new_empty(())
    num_valid = torch.empty((), dtype=torch.int32, device=lm.device)
    _lib.check(lib.skd_ohem_threshold(b, c, h, w, tg.shape[1], tg.shape[2], lm.data_ptr(), tg.data_ptr(), int(ignore_index),
                                      float(thresh), int(min_kept), factor, threshold.data_ptr(), num_valid.data_ptr(),
                                      _lib.ptr(pred_ds), ws.data_ptr(), _lib.stream_of(lm)), "skd_ohem_threshold")
    return threshold, num_valid


class _CrossEntropyOhemDSN(Function):
    @staticmethod
    def forward(ctx, logits_main, logits_dsn, target, ignore_index, thresh, min_kept, factor, aux_weight):
        _need("skd_ce_ohem_workspace_floats", "skd_ohem_threshold", "skd_ce_ohem_dsn_forward")
        lm, ld, tg, factor = _ohem_inputs(logits_main, logits_dsn, target, factor, "ce_ohem_dsn")
        if int(min_kept) < 0:
            raise ValueError("ce_ohem_dsn: min_kept >= 0 expected (got %d)" % int(min_kept))
        b, c, h, w = lm.shape
        H, W = tg.shape[1], tg.shape[2]
        lib, st = _lib.get(), _lib.stream_of(lm)
        need_m = ctx.needs_input_grad[0]
        need_d = ld is not None and ctx.needs_input_grad[1]
        loss, n_kept = lm.new_empty(()), lm.new_empty(())
        gm = torch.empty_like(lm) if need_m else None
        gd = torch.empty_like(ld) if need_d else None
        ws = lm.new_empty((max(8, lib.skd_ce_ohem_workspace_floats(b, c, h, w, H, W, factor)),))
        # two entry calls on one stream; the threshold stays in device memory between them
        threshold, _ = _ohem_threshold(lib, lm, tg, ignore_index, thresh, min_kept, factor, ws)
        _lib.check(lib.skd_ce_ohem_dsn_forward(b, c, h, w, H, W, lm.data_ptr(), _lib.ptr(ld), tg.data_ptr(), int(ignore_index),
                                               float(aux_weight), threshold.data_ptr(), loss.data_ptr(), n_kept.data_ptr(),
                                               None, _lib.ptr(gm), _lib.ptr(gd), ws.data_ptr(), st), "skd_ce_ohem_dsn_forward")
        ctx.save_for_backward(gm, gd)
        ctx.mark_non_differentiable(threshold, n_kept)
        return loss, threshold, n_kept

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_threshold, _g_kept):
        gm, gd = ctx.saved_tensors
        return (gm * g if gm is not None else None), (gd * g if gd is not None else None), None, None, None, None, None, None


def ce_ohem_dsn(logits_main, logits_dsn, target, ignore_index=255, thresh=0.7, min_kept=100000, factor=8, aux_weight=0.4):
    """CriterionOhemDSN (utils/criterion.py:190-209): OHEM cross-entropy on the up-sampled main logits + ``aux_weight`` * plain
    cross-entropy on the up-sampled dsn logits (``logits_dsn`` None: the single OhemCrossEntropy2d term).  A main-head pixel
    counts iff it is valid and the softmax probability of its label is <= the threshold that OhemCrossEntropy2d.find_threshold
    derives at 1 / ``factor`` resolution (the ``min_kept // factor**2``-th smallest such probability, at least ``thresh``; 1.0
    when fewer valid pixels than that exist).  Everything runs on the device (csrc/ce_ohem.hip): nothing is copied to the
    host and nothing of size (B, C, H, W) is written.  Returns (loss, threshold, n_kept): 0-dim tensors, the last two for
    logging (no gradient)."""
    return _CrossEntropyOhemDSN.apply(logits_main, logits_dsn, target, ignore_index, thresh, min_kept, factor, aux_weight)


def ohem_threshold(logits_main, target, ignore_index=255, thresh=0.7, min_kept=100000, factor=8, want_keys=False):
    """The OHEM threshold alone (OhemCrossEntropy2d.find_threshold on the up-sampled logits' softmax), without autograd:
    (threshold fp32 [], num_valid int32 []) device tensors, and with ``want_keys`` the (B, Hd, Wd) down-sampled label
    probabilities the selection ran on (-1 where the down-sampled label is ignored)."""
    _need("skd_ce_ohem_workspace_floats", "skd_ohem_threshold")
    lm, _, tg, factor = _ohem_inputs(logits_main.detach(), None, target, factor, "ohem_threshold")
    b, c, h, w = lm.shape
    H, W = tg.shape[1], tg.shape[2]
    lib = _lib.get()
    ws = lm.new_empty((max(8, lib.skd_ce_ohem_workspace_floats(b, c, h, w, H, W, factor)),))
    keys = lm.new_empty((b, zoom_size(H, 1.0 / factor), zoom_size(W, 1.0 / factor))) if want_keys else None
    threshold, num_valid = _ohem_threshold(lib, lm, tg, ignore_index, thresh, min_kept, factor, ws, keys)
    return (threshold, num_valid, keys) if want_keys else (threshold, num_valid)


def _is_cl(t):
    """4-D, channels-last memory (and not also plain-contiguous), channel count a multiple of 4."""
    return (t.dim() == 4 and t.shape[1] % 4 == 0 and not t.is_contiguous()
            and t.is_contiguous(memory_format=torch.channels_last))


def _cl(t):
    return t if t.is_contiguous(memory_format=torch.channels_last) else t.contiguous(memory_format=torch.channels_last)


def _new_cl(ref, b, c, h, w):
    """Uninitialised (b, c, h, w) tensor with channels-last memory (b, h, w, c)."""
    return ref.new_empty((b, h, w, c), dtype=torch.float32).permute(0, 3, 1, 2)


def _fp32_cl_map(x, host_ok=True):
    """A device tensor (``host_ok``: or a host tensor under the tests' C-ABI double), fp32, 4-D, channels-last memory."""
    return ((x.is_cuda or (host_ok and _lib.test_backend_active())) and x.dtype == torch.float32 and x.dim() == 4
            and x.is_contiguous(memory_format=torch.channels_last))


# ---- the one version-keyed cache of everything derived from module tensors (folded BN operands, ABN constants, weight packs) ----
# THE RULE: a cached value is that of its tensors for as long as their addresses and autograd version counters stand.  In-place
# ops, ``load_state_dict`` and torch's plain / foreach optimizers advance ``_version``; torch's FUSED multi-tensor optimizers write
# the parameters without advancing it, so whoever trains with one registers ``networks.kd_model.advance_versions_after_step`` as a
# step post-hook on it (NetModel does, always) -- and a write through ``tensor.data`` is never seen: drop the cache by hand.

def _version_key(tensors, *extras):
    """``(data_ptr, _version, data_ptr, _version, ..., *extras)``: two entries per tensor, ``None, None`` for an absent one."""
    return tuple(v for t in tensors for v in ((None, None) if t is None else (t.data_ptr(), t._version))) + extras


def _cached(owner, attr, key, build, hold=None):
    """The tuple ``build()`` returns, cached on ``owner`` (a dict, any object that takes attributes, or None: no cache) as
    ``(key, *values)`` under ``attr`` and rebuilt when ``key`` differs.  ``hold``: a tensor whose storage is kept alive behind the
    values -- while it lives no other tensor can take its address, so a weight moved to new storage (``.to()``) can never be
    mistaken for the cached one."""
    slot = owner if isinstance(owner, dict) or owner is None else vars(owner)
    hit = slot.get(attr) if slot is not None else None
    if hit is not None and hit[0] == key:
        return hit[1:len(hit) - (hold is not None)]
    values = tuple(build())
    if slot is not None:
        slot[attr] = (key,) + values + (() if hold is None else (hold.untyped_storage(),))
    return values


def drop_conv3x3_packs(owner):
    """Forget the weight packs conv3x3_pack_weights (both piece counts, both piece formats) / conv3x3_train_packs / conv3x3_narrow_pack_weights /
    conv3x3_split_train's narrow form cached on ``owner`` (a module, or a PSPModule's ``_fold_cache`` dict, whose packs sit under
    "pack3x3" / "pack3x3_2" / "pack3x3_2h" / "pack3x3_train"; the two-plane training pairs of include/skd_train2.h and
    skd_train2h.h and the narrow fp16 image of include/skd_infer2h.h too)."""
    slot = owner if isinstance(owner, dict) else vars(owner)
    for attr in _conv3x3_slots() + ("pack3x3", "pack3x3_2", "pack3x3_2h", "pack3x3_train"):
        slot.pop(attr, None)


class _PPMPool(Function):
    """All pyramid levels of AdaptiveAvgPool2d from one read of the feature map (NCHW or channels-last)."""

    @staticmethod
    def forward(ctx, x, sizes):
        _lib.require_device(x)
        if x.dtype != torch.float32:
            raise TypeError("ppm_pool: fp32 tensors only (got %s)" % x.dtype)
        ctx.cl = _is_cl(x)
        if ctx.cl:
            b, c, h, w = x.shape
            lib, st = _lib.get(), _lib.stream_of(x)
            arr = _lib.int_array(sizes)
            total = lib.skd_ppm_pooled_floats(b * c, len(sizes), arr)
            if total <= 0:
                raise ValueError("ppm_pool: bad pyramid sizes %r" % (sizes,))
            buf = x.new_empty((total,))
            ws = x.new_empty((max(1, lib.skd_ppm_nhwc_workspace_floats(b, c, 0, h, w, len(sizes), arr)),))
            _lib.check(lib.skd_ppm_pool_nhwc(b, c, h, w, len(sizes), arr, x.data_ptr(), buf.data_ptr(), ws.data_ptr(), st),
                       "skd_ppm_pool_nhwc")
            ctx.geom = (b, c, h, w, tuple(sizes))
            outs, off = [], 0
            for s_ in sizes:
                n = b * c * s_ * s_
                outs.append(buf[off:off + n].view(b, s_, s_, c).permute(0, 3, 1, 2))     # (b, c, s, s), channels-last memory
                off += n
            return tuple(outs)
        x = _f32c(x, "ppm_pool")
        b, c, h, w = x.shape
        lib, st = _lib.get(), _lib.stream_of(x)
        arr = _lib.int_array(sizes)
        total = lib.skd_ppm_pooled_floats(b * c, len(sizes), arr)
        if total <= 0:
            raise ValueError("ppm_pool: bad pyramid sizes %r" % (sizes,))
        buf = x.new_empty((total,))
        _lib.check(lib.skd_ppm_pool(b * c, h, w, len(sizes), arr, x.data_ptr(), buf.data_ptr(), st), "skd_ppm_pool")
        ctx.geom = (b, c, h, w, tuple(sizes))
        outs, off = [], 0
        for s_ in sizes:
            n = b * c * s_ * s_
            outs.append(buf[off:off + n].view(b, c, s_, s_))
            off += n
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        b, c, h, w, sizes = ctx.geom
        ref = next(g for g in grads if g is not None)
        if ctx.cl:
            flat = torch.cat([(_cl(g).permute(0, 2, 3, 1) if g is not None else ref.new_zeros((b, s_, s_, c))).reshape(-1)
                              for g, s_ in zip(grads, sizes)]).to(torch.float32)
            dx = _new_cl(ref, b, c, h, w)
            lib, st = _lib.get(), _lib.stream_of(flat)
            _lib.check(lib.skd_ppm_pool_backward_nhwc(b, c, h, w, len(sizes), _lib.int_array(sizes), flat.data_ptr(),
                                                      dx.data_ptr(), st), "skd_ppm_pool_backward_nhwc")
            return dx, None
        flat = torch.cat([(g if g is not None else ref.new_zeros((b, c, s_, s_))).reshape(-1)
                          for g, s_ in zip(grads, sizes)]).to(torch.float32)
        dx = ref.new_empty((b, c, h, w), dtype=torch.float32)
        lib, st = _lib.get(), _lib.stream_of(flat)
        _lib.check(lib.skd_ppm_pool_backward(b * c, h, w, len(sizes), _lib.int_array(sizes), flat.data_ptr(),
                                             dx.data_ptr(), st), "skd_ppm_pool_backward")
        return dx, None


def ppm_pool(x, sizes=(1, 2, 3, 6)):
    """[AdaptiveAvgPool2d(s)(x) for s in sizes] (pspnet_combine.py:102) -- one kernel, one read of x."""
    return _PPMPool.apply(x, tuple(int(s_) for s_ in sizes))


class _PPMConcat(Function):
    """cat([upsample(p, (H, W), bilinear, align_corners=True) for p in priors] + [feats], 1)."""

    @staticmethod
    def forward(ctx, feats, *priors):
        _lib.require_device(feats, *priors)
        ctx.cl = _is_cl(feats) and feats.dtype == torch.float32 and all(p.dtype == torch.float32 and p.shape[1] % 4 == 0 for p in priors)
        if ctx.cl:
            b, cf, h, w = feats.shape
            cout = priors[0].shape[1]
            sizes = []
            for p in priors:
                if p.shape[0] != b or p.shape[1] != cout or p.shape[2] != p.shape[3]:
                    raise ValueError("ppm_concat: priors must be (B, Cout, s, s)")
                sizes.append(p.shape[2])
            priors = [_cl(p) for p in priors]                     # memory (b, s, s, cout)
            lib, st = _lib.get(), _lib.stream_of(feats)
            cat = _new_cl(feats, b, len(priors) * cout + cf, h, w)
            _lib.check(lib.skd_ppm_concat_nhwc(b, cout, cf, h, w, len(sizes), _lib.int_array(sizes), _lib.ptr_array(priors),
                                               feats.data_ptr(), cat.data_ptr(), st), "skd_ppm_concat_nhwc")
            ctx.geom = (b, cout, cf, h, w, tuple(sizes))
            return cat
        feats = _f32c(feats, "ppm_concat")
        priors = [_f32c(p, "ppm_concat") for p in priors]
        b, cf, h, w = feats.shape
        cout = priors[0].shape[1]
        sizes = []
        for p in priors:
            if p.shape[0] != b or p.shape[1] != cout or p.shape[2] != p.shape[3]:
                raise ValueError("ppm_concat: priors must be (B, Cout, s, s)")
            sizes.append(p.shape[2])
        lib, st = _lib.get(), _lib.stream_of(feats)
        cat = feats.new_empty((b, len(priors) * cout + cf, h, w))
        _lib.check(lib.skd_ppm_concat(b, cout, cf, h, w, len(sizes), _lib.int_array(sizes), _lib.ptr_array(priors),
                                      feats.data_ptr(), cat.data_ptr(), st), "skd_ppm_concat")
        ctx.geom = (b, cout, cf, h, w, tuple(sizes))
        return cat

    @staticmethod
    @once_differentiable
    def backward(ctx, gcat):
        b, cout, cf, h, w, sizes = ctx.geom
        if ctx.cl:
            gcat = _cl(gcat.to(torch.float32))
            lib, st = _lib.get(), _lib.stream_of(gcat)
            arr = _lib.int_array(sizes)
            need_p = any(ctx.needs_input_grad[1:])
            gfeats = _new_cl(gcat, b, cf, h, w) if ctx.needs_input_grad[0] else None
            gpriors = [_new_cl(gcat, b, cout, s_, s_) for s_ in sizes] if need_p else None
            ws = gcat.new_empty((max(1, lib.skd_ppm_nhwc_workspace_floats(b, 0, cout, h, w, len(sizes), arr)),)) if need_p else None
            _lib.check(lib.skd_ppm_concat_backward_nhwc(b, cout, cf, h, w, len(sizes), arr, gcat.data_ptr(),
                                                        _lib.ptr_array(gpriors) if need_p else None, _lib.ptr(gfeats),
                                                        _lib.ptr(ws), st), "skd_ppm_concat_backward_nhwc")
            return (gfeats,) + (tuple(gpriors) if need_p else (None,) * len(sizes))
        gcat = _f32c(gcat, "ppm_concat backward")
        lib, st = _lib.get(), _lib.stream_of(gcat)
        gfeats = gcat[:, len(sizes) * cout:] if ctx.needs_input_grad[0] else None
        gpriors = [None] * len(sizes)
        if any(ctx.needs_input_grad[1:]):
            gpriors = [gcat.new_empty((b, cout, s_, s_)) for s_ in sizes]
            _lib.check(lib.skd_ppm_concat_backward(b, cout, cf, h, w, len(sizes), _lib.int_array(sizes),
                                                   gcat.data_ptr(), _lib.ptr_array(gpriors), st),
                       "skd_ppm_concat_backward")
        return (gfeats,) + tuple(gpriors)


def ppm_concat(priors, feats):
    """The concatenated input of the PSP bottleneck (pspnet_combine.py:110-111): up-sampled priors followed by
    the feature map, written directly into one (B, L*Cout + Cfeat, H, W) tensor."""
    return _PPMConcat.apply(feats, *priors)


def _fold_block_ptrs(z_all, b, cout, sizes):
    """Device addresses of the diagonal blocks of Z_all: rows of level k start at B * sum_{j<k} s_j^2, its columns at
    k * 9 * Cout."""
    ptrs, row = [], 0
    ld = z_all.shape[1]
    for k, s_ in enumerate(sizes):
        ptrs.append(z_all.data_ptr() + 4 * (row * ld + k * 9 * cout))
        row += b * s_ * s_
    return (ctypes.c_void_p * len(ptrs))(*ptrs), ld


class _PPMFold(Function):
    """base += fold(Z_1 .. Z_L) (include/skd.h section 8), in place on the channels-last convolution output `base`.
    z_all: (B * sum_k s_k^2, L * 9 * Cout), the product of the stacked priors with the stacked weight blocks; level k's Z
    is its k-th diagonal block (the off-diagonal blocks are never read, and receive zero gradient)."""

    @staticmethod
    def forward(ctx, base, sizes, z_all):
        _lib.require_device(base, z_all)
        b, cout, h, w = base.shape
        if cout % 4 or not base.is_contiguous(memory_format=torch.channels_last) or base.dtype != torch.float32:
            raise ValueError("ppm_fold: base must be a float32 channels-last (B, Cout, H, W) tensor")
        rows = b * sum(s_ * s_ for s_ in sizes)
        if z_all.dtype != torch.float32 or not z_all.is_contiguous() or tuple(z_all.shape) != (rows, len(sizes) * 9 * cout):
            raise ValueError("ppm_fold: Z must be a contiguous float32 (B * sum s^2, L * 9 * Cout) tensor")
        lib, st = _lib.get(), _lib.stream_of(base)
        ptrs, ld = _fold_block_ptrs(z_all, b, cout, sizes)
        _lib.check(lib.skd_ppm_fold_nhwc(b, cout, h, w, len(sizes), _lib.int_array(sizes), ptrs, ld, base.data_ptr(), st),
                   "skd_ppm_fold_nhwc")
        ctx.geom = (b, cout, h, w, tuple(sizes))
        ctx.zshape = z_all.shape
        ctx.mark_dirty(base)
        return base

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        b, cout, h, w, sizes = ctx.geom
        gout = _cl(gout.to(torch.float32))
        gz = None
        if ctx.needs_input_grad[2]:
            lib, st = _lib.get(), _lib.stream_of(gout)
            arr = _lib.int_array(sizes)
            gz = gout.new_zeros(ctx.zshape)
            ptrs, ld = _fold_block_ptrs(gz, b, cout, sizes)
            ws = gout.new_empty((max(1, lib.skd_ppm_fold_nhwc_workspace_floats(b, cout, h, w, len(sizes), arr)),))
            _lib.check(lib.skd_ppm_fold_backward_nhwc(b, cout, h, w, len(sizes), arr, gout.data_ptr(), ptrs, ld,
                                                      ws.data_ptr(), st), "skd_ppm_fold_backward_nhwc")
        return gout if ctx.needs_input_grad[0] else None, None, gz


def ppm_fold_supported(feats, sizes):
    """True when the folded evaluation of the PSP bottleneck (ppm_fold_bottleneck) takes this feature map."""
    return (feats.is_cuda or _lib.test_backend_active()) and feats.dtype == torch.float32 and feats.dim() == 4 \
        and _is_cl(feats) and 3 * sum(sizes) <= 64 and len(sizes) <= 4


def _ppm_fold_bottleneck(priors, feats, weight, cache=None, split3x3=False, split_train=False, split_wgrad=False, pieces=3,
                         piece_format="bf16", train_fp16=False):
    """conv3x3(cat([upsample(p) for p in priors] + [feats], 1), weight, padding=1) (pspnet_combine.py:104-111) without
    the concatenated tensor and without convolving the priors' channels: the feature-map slice of the weight goes through
    the convolution, the priors through a (B s^2) x Cm x 9 Cout GEMM each and the fold kernel (csrc/ppm.hip).
    priors: (B, Cm, s, s) channels-last; feats: (B, Cf, H, W) channels-last; weight: (Cout, L*Cm + Cf, 3, 3).
    `cache` (a dict) keeps the rearranged weight slices of a frozen network between calls.  `split3x3`: run the feature-map
    convolution on csrc/conv3x3.hip when conv3x3_split_supported-style conditions hold (no grad; weights packed once in `cache`).
    `split_train`: the same for a network in training, where conv3x3_train_supported says so (conv3x3_split_train on the strided
    slice of the weight, so that autograd carries its gradient back into the full weight; packs once per weight version in `cache`).
    `split_wgrad`: with `split_train`, the weight gradient of that slice on the split core too (conv3x3_split_train's ``wgrad``).
    `pieces` = 2: with `split3x3`, the frozen feature-map convolution on the two-piece core (conv3x3_split_eval's ``pieces``), its
    pack under a key of its own in `cache`; with `split_train`, the training form on two bf16 pieces (conv3x3_split_train2,
    include/skd_train2.h), its pack pair in a slot of its own; the fold's matrix products are what they were.
    `ppm_fold_bottleneck_fp16`: that convolution on two fp16 pieces (include/skd_split2h.h), its pack under a third key.
    `ppm_fold_bottleneck_train_fp16`: with `split_train`, the training form on two fp16 pieces (conv3x3_split_train_fp16,
    include/skd_train2h.h), its pack pair in a slot of its own; a frozen call is ppm_fold_bottleneck's."""
    check_pieces(pieces, piece_format)
    import torch.nn.functional as F
    cm = priors[0].shape[1]
    n_prior = len(priors) * cm
    cout = weight.shape[0]
    sizes = tuple(int(p.shape[2]) for p in priors)
    train = bool(split_train and cache is not None and conv3x3_train_supported(feats, weight[:, n_prior:], 1, 1, 1, 1))

    def mats():
        # (the routed training form reads the slice through its strides: no channels-last copy of it per step)
        wf = None if train else weight[:, n_prior:].contiguous(memory_format=torch.channels_last)
        # (Cout, L, Cm, 3, 3) -> (Cm, L, 3, 3, Cout): column block k of the (Cm, L * 9 * Cout) matrix is level k's weights
        return wf, weight[:, :n_prior].reshape(cout, len(priors), cm, 3, 3).permute(2, 1, 3, 4, 0).reshape(cm, len(priors) * 9 * cout)
    # cached for a frozen call only: a weight that is being trained needs its matrices inside this call's graph
    frozen = not train and not (torch.is_grad_enabled() and weight.requires_grad)
    wf, w_all = _cached(cache if frozen else None, "mats", _version_key((weight,), tuple(weight.shape)), mats)
    if train:
        extra = dict(wgrad=True) if split_wgrad else {}
        train_op = conv3x3_split_train2 if pieces == 2 and piece_format == "bf16" else conv3x3_split_train
        if train_fp16:
            train_op = conv3x3_split_train_fp16
        base = train_op(feats, weight[:, n_prior:], 1, None, cache.setdefault("pack3x3_train", {}), **extra)
    elif split3x3 and cache is not None and _conv3x3_ok(feats, weight[:, n_prior:], 1, 1, 1, 1, **_FROZEN):
        if pieces == 2:
            if piece_format == "fp16":
                base = conv3x3_split_eval_fp16(feats, conv3x3_pack_weights_fp16(None, weight[:, n_prior:], cache.setdefault("pack3x3_2h", {})),
                                               cout)
            else:
                base = conv3x3_split_eval(feats, conv3x3_pack_weights(None, weight[:, n_prior:], cache.setdefault("pack3x3_2", {}), pieces=2),
                                          cout, pieces=2)
        else:
            base = conv3x3_split_eval(feats, conv3x3_pack_weights(None, weight[:, n_prior:], cache.setdefault("pack3x3", {})), cout)
    else:
        base = F.conv2d(feats, wf, None, 1, 1)
    # ONE GEMM of all levels' priors against all levels' weight blocks (only the diagonal blocks are used: 4x the
    # necessary flops of a 2 GFLOP product, but a single well-shaped library call instead of four skinny ones)
    p_all = torch.cat([_cl(p).permute(0, 2, 3, 1).reshape(-1, cm) for p in priors], 0)
    return _PPMFold.apply(base, sizes, torch.mm(p_all, w_all))


def ppm_fold_bottleneck(priors, feats, weight, cache=None, split3x3=False, split_train=False, split_wgrad=False, pieces=3):
    return _ppm_fold_bottleneck(priors, feats, weight, cache, split3x3, split_train, split_wgrad, pieces)


def ppm_fold_bottleneck_fp16(priors, feats, weight, cache=None, split3x3=False, split_train=False, split_wgrad=False):
    """``ppm_fold_bottleneck`` with the frozen feature-map convolution on two FP16 pieces (``conv3x3_split_eval_fp16``)."""
    return _ppm_fold_bottleneck(priors, feats, weight, cache, split3x3, split_train, split_wgrad, 2, "fp16")


def ppm_fold_bottleneck_train_fp16(priors, feats, weight, cache=None, split3x3=False, split_train=False, split_wgrad=False):
    """``ppm_fold_bottleneck`` whose TRAINING form runs the feature-map convolution on two FP16 pieces with a scaled gradient
    (``conv3x3_split_train_fp16``, include/skd_train2h.h); without ``split_train`` it is ``ppm_fold_bottleneck``."""
    return _ppm_fold_bottleneck(priors, feats, weight, cache, split3x3, split_train, split_wgrad, 3, "bf16", train_fp16=True)


ppm_fold_bottleneck.__doc__ = _ppm_fold_bottleneck.__doc__


class _MaxPool3x3s2(Function):
    """MaxPool2d(3, 2, 1, ceil_mode) on a channels-last tensor (csrc/maxpool.hip): one byte of argmax per element."""

    @staticmethod
    def forward(ctx, x, oh, ow):
        _lib.require_device(x)
        b, c, h, w = x.shape
        lib, st = _lib.get(), _lib.stream_of(x)
        y = _new_cl(x, b, c, oh, ow)
        need = ctx.needs_input_grad[0]
        arg = torch.empty((b, oh, ow, c), dtype=torch.uint8, device=x.device) if need else None
        _lib.check(lib.skd_maxpool3x3s2_nhwc(b, c, h, w, oh, ow, x.data_ptr(), y.data_ptr(), _lib.ptr(arg), st), "skd_maxpool3x3s2_nhwc")
        ctx.geom = (b, c, h, w, oh, ow)
        if need:
            ctx.save_for_backward(arg)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        b, c, h, w, oh, ow = ctx.geom
        (arg,) = ctx.saved_tensors
        gy = _cl(gy.to(torch.float32))
        lib, st = _lib.get(), _lib.stream_of(gy)
        dx = _new_cl(gy, b, c, h, w)
        _lib.check(lib.skd_maxpool3x3s2_backward_nhwc(b, c, h, w, oh, ow, gy.data_ptr(), arg.data_ptr(), dx.data_ptr(), st),
                   "skd_maxpool3x3s2_backward_nhwc")
        return dx, None, None


def _pool_out(n, ceil_mode):
    o = (n + 2 - 3 + (1 if ceil_mode else 0)) // 2 + 1
    if ceil_mode and (o - 1) * 2 >= n + 1:
        o -= 1
    return o


stem_pool_out = _pool_out


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def is_stem_pool(pool):
    """nn.MaxPool2d(kernel_size=3, stride=2, padding=1[, ceil_mode]) without dilation / returned indices: what csrc/maxpool.hip and
    the fused stem kernels implement."""
    return (isinstance(pool, torch.nn.MaxPool2d) and _pair(pool.kernel_size) == (3, 3) and _pair(pool.stride) == (2, 2)
            and _pair(pool.padding) == (1, 1) and _pair(pool.dilation) == (1, 1) and not pool.return_indices)


def max_pool_stem(x, pool):
    """``pool(x)`` for the stem's nn.MaxPool2d(3, 2, 1, ceil_mode=True) (pspnet_combine.py:135): channels-last fp32
    tensors take csrc/maxpool.hip, anything else the stock operator."""
    if (x.dtype == torch.float32 and _is_cl(x) and (x.is_cuda or _lib.test_backend_active()) and is_stem_pool(pool)):
        return _MaxPool3x3s2.apply(x, _pool_out(x.shape[2], pool.ceil_mode), _pool_out(x.shape[3], pool.ceil_mode))
    return pool(x)


class _Head1x1(Function):
    """The 19-class 1x1 classifier head on a channels-last feature map (csrc/head.hip): logits come out in the reference's NCHW layout
    (what the criteria and the critic consume: no layout copy), the feature gradient goes back channels-last (what the InPlace-ABN
    backward wants: no copy either), dW / db in a fixed summation order."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        _lib.require_device(x, weight, bias)
        b, k, h, w = x.shape
        c = weight.shape[0]
        lib, st = _lib.get(), _lib.stream_of(x)
        wt = weight.reshape(c, k)
        wt = wt if wt.is_contiguous() else wt.contiguous()
        out = x.new_empty((b, c, h, w))
        _lib.check(lib.skd_head1x1_forward_nhwc(b, h * w, k, c, x.data_ptr(), wt.data_ptr(), _lib.ptr(bias), out.data_ptr(), st),
                   "skd_head1x1_forward_nhwc")
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        b, k, h, w = x.shape
        c = weight.shape[0]
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        g = g if (g.dtype == torch.float32 and g.is_contiguous()) else g.to(torch.float32).contiguous()
        lib, st = _lib.get(), _lib.stream_of(x)
        wt = weight.reshape(c, k)
        wt = wt if wt.is_contiguous() else wt.contiguous()
        gx = _new_cl(x, b, k, h, w) if need_x else None
        gw = torch.empty_like(wt) if need_w else None
        gb = x.new_empty((c,)) if need_b else None
        ws = x.new_empty((max(1, lib.skd_head1x1_backward_workspace_floats(b, h * w, k, c)),))
        _lib.check(lib.skd_head1x1_backward_nhwc(b, h * w, k, c, x.data_ptr(), wt.data_ptr(), g.data_ptr(), _lib.ptr(gx), _lib.ptr(gw),
                                                 _lib.ptr(gb), ws.data_ptr(), st), "skd_head1x1_backward_nhwc")
        return gx, (gw.view_as(weight) if gw is not None else None), gb


def head1x1_supported(x, conv):
    """True when csrc/head.hip takes this classifier: an fp32 channels-last input, a plain 1x1 / stride 1 / no padding / ungrouped
    convolution with <= 20 outputs, Cin a multiple of 128 (forward) and exactly 128 when a gradient is wanted."""
    if not (x.dtype == torch.float32 and x.dim() == 4 and _is_cl(x) and (x.is_cuda or _lib.test_backend_active())):
        return False
    if not (conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.padding == (0, 0) and conv.dilation == (1, 1)
            and conv.groups == 1 and conv.padding_mode == "zeros" and conv.weight.dtype == torch.float32):
        return False
    grad = torch.is_grad_enabled() and (x.requires_grad or conv.weight.requires_grad
                                        or (conv.bias is not None and conv.bias.requires_grad))
    return bool(_lib.get().skd_head1x1_supported(conv.in_channels, conv.out_channels, 1 if grad else 0))


def head1x1(x, conv):
    """``conv(x)`` for a classifier head that head1x1_supported() accepted: (B, C, H, W) logits, NCHW-contiguous."""
    return _Head1x1.apply(x, conv.weight, conv.bias)


def blas_1x1_bn_supported(x, conv):
    """True when conv1x1_bn_blas takes this call: an fp32 channels-last input of a frozen network (no graph) and a plain
    stride-1 1x1 convolution without bias."""
    return (not torch.is_grad_enabled() and x.dtype == torch.float32 and x.dim() == 4
            and x.is_contiguous(memory_format=torch.channels_last) and conv.kernel_size == (1, 1) and conv.stride == (1, 1)
            and conv.padding == (0, 0) and conv.groups == 1 and conv.bias is None
            and conv.in_channels >= 128 and conv.out_channels >= 128)   # 256 -> 64 at 129 x 129: 97 us vs MIOpen's 64


def conv1x1_bn_blas(x, conv, bn, relu):
    """relu?(bn(conv1x1(x))) of a FROZEN network (eval-mode InPlace-ABN, pspnet_combine.py:65-72) as one library GEMM with
    the bias (+ ReLU) epilogue: a channels-last 1x1 convolution IS the plain GEMM (B*H*W, Cin) x (Cin, Cout), the
    eval-mode normalisation folds into it -- W' = W * s, b' = beta - mean * s, s = (|gamma| + eps) / sqrt(var + eps) -- and
    rocBLAS / hipBLASLt run that GEMM faster than MIOpen's implicit-GEMM convolution on the teacher's reduce layers
    (1024 -> 256 at 65 x 65, batch 8: 144 us with the epilogue vs 175 us convolution + 27 us ABN pass;
    profiles/r02d_conv1x1_blas.jsonl), exact fp32 (no xf32 on gfx950).  The folded operands are cached on the BN module
    (_cached, under THE RULE above it).
    In isolation the split-operand kernel behind conv1x1_abn_eval is now faster on most of these shapes (1024 -> 256 at
    65 x 65: 130 us against 146-155, profiles/r11_stage2_isolated.md); which of the two a frozen network's layer takes is
    networks.pspnet_combine.SPLIT_REDUCE, set by the step A/B of profiles/r12_step_ab.md (the kernel, except 512 -> 128)."""
    def fold():
        gamma = (bn.weight.abs() + bn.eps) if bn.weight is not None else torch.ones_like(bn.running_var)
        scale = gamma / torch.sqrt(bn.running_var + bn.eps)
        w2 = (conv.weight.reshape(conv.out_channels, conv.in_channels) * scale.view(-1, 1)).contiguous()
        b2 = (bn.bias if bn.bias is not None else torch.zeros_like(scale)) - bn.running_mean * scale
        return w2, b2.contiguous()
    tensors = (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var)
    w2, b2 = _cached(bn, "_blas_fold", _version_key(tensors, float(bn.eps)), fold)
    b, _, h, w = x.shape
    x2 = x.permute(0, 2, 3, 1).reshape(b * h * w, conv.in_channels)
    out = torch._addmm_activation(b2, x2, w2.t()) if relu else torch.addmm(b2, x2, w2.t())
    return out.view(b, h, w, conv.out_channels).permute(0, 3, 1, 2)


def conv1x1_abn_supported(x, conv):
    """True when the fused 1x1-convolution + eval-ABN GEMM of csrc/conv1x1.hip takes this call: fp32 channels-last
    input, a plain stride-1 1x1 convolution without bias, Cin a multiple of 16 and Cout of 128."""
    if not _fp32_cl_map(x):
        return False
    if not (conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.padding == (0, 0) and conv.groups == 1
            and conv.bias is None and conv.weight.dtype == torch.float32):
        return False
    m = x.shape[0] * x.shape[2] * x.shape[3]
    return bool(_lib.get().skd_conv1x1_abn_supported(m, conv.in_channels, conv.out_channels))


def abn_pack_eval_params(bn):
    """(4, C) = [running_mean | 1 / sqrt(running_var + eps) | |weight| + eps | bias] of an eval-mode InPlace-ABN module (the
    constants of bn.cu:146-159), cached on the module as ``bn._skd_eval_pack`` and rebuilt when any of its tensors is written
    (their autograd version counters) or moved: the frozen teacher packs each BatchNorm once.  What counts as written is THE RULE
    above _version_key: ``load_state_dict``, ordinary in-place ops and torch's plain / foreach optimizers are seen; a fused
    optimizer's step is seen only with ``kd_model.advance_versions_after_step`` registered on it (NetModel registers it; a caller
    with a fused optimizer of their own must), a write through ``tensor.data`` never: drop ``bn._skd_eval_pack`` by hand."""
    def build():
        c = bn.running_mean.numel()
        pack = bn.running_mean.new_empty((4, c))
        _lib.check(_lib.get().skd_abn_pack_eval_params(c, bn.running_mean.data_ptr(), bn.running_var.data_ptr(), _lib.ptr(bn.weight),
                                                       _lib.ptr(bn.bias), float(bn.eps), pack.data_ptr(), _lib.stream_of(pack)),
                   "skd_abn_pack_eval_params")
        return (pack,)
    return _cached(bn, "_skd_eval_pack", _version_key((bn.running_mean, bn.running_var, bn.weight, bn.bias), float(bn.eps)), build)[0]


def check_piece_format(piece_format):
    """``piece_format``: "bf16" (every form but these) or "fp16" (include/skd_split2h.h and its kin); ValueError otherwise."""
    if piece_format not in ("bf16", "fp16"):
        raise ValueError("piece_format must be 'bf16' or 'fp16', not %r" % (piece_format,))
    return piece_format


def check_pieces(pieces, piece_format="bf16"):
    """The one validator of a ``(pieces, piece_format)`` pair, here and in networks.pspnet_combine: ``pieces`` is 3 (the six
    products of the three-piece split) or 2 (three products of two pieces), ``piece_format`` "bf16" or "fp16", and fp16 pieces exist
    for ``pieces`` = 2 alone.  Returns the pair; ValueError otherwise."""
    if type(pieces) is not int or pieces not in (2, 3):      # 2.0, True, "2": anything but the integers 2 and 3
        raise ValueError("pieces must be 2 or 3, not %r" % (pieces,))
    if check_piece_format(piece_format) == "fp16" and pieces != 2:
        raise ValueError("piece_format='fp16' requires pieces=2, not pieces=%r" % (pieces,))
    return pieces, piece_format


# (plain GEMM entry, entry with the ``pro`` prologue) of the fused 1x1 + eval-ABN GEMM per (pieces, piece_format): include/skd.h,
# skd_split2.h, skd_split2h.h
_CONV1X1_ABN = {(3, "bf16"): ("skd_conv1x1_abn_nhwc", "skd_conv1x1_abn_pro_nhwc"),
                (2, "bf16"): ("skd_conv1x1_abn2_nhwc", "skd_conv1x1_abn2_pro_nhwc"),
                (2, "fp16"): ("skd_conv1x1_abn2h_nhwc", "skd_conv1x1_abn2h_pro_nhwc")}

# include/skd_planes.h: piece planes -- an activation map as the three bf16 pieces the split core's consumer reads
_PLANES_PRODUCER = "skd_conv1x1_abn_planes_nhwc"
_PLANES_ENTRIES = tuple(_lib.ABI["skd_planes.h"])


def planes_supported():
    """True when the active back-end has the seven entries of include/skd_planes.h (the tests' plain-C double has none)."""
    return _has(*_PLANES_ENTRIES)


class Planes:
    """The piece planes of a (B, C, H, W) fp32 channels-last map (include/skd_planes.h): ``data``, the byte tensor of
    skd_planes_bytes(M, C) bytes in the layout of skd_planes_offset; ``M`` = B * H * W rows, ``C`` channels, ``shape`` =
    (B, H, W, C).  Made by ``conv1x1_abn_planes_eval`` or ``planes_split``, read by ``conv3x3_split_eval`` in place
    of ``x`` and by ``planes_join``.  Holds exactly the bf16 pieces the consumer would cut from the fp32 map itself."""

    __slots__ = ("data", "M", "C", "shape")

    def __init__(self, data, M, C, shape):
        self.data, self.M, self.C, self.shape = data, int(M), int(C), tuple(int(v) for v in shape)

    @property
    def device(self):
        return self.data.device

    @property
    def requires_grad(self):
        return False


def planes_bytes(m, c):
    """skd_planes_bytes(m, c): the allocation size of the planes of an (m, c) map; ValueError for sizes the kernels refuse."""
    _need(*_PLANES_ENTRIES)
    n = ctypes.c_int64(0)
    if not _lib.get().skd_planes_bytes(int(m), int(c), ctypes.cast(ctypes.byref(n), ctypes.c_void_p)):
        raise ValueError("piece planes: unsupported map of %d rows x %d channels (channels: a multiple of 16)" % (m, c))
    return int(n.value)


def _new_planes(ref, b, h, w, c):
    """An uninitialised Planes for a (b, c, h, w) map on ``ref``'s device, allocated through torch (so it lives on the current
    stream and inside a graph capture's pool like every other temporary)."""
    m = b * h * w
    return Planes(torch.empty((planes_bytes(m, c),), dtype=torch.uint8, device=ref.device), m, c, (b, h, w, c))


def planes_split(x):
    """The piece planes of the fp32 channels-last map ``x`` (B, C, H, W), by the stand-alone kernel skd_planes_split_nhwc: for a
    map no producer wrote."""
    _need(*_PLANES_ENTRIES)
    _lib.require_device(x)
    if not _fp32_cl_map(x):
        raise ValueError("planes_split: an fp32 channels-last map is required")
    b, c, h, w = x.shape
    out = _new_planes(x, b, h, w, c)
    _lib.check(_lib.get().skd_planes_split_nhwc(out.M, c, x.data_ptr(), out.data.data_ptr(), _lib.stream_of(x)), "skd_planes_split_nhwc")
    return out


def planes_join(planes):
    """The fp32 channels-last map (B, C, H, W) whose pieces ``planes`` holds, (p0 + p1) + p2: a debugging and test aid."""
    _need(*_PLANES_ENTRIES)
    b, h, w, c = planes.shape
    out = _new_cl(planes.data, b, c, h, w)
    _lib.check(_lib.get().skd_planes_join_nhwc(planes.M, c, planes.data.data_ptr(), out.data_ptr(), _lib.stream_of(planes.data)),
               "skd_planes_join_nhwc")
    return out


def conv1x1_abn_planes_eval(x, conv_weight, running_mean, running_var, weight, bias, eps=1e-5, activation="relu", slope=0.01):
    """``conv1x1_abn_eval(...)`` -- three pieces, no residual, no ``pro`` -- with the result returned as a ``Planes``
    (include/skd_planes.h): the three bf16 pieces of the very fp32 values that call would return, written by the GEMM's epilogue
    (skd_conv1x1_abn_planes_nhwc) for ``conv3x3_split_eval`` to read in place of ``x``; no fp32 tensor is written.  (An op of its
    own and not a keyword of conv1x1_abn_eval: that op's bound arguments are what tests/golden/routing_census.json records call by
    call.)  Inference only; a back-end without the entries raises."""
    if torch.is_grad_enabled() and (x.requires_grad or conv_weight.requires_grad):
        raise RuntimeError("conv1x1_abn_planes_eval is inference-only")
    _need(*_PLANES_ENTRIES)
    _lib.require_device(x, conv_weight, running_mean, running_var, weight, bias)
    b, k, h, w = x.shape
    n = conv_weight.shape[0]
    wt = conv_weight.reshape(n, k)      # (N, K, 1, 1): the same memory in NCHW and channels-last
    if not wt.is_contiguous():
        wt = wt.contiguous()
    out = _new_planes(x, b, h, w, n)
    _lib.check(getattr(_lib.get(), _PLANES_PRODUCER)(b * h * w, k, n, x.data_ptr(), wt.data_ptr(), out.data.data_ptr(),
                                                     running_mean.data_ptr(), running_var.data_ptr(), _lib.ptr(weight), _lib.ptr(bias),
                                                     float(eps), _ACT[activation], float(slope), _lib.stream_of(x)), _PLANES_PRODUCER)
    return out


def _conv1x1_abn_eval(x, conv_weight, running_mean, running_var, weight, bias, eps=1e-5, activation="relu", slope=0.01,
                      residual=None, pro=None, pieces=3, piece_format="bf16"):
    """act(bn_running(conv1x1(x)) [+ residual]) as ONE GEMM with the normalisation in its epilogue (inference only;
    networks/pspnet_combine.py:65-84 for the frozen teacher).  fp32 in and out; the products run on the bf16 MFMA with both
    operands split into three bf16 pieces and the six leading products accumulated in fp32 (csrc/conv1x1.hip): within 4 x of
    an fp32 fma chain's error against a double-precision product, at most 2e-6 of the output's largest magnitude
    (tests/test_conv1x1_split_gpu.py; measured for K = 64 ... 4096, where it reaches 1.55e-6 and within 1.5 x of the library
    GEMM's own error: profiles/r13_conv1x1_reduce_accuracy.md), exact on integer data; inputs beyond +-3.39e38 or infinite give NaN.  x (B, Cin, H, W)
    and residual / result (B, Cout, H, W) in channels-last memory; conv_weight (Cout, Cin, 1, 1).
    ``pro`` = ``abn_pack_eval_params(bn)`` of an eval-mode BatchNorm + ReLU that PRECEDES the convolution
    (bn2 -> relu -> conv3, pspnet_combine.py:71-75): applied to x on its way into the GEMM, x itself is left untouched.
    ``pieces`` = 2: the reduced-precision form of include/skd_split2.h -- two bf16 pieces per operand and the three products
    a0 b1, a1 b0, a0 b0: about 4e-6 of the output's largest magnitude per product instead of 3e-7 (tests/split2_ref.py is its model,
    tests/test_split2_gpu.py the comparison; profiles/r25_split2_accuracy.md); a back-end without the entries raises, the call is
    never downgraded.  ``conv1x1_abn_eval_fp16`` is the two-piece form on FP16 pieces (include/skd_split2h.h: the residual
    scaled by 2^11, the same three products in two accumulator sets, 22 significant bits per operand: the three-piece accuracy;
    tests/split2h_ref.py is its model; an input beyond +-65504 gives NaN) -- an op of its own, not a keyword of this one, whose
    bound arguments are recorded call by call in tests/golden/routing_census.json.  ``conv1x1_abn_planes_eval`` is the same GEMM with its result written as bf16 piece planes
    (include/skd_planes.h)."""
    plain_entry, pro_entry = _CONV1X1_ABN[check_pieces(pieces, piece_format)]
    if torch.is_grad_enabled() and (x.requires_grad or conv_weight.requires_grad):
        raise RuntimeError("conv1x1_abn_eval is inference-only")
    _lib.require_device(x, conv_weight, running_mean, running_var, weight, bias, residual)
    act = {"none": 0, "leaky_relu": 1, "relu": 3}[activation]
    b, k, h, w = x.shape
    n = conv_weight.shape[0]
    out = _new_cl(x, b, n, h, w)
    if residual is not None:
        residual = _cl(residual)
        if tuple(residual.shape) != (b, n, h, w):
            raise ValueError("residual shape %s != output shape %s" % (tuple(residual.shape), (b, n, h, w)))
    wt = conv_weight.reshape(n, k)      # (N, K, 1, 1): the same memory in NCHW and channels-last
    if not wt.is_contiguous():
        wt = wt.contiguous()
    if pro is not None:
        _lib.require_device(pro)
        if pro.dtype != torch.float32 or tuple(pro.shape) != (4, k) or not pro.is_contiguous():
            raise ValueError("pro must be the (4, Cin) fp32 pack of abn_pack_eval_params")
        _need(pro_entry)
        _lib.check(getattr(_lib.get(), pro_entry)(b * h * w, k, n, x.data_ptr(), wt.data_ptr(), _lib.ptr(residual), out.data_ptr(),
                                                  running_mean.data_ptr(), running_var.data_ptr(), _lib.ptr(weight),
                                                  _lib.ptr(bias), float(eps), pro.data_ptr(), act, float(slope),
                                                  _lib.stream_of(x)), pro_entry)
        return out
    _need(plain_entry)
    _lib.check(getattr(_lib.get(), plain_entry)(b * h * w, k, n, x.data_ptr(), wt.data_ptr(), _lib.ptr(residual), out.data_ptr(),
                                                running_mean.data_ptr(), running_var.data_ptr(), _lib.ptr(weight), _lib.ptr(bias),
                                                float(eps), act, float(slope), _lib.stream_of(x)), plain_entry)
    return out


def conv1x1_abn_eval(x, conv_weight, running_mean, running_var, weight, bias, eps=1e-5, activation="relu", slope=0.01,
                     residual=None, pro=None, pieces=3):
    return _conv1x1_abn_eval(x, conv_weight, running_mean, running_var, weight, bias, eps, activation, slope, residual, pro, pieces)


def conv1x1_abn_eval_fp16(x, conv_weight, running_mean, running_var, weight, bias, eps=1e-5, activation="relu", slope=0.01,
                          residual=None, pro=None):
    """``conv1x1_abn_eval`` on two FP16 pieces per operand with the scaled residual (include/skd_split2h.h): the arguments, the
    refusals and the result's layout of that op; never downgraded (a back-end without the entries raises NotImplementedError)."""
    return _conv1x1_abn_eval(x, conv_weight, running_mean, running_var, weight, bias, eps, activation, slope, residual, pro, 2, "fp16")


conv1x1_abn_eval.__doc__ = _conv1x1_abn_eval.__doc__


def conv2d_square_geometry(conv):
    """``(stride, padding, dilation)`` of a plain nn.Conv2d (zero padding given as numbers, square), None for anything else."""
    if not (isinstance(conv, torch.nn.Conv2d) and conv.padding_mode == "zeros" and not isinstance(conv.padding, str)):
        return None
    s, p, d = _pair(conv.stride), _pair(conv.padding), _pair(conv.dilation)
    return None if s[0] != s[1] or p[0] != p[1] or d[0] != d[1] else (s[0], p[0], d[0])


# ---- the forms of the split-core 3x3 kernel family (csrc/conv3x3.hip, csrc/conv3x3_wgrad.hip) ----
# One row per (column width, pieces, piece format) that exists.  A row names every C entry, size query, cache slot and public
# weight-gradient op of its form; None where the form has none -- which is how "statistics and the 64-column directions keep three
# bf16 pieces" or "two bf16 pieces have no residual epilogue" is said.  Every entry name of the family is written here and nowhere
# else; the ops below take a row and launch what it names.  ``wgrad_op`` is a NAME, looked up on this module when called: tests
# and the routing census wrap the public ops.
_Form = collections.namedtuple("_Form", (
    "headers",          # the headers of include/ that declare the row's entries, the convolution entry's first
    "query",            # geometry query of the frozen forward
    "conv",             # the convolution entry: act(bn(conv3x3(x) + bias))
    "res_arg",          # whether ``conv`` itself takes the residual pointer
    "res",              # the entry with the residual epilogue, where it is a separate one
    "planes",           # ``conv`` reading piece planes (include/skd_planes.h): dilation and geometry behind the epilogue
    "s2_query", "s2",   # the stride-2 forward (no dilation argument) and its geometry query
    "s2_pieces",        # whether ``s2`` takes the piece count (it then serves both bf16 piece counts)
    "stats",            # the training forward that also writes the batch-norm statistics records
    "scaled",           # the data gradient that takes the scale word of fp16_scale_word
    "train_query",      # geometry query of forward + data gradient in training
    "pack",             # writes the frozen weight image
    "pack_pair",        # writes the forward image and / or the data gradient's in one launch
    "bytes",            # size query of either image
    "wgrad_query", "wgrad", "wgrad_op",      # the weight gradient: geometry query, (plan entry, launch entry), the public op's name
    "pack_slot",        # cache slot of the frozen image
    "train_slot",       # cache slot of the training pair
    "packs_op",         # name of the public op that makes (and caches) the training pair
    "mixed_slot",       # cache slot of this form's half of a pair whose other direction is on the other column width
), defaults=(None,) * 22)

_WIDE3 = _Form(
    headers=("skd_eval.h", "skd_infer.h", "skd_planes.h", "skd_stride2.h", "skd_bnstats.h", "skd_train.h", "skd_wgrad.h"),
    query="skd_conv3x3_split_supported", conv="skd_conv3x3_split_nhwc", res_arg=False, res="skd_conv3x3_split_res_nhwc",
    planes="skd_conv3x3_split_planes_nhwc", s2_query="skd_conv3x3_split_s2_supported", s2="skd_conv3x3_split_s2_nhwc",
    s2_pieces=True, stats="skd_conv3x3_split_stats_nhwc", train_query="skd_conv3x3_split_train_supported",
    pack="skd_conv3x3_split_pack_weights", pack_pair="skd_conv3x3_split_pack_pair", bytes="skd_conv3x3_split_pack_bytes",
    wgrad_query="skd_conv3x3_split_wgrad_supported", wgrad=("skd_conv3x3_split_wgrad_plan", "skd_conv3x3_split_wgrad_nhwc"),
    wgrad_op="conv3x3_split_wgrad", pack_slot="_skd_conv3x3_pack", train_slot="_skd_conv3x3_train_pack",
    packs_op="conv3x3_train_packs",     mixed_slot="_skd_conv3x3_train_pack_wide")
# two bf16 pieces.  The geometry queries are the three-piece form's (the predicates ask _WIDE3), and so are the stride-2 entry, which
# takes the piece count, and the weight gradient's query; no residual epilogue, no piece planes, no statistics.
_WIDE2 = _Form(
    headers=("skd_split2.h", "skd_stride2.h", "skd_train2.h", "skd_wgrad.h"),
    conv="skd_conv3x3_split2_nhwc", res_arg=False, s2=_WIDE3.s2, s2_pieces=True, pack="skd_conv3x3_split2_pack_weights",
    pack_pair="skd_conv3x3_split2_pack_pair", bytes="skd_conv3x3_split2_pack_bytes", wgrad_query=_WIDE3.wgrad_query,
    wgrad=("skd_conv3x3_split2_wgrad_plan", "skd_conv3x3_split2_wgrad_nhwc"), wgrad_op="conv3x3_split_wgrad2",
    pack_slot="_skd_conv3x3_pack2", train_slot="_skd_conv3x3_train_pack2", packs_op="conv3x3_train_packs2")
# two fp16 pieces: a stride-2 entry of its own, without a piece count; a data gradient of its own, which takes the scale word; the
# weight gradient has no query of its own and does not depend on skd_wgrad.h
_WIDE2H = _Form(
    headers=("skd_split2h.h", "skd_infer2h.h", "skd_train2h.h"),
    conv="skd_conv3x3_split2h_nhwc", res_arg=False, res="skd_conv3x3_split2h_res_nhwc", s2="skd_conv3x3_split2h_s2_nhwc",
    s2_pieces=False, scaled="skd_conv3x3_split2h_scaled_nhwc", pack="skd_conv3x3_split2h_pack_weights",
    pack_pair="skd_conv3x3_split2h_pack_pair", bytes="skd_conv3x3_split2h_pack_bytes",
    wgrad=("skd_conv3x3_split2h_wgrad_plan", "skd_conv3x3_split2h_wgrad_nhwc"), wgrad_op="conv3x3_split_wgrad_fp16",
    pack_slot="_skd_conv3x3_pack2h", train_slot="_skd_conv3x3_train_pack2h", packs_op="conv3x3_train_packs_fp16")
# the 64-column form: its one convolution entry takes the residual pointer, its pack-pair entry writes the frozen image too
_NARROW3 = _Form(
    headers=("skd_narrow.h", "skd_bnstats.h", "skd_narrow_wgrad.h"),
    query="skd_conv3x3_narrow_supported", conv="skd_conv3x3_narrow_nhwc", res_arg=True, stats="skd_conv3x3_narrow_stats_nhwc",
    pack_pair="skd_conv3x3_narrow_pack_pair", bytes="skd_conv3x3_narrow_pack_bytes",
    wgrad_query="skd_conv3x3_narrow_wgrad_supported", wgrad=("skd_conv3x3_narrow_wgrad_plan", "skd_conv3x3_narrow_wgrad_nhwc"),
    wgrad_op="conv3x3_narrow_wgrad", pack_slot="_skd_conv3x3_narrow_pack", train_slot="_skd_conv3x3_train_pack_narrow")
_NARROW2H = _Form(
    headers=("skd_infer2h.h",),
    conv="skd_conv3x3_narrow2h_nhwc", res_arg=True, pack="skd_conv3x3_narrow2h_pack_weights",
    bytes="skd_conv3x3_narrow2h_pack_bytes", pack_slot="_skd_conv3x3_narrow_pack2h")
_FORMS = (_WIDE3, _WIDE2, _WIDE2H, _NARROW3, _NARROW2H)
_WIDE = {(3, "bf16"): _WIDE3, (2, "bf16"): _WIDE2, (2, "fp16"): _WIDE2H}      # check_pieces' answer -> the wide form
# the slots of the table under the names tests read them by
_TRAIN2_PACK_ATTR, _TRAIN2H_PACK_ATTR = _WIDE2.train_slot, _WIDE2H.train_slot
_NARROW_PACK_ATTRS = (_NARROW3.pack_slot, _WIDE3.mixed_slot, _NARROW3.train_slot)
# what _Conv3x3SplitTrain runs: the rows of the forward and of the data gradient, the row whose weight-gradient op is asked for
# (None: the library's), whether the forward also writes the statistics records
_TrainForms = collections.namedtuple("_TrainForms", "fwd bwd wgrad stats")


def _conv3x3_slots():
    """Every cache slot a form names: what drop_conv3x3_packs forgets on a module."""
    return tuple(s for form in _FORMS for s in (form.pack_slot, form.train_slot, form.mixed_slot) if s is not None)


def _res_entry(form):
    """The entry of ``form`` that takes the residual pointer: its convolution entry itself, or the separate one (None: none)."""
    return form.conv if form.res_arg else form.res


def _conv3x3_ok(x, weight, stride, padding, dilation, groups, grad, entries, query, host_ok):
    """The one predicate of the split-core 3x3 forms: grad is ``grad``, the back-end has every entry of ``entries``, ``x`` is an
    fp32 channels-last 16-byte-aligned device map (``host_ok``: a host one passes under a test double), ``weight`` a
    (Cout, Cin, 3, 3) fp32 tensor (any strided view) on its device with ``x.shape[1] == Cin * groups``, and the library's
    ``query`` takes the geometry."""
    if torch.is_grad_enabled() != grad or not all(_lib.has_entry(n) for n in entries):
        return False
    if not (_fp32_cl_map(x, host_ok) and x.data_ptr() % 16 == 0):
        return False
    if not (weight.dim() == 4 and tuple(weight.shape[2:]) == (3, 3) and weight.dtype == torch.float32
            and weight.device == x.device and x.shape[1] == weight.shape[1] * groups):
        return False
    return bool(getattr(_lib.get(), query)(int(weight.shape[1]), int(weight.shape[0]), int(stride), int(padding), int(dilation),
                                           int(groups)))


def _conv3x3_module_ok(x, conv, **form):
    geometry = conv2d_square_geometry(conv)
    return geometry is not None and _conv3x3_ok(x, conv.weight, *geometry, conv.groups, **form)


# The frozen form refuses host tensors even under a test double: under the recording and computing doubles that is what keeps the
# student's dsn[0] and PSP half on F.conv2d.
_FROZEN = dict(grad=False, entries=(_WIDE3.conv,), query=_WIDE3.query, host_ok=False)
_TRAIN_ENTRIES = (_WIDE3.train_query, _WIDE3.pack_pair, _WIDE3.conv)
_NARROW_ENTRIES = (_NARROW3.query, _NARROW3.bytes, _NARROW3.pack_pair, _NARROW3.conv)
_S2_ENTRIES = (_WIDE3.s2_query, _WIDE3.s2)
_WGRAD_ENTRIES = (_WIDE3.wgrad_query,) + _WIDE3.wgrad
_NARROW_WGRAD_ENTRIES = (_NARROW3.wgrad_query,) + _NARROW3.wgrad


def conv3x3_split_supported(x, conv):
    """True when the implicit-GEMM 3x3 convolution of csrc/conv3x3.hip takes ``conv(x)``: a back-end that has the entry (the
    tests' C double does not: callers then run ``F.conv2d`` as before), no grad, an fp32 channels-last input, a plain 3x3 /
    stride-1 / padding == dilation / ungrouped convolution with Cin a multiple of 16 and Cout of 128."""
    return _conv3x3_module_ok(x, conv, **_FROZEN)


def conv3x3_infer_supported(x, conv, residual=False):
    """True when a BasicBlock's inference form (networks.pspnet_combine.fuse_for_inference) may hand ``conv(x)`` to the split
    core: the conditions of conv3x3_split_supported, asked of a back-end that has the entry the call needs --
    ``skd_conv3x3_split_res_nhwc`` (include/skd_infer.h) with ``residual``, ``skd_conv3x3_split_nhwc`` without.  A back-end
    without it (the tests' C double) answers False and the block runs the sequence it ran before.  Host tensors pass only
    under a test double, as in conv1x1_abn_supported."""
    entry = _WIDE3.res if residual else _WIDE3.conv
    return _conv3x3_module_ok(x, conv, grad=False, entries=(entry, _WIDE3.query), query=_WIDE3.query, host_ok=True)


def conv3x3_train_supported(x, weight, stride, padding, dilation, groups):
    """True when conv3x3_split_train takes ``F.conv2d(x, weight, bias, stride, padding, dilation, groups)`` of a network that is
    being trained: grad enabled, a back-end that has the three entries (include/skd_train.h and skd_conv3x3_split_nhwc; the tests'
    C double does not: callers then run the convolution they ran before), an fp32 channels-last 16-byte-aligned device input and
    a (Cout, Cin, 3, 3) fp32 weight on its device whose forward AND data gradient fit the core: stride 1, padding == dilation,
    ungrouped, Cin and Cout multiples of 128.  ``weight`` may be any strided view.  Host tensors pass only under a test double,
    as in conv3x3_infer_supported."""
    return _conv3x3_ok(x, weight, stride, padding, dilation, groups, grad=True, entries=_TRAIN_ENTRIES,
                       query=_WIDE3.train_query, host_ok=True)


def _conv3x3_packs(w, owner, attr, entry, what, images, bytes_entry):
    """The image(s) of the (Cout, Cin, 3, 3) weight ``w`` that csrc/conv3x3.hip streams into LDS, written by one launch of
    ``entry`` and cached on ``owner`` as ``(key, *packs, storage)`` with ``key = (data_ptr, _version, shape, stride)``.
    ``images`` has one flag per (pointer, bytes) pair that ``entry`` takes, forward image first: ``(True,)`` for
    skd_conv3x3_split_pack_weights, ``(forward?, backward?)`` for the two pack_pair entries (skd_train.h, skd_narrow.h), which
    write the chosen image(s) alone.  One pack per flag, None for an image not asked for, each sized by ``bytes_entry`` for its
    direction; a direction the entry's form does not take (size 0) is a ValueError."""
    def build():
        _lib.require_device(w)
        cout, cin = int(w.shape[0]), int(w.shape[1])
        lib = _lib.get()
        sizes = [int(getattr(lib, bytes_entry)(*dims)) if want else None for want, dims in zip(images, ((cin, cout), (cout, cin)))]
        if (tuple(w.shape[2:]) != (3, 3) or w.dtype != torch.float32 or not any(images)
                or any(n is not None and n <= 0 for n in sizes)):
            raise ValueError("%s: unsupported weight %s" % (what, tuple(w.shape)))
        with torch.no_grad():
            packs = tuple(None if n is None else torch.empty((n,), dtype=torch.uint8, device=w.device) for n in sizes)
            sized = [v for pk, n in zip(packs, sizes) for v in ((None, 0) if pk is None else (pk.data_ptr(), n))]
            _lib.check(getattr(lib, entry)(cin, cout, w.data_ptr(), *(int(v) for v in w.stride()), *sized, _lib.stream_of(w)), entry)
        return packs
    return _cached(owner, attr, _version_key((w,), tuple(w.shape), tuple(w.stride())), build, hold=w)


def _conv3x3_pack_weights(conv, weight=None, owner=None, pieces=3, piece_format="bf16"):
    """The three bf16 planes of a frozen 3x3 convolution's weight in the layout csrc/conv3x3.hip streams into LDS (6 bytes per
    weight), cached on ``owner`` (default: the conv module) like abn_pack_eval_params and rebuilt when the weight is written or
    moved -- by THE RULE above _version_key: a fused optimizer's step counts as a write only with
    ``kd_model.advance_versions_after_step`` registered on it (NetModel's has it; a caller who trains with a fused optimizer of
    their own registers it themselves).  ``weight`` (default ``conv.weight``) may be any strided (Cout, Cin, 3, 3) view -- the PSP
    bottleneck packs the feature-map slice of its weight -- and either memory format gives the same pack.  The first call
    allocates: a frozen network makes it in its eager warm-up steps, before any graph capture.
    ``pieces`` = 2: the two-plane image of include/skd_split2.h (4 bytes per weight: the first two planes of the other), for
    ``conv3x3_split_eval(..., pieces=2)``; cached under the same rule in a slot of its own, so both packs of one module coexist.
    ``conv3x3_pack_weights_fp16``: the two fp16 planes of include/skd_split2h.h (p0 and the scaled p1, 4 bytes per weight
    again), in a third slot beside the other two."""
    form = _WIDE[check_pieces(pieces, piece_format)]
    w = conv.weight if weight is None else weight
    if torch.is_grad_enabled() and w.requires_grad:
        raise RuntimeError("conv3x3_pack_weights is for frozen (no-grad) convolutions")
    _need(form.pack, form.bytes)
    return _conv3x3_packs(w, conv if owner is None else owner, form.pack_slot, form.pack, "conv3x3_pack_weights", (True,),
                          form.bytes)[0]


def conv3x3_pack_weights(conv, weight=None, owner=None, pieces=3):
    return _conv3x3_pack_weights(conv, weight, owner, pieces)


def conv3x3_pack_weights_fp16(conv, weight=None, owner=None):
    """``conv3x3_pack_weights`` for ``conv3x3_split_eval_fp16``: the two-plane fp16 image of include/skd_split2h.h, cached
    under the same rule in a slot of its own."""
    return _conv3x3_pack_weights(conv, weight, owner, 2, "fp16")


conv3x3_pack_weights.__doc__ = _conv3x3_pack_weights.__doc__


def _conv3x3_train_packs(form, weight, owner, what="conv3x3_train_packs"):
    """The ``(pack_fwd, pack_bwd)`` of ``form``: one launch of its pack-pair entry, cached in its training slot (each form its own:
    switching the piece count or format never serves another form's image)."""
    _need(form.pack_pair, form.bytes)
    return _conv3x3_packs(weight, owner, form.train_slot, form.pack_pair, what, (True, True), form.bytes)


def conv3x3_train_packs(weight, owner=None):
    """``(pack_fwd, pack_bwd)`` of a trained (Cout, Cin, 3, 3) weight: the image csrc/conv3x3.hip streams for the forward
    convolution and the image of the flipped, transposed weight for its data gradient, written by ONE launch of
    skd_conv3x3_split_pack_pair under no_grad.  Cached on ``owner`` (a dict or any object that takes attributes; None: no cache)
    as conv3x3_pack_weights does: one split per weight version, so once per optimizer step -- provided the optimizer advances
    ``_version`` (torch's fused multi-tensor optimizers do not: networks.kd_model.advance_versions_after_step is the step
    post-hook that does it for them).
    ``conv3x3_train_packs2``: the two-plane images of include/skd_train2.h (skd_conv3x3_split2_pack_pair, 4 bytes per weight),
    for skd_conv3x3_split2_nhwc in both directions; cached under the same rule in a slot of its own, so the pairs of both piece
    counts coexist on one owner and neither is ever served for the other.  A back-end without the entry raises
    NotImplementedError.  (A twin, not a ``pieces`` argument: tests/golden/routing_census.json records every call of the public
    conv3x3_* ops with its defaults filled in, so their signatures stay what they are -- as for the ``_fp16`` twins.)"""
    return _conv3x3_train_packs(_WIDE3, weight, owner)


def conv3x3_train_packs2(weight, owner=None):
    """``conv3x3_train_packs`` for ``conv3x3_split_train2``: the two-plane pair of include/skd_train2.h, in a slot of its own."""
    return _conv3x3_train_packs(_WIDE2, weight, owner)


# the two entries of include/skd_train2h.h that belong to no form: the scale word of a gradient tensor
_SCALE_WORD = ("skd_fp16_scale_word_workspace_bytes", "skd_fp16_scale_word")


def split2_supported(piece_format="bf16"):
    """True when the back-end has the five entries of the frozen two-piece forms in ``piece_format``: include/skd_split2.h for
    "bf16", skd_split2h.h for "fp16" -- the 3x3 convolution, its pack entry and size query, and the two 1x1 GEMMs (the tests' C
    double has none of them)."""
    return _has(*_lib.ABI[_WIDE[2, check_piece_format(piece_format)].headers[0]])


def train2_supported():
    """True when the back-end has the three entries of include/skd_train2.h and the two of skd_split2.h they build on."""
    return _has(*_lib.ABI["skd_train2.h"], _WIDE2.bytes, _WIDE2.conv)


def train2h_supported():
    """True when the back-end has the six entries of include/skd_train2h.h and the two of skd_split2h.h they build on (the tests'
    C double has none of them)."""
    return _has(*_lib.ABI["skd_train2h.h"], _WIDE2H.conv, _WIDE2H.bytes)


def fp16_scale_word(g):
    """The scale word of the dense fp32 tensor ``g`` (include/skd_train2h.h): a one-element int32 device tensor holding
    ``max(bits(g) & 0x7fffffff)``, from which the fp16 training kernels derive the power of two that puts ``g``'s largest magnitude
    into [2^14, 2^15).  At most two launches on ``g``'s stream, no host synchronisation, the same word on every call; an infinity
    or a NaN in ``g`` makes it >= 0x7f800000 (scale 1: a non-finite gradient stays loud)."""
    _need(*_SCALE_WORD)
    _lib.require_device(g)
    if g.dtype != torch.float32 or g.numel() < 1 or not _non_overlapping_and_dense(g) or g.data_ptr() % 16:
        raise ValueError("fp16_scale_word: a dense, 16-byte aligned fp32 tensor of at least one element expected")
    lib = _lib.get()
    n = int(g.numel())
    nbytes = int(lib.skd_fp16_scale_word_workspace_bytes(n))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=g.device)
    word = torch.empty((1,), dtype=torch.int32, device=g.device)
    _lib.check(lib.skd_fp16_scale_word(n, g.data_ptr(), ws.data_ptr(), nbytes, word.data_ptr(), _lib.stream_of(g)), _SCALE_WORD[1])
    return word


def conv3x3_train_packs_fp16(weight, owner=None):
    """``conv3x3_train_packs`` for ``conv3x3_split_train_fp16``: the two-plane FP16 images of include/skd_train2h.h
    (skd_conv3x3_split2h_pack_pair, 4 bytes per weight: p0 and the scaled p1 of skd_split2h.h) for the forward and for the data
    gradient, one launch, cached per ``(data_ptr, _version)`` in a slot of its own beside the bf16 pairs.  A back-end without
    the entry raises NotImplementedError."""
    return _conv3x3_train_packs(_WIDE2H, weight, owner, "conv3x3_train_packs_fp16")


_ACT = {"none": 0, "leaky_relu": 1, "relu": 3}      # SKD_ACT_* of include/skd.h


def infer2h_supported():
    """True when the back-end has the five entries of include/skd_infer2h.h and the three of skd_split2h.h they build on (the
    tests' C double has none of them)."""
    return _has(*_lib.ABI["skd_infer2h.h"], _WIDE2H.bytes, _WIDE2H.pack, _WIDE2H.conv)


def _bn_epilogue(bn):
    """``(mean, var, gamma, beta, eps, slope)`` of a launch's epilogue: the running statistics and affine parameters of the
    eval-mode InPlace-ABN module ``bn``, or no normalisation for None."""
    if bn is None:
        return None, None, None, None, 0.0, 0.01
    return bn.running_mean, bn.running_var, bn.weight, bn.bias, float(bn.eps), float(bn.slope)


def _conv3x3_begin(form, entry, src, dims, pack, cout, out_hw, *others):
    """The host steps every launch of the family starts with: ``pack`` is the image ``form`` reads for a (cout, cin, 3, 3)
    weight, every tensor is on the device, and the output is allocated -- (b, cout, *out_hw) fp32 channels-last on the device of
    ``src``, the tensor the entry reads a ``dims = (b, cin, h, w)`` map from.  Returns ``(lib, out)``."""
    lib = _lib.get()
    b, cin = dims[:2]
    if pack.numel() != getattr(lib, form.bytes)(cin, cout):
        raise ValueError("%s: the pack is not that of a (%d, %d, 3, 3) weight" % (entry, cout, cin))
    _lib.require_device(src, pack, *others)
    # not a view (_new_cl's is one, with the same strides): the in-place ABN behind dsn[0] writes into a custom Function's output
    out = torch.empty((b, cout) + tuple(out_hw), dtype=torch.float32, device=src.device, memory_format=torch.channels_last)
    return lib, out


def _conv3x3_launch(form, entry, x, pack, cout, dilation, conv_bias=None, bn=None, activation="none", geometry=0, residual=None):
    """The one launcher of the split-core 3x3 forms: act(bn_running(conv3x3(x) + conv_bias) [+ residual]) by ``entry``, the
    convolution entry of ``form`` (a row of the table above) or its residual entry, which takes the ``residual`` pointer (None
    included)."""
    b, cin, h, w = x.shape
    mean, var, gamma, beta, eps, slope = _bn_epilogue(bn)
    lib, out = _conv3x3_begin(form, entry, x, x.shape, pack, cout, (h, w), residual, conv_bias, mean, var, gamma, beta)
    res = (_lib.ptr(residual),) if entry == _res_entry(form) else ()
    _lib.check(getattr(lib, entry)(b, h, w, cin, cout, int(dilation), x.data_ptr(), pack.data_ptr(), out.data_ptr(), *res,
                                   _lib.ptr(conv_bias), _lib.ptr(mean), _lib.ptr(var), _lib.ptr(gamma), _lib.ptr(beta), eps,
                                   _ACT[activation], slope, int(geometry), _lib.stream_of(x)), entry)
    return out


def _conv3x3_raw_launch(form, x, pack, cout, dilation, conv_bias=None):
    """conv3x3(x) + conv_bias on ``form``, raw (no normalisation, no activation): what training runs in both directions."""
    return _conv3x3_launch(form, form.conv, x, pack, cout, dilation, conv_bias)


def _conv3x3_planes_launch(form, planes, pack, cout, dilation, conv_bias=None, bn=None, activation="none", geometry=0):
    """_conv3x3_launch for the piece-plane entry of ``form`` (include/skd_planes.h): the input is a ``Planes``; the entry takes
    dilation and geometry behind the epilogue arguments."""
    b, h, w, cin = planes.shape
    if planes.data.numel() != planes_bytes(planes.M, cin) or planes.M != b * h * w:
        raise ValueError("%s: the planes are not those of a %s map" % (form.planes, (planes.shape,)))
    mean, var, gamma, beta, eps, slope = _bn_epilogue(bn)
    lib, out = _conv3x3_begin(form, form.planes, planes.data, (b, cin, h, w), pack, cout, (h, w), conv_bias, mean, var, gamma, beta)
    _lib.check(getattr(lib, form.planes)(b, h, w, cin, cout, planes.data.data_ptr(), pack.data_ptr(), out.data_ptr(),
                                         _lib.ptr(conv_bias), _lib.ptr(mean), _lib.ptr(var), _lib.ptr(gamma), _lib.ptr(beta), eps,
                                         _ACT[activation], slope, int(dilation), int(geometry), _lib.stream_of(planes.data)),
               form.planes)
    return out


def _residual_cl(x, cout, residual):
    """The residual of a split-core 3x3 launch on ``x`` with ``cout`` output channels: None, or a (B, cout, H, W) fp32 tensor,
    returned in channels-last memory (copied when it is not)."""
    if residual is None:
        return None
    want = (x.shape[0], cout) + tuple(x.shape[2:])
    if tuple(residual.shape) != want or residual.dtype != torch.float32:
        raise ValueError("residual %s %s != output %s fp32" % (tuple(residual.shape), residual.dtype, want))
    return _cl(residual)


def _conv3x3_split_eval(x, pack, cout, dilation=1, conv_bias=None, bn=None, activation="none", geometry=0, pieces=3,
                        piece_format="bf16"):
    """act(bn_running(conv3x3(x) + conv_bias)) with ``pack = conv3x3_pack_weights(...)`` (inference only; conv3x3_split_supported
    says when).  fp32 in and out, channels-last; the products run on the bf16 MFMA through the three-piece split (csrc/conv3x3.hip):
    within 4 x of the fp32 convolution's error against a float64 result and never above 2e-5 of the output's largest magnitude
    (tests/test_conv3x3_split_gpu.py), exact on integer data.  ``bn``: an eval-mode InPlace-ABN module (or None) whose running
    statistics and affine parameters go into the epilogue; ``activation``: 'none' / 'relu' / 'leaky_relu' (slope: ``bn.slope``).
    ``pieces`` = 2: the reduced-precision form of include/skd_split2.h with ``pack = conv3x3_pack_weights(..., pieces=2)`` -- two
    pieces per operand, the products a0 b1, a1 b0, a0 b0: within 2e-5 of its float64 model (tests/split2_ref.py), which itself is
    about 4e-6 of the output's largest magnitude from the exact product (profiles/r25_split2_accuracy.md).  A back-end without the
    entry raises; the call is never downgraded.  ``conv3x3_split_eval_fp16`` is the form of include/skd_split2h.h with
    ``pack = conv3x3_pack_weights_fp16(...)`` -- two fp16 pieces, scaled residual, the three-piece accuracy
    (tests/split2h_ref.py); an input beyond +-65504 gives NaN.
    ``x`` may be a ``Planes`` (include/skd_planes.h; three pieces only): the kernel loads the pieces instead of cutting the
    fp32 map (skd_conv3x3_split_planes_nhwc), and the result is bit for bit that of the call on the fp32 map."""
    form = _WIDE[check_pieces(pieces, piece_format)]
    if isinstance(x, Planes):
        if form.planes is None:
            raise ValueError("conv3x3_split_eval: piece planes hold three pieces")
        _need(*_PLANES_ENTRIES)
        return _conv3x3_planes_launch(form, x, pack, cout, dilation, conv_bias, bn, activation, geometry)
    if torch.is_grad_enabled() and x.requires_grad:
        raise RuntimeError("conv3x3_split_eval is inference-only")
    _need(form.conv)
    return _conv3x3_launch(form, form.conv, x, pack, cout, dilation, conv_bias, bn, activation, geometry)


def conv3x3_split_eval(x, pack, cout, dilation=1, conv_bias=None, bn=None, activation="none", geometry=0, pieces=3):
    return _conv3x3_split_eval(x, pack, cout, dilation, conv_bias, bn, activation, geometry, pieces)


def conv3x3_split_eval_fp16(x, pack, cout, dilation=1, conv_bias=None, bn=None, activation="none", geometry=0):
    """``conv3x3_split_eval`` on two FP16 pieces per operand with the scaled residual (include/skd_split2h.h), with
    ``pack = conv3x3_pack_weights_fp16(...)``; never downgraded (a back-end without the entry raises NotImplementedError)."""
    return _conv3x3_split_eval(x, pack, cout, dilation, conv_bias, bn, activation, geometry, 2, "fp16")


conv3x3_split_eval.__doc__ = _conv3x3_split_eval.__doc__


def _conv3x3_res_eval(form, what, x, pack, cout, dilation, residual, bn, activation, conv_bias, geometry):
    """The body of the four inference ops with a residual epilogue: the op ``what`` on the residual-taking entry of ``form``."""
    if torch.is_grad_enabled() and (x.requires_grad or (residual is not None and residual.requires_grad)):
        raise RuntimeError("%s is inference-only" % what)
    entry = _res_entry(form)
    _need(entry, form.bytes)
    return _conv3x3_launch(form, entry, x, pack, cout, dilation, conv_bias, bn, activation, geometry, _residual_cl(x, cout, residual))


def conv3x3_split_res_eval(x, pack, cout, dilation, residual, bn, activation, conv_bias=None, geometry=0):
    """act(bn_running(conv3x3(x) + conv_bias) + residual) in one launch of csrc/conv3x3.hip (include/skd_infer.h; inference
    only): conv3x3_split_eval with the residual added in the epilogue, behind the normalisation and in front of the activation
    -- ``relu(bn2(conv2(.)) + residual)`` of a BasicBlock.  ``pack = conv3x3_pack_weights(...)`` (the same cache), ``bn`` an
    eval-mode InPlace-ABN module or None, ``residual`` (B, cout, H, W) fp32, read in channels-last memory (copied when it is
    not) and never written; ``residual=None`` is conv3x3_split_eval bit for bit.  The numerics of the convolution are those of
    conv3x3_split_eval; the residual add is one more fp32 rounding."""
    return _conv3x3_res_eval(_WIDE3, "conv3x3_split_res_eval", x, pack, cout, dilation, residual, bn, activation, conv_bias, geometry)


def conv3x3_split_res_eval_fp16(x, pack, cout, dilation, residual, bn, activation, conv_bias=None, geometry=0):
    """``conv3x3_split_res_eval`` on two FP16 pieces per operand with the scaled residual (include/skd_infer2h.h), with
    ``pack = conv3x3_pack_weights_fp16(...)`` (the cache of conv3x3_split_eval_fp16): the same arguments, the residual added in
    fp32 behind the normalisation and never split; ``residual=None`` is conv3x3_split_eval_fp16 bit for bit.  The numerics of
    the convolution are those of include/skd_split2h.h (tests/split2h_ref.py); an input beyond +-65504 gives non-finite outputs.
    An op of its own, not a keyword: tests/golden/routing_census.json records every public conv3x3_* call with its defaults.
    Never downgraded: a back-end without the entry raises NotImplementedError."""
    return _conv3x3_res_eval(_WIDE2H, "conv3x3_split_res_eval_fp16", x, pack, cout, dilation, residual, bn, activation, conv_bias,
                             geometry)


# include/skd_bnstats.h: the training forward that also emits the batch-norm statistics records of its output, and their finalize
_BNSTATS_ENTRIES = tuple(_lib.ABI["skd_bnstats.h"])


def conv3x3_bnstats_supported():
    """True when the back-end has the four entries of include/skd_bnstats.h (the tests' C double does not: conv3x3_split_train is
    then not asked for statistics and the ABN forward behind it runs what it ran before)."""
    return _has(*_BNSTATS_ENTRIES)


def _conv3x3_stats_launch(form, x, pack, cout, dilation, conv_bias=None):
    """``(conv3x3(x) + conv_bias, partials)``: the raw _conv3x3_launch of ``form`` by its entry of include/skd_bnstats.h, which
    writes the same bits and, from its epilogue, one (mean, M2) per 32-row block and channel of the output into ``partials``
    (fp32, skd_conv3x3_bnstats_floats long, every element written)."""
    b, cin, h, w = x.shape
    lib, out = _conv3x3_begin(form, form.stats, x, x.shape, pack, cout, (h, w), conv_bias)
    n = int(lib.skd_conv3x3_bnstats_floats(b * h * w, cout))
    partials = torch.empty((max(n, 1),), dtype=torch.float32, device=x.device)
    _lib.check(getattr(lib, form.stats)(b, h, w, cin, cout, int(dilation), x.data_ptr(), pack.data_ptr(), out.data_ptr(),
                                        _lib.ptr(conv_bias), 0, partials.data_ptr(), n, _lib.stream_of(x)), form.stats)
    return out, partials


def conv3x3_narrow_supported(x, conv, residual=False):
    """True when the 64-column form of the split-core 3x3 convolution (csrc/conv3x3.hip, include/skd_narrow.h) takes
    ``conv(x)`` of a frozen forward: no grad, a back-end that has the four entries (the tests' C double does not: callers then run
    what they ran before), an fp32 channels-last 16-byte-aligned input, a plain 3x3 / stride-1 / padding == dilation / ungrouped
    convolution with Cin a multiple of 16 and Cout of 64.  ``residual``: the one entry takes it, so the answer is the same.
    Host tensors pass only under a test double, as in conv3x3_infer_supported."""
    return _conv3x3_module_ok(x, conv, grad=False, entries=_NARROW_ENTRIES, query=_NARROW3.query, host_ok=True)


def conv3x3_narrow_pack_weights(conv, weight=None, owner=None):
    """conv3x3_pack_weights for the 64-column form: the three bf16 planes of a frozen 3x3 convolution's weight per column tile of
    64 output channels (6 bytes per weight), written by skd_conv3x3_narrow_pack_pair and cached on ``owner`` (default: the conv
    module) under the same rule, in a slot of its own."""
    w = conv.weight if weight is None else weight
    if torch.is_grad_enabled() and w.requires_grad:
        raise RuntimeError("conv3x3_narrow_pack_weights is for frozen (no-grad) convolutions")
    return _conv3x3_packs(w, conv if owner is None else owner, _NARROW3.pack_slot, _NARROW3.pack_pair,
                          "conv3x3_narrow_pack_weights", (True, False), _NARROW3.bytes)[0]


def conv3x3_narrow_eval(x, pack, cout, dilation, residual=None, conv_bias=None, bn=None, activation="none", geometry=0):
    """act(bn_running(conv3x3(x) + conv_bias) [+ residual]) in one launch of csrc/conv3x3.hip's 64-column form (inference
    only), with ``pack = conv3x3_narrow_pack_weights(...)``: conv3x3_split_eval / conv3x3_split_res_eval for a Cout that is a
    multiple of 64.  The arithmetic of every output element is that of the 128-column form, in its order: where both take a
    convolution they give the same bits.  ``residual`` (B, cout, H, W) fp32 is read in channels-last memory (copied when it is not) and never written."""
    return _conv3x3_res_eval(_NARROW3, "conv3x3_narrow_eval", x, pack, cout, dilation, residual, bn, activation, conv_bias, geometry)


def conv3x3_narrow_pack_weights_fp16(conv, weight=None, owner=None):
    """``conv3x3_narrow_pack_weights`` for ``conv3x3_narrow_eval_fp16``: the two fp16 planes (p0 and the scaled p1) of the weight
    per column tile of 64 output channels (4 bytes per weight), written by skd_conv3x3_narrow2h_pack_weights
    (include/skd_infer2h.h) and cached on ``owner`` under the same ``(data_ptr, _version)`` rule in a slot of its own, beside the
    three-piece one.  A back-end without the entries raises NotImplementedError."""
    w = conv.weight if weight is None else weight
    if torch.is_grad_enabled() and w.requires_grad:
        raise RuntimeError("conv3x3_narrow_pack_weights_fp16 is for frozen (no-grad) convolutions")
    _need(_NARROW2H.pack, _NARROW2H.bytes)
    return _conv3x3_packs(w, conv if owner is None else owner, _NARROW2H.pack_slot, _NARROW2H.pack,
                          "conv3x3_narrow_pack_weights_fp16", (True,), _NARROW2H.bytes)[0]


def conv3x3_narrow_eval_fp16(x, pack, cout, dilation, residual=None, conv_bias=None, bn=None, activation="none", geometry=0):
    """``conv3x3_narrow_eval`` on two FP16 pieces per operand with the scaled residual (include/skd_infer2h.h), with
    ``pack = conv3x3_narrow_pack_weights_fp16(...)``: the same arguments; at a Cout both forms take it gives the bits of
    conv3x3_split_eval_fp16 / conv3x3_split_res_eval_fp16.  Never downgraded: a back-end without the entry raises
    NotImplementedError."""
    return _conv3x3_res_eval(_NARROW2H, "conv3x3_narrow_eval_fp16", x, pack, cout, dilation, residual, bn, activation, conv_bias,
                             geometry)


def conv3x3_s2_supported(x, conv):
    """True when the stride-2 form of the split-core 3x3 convolution (csrc/conv3x3.hip, include/skd_stride2.h) takes ``conv(x)``
    of a frozen forward: no grad, a back-end that has the entries (the tests' C double does not: callers then run what they ran
    before), an fp32 channels-last 16-byte-aligned input, a plain 3x3 / stride-2 / padding-1 / dilation-1 / ungrouped convolution
    with Cin a multiple of 16 and Cout of 128.  Host tensors pass only under a test double, as in conv3x3_infer_supported."""
    return _conv3x3_module_ok(x, conv, grad=False, entries=_S2_ENTRIES, query=_WIDE3.s2_query, host_ok=True)


def _conv3x3_s2_eval(x, pack, cout, conv_bias=None, bn=None, activation="none", pieces=3, piece_format="bf16"):
    """act(bn_running(conv3x3(x, stride 2, padding 1) + conv_bias)) in one launch of csrc/conv3x3.hip's stride-2 form
    (include/skd_stride2.h; inference only; conv3x3_s2_supported says when), returned as a plain channels-last (B, cout, Ho, Wo) allocation, Ho = (H - 1) // 2 + 1.
    ``pack = conv3x3_pack_weights(conv, pieces=pieces)``: the image does not depend on the stride, so it is the cache of the
    stride-1 form under the one rule of _version_key.  Only the row map differs from conv3x3_split_eval: the result is that
    op's output at the even pixels bit for bit (tests/test_conv3x3_stride2_gpu.py), and its numerics are that op's for either
    piece count.  ``activation``: 'none' or 'relu'.  A back-end without the entry raises; the call is never downgraded.
    ``conv3x3_s2_eval_fp16`` is the form of include/skd_infer2h.h with ``pack = conv3x3_pack_weights_fp16(conv)``: two fp16
    pieces, scaled residual, conv3x3_split_eval_fp16's output at the even pixels bit for bit."""
    form = _WIDE[check_pieces(pieces, piece_format)]
    if activation not in ("none", "relu"):
        raise ValueError("conv3x3_s2_eval: activation must be 'none' or 'relu', not %r" % (activation,))
    if torch.is_grad_enabled() and x.requires_grad:
        raise RuntimeError("conv3x3_s2_eval is inference-only")
    _need(form.s2, form.bytes)
    b, cin, h, w = x.shape
    mean, var, gamma, beta, eps, slope = _bn_epilogue(bn)
    lib, out = _conv3x3_begin(form, form.s2, x, x.shape, pack, cout, ((h - 1) // 2 + 1, (w - 1) // 2 + 1), conv_bias, mean, var,
                              gamma, beta)
    _lib.check(getattr(lib, form.s2)(b, h, w, cin, cout, x.data_ptr(), pack.data_ptr(), out.data_ptr(), _lib.ptr(conv_bias),
                                     _lib.ptr(mean), _lib.ptr(var), _lib.ptr(gamma), _lib.ptr(beta), eps, _ACT[activation], slope,
                                     *((pieces,) if form.s2_pieces else ()), 0, _lib.stream_of(x)), form.s2)
    return out


def conv3x3_s2_eval(x, pack, cout, conv_bias=None, bn=None, activation="none", pieces=3):
    return _conv3x3_s2_eval(x, pack, cout, conv_bias, bn, activation, pieces)


def conv3x3_s2_eval_fp16(x, pack, cout, conv_bias=None, bn=None, activation="none"):
    """``conv3x3_s2_eval`` on two FP16 pieces per operand with the scaled residual (include/skd_infer2h.h), with
    ``pack = conv3x3_pack_weights_fp16(conv)``; never downgraded (a back-end without the entry raises NotImplementedError)."""
    return _conv3x3_s2_eval(x, pack, cout, conv_bias, bn, activation, 2, "fp16")


conv3x3_s2_eval.__doc__ = _conv3x3_s2_eval.__doc__


def conv3x3_narrow_train_supported(x, weight, stride, padding, dilation, groups):
    """True when conv3x3_split_train(..., narrow=True) takes the convolution of a network that is being trained: everything
    conv3x3_train_supported asks, except that each direction need only fit the wide form OR the narrow one -- Cin and Cout
    multiples of 64 -- and the back-end has the entries of include/skd_narrow.h as well."""
    return (_conv3x3_ok(x, weight, stride, padding, dilation, groups, grad=True, entries=_TRAIN_ENTRIES + _NARROW_ENTRIES,
                        query=_NARROW3.query, host_ok=True)
            and bool(getattr(_lib.get(), _NARROW3.query)(int(weight.shape[0]), int(weight.shape[1]), int(stride), int(padding),
                                                         int(dilation), int(groups))))


def _conv3x3_narrow_train_packs(weight, owner):
    """``(pack_fwd, pack_bwd, fwd_form, bwd_form)`` of a trained weight whose directions are chosen by their N -- Cout for the
    forward, Cin for the data gradient: _WIDE3 and its image for a multiple of 128, _NARROW3 and its image otherwise.  One launch
    per entry that has an image to write, each cached in a slot of its own; both wide is conv3x3_train_packs."""
    cout, cin = int(weight.shape[0]), int(weight.shape[1])
    narrow = (cout % 128 != 0, cin % 128 != 0)
    forms = tuple(_NARROW3 if n else _WIDE3 for n in narrow)
    if not any(narrow):
        return conv3x3_train_packs(weight, owner) + forms
    wide = (None, None)
    if not all(narrow):
        wide = _conv3x3_packs(weight, owner, _WIDE3.mixed_slot, _WIDE3.pack_pair, "conv3x3_split_train",
                              (not narrow[0], not narrow[1]), _WIDE3.bytes)
    thin = _conv3x3_packs(weight, owner, _NARROW3.train_slot, _NARROW3.pack_pair, "conv3x3_split_train", narrow, _NARROW3.bytes)
    return tuple(t if n else v for t, v, n in zip(thin, wide, narrow)) + forms


_device_cus = {}


def conv3x3_wgrad_supported(x, weight, stride, padding, dilation, groups):
    """True when conv3x3_split_wgrad takes the weight gradient of ``F.conv2d(x, weight, bias, stride, padding, dilation, groups)``:
    a back-end that has the three entries of include/skd_wgrad.h (the tests' C double does not: the gradient then comes from the
    library, as before) and everything conv3x3_train_supported asks."""
    return (_has(*_WGRAD_ENTRIES) and conv3x3_train_supported(x, weight, stride, padding, dilation, groups)
            and bool(getattr(_lib.get(), _WIDE3.wgrad_query)(int(weight.shape[1]), int(weight.shape[0]), int(stride),
                                                             int(padding), int(dilation), int(groups))))


def _cus_of(device):
    """Compute units of ``device``, looked up once per device (0 -- the plan's default -- for a host tensor under a test double)."""
    if device.type != "cuda":
        return 0
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in _device_cus:
        _device_cus[key] = int(torch.cuda.get_device_properties(key).multi_processor_count)
    return _device_cus[key]


def _non_overlapping_and_dense(t):
    """Whether the elements of ``t`` fill a block of memory exactly once, in whatever dimension order."""
    want = 1
    for size, stride in sorted(((int(n), int(s)) for n, s in zip(t.shape, t.stride()) if n != 1), key=lambda p: p[1]):
        if stride != want:
            return False
        want *= size
    return True


def _conv3x3_wgrad_launch(form, what, x, g, weight_like, dilation, slices, word=()):
    """The body the four weight-gradient ops share: the checks, the plan call, the workspace, the layout of ``dw`` and the launch
    entry, on the plan / launch pair of ``form``; a back-end without the pair raises.  ``word``: ``(pointer,)`` for the form whose
    entry takes the scale word of ``g`` in front of the slice count (skd_train2h.h)."""
    plan_entry, run_entry = form.wgrad
    _need(plan_entry, run_entry)
    _lib.require_device(x, g)
    lib = _lib.get()
    b, cin, h, w = (int(v) for v in x.shape)
    cout = int(g.shape[1])
    if tuple(weight_like.shape) != (cout, cin, 3, 3) or tuple(g.shape) != (b, cout, h, w):
        raise ValueError("%s: x %s, g %s, weight %s" % (what, tuple(x.shape), tuple(g.shape), tuple(weight_like.shape)))
    if not (_fp32_cl_map(x, True) and _fp32_cl_map(g, True)):
        raise ValueError("%s: fp32 channels-last maps expected" % what)
    plan = (ctypes.c_int64 * 3)()
    _lib.check(getattr(lib, plan_entry)(b, h, w, cin, cout, int(slices), _cus_of(x.device), ctypes.cast(plan, ctypes.c_void_p)),
               plan_entry)
    ws = torch.empty((int(plan[2]),), dtype=torch.uint8, device=x.device)
    if _non_overlapping_and_dense(weight_like):
        dw = torch.empty_strided(tuple(weight_like.shape), tuple(weight_like.stride()), dtype=torch.float32, device=x.device)
    else:
        dw = torch.empty(tuple(weight_like.shape), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    _lib.check(getattr(lib, run_entry)(b, h, w, cin, cout, int(dilation), x.data_ptr(), g.data_ptr(), dw.data_ptr(),
                                       *(int(v) for v in dw.stride()), ws.data_ptr(), int(plan[2]), *word, int(plan[0]),
                                       _lib.stream_of(x)), run_entry)
    return dw


def conv3x3_split_wgrad(x, g, weight_like, dilation, slices=0):
    """The weight gradient of the same-size 3x3 convolution ``F.conv2d(x, w, None, 1, dilation, dilation)`` for the output gradient
    ``g``, on the split core (csrc/conv3x3_wgrad.hip: both operands split in the loop, split-K over the pixels into a workspace,
    a second launch that sums the slices in a fixed order -- the same bits on every call).  ``x`` (B, Cin, H, W) and ``g``
    (B, Cout, H, W): fp32, channels-last, 16-byte aligned.  ``weight_like`` gives shape, device and layout of the result: its own
    strides when it is non-overlapping and dense, channels-last otherwise (a channel slice of a wider weight).  ``slices``: 0 =
    the plan's choice for the tensor's device.
    ``conv3x3_split_wgrad2``: the two-piece form of include/skd_train2.h -- both operands cut into two bf16 pieces, three
    products, the same plan, workspace and slice sum (the numerics of conv3x3_split_eval's ``pieces=2``).  A back-end without
    the entries raises NotImplementedError."""
    return _conv3x3_wgrad_launch(_WIDE3, "conv3x3_split_wgrad", x, g, weight_like, dilation, slices)


def conv3x3_split_wgrad2(x, g, weight_like, dilation, slices=0):
    """``conv3x3_split_wgrad`` on two bf16 pieces per operand and three products (include/skd_train2.h): the same arguments, the
    same plan and result layout."""
    return _conv3x3_wgrad_launch(_WIDE2, "conv3x3_split_wgrad", x, g, weight_like, dilation, slices)


def _check_word(word, like):
    if word is not None and (word.dtype != torch.int32 or word.numel() != 1 or word.device != like.device):
        raise ValueError("word: the one-element int32 tensor of fp16_scale_word on the gradient's device expected")
    return word


def conv3x3_split_wgrad_fp16(x, g, weight_like, dilation, slices=0, word=None):
    """``conv3x3_split_wgrad`` on two FP16 pieces per operand and three products (include/skd_train2h.h): ``g``'s rows are
    multiplied by the power of two of ``word`` (``fp16_scale_word(g)``) in front of the split, the result by its reciprocal;
    ``x`` is not scaled and keeps skd_split2h.h's loud contract (|x| > 65504 gives NaN).  ``word=None``: scale 1 -- gradients
    below fp16's range are then lost, so a caller passes the word.  The same plan, workspace, slice sum and result layout; 22
    significant bits per operand.  A back-end without the entries raises NotImplementedError."""
    _lib.require_device(_check_word(word, g))
    return _conv3x3_wgrad_launch(_WIDE2H, "conv3x3_split_wgrad_fp16", x, g, weight_like, dilation, slices, (_lib.ptr(word),))


def _conv3x3_scaled_launch(g, pack, cout, dilation, word, form=_WIDE2H):
    """conv3x3(g) on the image ``pack`` of ``form`` with ``g`` scaled by its ``word``, by the form's scaled entry: the data gradient
    of include/skd_train2h.h (the one form that has such an entry), one launch, raw."""
    b, cin, h, w = g.shape
    lib, out = _conv3x3_begin(form, form.scaled, g, g.shape, pack, cout, (h, w), _check_word(word, g))
    _lib.check(getattr(lib, form.scaled)(b, h, w, cin, cout, int(dilation), g.data_ptr(), pack.data_ptr(), out.data_ptr(),
                                         word.data_ptr(), 0, _lib.stream_of(g)), form.scaled)
    return out


def conv3x3_narrow_wgrad_supported(x, weight, stride, padding, dilation, groups):
    """True when conv3x3_narrow_wgrad takes the weight gradient of ``F.conv2d(x, weight, bias, stride, padding, dilation, groups)``:
    a back-end that has the three entries of include/skd_narrow_wgrad.h (the tests' C double does not: the gradient then comes from
    the library, as before), everything conv3x3_narrow_train_supported asks, and Cin and Cout multiples of 64."""
    return (_has(*_NARROW_WGRAD_ENTRIES)
            and conv3x3_narrow_train_supported(x, weight, stride, padding, dilation, groups)
            and bool(getattr(_lib.get(), _NARROW3.wgrad_query)(int(weight.shape[1]), int(weight.shape[0]), int(stride),
                                                               int(padding), int(dilation), int(groups))))


def conv3x3_narrow_wgrad(x, g, weight_like, dilation, slices=0):
    """conv3x3_split_wgrad for channel counts that are multiples of 64: the 128 x 64 tile form of the same kernel
    (csrc/conv3x3_wgrad.hip, include/skd_narrow_wgrad.h) -- the same arguments, the same result layout, the same numerics; for a
    shape both take and the same slice count, the same bits."""
    return _conv3x3_wgrad_launch(_NARROW3, "conv3x3_narrow_wgrad", x, g, weight_like, dilation, slices)


class _Conv3x3SplitTrain(Function):
    """A same-size 3x3 convolution of a network in training, both directions on csrc/conv3x3.hip: the forward on ``pack_fwd``, the
    data gradient -- the same kind of convolution of the output gradient with the flipped, transposed weight -- on the
    ``pack_bwd`` THIS forward was given (kept in ctx: an optimizer step in between changes the cache, not this node).  The
    weight gradient (and the bias gradient) are the library's, as before.  ``cfg`` (a _TrainForms) says the rest: ``cfg.fwd`` and
    ``cfg.bwd`` are the table rows of the forward and of the data gradient -- chosen per direction by conv3x3_split_train's
    ``narrow``, two-plane images and two-piece entries from conv3x3_split_train2, the fp16 pair from conv3x3_split_train_fp16,
    whose row has a scaled data gradient: the backward then computes the scale word of ``g`` ONCE and hands it to that entry and
    to the weight gradient.  ``cfg.wgrad``: the row whose public weight-gradient op computes ``dw`` where the back-end has that
    op's entries (the library then computes the bias gradient alone), or None.  ``cfg.stats`` makes the forward return
    ``(y, partials)`` -- the same ``y`` and the statistics records of include/skd_bnstats.h, marked non-differentiable; the
    backward is the same."""

    @staticmethod
    def forward(ctx, x, weight, bias, dilation, pack_fwd, pack_bwd, cfg):
        _lib.require_device(x, weight, bias, pack_fwd, pack_bwd)
        ctx.save_for_backward(x, weight)
        ctx.pack_bwd, ctx.dilation, ctx.has_bias, ctx.cfg = pack_bwd, int(dilation), bias is not None, cfg
        if cfg.stats:
            y, partials = _conv3x3_stats_launch(cfg.fwd, x, pack_fwd, int(weight.shape[0]), dilation, bias)
            ctx.mark_non_differentiable(partials)
            return y, partials
        return _conv3x3_raw_launch(cfg.fwd, x, pack_fwd, int(weight.shape[0]), dilation, bias)

    @staticmethod
    @once_differentiable
    def backward(ctx, g, *_partials_grad):
        x, weight = ctx.saved_tensors         # a weight written since the forward raises autograd's version error here
        d, bwd, wg = ctx.dilation, ctx.cfg.bwd, ctx.cfg.wgrad
        g = _cl(g.to(torch.float32))
        if g.data_ptr() % 16:
            g = g.clone(memory_format=torch.channels_last)
        dx = dw = db = None
        # (the entries of the op launched below: its geometry query where it has one, its plan and launch entries)
        split_w = (wg is not None and ctx.needs_input_grad[1]
                   and _has(*((wg.wgrad_query,) if wg.wgrad_query else ()), *wg.wgrad))
        # a form with a scaled entry: ONE scale word of g for both gradient products
        scaled_w = split_w and wg.scaled is not None
        word = fp16_scale_word(g) if (ctx.needs_input_grad[0] and bwd.scaled) or scaled_w else None
        if ctx.needs_input_grad[0]:
            if bwd.scaled:
                dx = _conv3x3_scaled_launch(g, ctx.pack_bwd, int(weight.shape[1]), d, word, bwd)
            else:
                dx = _conv3x3_raw_launch(bwd, g, ctx.pack_bwd, int(weight.shape[1]), d)
        need_w, need_b = ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        if split_w:
            # (the public op, by its name on this module at call time)
            dw = globals()[wg.wgrad_op](x, g, weight, d, **(dict(word=word) if scaled_w else {}))
            need_w = False
        if need_w or need_b:
            _, lw, db = torch.ops.aten.convolution_backward(g, x, weight, [int(weight.shape[0])] if ctx.has_bias else None,
                                                            [1, 1], [d, d], [d, d], False, [0, 0], 1, (False, need_w, need_b))
            dw, db = lw if need_w else dw, db if need_b else None
        return dx, dw, db, None, None, None, None      # dilation, the two packs and cfg take no gradient


def _conv3x3_split_train(x, weight, dilation, bias=None, owner=None, *, wgrad=False, narrow=False, narrow_wgrad=False, stats=False,
                         pieces=3):
    """``F.conv2d(x, weight, bias, 1, dilation, dilation)`` for a call conv3x3_train_supported accepted, differentiable: forward
    and data gradient are one launch each of the split-core implicit GEMM (csrc/conv3x3.hip: fp32 in and out, three bf16 pieces,
    six products, fp32 accumulation; the numerics of conv3x3_split_eval in both directions), the weight and bias gradients come
    from ``aten.convolution_backward``.  The weight is split once per version (conv3x3_train_packs, cached on ``owner``); the
    bias is added in the forward's epilogue.  ``wgrad=True`` (opt-in): the weight gradient runs on the split core too
    (conv3x3_split_wgrad) where the back-end has the entries of include/skd_wgrad.h; the bias gradient stays with the library.
    ``narrow=True`` (opt-in; conv3x3_narrow_train_supported says when): each direction is chosen by its N -- Cout for the forward,
    Cin for the data gradient: the 128-column tiles for a multiple of 128, the 64-column ones otherwise -- which takes one pack
    launch per entry and weight version; the weight gradient of a shape with a 64-channel side stays with the library (``wgrad``
    is ignored for it) unless ``narrow_wgrad=True`` (a further opt-in, effective only with ``narrow``): then it is
    conv3x3_narrow_wgrad's where the back-end has the entries of include/skd_narrow_wgrad.h, the bias gradient the library's.
    ``stats=True`` (opt-in; conv3x3_bnstats_supported says when, a back-end without the entries raises): returns
    ``(y, partials)`` -- ``y`` bit for bit what the call returns without it, and ``partials``, the batch-norm statistics records the
    forward's epilogue wrote (include/skd_bnstats.h: one (mean, M2) per 32-row block of B * H * W and output channel), not
    differentiable, for ``abn_relu_train(y, ..., partials=partials)``.  The backward, and ``wgrad`` / ``narrow`` /
    ``narrow_wgrad``, are what they are without it.
    ``conv3x3_split_train2`` (opt-in, an ACCURACY trade; include/skd_train2.h): forward, data gradient and -- with ``wgrad`` -- weight
    gradient of the WIDE form on two bf16 pieces per operand and three products: 16 significant bits per operand, every element
    within 2^-15 of the sum of absolute products of the exact result.  The packs are the two-plane pair (conv3x3_train_packs2),
    cached apart from the three-piece pair.  A direction ``narrow`` puts on the 64-column form and a call with
    ``stats`` have no two-piece form: they keep three pieces.  The library's weight gradient (``wgrad=False``) and the bias gradient
    are what they were.  A back-end without the entries raises NotImplementedError."""
    form = _WIDE[check_pieces(pieces)]
    if stats:
        _need(*_BNSTATS_ENTRIES)
    if form is not _WIDE3:      # never downgraded -- while a three-piece call without skd_wgrad.h leaves the weight gradient on the library
        _need(form.pack_pair, form.conv, form.bytes, *(form.wgrad if wgrad else ()))
    if narrow:
        pack_fwd, pack_bwd, fwd, bwd = _conv3x3_narrow_train_packs(weight, owner)
        if _NARROW3 in (fwd, bwd):
            return _Conv3x3SplitTrain.apply(x, weight, bias, int(dilation), pack_fwd, pack_bwd,
                                            _TrainForms(fwd, bwd, _NARROW3 if narrow_wgrad else None, bool(stats)))
    if stats and form.stats is None:
        form = _WIDE3
    return _conv3x3_train_apply(form, x, weight, dilation, bias, owner, wgrad, stats)


def _conv3x3_train_apply(form, x, weight, dilation, bias, owner, wgrad, stats=False):
    """_Conv3x3SplitTrain with both directions on the wide ``form``, its pack pair from the form's public pack op (by its name on
    this module at call time)."""
    pack_fwd, pack_bwd = globals()[form.packs_op](weight, owner)
    return _Conv3x3SplitTrain.apply(x, weight, bias, int(dilation), pack_fwd, pack_bwd,
                                    _TrainForms(form, form, form if wgrad else None, bool(stats)))


def conv3x3_split_train(x, weight, dilation, bias=None, owner=None, *, wgrad=False, narrow=False, narrow_wgrad=False, stats=False):
    return _conv3x3_split_train(x, weight, dilation, bias, owner, wgrad=wgrad, narrow=narrow, narrow_wgrad=narrow_wgrad, stats=stats)


def conv3x3_split_train2(x, weight, dilation, bias=None, owner=None, *, wgrad=False, narrow=False, narrow_wgrad=False, stats=False):
    """``conv3x3_split_train`` with the wide form on two bf16 pieces per operand and three products (include/skd_train2.h)."""
    return _conv3x3_split_train(x, weight, dilation, bias, owner, wgrad=wgrad, narrow=narrow, narrow_wgrad=narrow_wgrad, stats=stats,
                                pieces=2)


conv3x3_split_train.__doc__ = _conv3x3_split_train.__doc__


def conv3x3_split_train_fp16(x, weight, dilation, bias=None, owner=None, *, wgrad=False, narrow=False, narrow_wgrad=False,
                             stats=False):
    """``conv3x3_split_train`` with the WIDE form on two FP16 pieces per operand, a scaled residual and three products
    (include/skd_train2h.h; opt-in): 22 significant bits per operand -- the three-piece accuracy at the two-piece product count.
    The forward is skd_conv3x3_split2h_nhwc on the fp16 forward pack (conv3x3_train_packs_fp16, cached apart from the bf16
    pairs); ``x`` and the weight are NOT scaled, so it keeps skd_split2h.h's loud contract: |x| or |w| above 65504 gives NaN.  The
    backward computes the scale word of the output gradient once (fp16_scale_word) and hands it to the scaled data gradient and,
    with ``wgrad``, to conv3x3_split_wgrad_fp16: gradients far below fp16's range lose nothing, a non-finite gradient stays
    non-finite.  A direction ``narrow`` puts on the 64-column form and a call with ``stats`` have no fp16 form: they keep three
    bf16 pieces, as under conv3x3_split_train2.  The library's weight gradient (``wgrad=False``) and the bias gradient are what
    they were.  A back-end without the entries raises NotImplementedError."""
    form = _WIDE2H
    _need(form.pack_pair, form.bytes, form.conv, *_SCALE_WORD, form.scaled, *(form.wgrad if wgrad else ()))
    # (a 64-channel side, decided from the shape as _conv3x3_narrow_train_packs decides it, in front of any pack launch)
    if stats or (narrow and (int(weight.shape[0]) % 128 != 0 or int(weight.shape[1]) % 128 != 0)):
        return _conv3x3_split_train(x, weight, dilation, bias, owner, wgrad=wgrad, narrow=narrow, narrow_wgrad=narrow_wgrad,
                                    stats=stats)
    return _conv3x3_train_apply(form, x, weight, dilation, bias, owner, wgrad)


# ---- the training student's 1x1 down-sample (shortcut) convolutions on the split core (include/skd_shortcut.h) ----
_SHORTCUT_ENTRIES = ("skd_conv1x1_train_supported", "skd_conv1x1_train_fwd_nhwc", "skd_conv1x1_train_dgrad_nhwc",
                     "skd_conv1x1_train_wgrad_plan", "skd_conv1x1_train_wgrad_nhwc")
SHORTCUT_PRODUCTS = ("fwd", "dgrad", "wgrad")


def conv1x1_train_supported(x, weight, stride, padding, dilation, groups):
    """True when conv1x1_split_train takes ``F.conv2d(x, weight, None, stride, padding, dilation, groups)`` of a network that is
    being trained: grad enabled, a back-end that has the entries of include/skd_shortcut.h (the tests' C double does not: callers
    then run the convolution they ran before), an fp32 channels-last 16-byte-aligned device input (a host one only under a test
    double) and a (Cout, Cin, 1, 1) fp32 weight on its device that skd_conv1x1_train_supported takes: stride 1 or 2, no padding,
    no dilation, ungrouped, Cin and Cout multiples of 64."""
    if not torch.is_grad_enabled() or not all(_lib.has_entry(n) for n in _SHORTCUT_ENTRIES):
        return False
    if not (_fp32_cl_map(x, True) and x.data_ptr() % 16 == 0):
        return False
    if not (weight.dim() == 4 and tuple(weight.shape[2:]) == (1, 1) and weight.dtype == torch.float32
            and weight.device == x.device and x.shape[1] == weight.shape[1] * groups):
        return False
    return bool(_lib.get().skd_conv1x1_train_supported(int(weight.shape[1]), int(weight.shape[0]), 1, int(stride), int(padding),
                                                       int(dilation), int(groups)))


def _conv1x1_train_mats(weight, owner):
    """``(w, wt)``: the dense (Cout, Cin) matrix of a (Cout, Cin, 1, 1) weight (the weight's own memory where that is dense) and its
    dense (Cin, Cout) transpose, the B operands of forward and data gradient.  Built under no_grad once per weight version and
    cached on ``owner`` by THE RULE above _version_key, like the 3x3 packs."""
    def build():
        with torch.no_grad():
            w = weight.detach().reshape(weight.shape[0], weight.shape[1])
            w = w if w.is_contiguous() and w.data_ptr() % 16 == 0 else w.clone(memory_format=torch.contiguous_format)
            return w, w.t().contiguous()
    return _cached(owner, "_skd_conv1x1_train_mats", _version_key((weight,), tuple(weight.shape), tuple(weight.stride())), build,
                   hold=weight)


def drop_conv1x1_train_mats(owner):
    """Forget the matrices conv1x1_split_train cached on ``owner``."""
    (owner if isinstance(owner, dict) else vars(owner)).pop("_skd_conv1x1_train_mats", None)


def _shortcut_out(h, stride):
    return (int(h) - 1) // int(stride) + 1


def conv1x1_train_wgrad(x, g, stride, slices=0):
    """The (Cout, Cin, 1, 1) weight gradient of ``F.conv2d(x, w, None, stride)`` for the output gradient ``g`` on the split core
    (the one-tap form of csrc/conv3x3_wgrad.hip: split-K over the output pixels into a workspace sized by
    skd_conv1x1_train_wgrad_plan for the device's compute units, a second launch that sums the slices in slice order -- the same
    bits on every call).  ``x`` and ``g``: fp32, channels-last, 16-byte aligned.  ``slices``: 0 = the plan's choice."""
    _lib.require_device(x, g)
    lib = _lib.get()
    b, cin, h, w = (int(v) for v in x.shape)
    cout = int(g.shape[1])
    if tuple(g.shape) != (b, cout, _shortcut_out(h, stride), _shortcut_out(w, stride)):
        raise ValueError("conv1x1_train_wgrad: x %s, g %s, stride %d" % (tuple(x.shape), tuple(g.shape), stride))
    if not (_fp32_cl_map(x, True) and _fp32_cl_map(g, True)):
        raise ValueError("conv1x1_train_wgrad: fp32 channels-last maps expected")
    plan = (ctypes.c_int64 * 3)()
    _lib.check(lib.skd_conv1x1_train_wgrad_plan(b, h, w, cin, cout, int(stride), int(slices), _cus_of(x.device),
                                                ctypes.cast(plan, ctypes.c_void_p)), "skd_conv1x1_train_wgrad_plan")
    ws = torch.empty((int(plan[2]),), dtype=torch.uint8, device=x.device)
    dw = torch.empty((cout, cin, 1, 1), dtype=torch.float32, device=x.device)
    _lib.check(lib.skd_conv1x1_train_wgrad_nhwc(b, h, w, cin, cout, int(stride), x.data_ptr(), g.data_ptr(), dw.data_ptr(),
                                                ws.data_ptr(), int(plan[2]), int(plan[0]), _lib.stream_of(x)),
               "skd_conv1x1_train_wgrad_nhwc")
    return dw


class _Conv1x1SplitTrain(Function):
    """A 1x1 convolution (stride 1 or 2, no padding, no bias) of a network in training.  The products listed in ``products`` run on
    the entries of include/skd_shortcut.h, the others on the library as before.  The data gradient uses the transposed weight
    THIS forward was given (kept in ctx: an optimizer step in between changes the cache, not this node)."""

    @staticmethod
    def forward(ctx, x, weight, stride, w, wt, products):
        _lib.require_device(x, weight, w, wt)
        ctx.save_for_backward(x, weight)
        ctx.wt, ctx.stride, ctx.products = wt, int(stride), products
        if "fwd" not in products:
            return torch.nn.functional.conv2d(x, weight, None, ctx.stride)
        b, cin, h, wd = (int(v) for v in x.shape)
        cout = int(weight.shape[0])
        # a plain allocation, not a view made inside the Function: the ABN that follows writes into it in place
        y = torch.empty((b, cout, _shortcut_out(h, stride), _shortcut_out(wd, stride)), dtype=torch.float32, device=x.device,
                        memory_format=torch.channels_last)
        _lib.check(_lib.get().skd_conv1x1_train_fwd_nhwc(b, h, wd, cin, cout, ctx.stride, x.data_ptr(), w.data_ptr(), y.data_ptr(),
                                                         _lib.stream_of(x)), "skd_conv1x1_train_fwd_nhwc")
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, weight = ctx.saved_tensors         # a weight written since the forward raises autograd's version error here
        s = ctx.stride
        g = _cl(g.to(torch.float32))
        if g.data_ptr() % 16:
            g = g.clone(memory_format=torch.channels_last)
        b, cin, h, wd = (int(v) for v in x.shape)
        cout = int(weight.shape[0])
        dx = dw = None
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if need_x and "dgrad" in ctx.products:
            dx = torch.empty((b, cin, h, wd), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
            _lib.check(_lib.get().skd_conv1x1_train_dgrad_nhwc(b, h, wd, cin, cout, s, g.data_ptr(), ctx.wt.data_ptr(), dx.data_ptr(),
                                                               _lib.stream_of(x)), "skd_conv1x1_train_dgrad_nhwc")
            need_x = False
        if need_w and "wgrad" in ctx.products:
            dw = conv1x1_train_wgrad(x, g, s)
            need_w = False
        if need_x or need_w:
            lx, lw, _ = torch.ops.aten.convolution_backward(g, x, weight, None, [s, s], [0, 0], [1, 1], False, [0, 0], 1,
                                                            (need_x, need_w, False))
            dx, dw = lx if need_x else dx, lw if need_w else dw
        return dx, dw, None, None, None, None


def conv1x1_split_train(x, weight, stride, owner=None, *, products=SHORTCUT_PRODUCTS):
    """``F.conv2d(x, weight, None, stride)`` for a call conv1x1_train_supported accepted, differentiable.  ``products`` names what
    runs on the split core (csrc/conv1x1_train.hip, include/skd_shortcut.h: fp32 in and out, three bf16 pieces, six products, fp32
    accumulation): "fwd", "dgrad" (every element of the input gradient is written: for stride 2 the pixels no output reads are
    +0.0) and "wgrad" (conv1x1_train_wgrad); a product not listed comes from ``F.conv2d`` / ``aten.convolution_backward`` as
    before.  The dense weight matrix and its transpose are built once per weight version (cached on ``owner`` like the 3x3 packs;
    a fused optimizer needs networks.kd_model.advance_versions_after_step).  The output is a plain channels-last allocation, not
    a view: an in-place ABN may write into it."""
    products = tuple(p for p in SHORTCUT_PRODUCTS if p in products)
    w, wt = _conv1x1_train_mats(weight, owner)
    return _Conv1x1SplitTrain.apply(x, weight, int(stride), w, wt, products)


def seg_confusion(logits, target=None, ignore_index=255, confusion=None, want_pred=True):
    """Evaluation tail (networks/evaluate.py:106-113, 186-198): bilinear (align_corners) upsample of ``logits``
    (B, C, h, w) to the size of ``target`` (B, H, W) [or of ``want_pred`` = (H, W) when no target], argmax over the
    classes (first maximum, uint8) and accumulation of the (C, C) int64 ``confusion`` matrix over the pixels whose
    label is not ``ignore_index`` -- one fused kernel, bit-exact integer results.  Returns (pred or None, confusion)."""
    _lib.require_device(logits, target, confusion)
    lg = _f32c(logits.detach(), "seg_confusion")
    b, c, h, w = lg.shape
    if target is not None:
        if target.dtype != torch.int64:
            raise TypeError("seg_confusion: int64 target expected (got %s)" % target.dtype)
        tg = target if target.is_contiguous() else target.contiguous()
        H, W = tg.shape[1], tg.shape[2]
        if confusion is None:
            confusion = torch.zeros((c, c), dtype=torch.int64, device=lg.device)
    else:
        tg = None
        H, W = want_pred
    pred = torch.empty((b, H, W), dtype=torch.uint8, device=lg.device) if want_pred else None
    _lib.check(_lib.get().skd_seg_confusion(b, c, h, w, H, W, lg.data_ptr(), _lib.ptr(tg), int(ignore_index), _lib.ptr(pred),
                                            _lib.ptr(confusion), _lib.stream_of(lg)), "skd_seg_confusion")
    return pred, confusion


SEG_SLIDING_MAX_CLASSES = 32   # csrc/evaluate_sliding.hip keeps 2 VGPRs per class; the entry point refuses more


def seg_sliding(logits, tiles, tile_size, out_size, target=None, ignore_index=255, confusion=None, remap=None, want_pred=True,
                want_probs=False):
    """Sliding-window evaluation tail (networks/evaluate.py:70-104, 187-198) as one fused kernel: tile ``t``'s ``logits``
    (T, C, h, w) are up-sampled (bilinear, align_corners) to ``tile_size``, cropped and accumulated in float64 over the
    window ``tiles[t] = (y1, x1, y2, x2)`` of the ``out_size`` = (H, W) image in table order; mean over the covering tiles,
    argmax (first maximum), optional 256-entry uint8 ``remap`` of the written prediction, (C, C) int64 ``confusion``
    accumulated with the un-remapped prediction over the pixels of ``target`` (H, W) int64 that are not ``ignore_index``.
    ``tiles``: a host sequence of 4-tuples (checked, then uploaded) or a (T, 4) int32 tensor on the logits' device.
    Returns (pred (H, W) uint8 or None, probs (H, W, C) float64 or None, confusion [None without target and confusion])."""
    _lib.require_device(logits, target, confusion, remap)
    _need("skd_seg_sliding")
    lg = _f32c(logits.detach(), "seg_sliding")
    if lg.dim() != 4:
        raise ValueError("seg_sliding: logits (T, C, h, w) expected (got %s)" % (tuple(lg.shape),))
    nt, c, h, w = lg.shape
    if not 1 <= c <= SEG_SLIDING_MAX_CLASSES:
        raise ValueError("seg_sliding: 1 <= classes <= %d (got %d)" % (SEG_SLIDING_MAX_CLASSES, c))
    (th, tw), (H, W) = (int(v) for v in tile_size), (int(v) for v in out_size)
    if min(th, tw, H, W) <= 0:
        raise ValueError("seg_sliding: tile_size and out_size must be positive")
    if torch.is_tensor(tiles):
        if tiles.dtype != torch.int32 or tiles.device != lg.device or tuple(tiles.shape) != (nt, 4):
            raise TypeError("seg_sliding: tiles tensor must be (%d, 4) int32 on %s" % (nt, lg.device))
        tl = tiles if tiles.is_contiguous() else tiles.contiguous()
    else:
        rows = [tuple(int(v) for v in t) for t in tiles]
        if len(rows) != nt:
            raise ValueError("seg_sliding: %d tiles for %d logit maps" % (len(rows), nt))
        for y1, x1, y2, x2 in rows:
            if not (0 <= y1 < y2 <= H and 0 <= x1 < x2 <= W and y2 - y1 <= th and x2 - x1 <= tw):
                raise ValueError("seg_sliding: tile (%d, %d, %d, %d) does not fit a %d x %d image with %d x %d tiles"
                                 % (y1, x1, y2, x2, H, W, th, tw))
        tl = torch.tensor(rows, dtype=torch.int32).reshape(nt, 4).to(lg.device)
    if target is not None:
        if target.dtype != torch.int64:
            raise TypeError("seg_sliding: int64 target expected (got %s)" % target.dtype)
        if tuple(target.shape[-2:]) != (H, W) or target.numel() != H * W:
            raise ValueError("seg_sliding: target %s does not match out_size %s" % (tuple(target.shape), (H, W)))
        tg = target if target.is_contiguous() else target.contiguous()
        if confusion is None:
            confusion = torch.zeros((c, c), dtype=torch.int64, device=lg.device)
    else:
        tg = None
    if confusion is not None and (confusion.dtype != torch.int64 or tuple(confusion.shape) != (c, c) or not confusion.is_contiguous()):
        raise TypeError("seg_sliding: confusion must be a contiguous (%d, %d) int64 tensor" % (c, c))
    if remap is not None and (remap.dtype != torch.uint8 or remap.numel() != 256 or not remap.is_contiguous()):
        raise TypeError("seg_sliding: remap must be 256 contiguous uint8 entries")
    pred = torch.empty((H, W), dtype=torch.uint8, device=lg.device) if want_pred else None
    probs = torch.empty((H, W, c), dtype=torch.float64, device=lg.device) if want_probs else None
    _lib.check(_lib.get().skd_seg_sliding(nt, c, h, w, th, tw, H, W, lg.data_ptr(), tl.data_ptr(), _lib.ptr(tg), int(ignore_index),
                                          _lib.ptr(remap), _lib.ptr(pred), _lib.ptr(probs), _lib.ptr(confusion), _lib.stream_of(lg)),
               "skd_seg_sliding")
    return pred, probs, confusion


def zoom_size(n, scale):
    """Output length of ``scipy.ndimage.zoom`` for an axis of ``n`` at ``scale``: Python's ``round``, half to even
    (30 x 0.75 = 22.5 gives 22, 50 x 0.75 = 37.5 gives 38)."""
    return int(round(int(n) * float(scale)))


def zoom_linear(image, scale, mirror=False, channels_last=False):
    """``scipy.ndimage.zoom(image, (1, 1, scale, scale), order=1, prefilter=False)`` of networks/evaluate.py:127 as one kernel
    (csrc/evaluate_multiscale.hip): float64 coordinates and weights, one cast to fp32, and scipy's zeroed last row / column
    where the last coordinate rounds above ``n - 1``.  ``image``: (1, C, H, W) or (C, H, W) fp32.  Returns (F, C, Ho, Wo) with
    F = 1 + mirror; element 1 is element 0 mirrored in X.  ``channels_last``: the result has channels-last memory."""
    _lib.require_device(image)
    _need("skd_zoom_linear")
    img = _f32c(image.detach(), "zoom_linear")
    if img.dim() == 4 and img.shape[0] == 1:
        img = img[0]
    if img.dim() != 3:
        raise ValueError("zoom_linear: one image (1, C, H, W) or (C, H, W) expected (got %s)" % (tuple(image.shape),))
    c, h, w = img.shape
    ho, wo = zoom_size(h, scale), zoom_size(w, scale)
    if min(c, h, w) <= 0 or ho < 2 or wo < 2:
        raise ValueError("zoom_linear: a %d x %d image at scale %r gives %d x %d; both axes need at least 2" % (h, w, scale, ho, wo))
    f = 2 if mirror else 1
    out = torch.empty((f, c, ho, wo), dtype=torch.float32, device=img.device,
                      memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    _lib.check(_lib.get().skd_zoom_linear(c, h, w, ho, wo, img.data_ptr(), out.data_ptr(), int(bool(mirror)), int(bool(channels_last)),
                                          _lib.stream_of(img)), "skd_zoom_linear")
    return out


def seg_multiscale(logits, out_size, target=None, ignore_index=255, confusion=None, remap=None, want_pred=True, want_probs=False):
    """Multi-scale / flip evaluation tail (networks/evaluate.py:115-134, 187-198) as one fused kernel.  ``logits``: a list of
    per-scale (F, C, h_s, w_s) fp32 tensors, the same F (1, or 2 = [forward, forward of the X-mirrored image]) and C throughout.
    Per scale, in list order: align-corners upsample to ``out_size`` = (H, W) in fp32, with F = 2 the fp32 average
    ``0.5 * (a + b mirrored back)``, float64 sum; mean over the scales, argmax (first maximum), optional 256-entry uint8
    ``remap`` of the written prediction, (C, C) int64 ``confusion`` accumulated with the un-remapped prediction over the pixels
    of ``target`` (H, W) int64 that are not ``ignore_index``.
    Returns (pred (H, W) uint8 or None, probs (H, W, C) float64 or None, confusion [None without target and confusion])."""
    logits = list(logits)
    _lib.require_device(target, confusion, remap, *logits)
    _need("skd_seg_multiscale")
    if not logits:
        raise ValueError("seg_multiscale: at least one scale expected")
    maps = [_f32c(lg.detach(), "seg_multiscale") for lg in logits]
    if any(m.dim() != 4 for m in maps):
        raise ValueError("seg_multiscale: per-scale logits (F, C, h, w) expected (got %s)" % ([tuple(m.shape) for m in maps],))
    f, c = maps[0].shape[0], maps[0].shape[1]
    if f not in (1, 2):
        raise ValueError("seg_multiscale: F is 1, or 2 with a mirrored forward (got %d)" % f)
    if not 1 <= c <= SEG_SLIDING_MAX_CLASSES:
        raise ValueError("seg_multiscale: 1 <= classes <= %d (got %d)" % (SEG_SLIDING_MAX_CLASSES, c))
    H, W = (int(v) for v in out_size)
    if min(H, W) <= 0:
        raise ValueError("seg_multiscale: out_size must be positive")
    rows, off = [], 0
    for m in maps:
        if m.shape[0] != f or m.shape[1] != c:
            raise ValueError("seg_multiscale: every scale needs the same (F, C) = (%d, %d) (got %s)" % (f, c, tuple(m.shape)))
        if min(m.shape[2], m.shape[3]) < 1 or m.numel() > 2 ** 31 - 1:
            raise ValueError("seg_multiscale: a per-scale map holds between 1 and 2^31 - 1 floats (got %s)" % (tuple(m.shape),))
        if m.device != maps[0].device:
            raise ValueError("seg_multiscale: all scales on one device expected")
        rows.append((off, m.shape[2], m.shape[3]))
        off += m.numel()
    dev = maps[0].device
    packed = maps[0].reshape(-1) if len(maps) == 1 else torch.cat([m.reshape(-1) for m in maps])
    table = torch.tensor(rows, dtype=torch.int64).reshape(len(rows), 3).to(dev)
    if target is not None:
        if target.dtype != torch.int64:
            raise TypeError("seg_multiscale: int64 target expected (got %s)" % target.dtype)
        if tuple(target.shape[-2:]) != (H, W) or target.numel() != H * W:
            raise ValueError("seg_multiscale: target %s does not match out_size %s" % (tuple(target.shape), (H, W)))
        tg = target if target.is_contiguous() else target.contiguous()
        if confusion is None:
            confusion = torch.zeros((c, c), dtype=torch.int64, device=dev)
    else:
        tg = None
    if confusion is not None and (confusion.dtype != torch.int64 or tuple(confusion.shape) != (c, c) or not confusion.is_contiguous()):
        raise TypeError("seg_multiscale: confusion must be a contiguous (%d, %d) int64 tensor" % (c, c))
    if remap is not None and (remap.dtype != torch.uint8 or remap.numel() != 256 or not remap.is_contiguous()):
        raise TypeError("seg_multiscale: remap must be 256 contiguous uint8 entries")
    pred = torch.empty((H, W), dtype=torch.uint8, device=dev) if want_pred else None
    probs = torch.empty((H, W, c), dtype=torch.float64, device=dev) if want_probs else None
    _lib.check(_lib.get().skd_seg_multiscale(len(rows), f, c, H, W, packed.data_ptr(), table.data_ptr(), _lib.ptr(tg), int(ignore_index),
                                             _lib.ptr(remap), _lib.ptr(pred), _lib.ptr(probs), _lib.ptr(confusion),
                                             _lib.stream_of(packed)), "skd_seg_multiscale")
    return pred, probs, confusion


def pool_out_size(n, k):
    """ceil_mode=True, stride = kernel, no padding."""
    return -(-n // k)


class _MaxPoolArgmax(Function):
    @staticmethod
    def forward(ctx, x, kh, kw):
        _lib.require_device(x)
        x = _f32c(x, "max_pool_argmax")
        b, c, h, w = x.shape
        oh, ow = pool_out_size(h, kh), pool_out_size(w, kw)
        lib, st = _lib.get(), _lib.stream_of(x)
        pooled = x.new_empty((b, c, oh, ow))
        need = ctx.needs_input_grad[0]
        index = torch.empty((b, c, oh, ow), dtype=torch.int32, device=x.device) if need else None
        _lib.check(lib.skd_maxpool_argmax(b * c, h, w, kh, kw, x.data_ptr(), pooled.data_ptr(),
                                          _lib.ptr(index), st), "skd_maxpool_argmax")
        ctx.geom = (b, c, h, w, kh, kw)
        ctx.save_for_backward(index)
        return pooled

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (index,) = ctx.saved_tensors
        if index is None:
            return None, None, None
        b, c, h, w, kh, kw = ctx.geom
        g = _f32c(g, "max_pool_argmax backward")
        m = g.shape[2] * g.shape[3]
        dx = g.new_empty((b, c, h, w))
        lib, st = _lib.get(), _lib.stream_of(g)
        _lib.check(lib.skd_maxunpool_scatter(b * c, h, w, kh, kw, g.data_ptr(), m, index.data_ptr(),
                                             dx.data_ptr(), st), "skd_maxunpool_scatter")
        return dx, None, None


def max_pool_argmax(x, kh, kw, return_indices=False):
    """MaxPool2d(kernel=stride=(kh,kw), padding=0, ceil_mode=True).  Indices (bit-exact with
    PyTorch's: flat h*W+w of the first maximum, int32) are available through max_pool_indices()."""
    return _MaxPoolArgmax.apply(x, int(kh), int(kw))


def max_pool_indices(x, kh, kw):
    """(pooled, int32 argmax) without autograd -- used by the parity tests."""
    _lib.require_device(x)
    x = _f32c(x, "max_pool_indices")
    b, c, h, w = x.shape
    oh, ow = pool_out_size(h, kh), pool_out_size(w, kw)
    pooled = x.new_empty((b, c, oh, ow))
    index = torch.empty((b, c, oh, ow), dtype=torch.int32, device=x.device)
    _lib.check(_lib.get().skd_maxpool_argmax(b * c, h, w, int(kh), int(kw), x.data_ptr(), pooled.data_ptr(),
                                             index.data_ptr(), _lib.stream_of(x)), "skd_maxpool_argmax")
    return pooled, index


class _SimDis(Function):
    """sim_dis_compute(f_S, f_T) on pooled features (B, C, oh, ow)."""

    @staticmethod
    def forward(ctx, f_s, f_t):
        _lib.require_device(f_s, f_t)
        f_s, f_t = _f32c(f_s, "sim_dis"), _f32c(f_t, "sim_dis")
        b, cs = f_s.shape[0], f_s.shape[1]
        ct = f_t.shape[1]
        m = f_t.shape[-1] * f_t.shape[-2]                      # utils.py:181
        assert f_s.shape[0] == f_t.shape[0] and f_s.shape[2:] == f_t.shape[2:]
        lib, st = _lib.get(), _lib.stream_of(f_s)
        ldm = lib.skd_pairwise_ldm(m)
        need = ctx.needs_input_grad[0]
        fh_s = f_s.new_empty((b, cs, ldm))
        fh_t = f_s.new_empty((b, ct, ldm))
        norm_s = f_s.new_empty((b, m)) if need else None
        _lib.check(lib.skd_channel_l2_normalise(b, cs, m, f_s.data_ptr(), fh_s.data_ptr(), ldm,
                                                None, 0, _lib.ptr(norm_s), st),
                   "skd_channel_l2_normalise")
        _lib.check(lib.skd_channel_l2_normalise(b, ct, m, f_t.data_ptr(), fh_t.data_ptr(), ldm,
                                                None, 0, None, st), "skd_channel_l2_normalise")
        g = f_s.new_empty((b, ldm, ldm)) if need else None
        loss = f_s.new_empty(())
        ws = f_s.new_empty((max(1, lib.skd_pairwise_workspace_floats(b, m)),))
        _lib.check(lib.skd_pairwise_gram_loss(b, cs, ct, m, ldm, fh_s.data_ptr(), fh_t.data_ptr(),
                                              _lib.ptr(g), loss.data_ptr(), ws.data_ptr(), st),
                   "skd_pairwise_gram_loss")
        ctx.geom = (tuple(f_s.shape), m, ldm)
        ctx.save_for_backward(fh_s if need else None, g, norm_s)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, gl):
        fh_s, g, norm_s = ctx.saved_tensors
        if g is None:
            return None, None
        shape, m, ldm = ctx.geom
        b, cs = shape[0], shape[1]
        lib, st = _lib.get(), _lib.stream_of(g)
        gl = gl.to(torch.float32).contiguous()
        dp = g.new_empty((b, cs, ldm))
        ws = g.new_empty((max(1, lib.skd_pairwise_backward_workspace_floats(b, cs, m)),))
        _lib.check(lib.skd_pairwise_backward(b, cs, m, ldm, fh_s.data_ptr(), g.data_ptr(),
                                             norm_s.data_ptr(), gl.data_ptr(), dp.data_ptr(), ws.data_ptr(), st),
                   "skd_pairwise_backward")
        return dp[:, :, :m].reshape(shape), None


def sim_dis(f_s, f_t):
    """sum((A_T - A_S)^2) / M^2 / B with A = normalised Gram over channels (utils.py:173-183);
    the channel L2 norm is a constant for autograd (utils.py:175) and f_T gets no gradient."""
    return _SimDis.apply(f_s, f_t.detach())


def _channels_last_quads(t):
    """A (B, C, H, W) tensor that is stored channels-last with whole channel quads: the layout the PSP features have inside
    NetModel -- the pooling kernels read it as it is (skd_maxpool_argmax_nhwc) instead of through an NCHW copy."""
    return (t.dim() == 4 and t.shape[1] % 4 == 0 and t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous()
            and t.data_ptr() % 16 == 0)


def _pool_feature(lib, t, kh, kw, pooled, index, st):
    """pooled (B, C, M) / int32 argmax (flat h * W + w, or None) of MaxPool2d((kh, kw), ceil_mode=True) for either layout.
    Returns the tensor that was read (the caller keeps its layout for the backward)."""
    b, c, h, w = t.shape
    if _channels_last_quads(t):
        _lib.check(lib.skd_maxpool_argmax_nhwc(b, c, h, w, kh, kw, t.data_ptr(), pooled.data_ptr(), _lib.ptr(index), st),
                   "skd_maxpool_argmax_nhwc")
        return t
    t = t if t.is_contiguous() else t.contiguous()
    _lib.check(lib.skd_maxpool_argmax(b * c, h, w, kh, kw, t.data_ptr(), pooled.data_ptr(), _lib.ptr(index), st), "skd_maxpool_argmax")
    return t


def _unpool_feature(lib, nhwc, geom, dp, ldp, index, st):
    """d loss / d feature from the pooled gradient dp (B, C, ldp) through the argmax, in the layout the feature had."""
    b, cs, h, w, kh, kw = geom
    if nhwc:
        dx = torch.empty_strided((b, cs, h, w), (h * w * cs, 1, w * cs, cs), dtype=dp.dtype, device=dp.device)   # channels-last
        _lib.check(lib.skd_maxunpool_scatter_nhwc(b, cs, h, w, kh, kw, dp.data_ptr(), ldp, index.data_ptr(), dx.data_ptr(), st),
                   "skd_maxunpool_scatter_nhwc")
        return dx
    dx = dp.new_empty((b, cs, h, w))
    _lib.check(lib.skd_maxunpool_scatter(b * cs, h, w, kh, kw, dp.data_ptr(), ldp, index.data_ptr(), dx.data_ptr(), st),
               "skd_maxunpool_scatter")
    return dx


class _PairWise(Function):
    """Whole Pa loss in one node: pool(+argmax) -> normalise -> Gram/loss; backward scatters the
    pooled gradient straight from the padded GEMM output (no slice/copy in between).  Features may arrive NCHW-contiguous or
    channels-last (round 5: NetModel hands the PSP features over as they are); the student's gradient comes back in the
    layout its feature had."""

    @staticmethod
    def forward(ctx, feat_s, feat_t, kh, kw, split=False):
        _lib.require_device(feat_s, feat_t)
        for t in (feat_s, feat_t):
            if t.dtype != torch.float32:
                raise TypeError("pair_wise_loss: fp32 tensors only (got %s)" % t.dtype)
        b, cs, h, w = feat_s.shape
        ct = feat_t.shape[1]
        assert feat_t.shape[0] == b and tuple(feat_t.shape[2:]) == (h, w)
        oh, ow = pool_out_size(h, kh), pool_out_size(w, kw)
        m = oh * ow
        lib, st = _lib.get(), _lib.stream_of(feat_s)
        need = ctx.needs_input_grad[0]
        ctx.nhwc = _channels_last_quads(feat_s)
        if m <= 64:
            # small graphs (the reference default pools to 3 x 3 = 9 nodes): pool, then ONE fused launch for
            # normalise + both Grams + loss + gradient w.r.t. the pooled student features
            p_s, p_t = feat_s.new_empty((b, cs, m)), feat_s.new_empty((b, ct, m))
            index = torch.empty((b, cs, m), dtype=torch.int32, device=feat_s.device) if need else None
            _pool_feature(lib, feat_s, kh, kw, p_s, index, st)
            _pool_feature(lib, feat_t, kh, kw, p_t, None, st)
            loss = feat_s.new_empty(())
            dp = feat_s.new_empty((b, cs, m)) if need else None
            ws = feat_s.new_empty((b,))
            _lib.check(lib.skd_pairwise_small(b, cs, ct, m, p_s.data_ptr(), p_t.data_ptr(), loss.data_ptr(), _lib.ptr(dp),
                                              ws.data_ptr(), st), "skd_pairwise_small")
            ctx.geom = (b, cs, h, w, kh, kw, m, 0, 0)
            ctx.small = True
            ctx.save_for_backward(dp, index)
            return loss
        ctx.small = False
        # the two matrix products on the split core (include/skd_pairwise_split.h)?  Decided once, here: the backward follows
        ctx.split = bool(split) and pairwise_split_supported() and (cs, ct, m) not in PAIRWISE_SPLIT_ROUTING_EXCLUDED
        ldm = lib.skd_pairwise_ldm(m)
        p_s = feat_s.new_empty((b, cs, m))
        p_t = feat_s.new_empty((b, ct, m))
        index = torch.empty((b, cs, m), dtype=torch.int32, device=feat_s.device) if need else None
        _pool_feature(lib, feat_s, kh, kw, p_s, index, st)
        _pool_feature(lib, feat_t, kh, kw, p_t, None, st)
        fh_s = feat_s.new_empty((b, cs, ldm))
        fh_t = feat_s.new_empty((b, ct, ldm))
        norm_s = feat_s.new_empty((b, m)) if need else None
        _lib.check(lib.skd_channel_l2_normalise(b, cs, m, p_s.data_ptr(), fh_s.data_ptr(), ldm,
                                                None, 0, _lib.ptr(norm_s), st),
                   "skd_channel_l2_normalise")
        _lib.check(lib.skd_channel_l2_normalise(b, ct, m, p_t.data_ptr(), fh_t.data_ptr(), ldm,
                                                None, 0, None, st), "skd_channel_l2_normalise")
        g = feat_s.new_empty((b, ldm, ldm)) if need else None
        loss = feat_s.new_empty(())
        if ctx.split:
            ws = feat_s.new_empty((max(1, lib.skd_pairwise_split_workspace_floats(b, cs, ct, m)),))
            _lib.check(lib.skd_pairwise_split_gram_loss(b, cs, ct, m, ldm, fh_s.data_ptr(), fh_t.data_ptr(),
                                                        _lib.ptr(g), loss.data_ptr(), ws.data_ptr(), st),
                       "skd_pairwise_split_gram_loss")
        else:
            ws = feat_s.new_empty((max(1, lib.skd_pairwise_workspace_floats(b, m)),))
            _lib.check(lib.skd_pairwise_gram_loss(b, cs, ct, m, ldm, fh_s.data_ptr(), fh_t.data_ptr(),
                                                  _lib.ptr(g), loss.data_ptr(), ws.data_ptr(), st),
                       "skd_pairwise_gram_loss")
        ctx.geom = (b, cs, h, w, kh, kw, m, ldm, 0)
        ctx.save_for_backward(fh_s if need else None, g, norm_s, index)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, gl):
        if ctx.small:
            dp, index = ctx.saved_tensors
            if dp is None:
                return None, None, None, None, None
            b, cs, h, w, kh, kw, m, _, _ = ctx.geom
            lib, st = _lib.get(), _lib.stream_of(dp)
            dpg = dp * gl.to(torch.float32)
            return _unpool_feature(lib, ctx.nhwc, (b, cs, h, w, kh, kw), dpg, m, index, st), None, None, None, None
        fh_s, g, norm_s, index = ctx.saved_tensors
        if g is None:
            return None, None, None, None, None
        b, cs, h, w, kh, kw, m, ldm, _ = ctx.geom
        lib, st = _lib.get(), _lib.stream_of(g)
        gl = gl.to(torch.float32).contiguous()
        dp = g.new_empty((b, cs, ldm))
        if ctx.split:
            ws = g.new_empty((max(1, lib.skd_pairwise_split_backward_workspace_floats(b, cs, m)),))
            _lib.check(lib.skd_pairwise_split_backward(b, cs, m, ldm, fh_s.data_ptr(), g.data_ptr(),
                                                       norm_s.data_ptr(), gl.data_ptr(), dp.data_ptr(), ws.data_ptr(), st),
                       "skd_pairwise_split_backward")
        else:
            ws = g.new_empty((max(1, lib.skd_pairwise_backward_workspace_floats(b, cs, m)),))
            _lib.check(lib.skd_pairwise_backward(b, cs, m, ldm, fh_s.data_ptr(), g.data_ptr(),
                                                 norm_s.data_ptr(), gl.data_ptr(), dp.data_ptr(), ws.data_ptr(), st),
                       "skd_pairwise_backward")
        return _unpool_feature(lib, ctx.nhwc, (b, cs, h, w, kh, kw), dp, ldm, index, st), None, None, None, None


# (Cs, Ct, M) of the pair-wise loss that stay on the fp32 kernels whatever `split` says: the measured shapes whose split forward +
# backward are not ahead of the fp32 pair (profiles/r29_pairwise_split_isolated.md has the table and the rule).
PAIRWISE_SPLIT_ROUTING_EXCLUDED = frozenset()

_PAIRWISE_SPLIT_ENTRIES = ("skd_pairwise_split_workspace_floats", "skd_pairwise_split_gram_loss",
                           "skd_pairwise_split_backward_workspace_floats", "skd_pairwise_split_backward")


def pairwise_split_supported():
    """Whether the active back-end has the entries of include/skd_pairwise_split.h (the plain-C double has not: not an error)."""
    return all(_lib.has_entry(n) for n in _PAIRWISE_SPLIT_ENTRIES)


def pair_wise_loss(feat_s, feat_t, kh, kw, split=False):
    """CriterionPairWiseforWholeFeatAfterPool.forward on raw (B,C,H,W) features, criterion.py:236-245.

    ``split=True``: for graphs of more than 64 nodes the Gram + loss and the backward product run on the split bf16-MFMA core
    (include/skd_pairwise_split.h) where the back-end has the entries and (Cs, Ct, M) is not in PAIRWISE_SPLIT_ROUTING_EXCLUDED;
    everything else -- pooling, normalising, the small-graph kernel, the unpool -- is what it is without it."""
    return _PairWise.apply(feat_s, feat_t.detach(), int(kh), int(kw), bool(split))


class _SpectralNormalize(Function):
    """w = w_bar / sigma after ONE power iteration that updates u and v in place (spectral.py:23-35).

    u and v are held by reference, not snapshotted: the reference rebinds ``u.data`` / ``v.data``
    without an autograd version bump, so a graph recorded by an earlier forward is back-propagated
    with whatever u, v hold at backward time (the D step runs three forwards before its single
    backward, kd_model.py:156-164).  Reading them at backward time reproduces that exactly.
    """

    @staticmethod
    def forward(ctx, w_bar, u, v):
        _lib.require_device(w_bar, u, v)
        wb = _f32c(w_bar, "spectral_normalize")
        h = wb.shape[0]
        wd = wb.numel() // h
        if not (u.is_contiguous() and v.is_contiguous()) or u.numel() != h or v.numel() != wd:
            raise ValueError("spectral_normalize: u/v must be contiguous vectors of length (out, in*kh*kw)")
        lib, st = _lib.get(), _lib.stream_of(wb)
        sigma = wb.new_empty(())
        w = torch.empty_like(wb)
        ws = wb.new_empty((max(1, lib.skd_spectral_workspace_floats(h, wd)),))
        _lib.check(lib.skd_spectral_norm_forward(h, wd, wb.data_ptr(), u.data_ptr(), v.data_ptr(),
                                                 sigma.data_ptr(), w.data_ptr(), ws.data_ptr(), st),
                   "skd_spectral_norm_forward")
        ctx.u, ctx.v = u, v
        ctx.save_for_backward(wb, sigma)
        return w

    @staticmethod
    @once_differentiable
    def backward(ctx, gw):
        wb, sigma = ctx.saved_tensors
        h = wb.shape[0]
        wd = wb.numel() // h
        gw = _f32c(gw, "spectral_normalize backward")
        lib, st = _lib.get(), _lib.stream_of(wb)
        gwb = torch.empty_like(wb)
        ws = wb.new_empty((max(1, lib.skd_spectral_workspace_floats(h, wd)),))
        _lib.check(lib.skd_spectral_norm_backward(h, wd, wb.data_ptr(), ctx.u.data_ptr(), ctx.v.data_ptr(),
                                                  sigma.data_ptr(), gw.data_ptr(), gwb.data_ptr(),
                                                  ws.data_ptr(), st), "skd_spectral_norm_backward")
        return gwb, None, None


def spectral_normalize(w_bar, u, v):
    return _SpectralNormalize.apply(w_bar, u, v)


class _SpectralNormalizeMulti(Function):
    """``_SpectralNormalize`` for ALL spectrally normalised layers of a network at once (skd_spectral_norm_*_multi): three
    launches forward and two backward for the whole set instead of per layer.  ``us`` / ``vs``: lists of the layers' u / v
    tensors (held by reference and read again at backward time, like the single-layer op); returns one normalised weight per
    layer."""

    @staticmethod
    def forward(ctx, us, vs, *w_bars):
        _lib.require_device(*w_bars, *us, *vs)
        wbs = [_f32c(w, "spectral_normalize_multi") for w in w_bars]
        hs = [w.shape[0] for w in wbs]
        ws_ = [w.numel() // h for w, h in zip(wbs, hs)]
        for u, v, h, wd in zip(us, vs, hs, ws_):
            if not (u.is_contiguous() and v.is_contiguous()) or u.numel() != h or v.numel() != wd:
                raise ValueError("spectral_normalize: u/v must be contiguous vectors of length (out, in*kh*kw)")
        lib, st = _lib.get(), _lib.stream_of(wbs[0])
        sigmas = wbs[0].new_empty((len(wbs),))
        outs = [torch.empty_like(w) for w in wbs]
        work = wbs[0].new_empty((sum(max(1, lib.skd_spectral_workspace_floats(h, wd)) for h, wd in zip(hs, ws_)),))
        sig = [sigmas[k:k + 1] for k in range(len(wbs))]
        _lib.check(lib.skd_spectral_norm_forward_multi(len(wbs), _lib.int_array(hs), _lib.int_array(ws_), _lib.ptr_array(wbs),
                                                       _lib.ptr_array(us), _lib.ptr_array(vs), _lib.ptr_array(sig),
                                                       _lib.ptr_array(outs), work.data_ptr(), st), "skd_spectral_norm_forward_multi")
        ctx.us, ctx.vs, ctx.hs, ctx.ws_ = list(us), list(vs), hs, ws_
        ctx.save_for_backward(sigmas, *wbs)
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *gws):
        sigmas, *wbs = ctx.saved_tensors
        lib, st = _lib.get(), _lib.stream_of(wbs[0])
        gws = [torch.zeros_like(w) if g is None else _f32c(g, "spectral_normalize backward") for g, w in zip(gws, wbs)]
        gwbs = [torch.empty_like(w) for w in wbs]
        work = wbs[0].new_empty((sum(max(1, lib.skd_spectral_workspace_floats(h, wd)) for h, wd in zip(ctx.hs, ctx.ws_)),))
        sig = [sigmas[k:k + 1] for k in range(len(wbs))]
        _lib.check(lib.skd_spectral_norm_backward_multi(len(wbs), _lib.int_array(ctx.hs), _lib.int_array(ctx.ws_), _lib.ptr_array(wbs),
                                                        _lib.ptr_array(ctx.us), _lib.ptr_array(ctx.vs), _lib.ptr_array(sig),
                                                        _lib.ptr_array(gws), _lib.ptr_array(gwbs), work.data_ptr(), st),
                   "skd_spectral_norm_backward_multi")
        return (None, None) + tuple(gwbs)


def spectral_normalize_multi(w_bars, us, vs):
    """[w_bar_k / sigma_k] after one power iteration per layer (u_k, v_k updated in place): all layers in 3 launches."""
    return _SpectralNormalizeMulti.apply(list(us), list(vs), *w_bars)


def spectral_power_iteration(w_bar, u, v):
    """u, v update only (extra iterations when power_iterations > 1); returns sigma (0-dim)."""
    _lib.require_device(w_bar, u, v)
    wb = _f32c(w_bar.detach(), "spectral_power_iteration")
    h = wb.shape[0]
    wd = wb.numel() // h
    lib, st = _lib.get(), _lib.stream_of(wb)
    sigma = wb.new_empty(())
    ws = wb.new_empty((max(1, lib.skd_spectral_workspace_floats(h, wd)),))
    _lib.check(lib.skd_spectral_norm_forward(h, wd, wb.data_ptr(), u.data_ptr(), v.data_ptr(),
                                             sigma.data_ptr(), None, ws.data_ptr(), st),
               "skd_spectral_norm_forward")
    return sigma
