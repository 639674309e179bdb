"""Evaluation (mIoU) and prediction dump on MI355X -- the ``evaluate_main`` that ``train_and_eval.py:28`` reaches through
``NetModel.evalute_model`` and that the reference's ``test.py`` calls with ``type='test'``.

Reference: networks/evaluate.py:156-206.  ``whole=True`` (what train_and_eval.py uses): per validation image, student
forward on the full 1024x2048 image, bilinear (align_corners) upsample of the 129x257 logits back to 1024x2048, argmax,
confusion matrix over the non-ignored pixels, IoU = tp / max(1, pos + res - tp), mean over classes.  The reference
materialises the up-sampled logits (159 MB), copies them to the host and runs numpy argmax/bincount; here the upsample +
argmax + confusion accumulation is one HIP kernel (csrc/evaluate.hip) and only the 19x19 int64 matrix ever leaves the GPU.

``whole=False`` (the reference's default, evaluate.py:70-104): the image is cut into overlapping tiles of ``input_size``
(``sliding_tiles``), the tiles are forwarded as one batch (``tile_batch`` caps it), and one HIP kernel
(csrc/evaluate_sliding.hip) does what the reference does tile after tile in numpy -- upsample each tile's logits, add
them into float64 H x W x C sums and cover counts, divide, argmax -- as a gather: a lane per image pixel sums, in tile
order, over the tiles that cover it, so the float64 sums carry the reference's bits and no H x W x C array exists.
``predict_sliding`` returns the reference's (H, W, classes) float64 probabilities for callers that want them.

``type='test'`` (evaluate.py:187-191): batches are (image, size, name); the prediction is remapped trainId -> id on the
device and written as a palette PNG ``<outputs>/<name>.png``; nothing is scored and None is returned.  ``outputs=`` also
dumps the (un-remapped) predictions of a validation run; without it a validation run writes no file.

Multi-scale / flip evaluation (evaluate.py:115-134, ``predict_multiscale`` with more than ``[1.0], False`` -- the mode of
reported Cityscapes numbers and test-server submissions): ``evaluate_main(whole=True, scales=[...], flip=True)``.  Per scale
one kernel resizes the image exactly as ``scipy.ndimage.zoom(order=1, prefilter=False)`` does (float64 coordinates, output
size by Python ``round``, the zeroed last row / column of some sizes included) and writes the X-mirrored copy next to it; the
two are forwarded as one batch of 2 and the logits stay on the device.  One gather kernel (csrc/evaluate_multiscale.hip)
then does per pixel what the reference does per scale on the host with H x W x C arrays: upsample, fp32 flip average,
float64 sum in scale order, mean, argmax, remap, confusion.  ``predict_multiscale`` / ``predict_whole`` return the
reference's arrays for callers that want them.  ``scales`` None or ``[1.0]`` without ``flip`` is the whole-image path above,
unchanged.

The student's fused inference form (``networks.fuse_for_inference(model)``, or ``default_args(fused_eval=True)`` for NetModel's
student): ``evaluate_main``, ``predict_whole``, ``predict_sliding`` and ``predict_multiscale`` take the model as it is given --
flagged or not -- and need no argument for it; a flagged model's eval-mode forwards run its BasicBlocks on the split-core 3x3
convolution (networks/pspnet_combine.py), everything behind the forward is the same code.  With ``split_narrow`` /
``SKD_SPLIT_NARROW=1`` the 64-channel convolutions join them, and with ``split_stride2`` / ``SKD_SPLIT_STRIDE2=1`` layer2.0's
stride-2 ``conv1`` does (``fuse_for_inference(model, stride2=True)``, include/skd_stride2.h).

Not provided: the cv2-based dataset readers; ``recurrence`` and flipping in sliding mode are accepted and ignored, as in the
reference.  A back-end without ``skd_seg_sliding`` / ``skd_zoom_linear`` / ``skd_seg_multiscale`` (the plain-C double of
oracle/) cannot run the sliding / multi-scale modes: NotImplementedError names the entry point.
"""
import os
from math import ceil

import numpy as np
import torch

from .. import _lib
from .. import functional as SF

ignore_label = 255
# Cityscapes label id -> train id (the public labels.py table the reference carries at evaluate.py:23-28)
id_to_trainid = {-1: ignore_label, 0: ignore_label, 1: ignore_label, 2: ignore_label, 3: ignore_label, 4: ignore_label,
                 5: ignore_label, 6: ignore_label, 7: 0, 8: 1, 9: ignore_label, 10: ignore_label, 11: 2, 12: 3, 13: 4,
                 14: ignore_label, 15: ignore_label, 16: ignore_label, 17: 5, 18: ignore_label, 19: 6, 20: 7, 21: 8, 22: 9,
                 23: 10, 24: 11, 25: 12, 26: 13, 27: 14, 28: 15, 29: ignore_label, 30: ignore_label, 31: 16, 32: 17, 33: 18}


def id2trainId(label, id_to_trainid=id_to_trainid, reverse=False):
    """evaluate.py:30-38 as a table look-up: every element equal to a key becomes that key's value (``reverse``: keys and
    values swapped; where several ids share one train id the table's last entry wins, like the reference's loop).  Values
    the table does not name are kept.  An entry whose source value does not occur in ``label`` is not applied, so a uint8
    prediction map goes through ``reverse=True`` although the table holds -1 (the reference's loop raises there under
    numpy 2); an entry that does occur and does not fit the dtype raises as numpy does."""
    label = np.asarray(label)
    out = label.copy()
    table = {}
    for k, v in id_to_trainid.items():
        src, dst = (v, k) if reverse else (k, v)
        table[src] = dst
    info = np.iinfo(label.dtype) if np.issubdtype(label.dtype, np.integer) else None
    for src, dst in table.items():
        if info is not None and not info.min <= src <= info.max:
            continue                                   # cannot occur in an array of this dtype
        hit = label == src
        if hit.any():
            out[hit] = dst
    return out


def trainid_to_id_table(table=id_to_trainid):
    """256-entry uint8 look-up: train id -> label id (``id2trainId(..., reverse=True)`` on 0 .. 255) for the device remap."""
    return id2trainId(np.arange(256, dtype=np.int64), table, reverse=True).astype(np.uint8)


def get_palette(num_cls):
    """evaluate.py:40-61: the PASCAL VOC colour map (bit k of the label goes to bit 7 - k // 3 of channel k % 3) as a
    flat [r0, g0, b0, r1, ...] list."""
    lab = np.arange(int(num_cls), dtype=np.int64)
    pal = np.zeros((int(num_cls), 3), dtype=np.int64)
    k = 0
    while (lab >> k).any():
        pal[:, k % 3] |= ((lab >> k) & 1) << (7 - k // 3)
        k += 1
    return [int(v) for v in pal.reshape(-1)]


def pad_image(img, target_size):
    """evaluate.py:63-68: zero-pad (N, C, h, w) at the bottom / right up to ``target_size``."""
    rows, cols = max(int(target_size[0]) - img.shape[2], 0), max(int(target_size[1]) - img.shape[3], 0)
    if torch.is_tensor(img):
        return torch.nn.functional.pad(img, (0, cols, 0, rows))
    return np.pad(img, ((0, 0), (0, 0), (0, rows), (0, cols)), "constant")


def sliding_tiles(H, W, tile_size):
    """The tile windows of evaluate.py:73-90 as a list of (y1, x1, y2, x2), row-major.  The stride comes from the tile
    HEIGHT for both axes; a window that would overhang is moved back inside (so an origin can occur twice, and is then
    counted twice); an image smaller than the tile gives one window per axis, to be zero-padded (also where the reference's
    formula gives none and divides 0 by 0: an image a whole stride smaller than the tile)."""
    th, tw = int(tile_size[0]), int(tile_size[1])
    H, W = int(H), int(W)
    if min(th, tw, H, W) <= 0:
        raise ValueError("sliding_tiles: positive sizes expected")
    stride = ceil(th * (1 - 1 / 3))
    rows = max(int(ceil((H - th) / stride) + 1), 1)
    cols = max(int(ceil((W - tw) / stride) + 1), 1)
    tiles = []
    for row in range(rows):
        for col in range(cols):
            x2, y2 = min(col * stride + tw, W), min(row * stride + th, H)
            tiles.append((max(y2 - th, 0), max(x2 - tw, 0), y2, x2))
    return tiles


def get_confusion_matrix(gt_label, pred_label, class_num):
    """evaluate.py:136-154 on host arrays (kept for API parity; evaluate_main uses the fused kernels)."""
    index = (np.asarray(gt_label).astype(np.int64) * class_num + np.asarray(pred_label).astype(np.int64))
    count = np.bincount(index.ravel(), minlength=class_num * class_num)[: class_num * class_num]
    return count.reshape(class_num, class_num).astype(np.float64)


def iou_from_confusion(confusion_matrix):
    """evaluate.py:200-206."""
    cm = np.asarray(confusion_matrix, dtype=np.float64)
    pos, res, tp = cm.sum(1), cm.sum(0), np.diag(cm)
    iu = tp / np.maximum(1.0, pos + res - tp)
    return float(iu.mean()), iu


def _require_sliding_backend(what):
    if not _lib.has_entry("skd_seg_sliding"):
        raise NotImplementedError("%s needs the entry point skd_seg_sliding (include/skd_eval.h, csrc/evaluate_sliding.hip), "
                                  "which the active back-end does not provide" % what)


def _parse_size(input_size):
    h, w = (input_size.split(",") if isinstance(input_size, str) else input_size)
    return int(h), int(w)


def _channels_last_model(model, device):
    """A network whose weights NetModel keeps channels-last (kd_model.py of this package) is fed channels-last images, so
    the forward stays on the NHWC ABN / pyramid / fold kernels."""
    w4 = [p for p in model.parameters() if p.dim() == 4 and p.shape[1] > 1 and p.shape[2] * p.shape[3] > 1]
    return device.type == "cuda" and bool(w4) and all(p.is_contiguous(memory_format=torch.channels_last) and not p.is_contiguous() for p in w4)


def _tile_logits(model, image, tiles, tile_size, cl_model, tile_batch):
    """Gather the (zero-padded) tiles of ``image`` (1, 3, H, W) into one batch and forward it: (T, C, h, w) fp32 logits."""
    th, tw = tile_size
    batch = image.new_zeros((len(tiles), image.shape[1], th, tw))
    for i, (y1, x1, y2, x2) in enumerate(tiles):
        batch[i, :, :y2 - y1, :x2 - x1] = image[0, :, y1:y2, x1:x2]
    if cl_model:
        batch = batch.contiguous(memory_format=torch.channels_last)
    step = len(tiles) if tile_batch is None else int(tile_batch)
    outs = []
    for s in range(0, len(tiles), step):
        out = model(batch[s:s + step])
        if isinstance(out, (list, tuple)):
            out = out[0]
        outs.append(out.float())
    return outs[0] if len(outs) == 1 else torch.cat(outs)


def _as_image(image, device):
    image = torch.as_tensor(np.asarray(image) if not torch.is_tensor(image) else image).float().to(device)
    if image.dim() != 4 or image.shape[0] != 1:
        raise ValueError("sliding-window evaluation takes one image (1, 3, H, W) per batch (got %s)" % (tuple(image.shape),))
    return image


def predict_sliding(net, image, tile_size, classes, flip_evaluation=False, recurrence=1, tile_batch=None):
    """evaluate.py:70-104: the (H, W, classes) float64 mean of the up-sampled tile logits as a numpy array.  ``image``:
    numpy or tensor (1, 3, H, W).  ``flip_evaluation`` and ``recurrence`` are accepted and ignored, as in the reference."""
    _require_sliding_backend("predict_sliding")
    try:
        device = next(net.parameters()).device
    except StopIteration:
        device = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    tile_size = _parse_size(tile_size)
    image = _as_image(image, device)
    tiles = sliding_tiles(image.shape[2], image.shape[3], tile_size)
    with torch.no_grad():
        logits = _tile_logits(net, image, tiles, tile_size, _channels_last_model(net, device), tile_batch)
        if logits.shape[1] != classes:
            raise ValueError("predict_sliding: the network returns %d classes, not %d" % (logits.shape[1], classes))
        _, probs, _ = SF.seg_sliding(logits, tiles, tile_size, image.shape[2:], want_pred=False, want_probs=True)
    return probs.cpu().numpy()


def _require_multiscale_backend(what):
    for entry in ("skd_zoom_linear", "skd_seg_multiscale"):
        if not _lib.has_entry(entry):
            raise NotImplementedError("%s needs the entry point %s (include/skd_eval_ms.h, csrc/evaluate_multiscale.hip), "
                                      "which the active back-end does not provide" % (what, entry))


def _model_device(net):
    try:
        return next(net.parameters()).device
    except StopIteration:
        return torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")


def _forward_logits(model, batch):
    out = model(batch)
    if isinstance(out, (list, tuple)):
        out = out[0]
    return out.float()


def _scale_logits(model, image, scales, flip, cl_model):
    """Per scale: resize ``image`` (1, C, H, W) on the device (with its X-mirrored copy when flipping) and forward the batch of
    F = 1 + flip once.  Returns the list of (F, classes, h_s, w_s) logits, kept on the device."""
    out = []
    for scale in scales:
        batch = SF.zoom_linear(image, float(scale), mirror=flip, channels_last=cl_model)
        out.append(_forward_logits(model, batch))
    return out


def predict_whole(net, image, tile_size, recurrence=1):
    """evaluate.py:106-113: the network's logits on ``image`` (1, 3, h, w), up-sampled (bilinear, align_corners) to
    ``tile_size`` = (th, tw): a (th, tw, classes) float32 numpy array.  ``recurrence`` is accepted and ignored."""
    _require_multiscale_backend("predict_whole")
    device = _model_device(net)
    th, tw = _parse_size(tile_size)
    image = torch.as_tensor(np.asarray(image) if not torch.is_tensor(image) else image).float().to(device)
    if image.dim() != 4 or image.shape[0] != 1:
        raise ValueError("predict_whole takes one image (1, 3, h, w) (got %s)" % (tuple(image.shape),))
    with torch.no_grad():
        if _channels_last_model(net, device):
            image = image.contiguous(memory_format=torch.channels_last)
        logits = _forward_logits(net, image)
        # one scale, no flip: sum = (double)v and v / 1.0 is exact, so the cast back to float32 loses nothing
        _, probs, _ = SF.seg_multiscale([logits], (th, tw), want_pred=False, want_probs=True)
    return probs.float().cpu().numpy()


def predict_multiscale(net, image, tile_size, scales, classes, flip_evaluation, recurrence=1):
    """evaluate.py:115-134: the (H, W, classes) float64 mean over ``scales`` of the up-sampled (and, with ``flip_evaluation``,
    flip-averaged) logits as a numpy array.  ``image``: numpy or tensor (1, 3, H, W); ``tile_size`` must be its (H, W) -- the
    reference's ``full_probs += scaled_probs`` only broadcasts then.  ``recurrence`` is accepted and ignored."""
    _require_multiscale_backend("predict_multiscale")
    device = _model_device(net)
    image = _as_image(image, device)
    H, W = int(image.shape[2]), int(image.shape[3])
    if _parse_size(tile_size) != (H, W):
        raise ValueError("predict_multiscale: tile_size %s must equal the image's size %s" % (tuple(_parse_size(tile_size)), (H, W)))
    scales = [float(v) for v in scales]
    if not scales:
        raise ValueError("predict_multiscale: at least one scale expected")
    with torch.no_grad():
        logits = _scale_logits(net, image, scales, bool(flip_evaluation), _channels_last_model(net, device))
        if logits[0].shape[1] != classes:
            raise ValueError("predict_multiscale: the network returns %d classes, not %d" % (logits[0].shape[1], classes))
        _, probs, _ = SF.seg_multiscale(logits, (H, W), want_pred=False, want_probs=True)
    return probs.cpu().numpy()


def _save_png(pred, directory, name, palette):
    """evaluate.py:189-191: mode-P PNG with the 256-colour palette."""
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("evaluate_main(outputs=%r) writes palette PNGs and needs PIL (Pillow)" % directory) from e
    im = Image.fromarray(pred)
    im.putpalette(palette)
    path = os.path.join(directory, "%s.png" % name)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    im.save(path)


def evaluate_main(model, loader, gpu_id, input_size, num_classes, whole=False, recurrence=1, type="val", rank=0, world=1,
                  group=None, outputs=None, tile_batch=None, scales=None, flip=False):
    """``type='val'``: returns (mean_IU, IU_array) like evaluate.py:156-206.  ``loader`` yields (image (1,3,H,W) float,
    label (1,H,W), size, name) like CSDataSet (dataset/datasets.py:121-210); ``size[0][:2]`` is the valid (h, w) of the label.
    ``type='test'``: ``loader`` yields (image, size, name); the predictions are remapped trainId -> id and written as
    palette PNGs ``<outputs>/<name[0]>.png`` (``outputs`` defaults to the reference's ``'outputs'``); returns None.
    ``whole=False``: sliding-window inference with tiles of ``input_size`` ('h,w'), all tiles of an image in one forward
    unless ``tile_batch`` caps the batch.  ``outputs`` with ``type='val'`` also dumps the (un-remapped) predictions.
    ``scales`` / ``flip`` (``whole=True`` only): multi-scale / flip evaluation, evaluate.py:115-134 -- the prediction is the
    argmax of the mean over ``scales`` of the (flip-averaged) up-sampled logits; the output size is the label's (the image's
    for ``type='test'``) and must equal the image's.  ``scales`` None or [1.0] without ``flip`` is plain whole-image scoring.
    ``rank`` / ``world`` (one process per GPU): every rank walks the same loader but evaluates only the batches with
    ``index % world == rank``; the integer confusion matrices are summed over ``group`` with one all-reduce, so every
    rank returns the identical result of the whole validation set (the reference's single process evaluated alone)."""
    if type not in ("val", "test"):
        raise ValueError("evaluate_main: type is 'val' or 'test' (got %r)" % (type,))
    tile_size = None
    multiscale = None
    if flip or (scales is not None and [float(v) for v in scales] != [1.0]):
        if not whole:
            raise ValueError("evaluate_main: scales / flip need whole=True (sliding-window evaluation ignores them in the reference)")
        multiscale = ([float(v) for v in scales] if scales is not None else [1.0], bool(flip))
        if not multiscale[0]:
            raise ValueError("evaluate_main: scales is None or a non-empty list (got %r)" % (scales,))
        _require_multiscale_backend("evaluate_main(scales=..., flip=...)")
    if not whole:
        _require_sliding_backend("evaluate_main(whole=False)")
        tile_size = _parse_size(input_size)
        if tile_batch is not None and int(tile_batch) < 1:
            raise ValueError("evaluate_main: tile_batch is None or a positive int (got %r)" % (tile_batch,))
    if type == "test" and outputs is None:
        outputs = "outputs"                              # evaluate.py:172-173,191
    if world > 1:
        # Sharding by ``index % world`` assumes every rank walks the SAME sequence of batches.  A loader that already shards
        # (DistributedSampler) or shuffles would have each rank skip most of its own subset and score a silently smaller set
        # (ADVICE r03): refuse it.
        sampler = getattr(loader, "sampler", None)
        from torch.utils.data import RandomSampler
        from torch.utils.data.distributed import DistributedSampler
        if isinstance(sampler, (DistributedSampler, RandomSampler)) or isinstance(getattr(loader, "batch_sampler", None), DistributedSampler):
            raise ValueError("evaluate_main shards the validation set itself (batch i on rank i %% world): hand it a plain, "
                             "unshuffled, unsharded loader (got sampler %s)" % sampler.__class__.__name__)   # (`type` is an argument here)
    device = torch.device("cuda", int(gpu_id) if str(gpu_id).isdigit() else 0) if torch.cuda.is_available() \
        else next(model.parameters()).device
    was_training = model.training
    model.eval()
    model.to(device)
    confusion = torch.zeros((num_classes, num_classes), dtype=torch.int64, device=device)
    cl_model = _channels_last_model(model, device)
    dump = None
    if outputs is not None:
        os.makedirs(outputs, exist_ok=True)
        dump = {"dir": outputs, "palette": get_palette(256),
                "remap": torch.from_numpy(trainid_to_id_table()).to(device) if type == "test" else None}
    seen, failure = 0, None
    with torch.no_grad():
        for index, batch in enumerate(loader):
            if index % world != rank:
                continue
            if failure is not None:
                continue
            seen += 1
            try:
                _score_batch(model, batch, device, num_classes, cl_model, confusion, type, tile_size, tile_batch, dump, multiscale)
            except Exception as e:                    # reported AFTER the collective below, so that no rank is left hanging in it
                if world <= 1:
                    raise
                failure = e
    if was_training:
        model.train()
    if world > 1:
        # one exchange: the confusion counts (exact, int64), how many batches were scored, and whether any rank failed
        extra = torch.tensor([seen, 1 if failure is not None else 0], dtype=torch.int64, device=device)
        flat = torch.cat([confusion.reshape(-1), extra])
        torch.distributed.all_reduce(flat, group=group)
        confusion = flat[:-2].reshape(num_classes, num_classes)
        total, failed = int(flat[-2]), int(flat[-1])
        if failure is not None:
            raise failure
        if failed:
            raise RuntimeError("evaluate_main: %d other rank(s) failed while scoring their share of the validation set" % failed)
        try:
            expected = len(loader)
        except TypeError:
            expected = None
        if expected is not None and total != expected:
            raise RuntimeError("evaluate_main: the ranks scored %d batches together but the loader holds %d" % (total, expected))
    if type == "test":
        return None
    return iou_from_confusion(confusion.cpu().numpy())


def _score_batch(model, batch, device, num_classes, cl_model, confusion, split="val", tile_size=None, tile_batch=None, dump=None,
                 multiscale=None):
    """One batch.  Whole image (``tile_size`` None): forward, fused upsample + argmax + confusion accumulation
    (csrc/evaluate.hip).  Sliding: batched tile forward, fused gather over the tiles (csrc/evaluate_sliding.hip).
    ``multiscale`` = (scales, flip): device resize and one forward per scale, fused gather over the scales
    (csrc/evaluate_multiscale.hip).  With
    ``dump`` the uint8 prediction (remapped on the device for the test split) is copied to the host and written as a PNG."""
    if split == "val":
        image, label, size = batch[0], batch[1], batch[2]
        name = batch[3] if len(batch) > 3 else None
    else:
        image, label, size, name = batch[0], None, batch[1], batch[2]
    full = None
    if label is not None:
        lab_np = np.asarray(label) if not torch.is_tensor(label) else label.numpy() if label.device.type == "cpu" else None
        if lab_np is not None and bool(((lab_np != ignore_label) & ((lab_np < 0) | (lab_np >= num_classes))).any()):
            # np.bincount of evaluate.py:188-198 would count such labels (and index out of the matrix); the fused
            # kernel skips them -- refuse instead of scoring a quietly smaller set (raw label ids not mapped to trainIds?)
            raise ValueError("label values outside [0, %d) other than ignore_label %d" % (num_classes, ignore_label))
        label = torch.as_tensor(np.asarray(label) if not torch.is_tensor(label) else label).long().to(device)
        sz = np.asarray(size[0] if (torch.is_tensor(size) or isinstance(size, (list, tuple))) else size).reshape(-1)
        hh, ww = int(sz[0]), int(sz[1])
        # only [:h, :w] of the label is scored (evaluate.py:194)
        full = label.new_full(label.shape, ignore_label)
        full[:, :hh, :ww] = label[:, :hh, :ww]
    remap = dump["remap"] if dump is not None else None
    if multiscale is not None:
        image = _as_image(image, device)
        H, W = int(image.shape[2]), int(image.shape[3])
        if full is not None and tuple(full.shape[-2:]) != (H, W):
            raise ValueError("label %s and image %s differ in size" % (tuple(full.shape), tuple(image.shape)))
        logits = _scale_logits(model, image, multiscale[0], multiscale[1], cl_model)
        if logits[0].shape[1] != num_classes:
            raise ValueError("the network returns %d classes, evaluate_main was told %d" % (logits[0].shape[1], num_classes))
        pred, _, _ = SF.seg_multiscale(logits, (H, W), full, ignore_label, confusion if full is not None else None, remap=remap,
                                       want_pred=dump is not None)
    elif tile_size is None:
        image = torch.as_tensor(np.asarray(image) if not torch.is_tensor(image) else image).float().to(device)
        if cl_model and image.dim() == 4:
            image = image.contiguous(memory_format=torch.channels_last)   # keep the network on its channels-last kernels
        logits = model(image)
        if isinstance(logits, (list, tuple)):
            logits = logits[0]
        # predict_whole upsamples to the tile size (1024, 2048) = the label's size; the test split has no label: the image's
        want = dump is not None if full is not None else tuple(image.shape[2:])
        pred, _ = SF.seg_confusion(logits.float(), full, ignore_label, confusion if full is not None else None, want_pred=want)
        if dump is not None and remap is not None:
            pred = remap[pred.long()]                    # 256-entry index on the device (evaluate.py:188)
    else:
        image = _as_image(image, device)
        H, W = int(image.shape[2]), int(image.shape[3])
        if full is not None and tuple(full.shape[-2:]) != (H, W):
            raise ValueError("label %s and image %s differ in size" % (tuple(full.shape), tuple(image.shape)))
        tiles = sliding_tiles(H, W, tile_size)
        logits = _tile_logits(model, image, tiles, tile_size, cl_model, tile_batch)
        if logits.shape[1] != num_classes:
            raise ValueError("the network returns %d classes, evaluate_main was told %d" % (logits.shape[1], num_classes))
        pred, _, _ = SF.seg_sliding(logits, tiles, tile_size, (H, W), full, ignore_label, confusion if full is not None else None,
                                    remap=remap, want_pred=dump is not None)
    if dump is not None:
        if name is None:
            raise ValueError("evaluate_main(outputs=...) needs batches that carry the image name")
        pred = pred.reshape(pred.shape[-2], pred.shape[-1]).cpu().numpy()
        _save_png(pred, dump["dir"], name[0] if isinstance(name, (list, tuple)) else name, dump["palette"])
