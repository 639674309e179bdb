"""The distillation criteria of the reference's utils/criterion.py, same class names, constructor
arguments and list-indexing convention (``preds[0]`` logits, ``preds[1]`` DSN logits, ``preds[-5]``
post-PSP feature), each returning a 0-dim tensor that participates in autograd.

    OhemCrossEntropy2d                        :11-90     fused HIP kernels (csrc/ce_ohem.hip): threshold + mined CE on the device
    CriterionDSN                              :168-188   fused HIP kernels (csrc/ce_dsn.hip): upsample + CE, main + 0.4*aux
    CriterionOhemDSN                          :190-209   fused HIP kernels (csrc/ce_ohem.hip): OHEM main head + 0.4*plain aux
    CriterionPixelWise                        :211-226   fused HIP kernel (csrc/pixelwise.hip)
    CriterionPairWiseforWholeFeatAfterPool    :228-245   fused HIP kernels (csrc/pairwise.hip)
    CriterionAdvForG / CriterionAdv           :122-166   wgan-gp / hinge on D's (B,1,1,1) output
    CriterionAdditionalGP                     :92-120    WGAN-GP gradient penalty (double backward in D)
The reference's kd_model.py imports CriterionOhemDSN and never constructs it (:18, :79); here NetModel builds it when
``args.ohem`` is set.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib, functional as SF
from .utils import sim_dis_compute


class OhemCrossEntropy2d(nn.Module):
    """Online hard-example mining cross-entropy on full-resolution logits (criterion.py:11-90): the mean of -log p over the
    valid pixels whose label probability is <= the threshold of ``find_threshold``.  The reference finds that threshold on
    the host (softmax copied out, scipy zoom, np.partition, a new target copied back); here it never leaves the device and
    ``forward`` does not synchronise.  Nothing is printed (the reference's ``print('Labels: ...')`` is logging): the last
    call's threshold and kept count stay on the module as 0-dim device tensors, ``last_threshold`` / ``last_kept``."""

    def __init__(self, ignore_label=255, thresh=0.7, min_kept=100000, factor=8):
        super().__init__()
        self.ignore_label = ignore_label
        self.thresh = float(thresh)
        self.min_kept = int(min_kept)
        self.factor = factor
        self.last_threshold = None
        self.last_kept = None

    def find_threshold(self, predict, target):
        """API parity with criterion.py:20-48.  ``predict`` (B, C, h, w), tensor or numpy array, holds either the softmax
        PROBABILITIES, as the reference's callers pass them, or LOGITS (up-sampled to the target's size when smaller);
        ``target`` (B, H, W).  Probabilities are recognised by what they are -- no negative element and every pixel's
        channels summing to 1 within 1e-3 -- and handed to the kernels as their logarithms, whose softmax they are.
        Returns a Python float, so this call (unlike ``forward``) waits for the device."""
        lg, tg = torch.as_tensor(predict, dtype=torch.float32), torch.as_tensor(target).long()
        if not lg.is_cuda and not _lib.test_backend_active():      # arrays, as the reference passes them: onto the device
            lg = lg.to(tg.device if tg.is_cuda else "cuda")
        tg = tg.to(lg.device)
        if lg.dim() == 4 and bool((lg >= 0).all()) and bool(((lg.sum(1) - 1.0).abs() <= 1e-3).all()):
            lg = lg.clamp_min(1e-30).log()                         # (a zero probability: exp(-69), not 0 * -inf in the interpolation)
        threshold, _ = SF.ohem_threshold(lg, tg, self.ignore_label, self.thresh, self.min_kept, self.factor)
        return float(threshold)

    def forward(self, predict, target, weight=None):
        """predict (n, c, h, w) logits, target (n, h, w); ``weight`` must be None (the reference ignores it)."""
        assert not target.requires_grad
        if weight is not None:
            raise NotImplementedError("OhemCrossEntropy2d: class weights are not supported (the reference ignores them)")
        loss, self.last_threshold, self.last_kept = SF.ce_ohem_dsn(predict, None, target, self.ignore_label, self.thresh,
                                                                   self.min_kept, self.factor, 0.0)
        return loss


class CriterionOhemDSN(nn.Module):
    """CriterionDSN with OHEM on the main head (criterion.py:190-209): OhemCrossEntropy2d(up(preds[0])) + 0.4 *
    CE(up(preds[1])), both up-samplings, the threshold search and both losses fused on the device (csrc/ce_ohem.hip).
    There is no ``criterion2`` attribute: the reference's second ``CrossEntropyLoss`` is part of the fused call, not a module
    of its own.  ``use_weight`` is accepted and unused, as in the reference."""

    def __init__(self, ignore_index=255, thresh=0.7, min_kept=100000, use_weight=True, reduce=True):
        super().__init__()
        if not reduce:
            raise NotImplementedError("CriterionOhemDSN(reduce=False): the fused criterion has no per-pixel output (the "
                                      "reference's criterion2 would return a loss map there)")
        self.ignore_index = ignore_index
        self.criterion1 = OhemCrossEntropy2d(ignore_index, thresh, min_kept)

    def forward(self, preds, target):
        c1 = self.criterion1
        loss, c1.last_threshold, c1.last_kept = SF.ce_ohem_dsn(preds[0], preds[1], target, self.ignore_index, c1.thresh,
                                                               c1.min_kept, c1.factor, 0.4)
        return loss


class CriterionDSN(nn.Module):
    def __init__(self, ignore_index=255, use_weight=True, reduce=True):
        super().__init__()
        self.ignore_index = ignore_index
        self.reduction = "mean" if reduce else "none"
        if not reduce:
            print("disabled the reduce.")

    def forward(self, preds, target):
        if self.reduction == "mean" and preds[0].shape[1] <= 64 and preds[0].dtype == torch.float32:
            # fused upsample + CE for both heads (csrc/ce_dsn.hip): nothing of size (B, C, H, W) is written
            return SF.cross_entropy_dsn(preds[0], preds[1], target, self.ignore_index, 0.4)
        h, w = target.size(1), target.size(2)     # reduce=False / very wide class counts: stock ops
        up = F.interpolate(preds[0], size=(h, w), mode="bilinear", align_corners=True)
        loss1 = F.cross_entropy(up, target, ignore_index=self.ignore_index, reduction=self.reduction)
        up = F.interpolate(preds[1], size=(h, w), mode="bilinear", align_corners=True)
        loss2 = F.cross_entropy(up, target, ignore_index=self.ignore_index, reduction=self.reduction)
        return loss1 + loss2 * 0.4


class CriterionPixelWise(nn.Module):
    def __init__(self, ignore_index=255, use_weight=True, reduce=True):
        super().__init__()
        self.ignore_index = ignore_index
        if not reduce:
            print("disabled the reduce.")

    def forward(self, preds_S, preds_T):
        assert preds_S[0].shape == preds_T[0].shape, "the output dim of teacher and student differ"
        return SF.pixel_wise_loss(preds_S[0], preds_T[0])


class CriterionPairWiseforWholeFeatAfterPool(nn.Module):
    def __init__(self, scale, feat_ind, split=False):
        """inter pair-wise loss from inter feature maps

        ``split`` (keyword, not in the reference's signature): the two matrix products of graphs with more than 64 nodes on the
        split bf16-MFMA core (functional.pair_wise_loss)."""
        super().__init__()
        self.criterion = sim_dis_compute
        self.feat_ind = feat_ind
        self.scale = scale
        self.split = bool(split)

    def forward(self, preds_S, preds_T):
        feat_S = preds_S[self.feat_ind]
        feat_T = preds_T[self.feat_ind]
        total_w, total_h = feat_T.shape[2], feat_T.shape[3]
        patch_w, patch_h = int(total_w * self.scale), int(total_h * self.scale)
        return SF.pair_wise_loss(feat_S.float(), feat_T.float(), patch_w, patch_h, split=self.split)


def _check_adv_type(adv_type):
    if adv_type != "wgan-gp" and adv_type != "hinge":
        raise ValueError("adv_type should be wgan-gp or hinge")


class CriterionAdvForG(nn.Module):
    def __init__(self, adv_type):
        super().__init__()
        _check_adv_type(adv_type)
        self.adv_loss = adv_type

    def forward(self, d_out_S, d_out_S_no_use=None):
        return -d_out_S[0].mean()          # identical for wgan-gp and hinge (criterion.py:131-134)


class CriterionAdv(nn.Module):
    def __init__(self, adv_type):
        super().__init__()
        _check_adv_type(adv_type)
        self.adv_loss = adv_type

    def forward(self, d_out_S, d_out_T):
        assert d_out_S[0].shape == d_out_T[0].shape, "the output dim of D with teacher and student as input differ"
        real, fake = d_out_T[0], d_out_S[0]
        if self.adv_loss == "wgan-gp":
            return -torch.mean(real) + fake.mean()
        return F.relu(1.0 - real).mean() + F.relu(1.0 + fake).mean()


class CriterionAdditionalGP(nn.Module):
    def __init__(self, D_net, lambda_gp):
        super().__init__()
        self.D = D_net
        self.lambda_gp = lambda_gp

    def forward(self, d_in_S, d_in_T, alpha=None):
        assert d_in_S[0].shape == d_in_T[0].shape, "the output dim of D with teacher and student as input differ"
        real, fake = d_in_T[0].detach(), d_in_S[0].detach()
        if alpha is None:   # criterion.py:104: one uniform sample per image
            alpha = torch.rand(real.size(0), 1, 1, 1, device=real.device, dtype=real.dtype)
        interpolated = (alpha * real + (1 - alpha) * fake).requires_grad_(True)
        out = self.D(interpolated)
        grad = torch.autograd.grad(outputs=out[0], inputs=interpolated, grad_outputs=torch.ones_like(out[0]),
                                   retain_graph=True, create_graph=True, only_inputs=True)[0]
        grad = grad.view(grad.size(0), -1)
        grad_l2norm = torch.sqrt(torch.sum(grad ** 2, dim=1))
        return self.lambda_gp * torch.mean((grad_l2norm - 1) ** 2)
