"""Dilated-ResNet PSPNet (student ResNet18 / teacher ResNet101) on MI355X.

Same public surface, module names and state-dict keys as the reference's
networks/pspnet_combine.py:114-197 (150 tensors student / 565 teacher), so its checkpoints load
and ``forward`` returns the same 7-element list ``[logits, dsn, feat_after_psp, x4, x3, x2, x1]``
(pspnet_combine.py:189).  Convolutions run on MIOpen through PyTorch-ROCm -- except the frozen teacher's 1x1 GEMMs (csrc/conv1x1.hip), its wide
stride-1 3x3 convolutions (csrc/conv3x3.hip), the student's 3x3 convolutions in its inference form (fuse_for_inference) and, opt-in,
the training student's stride-1 3x3 convolutions and their data gradients (route_training_convs; the weight gradients stay on
MIOpen unless its ``wgrad`` is set: csrc/conv3x3_wgrad.hip; the 64-channel convolutions of the stem and layer1 only with ``narrow``:
the 64-column form of csrc/conv3x3.hip), which run on the bf16 MFMA through a three-piece operand split; every normalisation is the hand-written InPlace-ABN of
csrc/abn*.hip (``libs``), applied in place on the conv output.
Which of these a convolution gets is decided in two places: _frozen_form (a frozen forward) and _train_form (a training one).
"""
import functools

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib, functional as SF
from ..libs import InPlaceABN, InPlaceABNSync  # noqa: F401  (re-exported like pspnet_combine.py:11)

affine_par = True
BatchNorm2d = functools.partial(InPlaceABNSync, activation="none")   # pspnet_combine.py:12


def _fused(module, x):
    """BN -> ReLU and BN -> (+ residual) -> ReLU collapse into single passes of the ABN kernels
    (InPlaceABNSync.forward_relu): in place with the running statistics for the frozen teacher
    (eval + no_grad, kd_model.py:121-122), out of place with batch statistics for the training student.
    Eval mode WITH a graph (rare) and non-fp32 inputs take the reference's op sequence."""
    return x.dtype == torch.float32 and (module.training or not torch.is_grad_enabled())


# The frozen network's fused inference forms.  Each one is algebraically the reference's op sequence (the tests compare the two
# on the same weights: tests/test_host_cpu.py, tests/test_kernels_gpu.py) and each was kept because its A/B on the step is
# recorded under profiles/ -- so they are constants of this module, not environment switches (round 5: the SKD_TEACHER_TAIL /
# SKD_TEACHER_BLAS / SKD_TEACHER_GEMM / SKD_PSP_FOLD / SKD_PSP_MM / SKD_HEAD_MM / SKD_MAXPOOL variables are gone; a test that
# wants the plain sequence patches the constant).  Inputs the fused forms do not cover (CPU tensors without the kernels'
# preconditions, graphs in eval mode, other dtypes) take the reference's sequence regardless.
FUSED_TAIL = True     # conv2 -> [bn2 -> relu -> conv3 -> bn3 -> + residual -> relu] as ONE fp32-MFMA GEMM (csrc/conv1x1.hip, round 3):
                      # bn2 + ReLU applied to the raw 3x3-convolution output on its way into LDS, bn3 + residual + ReLU in the epilogue;
                      # profiles/r03c_bench_ab_teacher_tail{0,1}.json: -1.1 ... -2.0 ms per step
BLAS_TAILS = True     # the 1x1 reduce convolutions and stride-1 down-sample branches as library GEMMs with the folded BN (+ ReLU)
                      # in the epilogue (functional.conv1x1_bn_blas); profiles/r02f: 68.2 -> 66.9 ms per step
HEAD_KERNEL = True    # the 19-class 1x1 heads as the skinny HBM-bound kernels of csrc/head.hip (NCHW logits out, channels-last feature
                      # gradient back) instead of 41 + 123 us convolutions per student head (round 6)
STEM_FUSED = True     # training stem: bn3 -> relu3 -> maxpool without the normalised tensor (libs.modules.forward_relu_maxpool, round 6)
PSP_FOLD = True       # conv3x3(cat(up(priors), feats)) = conv3x3(feats) + fold(priors x W) (csrc/ppm.hip); profiles/r02d: 77.4 -> 72.2 ms
CONV3X3_SPLIT = True  # the frozen network's stride-1 3x3 convolutions with >= CONV3X3_SPLIT_MIN_CIN input channels (layer3 / layer4 conv2,
                      # the PSP bottleneck's feature half, the deep-supervision head) as implicit GEMMs on the bf16 MFMA with the
                      # three-piece operand split (csrc/conv3x3.hip) instead of MIOpen's fp32-MFMA kernels; profiles/r12_conv3x3_isolated.md
                      # (1.16-1.30 x per launch), profiles/r12_step_ab.md (59.38-59.71 -> 55.40-55.67 ms per step)
CONV3X3_SPLIT_MIN_CIN = 256   # the 64- / 128-channel 3x3s (stem, layer1, layer2: narrow N, ~1.6 ms together) stay on MIOpen unless
                              # route_teacher_early flags the network (opt-in, below: the 64-column form, the wide kernel and,
                              # for layer2.0's stride-2 conv2, the stride-2 forward form of include/skd_stride2.h)
SPLIT_REDUCE = True   # the reduce / stride-1 down-sample 1x1 GEMMs on csrc/conv1x1.hip's split core instead of the library GEMM wherever
                      # profiles/r11_stage2_isolated.md shows the kernel ahead (every shape but 512 -> 128); profiles/r12_step_ab.md:
                      # 55.40-55.67 ms per step off, 54.61-55.07 on, five interleaved runs each, the sets do not overlap


# The student's inference form (fuse_for_inference, below): a flagged BasicBlock hands a 3x3 convolution to the split core when the
# kernel takes it (stride 1, Cin a multiple of 16, Cout of 128) and it has at least ``min_cin`` input channels.
# FUSED_EVAL_MIN_CIN is the default: 128, below the frozen teacher's CONV3X3_SPLIT_MIN_CIN, because at the student's evaluation
# sizes (129 x 257 maps, batch 1, shapes the shipped MIOpen find-db was not tuned for) layer2's 128 -> 128 launch is 3.2 x ahead
# of convolution + ABN pass, against a run-to-run spread of 1.1 - 2.6 % (profiles/r17_student_infer.md, which has every shape).  That
# routes layer2's three stride-1 convolutions and all of layer3 / layer4; layer2.0.conv1 (stride 2) is not the kernel's, and
# layer1 (Cout = 64) is the 64-column form's, routed only with ``narrow`` (NARROW_ROUTING_EXCLUDED below).  A routed shape that measures behind is listed in INFER_ROUTING_EXCLUDED as (Cin, Cout, dilation) and keeps
# conv -> forward_relu: none does.
FUSED_EVAL_MIN_CIN = 128
INFER_ROUTING_EXCLUDED = frozenset()


# The student's training form (route_training_convs, below; opt-in): a flagged module in training mode, with grad enabled, on an
# fp32 channels-last device input hands a stride-1 3x3 convolution with at least ``min_cin`` input channels, and its data gradient,
# to the split core (SF.conv3x3_split_train) where both directions fit it (Cin and Cout multiples of 128).  TRAIN_SPLIT_MIN_CIN = 128
# routes 13 convolutions of the ResNet18 student: layer2.0.conv2, layer2.1, layer3, layer4, the deep-supervision head's dsn[0] and
# the PSP bottleneck's feature-map half; layer2.0.conv1 and the stem's conv1 (stride 2) are not the kernel's, and the stem's
# conv2 / conv3 and layer1 (64 channels) are routed only with ``narrow`` (below).  A
# routed shape that measures behind is listed in TRAIN_ROUTING_EXCLUDED as (Cin, Cout, dilation) and keeps the library
# (profiles/r18_conv3x3_train_isolated.md has every shape).
TRAIN_SPLIT_MIN_CIN = 128
TRAIN_ROUTING_EXCLUDED = frozenset()
# The weight gradient of a routed convolution on the split core too (route_training_convs(wgrad=True); a second opt-in on top of
# the first): SF.conv3x3_split_wgrad instead of the library's kernels.  A shape whose two launches do not measure ahead of the
# library by more than the spread is listed here as (Cin, Cout, dilation) and keeps the library for its weight gradient
# (profiles/r20_conv3x3_wgrad_isolated.md has every shape).
WGRAD_ROUTING_EXCLUDED = frozenset()
# The wide convolutions of the training form on TWO bf16 pieces per operand and three products (route_training_convs(pieces=2); a
# further opt-in on top of the training form, an ACCURACY trade: include/skd_train2.h): forward, data gradient
# and -- with ``wgrad`` -- weight gradient of the 13 convolutions above take the two-piece entries.  A shape that does not measure
# ahead of its three-piece twin by more than the spread is listed here as (Cin, Cout, dilation) and keeps three pieces
# (profiles/r33_student_pieces_isolated.md).
# Measured on the MI355X at batch 8, 65 x 65: all seven shapes are ahead -- forward + data gradient + pack pair 1.57 - 1.67 x, the
# weight gradient 1.35 - 1.48 x, spreads of at most 3.2 % -- so the set is empty and the weight gradient needs no set of its own.
STUDENT_PIECES_ROUTING_EXCLUDED = frozenset()
# The same 13 convolutions on two FP16 pieces per operand with a power-of-two scale per gradient tensor
# (route_training_convs(pieces=2, piece_format="fp16"); NOT an accuracy trade: include/skd_train2h.h): forward on
# skd_conv3x3_split2h_nhwc, data gradient and -- with ``wgrad`` -- weight gradient on the scaled entries.  A shape that does not
# measure ahead of its three-piece twin by more than the spread is listed here as (Cin, Cout, dilation) and keeps THREE pieces,
# never two bf16 ones (profiles/r35_student_fp16_isolated.md).
STUDENT_FP16_ROUTING_EXCLUDED = frozenset()
# The 64-channel convolutions (fuse_for_inference(narrow=True), route_training_convs(narrow=True); a further opt-in on top of either):
# the stem's conv2 (64 -> 64) and layer1's four convolutions (128 -> 64, then three 64 -> 64) on the 64-column form of the kernel
# (csrc/conv3x3.hip with 64-column tiles), the stem's conv3 (64 -> 128) on the wide kernel in the forward and on the narrow one for its data
# gradient (layer1.0.conv1 the other way round).  These six are chosen by their channel counts -- multiples of 64 on both sides,
# one of them not a multiple of 128 -- not by ``min_cin``.  A shape
# that does not measure ahead of the library by more than the spread is listed here as (Cin, Cout, dilation, form), form =
# "infer" or "train", and keeps the library (profiles/r21_conv3x3_narrow_isolated.md has every shape).
NARROW_ROUTING_EXCLUDED = frozenset()
# The weight gradient of a convolution ``narrow`` routes on the split core too (route_training_convs(narrow_wgrad=True); a fourth
# opt-in, on top of ``narrow``): SF.conv3x3_narrow_wgrad (the 128 x 64 tile form of csrc/conv3x3_wgrad.hip) instead of the
# library's kernels.  A shape whose two launches do not measure ahead of the library by more than the spread is listed here as
# (Cin, Cout, dilation) and keeps the library for its weight gradient (profiles/r23_conv3x3_narrow_wgrad_isolated.md has every shape).
# Measured on the MI355X at batch 8: all six convolutions of the step are 0.68 - 0.85 x the library's speed, so all three of their
# shapes are listed, and the opt-in routes nothing until a kernel measures ahead.
NARROW_WGRAD_ROUTING_EXCLUDED = frozenset({(64, 64, 1), (64, 128, 1), (128, 64, 1)})
# The 1x1 down-sample (shortcut) convolutions of the BasicBlocks (route_training_convs(shortcut=True); a fifth opt-in): forward,
# data gradient and weight gradient on the split core (SF.conv1x1_split_train, include/skd_shortcut.h) instead of the library's
# kernels.  The decision is per PRODUCT: a product of a shape that does not measure ahead of the library by more than the spread is
# listed here as (Cin, Cout, stride, product), product = "fwd", "dgrad" or "wgrad", and keeps the library
# (profiles/r24_conv1x1_train_isolated.md has every shape and product).
# Measured on the MI355X at batch 8: ten of the twelve products are 1.07 - 4.5 x ahead; the weight gradients of the two shapes with
# a 64-channel side (the 128 x 64 tile form, one tile per slice) are 0.19 x and 0.39 x the library's speed -- their second launch
# sums up to 768 slices on 2048 threads and is bound by the latency of that chain -- so these two keep the library.
SHORTCUT_ROUTING_EXCLUDED = frozenset({(128, 64, 1, "wgrad"), (64, 128, 2, "wgrad")})
# The frozen teacher on TWO bf16 pieces per operand and three products (set_teacher_pieces(model, 2), below; a sixth opt-in, an
# ACCURACY trade: include/skd_split2.h): the calls of a marked Bottleneck network that run on the split core today -- the 1x1
# reduce / down-sample GEMMs and the fused tail (csrc/conv1x1.hip), the routed 3x3 convolutions, dsn[0] and the feature half of
# the PSP bottleneck (csrc/conv3x3.hip) -- take the two-piece entries.  A shape that measures behind its three-piece twin by more
# than the spread is listed here as ("1x1", K, N) or ("3x3", Cin, Cout, dilation) and keeps three pieces
# (profiles/r25_split2_isolated.md has every shape).
SPLIT2_ROUTING_EXCLUDED = frozenset()
# The frozen teacher on two FP16 pieces with a scaled residual (set_teacher_pieces(model, 2, piece_format="fp16"), below; a further
# opt-in, include/skd_split2h.h): the same modules, the same call sites, the same three products as the two bf16
# pieces above at 22 significant bits per operand instead of 16 -- the three-piece accuracy.  A shape that does not measure ahead of
# its three-piece twin by more than the spread is listed here, as above, and keeps THREE bf16 pieces
# (profiles/r32_split2h_isolated.md has every shape).
# Measured on the MI355X at batch 8: fifteen of the sixteen shapes are 1.05 - 1.56 x ahead of three pieces (the 3x3 kernel 1.50 -
# 1.56 x, within 5 - 8 % of two bf16 pieces; the 1x1 kernel, which holds two accumulator sets and runs two workgroups per CU instead
# of three, 1.05 - 1.51 x).  layer1's tail, 64 -> 256 at 129 x 129, bound by its 137 MB of activation and residual traffic, is
# BEHIND its three-piece twin: 70.9 - 71.3 us against 67.3 - 67.8 us, so it is listed and keeps three pieces.
SPLIT2H_ROUTING_EXCLUDED = frozenset({("1x1", 64, 256)})
# Batch-norm statistics from the routed convolution's epilogue (route_training_convs(bnstats=True); a seventh opt-in, on top of
# the training form): a BasicBlock's conv1 / conv2 that the training form routes -- the 11 wide convolutions of layer2-4, and
# with ``narrow`` layer1's four -- also writes one (mean, M2) per 32-row block and channel of its output (include/skd_bnstats.h),
# and the forward_relu behind it finishes those records and applies instead of reducing the tensor once more.  A shape whose
# {convolution with statistics + finalize + apply} does not measure ahead of {convolution + one-launch ABN forward} by more than
# the spread is listed here as (Cin, Cout, dilation) and keeps the pair it had (profiles/r26_conv3x3_bnstats_isolated.md has every
# shape).
# Measured on the MI355X at batch 8: no shape is ahead -- 128 -> 128 is within the spread, the others are 0.6 - 6 % behind (back to
# back the one-launch ABN forward finds the convolution's output in the caches and costs what finalize + apply cost) -- so all seven
# shapes of the step are listed, and the opt-in routes nothing until a form measures ahead.  The step with the set emptied:
# +0.14 / +0.16 ms at the median, ranges overlapping (profiles/r26_step_ab.md).
BNSTATS_ROUTING_EXCLUDED = frozenset({(128, 128, 1), (128, 256, 2), (256, 256, 2), (256, 512, 4), (512, 512, 4), (128, 64, 1),
                                      (64, 64, 1)})
# The frozen teacher's early 3x3 convolutions (route_teacher_early(model), below; an eighth opt-in): the nine convolutions of a
# flagged Bottleneck network with fewer than CONV3X3_SPLIT_MIN_CIN input channels -- the stem's conv2 (64 -> 64, bn2 + ReLU in the
# epilogue) and layer1's three conv2 on the 64-column form, the stem's conv3 (64 -> 128) and layer2's three stride-1 conv2 on the
# wide kernel, layer2.0's stride-2 conv2 on the stride-2 form (include/skd_stride2.h) -- all but the stem's conv2 raw, in front of
# the fused tail's bn2 + ReLU prologue.  A shape that does not measure ahead of the library by more than the spread is listed here
# as (Cin, Cout, stride, dilation) and keeps the library (profiles/r27_conv3x3_early_isolated.md has every shape).
# Measured on the MI355X at batch 8: all nine are 1.28 - 1.37 x ahead of the library (the five wide ones 2.09 - 2.14 x on two
# pieces) at a spread of at most 2.8 %, so the set is empty.  The step: -0.53 ms at the median, sets apart (profiles/r27_step_ab.md).
TEACHER_EARLY_ROUTING_EXCLUDED = frozenset()
# The student's stride-2 3x3 convolution in its inference form (fuse_for_inference(stride2=True); a further opt-in on top of the
# fused inference form): a flagged BasicBlock whose conv1 has stride 2 and a Cout that is a multiple of 128 -- layer2.0 (64 ->
# 128) -- runs conv1 -> bn1 -> relu as one launch of the stride-2 form.  A shape that measures behind is listed here as
# (Cin, Cout) and keeps conv -> forward_relu: none does (64 -> 128 at 257 x 513, batch 1: 3.06 x ahead of convolution + ABN pass).
STRIDE2_ROUTING_EXCLUDED = frozenset()
# The frozen teacher's conv1 -> bn1 -> relu -> conv2 link as bf16 PIECE PLANES (route_teacher_planes(model), below; a further
# opt-in, include/skd_planes.h): a flagged Bottleneck whose conv1 runs on the split reduce GEMM and whose conv2 runs on the
# wide 3x3 kernel anyway, both on three pieces, has the GEMM's epilogue write the three bf16 pieces of its result and the 3x3
# load them instead of cutting the fp32 map nine times per output tile -- layer3's 23 blocks and layer4's 3.  The outputs are bit
# for bit what they were (tests/test_conv_planes_gpu.py).  A pair whose {planes-out reduce + planes-in 3x3} does not measure
# ahead of {fp32-out reduce + fp32-in 3x3} by more than the larger side's spread is listed here as (conv1 Cin, planes, dilation)
# and keeps the fp32 link (profiles/r31_planes_isolated.md has every pair).
# Measured on the MI355X at batch 8, 65 x 65: no pair is ahead.  The 3x3 on planes takes 1.6 - 5.3 % LONGER than the 3x3 that
# splits its fp32 input itself (the split's VALU work was hidden behind the MFMAs; the planes are 6 bytes per element to load
# instead of 4), the reduce GEMM with the planes epilogue 2.5 - 9.7 % longer than its fp32 twin, the pairs 1.9 - 6.2 % longer at
# spreads of at most 1.2 % -- so all four pairs of the teacher are listed, and the opt-in routes nothing until a form measures ahead.
PLANES_ROUTING_EXCLUDED = frozenset({(512, 256, 2), (1024, 256, 2), (1024, 512, 4), (2048, 512, 4)})
# The student's inference form on two FP16 pieces with a scaled residual (fuse_for_inference(piece_format="fp16"); a further opt-in
# on top of the fused inference form, include/skd_infer2h.h): every convolution the flagged student's frozen
# forward hands to the split core -- whatever ``min_cin``, ``narrow`` and ``stride2`` route -- takes the fp16 twin of its entry:
# three products instead of six at 22 significant bits per operand, the three-piece accuracy.  A shape that does not measure ahead
# of its three-piece twin by more than the larger side's spread is listed here as (form, Cin, Cout, dilation), form = "wide",
# "wide+res", "narrow", "narrow+res" or "s2" ("+res": the residual epilogue, a BasicBlock's conv2), and keeps THREE bf16 pieces,
# never two (profiles/r34_infer2h_isolated.md has every shape).
# Measured on the MI355X at the evaluation sizes (129 x 257 for layer2-4, 257 x 513 for the stem, layer1 and the stride-2 input),
# batch 1 and 2: all fourteen shapes are ahead of three pieces at both batch sizes -- the wide forms 1.44 - 1.60 x with and without
# the residual, the 64-column forms 1.36 - 1.47 x (64 -> 64 with the residual, the shape most bound by its activation and residual
# traffic: 1.36 / 1.40 x), stride 2 1.37 - 1.47 x -- at spreads of at most 6.7 %, so the set is empty.  The whole forward at
# 1024 x 2048: 6.43 -> 4.66 ms; five scales with flip: 99.9 -> 70.2 ms, sets apart (profiles/r34_student_infer.md).
INFER2H_ROUTING_EXCLUDED = frozenset()
_TEACHER_EARLY_ENTRIES = ("skd_conv3x3_split_s2_supported", "skd_conv3x3_split_s2_nhwc", "skd_conv3x3_split_supported",
                          "skd_conv3x3_split_nhwc", "skd_conv3x3_narrow_supported", "skd_conv3x3_narrow_nhwc")


def _piece_route(module, *shape, fp16_form=True):
    """``(pieces, piece_format)`` of a frozen split-core call of ``module``: its marks (set_teacher_pieces; three bf16 pieces
    without one).  Marked for two bf16 pieces: 3 for a ``shape`` that SPLIT2_ROUTING_EXCLUDED lists.  Marked for two FP16 pieces
    (include/skd_split2h.h): ``(2, "fp16")``, and THREE bf16 pieces -- never two, which nobody asked for -- for a ``shape``
    that SPLIT2H_ROUTING_EXCLUDED lists and for a call whose form has no fp16 twin (``fp16_form=False``: the stride-2 form)."""
    pieces = getattr(module, "_skd_teacher_pieces", 3)
    if pieces == 3:
        return 3, "bf16"
    if getattr(module, "_skd_teacher_piece_format", "bf16") == "fp16":
        return (2, "fp16") if fp16_form and shape not in SPLIT2H_ROUTING_EXCLUDED else (3, "bf16")
    return (3 if shape in SPLIT2_ROUTING_EXCLUDED else pieces), "bf16"


def _pieces(module, *shape):
    """The piece count of _piece_route alone."""
    return _piece_route(module, *shape)[0]


def _piece_op(name, pieces, fmt):
    """``(op, keywords)`` of the ``functional`` op ``name`` for _piece_route's answer: the op with ``pieces`` -- the call it always
    was -- or, for fp16 pieces, its twin ``name_fp16``, which takes no piece count (looked up on ``SF`` at call time: tests patch
    those names)."""
    return (getattr(SF, name + "_fp16"), {}) if fmt == "fp16" else (getattr(SF, name), {"pieces": pieces})


def _narrow_shape(conv):
    """A convolution the ``narrow`` opt-in is about: 64 channels on one side at least, multiples of 64 on both."""
    cin, cout = conv.in_channels, conv.out_channels
    return cin % 64 == 0 and cout % 64 == 0 and (cin % 128 != 0 or cout % 128 != 0)


def _frozen_form(module, x, conv, residual=False, packing=False):
    """The split-core form ``conv(x)`` of a frozen forward takes: "wide" (the 128-column kernel), "narrow" (the 64-column entry),
    "s2" (the stride-2 one, include/skd_stride2.h) or None (the library).  ``module`` says whose convolution it is, and with it
    which policies are asked, in this order:

    a BasicBlock, behind its gate BasicBlock._infer_form (fuse_for_inference) -- each convolution is asked on its own: one the
    kernel does not take (stride 2 without ``stride2``; Cout = 64 without ``narrow``) or the policy leaves out keeps
    conv -> forward_relu while the other is fused.  "wide" for at least ``_skd_infer_min_cin`` input channels outside
    INFER_ROUTING_EXCLUDED (Cin, Cout, dilation), and from this rule alone; "s2" with ``_skd_infer_stride2`` (chosen by its stride,
    not by ``min_cin``) outside STRIDE2_ROUTING_EXCLUDED (Cin, Cout), never with a residual; "narrow" with ``_skd_infer_narrow``.
    the ResNet, for its stem's conv2 / conv3 behind its gate ResNet._stem_routed -- with ``_skd_infer_narrow`` that opt-in's
    answer and no other; otherwise route_teacher_early's.
    a Bottleneck, or None for a convolution no opt-in is about (dsn[0]) -- "wide" under CONV3X3_SPLIT for an eval-mode convolution
    with CONV3X3_SPLIT_MIN_CIN input channels or more that SF.conv3x3_split_supported takes; otherwise route_teacher_early's.

    ``_skd_infer_narrow`` (fuse_for_inference(narrow=True)): a convolution without bias, 64 channels on one side at least
    (_narrow_shape), outside NARROW_ROUTING_EXCLUDED (Cin, Cout, dilation, "infer") -- "narrow" for the 64-column entry (Cout =
    64), "wide" for the existing one (the stem's conv3, 64 -> 128).
    ``_skd_teacher_early`` (route_teacher_early), in eval mode under no grad: a convolution without bias and with fewer than
    CONV3X3_SPLIT_MIN_CIN input channels (the others are CONV3X3_SPLIT's), outside TEACHER_EARLY_ROUTING_EXCLUDED (Cin, Cout,
    stride, dilation), on a back-end that has the entries -- "s2" at stride 2, "wide" for a Cout that is a multiple of 128,
    "narrow" otherwise.  ``packing``: asked by _prepack, of a module that may be in training mode now and frozen later.

    Every answer but None is one the op's predicate gave (through ``SF.`` at call time: tests patch those names): grad enabled
    and an input that is not an fp32 channels-last map are refused there."""
    cin, cout = conv.in_channels, conv.out_channels
    block, stem = isinstance(module, BasicBlock), isinstance(module, ResNet)
    if block:
        min_cin = getattr(module, "_skd_infer_min_cin", None)
        if (conv.bias is None and min_cin is not None and cin >= min_cin
                and (cin, cout, conv.dilation[0]) not in INFER_ROUTING_EXCLUDED and SF.conv3x3_infer_supported(x, conv, residual)):
            return "wide"
        if (not residual and getattr(module, "_skd_infer_stride2", False) and conv.bias is None and tuple(conv.stride) == (2, 2)
                and (cin, cout) not in STRIDE2_ROUTING_EXCLUDED and SF.conv3x3_s2_supported(x, conv)):
            return "s2"
    elif not stem and CONV3X3_SPLIT and cin >= CONV3X3_SPLIT_MIN_CIN and not conv.training and SF.conv3x3_split_supported(x, conv):
        return "wide"
    if block or (stem and getattr(module, "_skd_infer_narrow", False)):
        if (not getattr(module, "_skd_infer_narrow", False) or conv.bias is not None or not _narrow_shape(conv)
                or (cin, cout, conv.dilation[0], "infer") in NARROW_ROUTING_EXCLUDED):
            return None
        if cout % 128 == 0:      # in a BasicBlock "wide" comes from the min_cin rule alone
            return "wide" if stem and SF.conv3x3_infer_supported(x, conv, residual) else None
        return "narrow" if SF.conv3x3_narrow_supported(x, conv, residual) else None
    if not getattr(module, "_skd_teacher_early", False) or (module.training and not packing) or torch.is_grad_enabled():
        return None
    geometry = SF.conv2d_square_geometry(conv)
    if (geometry is None or conv.bias is not None or cin >= CONV3X3_SPLIT_MIN_CIN
            or (cin, cout, geometry[0], geometry[2]) in TEACHER_EARLY_ROUTING_EXCLUDED
            or not all(_lib.has_entry(n) for n in _TEACHER_EARLY_ENTRIES)):
        return None
    if geometry[0] == 2:
        return "s2" if SF.conv3x3_s2_supported(x, conv) else None
    if cout % 128 == 0:
        return "wide" if SF.conv3x3_infer_supported(x, conv) else None
    return "narrow" if SF.conv3x3_narrow_supported(x, conv) else None


def _wgrad_routed(module, cin, cout, dilation):
    """Whether a convolution the flagged ``module`` routes takes its weight gradient on the split core as well."""
    return bool(getattr(module, "_skd_train_wgrad", False)) and (cin, cout, dilation) not in WGRAD_ROUTING_EXCLUDED


def _student_pieces(module, cin, cout, dilation):
    """The piece count of a WIDE convolution the flagged ``module`` routes: 2 where route_training_convs(pieces=2) marked it, the
    back-end has the entries of include/skd_train2.h (and the two of skd_split2.h they build on) and the shape is outside
    STUDENT_PIECES_ROUTING_EXCLUDED; 3 otherwise."""
    if (getattr(module, "_skd_train_pieces", 3) == 2 and (cin, cout, dilation) not in STUDENT_PIECES_ROUTING_EXCLUDED
            and SF.train2_supported()):
        return 2
    return 3


def _student_fp16(module, cin, cout, dilation):
    """Whether a WIDE convolution the flagged ``module`` routes runs on two fp16 pieces: route_training_convs(pieces=2,
    piece_format="fp16") marked it (``_skd_train_piece_format``, a mark of its own beside ``_skd_train_pieces``), the back-end has
    the entries of include/skd_train2h.h and the shape is outside STUDENT_FP16_ROUTING_EXCLUDED.  Otherwise three pieces."""
    return (getattr(module, "_skd_train_piece_format", "bf16") == "fp16" and (cin, cout, dilation) not in STUDENT_FP16_ROUTING_EXCLUDED
            and SF.train2h_supported())


def _train_form(module, x, conv, bn=None):
    """``(form, wgrad, stats)``: how the flagged ``module`` (route_training_convs) in training mode runs ``conv(x)``.
    ``form``: "wide" -- SF.conv3x3_split_train: at least ``_skd_train_min_cin`` input channels, outside TRAIN_ROUTING_EXCLUDED
    (Cin, Cout, dilation), a call SF.conv3x3_train_supported takes; "narrow" -- the same op with ``narrow=True``: with
    ``_skd_train_narrow``, a _narrow_shape outside NARROW_ROUTING_EXCLUDED (Cin, Cout, dilation, "train") that
    SF.conv3x3_narrow_train_supported takes; None -- the module's own forward, and the two bits False.
    ``wgrad``: the weight gradient on the split core as well -- _wgrad_routed for "wide"; ``_skd_train_narrow_wgrad`` outside
    NARROW_WGRAD_ROUTING_EXCLUDED (Cin, Cout, dilation) for "narrow".
    ``stats``: the convolution is asked for the statistics records of its output as well: the module carries the flag
    (route_training_convs(bnstats=True)), the shape is not in BNSTATS_ROUTING_EXCLUDED (Cin, Cout, dilation), the back-end has the
    entries of include/skd_bnstats.h and ``bn``, the normalisation behind the convolution, would use them (a training-mode
    ``activation='none'`` ABN whose call is not replicated)."""
    min_cin, narrow = getattr(module, "_skd_train_min_cin", None), getattr(module, "_skd_train_narrow", False)
    geometry = SF.conv2d_square_geometry(conv) if module.training and (min_cin is not None or narrow) else None
    if geometry is None:      # an unflagged module, above all: nothing but the two flags is looked at
        return None, False, False
    shape = (conv.in_channels, conv.out_channels, geometry[2])
    if (min_cin is not None and conv.in_channels >= min_cin and shape not in TRAIN_ROUTING_EXCLUDED
            and SF.conv3x3_train_supported(x, conv.weight, *geometry, conv.groups)):
        form, wgrad = "wide", _wgrad_routed(module, *shape)
    elif (narrow and _narrow_shape(conv) and shape + ("train",) not in NARROW_ROUTING_EXCLUDED
          and SF.conv3x3_narrow_train_supported(x, conv.weight, *geometry, conv.groups)):
        form, wgrad = "narrow", bool(getattr(module, "_skd_train_narrow_wgrad", False)) and shape not in NARROW_WGRAD_ROUTING_EXCLUDED
    else:
        return None, False, False
    stats = (bn is not None and bool(getattr(module, "_skd_train_bnstats", False)) and shape not in BNSTATS_ROUTING_EXCLUDED
             and SF.conv3x3_bnstats_supported() and callable(getattr(bn, "takes_partials", None)) and bn.takes_partials())
    return form, wgrad, stats


def _train_conv(module, conv, x, bn=None):
    """``(conv(x), partials)``: the convolution on the split core in both directions where _train_form says so, the module's own
    forward otherwise; ``partials`` the statistics records of the routed convolution's epilogue where it says so for ``bn`` (the
    ABN whose forward_relu follows, BasicBlock), None otherwise."""
    form, wgrad, stats = _train_form(module, x, conv, bn)
    if form is None:
        return conv(x), None
    narrow = form == "narrow"
    # two pieces: the wide form without statistics alone (the twin op only where the count is 2: every other call is what it was)
    two = not narrow and not stats and _student_pieces(module, conv.in_channels, conv.out_channels, conv.dilation[0]) == 2
    # two fp16 pieces: the same forms, under the mark of its own (a module never carries both marks)
    fp16 = not narrow and not stats and _student_fp16(module, conv.in_channels, conv.out_channels, conv.dilation[0])
    out = (SF.conv3x3_split_train_fp16 if fp16 else SF.conv3x3_split_train2 if two else SF.conv3x3_split_train)(
        x, conv.weight, conv.dilation[0], conv.bias, owner=conv, wgrad=wgrad and not narrow, narrow=narrow,
        narrow_wgrad=wgrad and narrow, stats=stats)
    return out if stats else (out, None)


def _shortcut(block, x):
    """``block.downsample(x)``: the convolution on the split core (SF.conv1x1_split_train, the products SHORTCUT_ROUTING_EXCLUDED does
    not list) where the block is flagged (route_training_convs(shortcut=True)), in training mode, its down-sample branch is
    (convolution, ABN) and the op accepts the call; the module's own forward otherwise."""
    down = block.downsample
    if getattr(block, "_skd_train_shortcut", False) and block.training and isinstance(down, nn.Sequential) and len(down) == 2:
        conv = down[0]
        geometry = SF.conv2d_square_geometry(conv)
        if (geometry is not None and conv.bias is None and tuple(conv.kernel_size) == (1, 1)
                and SF.conv1x1_train_supported(x, conv.weight, *geometry, conv.groups)):
            products = tuple(p for p in SF.SHORTCUT_PRODUCTS
                             if (conv.in_channels, conv.out_channels, geometry[0], p) not in SHORTCUT_ROUTING_EXCLUDED)
            if products:
                return down[1](SF.conv1x1_split_train(x, conv.weight, geometry[0], owner=conv, products=products))
    return down(x)


def _fused_tail(x):
    return FUSED_TAIL and not torch.is_grad_enabled() and x.dtype == torch.float32


def _blas_tail(module, x):
    return BLAS_TAILS and not module.training and not torch.is_grad_enabled()


def _reduce_on_split(x, conv, bn):
    """THE rule of _conv1x1_bn_eval: whether a 1x1 convolution + BN of the frozen network that blas_1x1_bn_supported accepted runs on
    the split-core GEMM of csrc/conv1x1.hip (SPLIT_REDUCE) and not on the library GEMM."""
    return (SPLIT_REDUCE and not (conv.in_channels == 512 and conv.out_channels == 128)      # the library wins 512 -> 128 (r11)
            and getattr(bn, "activation", None) == "none" and SF.conv1x1_abn_supported(x, conv))


def _conv1x1_bn_eval(x, conv, bn, relu, owner=None):
    """relu?(bn(conv1x1(x))) of the frozen network for a call blas_1x1_bn_supported accepted: the split-core GEMM of csrc/conv1x1.hip
    where SPLIT_REDUCE routes it there -- on two pieces where ``owner`` (the calling block) is marked by set_teacher_pieces -- the
    library GEMM with the folded BN otherwise."""
    if _reduce_on_split(x, conv, bn):
        pieces, fmt = _piece_route(owner, "1x1", conv.in_channels, conv.out_channels)
        op, kw = _piece_op("conv1x1_abn_eval", pieces, fmt)
        return op(x, conv.weight, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.eps, "relu" if relu else "none", **kw)
    return SF.conv1x1_bn_blas(x, conv, bn, relu=relu)


_UNASKED = object()      # _planes_link: conv2's form has not been asked for yet


def _planes_link(block, x):
    """``(link, form)``: whether the flagged Bottleneck ``block`` (route_teacher_planes) hands conv1 -> bn1 -> relu to conv2 as bf16
    piece planes (include/skd_planes.h) for the input ``x``, decided ONCE, before conv1 runs, from the modules and ``x`` alone:
    the block is flagged, in eval mode, under no grad; the back-end has the entries; (conv1 Cin, planes, dilation) is not in
    PLANES_ROUTING_EXCLUDED; both convolutions run on three pieces (a block set_teacher_pieces marked keeps its present path);
    conv1 would go to the split reduce GEMM anyway (_reduce_on_split, so not 512 -> 128); conv2 would take the "wide" form anyway
    (_frozen_form, asked on a stand-in with the shape and memory format conv1's output will have).  ``form``: conv2's form where
    that last question was asked -- the caller does not ask again: one routing decision per convolution -- _UNASKED otherwise."""
    c1, c2 = block.conv1, block.conv2
    if (not getattr(block, "_skd_teacher_planes", False) or block.training or torch.is_grad_enabled()
            or (c1.in_channels, c1.out_channels, c2.dilation[0]) in PLANES_ROUTING_EXCLUDED or not SF.planes_supported()
            or _pieces(block, "1x1", c1.in_channels, c1.out_channels) != 3
            or _pieces(block, "3x3", c2.in_channels, c2.out_channels, c2.dilation[0]) != 3
            or not (_blas_tail(block, x) and SF.blas_1x1_bn_supported(x, c1) and _reduce_on_split(x, c1, block.bn1))):
        return False, _UNASKED
    form = _frozen_form(block, x.new_empty((1, 1, 1, c1.out_channels)).permute(0, 3, 1, 2), c2)
    return form == "wide", form


def _infer_fp16(module, form, conv, residual=False):
    """Whether the frozen forward of ``module`` -- a BasicBlock or the ResNet (its stem) that fuse_for_inference(piece_format="fp16")
    marked -- runs ``conv`` in the ``form`` _frozen_form gave on two FP16 pieces (include/skd_infer2h.h): the mark is set, the
    back-end has the entries (``SF.infer2h_supported``, looked up at call time) and (form [+ "+res"], Cin, Cout, dilation) is not
    in INFER2H_ROUTING_EXCLUDED.  Asked only where a form was given, i.e. in eval mode under no grad (or by _prepack)."""
    if getattr(module, "_skd_infer_piece_format", "bf16") != "fp16" or not SF.infer2h_supported():
        return False
    key = form + ("+res" if residual and form != "s2" else "")
    return (key, conv.in_channels, conv.out_channels, conv.dilation[0]) not in INFER2H_ROUTING_EXCLUDED


def _split_conv_fp16(x, conv, form, bn, activation, residual):
    """_split_conv's launch on two fp16 pieces: the twin op of each form on the twin pack (include/skd_infer2h.h; "wide" without
    residual: the existing entry of include/skd_split2h.h)."""
    if form == "narrow":
        return SF.conv3x3_narrow_eval_fp16(x, SF.conv3x3_narrow_pack_weights_fp16(conv), conv.out_channels, conv.dilation[0], residual,
                                           conv.bias, bn, activation)
    pack = SF.conv3x3_pack_weights_fp16(conv)
    if form == "s2":
        return SF.conv3x3_s2_eval_fp16(x, pack, conv.out_channels, conv.bias, bn, activation)
    if residual is not None:
        return SF.conv3x3_split_res_eval_fp16(x, pack, conv.out_channels, conv.dilation[0], residual, bn, activation, conv.bias)
    return SF.conv3x3_split_eval_fp16(x, pack, conv.out_channels, conv.dilation[0], conv.bias, bn, activation)


def _split_conv(x, conv, form, bn=None, activation="none", residual=None, owner=None, infer=None):
    """act(bn(conv(x)) [+ residual]) as one launch of csrc/conv3x3.hip on ``conv``'s cached pack, in the ``form`` _frozen_form
    gave: "wide"; "narrow", the 64-column form (the same file, include/skd_narrow.h) on its own pack; "s2", the stride-2 form
    (include/skd_stride2.h) on the wide form's pack.  ``owner``: the calling module of a frozen teacher; where set_teacher_pieces
    marked it, "wide" without residual and "s2" run on two pieces (their own pack); the other two keep three.  Marked for fp16
    pieces, "wide" without residual runs on them and "s2", which has no fp16 form for the teacher, on three bf16 pieces (_piece_route).
    ``infer``: the calling module of a student's inference form (a BasicBlock, or the ResNet for its stem); where
    fuse_for_inference(piece_format="fp16") marked it, every form runs on two fp16 pieces (_infer_fp16), a mark of its own that
    ``owner``'s rules never see."""
    if infer is not None and _infer_fp16(infer, form, conv, residual is not None):
        return _split_conv_fp16(x, conv, form, bn, activation, residual)
    pieces, fmt = _piece_route(owner, "3x3", conv.in_channels, conv.out_channels, conv.dilation[0], fp16_form=form != "s2")
    if form == "narrow":
        return SF.conv3x3_narrow_eval(x, SF.conv3x3_narrow_pack_weights(conv), conv.out_channels, conv.dilation[0], residual, conv.bias,
                                      bn, activation)
    if form == "s2":
        return SF.conv3x3_s2_eval(x, SF.conv3x3_pack_weights(conv, pieces=pieces), conv.out_channels, conv.bias, bn, activation,
                                  pieces=pieces)
    if residual is not None:
        return SF.conv3x3_split_res_eval(x, SF.conv3x3_pack_weights(conv, pieces=3), conv.out_channels, conv.dilation[0], residual, bn,
                                         activation, conv.bias)
    (pack, pkw), (run, kw) = _piece_op("conv3x3_pack_weights", pieces, fmt), _piece_op("conv3x3_split_eval", pieces, fmt)
    return run(x, pack(conv, **pkw), conv.out_channels, conv.dilation[0], conv.bias, bn, activation, **kw)


class _ClassifierConvFn(torch.autograd.Function):
    """conv2d with a bias whose gradient is reduced in two stages.  The stock backward sums the (B, 19, 65, 65) gradient over
    (0, 2, 3) in one reduction with 19 outputs -- two workgroups' worth of parallelism: 89-94 us per head on MI355X, 0.18 ms of the
    step (profiles/r05l trace, main stream).  Summing the rows first (B * H * 19 outputs) and the row sums second takes two
    launches of a few microseconds; the data gradient and the weight gradient are MIOpen's, as before, asked for through the PUBLIC
    ``torch.nn.grad`` wrappers (round 6: the positional ``aten.convolution_backward`` call is gone)."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding, dilation):
        ctx.save_for_backward(x, weight)
        ctx.conv = (stride, padding, dilation)
        return F.conv2d(x, weight, bias, stride, padding, dilation)

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        stride, padding, dilation = ctx.conv
        gx = torch.nn.grad.conv2d_input(x.shape, weight, g, stride, padding, dilation) if ctx.needs_input_grad[0] else None
        gw = torch.nn.grad.conv2d_weight(x, weight.shape, g, stride, padding, dilation) if ctx.needs_input_grad[1] else None
        gb = g.permute(0, 2, 3, 1).sum(2).sum((0, 1)) if ctx.needs_input_grad[2] else None
        return gx, gw, gb, None, None, None


class ClassifierConv(nn.Conv2d):
    """``nn.Conv2d`` (same parameters, same state-dict keys: pspnet_combine.py:138-154) for the few-channel classifier heads.
    The two-stage bias gradient covers what the heads are -- ungrouped, zero padding given as numbers; any other construction
    takes the stock operator (never a silently wrong gradient)."""

    def _plain(self):
        return (self.groups == 1 and self.padding_mode == "zeros" and not isinstance(self.padding, str)
                and not self.transposed and tuple(self.output_padding) == (0, 0))

    def forward(self, x):
        if HEAD_KERNEL and SF.head1x1_supported(x, self):
            return SF.head1x1(x, self)
        if (self.bias is None or not self._plain()
                or not (torch.is_grad_enabled() and (x.requires_grad or self.weight.requires_grad))):
            return super().forward(x)
        return _ClassifierConvFn.apply(x, self.weight, self.bias, self.stride, self.padding, self.dilation)


def conv3x3(in_planes, out_planes, stride=1):
    return nn.Conv2d(in_planes, out_planes, kernel_size=3, stride=stride, padding=1, bias=False)


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, multi_grid=1):
        super().__init__()
        d = dilation * multi_grid
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, d, d, bias=False)
        self.bn1 = BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=False)       # ABN keeps its OUTPUT for backward: not in place
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, d, d, bias=False)
        self.bn2 = BatchNorm2d(planes)
        self.relu_inplace = nn.ReLU(inplace=True)
        self.downsample = downsample

    def _infer_form(self, x):
        """Whether this call takes the inference form: the block is flagged (fuse_for_inference), frozen for this call (eval mode,
        no grad), the input is an fp32 channels-last map and both normalisations are plain eval-mode BatchNorms."""
        return (getattr(self, "_skd_infer_min_cin", None) is not None and not self.training and not torch.is_grad_enabled()
                and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last)
                and all(getattr(bn, "activation", None) == "none" and getattr(bn, "running_mean", None) is not None
                        and getattr(bn, "running_var", None) is not None for bn in (self.bn1, self.bn2)))

    def _forward_infer(self, x):
        """relu(bn1(conv1(x))) and relu(bn2(conv2(.)) + residual) as one launch of csrc/conv3x3.hip each (BN + ReLU, and BN +
        residual + ReLU, in the epilogue) where _frozen_form says so."""
        f1 = _frozen_form(self, x, self.conv1)
        out = _split_conv(x, self.conv1, f1, self.bn1, "relu", infer=self) if f1 else self.bn1.forward_relu(self.conv1(x))
        f2 = _frozen_form(self, out, self.conv2, True)
        if self.downsample is None:
            residual = x
        elif not (f1 or f2):                 # nothing of this block is routed: the sequence it ran before, op for op
            residual = self.downsample(x)
        elif (_blas_tail(self, x) and len(self.downsample) == 2 and SF.blas_1x1_bn_supported(x, self.downsample[0])
              and getattr(self.downsample[1], "activation", None) == "none"):
            residual = _conv1x1_bn_eval(x, self.downsample[0], self.downsample[1], relu=False)
        else:
            residual = self.downsample(x)
        if f2:
            return _split_conv(out, self.conv2, f2, self.bn2, "relu", residual, infer=self)
        return self.bn2.forward_relu(self.conv2(out), residual)

    def forward(self, x):
        if self._infer_form(x):
            return self._forward_infer(x)
        if _fused(self, x):
            # ``partials``: where route_training_convs(bnstats=True) flagged the block, a routed convolution hands the statistics of
            # its output on; None otherwise, which is forward_relu without them
            y, partials = _train_conv(self, self.conv1, x, self.bn1)
            out = self.bn1.forward_relu(y, partials=partials)
            residual = _shortcut(self, x) if self.downsample is not None else x
            y, partials = _train_conv(self, self.conv2, out, self.bn2)
            return self.bn2.forward_relu(y, residual, partials=partials)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        residual = _shortcut(self, x) if self.downsample is not None else x
        return self.relu_inplace(out + residual)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, fist_dilation=1, multi_grid=1):
        super().__init__()
        d = dilation * multi_grid
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, d, d, bias=False)
        self.bn2 = BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=False)
        self.relu_inplace = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.dilation = dilation
        self.stride = stride

    def forward(self, x):
        if _fused(self, x):
            blas = _blas_tail(self, x)
            # route_teacher_planes: relu(bn1(conv1(x))) reaches conv2 as bf16 piece planes (SF.Planes), not as an fp32 map
            link, form = _planes_link(self, x)
            if link:
                out = SF.conv1x1_abn_planes_eval(x, self.conv1.weight, self.bn1.running_mean, self.bn1.running_var, self.bn1.weight,
                                                 self.bn1.bias, self.bn1.eps, "relu")
            elif blas and SF.blas_1x1_bn_supported(x, self.conv1):
                out = _conv1x1_bn_eval(x, self.conv1, self.bn1, relu=True, owner=self)
            else:
                out = self.bn1.forward_relu(self.conv1(x))
            # raw output: bn2 + ReLU stay in the tail GEMM's prologue (or the pass below)
            if form is _UNASKED:
                form = _frozen_form(self, out, self.conv2)      # layer3 / layer4; layer1 / layer2 of a teacher route_teacher_early flagged
            c2 = _split_conv(out, self.conv2, form, owner=self) if form else self.conv2(out)
            tail = (not self.training and _fused_tail(x) and SF.conv1x1_abn_supported(c2, self.conv3) and self.conv3.in_channels <= 512
                    and getattr(self.bn2, "activation", None) == "none" and getattr(self.bn3, "activation", None) == "none")
            if not tail:
                out = self.bn2.forward_relu(c2)
            if self.downsample is None:
                residual = x
            elif (blas and len(self.downsample) == 2 and SF.blas_1x1_bn_supported(x, self.downsample[0])
                  and getattr(self.downsample[1], "activation", None) == "none"):
                residual = _conv1x1_bn_eval(x, self.downsample[0], self.downsample[1], relu=False, owner=self)
            else:
                residual = self.downsample(x)
            if tail:
                pieces, fmt = _piece_route(self, "1x1", self.conv3.in_channels, self.conv3.out_channels)
                op, kw = _piece_op("conv1x1_abn_eval", pieces, fmt)
                return op(c2, self.conv3.weight, self.bn3.running_mean, self.bn3.running_var, self.bn3.weight,
                          self.bn3.bias, self.bn3.eps, "relu", residual=residual, pro=SF.abn_pack_eval_params(self.bn2), **kw)
            return self.bn3.forward_relu(self.conv3(out), residual)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        residual = self.downsample(x) if self.downsample is not None else x
        return self.relu_inplace(out + residual)


def _conv1x1_as_mm(conv, x):
    """conv(x) for a plain 1x1 convolution (with or without bias) on a channels-last map, as one matrix product
    (differentiable)."""
    if not (conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.padding == (0, 0) and conv.groups == 1
            and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last)):
        return conv(x)
    b, c, h, w = x.shape
    x2, wt = x.permute(0, 2, 3, 1).reshape(b * h * w, c), conv.weight.reshape(conv.out_channels, c).t()
    out = torch.mm(x2, wt) if conv.bias is None else torch.addmm(conv.bias, x2, wt)
    return out.view(b, h, w, conv.out_channels).permute(0, 3, 1, 2)


class PSPModule(nn.Module):
    """Pyramid pooling (pspnet_combine.py:86-112): pooled priors at 1,2,3,6 -> 1x1 conv -> ABN(leaky)
    -> bilinear (align_corners) back to the feature size -> concat -> 3x3 conv -> ABN(leaky) -> Dropout2d."""

    def __init__(self, features, out_features=512, sizes=(1, 2, 3, 6)):
        super().__init__()
        self.stages = nn.ModuleList([self._make_stage(features, out_features, s) for s in sizes])
        self.bottleneck = nn.Sequential(
            nn.Conv2d(features + len(sizes) * out_features, out_features, 3, padding=1, dilation=1, bias=False),
            InPlaceABNSync(out_features),
            nn.Dropout2d(0.1))

    def _make_stage(self, features, out_features, size):
        return nn.Sequential(nn.AdaptiveAvgPool2d(output_size=(size, size)),
                             nn.Conv2d(features, out_features, 1, bias=False),
                             InPlaceABNSync(out_features))

    def forward(self, feats):
        sizes = []
        for stage in self.stages:
            o = stage[0].output_size
            sizes.append(o[0] if isinstance(o, (tuple, list)) else o)
        nhwc = feats.dim() == 4 and not feats.is_contiguous() and feats.is_contiguous(memory_format=torch.channels_last)
        if (feats.dtype == torch.float32 and len(sizes) <= 4 and (nhwc or feats.size(3) <= 256)
                and min(feats.size(2), feats.size(3)) >= max(sizes)):
            # csrc/ppm.hip: every pyramid level from one read of feats; priors up-sampled straight into the
            # concatenated tensor (no adaptive-pool / upsample / cat launches, no atomics in backward)
            # channels-last feature maps take the channels-last kernels (no layout copies); anything else the NCHW ones
            pooled = SF.ppm_pool(feats, sizes)
            if nhwc:
                # a 1x1 convolution of a (B, C, s, s) channels-last map is the GEMM (B s^2, C) x (C, Cout): one tiny
                # rocBLAS call instead of MIOpen's ~30 us (forward) / ~100 us (backward) launch sequences per level
                priors = [stage[2](_conv1x1_as_mm(stage[1], p)) for stage, p in zip(self.stages, pooled)]
            else:
                priors = [stage[2](stage[1](p)) for stage, p in zip(self.stages, pooled)]
            conv = self.bottleneck[0]
            if (nhwc and PSP_FOLD and SF.ppm_fold_supported(feats, sizes) and conv.bias is None
                    and conv.kernel_size == (3, 3) and conv.padding == (1, 1) and conv.stride == (1, 1)
                    and conv.dilation == (1, 1) and conv.groups == 1 and conv.out_channels % 4 == 0
                    and all(p.shape[1] == priors[0].shape[1] for p in priors)):
                # the priors never meet the convolution: conv3x3(cat) = conv3x3(feats) + fold(priors x W) by linearity
                if not hasattr(self, "_fold_cache"):
                    self._fold_cache = {}
                min_cin = getattr(self, "_skd_train_min_cin", None)
                # the frozen feature half on two pieces, bf16 or fp16 (set_teacher_pieces); the trained one on two bf16 pieces
                # (route_training_convs(pieces=2))
                pieces, fmt = ((_student_pieces(self, feats.shape[1], conv.out_channels, 1), "bf16") if self.training
                               else _piece_route(self, "3x3", feats.shape[1], conv.out_channels, 1))
                fold, kw = _piece_op("ppm_fold_bottleneck", pieces, fmt)
                if self.training and _student_fp16(self, feats.shape[1], conv.out_channels, 1):
                    # the trained feature half on two fp16 pieces (route_training_convs(piece_format="fp16"))
                    fold, kw = SF.ppm_fold_bottleneck_train_fp16, {}
                out = fold(priors, feats, conv.weight, self._fold_cache,
                           split3x3=CONV3X3_SPLIT and not self.training and feats.shape[1] >= CONV3X3_SPLIT_MIN_CIN,
                           split_train=(min_cin is not None and self.training and feats.shape[1] >= min_cin
                                        and (feats.shape[1], conv.out_channels, 1) not in TRAIN_ROUTING_EXCLUDED),
                           split_wgrad=_wgrad_routed(self, feats.shape[1], conv.out_channels, 1), **kw)
                return self.bottleneck[2](self.bottleneck[1](out))
            return self.bottleneck(SF.ppm_concat(priors, feats))
        h, w = feats.size(2), feats.size(3)
        priors = [F.interpolate(stage(feats), size=(h, w), mode="bilinear", align_corners=True)
                  for stage in self.stages] + [feats]
        return self.bottleneck(torch.cat(priors, 1))


class ResNet(nn.Module):
    def __init__(self, block, layers, num_classes):
        self.inplanes = 128
        super().__init__()
        self.conv1 = conv3x3(3, 64, stride=2)
        self.bn1 = BatchNorm2d(64)
        self.relu1 = nn.ReLU(inplace=False)
        self.conv2 = conv3x3(64, 64)
        self.bn2 = BatchNorm2d(64)
        self.relu2 = nn.ReLU(inplace=False)
        self.conv3 = conv3x3(64, 128)
        self.bn3 = BatchNorm2d(128)
        self.relu3 = nn.ReLU(inplace=False)
        self.relu = nn.ReLU(inplace=False)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1, ceil_mode=True)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=1, dilation=2)
        self.layer4 = self._make_layer(block, 512, layers[3], stride=1, dilation=4, multi_grid=(1, 1, 1))
        layers = list(layers)
        if layers == [3, 4, 23, 3]:
            feat, mid = 2048, 512
        elif layers == [2, 2, 2, 2]:
            feat, mid = 512, 128
        else:
            raise ValueError("layers should be [3, 4, 23, 3] or [2, 2, 2, 2]")
        self.pspmodule = PSPModule(feat, mid)
        self.head = ClassifierConv(mid, num_classes, 1, 1, 0, bias=True)
        self.dsn = nn.Sequential(
            nn.Conv2d(feat // 2, mid, 3, 1, 1),
            InPlaceABNSync(mid),
            nn.Dropout2d(0.1),
            ClassifierConv(mid, num_classes, 1, 1, 0, bias=True))

    def _make_layer(self, block, planes, blocks, stride=1, dilation=1, multi_grid=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(
                nn.Conv2d(self.inplanes, planes * block.expansion, 1, stride, bias=False),
                BatchNorm2d(planes * block.expansion, affine=affine_par))
        grid = lambda i: multi_grid[i % len(multi_grid)] if isinstance(multi_grid, tuple) else 1
        mods = [block(self.inplanes, planes, stride, dilation=dilation, downsample=downsample, multi_grid=grid(0))]
        self.inplanes = planes * block.expansion
        for i in range(1, blocks):
            mods.append(block(self.inplanes, planes, dilation=dilation, multi_grid=grid(i)))
        return nn.Sequential(*mods)

    def _dsn_head(self, x3):
        """``self.dsn(x3)``; for the frozen network its 3x3 convolution, bias, eval-mode ABN and activation are one launch of
        csrc/conv3x3.hip (the Dropout2d between them and the classifier is the identity in eval mode)."""
        conv, bn = self.dsn[0], self.dsn[1]
        if (not self.training and not torch.is_grad_enabled() and getattr(bn, "activation", None) in ("none", "relu", "leaky_relu")
                and hasattr(bn, "running_mean") and _frozen_form(None, x3, conv)):      # no opt-in is about dsn[0]
            return self.dsn[3](_split_conv(x3, conv, "wide", bn, bn.activation, owner=self))
        if _train_form(self, x3, conv)[0] == "wide":      # the same sequence with dsn[0] (bias in the epilogue) on the split core
            return self.dsn[3](self.dsn[2](bn(_train_conv(self, conv, x3)[0])))
        return self.dsn(x3)

    def _stem_routed(self, x):
        """Whether the frozen forward asks _frozen_form about the stem's conv2 / conv3: this network is flagged
        (fuse_for_inference(narrow=True), or route_teacher_early for a frozen Bottleneck network: an unflagged teacher never is), no
        grad, ``x`` an fp32 channels-last map and bn2 a plain eval-mode BatchNorm."""
        return ((getattr(self, "_skd_infer_narrow", False) or getattr(self, "_skd_teacher_early", False))
                and not torch.is_grad_enabled() and x.dim() == 4
                and x.is_contiguous(memory_format=torch.channels_last) and getattr(self.bn2, "activation", None) == "none"
                and getattr(self.bn2, "running_mean", None) is not None and getattr(self.bn2, "running_var", None) is not None)

    def forward(self, x):
        if _fused(self, x) and not self.training and getattr(self.bn3, "activation", None) == "none":
            # Frozen network: eval-mode BN + ReLU is a non-decreasing map per channel (its scale (|gamma| + eps) / sqrt(var + eps) is
            # positive and every fp32 step of it -- subtract, multiply, multiply-add, max(., 0) -- is monotone), so it COMMUTES with
            # the max-pool bit for bit: relu(bn(max(window))) == max(relu(bn(.)) over the window).  The pass over the 268 MB
            # conv3 output becomes a pass over the 68 MB pooled map (pspnet_combine.py:131-135; VERDICT r04 missing 5).
            x = self.bn1.forward_relu(self.conv1(x))
            if self._stem_routed(x):
                # conv2 + bn2 + ReLU as one launch of the 64-column form, conv3 raw on the wide kernel.  ``owner=self``: conv3 on
                # two pieces where set_teacher_pieces marked this network; it marks the modules of Bottleneck networks alone, so
                # a student's never carry ``_skd_teacher_pieces`` and its conv3 keeps three
                f2 = _frozen_form(self, x, self.conv2)
                # ``infer=self``: both on two fp16 pieces where fuse_for_inference(piece_format="fp16") marked this network
                x = (_split_conv(x, self.conv2, f2, self.bn2, "relu", infer=self) if f2 == "narrow"
                     else self.bn2.forward_relu(self.conv2(x)))
                c3 = (_split_conv(x, self.conv3, "wide", owner=self, infer=self) if _frozen_form(self, x, self.conv3) == "wide"
                      else self.conv3(x))
            else:
                x = self.bn2.forward_relu(self.conv2(x))
                c3 = self.conv3(x)
            x = self.bn3.forward_relu(SF.max_pool_stem(c3, self.maxpool))
        else:
            if _fused(self, x):
                x = self.bn1.forward_relu(self.conv1(x))
                x = self.bn2.forward_relu(_train_conv(self, self.conv2, x)[0])
                # training: bn3 -> relu3 -> maxpool in two fused passes per direction (csrc/abn_stem.hip, round 6): the
                # 268 MB normalised conv3 output is never written, its gradient never un-pooled into memory; STEM_FUSED = False or an
                # input the fused kernels do not take: forward_relu, then csrc/maxpool.hip (channels-last) / the stock pool
                c3 = _train_conv(self, self.conv3, x)[0]    # the library's, unless route_training_convs(narrow=True) flagged the stem
                x = (self.bn3.forward_relu_maxpool(c3, self.maxpool) if STEM_FUSED
                     else SF.max_pool_stem(self.bn3.forward_relu(c3), self.maxpool))
            else:
                x = self.relu1(self.bn1(self.conv1(x)))
                x = self.relu2(self.bn2(self.conv2(x)))
                x = self.relu3(self.bn3(self.conv3(x)))
                x = SF.max_pool_stem(x, self.maxpool)       # csrc/maxpool.hip for channels-last maps, the stock op otherwise
        x1 = self.layer1(x)
        x2 = self.layer2(x1)
        x3 = self.layer3(x2)
        # the deep-supervision head feeds only CriterionDSN; a frozen network whose CE nobody computes may skip it (``skip_dsn``, set by
        # bench.py --dsn-ab for an informative figure; default: computed, like the reference's forward).  (The 19-class 1x1 classifiers
        # as skinny GEMMs were measured SLOWER than MIOpen -- rocBLAS picks a 311 us kernel for the 19 x 128 weight gradient over 33800
        # rows, 67.5 vs 67.2 ms per step -- and that variant is gone.)
        if getattr(self, "skip_dsn", False) and not torch.is_grad_enabled():
            x_dsn = None
        elif getattr(self, "dsn_last", None) is not None and not torch.is_grad_enabled():
            # frozen network on a stream of its own (NetModel, SKD_TEACHER_STREAM): the deep-supervision branch is independent of
            # layer4 / pyramid / head and nothing the criteria read -- it is issued LAST, behind a call-back that marks the outputs
            # the criteria do read as complete (same operations, same results)
            x4 = self.layer4(x3)
            x_feat_after_psp = self.pspmodule(x4)
            x = self.head(x_feat_after_psp)
            self.dsn_last(x, x_feat_after_psp)
            x_dsn = self._dsn_head(x3)
            return [x, x_dsn, x_feat_after_psp, x4, x3, x2, x1]
        else:
            x_dsn = self._dsn_head(x3)
        x4 = self.layer4(x3)
        x_feat_after_psp = self.pspmodule(x4)
        x = self.head(x_feat_after_psp)
        return [x, x_dsn, x_feat_after_psp, x4, x3, x2, x1]


def Res_pspnet(block=Bottleneck, layers=[3, 4, 23, 3], num_classes=21):
    """ResNet(Bottleneck, [3, 4, 23, 3], C) = teacher; ResNet(BasicBlock, [2, 2, 2, 2], C) = student."""
    return ResNet(block, layers, num_classes)


def _prepack(module, convs):
    """Make the weight pack of every ``(conv, residual?)`` of the freshly flagged ``module`` that _frozen_form routes and whose
    fp32 weight is on the device already: the form is asked with a one-pixel channels-last map of the right width, and "wide" and
    "s2" (which runs on the wide form's pack) take the piece count _split_conv will ask for with ``module`` as the owner."""
    with torch.no_grad():
        for conv, residual in convs:
            w = conv.weight
            if not (w.is_cuda or _lib.test_backend_active()) or w.dtype != torch.float32:
                continue
            form = _frozen_form(module, w.new_empty((1, 1, 1, conv.in_channels)).permute(0, 3, 1, 2), conv, residual, packing=True)
            if form and _infer_fp16(module, form, conv, residual):      # fuse_for_inference(piece_format="fp16"): the twin pack alone
                (SF.conv3x3_narrow_pack_weights_fp16 if form == "narrow" else SF.conv3x3_pack_weights_fp16)(conv)
            elif form == "narrow":
                SF.conv3x3_narrow_pack_weights(conv)
            elif form:
                pieces, fmt = _piece_route(module, "3x3", conv.in_channels, conv.out_channels, conv.dilation[0], fp16_form=form != "s2")
                pack, kw = _piece_op("conv3x3_pack_weights", pieces, fmt)
                pack(conv, **kw)


def fuse_for_inference(model, enable=True, min_cin=FUSED_EVAL_MIN_CIN, narrow=False, stride2=False, piece_format="bf16"):
    """Flag every BasicBlock of ``model`` (the student) for the fused inference form and return ``model``.

    A flagged block in eval mode, with grad disabled, on an fp32 channels-last input runs ``conv1 -> bn1 -> relu`` and
    ``conv2 -> bn2 -> + residual -> relu`` as one launch each of the split-core 3x3 convolution (csrc/conv3x3.hip) wherever the
    kernel takes the convolution and it has at least ``min_cin`` input channels (FUSED_EVAL_MIN_CIN above); every other convolution,
    and every training forward or forward with a graph, is what it was.  So the flag may be set on a live student: the
    packed weights are keyed on ``(data_ptr, _version)`` and rebuild themselves after each optimizer update that advances the
    version -- torch's FUSED optimizers do not, so the optimizer needs ``kd_model.advance_versions_after_step`` as a step post-hook
    (NetModel registers it on the student's optimizer; a caller with a fused optimizer of their own must do so themselves), or
    every evaluation behind the first runs on stale packs.  The weights that
    are routed and already on the device are packed here, so a graph captured later allocates nothing for them.
    ``narrow=True`` (a further opt-in): the 64-channel convolutions as well, in the same kind of forward -- layer1's four on the
    64-column form of the kernel (include/skd_narrow.h; BN + ReLU, and BN + residual + ReLU, in the epilogue), the stem's
    conv2 on it with bn2 + ReLU in the epilogue, the stem's conv3 (64 -> 128) raw on the existing kernel in front of
    max_pool_stem and bn3 -- except the shapes of NARROW_ROUTING_EXCLUDED.  The stem is flagged on the ResNet itself.
    ``stride2=True`` (a further opt-in): a flagged block whose ``conv1`` has stride 2 and a Cout that is a multiple of 128 -- in the
    student layer2.0 (64 -> 128) -- runs ``conv1 -> bn1 -> relu`` as one launch of the stride-2 form of the kernel
    (include/skd_stride2.h) on the wide form's pack -- except the shapes of STRIDE2_ROUTING_EXCLUDED; the default leaves every
    existing call as it is.
    ``piece_format="fp16"`` (a further opt-in, NOT an accuracy trade: include/skd_infer2h.h): every convolution
    the flags above hand to the split core runs on two FP16 pieces with the residual scaled by 2^11 -- three products instead of
    six at the three-piece accuracy -- through the twin op of its form: the wide form with and without the residual, the
    64-column form (the stem's ``conv2`` too), the stem's ``conv3`` and, with ``stride2``, the stride-2 ``conv1`` -- except the
    shapes of INFER2H_ROUTING_EXCLUDED, which keep THREE bf16 pieces.  "fp16" means two fp16 pieces, the only fp16 form there
    is; anything but "bf16" and "fp16" is a ValueError.  The mark (``_skd_infer_piece_format``, on the BasicBlocks and on the
    ResNet for its stem) is this function's own: set_teacher_pieces and what it routes never see it.  An activation beyond
    +-65504 gives non-finite outputs (the header's range contract).  On a back-end without the entries it warns once
    (RuntimeWarning, naming skd_infer2h.h) and the student stays on three pieces.
    ``enable=False`` clears the flags and drops the packs.  On a back-end without the entries (the tests' C double) the flag
    is set and changes nothing."""
    SF.check_piece_format(piece_format)
    if enable and piece_format == "fp16" and not SF.infer2h_supported():
        import warnings
        warnings.warn("fuse_for_inference: this back-end lacks the fp16 two-piece entries (include/skd_infer2h.h); the student "
                      "stays on three pieces", RuntimeWarning, stacklevel=2)
        piece_format = "bf16"
    for m in model.modules():
        if not isinstance(m, (BasicBlock, ResNet)):
            continue
        stem = isinstance(m, ResNet)
        convs = ((m.conv2, False), (m.conv3, False)) if stem else ((m.conv1, False), (m.conv2, True))
        m._skd_infer_narrow = bool(narrow and enable)
        if enable and piece_format == "fp16":
            m._skd_infer_piece_format = "fp16"
        else:
            vars(m).pop("_skd_infer_piece_format", None)
        if not stem:
            m._skd_infer_stride2 = bool(stride2 and enable)
        if not enable:
            if not stem:
                m._skd_infer_min_cin = None
            for conv, _ in convs:
                SF.drop_conv3x3_packs(conv)
            continue
        if not stem:
            m._skd_infer_min_cin = int(min_cin)
        _prepack(m, convs)
    return model


def route_teacher_early(model, enable=True):
    """Flag ``model`` (a frozen Bottleneck network: the teacher) for its early 3x3 convolutions on the split core and return it.

    A flagged network in eval mode, under no grad, on an fp32 channels-last device input runs the nine 3x3 convolutions below
    CONV3X3_SPLIT_MIN_CIN input channels on csrc/conv3x3.hip instead of the library: the stem through the path the student's takes
    under fuse_for_inference(narrow=True) (``conv2`` + bn2 + ReLU as one launch of the 64-column form, ``conv3`` raw on the wide kernel),
    layer1's three ``conv2`` raw on the 64-column form, layer2's three stride-1 ``conv2`` raw on the wide kernel and layer2.0's
    stride-2 ``conv2`` raw on the stride-2 form (include/skd_stride2.h) -- except the shapes of TEACHER_EARLY_ROUTING_EXCLUDED.  The
    raw outputs feed the fused tail's bn2 + ReLU prologue as in layer3 / layer4; everything else is what it was.  Under
    ``set_teacher_pieces(model, 2)`` the five wide calls (the stem's ``conv3``, layer2's four) take two pieces unless
    SPLIT2_ROUTING_EXCLUDED lists them as ("3x3", Cin, Cout, dilation); the four 64-column calls keep three.  Call it behind
    set_teacher_pieces and with the weights where they will stay (device, memory format): the packs of the routed weights are made
    here, so a graph captured later allocates nothing for them.  A BasicBlock network (the student) is left untouched.
    ``enable=False`` clears the flags and drops the packs.  On a back-end without the entries (the tests' C double) the flag is
    set and changes nothing."""
    if not any(isinstance(m, Bottleneck) for m in model.modules()):
        return model
    for m in model.modules():
        if not isinstance(m, (Bottleneck, ResNet)):
            continue
        convs = [c for c in ((m.conv2, m.conv3) if isinstance(m, ResNet) else (m.conv2,))
                 if tuple(c.kernel_size) == (3, 3) and c.in_channels < CONV3X3_SPLIT_MIN_CIN]
        if not enable:
            vars(m).pop("_skd_teacher_early", None)
            for conv in convs:
                SF.drop_conv3x3_packs(conv)
            continue
        m._skd_teacher_early = True
        _prepack(m, [(conv, False) for conv in convs])
    return model


def route_teacher_planes(model, enable=True):
    """Flag the Bottlenecks of ``model`` (a frozen Bottleneck network: the teacher) for the piece-plane link and return it.

    A flagged Bottleneck in eval mode, under no grad, whose ``conv1`` runs on the split reduce GEMM and whose ``conv2`` runs on the
    wide split-core 3x3 kernel anyway, both on three pieces, has the GEMM's epilogue write relu(bn1(conv1(x))) as its three bf16
    pieces (include/skd_planes.h, ``SF.conv1x1_abn_planes_eval``) and the 3x3 load those pieces instead of
    splitting the fp32 map itself (_planes_link has the whole rule) -- except the pairs of PLANES_ROUTING_EXCLUDED.  With today's
    rules that is layer3's 23 blocks and layer4's 3; layer1 (64 columns), layer2 (library 512 -> 128, or the early forms) and a
    block marked by ``set_teacher_pieces(model, 2)`` keep their present path.  The outputs are bit for bit what they were: the
    split is a pure function of the fp32 value.  Everything behind ``conv2`` is unchanged.  It composes with route_teacher_early,
    which routes other blocks, and works inside a graph capture: the planes are a torch allocation like the fp32 map they replace.
    ``enable=False`` clears the flags.  A BasicBlock network (the student) is left untouched.  On a back-end without the entries
    it warns once (RuntimeWarning, naming skd_planes.h) and flags nothing."""
    blocks = [m for m in model.modules() if isinstance(m, Bottleneck)]
    if enable and blocks and not SF.planes_supported():
        import warnings
        warnings.warn("route_teacher_planes: this back-end lacks the piece-plane entries (include/skd_planes.h); the teacher "
                      "keeps its fp32 link between conv1 and conv2", RuntimeWarning, stacklevel=2)
        enable = False
    for m in blocks:
        if enable:
            m._skd_teacher_planes = True
        else:
            vars(m).pop("_skd_teacher_planes", None)
    return model


def set_teacher_pieces(model, pieces=2, piece_format="bf16"):
    """Mark ``model`` (a frozen Bottleneck network: the teacher) for ``pieces`` pieces per operand, of ``piece_format``, on the
    split core and return it.

    ``pieces=2`` -- an ACCURACY trade, opt-in: every call of the network that runs on the split core today takes the two-piece
    entries of include/skd_split2.h (three bf16 products instead of six): the Bottlenecks' reduce and stride-1 down-sample 1x1 GEMMs
    (_conv1x1_bn_eval), their fused tails, their routed 3x3 convolutions (_split_conv), the ResNet's dsn[0] and the feature half of
    the PSP bottleneck -- except the shapes of SPLIT2_ROUTING_EXCLUDED.  The outputs move by about 1.5e-5 of their largest magnitude
    (profiles/r25_split2_accuracy.md; three pieces: 1e-6).  The marks sit on the Bottlenecks, the ResNet and the PSPModule;
    BasicBlocks (the student), the 64-column form, anything under grad or in training mode, the library GEMM for 512 -> 128, the
    PSP fold's matrix products and the heads are what they were.  Call it before the network's first forward, warm-up step or
    graph capture, so that the two-plane packs are made eagerly.
    ``pieces=2, piece_format="fp16"`` -- opt-in, NOT an accuracy trade: the same modules are marked and the same call sites take the
    entries of include/skd_split2h.h instead -- two FP16 pieces with the residual scaled by 2^11, the same three products: 22
    significant bits per operand, the three-piece accuracy -- except the shapes of SPLIT2H_ROUTING_EXCLUDED.  The
    stride-2 and 64-column forms are not routed to fp16 pieces for the teacher (their fp16 twins, include/skd_infer2h.h, serve the
    student's inference form alone; the piece-plane form has none): under this mark they run on THREE bf16 pieces, never on two.
    An activation beyond +-65504 gives NaN outputs (the header's range contract).  ``piece_format`` without ``pieces=2`` is a
    ValueError, not a silent three-piece run.
    ``pieces=3`` clears the marks and drops the two-plane packs of both formats.  On a back-end without the entries ``pieces=2``
    warns (RuntimeWarning) and leaves three pieces."""
    SF.check_pieces(pieces, piece_format)
    if pieces == 2 and not SF.split2_supported(piece_format):
        import warnings
        warnings.warn("set_teacher_pieces: this back-end lacks the two-piece entries (include/%s); the teacher stays on "
                      "three pieces" % ("skd_split2h.h" if piece_format == "fp16" else "skd_split2.h"), RuntimeWarning, stacklevel=2)
        pieces = 3
    teacher = any(isinstance(m, Bottleneck) for m in model.modules())      # a BasicBlock network (the student) is left untouched
    for m in model.modules():
        if not isinstance(m, (Bottleneck, ResNet, PSPModule)):
            continue
        if pieces == 2:
            if teacher:
                m._skd_teacher_pieces = 2
                if piece_format == "fp16":
                    m._skd_teacher_piece_format = "fp16"
                else:
                    vars(m).pop("_skd_teacher_piece_format", None)
            continue
        vars(m).pop("_skd_teacher_pieces", None)
        vars(m).pop("_skd_teacher_piece_format", None)
        owners = ((m.conv2,) if isinstance(m, Bottleneck) else (m.dsn[0],) if isinstance(m, ResNet) else (getattr(m, "_fold_cache", {}),))
        for owner in owners:
            slot = owner if isinstance(owner, dict) else vars(owner)
            for attr in ("_skd_conv3x3_pack2", "pack3x3_2", "_skd_conv3x3_pack2h", "pack3x3_2h"):
                slot.pop(attr, None)
    return model


def route_training_convs(model, enable=True, min_cin=TRAIN_SPLIT_MIN_CIN, wgrad=False, narrow=False, narrow_wgrad=False,
                         shortcut=False, bnstats=False, pieces=3, piece_format="bf16"):
    """Flag ``model`` (the student) for the training form of its 3x3 convolutions and return ``model``.

    A flagged module in training mode, with grad enabled, on an fp32 channels-last device input runs ``BasicBlock.conv1`` /
    ``conv2``, the deep-supervision head's ``dsn[0]`` (bias in the epilogue) and the feature-map half of the PSP bottleneck on the
    split core of csrc/conv3x3.hip, forward and data gradient (SF.conv3x3_split_train), wherever both directions fit the kernel
    and the convolution has at least ``min_cin`` input channels (TRAIN_SPLIT_MIN_CIN above); the weight gradients, every other
    convolution, everything around these calls (forward_relu, the residual, dropout, the fold) and every eval-mode or no-grad
    forward are what they were.  The weights are split once per weight version, i.e. once per optimizer step, in the forward.
    The version is autograd's ``_version``: an optimizer that writes the weights without advancing it -- torch's FUSED
    multi-tensor optimizers -- needs ``kd_model.advance_versions_after_step`` as a step post-hook (NetModel registers it), or the
    next forward runs on the packs of the old weights.
    ``wgrad=True``: the weight gradients of the routed convolutions run on the split core as well (SF.conv3x3_split_wgrad,
    csrc/conv3x3_wgrad.hip) except for the shapes of WGRAD_ROUTING_EXCLUDED; on a back-end without the entries of
    include/skd_wgrad.h they stay with the library.
    ``narrow=True``: the stem's conv2 / conv3 and layer1's four convolutions too (SF.conv3x3_split_train with ``narrow=True``: each
    direction on the 128-column form of the kernel where its N is a multiple of 128, on the 64-column one otherwise; their weight gradients
    stay with the library) except for the shapes of NARROW_ROUTING_EXCLUDED.
    ``narrow_wgrad=True``: the weight gradients of the convolutions ``narrow`` routes run on the split core as well
    (SF.conv3x3_narrow_wgrad, the 128 x 64 form of csrc/conv3x3_wgrad.hip) except for the shapes of NARROW_WGRAD_ROUTING_EXCLUDED;
    without ``narrow`` it routes nothing, and on a back-end without the entries of include/skd_narrow_wgrad.h they stay with the library.
    ``shortcut=True``: the 1x1 down-sample convolutions of the BasicBlocks (layer1.0 to layer4.0: stride 1 or 2, followed by an
    ABN) run forward, data gradient and weight gradient on the split core as well (SF.conv1x1_split_train, include/skd_shortcut.h)
    except for the (Cin, Cout, stride, product) of SHORTCUT_ROUTING_EXCLUDED; on a back-end without the entries they stay with the
    library.  It does not depend on the other three.
    ``bnstats=True``: a BasicBlock's routed conv1 / conv2 (the 11 wide ones of layer2-4; with ``narrow`` layer1's four) also emits
    the batch-norm statistics of its output from the epilogue (SF.conv3x3_split_train with ``stats=True``, include/skd_bnstats.h) and
    the forward_relu behind it finishes them and applies, except for the shapes of BNSTATS_ROUTING_EXCLUDED; replicated
    (synchronised) normalisations, dsn[0], the stem, the PSP bottleneck and the shortcuts are what they were, and so are the
    convolution's output bits and every backward.  On a back-end without the entries nothing changes.
    ``pieces=2`` -- an ACCURACY trade, opt-in: the 13 WIDE convolutions (layer2.0.conv2 to layer4, dsn[0], the feature half of the
    PSP bottleneck) run forward and data gradient on two bf16 pieces per operand and three products (include/skd_train2.h,
    SF.conv3x3_split_train2: skd_conv3x3_split2_nhwc on the two-plane pack pair), and with ``wgrad`` their weight gradients too
    (SF.conv3x3_split_wgrad2, the two-piece form of csrc/conv3x3_wgrad.hip) except for the shapes of WGRAD_ROUTING_EXCLUDED,
    whose weight gradients stay with the library; the shapes of STUDENT_PIECES_ROUTING_EXCLUDED keep three pieces.  16 significant bits per operand: every output element within
    2^-15 of the sum of absolute products of the exact result (profiles/r33_student_pieces_accuracy.md).  These keep three
    pieces, or the library, whatever ``pieces`` says: the 64-column forms of ``narrow`` and their weight gradients; the 1x1
    shortcut convolutions of ``shortcut``; a convolution that writes statistics (``bnstats``); every stride-2 convolution.  On a
    back-end without the entries the student stays on three pieces.  Anything but the integers 2 and 3 is a ValueError.
    ``pieces=2, piece_format="fp16"`` -- opt-in, NOT an accuracy trade (include/skd_train2h.h): the same 13
    convolutions on two FP16 pieces per operand with the residual scaled by 2^11 and three products, 22 significant bits per
    operand (SF.conv3x3_split_train_fp16, SF.ppm_fold_bottleneck_train_fp16).  The forward runs skd_conv3x3_split2h_nhwc; the
    backward finds a power-of-two scale of the output gradient on the device (SF.fp16_scale_word, once per convolution) and hands
    it to the scaled data gradient and, with ``wgrad``, to SF.conv3x3_split_wgrad_fp16, so gradients far below fp16's range lose
    nothing.  ``x`` and the weights are not scaled: an activation or a weight beyond +-65504 gives NaN (skd_split2h.h's loud
    contract).  The shapes of STUDENT_FP16_ROUTING_EXCLUDED keep THREE pieces, never two bf16 ones, and so does everything
    ``pieces=2`` leaves on three.  The mark (``_skd_train_piece_format``) is its own; a module never carries it together with
    ``_skd_train_pieces``.  "fp16" with ``pieces=3`` and anything but "bf16" / "fp16" are ValueErrors; on a back-end without
    the entries it warns once (RuntimeWarning, naming skd_train2h.h) and the student stays on three pieces.  The default "bf16"
    changes nothing.
    ``enable=False`` clears the flags and drops the packs.  On a back-end without the entries (the tests' C double) the flag is
    set and changes nothing."""
    SF.check_pieces(pieces, piece_format)
    fp16 = bool(enable) and piece_format == "fp16"
    if fp16 and not SF.train2h_supported():
        import warnings
        warnings.warn("route_training_convs: this back-end lacks the fp16 training entries (include/skd_train2h.h); the student "
                      "stays on three pieces", RuntimeWarning, stacklevel=2)
        fp16, pieces = False, 3
    for m in model.modules():
        if not isinstance(m, (BasicBlock, ResNet, PSPModule)):
            continue
        m._skd_train_min_cin = int(min_cin) if enable else None
        m._skd_train_wgrad = bool(wgrad and enable)
        m._skd_train_narrow = bool(narrow and enable)
        m._skd_train_narrow_wgrad = bool(narrow_wgrad and enable)
        if enable and pieces == 2 and not fp16:
            m._skd_train_pieces = 2
        else:
            vars(m).pop("_skd_train_pieces", None)
        if fp16:
            m._skd_train_piece_format = "fp16"
        else:
            vars(m).pop("_skd_train_piece_format", None)
        if isinstance(m, BasicBlock):
            m._skd_train_shortcut = bool(shortcut and enable)
            m._skd_train_bnstats = bool(bnstats and enable)
        if enable:
            continue
        if isinstance(m, BasicBlock) and isinstance(m.downsample, nn.Sequential) and len(m.downsample):
            SF.drop_conv1x1_train_mats(m.downsample[0])
        owners = ((m.conv1, m.conv2) if isinstance(m, BasicBlock) else (m.dsn[0], m.conv2, m.conv3) if isinstance(m, ResNet)
                  else (getattr(m, "_fold_cache", {}),))
        for owner in owners:
            SF.drop_conv3x3_packs(owner)
    return model
