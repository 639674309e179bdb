"""ctypes binding of libskd_hip.so (the C ABI declared in the headers of include/).

Replaces the reference's cffi shim (libs/_ext/__init__.py + libs/src/lib_cffi.cpp, which unwrap
THCudaTensor*): here the Python side passes raw device pointers (``tensor.data_ptr()``) and the
current HIP stream.  There is NO fallback: if the shared library is missing or a symbol cannot
be resolved, every op raises -- a GPU box must never silently run an eager substitute.

The registry is ``ABI``: one ``{name: (restype, argtypes)}`` table per header of include/, keyed by the header's base name,
in the order the headers were added.  ``skd.h`` is the core (``SIGNATURES``): the plain-C double of oracle/ is typed from it
and has exactly its entries.  Every other header is an extension: the double lacks its entries, so a caller that needs one
asks ``has_entry()`` first.  A new feature adds one header to include/ and one table to ``ABI``; tests/test_abi.py checks
header <-> table <-> exported symbols for every key, with nothing else to edit.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libskd_hip.so")
INCLUDE_DIR = os.path.normpath(os.path.join(_HERE, "..", "include"))
HEADER_PATH = os.path.join(INCLUDE_DIR, "skd.h")

_c = ctypes
_P = _c.c_void_p
_I = _c.c_int
_L = _c.c_int64
_F = _c.c_float
_D = _c.c_double

# name -> (restype, argtypes) per header.  include/skd.h: the core ABI, every csrc/*.hip file not named below.
ABI = {}
ABI["skd.h"] = {
    "skd_abi_version": (_I, []),
    "skd_target_arch": (_I, []),
    "skd_bn_mean_var": (_I, [_I, _I, _I, _P, _P, _P, _P]),
    "skd_bn_forward": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _F, _P]),
    "skd_bn_edz_eydz": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _F, _P]),
    "skd_bn_backward": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _F, _P]),
    "skd_leaky_relu": (_I, [_L, _P, _F, _P]),
    "skd_leaky_relu_backward": (_I, [_L, _P, _P, _F, _P]),
    "skd_elu": (_I, [_L, _P, _P]),
    "skd_elu_backward": (_I, [_L, _P, _P, _P]),
    "skd_elu_inv": (_I, [_L, _P, _P]),
    "skd_abn_workspace_floats": (_L, [_I, _I, _I]),
    "skd_abn_forward_train": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _F, _F, _I, _F, _P, _P]),
    "skd_abn_stats": (_I, [_I, _I, _I, _P, _P, _P, _P, _P]),
    "skd_abn_apply": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _F, _I, _F, _P]),
    "skd_abn_apply_residual": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _F, _I, _F, _P]),
    "skd_abn_apply_to": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _F, _I, _F, _P]),
    "skd_abn_forward_train_to": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _F, _F, _I, _F, _P, _P]),
    "skd_abn_relu_backward_reduce": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _F, _P, _P]),
    "skd_abn_relu_backward_dx": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _F, _P]),
    "skd_abn_apply_nhwc": (_I, [_L, _I, _P, _P, _P, _P, _P, _P, _F, _I, _F, _P]),
    "skd_abn_nhwc_workspace_floats": (_L, [_L, _I]),
    "skd_abn_stats_nhwc": (_I, [_L, _I, _P, _P, _P, _P, _P]),
    "skd_abn_apply_nhwc_to": (_I, [_L, _I, _P, _P, _P, _P, _P, _P, _P, _F, _I, _F, _P]),
    "skd_abn_forward_train_nhwc": (_I, [_L, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _F, _F, _I, _F, _P, _P]),
    "skd_abn_backward_reduce_nhwc": (_I, [_L, _I, _P, _P, _P, _P, _P, _P, _F, _I, _F, _P, _P]),
    "skd_abn_backward_dx_nhwc": (_I, [_L, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _F, _I, _F, _I, _P]),
    "skd_abn_relu_backward_reduce_nhwc": (_I, [_L, _I, _P, _P, _P, _P, _P, _P, _P, _F, _P, _P]),
    "skd_abn_relu_backward_reduce_nhwc_x": (_I, [_L, _I, _P, _P, _P, _P, _P, _P, _P, _P, _F, _P, _P]),
    "skd_abn_relu_backward_dx_nhwc_x": (_I, [_L, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _F, _I, _P]),
    "skd_abn_backward_nhwc": (_I, [_L, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _F, _I, _F, _I, _P, _P]),
    "skd_abn_relu_backward_nhwc": (_I, [_L, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _F, _I, _P, _P]),
    "skd_abn_relu_backward_dx_nhwc": (_I, [_L, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _F, _I, _P]),
    "skd_abn_combine_stats": (_I, [_I, _I, _P, _P, _I, _P, _P, _P, _P, _F, _D, _P]),
    "skd_abn_update_running": (_I, [_I, _P, _P, _P, _P, _F, _D, _P]),
    "skd_abn_backward_reduce": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _F, _I, _F, _P, _P]),
    "skd_abn_backward_dx": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _F, _I, _F, _P]),
    "skd_abn_backward": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _F, _I, _F, _I, _P, _P]),
    "skd_pixelwise_workspace_floats": (_L, [_I, _I]),
    "skd_pixelwise_loss": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "skd_maxpool_argmax": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "skd_pairwise_ldm": (_I, [_I]),
    "skd_channel_l2_normalise": (_I, [_I, _I, _I, _P, _P, _I, _P, _I, _P, _P]),
    "skd_pairwise_workspace_floats": (_L, [_I, _I]),
    "skd_pairwise_gram_loss": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "skd_pairwise_backward_workspace_floats": (_L, [_I, _I, _I]),
    "skd_pairwise_backward": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "skd_maxunpool_scatter": (_I, [_I, _I, _I, _I, _I, _P, _L, _P, _P, _P]),
    "skd_maxpool_argmax_nhwc": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "skd_maxunpool_scatter_nhwc": (_I, [_I, _I, _I, _I, _I, _I, _P, _L, _P, _P, _P]),
    "skd_spectral_workspace_floats": (_L, [_I, _I]),
    "skd_spectral_norm_forward": (_I, [_I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "skd_spectral_norm_backward": (_I, [_I, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
    "skd_spectral_norm_forward_multi": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "skd_spectral_norm_backward_multi": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "skd_ce_dsn_workspace_floats": (_L, [_I, _I, _I, _I, _I, _I]),
    "skd_ce_dsn_forward": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _I, _F, _P, _P, _P, _P, _P]),
    "skd_ppm_pooled_floats": (_L, [_I, _I, _P]),
    "skd_ppm_pool": (_I, [_I, _I, _I, _I, _P, _P, _P, _P]),
    "skd_ppm_pool_backward": (_I, [_I, _I, _I, _I, _P, _P, _P, _P]),
    "skd_ppm_concat": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "skd_ppm_concat_backward": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "skd_conv1x1_abn_supported": (_I, [_L, _I, _I]),
    "skd_conv1x1_abn_nhwc": (_I, [_L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _F, _I, _F, _P]),
    "skd_abn_pack_eval_params": (_I, [_I, _P, _P, _P, _P, _F, _P, _P]),
    "skd_conv1x1_abn_pro_nhwc": (_I, [_L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _F, _P, _I, _F, _P]),
    "skd_pairwise_small": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "skd_cs_transform": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _I, _P, _I, _P, _P]),
    "skd_ppm_nhwc_workspace_floats": (_L, [_I, _I, _I, _I, _I, _I, _P]),
    "skd_ppm_pool_nhwc": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "skd_ppm_pool_backward_nhwc": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "skd_ppm_concat_nhwc": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "skd_ppm_concat_backward_nhwc": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "skd_ppm_fold_nhwc_workspace_floats": (_L, [_I, _I, _I, _I, _I, _P]),
    "skd_ppm_fold_nhwc": (_I, [_I, _I, _I, _I, _I, _P, _P, _L, _P, _P]),
    "skd_ppm_fold_backward_nhwc": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _L, _P, _P]),
    "skd_maxpool3x3s2_nhwc": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "skd_head1x1_supported": (_I, [_I, _I, _I]),
    "skd_head1x1_forward_nhwc": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "skd_head1x1_backward_workspace_floats": (_L, [_I, _I, _I, _I]),
    "skd_head1x1_backward_nhwc": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
    "skd_maxpool3x3s2_backward_nhwc": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "skd_abn_relu_maxpool3x3s2_nhwc": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _F, _P, _P, _P]),
    "skd_abn_relu_maxpool3x3s2_backward_reduce_nhwc": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _F, _P, _P]),
    "skd_abn_relu_maxpool3x3s2_backward_dx_nhwc": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _F,
                                                         _I, _P]),
    "skd_seg_confusion": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _I, _P, _P, _P]),
    "skd_sum_f32": (_I, [_L, _P, _P, _F, _P, _P]),
    "skd_sync_handle_bytes": (_I, []),
    "skd_sync_max_floats": (_I, []),
    "skd_sync_create": (_P, [_I, _I, _P]),
    "skd_sync_connect": (_I, [_P, _P]),
    "skd_sync_destroy": (_I, [_P]),
    "skd_sync_all_gather": (_I, [_P, _I, _P, _P, _P]),
    "skd_abn_sync_stats": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _F, _D, _P]),
    "skd_abn_sync_grad_stats": (_I, [_P, _I, _P, _P, _P]),
    "skd_sync_set_timeout": (_I, [_P, _D]),
    "skd_abn_forward_train_nhwc_sync": (_I, [_P, _L, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _F, _F, _I, _F, _D, _P, _P]),
    "skd_abn_backward_nhwc_sync": (_I, [_P, _L, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _F, _I, _F, _I, _P, _P]),
    "skd_abn_relu_backward_nhwc_sync": (_I, [_P, _L, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _F, _I, _P, _P]),
    "skd_status_words": (_I, []),
    "skd_status_read": (_I, [_P]),
    "skd_status_clear": (_I, []),
    "skd_abn_set_fused_max_workgroups": (_I, [_I]),
    "skd_abn_set_fused": (_I, [_I]),
    "skd_abn_get_fused": (_I, []),
    "skd_abn_set_sync_fused": (_I, [_I]),
    "skd_abn_get_sync_fused": (_I, []),
    "skd_abn_sync_form_counts": (_I, [_P]),
}

# include/skd_eval.h (csrc/evaluate_sliding.hip, csrc/conv3x3.hip, csrc/conv1x1.hip): sliding-window evaluation, the frozen split
# 3x3 convolution and the split GEMM's geometry queries.  The ops that need them raise on a back-end without them.
ABI["skd_eval.h"] = {
    "skd_seg_sliding": (_I, [_I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _I, _P, _P, _P, _P, _P]),
    "skd_conv3x3_split_supported": (_I, [_I, _I, _I, _I, _I, _I]),
    "skd_conv3x3_split_pack_bytes": (_L, [_I, _I]),
    "skd_conv3x3_split_pack_weights": (_I, [_I, _I, _P, _L, _L, _L, _L, _P, _L, _P]),
    "skd_conv3x3_split_nhwc": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _F, _I, _F, _I, _P]),
    "skd_conv1x1_abn_geometry": (_I, [_L, _I, _I, _I, _P]),
    "skd_conv1x1_abn_tile_of": (_I, [_L, _I, _I, _I, _L, _L, _P]),
}

# include/skd_eval_ms.h (csrc/evaluate_multiscale.hip): multi-scale and flip evaluation.
ABI["skd_eval_ms.h"] = {
    "skd_zoom_linear": (_I, [_I, _I, _I, _I, _I, _P, _P, _I, _I, _P]),
    "skd_seg_multiscale": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _I, _P, _P, _P, _P, _P]),
}

# include/skd_ohem.h (csrc/ce_ohem.hip): the OHEM criterion.
ABI["skd_ohem.h"] = {
    "skd_ce_ohem_workspace_floats": (_L, [_I, _I, _I, _I, _I, _I, _I]),
    "skd_ohem_threshold": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _I, _F, _I, _I, _P, _P, _P, _P, _P]),
    "skd_ce_ohem_dsn_forward": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _I, _F, _P, _P, _P, _P, _P, _P, _P, _P]),
}

# include/skd_infer.h (csrc/conv3x3.hip): the student's fused inference path.  A back-end without them leaves the BasicBlocks on
# the op sequence they ran before: nothing raises.
ABI["skd_infer.h"] = {
    "skd_conv3x3_split_res_nhwc": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _F, _I, _F, _I, _P]),
}

# include/skd_train.h (csrc/conv3x3.hip): the training student's 3x3 convolutions on the split core.  A back-end without them
# leaves the student's convolutions on the library: nothing raises.
ABI["skd_train.h"] = {
    "skd_conv3x3_split_train_supported": (_I, [_I, _I, _I, _I, _I, _I]),
    "skd_conv3x3_split_pack_pair": (_I, [_I, _I, _P, _L, _L, _L, _L, _P, _L, _P, _L, _P]),
}

# include/skd_wgrad.h (csrc/conv3x3_wgrad.hip): the weight gradient of those convolutions on the split core.  A back-end without
# them leaves the weight gradients on the library: nothing raises.
ABI["skd_wgrad.h"] = {
    "skd_conv3x3_split_wgrad_supported": (_I, [_I, _I, _I, _I, _I, _I]),
    "skd_conv3x3_split_wgrad_plan": (_I, [_I, _I, _I, _I, _I, _I, _I, _P]),
    "skd_conv3x3_split_wgrad_nhwc": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _L, _L, _L, _L, _P, _L, _I, _P]),
}

# include/skd_narrow.h (csrc/conv3x3.hip): the 64-column form of the split-core 3x3 convolution.  A back-end without them leaves
# the 64-channel convolutions where they were: nothing raises.
ABI["skd_narrow.h"] = {
    "skd_conv3x3_narrow_supported": (_I, [_I, _I, _I, _I, _I, _I]),
    "skd_conv3x3_narrow_pack_bytes": (_L, [_I, _I]),
    "skd_conv3x3_narrow_pack_pair": (_I, [_I, _I, _P, _L, _L, _L, _L, _P, _L, _P, _L, _P]),
    "skd_conv3x3_narrow_nhwc": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _F, _I, _F, _I, _P]),
}

# include/skd_narrow_wgrad.h (csrc/conv3x3_wgrad.hip, the 128 x 64 tile form): the weight gradient of the convolutions with a
# 64-channel side.  A back-end without them leaves those weight gradients on the library: nothing raises.
ABI["skd_narrow_wgrad.h"] = {
    "skd_conv3x3_narrow_wgrad_supported": (_I, [_I, _I, _I, _I, _I, _I]),
    "skd_conv3x3_narrow_wgrad_plan": (_I, [_I, _I, _I, _I, _I, _I, _I, _P]),
    "skd_conv3x3_narrow_wgrad_nhwc": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _L, _L, _L, _L, _P, _L, _I, _P]),
}

# include/skd_shortcut.h (csrc/conv1x1_train.hip; the weight gradient: csrc/conv3x3_wgrad.hip, its one-tap form): the training
# student's 1x1 down-sample convolutions on the split core.  A back-end without them leaves them on the library: nothing raises.
ABI["skd_shortcut.h"] = {
    "skd_conv1x1_train_supported": (_I, [_I, _I, _I, _I, _I, _I, _I]),
    "skd_conv1x1_train_fwd_nhwc": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "skd_conv1x1_train_fwd_cols64_nhwc": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "skd_conv1x1_train_dgrad_nhwc": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "skd_conv1x1_train_dgrad_cols64_nhwc": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "skd_conv1x1_train_wgrad_plan": (_I, [_I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "skd_conv1x1_train_wgrad_nhwc": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _L, _I, _P]),
}

# include/skd_split2.h (csrc/conv3x3.hip, csrc/conv1x1.hip with two pieces per operand): the frozen teacher's reduced-precision
# mode.  A back-end without them leaves the teacher on three pieces (pspnet_combine.set_teacher_pieces warns): nothing raises.
ABI["skd_split2.h"] = {
    "skd_conv3x3_split2_pack_bytes": (_L, [_I, _I]),
    "skd_conv3x3_split2_pack_weights": (_I, [_I, _I, _P, _L, _L, _L, _L, _P, _L, _P]),
    "skd_conv3x3_split2_nhwc": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _F, _I, _F, _I, _P]),
    "skd_conv1x1_abn2_nhwc": (_I, [_L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _F, _I, _F, _P]),
    "skd_conv1x1_abn2_pro_nhwc": (_I, [_L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _F, _P, _I, _F, _P]),
}

# include/skd_bnstats.h (csrc/conv3x3.hip with STATS, csrc/abn_nhwc.hip): the student's training 3x3 forward with the batch-norm
# statistics records from its epilogue, and their finalize.  A back-end without them leaves the convolutions and the ABN forward
# behind them where they were: nothing raises.
ABI["skd_bnstats.h"] = {
    "skd_conv3x3_bnstats_floats": (_L, [_L, _I]),
    "skd_conv3x3_split_stats_nhwc": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P, _L, _P]),
    "skd_conv3x3_narrow_stats_nhwc": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P, _L, _P]),
    "skd_abn_stats_from_partials_nhwc": (_I, [_L, _I, _P, _L, _P, _P, _P, _P, _F, _P]),
}

# include/skd_stride2.h (csrc/conv3x3.hip with STRIDE = 2): the stride-2 frozen forward of the 128-column 3x3 family.  A back-end
# without them leaves those convolutions on the library: nothing raises.
ABI["skd_stride2.h"] = {
    "skd_conv3x3_split_s2_supported": (_I, [_I, _I, _I, _I, _I, _I]),
    "skd_conv3x3_split_s2_taps": (_I, [_I, _I, _L, _P, _P]),
    "skd_conv3x3_split_s2_nhwc": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _F, _I, _F, _I, _I, _P]),
}

# include/skd_pairwise_split.h (csrc/pairwise_split.hip): the pair-wise loss's Gram + loss and backward product on the split core,
# twins of skd_pairwise_gram_loss / skd_pairwise_backward.  A back-end without them leaves the loss on the fp32 kernels (kd_model
# warns when the switch asks for them): nothing raises.
ABI["skd_pairwise_split.h"] = {
    "skd_pairwise_split_workspace_floats": (_L, [_I, _I, _I, _I]),
    "skd_pairwise_split_gram_loss": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "skd_pairwise_split_backward_workspace_floats": (_L, [_I, _I, _I]),
    "skd_pairwise_split_backward": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
}

# include/skd_planes.h (csrc/planes.hip, csrc/conv1x1.hip and csrc/conv3x3.hip with PLANES): piece planes, an activation map handed
# from the frozen teacher's split reduce GEMM to its 3x3 convolution as three bf16 pieces.  A back-end without them leaves the
# teacher's link on fp32 (kd_model warns when the switch asks for them): nothing raises.
ABI["skd_planes.h"] = {
    "skd_planes_supported": (_I, [_I]),
    "skd_planes_bytes": (_I, [_L, _I, _P]),
    "skd_planes_offset": (_I, [_L, _I, _L, _I, _I, _P]),
    "skd_planes_split_nhwc": (_I, [_L, _I, _P, _P, _P]),
    "skd_planes_join_nhwc": (_I, [_L, _I, _P, _P, _P]),
    "skd_conv1x1_abn_planes_nhwc": (_I, [_L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _F, _I, _F, _P]),
    "skd_conv3x3_split_planes_nhwc": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _F, _I, _F, _I, _I, _P]),
}

# include/skd_split2h.h (csrc/conv3x3.hip, csrc/conv1x1.hip with two FP16 pieces per operand and a scaled residual): the frozen
# teacher's two-piece mode at the three-piece accuracy, twins of skd_split2.h.  A back-end without them leaves the teacher on three
# pieces (pspnet_combine.set_teacher_pieces warns): nothing raises.
ABI["skd_split2h.h"] = {
    "skd_conv3x3_split2h_pack_bytes": (_L, [_I, _I]),
    "skd_conv3x3_split2h_pack_weights": (_I, [_I, _I, _P, _L, _L, _L, _L, _P, _L, _P]),
    "skd_conv3x3_split2h_nhwc": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _F, _I, _F, _I, _P]),
    "skd_conv1x1_abn2h_nhwc": (_I, [_L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _F, _I, _F, _P]),
    "skd_conv1x1_abn2h_pro_nhwc": (_I, [_L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _F, _P, _I, _F, _P]),
}

# include/skd_train2.h (csrc/conv3x3.hip, csrc/conv3x3_wgrad.hip with two pieces per operand): the training student's wide 3x3
# convolutions at reduced precision, twins of skd_train.h / skd_wgrad.h.  A back-end without them leaves the student on three
# pieces (route_training_convs(pieces=2) then routes the three-piece ops; the two-piece ops themselves raise NotImplementedError).
ABI["skd_train2.h"] = {
    "skd_conv3x3_split2_pack_pair": (_I, [_I, _I, _P, _L, _L, _L, _L, _P, _L, _P, _L, _P]),
    "skd_conv3x3_split2_wgrad_plan": (_I, [_I, _I, _I, _I, _I, _I, _I, _P]),
    "skd_conv3x3_split2_wgrad_nhwc": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _L, _L, _L, _L, _P, _L, _I, _P]),
}

# include/skd_infer2h.h (csrc/conv3x3.hip's residual-epilogue, 64-column and stride-2 forms with two FP16 pieces per operand): the
# student's fused inference form at three products per K-step and the three-piece accuracy, twins of skd_infer.h / skd_narrow.h /
# skd_stride2.h.  A back-end without them leaves the student on three bf16 pieces (pspnet_combine.fuse_for_inference warns; the
# fp16 ops themselves raise NotImplementedError).
ABI["skd_infer2h.h"] = {
    "skd_conv3x3_split2h_res_nhwc": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _F, _I, _F, _I, _P]),
    "skd_conv3x3_narrow2h_pack_bytes": (_L, [_I, _I]),
    "skd_conv3x3_narrow2h_pack_weights": (_I, [_I, _I, _P, _L, _L, _L, _L, _P, _L, _P]),
    "skd_conv3x3_narrow2h_nhwc": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _F, _I, _F, _I, _P]),
    "skd_conv3x3_split2h_s2_nhwc": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _F, _I, _F, _I, _P]),
}

# include/skd_train2h.h (csrc/scale_word.hip, csrc/conv3x3.hip's SCALED form, csrc/conv3x3_wgrad.hip with FMT = kFp16): the training
# student's wide 3x3 convolutions on two FP16 pieces per operand with a power-of-two scale per gradient tensor, found on the
# device -- twins of skd_train2.h / skd_split2h.h plus the scale word.  A back-end without them leaves the student on three bf16
# pieces (route_training_convs(piece_format="fp16") warns once; the fp16 training ops themselves raise NotImplementedError).
ABI["skd_train2h.h"] = {
    "skd_fp16_scale_word_workspace_bytes": (_L, [_L]),
    "skd_fp16_scale_word": (_I, [_L, _P, _P, _L, _P, _P]),
    "skd_conv3x3_split2h_pack_pair": (_I, [_I, _I, _P, _L, _L, _L, _L, _P, _L, _P, _L, _P]),
    "skd_conv3x3_split2h_scaled_nhwc": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P]),
    "skd_conv3x3_split2h_wgrad_plan": (_I, [_I, _I, _I, _I, _I, _I, _I, _P]),
    "skd_conv3x3_split2h_wgrad_nhwc": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _L, _L, _L, _L, _P, _L, _P, _I, _P]),
}

SIGNATURES = ABI["skd.h"]    # the core ABI: what the plain-C double of oracle/ is typed from

_lib = None
_test_backend = None  # see install_test_backend()


class SkdLibraryError(RuntimeError):
    pass


def header_path(header):
    """Path of the header ``header`` (a key of ``ABI``) in include/."""
    return os.path.join(INCLUDE_DIR, header)


def signature(name):
    """(restype, argtypes) of the entry ``name``, whichever header declares it (names are disjoint across headers)."""
    for table in ABI.values():
        if name in table:
            return table[name]
    raise KeyError(name)


def _header_text(path):
    with open(path) as fh:
        return re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)


def header_prototypes(path=HEADER_PATH):
    """Names of all functions declared in the header at ``path`` (used by tests/test_abi.py)."""
    return sorted(set(re.findall(r"\b(skd_[a-z0-9_]+)\s*\(", _header_text(path))))


def header_arg_counts(path=HEADER_PATH):
    """{name: number of arguments} of the prototypes in the header at ``path`` (used by tests/test_abi.py)."""
    counts = {}
    for m in re.finditer(r"\b(skd_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", _header_text(path), flags=re.S):
        args = m.group(2).strip()
        counts[m.group(1)] = 0 if args in ("", "void") else args.count(",") + 1
    return counts


def load(path=None):
    """dlopen libskd_hip.so and type every entry point.  Raises SkdLibraryError when absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise SkdLibraryError(
            "libskd_hip.so not found at %s -- build it with "
            "`python -m structure_knowledge_distillation_amd.build` (there is no CPU/eager fallback)" % path)
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:  # pragma: no cover
        raise SkdLibraryError("cannot load %s: %s" % (path, e))
    for table in ABI.values():
        for name, (res, args) in table.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                raise SkdLibraryError("libskd_hip.so does not export %s (stale build?)" % name)
            fn.restype = res
            fn.argtypes = args
    if path == LIB_PATH:
        _lib = lib
    return lib


def get():
    """The library object the ops call into (the HIP library, or a test double)."""
    if _test_backend is not None:
        return _test_backend
    if _timing is not None:
        return _TimedLib(load())
    return load()


def has_entry(name):
    """Whether the active back-end (the HIP library, or a test double) provides the extension entry ``name``."""
    return hasattr(get(), name)


# ---- optional per-entry HIP-event timing (bench.py's roofline leg) ---------------------------------
_timing = None


class _TimedLib:
    """Brackets the selected C-ABI calls with HIP events recorded on the stream the kernels are
    launched on (torch's current stream, the `stream` argument every op passes)."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        rec = _timing.get(name) if _timing is not None else None
        if rec is None:
            return fn
        import torch

        def timed(*args):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*args)
            e1.record()
            rec.append((e0, e1, args[:4]))
            return r
        return timed


def enable_kernel_timing(names):
    """Start collecting (start event, end event, first four args) for every call of ``names``."""
    global _timing
    _timing = {n: [] for n in names}


def disable_kernel_timing():
    """Stop collecting; returns {name: [(ms, first four args), ...]} (synchronises the device)."""
    global _timing
    import torch
    out = {}
    if _timing is not None:
        torch.cuda.synchronize()
        for n, recs in _timing.items():
            out[n] = [(e0.elapsed_time(e1), dims) for e0, e1, dims in recs]
    _timing = None
    return out


def install_test_backend(backend):
    """TEST HOOK ONLY: route the C-ABI calls to ``backend`` (an object exposing the same
    functions on HOST pointers).  tests/ uses it to exercise the host-side logic (autograd
    wiring, in-place contract, cross-rank statistics exchange over gloo) on a box without a GPU.
    Product code never calls this; with no backend installed every op requires CUDA tensors."""
    global _test_backend
    _test_backend = backend


def test_backend_active():
    return _test_backend is not None


class SkdDeviceError(RuntimeError):
    """A kernel gave up waiting inside a launch (include/skd.h section 13): its outputs are NaN from there on."""


_STATUS_MEANING = {
    0: "a cross-replica InPlace-ABN exchange timed out waiting for a peer rank (SKD_SYNC_TIMEOUT_S): a rank stalled, died or "
       "called the synchronised layers in a different order; statistics are NaN from that exchange on",
    1: "the grid barrier of a one-launch InPlace-ABN pass timed out: its workgroups were not co-resident (device shared with "
       "another grid-barrier launch, partitioned or CU-masked device) -- set SKD_ABN_FUSED=0 or lower "
       "skd_abn_set_fused_max_workgroups",
}


def device_status():
    """The device-raised error words (no device synchronisation), or None when the buffer does not exist."""
    lib = get()
    n = lib.skd_status_words()
    buf = (ctypes.c_uint * n)()
    if not lib.skd_status_read(ctypes.cast(buf, ctypes.c_void_p)):
        return None
    return list(buf)


def sync_form_counts():
    """(one-launch, three-launch) counts of the synchronised InPlace-ABN calls so far (include/skd.h section 13)."""
    buf = (ctypes.c_int64 * 2)()
    get().skd_abn_sync_form_counts(ctypes.cast(buf, ctypes.c_void_p))
    return int(buf[0]), int(buf[1])


def raise_on_device_errors():
    """Called once per step (NetModel.optimize_parameters) and after a logged scalar has been read back: turns a timed-out
    in-kernel wait into an exception instead of NaN that silently spreads through the gradient all-reduce."""
    words = device_status()
    if words and any(words):
        get().skd_status_clear()
        what = "; ".join("%s (code 0x%08x)" % (_STATUS_MEANING.get(i, "status word %d" % i), w) for i, w in enumerate(words) if w)
        raise SkdDeviceError("structure_knowledge_distillation_amd: " + what)


def check(ok, what):
    """1 = success / 0 = failure, like libs/functions.py:13-16 (_check)."""
    if not ok:
        raise RuntimeError("HIP error encountered in %s" % what)


def ptr(t):
    """Device pointer of a tensor, or NULL for None (lib_cffi.cpp:62-63 convention)."""
    return None if t is None else t.data_ptr()


def int_array(values):
    """Host int[] argument (e.g. the pyramid sizes of skd_ppm_*)."""
    return (ctypes.c_int * len(values))(*[int(v) for v in values])


def ptr_array(tensors):
    """Host array of device pointers (``const float *const *`` arguments)."""
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def stream_of(t):
    """hipStream_t of torch's current stream on t's device (replaces THCState_getCurrentStream)."""
    if _test_backend is not None or not t.is_cuda:
        return None
    import torch
    return torch.cuda.current_stream(t.device).cuda_stream


def require_device(*tensors):
    """Fail loudly instead of falling back when handed CPU tensors (unless a test double is in)."""
    if _test_backend is not None:
        return
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise SkdLibraryError(
                "structure_knowledge_distillation_amd ops run on MI355X only: got a %s tensor "
                "(no CPU fallback exists)" % t.device)
