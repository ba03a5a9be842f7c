"""ctypes binding of librpnet_hip.so (C ABI: include/rpnet_abi.h).

This is the whole FFI surface: plain pointers, ints and a stream.  torch is used only
to own device memory and to give the current HIP stream.  There is NO fallback: if the
library is missing or a call fails, a RuntimeError is raised (the product path never
routes through the CPU oracle).
"""
import ctypes as C
import os

import torch

_LIB_PATH = os.environ.get("RPNET_LIB_PATH") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "librpnet_hip.so")
_lib = None

vp, ci, cf, cs, cd = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_double


class ConvDesc(C.Structure):
    """struct rpnet_conv_desc"""
    _fields_ = [("x0", vp), ("x1", vp), ("C0", ci), ("C1", ci), ("w", vp), ("bias", vp), ("in_scale", vp),
                ("in_scale_mode", ci), ("y0", vp), ("y1", vp), ("Co0", ci), ("Co1", ci), ("ep_scale", vp),
                ("ep_shift", vp), ("ep_relu", ci), ("out_scale", vp), ("out_scale_mode", ci), ("accumulate", ci),
                ("N", ci), ("H", ci), ("W", ci), ("taps", ci), ("upsample", ci), ("groups", ci), ("dilation", ci), ("stats_partial", vp), ("split_planes", ci), ("y_split", vp), ("split_out_planes", ci),
                ("acc_scale_col", vp), ("acc_scale_x", vp), ("acc_scale_dy", vp), ("bnb_y", vp), ("bnb_stats", vp), ("bnb_partial", vp), ("bnb_pmax", vp), ("bnb_groups", ci),
                ("acc_scale_x1", vp), ("out_absmax", vp), ("tune", ci), ("y_split_scale", vp), ("splitk_ws", vp), ("splitk_ws_bytes", cs),
                ("skip_mask", vp), ("skip_mode", ci), ("skip_halo", ci), ("skip_ws", vp), ("tile_skip", vp),
                ("y_enc", vp), ("y_enc_stride", ci)]


PACK_MAX = 24     # layers per rpnet_pack_conv_weights_split call


class PackItem(C.Structure):
    """struct rpnet_pack_item"""
    _fields_ = [("w", vp), ("wp", vp), ("wd", vp), ("row_scale_wp", vp), ("row_scale_wd", vp), ("cout", ci), ("cin", ci),
                ("taps", ci), ("cin_off0", ci), ("cin_split", ci), ("cin_off1", ci), ("cin_pad", ci)]


_SIGS = {
    "rpnet_version": (ci, []),
    "rpnet_last_error_string": (C.c_char_p, []),
    "rpnet_pack_conv_weight": (ci, [vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp]),
    "rpnet_split_bf16": (ci, [vp, vp, ci, vp, cs, ci, ci, vp]),
    "rpnet_split_f16": (ci, [vp, vp, ci, vp, vp, vp, vp, cs, ci, ci, ci, vp]),
    "rpnet_pack_conv_weight_split": (ci, [vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp]),
    "rpnet_pack_conv_weights_split": (ci, [C.POINTER(PackItem), ci, ci, vp]),
    "rpnet_conv_fwd": (ci, [C.POINTER(ConvDesc), vp]),
    "rpnet_upconv_collapse_weights": (ci, [vp, vp, ci, ci, vp]),
    "rpnet_conv_up4_supported": (ci, [C.POINTER(ConvDesc), ci]),
    "rpnet_conv_up4_stats_blocks": (ci, [C.POINTER(ConvDesc)]),
    "rpnet_conv_up4": (ci, [C.POINTER(ConvDesc), ci, vp]),
    "rpnet_conv_wgrad_up4_supported": (ci, [C.POINTER(ConvDesc)]),
    "rpnet_conv_wgrad_up4_workspace_bytes": (cs, [ci, ci, ci, ci, ci]),
    "rpnet_conv_wgrad_up4": (ci, [C.POINTER(ConvDesc), vp, vp, vp, cs, vp]),
    "rpnet_conv_stats_blocks": (ci, [C.POINTER(ConvDesc)]),
    "rpnet_conv_tile_variant": (ci, [C.POINTER(ConvDesc)]),
    "rpnet_conv_splitk_workspace_bytes": (cs, [C.POINTER(ConvDesc)]),
    "rpnet_bn_stats_from_partial": (ci, [vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, cf, cf, vp, vp, vp, vp, vp]),
    "rpnet_conv_wgrad_workspace_bytes": (cs, [ci, ci, ci, ci, ci, ci]),
    "rpnet_conv_wgrad": (ci, [C.POINTER(ConvDesc), vp, vp, ci, ci, ci, ci, vp, cs, vp]),
    "rpnet_conv1_fwd": (ci, [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp, vp, ci, vp]),
    "rpnet_conv1_stats_blocks": (ci, [ci, ci, ci, ci, ci]),
    "rpnet_pow2_scale": (ci, [vp, vp, vp]),
    "rpnet_predict_scales": (ci, [vp, vp, vp, ci, cf, ci, vp, vp]),
    "rpnet_conv1_wgrad_workspace_bytes": (cs, [ci, ci, ci, ci]),
    "rpnet_conv1_wgrad": (ci, [vp, vp, vp, ci, ci, ci, ci, vp, cs, vp]),
    "rpnet_conv1_wgrad_bn": (ci, [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp, cs, vp, vp, vp]),
    "rpnet_conv1_bn_relu": (ci, [vp, vp, vp, vp, vp, vp, vp, ci, vp, vp, vp, ci, ci, ci, ci, ci, vp]),
    "rpnet_conv1_bn_bwd_rows": (ci, [ci, ci, ci, ci, ci]),
    "rpnet_conv1_bn_bwd_partial": (ci, [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp]),
    "rpnet_conv1_dgrad_bn": (ci, [vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp]),
    "rpnet_bn_bwd_coef_offset": (cs, [ci, ci]),
    "rpnet_bn_workspace_bytes": (cs, [ci, ci]),
    "rpnet_bn_stats": (ci, [vp, ci, ci, ci, ci, vp, vp, vp, vp, vp, cf, cf, vp, vp, vp, vp, vp, cs, vp]),
    "rpnet_bn_eval_affine": (ci, [vp, vp, vp, vp, cf, vp, vp, ci, vp]),
    "rpnet_bn_relu": (ci, [vp, vp, vp, vp, vp, ci, vp, vp, vp, ci, ci, ci, ci, ci, vp, ci, vp]),
    "rpnet_bn_act_scale": (ci, [vp, vp, vp, ci, ci, ci, ci, vp]),
    "rpnet_bn_bwd": (ci, [vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp, vp, vp, ci, ci, ci, ci, ci, vp, vp, ci, ci, vp, cs, vp, ci, vp]),
    "rpnet_bn_eval_relu": (ci, [vp, vp, vp, vp, vp, cs, ci, vp]),
    "rpnet_bn_eval_bwd": (ci, [vp, vp, vp, vp, vp, vp, vp, vp, ci, vp, vp, vp, ci, ci, ci, ci, ci, vp, cs, vp]),
    "rpnet_bias_relu_bwd_workspace_bytes": (cs, [ci]),
    "rpnet_bias_relu_bwd": (ci, [vp, vp, vp, vp, cs, ci, vp, cs, vp]),
    "rpnet_maxpool3_fwd": (ci, [vp, vp, ci, ci, ci, ci, ci, vp]),
    "rpnet_maxpool3_bwd": (ci, [vp, vp, vp, ci, ci, ci, ci, ci, vp]),
    "rpnet_maxpool2_fwd": (ci, [vp, vp, ci, ci, ci, ci, vp]),
    "rpnet_maxpool2_bwd": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, vp]),
    "rpnet_upsample2_bwd": (ci, [vp, vp, ci, ci, ci, ci, vp]),
    "rpnet_mask_avgpool": (ci, [vp, vp, ci, ci, ci, ci, vp]),
    "rpnet_local_corr_fwd": (ci, [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp]),
    "rpnet_local_corr_bwd_workspace_bytes": (cs, [ci, ci, ci, ci]),
    "rpnet_local_corr_bwd": (ci, [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, cs, vp]),
    "rpnet_local_corr_split_fwd": (ci, [vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp]),
    "rpnet_local_corr_split_bwd": (ci, [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, cs, vp]),
    "rpnet_affine_register": (ci, [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, cd, cd, cd, cd, vp]),
    "rpnet_sum_n": (ci, [vp, ci, vp, cs, vp]),
    "rpnet_demons_workspace_bytes": (cs, [ci, ci, ci]),
    "rpnet_demons_register": (ci, [vp, vp, vp, ci, vp, vp, vp, ci, ci, ci, ci, cd, cd, cd, cd, vp, cs, vp]),
    "rpnet_displacement_warp": (ci, [vp, vp, vp, ci, ci, ci, cf, cf, cf, vp]),
    "rpnet_affine_warp": (ci, [vp, vp, vp, vp, vp, ci, ci, ci, cf, cf, cf, vp]),
    "rpnet_identity_grid_warp": (ci, [vp, vp, ci, ci, ci, cf, cf, cf, vp]),
    "rpnet_mask_adjoint": (ci, [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp]),
    "rpnet_masked_pool_workspace_bytes": (cs, [ci, ci, ci, ci]),
    "rpnet_masked_pool_fwd": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, vp, cs, vp]),
    "rpnet_masked_pool_bwd": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, ci, vp]),
    "rpnet_cosine_match_fwd": (ci, [vp, vp, vp, ci, ci, ci, ci, cf, vp]),
    "rpnet_cosine_match_bwd_workspace_bytes": (cs, [ci, ci, ci, ci]),
    "rpnet_cosine_match_bwd": (ci, [vp, vp, vp, vp, vp, ci, ci, ci, ci, cf, ci, vp, cs, vp]),
    "rpnet_bilinear_up_fwd": (ci, [vp, vp, ci, ci, ci, ci, ci, vp]),
    "rpnet_bilinear_up_bwd": (ci, [vp, vp, ci, ci, ci, ci, ci, vp]),
    "rpnet_softmax_thresh_pool": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, vp]),
    "rpnet_refine_glue_supported": (ci, [ci, ci, ci, ci, ci, ci]),
    "rpnet_refine_glue_fwd": (ci, [vp, vp, vp, vp, cf, vp, vp, vp, vp, ci, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp]),
    "rpnet_refine_glue_bwd_workspace_bytes": (cs, [ci, ci, ci, ci, ci]),
    "rpnet_refine_glue_bwd": (ci, [vp, vp, vp, cf, vp, vp, ci, ci, ci, ci, ci, vp, cs, vp]),
    "rpnet_rowdot_scale": (ci, [vp, vp, vp, vp, vp, cs, ci, ci, ci, vp]),
    "rpnet_softmax_pool_bwd": (ci, [vp, vp, vp, ci, ci, ci, ci, ci, vp]),
    "rpnet_loss_workspace_bytes": (cs, [ci, ci, ci, ci]),
    "rpnet_dice_ce_fwd": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, vp, cs, vp]),
    "rpnet_dice_ce_bwd": (ci, [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, ci, vp]),
    "rpnet_dice_ce_multi_fwd": (ci, [C.POINTER(vp), ci, vp, vp, vp, ci, ci, ci, ci, vp, cs, vp]),
    "rpnet_dice_ce_multi_bwd": (ci, [C.POINTER(vp), C.POINTER(vp), ci, vp, vp, vp, ci, ci, ci, ci, vp]),
    "rpnet_objective_fwd": (ci, [C.POINTER(vp), C.POINTER(cf), ci, vp, vp, cf, vp, vp, ci, ci, ci, ci, vp, cs, vp]),
    "rpnet_objective_bwd": (ci, [C.POINTER(vp), C.POINTER(vp), C.POINTER(cf), ci, vp, vp, vp, vp, cf, ci, ci, ci, ci, vp]),
    "rpnet_seg_tally": (ci, [C.POINTER(vp), C.POINTER(C.c_int32), ci, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp]),
    "rpnet_argmax_masks": (ci, [vp, vp, vp, vp, ci, ci, ci, vp]),
    "rpnet_align_labels": (ci, [vp, vp, vp, cs, vp]),
    "rpnet_slice_minmax": (ci, [vp, vp, ci, ci, ci, vp]),
    "rpnet_augment_affine": (ci, [vp, vp, vp, vp, vp, vp, ci, ci, ci, vp]),
    "rpnet_elastic_field": (ci, [vp, vp, ci, cd, vp, vp, ci, ci, vp]),
    "rpnet_elastic_apply": (ci, [vp, vp, C.POINTER(cd), vp, vp, vp, vp, vp, ci, ci, ci, cf, vp]),
    "rpnet_debug_lds_canary": (ci, [ci, ci, C.c_longlong, vp, vp]),
    "rpnet_debug_fastdiv_selftest": (C.c_longlong, [ci]),
    "rpnet_debug_mfma_spin": (ci, [ci, ci, C.c_longlong, vp, vp]),
}
ABI_SYMBOLS = tuple(_SIGS)
ABI_VERSION = 111     # RPNET_ABI_VERSION of include/rpnet_abi.h

# the evaluation-item entry points: include/rpnet_eval_abi.h (ledger: tests/eval_abi_ledger.py)
_EVAL_SIGS = {
    "rpnet_eval_abi_version": (ci, []),
    "rpnet_eval_item_gather": (ci, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]),
    "rpnet_ncc_pairs_workspace_bytes": (cs, [cs]),
    "rpnet_ncc_pairs": (ci, [vp, vp, vp, cs, vp, ci, ci, vp, cs, vp]),
}
EVAL_ABI_SYMBOLS = tuple(_EVAL_SIGS)
EVAL_ABI_VERSION = 1     # RPNET_EVAL_ABI_VERSION of include/rpnet_eval_abi.h

# the optimizer entry points: include/rpnet_optim_abi.h (ledger: tests/optim_abi_ledger.py)
i64p = C.POINTER(C.c_int64)
_OPTIM_SIGS = {
    "rpnet_optim_abi_version": (ci, []),
    "rpnet_adam_plan_bytes": (cs, [i64p, ci]),
    "rpnet_adam_plan": (ci, [C.POINTER(vp), i64p, i64p, ci, vp, cs, i64p]),
    "rpnet_adam_step": (ci, [vp, C.c_int64, vp, vp, vp, vp, vp]),
}
OPTIM_ABI_SYMBOLS = tuple(_OPTIM_SIGS)
OPTIM_ABI_VERSION = 1     # RPNET_OPTIM_ABI_VERSION of include/rpnet_optim_abi.h

# the gradient guard of the optimizer step: include/rpnet_guard_abi.h (ledger: tests/guard_abi_ledger.py)
_GUARD_SIGS = {
    "rpnet_guard_abi_version": (ci, []),
    "rpnet_grad_guard_init": (ci, [vp, cd, ci, C.c_int64]),
    "rpnet_grad_sumsq": (ci, [vp, C.c_int64, vp, vp, vp, vp, vp]),
    "rpnet_adam_step_guarded": (ci, [vp, C.c_int64, vp, vp, vp, vp, vp, vp, vp, vp]),
}
GUARD_ABI_SYMBOLS = tuple(_GUARD_SIGS)
GUARD_ABI_VERSION = 1     # RPNET_GUARD_ABI_VERSION of include/rpnet_guard_abi.h

# the surface-distance tallies of an evaluated volume: include/rpnet_surface_abi.h (ledger: tests/surface_abi_ledger.py)
_SURFACE_SIGS = {
    "rpnet_surface_abi_version": (ci, []),
    "rpnet_surface_workspace_bytes": (cs, [ci, ci, ci]),
    "rpnet_surface_tally": (ci, [vp, ci, vp, ci, ci, ci, ci, ci, vp, C.c_int64, vp, C.c_int64, C.c_int64, vp, cs, vp]),
}
SURFACE_ABI_SYMBOLS = tuple(_SURFACE_SIGS)
SURFACE_ABI_VERSION = 1     # RPNET_SURFACE_ABI_VERSION of include/rpnet_surface_abi.h

# connected components of an evaluated volume and the largest-component filter: include/rpnet_cc_abi.h
# (ledger: tests/cc_abi_ledger.py)
_CC_SIGS = {
    "rpnet_cc_abi_version": (ci, []),
    "rpnet_cc_workspace_bytes": (cs, [ci, ci, ci]),
    "rpnet_cc_label": (ci, [vp, ci, ci, ci, ci, ci, ci, vp, vp, C.c_int64, C.c_int64, vp, cs, vp]),
    "rpnet_cc_keep_largest": (ci, [vp, ci, vp, ci, ci, ci, ci, ci, vp, ci, vp, C.c_int64, vp, C.c_int64, C.c_int64, vp, cs, vp]),
}
CC_ABI_SYMBOLS = tuple(_CC_SIGS)
CC_ABI_VERSION = 1     # RPNET_CC_ABI_VERSION of include/rpnet_cc_abi.h

# surface distances on a grid with a per-axis voxel spacing: include/rpnet_surface_spacing_abi.h (ledger: tests/surface_spacing_abi_ledger.py)
_SURFACE_SPACING_SIGS = {
    "rpnet_surface_spacing_abi_version": (ci, []),
    "rpnet_surface_spacing_workspace_bytes": (cs, [ci, ci, ci]),
    "rpnet_surface_spacing_tally": (ci, [vp, ci, vp, ci, ci, ci, ci, ci, C.POINTER(cd), cd, vp, C.c_int64, vp, C.c_int64, C.c_int64, vp, cs, vp]),
}
SURFACE_SPACING_ABI_SYMBOLS = tuple(_SURFACE_SPACING_SIGS)
SURFACE_SPACING_ABI_VERSION = 1     # RPNET_SURFACE_SPACING_ABI_VERSION of include/rpnet_surface_spacing_abi.h

# hole filling and the small-component filter of an evaluated volume: include/rpnet_ccpost_abi.h
# (ledger: tests/ccpost_abi_ledger.py)
_CCPOST_SIGS = {
    "rpnet_ccpost_abi_version": (ci, []),
    "rpnet_ccpost_workspace_bytes": (cs, [ci, ci, ci]),
    "rpnet_ccpost_fill_holes": (ci, [vp, ci, vp, ci, ci, ci, ci, ci, ci, C.c_int64, vp, ci, vp, C.c_int64, vp, C.c_int64, C.c_int64, vp, cs, vp]),
    "rpnet_ccpost_remove_small": (ci, [vp, ci, vp, ci, ci, ci, ci, ci, C.c_int64, vp, ci, vp, C.c_int64, vp, C.c_int64, C.c_int64, vp, cs, vp]),
}
CCPOST_ABI_SYMBOLS = tuple(_CCPOST_SIGS)
CCPOST_ABI_VERSION = 1     # RPNET_CCPOST_ABI_VERSION of include/rpnet_ccpost_abi.h

# ball morphology of an evaluated volume (erode, dilate, open, close): include/rpnet_morph_abi.h (ledger: tests/morph_abi_ledger.py)
_MORPH_TAIL = [vp, ci, vp, C.c_int64, vp, C.c_int64, C.c_int64, vp, cs, vp]     # truth, kind, counts, row, stats, row, rows, workspace, bytes, stream
_MORPH_SIGS = {
    "rpnet_morph_abi_version": (ci, []),
    "rpnet_morph_workspace_bytes": (cs, [ci, ci, ci]),
    "rpnet_morph_apply": (ci, [vp, ci, vp, ci, ci, ci, ci, ci, C.c_int64, ci, ci] + _MORPH_TAIL),
    "rpnet_morph_apply_spacing": (ci, [vp, ci, vp, ci, ci, ci, ci, ci, C.POINTER(cd), cd, ci, ci] + _MORPH_TAIL),
}
MORPH_ABI_SYMBOLS = tuple(_MORPH_SIGS)
MORPH_ABI_VERSION = 1     # RPNET_MORPH_ABI_VERSION of include/rpnet_morph_abi.h


# The families of entry points beside rpnet_abi.h, one per header: (header under include/, the words its version error uses, version
# symbol, version this binding was written for, signatures).  load() binds and checks them all in one loop.
SIDE_ABIS = [
    ("rpnet_eval_abi.h", "evaluation-item", "rpnet_eval_abi_version", EVAL_ABI_VERSION, _EVAL_SIGS),
    ("rpnet_optim_abi.h", "optimizer", "rpnet_optim_abi_version", OPTIM_ABI_VERSION, _OPTIM_SIGS),
    ("rpnet_guard_abi.h", "gradient-guard", "rpnet_guard_abi_version", GUARD_ABI_VERSION, _GUARD_SIGS),
    ("rpnet_surface_abi.h", "surface-distance", "rpnet_surface_abi_version", SURFACE_ABI_VERSION, _SURFACE_SIGS),
    ("rpnet_cc_abi.h", "connected-component", "rpnet_cc_abi_version", CC_ABI_VERSION, _CC_SIGS),
    ("rpnet_surface_spacing_abi.h", "surface-spacing", "rpnet_surface_spacing_abi_version", SURFACE_SPACING_ABI_VERSION, _SURFACE_SPACING_SIGS),
    ("rpnet_ccpost_abi.h", "post-processing", "rpnet_ccpost_abi_version", CCPOST_ABI_VERSION, _CCPOST_SIGS),
    ("rpnet_morph_abi.h", "morphology", "rpnet_morph_abi_version", MORPH_ABI_VERSION, _MORPH_SIGS),
]

# body-mask preprocessing of raw volumes (threshold, seeded component, mask and box): include/rpnet_prep_abi.h (ledger:
# tests/prep_abi_ledger.py).  The ninth side family.  tests/test_host_morph_abi_ledger.py holds SIDE_ABIS to the eight rows above with the
# morphology row last, so the families that came after it stand in a table of their own, of the same form; load() binds and checks
# ALL_SIDE_ABIS, and tests/test_host_prep_abi_ledger.py asserts over ALL_SIDE_ABIS what tests/test_host_side_abi_table.py asserts
# over SIDE_ABIS.
_PREP_SIGS = {
    "rpnet_prep_abi_version": (ci, []),
    "rpnet_prep_threshold_workspace_bytes": (cs, [ci, ci, ci]),
    "rpnet_prep_threshold": (ci, [vp, ci, vp, ci, ci, ci, ci, cd, vp, vp, vp, cs, vp]),
    "rpnet_prep_seeded_component_workspace_bytes": (cs, [ci, ci, ci]),
    "rpnet_prep_seeded_component": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, vp, cs, vp]),
    "rpnet_prep_mask_bbox_workspace_bytes": (cs, [ci, ci, ci]),
    "rpnet_prep_mask_bbox": (ci, [vp, ci, vp, vp, cd, ci, ci, ci, vp, C.c_int64, C.c_int64, vp, cs, vp]),
}
PREP_ABI_SYMBOLS = tuple(_PREP_SIGS)
PREP_ABI_VERSION = 1     # RPNET_PREP_ABI_VERSION of include/rpnet_prep_abi.h
LATER_SIDE_ABIS = [
    ("rpnet_prep_abi.h", "preprocessing", "rpnet_prep_abi_version", PREP_ABI_VERSION, _PREP_SIGS),
]
ALL_SIDE_ABIS = SIDE_ABIS + LATER_SIDE_ABIS

# resampling of images and label maps to another grid: include/rpnet_resample_abi.h (ledger: tests/resample_abi_ledger.py).  The tenth
# side family.  tests/test_host_prep_abi_ledger.py holds ALL_SIDE_ABIS to the nine rows above with the preprocessing row last, so the
# families that came after it stand in a further table of the same form; load() binds and checks ALL_SIDE_ABIS + SIDE_ABIS_AFTER_PREP.
_RESAMPLE_SIGS = {
    "rpnet_resample_abi_version": (ci, []),
    "rpnet_resample_workspace_bytes": (cs, [ci, ci, ci, ci, ci, ci]),
    "rpnet_resample_image": (ci, [vp, ci, ci, ci, ci, vp, ci, ci, ci, ci, ci, vp, cs, vp]),
    "rpnet_resample_labels": (ci, [vp, ci, ci, ci, vp, ci, ci, ci, ci, ci, ci, ci, vp, C.c_int64, C.c_int64, vp, cs, vp]),
}
RESAMPLE_ABI_SYMBOLS = tuple(_RESAMPLE_SIGS)
RESAMPLE_ABI_VERSION = 1     # RPNET_RESAMPLE_ABI_VERSION of include/rpnet_resample_abi.h
SIDE_ABIS_AFTER_PREP = [
    ("rpnet_resample_abi.h", "resampling", "rpnet_resample_abi_version", RESAMPLE_ABI_VERSION, _RESAMPLE_SIGS),
]

# separable Gaussian smoothing of a volume, the prefilter of a shrinking resample: include/rpnet_smooth_abi.h (ledger:
# tests/smooth_abi_ledger.py).  The eleventh side family.  tests/test_host_resample_abi_ledger.py holds SIDE_ABIS_AFTER_PREP to the one
# row above, so this family stands in a further table of the same form; load() binds and checks ALL_SIDE_ABIS + SIDE_ABIS_AFTER_PREP +
# SIDE_ABIS_AFTER_RESAMPLE.
_SMOOTH_SIGS = {
    "rpnet_smooth_abi_version": (ci, []),
    "rpnet_smooth_workspace_bytes": (cs, [ci, ci, ci, ci, ci, ci]),
    "rpnet_smooth_image": (ci, [vp, ci, ci, ci, ci, vp, vp, ci, vp, ci, vp, ci, ci, vp, cs, vp]),
}
SMOOTH_ABI_SYMBOLS = tuple(_SMOOTH_SIGS)
SMOOTH_ABI_VERSION = 1     # RPNET_SMOOTH_ABI_VERSION of include/rpnet_smooth_abi.h
SIDE_ABIS_AFTER_RESAMPLE = [
    ("rpnet_smooth_abi.h", "smoothing", "rpnet_smooth_abi_version", SMOOTH_ABI_VERSION, _SMOOTH_SIGS),
]

# the reader's preprocessing of a volume from the payload of its file (annotated z range, gather, rank selection, clip and map):
# include/rpnet_volload_abi.h (ledger: tests/volload_abi_ledger.py).  The twelfth side family.  tests/test_host_smooth_abi_ledger.py holds
# SIDE_ABIS_AFTER_RESAMPLE to the one row above, so this family stands in a further table of the same form; load() binds and checks
# ALL_SIDE_ABIS + SIDE_ABIS_AFTER_PREP + SIDE_ABIS_AFTER_RESAMPLE + SIDE_ABIS_AFTER_SMOOTH.
_VOLLOAD_SOURCE = [vp, ci, ci, ci, ci, ci, ci, ci, ci]      # source, kind, layout, D, H, W, num_slice, num_y, num_x
_VOLLOAD_SIGS = {
    "rpnet_volload_abi_version": (ci, []),
    "rpnet_volload_select_workspace_bytes": (cs, [cs]),
    "rpnet_volload_range": (ci, _VOLLOAD_SOURCE + [vp, vp]),
    "rpnet_volload_gather": (ci, _VOLLOAD_SOURCE + [ci, ci, ci, ci, cf, vp, vp]),
    "rpnet_volload_select": (ci, [vp, cs, cs, cs, vp, vp, cs, vp]),
    "rpnet_volload_normalize": (ci, [vp, vp, cs, vp, cf, cf, cf, cf, vp]),
}
VOLLOAD_ABI_SYMBOLS = tuple(_VOLLOAD_SIGS)
VOLLOAD_ABI_VERSION = 1     # RPNET_VOLLOAD_ABI_VERSION of include/rpnet_volload_abi.h
SIDE_ABIS_AFTER_SMOOTH = [
    ("rpnet_volload_abi.h", "volume-loading", "rpnet_volload_abi_version", VOLLOAD_ABI_VERSION, _VOLLOAD_SIGS),
]

# DEEDS registration of the reader's slices (cost volume in LDS, softmax expectation, warp by the upsampled grid):
# include/rpnet_deeds_abi.h (ledger: tests/deeds_abi_ledger.py).  The thirteenth side family.  tests/test_host_volload_abi_ledger.py holds
# SIDE_ABIS_AFTER_SMOOTH to the one row above, so this family stands in a further table of the same form; load() binds and checks
# ALL_SIDE_ABIS + SIDE_ABIS_AFTER_PREP + SIDE_ABIS_AFTER_RESAMPLE + SIDE_ABIS_AFTER_SMOOTH + SIDE_ABIS_AFTER_VOLLOAD.
_DEEDS_SIGS = {
    "rpnet_deeds_abi_version": (ci, []),
    "rpnet_deeds_workspace_bytes": (cs, [ci, ci, ci, ci]),
    # moving, fixed, gbase, sbase, S, H, W, G, D, disp_range, alpha0..5, pred, cost_out, ws, ws_bytes, stream
    "rpnet_deeds_register": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, ci, cf, cf, cf, cf, cf, cf, cf, vp, vp, vp, cs, vp]),
    "rpnet_deeds_warp": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, ci, cf, cf, cf, vp]),
}
DEEDS_ABI_SYMBOLS = tuple(_DEEDS_SIGS)
DEEDS_ABI_VERSION = 1     # RPNET_DEEDS_ABI_VERSION of include/rpnet_deeds_abi.h
SIDE_ABIS_AFTER_VOLLOAD = [
    ("rpnet_deeds_abi.h", "DEEDS-registration", "rpnet_deeds_abi_version", DEEDS_ABI_VERSION, _DEEDS_SIGS),
]

# label fusion of the masks several raters gave one volume (patterns and their histogram, the decision table, the fused mask):
# include/rpnet_fusion_abi.h (ledger: tests/fusion_abi_ledger.py).  The fourteenth side family.  tests/test_host_deeds_abi_ledger.py holds
# SIDE_ABIS_AFTER_VOLLOAD to the one row above, so this family stands in a further table of the same form; load() binds and checks
# ALL_SIDE_ABIS + SIDE_ABIS_AFTER_PREP + SIDE_ABIS_AFTER_RESAMPLE + SIDE_ABIS_AFTER_SMOOTH + SIDE_ABIS_AFTER_VOLLOAD + SIDE_ABIS_AFTER_DEEDS.
_FUSION_RATERS = [C.POINTER(vp), ci, ci, ci, ci, ci, ci]        # raters (a host array of device pointers), R, kind, cls, D, H, W
_FUSION_SIGS = {
    "rpnet_fusion_abi_version": (ci, []),
    "rpnet_fusion_workspace_bytes": (cs, [ci, ci, ci, ci]),
    "rpnet_fusion_patterns": (ci, _FUSION_RATERS + [vp, vp, vp]),
    # method, min_votes, weights, consensus, max_iter, tol, out, merge, prob, truth, truth_kind, counts, counts_row, stats, rater_f, rater_i,
    # row, n_rows, workspace, workspace_bytes, stream
    "rpnet_fusion_fuse": (ci, _FUSION_RATERS + [ci, ci, C.POINTER(cd), ci, ci, cd, vp, ci, vp, vp, ci, vp, C.c_int64, vp, vp, vp, C.c_int64,
                                                C.c_int64, vp, cs, vp]),
}
FUSION_ABI_SYMBOLS = tuple(_FUSION_SIGS)
FUSION_ABI_VERSION = 1     # RPNET_FUSION_ABI_VERSION of include/rpnet_fusion_abi.h
SIDE_ABIS_AFTER_DEEDS = [
    ("rpnet_fusion_abi.h", "label-fusion", "rpnet_fusion_abi_version", FUSION_ABI_VERSION, _FUSION_SIGS),
]

# region statistics of a segmented volume (per label the count, box, coordinate moments and the intensity sums of an image):
# include/rpnet_region_abi.h (ledger: tests/regions_abi_ledger.py).  The fifteenth side family.  tests/test_host_fusion_abi_ledger.py holds
# SIDE_ABIS_AFTER_DEEDS to the one row above, so this family stands in a further table of the same form; load() binds and checks
# ALL_SIDE_ABIS + SIDE_ABIS_AFTER_PREP + SIDE_ABIS_AFTER_RESAMPLE + SIDE_ABIS_AFTER_SMOOTH + SIDE_ABIS_AFTER_VOLLOAD + SIDE_ABIS_AFTER_DEEDS +
# SIDE_ABIS_AFTER_FUSION.
_REGION_SIGS = {
    "rpnet_region_abi_version": (ci, []),
    "rpnet_region_workspace_bytes": (cs, [ci, ci, ci, ci]),
    # labels, label_kind, image, image_kind, D, H, W, lo, L, rows_i, rows_f, row, n_rows, workspace, workspace_bytes, stream
    "rpnet_region_stats": (ci, [vp, ci, vp, ci, ci, ci, ci, ci, ci, vp, vp, C.c_int64, C.c_int64, vp, cs, vp]),
}
REGION_ABI_SYMBOLS = tuple(_REGION_SIGS)
REGION_ABI_VERSION = 1     # RPNET_REGION_ABI_VERSION of include/rpnet_region_abi.h
SIDE_ABIS_AFTER_FUSION = [
    ("rpnet_region_abi.h", "region-statistics", "rpnet_region_abi_version", REGION_ABI_VERSION, _REGION_SIGS),
]

# per-component statistics of a segmented volume (the dense renumbering of the sparse labels of rpnet_cc_label, then per component the
# count, box, coordinate moments, exact sums of the quantised image and the overlap with a class of a second volume):
# include/rpnet_compstat_abi.h (ledger: tests/compstat_abi_ledger.py).  The sixteenth side family.  tests/test_host_regions_abi_ledger.py
# holds SIDE_ABIS_AFTER_FUSION to the one row above, so this family stands in a further table of the same form; load() binds and checks
# it behind the others.
_COMPSTAT_SIGS = {
    "rpnet_compstat_abi_version": (ci, []),
    "rpnet_compstat_workspace_bytes": (cs, [ci, ci, ci, ci]),
    # labels, D, H, W, dense, stats, stats_row, n_rows, workspace, workspace_bytes, stream
    "rpnet_compstat_rank": (ci, [vp, ci, ci, ci, vp, vp, C.c_int64, C.c_int64, vp, cs, vp]),
    # dense, image, image_kind, scale_log2, other, other_kind, other_cls, D, H, W, max_components, rows, row, n_rows, workspace,
    # workspace_bytes, stream
    "rpnet_compstat_table": (ci, [vp, vp, ci, ci, vp, ci, ci, ci, ci, ci, ci, vp, C.c_int64, C.c_int64, vp, cs, vp]),
}
COMPSTAT_ABI_SYMBOLS = tuple(_COMPSTAT_SIGS)
COMPSTAT_ABI_VERSION = 1     # RPNET_COMPSTAT_ABI_VERSION of include/rpnet_compstat_abi.h
SIDE_ABIS_AFTER_REGIONS = [
    ("rpnet_compstat_abi.h", "component-statistics", "rpnet_compstat_abi_version", COMPSTAT_ABI_VERSION, _COMPSTAT_SIGS),
]


def lib_path():
    return _LIB_PATH


def load():
    """dlopen librpnet_hip.so once; loud failure if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError(f"{_LIB_PATH} not found: build it with `make -C rpnet_amd/csrc` "
                               "(or __graft_entry__.build()); rpnet_amd has no CPU fallback")
        lib = C.CDLL(_LIB_PATH)
        lib.rpnet_version.restype = ci
        if lib.rpnet_version() != ABI_VERSION:
            raise RuntimeError(f"{_LIB_PATH} has ABI version {lib.rpnet_version()}, this binding was written for {ABI_VERSION} "
                               "(include/rpnet_abi.h RPNET_ABI_VERSION): rebuild it with `make -C rpnet_amd/csrc`")
        side_abis = (ALL_SIDE_ABIS + SIDE_ABIS_AFTER_PREP + SIDE_ABIS_AFTER_RESAMPLE + SIDE_ABIS_AFTER_SMOOTH + SIDE_ABIS_AFTER_VOLLOAD
                     + SIDE_ABIS_AFTER_DEEDS + SIDE_ABIS_AFTER_FUSION + SIDE_ABIS_AFTER_REGIONS)
        for sigs in [_SIGS] + [family[4] for family in side_abis]:
            for name, (res, args) in sigs.items():
                fn = getattr(lib, name, None)
                if fn is None:
                    raise RuntimeError(f"{_LIB_PATH} does not export {name}: rebuild it with `make -C rpnet_amd/csrc`")
                fn.restype, fn.argtypes = res, args
        for header, words, version_symbol, version, _ in side_abis:
            if getattr(lib, version_symbol)() != version:
                raise RuntimeError(f"{_LIB_PATH} has {words} ABI version {getattr(lib, version_symbol)()}, this binding was written for "
                                   f"{version} (include/{header}): rebuild it with `make -C rpnet_amd/csrc`")
        _lib = lib
    return _lib


def ptr(t):
    return None if t is None else t.data_ptr()


try:        # the raw handle of the current stream without building a torch.cuda.Stream object (10 us -> 0.5 us per C-ABI call)
    _raw_stream, _cur_device = torch._C._cuda_getCurrentRawStream, torch._C._cuda_getDevice
except AttributeError:      # a torch build without the private accessors
    _raw_stream = None


def stream():
    if _raw_stream is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


def call(name, *args):
    """Invoke an int-returning entry point on the current stream; raise on failure."""
    lib = load()
    rc = getattr(lib, name)(*args, stream())
    if rc != 0:
        raise RuntimeError(f"{name} failed (rc={rc}): {lib.rpnet_last_error_string().decode()}")


def query(name, *args):
    return getattr(load(), name)(*args)


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("rpnet_amd runs on MI355X only: got a CPU tensor (there is no CPU fallback; "
                               "the CPU restatement lives in oracle/ and is test infrastructure)")
