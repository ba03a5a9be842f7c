"""Ledger of the C ABI (include/rpnet_abi.h): which GPU test exercises each exported symbol.  tests/test_host_abi_ledger.py
keeps it honest: the keys are exactly the header's symbols, every named test exists and is a GPU test, and the test's source
names the symbol — or, where the symbol is reached through the Python side, a name listed in VIA, which must lead to the symbol
inside rpnet_amd (a top-level function or class that holds the name and reaches the call, directly or through the functions it
names).  A new entry point therefore cannot land without a test that is written down here."""

OPS, SMALL, DMA, F16, MODEL, AUTOGRAD, VOLUME, AUGMENT, REG = (
    "tests/test_gpu_ops.py", "tests/test_gpu_small_ops.py", "tests/test_gpu_conv_dma.py", "tests/test_gpu_f16.py",
    "tests/test_gpu_model.py", "tests/test_gpu_autograd.py", "tests/test_gpu_volume.py", "tests/test_gpu_augment.py",
    "tests/test_registration.py")
REG64 = "tests/test_gpu_registration_fp64.py"
WGRAD64 = "tests/test_gpu_wgrad_fp64.py"
CONV164 = "tests/test_gpu_conv1_fp64.py"
CONV64 = "tests/test_gpu_conv_fp64.py"         # forward and input gradient at every dispatch edge: tests/conv_cases.py
OPERANDS = "tests/test_gpu_operands.py"        # the splitters and packers bit for bit: tests/operand_cases.py
GLUE64 = "tests/test_gpu_glue_fp64.py"         # the fused refinement glue, the multi-tensor loss and the objective: tests/glue_cases.py
AUG64 = "tests/test_gpu_augment_fp64.py"       # the train-time augmentation against the header's rules: tests/augment_ref_cases.py

COVERED_BY = {
    "rpnet_last_error_string": [VOLUME + "::test_tally_error_returns", SMALL + "::test_refusals"],
    # ---- weight packing, operand planes
    "rpnet_pack_conv_weight": [F16 + "::test_weight_pack_row_scales", OPERANDS + "::test_pack_f32", OPERANDS + "::test_refusals"],
    "rpnet_pack_conv_weight_split": [F16 + "::test_weight_pack_row_scales", OPERANDS + "::test_pack_split", OPERANDS + "::test_pack_impulses",
                                     OPERANDS + "::test_collapse_then_pack", OPERANDS + "::test_refusals"],
    "rpnet_pack_conv_weights_split": [OPS + "::test_conv_bn_relu", OPERANDS + "::test_pack_many_layers", OPERANDS + "::test_refusals"],
    "rpnet_upconv_collapse_weights": [DMA + "::test_upconv_collapsed_kernels_against_nine_tap_form_and_fp64", OPERANDS + "::test_collapse",
                                      OPERANDS + "::test_collapse_then_pack", OPERANDS + "::test_refusals"],
    "rpnet_split_bf16": [OPS + "::test_masked_split_on_a_channel_count_that_is_no_power_of_two", OPERANDS + "::test_split", OPERANDS + "::test_refusals"],
    "rpnet_split_f16": [OPS + "::test_masked_split_on_a_channel_count_that_is_no_power_of_two", OPERANDS + "::test_split", OPERANDS + "::test_refusals"],
    "rpnet_predict_scales": [MODEL + "::test_eval_fp16_planes_on_predicted_scales", OPERANDS + "::test_predict_scales", OPERANDS + "::test_refusals"],
    "rpnet_pow2_scale": [SMALL + "::test_pow2_scale", OPERANDS + "::test_pow2_scale", OPERANDS + "::test_refusals"],
    # ---- convolutions
    "rpnet_conv_fwd": [DMA + "::test_upconv_collapsed_kernels_against_nine_tap_form_and_fp64", OPS + "::test_conv_bn_relu", CONV64 + "::test_fp32_operands",
                       CONV64 + "::test_plain_split_kernels", CONV64 + "::test_patch_kernels", CONV64 + "::test_epilogue_features", CONV64 + "::test_input_gradient",
                       CONV64 + "::test_refusals"],
    "rpnet_conv_stats_blocks": [DMA + "::test_upconv_collapsed_kernels_against_nine_tap_form_and_fp64", CONV64 + "::test_epilogue_features"],
    "rpnet_conv_tile_variant": [DMA + "::test_dma_patch_kernel_bit_identical_and_accurate", CONV64 + "::test_plain_split_kernels", CONV64 + "::test_patch_kernels"],
    "rpnet_conv_splitk_workspace_bytes": [DMA + "::test_dma_patch_kernel_split_k", CONV64 + "::test_split_k"],
    "rpnet_conv_up4": [DMA + "::test_upconv_collapsed_kernels_against_nine_tap_form_and_fp64", CONV64 + "::test_collapsed_up_conv", CONV64 + "::test_refusals"],
    "rpnet_conv_up4_supported": [DMA + "::test_upconv_collapsed_kernels_against_nine_tap_form_and_fp64", CONV64 + "::test_collapsed_up_conv_turns_away"],
    "rpnet_conv_up4_stats_blocks": [DMA + "::test_upconv_collapsed_kernels_against_nine_tap_form_and_fp64", CONV64 + "::test_collapsed_up_conv"],
    "rpnet_conv_wgrad": [DMA + "::test_upconv_collapsed_kernels_against_nine_tap_form_and_fp64", WGRAD64 + "::test_fp32_dense_3x3", WGRAD64 + "::test_fp32_1x1_and_dilated",
                         WGRAD64 + "::test_planes_dense_3x3", WGRAD64 + "::test_planes_1x1", WGRAD64 + "::test_dynamic_range",
                         WGRAD64 + "::test_refusals"],
    "rpnet_conv_wgrad_workspace_bytes": [DMA + "::test_upconv_collapsed_kernels_against_nine_tap_form_and_fp64", WGRAD64 + "::test_planes_dense_3x3"],
    "rpnet_conv_wgrad_up4": [DMA + "::test_upconv_collapsed_kernels_against_nine_tap_form_and_fp64", WGRAD64 + "::test_collapsed_up_conv", WGRAD64 + "::test_refusals"],
    "rpnet_conv_wgrad_up4_supported": [DMA + "::test_upconv_collapsed_kernels_against_nine_tap_form_and_fp64", WGRAD64 + "::test_collapsed_up_conv_turns_away"],
    "rpnet_conv_wgrad_up4_workspace_bytes": [DMA + "::test_upconv_collapsed_kernels_against_nine_tap_form_and_fp64", WGRAD64 + "::test_collapsed_up_conv"],
    # ---- the first layer (Cin = 1)
    "rpnet_conv1_fwd": [AUTOGRAD + "::test_conv1_dgrad_bn_kernel", OPS + "::test_first_conv_cin1", CONV164 + "::test_forward", CONV164 + "::test_forward_impulses", CONV164 + "::test_block_caps", CONV164 + "::test_refusals"],
    "rpnet_conv1_stats_blocks": [OPS + "::test_first_conv_cin1", CONV164 + "::test_forward"],
    "rpnet_conv1_wgrad_workspace_bytes": [OPS + "::test_first_conv_cin1", WGRAD64 + "::test_first_layer", CONV164 + "::test_weight_gradient_from_the_bn_output_gradient"],
    "rpnet_conv1_wgrad": [MODEL + "::test_conv1_weight_gradient_from_bn_output_gradient", WGRAD64 + "::test_first_layer", WGRAD64 + "::test_refusals"],
    "rpnet_conv1_wgrad_bn": [MODEL + "::test_conv1_weight_gradient_from_bn_output_gradient", CONV164 + "::test_weight_gradient_from_the_bn_output_gradient", CONV164 + "::test_block_caps", CONV164 + "::test_refusals"],
    "rpnet_conv1_bn_relu": [MODEL + "::test_first_layer_without_its_pre_batchnorm_tensor", CONV164 + "::test_bn_relu_made_again_from_the_image", CONV164 + "::test_refusals"],
    "rpnet_conv1_bn_bwd_rows": [MODEL + "::test_first_layer_without_its_pre_batchnorm_tensor", CONV164 + "::test_bn_backward_reduction_made_again_from_the_image"],
    "rpnet_conv1_bn_bwd_partial": [MODEL + "::test_first_layer_without_its_pre_batchnorm_tensor", CONV164 + "::test_bn_backward_reduction_made_again_from_the_image", CONV164 + "::test_refusals"],
    "rpnet_conv1_dgrad_bn": [AUTOGRAD + "::test_conv1_dgrad_bn_kernel", CONV164 + "::test_input_gradient_from_the_bn_output_gradient", CONV164 + "::test_input_gradient_impulses", CONV164 + "::test_refusals"],
    # ---- BatchNorm
    "rpnet_bn_workspace_bytes": [AUTOGRAD + "::test_bn_eval_bwd_kernel", OPS + "::test_pooled_batchnorm_passes_on_odd_shapes", CONV164 + "::test_bn_backward_reduction_made_again_from_the_image"],
    "rpnet_bn_bwd_coef_offset": [AUTOGRAD + "::test_bn_eval_bwd_kernel", CONV164 + "::test_bn_backward_reduction_made_again_from_the_image"],
    "rpnet_bn_stats": [OPS + "::test_conv_bn_relu"],
    "rpnet_bn_stats_from_partial": [OPS + "::test_conv_bn_relu", OPS + "::test_first_conv_cin1"],
    "rpnet_bn_eval_affine": [AUTOGRAD + "::test_bn_eval_bwd_kernel"],
    "rpnet_bn_relu": [OPS + "::test_pooled_batchnorm_passes_on_odd_shapes", MODEL + "::test_bn_relu_maxpool_in_one_pass", CONV164 + "::test_bn_relu_made_again_from_the_image"],
    "rpnet_bn_act_scale": [SMALL + "::test_bn_act_scale"],
    "rpnet_bn_bwd": [OPS + "::test_pooled_batchnorm_passes_on_odd_shapes", MODEL + "::test_bn_relu_maxpool_in_one_pass", CONV164 + "::test_bn_backward_reduction_made_again_from_the_image"],
    "rpnet_bn_eval_relu": [AUTOGRAD + "::test_bn_eval_relu_kernel"],
    "rpnet_bn_eval_bwd": [AUTOGRAD + "::test_bn_eval_bwd_kernel"],
    # ---- VGG pieces, pooling
    "rpnet_bias_relu_bwd_workspace_bytes": [SMALL + "::test_bias_relu_bwd"],
    "rpnet_bias_relu_bwd": [SMALL + "::test_bias_relu_bwd", SMALL + "::test_refusals"],
    "rpnet_maxpool3_fwd": [SMALL + "::test_maxpool3", SMALL + "::test_refusals"],
    "rpnet_maxpool3_bwd": [SMALL + "::test_maxpool3", SMALL + "::test_refusals"],
    "rpnet_maxpool2_fwd": [SMALL + "::test_maxpool2_and_upsample2", SMALL + "::test_refusals"],
    "rpnet_maxpool2_bwd": [SMALL + "::test_maxpool2_and_upsample2", SMALL + "::test_refusals"],
    "rpnet_upsample2_bwd": [SMALL + "::test_maxpool2_and_upsample2", SMALL + "::test_refusals"],
    "rpnet_sum_n": [F16 + "::test_sum_n"],
    "rpnet_mask_avgpool": [SMALL + "::test_softmax_thresh_pool", SMALL + "::test_refusals"],
    # ---- local correlation
    "rpnet_local_corr_fwd": [OPS + "::test_local_correlation", OPS + "::test_local_correlation_golden"],
    "rpnet_local_corr_bwd_workspace_bytes": [OPS + "::test_local_correlation"],
    "rpnet_local_corr_bwd": [OPS + "::test_local_correlation"],
    "rpnet_local_corr_split_fwd": [OPS + "::test_local_correlation_writes_its_planes_on_a_given_scale", OPS + "::test_local_correlation"],
    "rpnet_local_corr_split_bwd": [OPS + "::test_local_correlation", OPS + "::test_local_correlation_f16_planes"],
    # ---- matcher
    "rpnet_mask_adjoint": [SMALL + "::test_masked_pool", SMALL + "::test_refusals"],
    "rpnet_masked_pool_workspace_bytes": [SMALL + "::test_masked_pool"],
    "rpnet_masked_pool_fwd": [SMALL + "::test_masked_pool", SMALL + "::test_refusals"],
    "rpnet_masked_pool_bwd": [SMALL + "::test_masked_pool", SMALL + "::test_refusals"],
    "rpnet_cosine_match_fwd": [SMALL + "::test_cosine_match", SMALL + "::test_refusals"],
    "rpnet_cosine_match_bwd_workspace_bytes": [SMALL + "::test_cosine_match"],
    "rpnet_cosine_match_bwd": [SMALL + "::test_cosine_match", SMALL + "::test_refusals"],
    "rpnet_bilinear_up_fwd": [SMALL + "::test_bilinear", SMALL + "::test_bilinear_forward_takes_a_ratio_that_is_no_integer"],
    "rpnet_bilinear_up_bwd": [SMALL + "::test_bilinear", SMALL + "::test_refusals"],
    "rpnet_softmax_thresh_pool": [SMALL + "::test_softmax_thresh_pool", SMALL + "::test_softmax_tie_block_counts_nothing"],
    "rpnet_refine_glue_supported": [OPS + "::test_refine_glue_is_the_separate_launches_bit_for_bit", GLUE64 + "::test_glue_supported_answers", GLUE64 + "::test_glue_forward"],
    "rpnet_refine_glue_fwd": [OPS + "::test_refine_glue_is_the_separate_launches_bit_for_bit", GLUE64 + "::test_glue_forward", GLUE64 + "::test_glue_forward_with_operand_planes", GLUE64 + "::test_glue_hard_mask_of_a_tie_is_zero", GLUE64 + "::test_glue_zero_patch", GLUE64 + "::test_refusals"],
    "rpnet_refine_glue_bwd_workspace_bytes": [OPS + "::test_refine_glue_is_the_separate_launches_bit_for_bit", GLUE64 + "::test_glue_backward", GLUE64 + "::test_glue_supported_answers"],
    "rpnet_refine_glue_bwd": [OPS + "::test_refine_glue_is_the_separate_launches_bit_for_bit", GLUE64 + "::test_glue_backward", GLUE64 + "::test_glue_zero_patch", GLUE64 + "::test_refusals"],
    "rpnet_rowdot_scale": [SMALL + "::test_rowdot_scale", SMALL + "::test_refusals"],
    "rpnet_softmax_pool_bwd": [SMALL + "::test_softmax_thresh_pool", SMALL + "::test_refusals"],
    # ---- losses, evaluation tallies, align pieces
    "rpnet_loss_workspace_bytes": [SMALL + "::test_dice_ce"],
    "rpnet_dice_ce_fwd": [SMALL + "::test_dice_ce", SMALL + "::test_refusals"],
    "rpnet_dice_ce_bwd": [SMALL + "::test_dice_ce", SMALL + "::test_refusals"],
    "rpnet_dice_ce_multi_fwd": [OPS + "::test_dice_ce_sum_matches_separate_calls", GLUE64 + "::test_multi_loss_and_objective", GLUE64 + "::test_refusals"],
    "rpnet_dice_ce_multi_bwd": [OPS + "::test_dice_ce_sum_matches_separate_calls", GLUE64 + "::test_multi_loss_and_objective", GLUE64 + "::test_refusals"],
    "rpnet_objective_fwd": [OPS + "::test_objective_is_the_tensor_expression_bit_for_bit", GLUE64 + "::test_multi_loss_and_objective", GLUE64 + "::test_refusals"],
    "rpnet_objective_bwd": [OPS + "::test_objective_is_the_tensor_expression_bit_for_bit", GLUE64 + "::test_multi_loss_and_objective", GLUE64 + "::test_refusals"],
    "rpnet_seg_tally": [VOLUME + "::test_tally_error_returns", VOLUME + "::test_captured_launch_follows_n_valid"],
    "rpnet_argmax_masks": [SMALL + "::test_argmax_masks", SMALL + "::test_refusals"],
    "rpnet_align_labels": [SMALL + "::test_align_labels", SMALL + "::test_refusals"],
    # ---- registration pre-step
    "rpnet_affine_register": [REG + "::test_hip_registration_pieces_vs_oracle", REG64 + "::test_affine_gradient_and_loss", REG64 + "::test_affine_default_adam_first_step",
        REG64 + "::test_registration_refusals"],
    "rpnet_affine_warp": [REG + "::test_hip_registration_pieces_vs_oracle", REG64 + "::test_warps",
        REG64 + "::test_registration_refusals"],
    "rpnet_identity_grid_warp": [REG + "::test_hip_registration_pieces_vs_oracle", REG64 + "::test_warps",
        REG64 + "::test_registration_refusals"],
    "rpnet_demons_workspace_bytes": [REG + "::test_hip_demons_stage_vs_oracle", REG64 + "::test_demons_first_step",
        REG64 + "::test_registration_refusals"],
    "rpnet_demons_register": [REG + "::test_hip_demons_stage_vs_oracle", REG64 + "::test_demons_first_step", REG64 + "::test_demons_second_step", REG64 + "::test_demons_degenerate_inputs",
        REG64 + "::test_registration_refusals"],
    "rpnet_displacement_warp": [REG + "::test_hip_demons_stage_vs_oracle", REG64 + "::test_warps",
        REG64 + "::test_registration_refusals"],
    # ---- train-time augmentation
    "rpnet_slice_minmax": [AUGMENT + "::test_gamma_affine_matches_host", AUG64 + "::test_slice_minmax", AUG64 + "::test_sixty_five_thousand_slices",
                           AUG64 + "::test_production_size_once", AUG64 + "::test_no_slices_is_success_and_writes_nothing", AUG64 + "::test_refusals"],
    "rpnet_augment_affine": [AUGMENT + "::test_gamma_affine_matches_host", AUG64 + "::test_affine_exact_maps", AUG64 + "::test_affine_drawn_maps",
                             AUG64 + "::test_affine_image_path", AUG64 + "::test_sixty_five_thousand_slices", AUG64 + "::test_production_size_once",
                             AUG64 + "::test_no_slices_is_success_and_writes_nothing", AUG64 + "::test_refusals"],
    "rpnet_elastic_field": [AUGMENT + "::test_elastic_field_matches_scipy", AUG64 + "::test_elastic_field", AUG64 + "::test_production_size_once",
                            AUG64 + "::test_refusals"],
    "rpnet_elastic_apply": [AUGMENT + "::test_elastic_slices_match_host", AUG64 + "::test_elastic_apply_crafted", AUG64 + "::test_elastic_apply_drawn",
                            AUG64 + "::test_production_size_once", AUG64 + "::test_no_slices_is_success_and_writes_nothing", AUG64 + "::test_refusals"],
}

# names on the Python side through which a test reaches a symbol it does not spell out
VIA = {
    "rpnet_pack_conv_weight": ["PackedWeight"],
    "rpnet_pack_conv_weight_split": ["PackedWeight"],
    "rpnet_pack_conv_weights_split": ["WeightCache"],
    "rpnet_upconv_collapse_weights": ["PackedWeight"],
    "rpnet_predict_scales": ["RP_Net"],
    "rpnet_conv_fwd": ["conv_bn_relu"],
    "rpnet_conv_splitk_workspace_bytes": ["conv_bn_relu_op"],
    "rpnet_conv1_fwd": ["conv_bn_relu"],
    "rpnet_conv1_stats_blocks": ["conv_bn_relu"],
    "rpnet_conv1_wgrad_workspace_bytes": ["conv_bn_relu"],
    "rpnet_conv1_wgrad": ["_CONV1_BN_FUSE"],
    "rpnet_conv1_bn_relu": ["_CONV1_RECOMP"],
    "rpnet_conv1_bn_bwd_rows": ["_CONV1_RECOMP"],
    "rpnet_conv1_bn_bwd_partial": ["_CONV1_RECOMP"],
    "rpnet_bn_stats": ["conv_bn_relu"],
    "rpnet_bn_stats_from_partial": ["conv_bn_relu"],
    "rpnet_sum_n": ["sum_n"],
    "rpnet_local_corr_fwd": ["LocalCorr"],
    "rpnet_local_corr_bwd_workspace_bytes": ["LocalCorr"],
    "rpnet_local_corr_bwd": ["LocalCorr"],
    "rpnet_local_corr_split_fwd": ["LocalCorr"],
    "rpnet_local_corr_split_bwd": ["LocalCorr", "local_corr"],
    "rpnet_refine_glue_supported": ["glue_supported"],
    "rpnet_refine_glue_bwd_workspace_bytes": ["CosineMatchUp"],
    "rpnet_refine_glue_bwd": ["CosineMatchUp"],
    "rpnet_dice_ce_multi_fwd": ["dice_ce_sum"],
    "rpnet_dice_ce_multi_bwd": ["dice_ce_sum"],
    "rpnet_objective_bwd": ["objective"],
    "rpnet_seg_tally": ["seg_tally"],
    "rpnet_affine_register": ["affine_register"],
    "rpnet_affine_warp": ["affine_warp"],
    "rpnet_identity_grid_warp": ["identity_grid_warp"],
    "rpnet_demons_workspace_bytes": ["demons_register"],
    "rpnet_demons_register": ["demons_register"],
    "rpnet_displacement_warp": ["displacement_warp"],
    "rpnet_slice_minmax": ["augment_slices"],
    "rpnet_augment_affine": ["augment_slices"],
    "rpnet_elastic_field": ["elastic_field"],
    "rpnet_elastic_apply": ["elastic_slices"],
}

# symbols no GPU test should call
EXEMPT = {
    "rpnet_version": "checked by every load of the library (rpnet_amd.hip.load compares it with ABI_VERSION) and, without a GPU, "
                     "by tests/test_host_cpu.py",
    "rpnet_debug_lds_canary": "diagnostic probe: occupies LDS beside other kernels on purpose, tools/lds_canary.py only",
    "rpnet_debug_mfma_spin": "diagnostic probe: a spinner that holds the matrix pipe, tools/corun_probe.py only",
    "rpnet_debug_fastdiv_selftest": "host-only self-test, needs no GPU: run by tests/test_host_cpu.py",
}
