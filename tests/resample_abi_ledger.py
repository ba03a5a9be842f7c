"""Ledger of the resampling entry points (include/rpnet_resample_abi.h), in the form of tests/abi_ledger.py: which GPU test exercises each
exported symbol.  tests/test_host_resample_abi_ledger.py holds it to the same rules: the keys are exactly that header's symbols, every named
test exists and is a GPU test, and the test's source names the symbol or a name listed in VIA that leads to it inside rpnet_amd."""

RG = "tests/test_gpu_resample.py"

COVERED_BY = {
    "rpnet_resample_workspace_bytes": [RG + "::test_small_grids_equal_the_restatement", RG + "::test_guard_words_out_given_and_graph_replay",
                                       RG + "::test_refusals_launch_nothing"],
    "rpnet_resample_image": [RG + "::test_small_grids_equal_the_restatement", RG + "::test_lane_runs_and_unaligned_rows",
                             RG + "::test_a_line_of_1024_along_each_axis", RG + "::test_ties_saturation_and_non_finite_neighbours",
                             RG + "::test_guard_words_out_given_and_graph_replay", RG + "::test_refusals_launch_nothing"],
    "rpnet_resample_labels": [RG + "::test_label_maps_with_three_classes", RG + "::test_lane_runs_and_unaligned_rows",
                              RG + "::test_a_line_of_1024_along_each_axis", RG + "::test_ties_saturation_and_non_finite_neighbours",
                              RG + "::test_guard_words_out_given_and_graph_replay", RG + "::test_refusals_launch_nothing"],
}

# names on the Python side through which a test reaches a symbol it does not spell out
VIA = {
    "rpnet_resample_workspace_bytes": ["resample_image", "resample_labels", "resample_to_spacing", "resample_like"],
    "rpnet_resample_image": ["resample_image", "resample_to_spacing", "resample_like"],
    "rpnet_resample_labels": ["resample_labels", "resample_to_spacing", "resample_like"],
}

# symbols no GPU test should call
EXEMPT = {
    "rpnet_resample_abi_version": "checked by every load of the library (rpnet_amd.hip.load compares it with RESAMPLE_ABI_VERSION) and, "
                                  "without a GPU, by tests/test_host_resample_abi_ledger.py",
}
