"""Ledger of the smoothing entry points (include/rpnet_smooth_abi.h), in the form of tests/abi_ledger.py: which GPU test exercises each
exported symbol.  tests/test_host_smooth_abi_ledger.py holds it to the same rules: the keys are exactly that header's symbols, every named
test exists and is a GPU test, and the test's source names the symbol or a name listed in VIA that leads to it inside rpnet_amd."""

SG = "tests/test_gpu_smooth.py"

COVERED_BY = {
    "rpnet_smooth_workspace_bytes": [SG + "::test_small_volumes_equal_the_restatement", SG + "::test_guard_words_out_given_and_graph_replay",
                                     SG + "::test_refusals_launch_nothing"],
    "rpnet_smooth_image": [SG + "::test_small_volumes_equal_the_restatement", SG + "::test_tiles_runs_and_unaligned_rows",
                           SG + "::test_lines_of_1024_and_radius_255", SG + "::test_more_lanes_than_one_sweep",
SG + "::test_ties_saturation_impulses_and_non_finite",
                           SG + "::test_guard_words_out_given_and_graph_replay", SG + "::test_refusals_launch_nothing",
                           SG + "::test_antialiased_resample_equals_the_composed_restatement"],
}

# names on the Python side through which a test reaches a symbol it does not spell out
VIA = {
    "rpnet_smooth_workspace_bytes": ["smooth_image", "resample_image", "resample_to_spacing"],
    "rpnet_smooth_image": ["smooth_image", "resample_image", "resample_to_spacing"],
}

# symbols no GPU test should call
EXEMPT = {
    "rpnet_smooth_abi_version": "checked by every load of the library (rpnet_amd.hip.load compares it with SMOOTH_ABI_VERSION) and, "
                                "without a GPU, by tests/test_host_smooth_abi_ledger.py",
}
