"""Ledger of the surface-distance entry points for a per-axis voxel spacing (include/rpnet_surface_spacing_abi.h), in the form of
tests/abi_ledger.py: which GPU test exercises each exported symbol.  tests/test_host_surface_spacing.py holds it to the same rules: the
keys are exactly that header's symbols, every named test exists and is a GPU test, and the test's source names the symbol or a name
listed in VIA that leads to it inside rpnet_amd."""

SP = "tests/test_gpu_surface_spacing.py"

COVERED_BY = {
    "rpnet_surface_spacing_workspace_bytes": [SP + "::test_rows_equal_the_restatement", SP + "::test_refusals_launch_nothing",
                                              SP + "::test_workspace_guard_determinism_and_graph_replay"],
    "rpnet_surface_spacing_tally": [SP + "::test_rows_equal_the_restatement", SP + "::test_unit_spacing_equals_the_integer_path",
                                    SP + "::test_small_pooled_counts", SP + "::test_ties_across_the_rank_and_low_bits",
                                    SP + "::test_every_element_kind_and_class", SP + "::test_nsd_counts",
                                    SP + "::test_workspace_guard_determinism_and_graph_replay", SP + "::test_refusals_launch_nothing",
                                    SP + "::test_volume_segmenter_spacing", SP + "::test_evaluate_dataset_spacing_from_the_header"],
}

# names on the Python side through which a test reaches a symbol it does not spell out
VIA = {
    "rpnet_surface_spacing_tally": ["surface_tally_spacing", "VolumeSegmenter", "evaluate_dataset"],
}

# symbols no GPU test should call
EXEMPT = {
    "rpnet_surface_spacing_abi_version": "checked by every load of the library (rpnet_amd.hip.load compares it with "
                                         "SURFACE_SPACING_ABI_VERSION) and, without a GPU, by tests/test_host_surface_spacing.py",
}
