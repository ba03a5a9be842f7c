"""Ledger of the label-fusion entry points (include/rpnet_fusion_abi.h), in the form of tests/abi_ledger.py: which GPU test exercises each
exported symbol.  tests/test_host_fusion_abi_ledger.py holds it to the same rules: the keys are exactly that header's symbols, every
named test exists and is a GPU test, and the test's source names the symbol or a name listed in VIA that leads to it inside rpnet_amd."""

FG = "tests/test_gpu_fusion.py"

COVERED_BY = {
    "rpnet_fusion_workspace_bytes": [FG + "::test_workspace_guard_and_raw_entry_points", FG + "::test_refusals_launch_nothing",
                                     FG + "::test_shapes_and_rater_counts"],
    "rpnet_fusion_patterns": [FG + "::test_shapes_and_rater_counts", FG + "::test_workspace_guard_and_raw_entry_points",
                              FG + "::test_refusals_launch_nothing"],
    "rpnet_fusion_fuse": [FG + "::test_shapes_and_rater_counts", FG + "::test_second_trip_of_a_block", FG + "::test_special_inputs",
                          FG + "::test_every_element_kind_offset_pointers_and_a_truth_of_another_kind", FG + "::test_vote_and_weighted_options",
                          FG + "::test_staple_options", FG + "::test_three_classes_out_given_counts_added_sentinels_and_guards",
                          FG + "::test_workspace_guard_and_raw_entry_points", FG + "::test_captured_graph_of_fuse_replayed_twice",
                          FG + "::test_refusals_launch_nothing", FG + "::test_evaluate_runs_equals_plain_calls_and_fuses_their_masks"],
}

# names on the Python side through which a test reaches a symbol it does not spell out
VIA = {
    "rpnet_fusion_workspace_bytes": ["fuse", "run_fuse"],
    "rpnet_fusion_patterns": ["pattern_histogram"],
    "rpnet_fusion_fuse": ["fuse", "evaluate_runs"],
}

# symbols no GPU test should call
EXEMPT = {
    "rpnet_fusion_abi_version": "checked by every load of the library (rpnet_amd.hip.load compares it with FUSION_ABI_VERSION) and, "
                                "without a GPU, by tests/test_host_fusion_abi_ledger.py",
}
