"""Ledger of the per-component statistics entry points (include/rpnet_compstat_abi.h), in the form of tests/abi_ledger.py: which GPU test
exercises each exported symbol.  tests/test_host_compstat_abi_ledger.py holds it to the same rules: the keys are exactly that header's
symbols, every named test exists and is a GPU test, and the test's source names the symbol or a name listed in VIA that leads to it
inside rpnet_amd."""

CG = "tests/test_gpu_compstat.py"

COVERED_BY = {
    "rpnet_compstat_workspace_bytes": [CG + "::test_shapes", CG + "::test_refusals_launch_nothing"],
    "rpnet_compstat_rank": [CG + "::test_shapes", CG + "::test_empty_full_and_the_scan_past_its_block", CG + "::test_checkerboard_more_ids_than_slots",
                            CG + "::test_component_count_at_and_one_above_the_table",
                            CG + "::test_every_label_kind_both_connectivities_and_offset_pointers",
                            CG + "::test_invalid_labels_set_the_word_and_write_nothing_out_of_bounds",
                            CG + "::test_captured_graph_of_component_table_replayed_twice", CG + "::test_refusals_launch_nothing",
                            CG + "::test_volume_segmenter_components_eager_and_graphed", CG + "::test_evaluate_dataset_components_and_the_driver"],
    "rpnet_compstat_table": [CG + "::test_shapes", CG + "::test_empty_full_and_the_scan_past_its_block", CG + "::test_checkerboard_more_ids_than_slots",
                             CG + "::test_component_count_at_and_one_above_the_table",
                             CG + "::test_every_label_kind_both_connectivities_and_offset_pointers", CG + "::test_image_values",
                             CG + "::test_invalid_labels_set_the_word_and_write_nothing_out_of_bounds",
                             CG + "::test_captured_graph_of_component_table_replayed_twice", CG + "::test_refusals_launch_nothing",
                             CG + "::test_volume_segmenter_components_eager_and_graphed", CG + "::test_evaluate_dataset_components_and_the_driver"],
}

# names on the Python side through which a test reaches a symbol it does not spell out
VIA = {
    "rpnet_compstat_workspace_bytes": ["rank_components", "tally_components", "component_workspace"],
    "rpnet_compstat_rank": ["rank_components", "component_table", "VolumeSegmenter", "evaluate_dataset"],
    "rpnet_compstat_table": ["tally_components", "component_table", "VolumeSegmenter", "evaluate_dataset"],
}

# symbols no GPU test should call
EXEMPT = {
    "rpnet_compstat_abi_version": "checked by every load of the library (rpnet_amd.hip.load compares it with COMPSTAT_ABI_VERSION) and, "
                                  "without a GPU, by tests/test_host_compstat_abi_ledger.py",
}
