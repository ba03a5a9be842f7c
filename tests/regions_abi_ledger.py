"""Ledger of the region-statistics entry points (include/rpnet_region_abi.h), in the form of tests/abi_ledger.py: which GPU test exercises
each exported symbol.  tests/test_host_regions_abi_ledger.py holds it to the same rules: the keys are exactly that header's symbols, every
named test exists and is a GPU test, and the test's source names the symbol or a name listed in VIA that leads to it inside rpnet_amd."""

RG = "tests/test_gpu_regions.py"

COVERED_BY = {
    "rpnet_region_workspace_bytes": [RG + "::test_shapes", RG + "::test_refusals_launch_nothing", RG + "::test_image_values"],
    "rpnet_region_stats": [RG + "::test_shapes", RG + "::test_second_trip_of_a_block", RG + "::test_label_counts",
                           RG + "::test_every_label_kind_both_image_kinds_and_offset_pointers", RG + "::test_image_values",
                           RG + "::test_captured_graph_of_region_stats_replayed_twice", RG + "::test_refusals_launch_nothing",
                           RG + "::test_volume_segmenter_regions_eager_and_graphed", RG + "::test_evaluate_dataset_regions_and_the_driver"],
}

# names on the Python side through which a test reaches a symbol it does not spell out
VIA = {
    "rpnet_region_workspace_bytes": ["region_stats", "region_workspace"],
    "rpnet_region_stats": ["region_stats", "VolumeSegmenter", "evaluate_dataset"],
}

# symbols no GPU test should call
EXEMPT = {
    "rpnet_region_abi_version": "checked by every load of the library (rpnet_amd.hip.load compares it with REGION_ABI_VERSION) and, "
                                "without a GPU, by tests/test_host_regions_abi_ledger.py",
}
