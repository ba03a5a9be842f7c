"""Ledger of the preprocessing entry points (include/rpnet_prep_abi.h), in the form of tests/abi_ledger.py: which GPU test exercises each
exported symbol.  tests/test_host_prep_abi_ledger.py holds it to the same rules: the keys are exactly that header's symbols, every named
test exists and is a GPU test, and the test's source names the symbol or a name listed in VIA that leads to it inside rpnet_amd."""

PG = "tests/test_gpu_preprocess.py"

COVERED_BY = {
    "rpnet_prep_threshold_workspace_bytes": [PG + "::test_threshold_equals_the_restatement", PG + "::test_guard_words_graph_replay_and_repeatability",
                                             PG + "::test_refusals_launch_nothing"],
    "rpnet_prep_threshold": [PG + "::test_threshold_equals_the_restatement", PG + "::test_threshold_cases",
                             PG + "::test_guard_words_graph_replay_and_repeatability", PG + "::test_refusals_launch_nothing",
                             PG + "::test_phantom_body_mask_and_clean_volume", PG + "::test_driver_end_to_end"],
    "rpnet_prep_seeded_component_workspace_bytes": [PG + "::test_seeded_component_equals_the_restatement",
                                                    PG + "::test_guard_words_graph_replay_and_repeatability", PG + "::test_refusals_launch_nothing"],
    "rpnet_prep_seeded_component": [PG + "::test_seeded_component_equals_the_restatement", PG + "::test_guard_words_graph_replay_and_repeatability",
                                    PG + "::test_refusals_launch_nothing", PG + "::test_phantom_body_mask_and_clean_volume",
                                    PG + "::test_driver_end_to_end"],
    "rpnet_prep_mask_bbox_workspace_bytes": [PG + "::test_mask_bbox_equals_the_restatement", PG + "::test_guard_words_graph_replay_and_repeatability",
                                             PG + "::test_refusals_launch_nothing"],
    "rpnet_prep_mask_bbox": [PG + "::test_mask_bbox_equals_the_restatement", PG + "::test_guard_words_graph_replay_and_repeatability",
                             PG + "::test_refusals_launch_nothing", PG + "::test_phantom_body_mask_and_clean_volume", PG + "::test_driver_end_to_end"],
}

# names on the Python side through which a test reaches a symbol it does not spell out
VIA = {
    "rpnet_prep_threshold_workspace_bytes": ["threshold_mask", "body_mask", "clean_volume"],
    "rpnet_prep_threshold": ["threshold_mask", "body_mask", "clean_volume"],
    "rpnet_prep_seeded_component_workspace_bytes": ["seeded_component", "body_mask", "clean_volume"],
    "rpnet_prep_seeded_component": ["seeded_component", "body_mask", "clean_volume"],
    "rpnet_prep_mask_bbox_workspace_bytes": ["mask_bbox", "clean_volume"],
    "rpnet_prep_mask_bbox": ["mask_bbox", "clean_volume"],
}

# symbols no GPU test should call
EXEMPT = {
    "rpnet_prep_abi_version": "checked by every load of the library (rpnet_amd.hip.load compares it with PREP_ABI_VERSION) and, "
                              "without a GPU, by tests/test_host_prep_abi_ledger.py",
}
