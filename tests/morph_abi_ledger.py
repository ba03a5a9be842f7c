"""Ledger of the ball-morphology entry points (include/rpnet_morph_abi.h), in the form of tests/abi_ledger.py: which GPU test exercises
each exported symbol.  tests/test_host_morph_abi_ledger.py holds it to the same rules: the keys are exactly that header's symbols, every
named test exists and is a GPU test, and the test's source names the symbol or a name listed in VIA that leads to it inside rpnet_amd."""

MG = "tests/test_gpu_morphology.py"

COVERED_BY = {
    "rpnet_morph_workspace_bytes": [MG + "::test_every_shape_equals_the_restatement", MG + "::test_graph_replay_guard_words_and_repeatability",
                                    MG + "::test_refusals_launch_nothing"],
    "rpnet_morph_apply": [MG + "::test_every_shape_equals_the_restatement", MG + "::test_borders_and_contents",
                          MG + "::test_ball_larger_than_the_volume", MG + "::test_ties_at_the_threshold",
                          MG + "::test_label_volumes_and_element_kinds", MG + "::test_graph_replay_guard_words_and_repeatability",
                          MG + "::test_refusals_launch_nothing", MG + "::test_volume_segmenter_morphology",
                          MG + "::test_evaluate_dataset_morphology", MG + "::test_driver_morphology"],
    "rpnet_morph_apply_spacing": [MG + "::test_every_shape_equals_the_restatement", MG + "::test_borders_and_contents",
                                  MG + "::test_ball_larger_than_the_volume", MG + "::test_ties_at_the_threshold",
                                  MG + "::test_label_volumes_and_element_kinds", MG + "::test_graph_replay_guard_words_and_repeatability",
                                  MG + "::test_refusals_launch_nothing", MG + "::test_volume_segmenter_morphology",
                                  MG + "::test_evaluate_dataset_morphology", MG + "::test_driver_morphology"],
}

# names on the Python side through which a test reaches a symbol it does not spell out
VIA = {
    "rpnet_morph_workspace_bytes": ["erode", "dilate", "opening", "closing"],
    "rpnet_morph_apply": ["erode", "dilate", "opening", "closing", "VolumeSegmenter", "evaluate_dataset"],
    "rpnet_morph_apply_spacing": ["erode", "dilate", "opening", "closing", "VolumeSegmenter", "evaluate_dataset"],
}

# symbols no GPU test should call
EXEMPT = {
    "rpnet_morph_abi_version": "checked by every load of the library (rpnet_amd.hip.load compares it with MORPH_ABI_VERSION) and, "
                               "without a GPU, by tests/test_host_morph_abi_ledger.py",
}
