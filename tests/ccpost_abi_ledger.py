"""Ledger of the post-processing entry points (include/rpnet_ccpost_abi.h), in the form of tests/abi_ledger.py: which GPU test
exercises each exported symbol.  tests/test_host_ccpost_abi_ledger.py holds it to the same rules: the keys are exactly that header's
symbols, every named test exists and is a GPU test, and the test's source names the symbol or a name listed in VIA that leads to it
inside rpnet_amd."""

PP = "tests/test_gpu_postprocess.py"

COVERED_BY = {
    "rpnet_ccpost_workspace_bytes": [PP + "::test_fill_holes_equals_the_restatement", PP + "::test_graph_replay_and_guard_words",
                                     PP + "::test_refusals_launch_nothing"],
    "rpnet_ccpost_fill_holes": [PP + "::test_fill_holes_equals_the_restatement", PP + "::test_every_element_kind_and_three_classes",
                                PP + "::test_graph_replay_and_guard_words", PP + "::test_refusals_launch_nothing",
                                PP + "::test_volume_segmenter_chain", PP + "::test_evaluate_dataset_chain",
                                PP + "::test_driver_on_device_chain"],
    "rpnet_ccpost_remove_small": [PP + "::test_remove_small_equals_the_restatement", PP + "::test_every_element_kind_and_three_classes",
                                  PP + "::test_graph_replay_and_guard_words", PP + "::test_refusals_launch_nothing",
                                  PP + "::test_volume_segmenter_chain", PP + "::test_evaluate_dataset_chain",
                                  PP + "::test_driver_on_device_chain"],
}

# names on the Python side through which a test reaches a symbol it does not spell out
VIA = {
    "rpnet_ccpost_workspace_bytes": ["fill_holes", "remove_small"],
    "rpnet_ccpost_fill_holes": ["fill_holes", "VolumeSegmenter", "evaluate_dataset"],
    "rpnet_ccpost_remove_small": ["remove_small", "VolumeSegmenter", "evaluate_dataset"],
}

# symbols no GPU test should call
EXEMPT = {
    "rpnet_ccpost_abi_version": "checked by every load of the library (rpnet_amd.hip.load compares it with CCPOST_ABI_VERSION) and, "
                                "without a GPU, by tests/test_host_ccpost_abi_ledger.py",
}
