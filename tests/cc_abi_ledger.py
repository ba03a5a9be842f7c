"""Ledger of the connected-component entry points (include/rpnet_cc_abi.h), in the form of tests/abi_ledger.py: which GPU test
exercises each exported symbol.  tests/test_host_cc_abi_ledger.py holds it to the same rules: the keys are exactly that header's
symbols, every named test exists and is a GPU test, and the test's source names the symbol or a name listed in VIA that leads to it
inside rpnet_amd."""

CC = "tests/test_gpu_components.py"

COVERED_BY = {
    "rpnet_cc_workspace_bytes": [CC + "::test_labels_equal_the_reference", CC + "::test_refusals_launch_nothing"],
    "rpnet_cc_label": [CC + "::test_labels_equal_the_reference", CC + "::test_every_element_kind_and_three_classes",
                       CC + "::test_runs_are_bit_identical", CC + "::test_refusals_launch_nothing"],
    "rpnet_cc_keep_largest": [CC + "::test_keep_largest_equals_the_reference", CC + "::test_every_element_kind_and_three_classes",
                              CC + "::test_runs_are_bit_identical", CC + "::test_refusals_launch_nothing",
                              CC + "::test_volume_segmenter_keep_largest", CC + "::test_evaluate_dataset_keep_largest",
                              CC + "::test_driver_on_device_keep_largest"],
}

# names on the Python side through which a test reaches a symbol it does not spell out
VIA = {
    "rpnet_cc_workspace_bytes": ["label_components", "keep_largest"],
    "rpnet_cc_label": ["label_components"],
    "rpnet_cc_keep_largest": ["keep_largest", "VolumeSegmenter", "evaluate_dataset"],
}

# symbols no GPU test should call
EXEMPT = {
    "rpnet_cc_abi_version": "checked by every load of the library (rpnet_amd.hip.load compares it with CC_ABI_VERSION) and, without a "
                            "GPU, by tests/test_host_cc_abi_ledger.py",
}
