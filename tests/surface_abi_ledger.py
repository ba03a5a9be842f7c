"""Ledger of the surface-distance entry points (include/rpnet_surface_abi.h), in the form of tests/abi_ledger.py: which GPU test
exercises each exported symbol.  tests/test_host_surface_abi_ledger.py holds it to the same rules: the keys are exactly that header's
symbols, every named test exists and is a GPU test, and the test's source names the symbol or a name listed in VIA that leads to it
inside rpnet_amd."""

SURFACE = "tests/test_gpu_surface.py"

COVERED_BY = {
    "rpnet_surface_workspace_bytes": [SURFACE + "::test_refusals_launch_nothing", SURFACE + "::test_tally_equals_the_reference"],
    "rpnet_surface_tally": [SURFACE + "::test_tally_equals_the_reference", SURFACE + "::test_long_lines_and_the_axis_limit",
                            SURFACE + "::test_empty_borders_give_the_k_minus_one_row", SURFACE + "::test_every_element_kind_and_class",
                            SURFACE + "::test_runs_are_byte_identical_and_rows_are_kept", SURFACE + "::test_refusals_launch_nothing",
                            SURFACE + "::test_volume_segmenter_surface", SURFACE + "::test_evaluate_dataset_surface"],
}

# names on the Python side through which a test reaches a symbol it does not spell out
VIA = {
    "rpnet_surface_workspace_bytes": ["surface_tally"],
    "rpnet_surface_tally": ["surface_tally", "VolumeSegmenter", "evaluate_dataset"],
}

# symbols no GPU test should call
EXEMPT = {
    "rpnet_surface_abi_version": "checked by every load of the library (rpnet_amd.hip.load compares it with SURFACE_ABI_VERSION) and, "
                                 "without a GPU, by tests/test_host_surface_abi_ledger.py",
}
