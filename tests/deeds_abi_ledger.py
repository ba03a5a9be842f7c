"""Ledger of the DEEDS registration entry points (include/rpnet_deeds_abi.h), in the form of tests/abi_ledger.py: which GPU test exercises
each exported symbol.  tests/test_host_deeds_abi_ledger.py holds it to the same rules: the keys are exactly that header's symbols, every
named test exists and is a GPU test, and the test's source names the symbol or a name listed in VIA that leads to it inside rpnet_amd."""

DG = "tests/test_gpu_deeds.py"

COVERED_BY = {
    "rpnet_deeds_workspace_bytes": [DG + "::test_outputs_and_workspace_prefilled_with_nan_and_guarded", DG + "::test_refusals_launch_nothing",
                                    DG + "::test_captured_graph_of_register_and_warp_replayed"],
    "rpnet_deeds_register": [DG + "::test_pred_and_cost_against_float64", DG + "::test_fixture_cases_through_deeds_register",
                             DG + "::test_recovers_a_constructed_shift", DG + "::test_outputs_and_workspace_prefilled_with_nan_and_guarded",
                             DG + "::test_captured_graph_of_register_and_warp_replayed", DG + "::test_refusals_launch_nothing",
                             DG + "::test_register_slices_deeds_is_the_entry_points_composed", DG + "::test_readers_sources_and_drivers_with_deeds"],
    "rpnet_deeds_warp": [DG + "::test_deeds_warp_against_float64_grid_sample", DG + "::test_fixture_cases_through_deeds_register",
                         DG + "::test_outputs_and_workspace_prefilled_with_nan_and_guarded", DG + "::test_captured_graph_of_register_and_warp_replayed",
                         DG + "::test_refusals_launch_nothing", DG + "::test_register_slices_deeds_is_the_entry_points_composed",
                         DG + "::test_readers_sources_and_drivers_with_deeds"],
}

# names on the Python side through which a test reaches a symbol it does not spell out
VIA = {
    "rpnet_deeds_workspace_bytes": ["deeds_register"],
    "rpnet_deeds_register": ["deeds_register", "register_slices", "get_registration_field", "DeviceEvalSource"],
    "rpnet_deeds_warp": ["deeds_warp", "register_slices", "get_registration_field", "DeviceEvalSource"],
}

# symbols no GPU test should call
EXEMPT = {
    "rpnet_deeds_abi_version": "checked by every load of the library (rpnet_amd.hip.load compares it with DEEDS_ABI_VERSION) and, "
                               "without a GPU, by tests/test_host_deeds_abi_ledger.py",
}
