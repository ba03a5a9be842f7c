"""Ledger of the volume-loading entry points (include/rpnet_volload_abi.h), in the form of tests/abi_ledger.py: which GPU test exercises
each exported symbol.  tests/test_host_volload_abi_ledger.py holds it to the same rules: the keys are exactly that header's symbols, every
named test exists and is a GPU test, and the test's source names the symbol or a name listed in VIA that leads to it inside rpnet_amd."""

VG = "tests/test_gpu_volload.py"

COVERED_BY = {
    "rpnet_volload_select_workspace_bytes": [VG + "::test_selection_cases_equal_the_restatement_and_numpy", VG + "::test_refusals_launch_nothing"],
    "rpnet_volload_range": [VG + "::test_gather_and_range_equal_the_restatement", VG + "::test_refusals_launch_nothing",
                            VG + "::test_loader_equals_the_host_reader"],
    "rpnet_volload_gather": [VG + "::test_gather_and_range_equal_the_restatement", VG + "::test_refusals_launch_nothing",
                             VG + "::test_loader_equals_the_host_reader"],
    "rpnet_volload_select": [VG + "::test_selection_cases_equal_the_restatement_and_numpy",
                             VG + "::test_selection_past_one_sweep_unaligned_and_ragged", VG + "::test_refusals_launch_nothing",
                             VG + "::test_clip_and_map_equals_the_restatement"],
    "rpnet_volload_normalize": [VG + "::test_clip_and_map_equals_the_restatement", VG + "::test_graph_of_window_normalize_replayed_with_new_input",
                                VG + "::test_refusals_launch_nothing", VG + "::test_loader_equals_the_host_reader",
                                VG + "::test_episode_items_are_the_same_with_device_load",
                                VG + "::test_dataset_evaluation_and_drivers_with_device_load"],
}

# names on the Python side through which a test reaches a symbol it does not spell out
VIA = {
    "rpnet_volload_select_workspace_bytes": ["order_statistics", "window_normalize"],
    "rpnet_volload_range": ["annotated_range", "DeviceVolumeLoader"],
    "rpnet_volload_gather": ["gather_volume", "DeviceVolumeLoader"],
    "rpnet_volload_select": ["order_statistics", "percentile_f32", "window_normalize"],
    "rpnet_volload_normalize": ["window_normalize", "DeviceVolumeLoader", "DeviceEpisodeSource", "DeviceEvalSource"],
}

# symbols no GPU test should call
EXEMPT = {
    "rpnet_volload_abi_version": "checked by every load of the library (rpnet_amd.hip.load compares it with VOLLOAD_ABI_VERSION) and, "
                                 "without a GPU, by tests/test_host_volload_abi_ledger.py",
}
