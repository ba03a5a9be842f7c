"""Ledger of the evaluation-item entry points (include/rpnet_eval_abi.h), in the form of tests/abi_ledger.py: which GPU test exercises
each exported symbol.  tests/test_host_eval_abi_ledger.py holds it to the same rules: the keys are exactly that header's symbols,
every named test exists and is a GPU test, and the test's source names the symbol or a name listed in VIA that leads to it inside
rpnet_amd."""

DATASET_EVAL = "tests/test_gpu_dataset_eval.py"

COVERED_BY = {
    "rpnet_eval_item_gather": [DATASET_EVAL + "::test_gather_matches_numpy_indexing", DATASET_EVAL + "::test_gather_error_returns"],
    "rpnet_ncc_pairs_workspace_bytes": [DATASET_EVAL + "::test_ncc_pairs_against_float64_numpy"],
    "rpnet_ncc_pairs": [DATASET_EVAL + "::test_ncc_pairs_against_float64_numpy", DATASET_EVAL + "::test_ncc_pairs_constant_image_and_refusals"],
}

# names on the Python side through which a test reaches a symbol it does not spell out
VIA = {
    "rpnet_eval_item_gather": ["eval_item_gather"],
    "rpnet_ncc_pairs_workspace_bytes": ["ncc_pairs"],
    "rpnet_ncc_pairs": ["ncc_pairs"],
}

# symbols no GPU test should call
EXEMPT = {
    "rpnet_eval_abi_version": "checked by every load of the library (rpnet_amd.hip.load compares it with EVAL_ABI_VERSION) and, without a "
                              "GPU, by tests/test_host_eval_abi_ledger.py",
}
