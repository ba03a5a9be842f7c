"""Ledger of the gradient-guard entry points (include/rpnet_guard_abi.h), in the form of tests/abi_ledger.py: which GPU test exercises
each exported symbol.  tests/test_host_guard_abi_ledger.py holds it to the same rules: the keys are exactly that header's symbols,
every named test exists and is a GPU test, and the test's source names the symbol or a name listed in VIA that leads to it inside
rpnet_amd."""

GUARD = "tests/test_gpu_grad_guard.py"

COVERED_BY = {
    "rpnet_grad_guard_init": [GUARD + "::test_norm_against_fp64", GUARD + "::test_fused_adam"],
    "rpnet_grad_sumsq": [GUARD + "::test_norm_against_fp64", GUARD + "::test_driver_clips_under_both_optimizers"],
    "rpnet_adam_step_guarded": [GUARD + "::test_no_clipping_is_bit_identical", GUARD + "::test_clipping_against_torch",
                                GUARD + "::test_nonfinite_skip", GUARD + "::test_history_ring", GUARD + "::test_fused_adam",
                                GUARD + "::test_guarded_capture_and_replay"],
}

# names on the Python side through which a test reaches a symbol it does not spell out
VIA = {
    "rpnet_grad_guard_init": ["guard_block", "FusedAdam"],
    "rpnet_grad_sumsq": ["FusedAdam"],
    "rpnet_adam_step_guarded": ["FusedAdam"],
}

# symbols no GPU test should call
EXEMPT = {
    "rpnet_guard_abi_version": "checked by every load of the library (rpnet_amd.hip.load compares it with GUARD_ABI_VERSION) and, "
                               "without a GPU, by tests/test_host_guard_abi_ledger.py",
}
