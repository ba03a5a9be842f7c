"""Ledger of the optimizer entry points (include/rpnet_optim_abi.h), in the form of tests/abi_ledger.py: which GPU test exercises each
exported symbol.  tests/test_host_optim_abi_ledger.py holds it to the same rules: the keys are exactly that header's symbols, every
named test exists and is a GPU test, and the test's source names the symbol or a name listed in VIA that leads to it inside
rpnet_amd."""

OPTIM = "tests/test_gpu_optim.py"

COVERED_BY = {
    "rpnet_adam_plan_bytes": [OPTIM + "::test_the_real_table", OPTIM + "::test_resume_from_torch_adam_and_back"],
    "rpnet_adam_plan": [OPTIM + "::test_the_real_table", OPTIM + "::test_resume_from_torch_adam_and_back"],
    "rpnet_adam_step": [OPTIM + "::test_awkward_sizes", OPTIM + "::test_misaligned_parameter_pointer",
                        OPTIM + "::test_zero_gradient_and_repeatability", OPTIM + "::test_capture_and_replay",
                        OPTIM + "::test_the_real_table"],
}

# names on the Python side through which a test reaches a symbol it does not spell out
VIA = {
    "rpnet_adam_plan_bytes": ["FusedAdam"],
    "rpnet_adam_plan": ["FusedAdam"],
    "rpnet_adam_step": ["FusedAdam"],
}

# symbols no GPU test should call
EXEMPT = {
    "rpnet_optim_abi_version": "checked by every load of the library (rpnet_amd.hip.load compares it with OPTIM_ABI_VERSION) and, "
                               "without a GPU, by tests/test_host_optim_abi_ledger.py",
}
