"""No untested gradient-guard entry point: tests/guard_abi_ledger.py names, for every symbol of include/rpnet_guard_abi.h, the GPU
test(s) that exercise it.  The rules and the machinery are those of tests/test_host_abi_ledger.py and its two followers (whose
headers these additions leave as they were); runs without a GPU."""
import ctypes
import os
import re

from rpnet_amd import hip
from tests import guard_abi_ledger as L
from tests.test_host_abi_ledger import ROOT, gpu_tests, header_symbols, package_defs, reaches

HEADER = os.path.join(ROOT, "include", "rpnet_guard_abi.h")


def _symbols(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(rpnet_\w+)\s*\(", text))


def guard_header_symbols():
    return _symbols(HEADER)


def test_ledger_keys_are_the_header_symbols_and_the_binding_knows_them():
    syms = guard_header_symbols()
    assert syms == {"rpnet_guard_abi_version", "rpnet_grad_guard_init", "rpnet_grad_sumsq", "rpnet_adam_step_guarded"}
    covered, exempt = set(L.COVERED_BY), set(L.EXEMPT)
    assert not (covered & exempt)
    assert covered | exempt == syms, (sorted(syms - covered - exempt), sorted((covered | exempt) - syms))
    assert set(L.VIA) <= covered
    assert all(isinstance(r, str) and len(r) > 20 for r in L.EXEMPT.values())
    assert set(hip.GUARD_ABI_SYMBOLS) == syms
    # one name, one header: nothing here is also declared in rpnet_abi.h, rpnet_eval_abi.h or rpnet_optim_abi.h
    assert not (syms & header_symbols()) and not (syms & set(hip.ABI_SYMBOLS))
    for other, known in (("rpnet_eval_abi.h", hip.EVAL_ABI_SYMBOLS), ("rpnet_optim_abi.h", hip.OPTIM_ABI_SYMBOLS)):
        assert not (syms & _symbols(os.path.join(ROOT, "include", other))) and not (syms & set(known)), other


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(hip.lib_path())
    for name in guard_header_symbols():
        assert hasattr(lib, name), f"{name} declared in rpnet_guard_abi.h but not exported"
    hdr = open(HEADER).read()
    lib.rpnet_guard_abi_version.restype = ctypes.c_int
    assert lib.rpnet_guard_abi_version() == hip.GUARD_ABI_VERSION == int(re.search(r"#define RPNET_GUARD_ABI_VERSION (\d+)", hdr).group(1))
    loaded = hip.load()
    assert loaded.rpnet_version() == hip.ABI_VERSION and loaded.rpnet_optim_abi_version() == hip.OPTIM_ABI_VERSION


def test_every_named_test_exists_is_a_gpu_test_and_names_what_it_covers():
    gpu, every = gpu_tests()
    defs = package_defs()
    problems = []
    for sym, tests in L.COVERED_BY.items():
        if not tests:
            problems.append(f"{sym}: no test")
        for tid in tests:
            if tid not in every:
                problems.append(f"{sym}: {tid} does not exist")
                continue
            if tid not in gpu:
                problems.append(f"{sym}: {tid} is not marked gpu")
                continue
            text = gpu[tid]
            if re.search(r"\b%s\b" % sym, text):
                continue
            via = [v for v in L.VIA.get(sym, []) if re.search(r"\b%s\b" % re.escape(v), text)]
            if not via:
                problems.append(f"{sym}: {tid} names neither the symbol nor any of {L.VIA.get(sym, [])}")
                continue
            if not any(reaches(defs, v, sym) for v in via if v in defs):
                problems.append(f"{sym}: nothing in rpnet_amd leads from {via} to the symbol")
    assert not problems, "\n".join(problems)


def test_the_check_would_notice():
    defs = package_defs()
    assert reaches(defs, "FusedAdam", "rpnet_adam_step_guarded") and reaches(defs, "FusedAdam", "rpnet_grad_sumsq")
    assert reaches(defs, "guard_block", "rpnet_grad_guard_init") and not reaches(defs, "guard_block", "rpnet_adam_step_guarded")
    assert not reaches(defs, "plan_chunks", "rpnet_adam_step_guarded") and not reaches(defs, "plan_chunks", "rpnet_grad_sumsq")
