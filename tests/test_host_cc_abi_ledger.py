"""No untested connected-component entry point: tests/cc_abi_ledger.py names, for every symbol of include/rpnet_cc_abi.h, the GPU
test(s) that exercise it.  The rules and the machinery are those of tests/test_host_abi_ledger.py and its followers (whose headers
these additions leave as they were); runs without a GPU."""
import ctypes
import os
import re

from rpnet_amd import hip
from tests import cc_abi_ledger as L
from tests.test_host_abi_ledger import ROOT, gpu_tests, header_symbols, package_defs, reaches
from tests.test_host_guard_abi_ledger import _symbols

HEADER = os.path.join(ROOT, "include", "rpnet_cc_abi.h")


def test_ledger_keys_are_the_header_symbols_and_the_binding_knows_them():
    syms = _symbols(HEADER)
    assert syms == {"rpnet_cc_abi_version", "rpnet_cc_workspace_bytes", "rpnet_cc_label", "rpnet_cc_keep_largest"}
    covered, exempt = set(L.COVERED_BY), set(L.EXEMPT)
    assert not (covered & exempt)
    assert covered | exempt == syms, (sorted(syms - covered - exempt), sorted((covered | exempt) - syms))
    assert set(L.VIA) <= covered
    assert all(isinstance(r, str) and len(r) > 20 for r in L.EXEMPT.values())
    assert set(hip.CC_ABI_SYMBOLS) == syms
    # one name, one header: nothing here is also declared in one of the five earlier headers
    assert not (syms & header_symbols()) and not (syms & set(hip.ABI_SYMBOLS))
    for other, known in (("rpnet_eval_abi.h", hip.EVAL_ABI_SYMBOLS), ("rpnet_optim_abi.h", hip.OPTIM_ABI_SYMBOLS),
                         ("rpnet_guard_abi.h", hip.GUARD_ABI_SYMBOLS), ("rpnet_surface_abi.h", hip.SURFACE_ABI_SYMBOLS)):
        assert not (syms & _symbols(os.path.join(ROOT, "include", other))) and not (syms & set(known)), other


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(hip.lib_path())
    for name in _symbols(HEADER):
        assert hasattr(lib, name), f"{name} declared in rpnet_cc_abi.h but not exported"
    hdr = open(HEADER).read()
    lib.rpnet_cc_abi_version.restype = ctypes.c_int
    assert lib.rpnet_cc_abi_version() == hip.CC_ABI_VERSION == int(re.search(r"#define RPNET_CC_ABI_VERSION (\d+)", hdr).group(1))
    surface = open(os.path.join(ROOT, "include", "rpnet_surface_abi.h")).read()
    assert re.search(r"#define RPNET_CC_MAX_DIM (\d+)", hdr).group(1) == re.search(r"#define RPNET_SURFACE_MAX_DIM (\d+)", surface).group(1)
    for kind in ("U8", "I32", "I64", "F32"):           # the element kinds are those of the surface ABI
        assert re.search(r"#define RPNET_CC_%s (\d)" % kind, hdr).group(1) == re.search(r"#define RPNET_SURFACE_%s (\d)" % kind, surface).group(1)
    loaded = hip.load()
    assert loaded.rpnet_version() == hip.ABI_VERSION and loaded.rpnet_surface_abi_version() == hip.SURFACE_ABI_VERSION
    # the size query needs no GPU
    loaded.rpnet_cc_workspace_bytes.restype = ctypes.c_size_t
    assert loaded.rpnet_cc_workspace_bytes(2, 3, 5) == 64 + 2 * 128 and loaded.rpnet_cc_workspace_bytes(0, 3, 5) == 0
    assert loaded.rpnet_last_error_string().decode().startswith("components: D=0")


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
    assert reaches(defs, "keep_largest", "rpnet_cc_keep_largest") and reaches(defs, "keep_largest", "rpnet_cc_workspace_bytes")
    assert reaches(defs, "label_components", "rpnet_cc_label") and not reaches(defs, "label_components", "rpnet_cc_keep_largest")
    assert reaches(defs, "VolumeSegmenter", "rpnet_cc_keep_largest") and reaches(defs, "evaluate_dataset", "rpnet_cc_keep_largest")
    assert not reaches(defs, "components_figures", "rpnet_cc_keep_largest") and not reaches(defs, "surface_tally", "rpnet_cc_label")
