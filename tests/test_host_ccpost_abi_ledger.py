"""No untested post-processing entry point: tests/ccpost_abi_ledger.py names, for every symbol of include/rpnet_ccpost_abi.h, the GPU
test(s) that exercise it.  The rules and the machinery are those of tests/test_host_abi_ledger.py and its followers (whose headers
these additions leave as they were); runs without a GPU."""
import ctypes
import os
import re

from rpnet_amd import hip
from tests import ccpost_abi_ledger as L
from tests.test_host_abi_ledger import ROOT, gpu_tests, header_symbols, package_defs, reaches
from tests.test_host_guard_abi_ledger import _symbols

HEADER = os.path.join(ROOT, "include", "rpnet_ccpost_abi.h")
EARLIER = (("rpnet_eval_abi.h", hip.EVAL_ABI_SYMBOLS), ("rpnet_optim_abi.h", hip.OPTIM_ABI_SYMBOLS), ("rpnet_guard_abi.h", hip.GUARD_ABI_SYMBOLS),
           ("rpnet_surface_abi.h", hip.SURFACE_ABI_SYMBOLS), ("rpnet_cc_abi.h", hip.CC_ABI_SYMBOLS),
           ("rpnet_surface_spacing_abi.h", hip.SURFACE_SPACING_ABI_SYMBOLS))


def test_ledger_keys_are_the_header_symbols_and_the_binding_knows_them():
    syms = _symbols(HEADER)
    assert syms == {"rpnet_ccpost_abi_version", "rpnet_ccpost_workspace_bytes", "rpnet_ccpost_fill_holes", "rpnet_ccpost_remove_small"}
    covered, exempt = set(L.COVERED_BY), set(L.EXEMPT)
    assert not (covered & exempt)
    assert covered | exempt == syms, (sorted(syms - covered - exempt), sorted((covered | exempt) - syms))
    assert set(L.VIA) <= covered
    assert all(isinstance(r, str) and len(r) > 20 for r in L.EXEMPT.values())
    assert set(hip.CCPOST_ABI_SYMBOLS) == syms
    # one name, one header: nothing here is also declared in one of the earlier headers
    assert not (syms & header_symbols()) and not (syms & set(hip.ABI_SYMBOLS))
    for other, known in EARLIER:
        assert not (syms & _symbols(os.path.join(ROOT, "include", other))) and not (syms & set(known)), other
    # and the component header still declares exactly its four
    assert _symbols(os.path.join(ROOT, "include", "rpnet_cc_abi.h")) == set(hip.CC_ABI_SYMBOLS) and len(hip.CC_ABI_SYMBOLS) == 4


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(hip.lib_path())
    for name in _symbols(HEADER):
        assert hasattr(lib, name), f"{name} declared in rpnet_ccpost_abi.h but not exported"
    hdr = open(HEADER).read()
    lib.rpnet_ccpost_abi_version.restype = ctypes.c_int
    assert lib.rpnet_ccpost_abi_version() == hip.CCPOST_ABI_VERSION == int(re.search(r"#define RPNET_CCPOST_ABI_VERSION (\d+)", hdr).group(1))
    cc = open(os.path.join(ROOT, "include", "rpnet_cc_abi.h")).read()
    for name in ("STATS_ROW", "COUNTS_ROW", "OVERRUN_OFFSET"):          # the tables and the head have the shape of the component ABI's
        assert re.search(r"#define RPNET_CCPOST_%s (\d+)" % name, hdr).group(1) == re.search(r"#define RPNET_CC_%s (\d+)" % name, cc).group(1)
    from rpnet_amd import postprocess as PP
    assert (PP.STATS_ROW, PP.COUNTS_ROW, PP.OVERRUN_OFFSET) == tuple(
        int(re.search(r"#define RPNET_CCPOST_%s (\d+)" % n, hdr).group(1)) for n in ("STATS_ROW", "COUNTS_ROW", "OVERRUN_OFFSET"))
    loaded = hip.load()
    assert loaded.rpnet_version() == hip.ABI_VERSION and loaded.rpnet_cc_abi_version() == hip.CC_ABI_VERSION
    # the size query needs no GPU
    assert loaded.rpnet_ccpost_workspace_bytes(2, 3, 5) == 64 + 2 * 128 and loaded.rpnet_ccpost_workspace_bytes(0, 3, 5) == 0
    assert loaded.rpnet_last_error_string().decode().startswith("ccpost: D=0")


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
    assert reaches(defs, "fill_holes", "rpnet_ccpost_fill_holes") and reaches(defs, "fill_holes", "rpnet_ccpost_workspace_bytes")
    assert reaches(defs, "remove_small", "rpnet_ccpost_remove_small") and not reaches(defs, "keep_largest", "rpnet_ccpost_fill_holes")
    assert not reaches(defs, "label_components", "rpnet_ccpost_remove_small")
    assert reaches(defs, "VolumeSegmenter", "rpnet_ccpost_fill_holes") and reaches(defs, "VolumeSegmenter", "rpnet_ccpost_remove_small")
    assert not reaches(defs, "holes_figures", "rpnet_ccpost_fill_holes") and not reaches(defs, "min_voxels_from_mm3", "rpnet_ccpost_remove_small")
