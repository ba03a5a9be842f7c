"""No untested per-component statistics entry point: tests/compstat_abi_ledger.py names, for every symbol of
include/rpnet_compstat_abi.h, the GPU test(s) that exercise it.  The rules and the machinery are those of tests/test_host_abi_ledger.py
and its followers (whose headers and tables this addition leaves as they were); runs without a GPU."""
import ast
import ctypes
import glob
import os
import re

from rpnet_amd import component_stats as CS
from rpnet_amd import hip
from tests import compstat_abi_ledger as L
from tests.test_host_abi_ledger import ROOT, gpu_tests, header_symbols, package_defs, reaches
from tests.test_host_guard_abi_ledger import _symbols

HEADER = os.path.join(ROOT, "include", "rpnet_compstat_abi.h")
EARLIER = (hip.ALL_SIDE_ABIS + hip.SIDE_ABIS_AFTER_PREP + hip.SIDE_ABIS_AFTER_RESAMPLE + hip.SIDE_ABIS_AFTER_SMOOTH
           + hip.SIDE_ABIS_AFTER_VOLLOAD + hip.SIDE_ABIS_AFTER_DEEDS + hip.SIDE_ABIS_AFTER_FUSION)
EVERY_SIDE_ABI = EARLIER + hip.SIDE_ABIS_AFTER_REGIONS


def test_ledger_keys_are_the_header_symbols_and_the_binding_knows_them():
    syms = _symbols(HEADER)
    assert syms == {"rpnet_compstat_abi_version", "rpnet_compstat_workspace_bytes", "rpnet_compstat_rank", "rpnet_compstat_table"}
    covered, exempt = set(L.COVERED_BY), set(L.EXEMPT)
    assert not (covered & exempt)
    assert covered | exempt == syms, (sorted(syms - covered - exempt), sorted((covered | exempt) - syms))
    assert set(L.VIA) <= covered
    assert all(isinstance(r, str) and len(r) > 20 for r in L.EXEMPT.values())
    assert set(hip.COMPSTAT_ABI_SYMBOLS) == syms
    # one name, one header: nothing here is also declared in one of the earlier headers, and those still declare what they did
    assert not (syms & header_symbols()) and not (syms & set(hip.ABI_SYMBOLS))
    for header, _, _, _, sigs in EARLIER:
        theirs = _symbols(os.path.join(ROOT, "include", header))
        assert not (syms & theirs) and theirs == set(sigs), header


def test_the_sixteenth_family_is_bound_and_checked_like_the_tables():
    """the earlier tables are what they were, in length and last row; the sixteenth family stands behind them in a table of the same form
    that load() binds with them; the sixteen families are disjoint and every version macro equals the binding's"""
    assert len(hip.ALL_SIDE_ABIS) == 9 and len(hip.SIDE_ABIS_AFTER_PREP) == 1 and len(hip.SIDE_ABIS_AFTER_RESAMPLE) == 1
    assert len(hip.SIDE_ABIS_AFTER_SMOOTH) == 1 and len(hip.SIDE_ABIS_AFTER_VOLLOAD) == 1 and len(hip.SIDE_ABIS_AFTER_DEEDS) == 1
    assert len(hip.SIDE_ABIS_AFTER_FUSION) == 1
    assert hip.SIDE_ABIS_AFTER_FUSION[-1][0] == "rpnet_region_abi.h" and hip.SIDE_ABIS_AFTER_FUSION[-1][4] is hip._REGION_SIGS
    assert len(hip._REGION_SIGS) == 3
    assert len(hip.SIDE_ABIS_AFTER_REGIONS) == 1 and len(EVERY_SIDE_ABI) == 16
    last = hip.SIDE_ABIS_AFTER_REGIONS[-1]
    assert last[0] == "rpnet_compstat_abi.h" and last[4] is hip._COMPSTAT_SIGS and last[3] == hip.COMPSTAT_ABI_VERSION
    assert tuple(hip._COMPSTAT_SIGS) == hip.COMPSTAT_ABI_SYMBOLS
    seen = set(hip.ABI_SYMBOLS)
    for header, words, version_symbol, version, sigs in EVERY_SIDE_ABI:
        path = os.path.join(ROOT, "include", header)
        macro = re.search(r"#define %s (\d+)" % version_symbol.upper(), open(path).read())
        assert macro is not None and int(macro.group(1)) == version, (header, version_symbol)
        assert words and version_symbol in sigs and set(sigs) == _symbols(path), header
        assert not (set(sigs) & seen), (header, sorted(set(sigs) & seen))
        seen |= set(sigs)
    lib = hip.load()
    for name, (res, args) in hip._COMPSTAT_SIGS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(hip.lib_path())
    for name in _symbols(HEADER):
        assert hasattr(lib, name), f"{name} declared in rpnet_compstat_abi.h but not exported"
    hdr = open(HEADER).read()
    lib.rpnet_compstat_abi_version.restype = ctypes.c_int
    assert lib.rpnet_compstat_abi_version() == hip.COMPSTAT_ABI_VERSION == int(re.search(r"#define RPNET_COMPSTAT_ABI_VERSION (\d+)", hdr).group(1))
    macro = lambda n: int(re.search(r"#define RPNET_COMPSTAT_%s (\d+)" % n, hdr).group(1))  # noqa: E731
    assert (macro("MAX_COMPONENTS"), macro("ROW"), macro("STATS_ROW"), macro("CHUNK"), macro("HEAD_BYTES"), macro("MAX_SCALE_LOG2")) == (
        CS.MAX_COMPONENTS, CS.COMP_ROW, CS.COMP_STATS_ROW, CS.COMP_CHUNK, CS.COMP_HEAD_BYTES, CS.MAX_SCALE_LOG2) == (65536, 24, 4, 4096, 64, 30)
    assert (macro("COUNT_OFFSET"), macro("INVALID_OFFSET"), macro("BEYOND_OFFSET"), macro("TABLE_INVALID_OFFSET")) == (
        CS.COUNT_OFFSET, CS.INVALID_OFFSET, CS.BEYOND_OFFSET, CS.TABLE_INVALID_OFFSET) == (0, 8, 16, 24)
    assert CS.HEAD_WORDS * 8 <= CS.COMP_HEAD_BYTES and (macro("SCAN_THREADS"), macro("SLOTS")) == (256, 128)
    region = open(os.path.join(ROOT, "include", "rpnet_region_abi.h")).read()
    cc = open(os.path.join(ROOT, "include", "rpnet_cc_abi.h")).read()
    assert CS.COMP_CHUNK == int(re.search(r"#define RPNET_REGION_CHUNK (\d+)", region).group(1))
    assert CS.MAX_DIM == int(re.search(r"#define RPNET_CC_MAX_DIM (\d+)", cc).group(1))
    loaded = hip.load()
    assert loaded.rpnet_version() == hip.ABI_VERSION and loaded.rpnet_compstat_abi_version() == hip.COMPSTAT_ABI_VERSION
    # the size query needs no GPU, and its formula is the header's
    assert "rpnet_compstat_workspace_bytes = 64 + 4 * ((nc + 3) / 4 * 4) + 4 * n" in hdr
    for D, H, W in ((1, 1, 1), (1, 1, 17), (2, 33, 65), (64, 256, 256), (257, 64, 64), (5, 1024, 821), (1024, 1024, 1024)):
        for m in (1, 7, 4096, 65536):
            assert loaded.rpnet_compstat_workspace_bytes(D, H, W, m) == CS._compstat_workspace_layout(D, H, W)[1], (D, H, W, m)
    assert CS._compstat_workspace_layout(2, 33, 65) == ((64, 80), 80 + 4 * 4290)
    for bad in ((0, 1, 1, 1), (1, 1025, 1, 1), (1, 1, 1, 0), (1, 1, 1, 65537)):
        assert loaded.rpnet_compstat_workspace_bytes(*bad) == 0
        assert loaded.rpnet_last_error_string().decode() == (
            "compstat_workspace_bytes: D=%d H=%d W=%d max_components=%d (every extent 1..1024, max_components 1..65536)" % bad)


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
    assert reaches(defs, "rank_components", "rpnet_compstat_rank") and reaches(defs, "rank_components", "rpnet_compstat_workspace_bytes")
    assert reaches(defs, "tally_components", "rpnet_compstat_table") and not reaches(defs, "tally_components", "rpnet_compstat_rank")
    assert not reaches(defs, "rank_components", "rpnet_compstat_table")
    assert reaches(defs, "component_table", "rpnet_compstat_rank") and reaches(defs, "component_table", "rpnet_compstat_table")
    assert reaches(defs, "component_table", "rpnet_cc_label")
    assert reaches(defs, "component_workspace", "rpnet_compstat_workspace_bytes") and not reaches(defs, "component_head", "rpnet_compstat_table")
    assert reaches(defs, "VolumeSegmenter", "rpnet_compstat_table") and reaches(defs, "evaluate_dataset", "rpnet_compstat_rank")
    for host_only in ("derive_components", "detection_counts", "detection_figures", "detection_line_suffix", "_compstat_workspace_layout",
                      "components_option", "check_components_out"):
        assert not reaches(defs, host_only, "rpnet_compstat_table") and not reaches(defs, host_only, "rpnet_compstat_rank"), host_only
    # every new top-level name of the package is new to it: package_defs is keyed by the bare name
    names = [n.name for path in glob.glob(os.path.join(ROOT, "rpnet_amd", "**", "*.py"), recursive=True)
             for n in ast.parse(open(path).read()).body if isinstance(n, (ast.FunctionDef, ast.ClassDef))]
    for name in ("rank_components", "tally_components", "component_table", "derive_components", "detection_counts", "component_workspace",
                 "component_head", "check_max_components", "components_option", "default_scale_log2", "check_components_out", "detection_figures",
                 "detection_line_suffix", "detection_mean_suffix", "_compstat_workspace_layout", "_take_workspace", "_check_extents", "_detected"):
        assert names.count(name) == 1, name
    for name in ("derive", "compare", "fuse", "_workspace_layout", "region_stats", "components_figures", "label_components"):
        assert names.count(name) == 1, name
