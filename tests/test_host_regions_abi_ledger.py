"""No untested region-statistics entry point: tests/regions_abi_ledger.py names, for every symbol of include/rpnet_region_abi.h, the GPU
test(s) that exercise it.  The rules and the machinery are those of tests/test_host_abi_ledger.py and its followers (whose headers and
tables this addition leaves as they were); runs without a GPU."""
import ast
import ctypes
import glob
import os
import re

from rpnet_amd import hip
from rpnet_amd import regions as R
from tests import regions_abi_ledger as L
from tests.test_host_abi_ledger import ROOT, gpu_tests, header_symbols, package_defs, reaches
from tests.test_host_guard_abi_ledger import _symbols

HEADER = os.path.join(ROOT, "include", "rpnet_region_abi.h")
EARLIER = (hip.ALL_SIDE_ABIS + hip.SIDE_ABIS_AFTER_PREP + hip.SIDE_ABIS_AFTER_RESAMPLE + hip.SIDE_ABIS_AFTER_SMOOTH
           + hip.SIDE_ABIS_AFTER_VOLLOAD + hip.SIDE_ABIS_AFTER_DEEDS)
EVERY_SIDE_ABI = EARLIER + hip.SIDE_ABIS_AFTER_FUSION


def test_ledger_keys_are_the_header_symbols_and_the_binding_knows_them():
    syms = _symbols(HEADER)
    assert syms == {"rpnet_region_abi_version", "rpnet_region_workspace_bytes", "rpnet_region_stats"}
    covered, exempt = set(L.COVERED_BY), set(L.EXEMPT)
    assert not (covered & exempt)
    assert covered | exempt == syms, (sorted(syms - covered - exempt), sorted((covered | exempt) - syms))
    assert set(L.VIA) <= covered
    assert all(isinstance(r, str) and len(r) > 20 for r in L.EXEMPT.values())
    assert set(hip.REGION_ABI_SYMBOLS) == syms
    # one name, one header: nothing here is also declared in one of the earlier headers, and those still declare what they did
    assert not (syms & header_symbols()) and not (syms & set(hip.ABI_SYMBOLS))
    for header, _, _, _, sigs in EARLIER:
        theirs = _symbols(os.path.join(ROOT, "include", header))
        assert not (syms & theirs) and theirs == set(sigs), header


def test_the_fifteenth_family_is_bound_and_checked_like_the_tables():
    """the earlier tables are what they were, in length and last row; the fifteenth family stands behind them in a table of the same form
    that load() binds with them; the fifteen families are disjoint and every version macro equals the binding's"""
    assert len(hip.ALL_SIDE_ABIS) == 9 and len(hip.SIDE_ABIS_AFTER_PREP) == 1 and len(hip.SIDE_ABIS_AFTER_RESAMPLE) == 1
    assert len(hip.SIDE_ABIS_AFTER_SMOOTH) == 1 and len(hip.SIDE_ABIS_AFTER_VOLLOAD) == 1 and len(hip.SIDE_ABIS_AFTER_DEEDS) == 1
    assert hip.SIDE_ABIS_AFTER_DEEDS[-1][0] == "rpnet_fusion_abi.h" and hip.SIDE_ABIS_AFTER_DEEDS[-1][4] is hip._FUSION_SIGS
    assert len(hip._FUSION_SIGS) == 4
    assert len(hip.SIDE_ABIS_AFTER_FUSION) == 1 and len(EVERY_SIDE_ABI) == 15
    last = hip.SIDE_ABIS_AFTER_FUSION[-1]
    assert last[0] == "rpnet_region_abi.h" and last[4] is hip._REGION_SIGS and last[3] == hip.REGION_ABI_VERSION
    assert tuple(hip._REGION_SIGS) == hip.REGION_ABI_SYMBOLS
    seen = set(hip.ABI_SYMBOLS)
    for header, words, version_symbol, version, sigs in EVERY_SIDE_ABI:
        path = os.path.join(ROOT, "include", header)
        macro = re.search(r"#define %s (\d+)" % version_symbol.upper(), open(path).read())
        assert macro is not None and int(macro.group(1)) == version, (header, version_symbol)
        assert words and version_symbol in sigs and set(sigs) == _symbols(path), header
        assert not (set(sigs) & seen), (header, sorted(set(sigs) & seen))
        seen |= set(sigs)
    lib = hip.load()
    for name, (res, args) in hip._REGION_SIGS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(hip.lib_path())
    for name in _symbols(HEADER):
        assert hasattr(lib, name), f"{name} declared in rpnet_region_abi.h but not exported"
    hdr = open(HEADER).read()
    lib.rpnet_region_abi_version.restype = ctypes.c_int
    assert lib.rpnet_region_abi_version() == hip.REGION_ABI_VERSION == int(re.search(r"#define RPNET_REGION_ABI_VERSION (\d+)", hdr).group(1))
    macro = lambda n: int(re.search(r"#define RPNET_REGION_%s (\d+)" % n, hdr).group(1))  # noqa: E731
    assert (macro("MAX_LABELS"), macro("IROW"), macro("FROW"), macro("CHUNK"), macro("MAX_BLOCKS"), macro("HEAD_BYTES"), macro("OUTSIDE_OFFSET")) == (
        R.MAX_LABELS, R.IROW, R.FROW, R.CHUNK, R.MAX_BLOCKS, R.HEAD_BYTES, R.OUTSIDE_OFFSET) == (256, 20, 2, 4096, 1024, 64, 0)
    cc = open(os.path.join(ROOT, "include", "rpnet_cc_abi.h")).read()
    prep = open(os.path.join(ROOT, "include", "rpnet_prep_abi.h")).read()
    assert R.MAX_DIM == int(re.search(r"#define RPNET_CC_MAX_DIM (\d+)", cc).group(1))
    import torch
    assert R.IMAGE_KINDS == {torch.float32: int(re.search(r"#define RPNET_PREP_F32 (\d+)", prep).group(1)),
                             torch.int16: int(re.search(r"#define RPNET_PREP_I16 (\d+)", prep).group(1))}
    loaded = hip.load()
    assert loaded.rpnet_version() == hip.ABI_VERSION and loaded.rpnet_region_abi_version() == hip.REGION_ABI_VERSION
    # the size query needs no GPU, and its formula is the header's
    assert "rpnet_region_workspace_bytes = 64 + 160 * L + 16 * G * L" in hdr
    for D, H, W in ((1, 1, 1), (1, 1, 17), (3, 9, 13), (64, 256, 256), (5, 1024, 821), (1024, 1024, 1024)):
        for n_labels in (1, 2, 5, 256):
            assert loaded.rpnet_region_workspace_bytes(D, H, W, n_labels) == R._workspace_layout(D, H, W, n_labels)[1], (D, H, W, n_labels)
    assert R._workspace_layout(3, 9, 13, 5) == ((64, 64 + 800), 64 + 800 + 80)
    assert R._workspace_layout(5, 1024, 821, 4) == ((64, 64 + 640), 64 + 640 + 16 * 1024 * 4)
    for bad in ((0, 1, 1, 1), (1, 1025, 1, 1), (1, 1, 1, 0), (1, 1, 1, 257)):
        assert loaded.rpnet_region_workspace_bytes(*bad) == 0
        assert loaded.rpnet_last_error_string().decode() == (
            "region_workspace_bytes: D=%d H=%d W=%d L=%d (every extent 1..1024, L 1..256)" % bad)


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
    assert reaches(defs, "region_stats", "rpnet_region_stats") and reaches(defs, "region_stats", "rpnet_region_workspace_bytes")
    assert reaches(defs, "region_workspace", "rpnet_region_workspace_bytes") and not reaches(defs, "region_outside", "rpnet_region_stats")
    assert reaches(defs, "VolumeSegmenter", "rpnet_region_stats") and reaches(defs, "evaluate_dataset", "rpnet_region_stats")
    assert not reaches(defs, "key_to_float", "rpnet_region_stats") and not reaches(defs, "_volume_of", "rpnet_region_stats")
    assert not reaches(defs, "_region_workspace_layout", "rpnet_region_stats")
    # every new top-level name of the package is new to it: package_defs is keyed by the bare name
    names = [n.name for path in glob.glob(os.path.join(ROOT, "rpnet_amd", "**", "*.py"), recursive=True)
             for n in ast.parse(open(path).read()).body if isinstance(n, (ast.FunctionDef, ast.ClassDef))]
    for name in ("region_stats", "derive", "compare", "region_workspace", "region_outside", "check_region_labels", "key_to_float",
                 "check_regions_out", "region_figures", "region_line_suffix", "region_mean_suffix", "_region_workspace_layout", "_volume_of"):
        assert names.count(name) == 1, name
    for name in ("fuse", "check_spacing", "_workspace_layout"):
        assert names.count(name) == 1, name
