"""No untested volume-loading entry point: tests/volload_abi_ledger.py names, for every symbol of include/rpnet_volload_abi.h, the GPU
test(s) that exercise it.  The rules and the machinery are those of tests/test_host_abi_ledger.py and its followers (whose headers and
tables this addition leaves as they were); runs without a GPU."""
import ast
import ctypes
import glob
import os
import re

import torch

from rpnet_amd import hip
from rpnet_amd import volume_load as VL
from tests import volload_abi_ledger as L
from tests.test_host_abi_ledger import ROOT, gpu_tests, header_symbols, package_defs, reaches
from tests.test_host_guard_abi_ledger import _symbols

HEADER = os.path.join(ROOT, "include", "rpnet_volload_abi.h")
EARLIER = hip.ALL_SIDE_ABIS + hip.SIDE_ABIS_AFTER_PREP + hip.SIDE_ABIS_AFTER_RESAMPLE
EVERY_SIDE_ABI = EARLIER + hip.SIDE_ABIS_AFTER_SMOOTH


def test_ledger_keys_are_the_header_symbols_and_the_binding_knows_them():
    syms = _symbols(HEADER)
    assert syms == {"rpnet_volload_abi_version", "rpnet_volload_select_workspace_bytes", "rpnet_volload_range", "rpnet_volload_gather",
                    "rpnet_volload_select", "rpnet_volload_normalize"}
    covered, exempt = set(L.COVERED_BY), set(L.EXEMPT)
    assert not (covered & exempt)
    assert covered | exempt == syms, (sorted(syms - covered - exempt), sorted((covered | exempt) - syms))
    assert set(L.VIA) <= covered
    assert all(isinstance(r, str) and len(r) > 20 for r in L.EXEMPT.values())
    assert set(hip.VOLLOAD_ABI_SYMBOLS) == syms
    # one name, one header: nothing here is also declared in one of the earlier headers, and those still declare what they did
    assert not (syms & header_symbols()) and not (syms & set(hip.ABI_SYMBOLS))
    for header, _, _, _, sigs in EARLIER:
        theirs = _symbols(os.path.join(ROOT, "include", header))
        assert not (syms & theirs) and theirs == set(sigs), header


def test_the_twelfth_family_is_bound_and_checked_like_the_tables():
    """the four earlier tables are what they were, in length and last row; the twelfth family stands behind them in a table of the same
    form that load() binds with them; the twelve families are disjoint and every version macro equals the binding's"""
    assert hip.ALL_SIDE_ABIS == hip.SIDE_ABIS + hip.LATER_SIDE_ABIS and len(hip.ALL_SIDE_ABIS) == 9 and len(hip.SIDE_ABIS) == 8
    assert hip.SIDE_ABIS[-1][0] == "rpnet_morph_abi.h" and hip.ALL_SIDE_ABIS[-1][0] == "rpnet_prep_abi.h"
    assert len(hip.SIDE_ABIS_AFTER_PREP) == 1 and hip.SIDE_ABIS_AFTER_PREP[-1][0] == "rpnet_resample_abi.h"
    assert len(hip.SIDE_ABIS_AFTER_RESAMPLE) == 1 and hip.SIDE_ABIS_AFTER_RESAMPLE[-1][0] == "rpnet_smooth_abi.h"
    assert hip.SIDE_ABIS_AFTER_RESAMPLE[-1][4] is hip._SMOOTH_SIGS and len(hip._SMOOTH_SIGS) == 3
    assert len(hip.SIDE_ABIS_AFTER_SMOOTH) == 1 and len(EVERY_SIDE_ABI) == 12
    last = hip.SIDE_ABIS_AFTER_SMOOTH[-1]
    assert last[0] == "rpnet_volload_abi.h" and last[4] is hip._VOLLOAD_SIGS and last[3] == hip.VOLLOAD_ABI_VERSION
    assert tuple(hip._VOLLOAD_SIGS) == hip.VOLLOAD_ABI_SYMBOLS
    seen = set(hip.ABI_SYMBOLS)
    for header, words, version_symbol, version, sigs in EVERY_SIDE_ABI:
        path = os.path.join(ROOT, "include", header)
        macro = re.search(r"#define %s (\d+)" % version_symbol.upper(), open(path).read())
        assert macro is not None and int(macro.group(1)) == version, (header, version_symbol)
        assert words and version_symbol in sigs and set(sigs) == _symbols(path), header
        assert not (set(sigs) & seen), (header, sorted(set(sigs) & seen))
        seen |= set(sigs)
    lib = hip.load()
    for name, (res, args) in hip._VOLLOAD_SIGS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(hip.lib_path())
    for name in _symbols(HEADER):
        assert hasattr(lib, name), f"{name} declared in rpnet_volload_abi.h but not exported"
    hdr = open(HEADER).read()
    lib.rpnet_volload_abi_version.restype = ctypes.c_int
    assert lib.rpnet_volload_abi_version() == hip.VOLLOAD_ABI_VERSION == int(re.search(r"#define RPNET_VOLLOAD_ABI_VERSION (\d+)", hdr).group(1))
    macro = lambda n: int(re.search(r"#define RPNET_VOLLOAD_%s (\d+)" % n, hdr).group(1))  # noqa: E731
    assert (VL.X_FASTEST, VL.Z_FASTEST, VL.MAX_VALUES, VL.SELECT_BLOCKS) == (macro("X_FASTEST"), macro("Z_FASTEST"), macro("MAX_N"), macro("SELECT_BLOCKS"))
    assert VL.SELECT_SWEEP == VL.SELECT_BLOCKS * 256 * 4 and VL.MAX_VALUES == 1024 ** 3
    prep = open(os.path.join(ROOT, "include", "rpnet_prep_abi.h")).read()
    kinds = tuple(int(re.search(r"#define RPNET_PREP_%s (\d+)" % n, prep).group(1)) for n in ("F32", "I16"))
    assert (VL.SOURCE_KINDS[torch.float32], VL.SOURCE_KINDS[torch.int16], VL.SOURCE_KINDS[torch.uint8]) == kinds + (macro("U8"),) == (0, 1, 2)
    cc = open(os.path.join(ROOT, "include", "rpnet_cc_abi.h")).read()
    assert VL.MAX_EXTENT == int(re.search(r"#define RPNET_CC_MAX_DIM (\d+)", cc).group(1)) == 1024
    loaded = hip.load()
    assert loaded.rpnet_version() == hip.ABI_VERSION and loaded.rpnet_volload_abi_version() == hip.VOLLOAD_ABI_VERSION
    # the size query needs no GPU, and its formula is the header's
    assert "rpnet_volload_select_workspace_bytes = 64 + 4 * 2 * 256 * 4" in hdr
    for n in (1, 2, 201, 64 * 256 * 256, 1024 ** 3):
        assert loaded.rpnet_volload_select_workspace_bytes(n) == 64 + 4 * 2 * 256 * 4, n
    for bad in (0, 1024 ** 3 + 1):
        assert loaded.rpnet_volload_select_workspace_bytes(bad) == 0
        assert loaded.rpnet_last_error_string().decode() == f"volload_select: n={bad} (1..1073741824 values)"


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
    assert reaches(defs, "window_normalize", "rpnet_volload_normalize") and reaches(defs, "window_normalize", "rpnet_volload_select")
    assert reaches(defs, "percentile_f32", "rpnet_volload_select") and not reaches(defs, "percentile_f32", "rpnet_volload_normalize")
    assert not reaches(defs, "order_statistics", "rpnet_volload_gather") and not reaches(defs, "gather_volume", "rpnet_volload_range")
    assert not reaches(defs, "load_geometry", "rpnet_volload_gather") and not reaches(defs, "percentile_rank", "rpnet_volload_select")
    for sym in hip.VOLLOAD_ABI_SYMBOLS[1:]:
        assert reaches(defs, "DeviceVolumeLoader", sym) and reaches(defs, "DeviceEpisodeSource", sym) and reaches(defs, "DeviceEvalSource", sym), sym
        assert not reaches(defs, "smooth_image", sym) and not reaches(defs, "FewshotVolumeReader", sym), sym
    assert not reaches(defs, "DeviceVolumeLoader", "rpnet_smooth_image")
    # every new top-level name of the package is new to it: package_defs is keyed by the bare name
    names = [n.name for path in glob.glob(os.path.join(ROOT, "rpnet_amd", "**", "*.py"), recursive=True)
             for n in ast.parse(open(path).read()).body if isinstance(n, (ast.FunctionDef, ast.ClassDef))]
    for name in ("load_geometry", "_source", "_window_args", "annotated_range", "gather_volume", "_flat_f32", "order_statistics", "percentile_rank",
                 "percentile_f32", "window_normalize", "read_payload", "upload_payload", "DeviceVolumeLoader"):
        assert names.count(name) == 1, name
