"""No untested resampling entry point: tests/resample_abi_ledger.py names, for every symbol of include/rpnet_resample_abi.h, the GPU
test(s) that exercise it.  The rules and the machinery are those of tests/test_host_abi_ledger.py and its followers (whose headers this
addition leaves as they were); runs without a GPU."""
import ctypes
import os
import re

import torch

from rpnet_amd import hip
from rpnet_amd import resample as RS
from tests import resample_abi_ledger as L
from tests.test_host_abi_ledger import ROOT, gpu_tests, header_symbols, package_defs, reaches
from tests.test_host_guard_abi_ledger import _symbols

HEADER = os.path.join(ROOT, "include", "rpnet_resample_abi.h")
ENTRY = ("rpnet_resample_image", "rpnet_resample_labels")
EVERY_SIDE_ABI = hip.ALL_SIDE_ABIS + hip.SIDE_ABIS_AFTER_PREP


def test_ledger_keys_are_the_header_symbols_and_the_binding_knows_them():
    syms = _symbols(HEADER)
    assert syms == {"rpnet_resample_abi_version", "rpnet_resample_workspace_bytes"} | set(ENTRY)
    covered, exempt = set(L.COVERED_BY), set(L.EXEMPT)
    assert not (covered & exempt)
    assert covered | exempt == syms, (sorted(syms - covered - exempt), sorted((covered | exempt) - syms))
    assert set(L.VIA) <= covered
    assert all(isinstance(r, str) and len(r) > 20 for r in L.EXEMPT.values())
    assert set(hip.RESAMPLE_ABI_SYMBOLS) == syms
    # one name, one header: nothing here is also declared in one of the earlier headers, and those still declare what they did
    assert not (syms & header_symbols()) and not (syms & set(hip.ABI_SYMBOLS))
    for header, _, _, _, sigs in hip.ALL_SIDE_ABIS:
        theirs = _symbols(os.path.join(ROOT, "include", header))
        assert not (syms & theirs) and theirs == set(sigs), header


def test_the_tenth_family_is_bound_and_checked_like_the_table():
    """ALL_SIDE_ABIS is still the nine rows with the preprocessing row last; the tenth family stands behind them in a table of the same
    form that load() binds with them; what tests/test_host_side_abi_table.py asserts over SIDE_ABIS holds over all ten"""
    assert hip.ALL_SIDE_ABIS == hip.SIDE_ABIS + hip.LATER_SIDE_ABIS and len(hip.ALL_SIDE_ABIS) == 9 and len(hip.SIDE_ABIS) == 8
    assert hip.ALL_SIDE_ABIS[-1][0] == "rpnet_prep_abi.h"
    assert len(hip.SIDE_ABIS_AFTER_PREP) == 1 and len(EVERY_SIDE_ABI) == 10
    last = hip.SIDE_ABIS_AFTER_PREP[-1]
    assert last[0] == "rpnet_resample_abi.h" and last[4] is hip._RESAMPLE_SIGS and last[3] == hip.RESAMPLE_ABI_VERSION
    assert tuple(hip._RESAMPLE_SIGS) == hip.RESAMPLE_ABI_SYMBOLS
    seen = set(hip.ABI_SYMBOLS)
    for header, words, version_symbol, version, sigs in EVERY_SIDE_ABI:
        path = os.path.join(ROOT, "include", header)
        macro = re.search(r"#define %s (\d+)" % version_symbol.upper(), open(path).read())
        assert macro is not None and int(macro.group(1)) == version, (header, version_symbol)
        assert words and version_symbol in sigs and set(sigs) == _symbols(path), header
        assert not (set(sigs) & seen), (header, sorted(set(sigs) & seen))
        seen |= set(sigs)
    # load() went through all ten: every symbol of the family carries the signature of the binding
    lib = hip.load()
    for name, (res, args) in hip._RESAMPLE_SIGS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(hip.lib_path())
    for name in _symbols(HEADER):
        assert hasattr(lib, name), f"{name} declared in rpnet_resample_abi.h but not exported"
    hdr = open(HEADER).read()
    lib.rpnet_resample_abi_version.restype = ctypes.c_int
    assert lib.rpnet_resample_abi_version() == hip.RESAMPLE_ABI_VERSION == int(re.search(r"#define RPNET_RESAMPLE_ABI_VERSION (\d+)", hdr).group(1))
    macro = lambda n: int(re.search(r"#define RPNET_RESAMPLE_%s (\d+)" % n, hdr).group(1))  # noqa: E731
    assert (RS.ALIGNS["corner"], RS.ALIGNS["center"]) == (macro("CORNER"), macro("CENTER")) == (0, 1)
    assert (RS.NEAREST, RS.LINEAR, RS.STATS_ROW) == (macro("NEAREST"), macro("LINEAR"), macro("STATS_ROW")) == (0, 1, 4)
    assert RS.MODES == {"nearest": RS.NEAREST, "linear": RS.LINEAR}
    prep = open(os.path.join(ROOT, "include", "rpnet_prep_abi.h")).read()
    kinds = tuple(int(re.search(r"#define RPNET_PREP_%s (\d+)" % n, prep).group(1)) for n in ("F32", "I16"))
    assert (RS.IMAGE_KINDS[torch.float32], RS.IMAGE_KINDS[torch.int16]) == kinds
    cc = open(os.path.join(ROOT, "include", "rpnet_cc_abi.h")).read()
    assert RS.MAX_DIM == int(re.search(r"#define RPNET_CC_MAX_DIM (\d+)", cc).group(1)) == 1024
    assert all(run * torch.empty((), dtype=dtype).element_size() == 16 for dtype, run in RS.RUN.items())
    loaded = hip.load()
    assert loaded.rpnet_version() == hip.ABI_VERSION and loaded.rpnet_resample_abi_version() == hip.RESAMPLE_ABI_VERSION
    # the size query needs no GPU, and its formula is the header's: a 64-byte head and 16 bytes per output index of each axis
    assert "64 + 16 * (Do + Ho + Wo)" in hdr
    assert loaded.rpnet_resample_workspace_bytes(2, 3, 5, 7, 11, 13) == 64 + 16 * (7 + 11 + 13)
    for bad in ((0, 3, 5, 7, 11, 13), (2, 3, 5, 7, 0, 13), (1025, 3, 5, 7, 11, 13), (2, 3, 5, 7, 11, 1025)):
        assert loaded.rpnet_resample_workspace_bytes(*bad) == 0
        text = loaded.rpnet_last_error_string().decode()
        assert text.startswith(f"resample: D={bad[0]} H=3 W=5 -> D=7 H={bad[4]} W={bad[5]}") and "every extent 1..1024" in text


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
    assert reaches(defs, "resample_image", "rpnet_resample_image") and reaches(defs, "resample_image", "rpnet_resample_workspace_bytes")
    assert reaches(defs, "resample_labels", "rpnet_resample_labels") and reaches(defs, "resample_labels", "rpnet_resample_workspace_bytes")
    for sym in ENTRY:
        assert reaches(defs, "resample_to_spacing", sym) and reaches(defs, "resample_like", sym), sym
    assert not reaches(defs, "resample_image", "rpnet_resample_labels") and not reaches(defs, "resample_labels", "rpnet_resample_image")
    assert not reaches(defs, "output_shape", "rpnet_resample_image") and not reaches(defs, "out_spacing", "rpnet_resample_labels")
    assert not reaches(defs, "resample_to_spacing", "rpnet_prep_threshold") and not reaches(defs, "clean_volume", "rpnet_resample_image")
