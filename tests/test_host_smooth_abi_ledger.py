"""No untested smoothing entry point: tests/smooth_abi_ledger.py names, for every symbol of include/rpnet_smooth_abi.h, the GPU test(s)
that exercise it.  The rules and the machinery are those of tests/test_host_abi_ledger.py and its followers (whose headers and tables this
addition leaves as they were); runs without a GPU."""
import ctypes
import os
import re

import numpy as np
import torch

from rpnet_amd import hip
from rpnet_amd import smooth as SM
from tests import smooth_abi_ledger as L
from tests import smooth_cases as SC
from tests.test_host_abi_ledger import ROOT, gpu_tests, header_symbols, package_defs, reaches
from tests.test_host_guard_abi_ledger import _symbols

HEADER = os.path.join(ROOT, "include", "rpnet_smooth_abi.h")
EVERY_SIDE_ABI = hip.ALL_SIDE_ABIS + hip.SIDE_ABIS_AFTER_PREP + hip.SIDE_ABIS_AFTER_RESAMPLE


def test_ledger_keys_are_the_header_symbols_and_the_binding_knows_them():
    syms = _symbols(HEADER)
    assert syms == {"rpnet_smooth_abi_version", "rpnet_smooth_workspace_bytes", "rpnet_smooth_image"}
    covered, exempt = set(L.COVERED_BY), set(L.EXEMPT)
    assert not (covered & exempt)
    assert covered | exempt == syms, (sorted(syms - covered - exempt), sorted((covered | exempt) - syms))
    assert set(L.VIA) <= covered
    assert all(isinstance(r, str) and len(r) > 20 for r in L.EXEMPT.values())
    assert set(hip.SMOOTH_ABI_SYMBOLS) == syms
    # one name, one header: nothing here is also declared in one of the earlier headers, and those still declare what they did
    assert not (syms & header_symbols()) and not (syms & set(hip.ABI_SYMBOLS))
    for header, _, _, _, sigs in hip.ALL_SIDE_ABIS + hip.SIDE_ABIS_AFTER_PREP:
        theirs = _symbols(os.path.join(ROOT, "include", header))
        assert not (syms & theirs) and theirs == set(sigs), header


def test_the_eleventh_family_is_bound_and_checked_like_the_tables():
    """the three earlier tables are what they were, in length and last row; the eleventh family stands behind them in a table of the same
    form that load() binds with them; what tests/test_host_side_abi_table.py asserts over SIDE_ABIS holds over all eleven"""
    assert hip.ALL_SIDE_ABIS == hip.SIDE_ABIS + hip.LATER_SIDE_ABIS and len(hip.ALL_SIDE_ABIS) == 9 and len(hip.SIDE_ABIS) == 8
    assert hip.SIDE_ABIS[-1][0] == "rpnet_morph_abi.h" and hip.ALL_SIDE_ABIS[-1][0] == "rpnet_prep_abi.h"
    assert len(hip.SIDE_ABIS_AFTER_PREP) == 1 and hip.SIDE_ABIS_AFTER_PREP[-1][0] == "rpnet_resample_abi.h"
    assert hip.SIDE_ABIS_AFTER_PREP[-1][4] is hip._RESAMPLE_SIGS and len(hip._RESAMPLE_SIGS) == 4
    assert len(hip.SIDE_ABIS_AFTER_RESAMPLE) == 1 and len(EVERY_SIDE_ABI) == 11
    last = hip.SIDE_ABIS_AFTER_RESAMPLE[-1]
    assert last[0] == "rpnet_smooth_abi.h" and last[4] is hip._SMOOTH_SIGS and last[3] == hip.SMOOTH_ABI_VERSION
    assert tuple(hip._SMOOTH_SIGS) == hip.SMOOTH_ABI_SYMBOLS
    seen = set(hip.ABI_SYMBOLS)
    for header, words, version_symbol, version, sigs in EVERY_SIDE_ABI:
        path = os.path.join(ROOT, "include", header)
        macro = re.search(r"#define %s (\d+)" % version_symbol.upper(), open(path).read())
        assert macro is not None and int(macro.group(1)) == version, (header, version_symbol)
        assert words and version_symbol in sigs and set(sigs) == _symbols(path), header
        assert not (set(sigs) & seen), (header, sorted(set(sigs) & seen))
        seen |= set(sigs)
    # load() went through all eleven: every symbol of the family carries the signature of the binding
    lib = hip.load()
    for name, (res, args) in hip._SMOOTH_SIGS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(hip.lib_path())
    for name in _symbols(HEADER):
        assert hasattr(lib, name), f"{name} declared in rpnet_smooth_abi.h but not exported"
    hdr = open(HEADER).read()
    lib.rpnet_smooth_abi_version.restype = ctypes.c_int
    assert lib.rpnet_smooth_abi_version() == hip.SMOOTH_ABI_VERSION == int(re.search(r"#define RPNET_SMOOTH_ABI_VERSION (\d+)", hdr).group(1))
    macro = lambda n: int(re.search(r"#define RPNET_SMOOTH_%s (\d+)" % n, hdr).group(1))  # noqa: E731
    assert (SM.REFLECT, SM.CLAMP, SM.MAX_RADIUS) == (macro("REFLECT"), macro("NEAREST"), macro("MAX_RADIUS")) == (0, 1, 255)
    assert SM.BORDERS == {"reflect": SM.REFLECT, "nearest": SM.CLAMP}
    prep = open(os.path.join(ROOT, "include", "rpnet_prep_abi.h")).read()
    kinds = tuple(int(re.search(r"#define RPNET_PREP_%s (\d+)" % n, prep).group(1)) for n in ("F32", "I16"))
    assert (SM.VOLUME_KINDS[torch.float32], SM.VOLUME_KINDS[torch.int16]) == kinds
    cc = open(os.path.join(ROOT, "include", "rpnet_cc_abi.h")).read()
    assert SM.MAX_EXTENT == int(re.search(r"#define RPNET_CC_MAX_DIM (\d+)", cc).group(1)) == 1024
    # the tiles the kernels are built with are the ones Python exports and the cases are placed by
    src = open(os.path.join(ROOT, "rpnet_amd", "csrc", "smooth.hip")).read()
    const = lambda n: int(re.search(r"constexpr int %s = (\d+);" % n, src).group(1))  # noqa: E731
    for dtype, run in SM.LANE_RUN.items():
        size = torch.empty((), dtype=dtype).element_size()
        d = np.dtype(str(dtype)[6:])
        assert run * size == const("kSmoothRunBytes") == 16 and SM.X_TILE[dtype] == 64 * run and SM.AXIS_SEG[dtype] * run == const("kSmoothSegVoxels")
        assert (SC.LANE_RUN[d], SC.X_TILE[d], SC.AXIS_SEG[d]) == (run, SM.X_TILE[dtype], SM.AXIS_SEG[dtype])
    assert SM.X_ROWS == SC.X_ROWS == const("kSmoothXRows")
    loaded = hip.load()
    assert loaded.rpnet_version() == hip.ABI_VERSION and loaded.rpnet_smooth_abi_version() == hip.SMOOTH_ABI_VERSION
    # the size query needs no GPU, and its formula is the header's: a 64-byte head and B float64 volumes padded to 16 bytes
    assert "64 + 16 * ((D * H * W + 1) / 2) * B" in hdr and "B = min(2, max(0, P - 1))" in hdr
    for radii, buffers in (((0, 0, 0), 0), ((0, 3, 0), 0), ((255, 0, 0), 0), ((1, 0, 2), 1), ((0, 1, 2), 1), ((1, 2, 0), 1), ((1, 2, 3), 2)):
        assert loaded.rpnet_smooth_workspace_bytes(3, 5, 7, *radii) == 64 + 16 * ((3 * 5 * 7 + 1) // 2) * buffers, radii
    assert loaded.rpnet_smooth_workspace_bytes(1024, 1024, 1024, 1, 1, 1) == 64 + 16 * 2 ** 29 * 2
    for bad in ((0, 5, 7, 1, 1, 1), (1025, 5, 7, 1, 1, 1), (3, 0, 7, 1, 1, 1), (3, 5, 1025, 1, 1, 1), (3, 5, 7, -1, 1, 1), (3, 5, 7, 256, 1, 1),
                (3, 5, 7, 1, -1, 1), (3, 5, 7, 1, 1, 256)):
        assert loaded.rpnet_smooth_workspace_bytes(*bad) == 0
        text = loaded.rpnet_last_error_string().decode()
        assert text.startswith(f"smooth: D={bad[0]} H={bad[1]} W={bad[2]}, radii z={bad[3]} y={bad[4]} x={bad[5]}")
        assert "every extent 1..1024" in text and "every radius 0..255" in text


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
    assert reaches(defs, "smooth_image", "rpnet_smooth_image") and reaches(defs, "smooth_image", "rpnet_smooth_workspace_bytes")
    for sym in hip.RESAMPLE_ABI_SYMBOLS:
        assert not reaches(defs, "smooth_image", sym), sym
    for start in ("resample_image", "resample_to_spacing", "resample_like"):
        assert reaches(defs, start, "rpnet_smooth_image") and reaches(defs, start, "rpnet_resample_image"), start
    assert not reaches(defs, "resample_image", "rpnet_resample_labels") and not reaches(defs, "resample_labels", "rpnet_smooth_image")
    assert not reaches(defs, "smooth_weights", "rpnet_smooth_image") and not reaches(defs, "antialias_sigma", "rpnet_smooth_image")
    assert not reaches(defs, "smooth_image", "rpnet_prep_threshold") and not reaches(defs, "clean_volume", "rpnet_smooth_image")
    # every new top-level name of the package is new to it: package_defs is keyed by the bare name
    import ast
    import glob
    names = [n.name for path in glob.glob(os.path.join(ROOT, "rpnet_amd", "**", "*.py"), recursive=True)
             for n in ast.parse(open(path).read()).body if isinstance(n, (ast.FunctionDef, ast.ClassDef))]
    for name in ("smooth_radius", "smooth_weights", "smooth_device_weights", "_smooth_sigmas", "antialias_sigma", "smooth_image", "_antialiased"):
        assert names.count(name) == 1, name
