"""No untested DEEDS registration entry point: tests/deeds_abi_ledger.py names, for every symbol of include/rpnet_deeds_abi.h, the GPU
test(s) that exercise it.  The rules and the machinery are those of tests/test_host_abi_ledger.py and its followers (whose headers and
tables this addition leaves as they were); runs without a GPU."""
import ast
import ctypes
import glob
import os
import re

from rpnet_amd import hip
from rpnet_amd import registration as R
from tests import deeds_abi_ledger as L
from tests.test_host_abi_ledger import ROOT, gpu_tests, header_symbols, package_defs, reaches
from tests.test_host_guard_abi_ledger import _symbols

HEADER = os.path.join(ROOT, "include", "rpnet_deeds_abi.h")
EARLIER = hip.ALL_SIDE_ABIS + hip.SIDE_ABIS_AFTER_PREP + hip.SIDE_ABIS_AFTER_RESAMPLE + hip.SIDE_ABIS_AFTER_SMOOTH
EVERY_SIDE_ABI = EARLIER + hip.SIDE_ABIS_AFTER_VOLLOAD


def test_ledger_keys_are_the_header_symbols_and_the_binding_knows_them():
    syms = _symbols(HEADER)
    assert syms == {"rpnet_deeds_abi_version", "rpnet_deeds_workspace_bytes", "rpnet_deeds_register", "rpnet_deeds_warp"}
    covered, exempt = set(L.COVERED_BY), set(L.EXEMPT)
    assert not (covered & exempt)
    assert covered | exempt == syms, (sorted(syms - covered - exempt), sorted((covered | exempt) - syms))
    assert set(L.VIA) <= covered
    assert all(isinstance(r, str) and len(r) > 20 for r in L.EXEMPT.values())
    assert set(hip.DEEDS_ABI_SYMBOLS) == syms
    # one name, one header: nothing here is also declared in one of the earlier headers, and those still declare what they did
    assert not (syms & header_symbols()) and not (syms & set(hip.ABI_SYMBOLS))
    for header, _, _, _, sigs in EARLIER:
        theirs = _symbols(os.path.join(ROOT, "include", header))
        assert not (syms & theirs) and theirs == set(sigs), header


def test_the_thirteenth_family_is_bound_and_checked_like_the_tables():
    """the five earlier tables are what they were, in length and last row; the thirteenth family stands behind them in a table of the
    same form that load() binds with them; the thirteen families are disjoint and every version macro equals the binding's"""
    assert hip.ALL_SIDE_ABIS == hip.SIDE_ABIS + hip.LATER_SIDE_ABIS and len(hip.ALL_SIDE_ABIS) == 9 and len(hip.SIDE_ABIS) == 8
    assert hip.SIDE_ABIS[-1][0] == "rpnet_morph_abi.h" and hip.ALL_SIDE_ABIS[-1][0] == "rpnet_prep_abi.h"
    assert len(hip.SIDE_ABIS_AFTER_PREP) == 1 and hip.SIDE_ABIS_AFTER_PREP[-1][0] == "rpnet_resample_abi.h"
    assert len(hip.SIDE_ABIS_AFTER_RESAMPLE) == 1 and hip.SIDE_ABIS_AFTER_RESAMPLE[-1][0] == "rpnet_smooth_abi.h"
    assert len(hip.SIDE_ABIS_AFTER_SMOOTH) == 1 and hip.SIDE_ABIS_AFTER_SMOOTH[-1][0] == "rpnet_volload_abi.h"
    assert hip.SIDE_ABIS_AFTER_SMOOTH[-1][4] is hip._VOLLOAD_SIGS and len(hip._VOLLOAD_SIGS) == 6
    assert len(hip.SIDE_ABIS_AFTER_VOLLOAD) == 1 and len(EVERY_SIDE_ABI) == 13
    last = hip.SIDE_ABIS_AFTER_VOLLOAD[-1]
    assert last[0] == "rpnet_deeds_abi.h" and last[4] is hip._DEEDS_SIGS and last[3] == hip.DEEDS_ABI_VERSION
    assert tuple(hip._DEEDS_SIGS) == hip.DEEDS_ABI_SYMBOLS
    seen = set(hip.ABI_SYMBOLS)
    for header, words, version_symbol, version, sigs in EVERY_SIDE_ABI:
        path = os.path.join(ROOT, "include", header)
        macro = re.search(r"#define %s (\d+)" % version_symbol.upper(), open(path).read())
        assert macro is not None and int(macro.group(1)) == version, (header, version_symbol)
        assert words and version_symbol in sigs and set(sigs) == _symbols(path), header
        assert not (set(sigs) & seen), (header, sorted(set(sigs) & seen))
        seen |= set(sigs)
    lib = hip.load()
    for name, (res, args) in hip._DEEDS_SIGS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def workspace_formula(S, G, D, general):
    """the header's: general ? min(S, max(1, min(32768, 2^28 / (G*G*D*D*4)))) * G*G*D*D*4 : 0"""
    per = G * G * D * D * 4
    return min(S, max(1, min(32768, 2 ** 28 // per))) * per if general else 0


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(hip.lib_path())
    for name in _symbols(HEADER):
        assert hasattr(lib, name), f"{name} declared in rpnet_deeds_abi.h but not exported"
    hdr = open(HEADER).read()
    lib.rpnet_deeds_abi_version.restype = ctypes.c_int
    assert lib.rpnet_deeds_abi_version() == hip.DEEDS_ABI_VERSION == int(re.search(r"#define RPNET_DEEDS_ABI_VERSION (\d+)", hdr).group(1))
    macro = lambda n: int(re.search(r"#define RPNET_DEEDS_%s (\d+)" % n, hdr).group(1))  # noqa: E731
    assert (macro("MAX_GRID"), macro("MAX_WIDTH")) == (512, 31)
    assert R.DEEDS_MODES == {"nearest": macro("NEAREST"), "bilinear": macro("BILINEAR")}
    loaded = hip.load()
    assert loaded.rpnet_version() == hip.ABI_VERSION and loaded.rpnet_deeds_abi_version() == hip.DEEDS_ABI_VERSION
    # the size query needs no GPU, and its formula is the header's
    assert "rpnet_deeds_workspace_bytes = general ? min(S, max(1, min(32768, 2^28 / (G*G*D*D*4)))) * G*G*D*D*4 : 0" in hdr
    for S, G, D in ((1, 1, 1), (3, 18, 7), (64, 128, 15), (5, 128, 15), (18, 128, 15), (19, 128, 15), (2, 512, 31), (70000, 1, 1), (0, 8, 5)):
        for general in (0, 1):
            assert loaded.rpnet_deeds_workspace_bytes(S, G, D, general) == workspace_formula(S, G, D, general), (S, G, D, general)
    assert workspace_formula(64, 128, 15, 1) == 18 * 128 * 128 * 225 * 4 and workspace_formula(2, 512, 31, 1) == 512 * 512 * 961 * 4
    for bad in ((-1, 8, 5), (1, 0, 5), (1, 513, 5), (1, 8, 0), (1, 8, 4), (1, 8, 33)):
        assert loaded.rpnet_deeds_workspace_bytes(*bad, 1) == 0
        assert loaded.rpnet_last_error_string().decode() == "deeds_workspace_bytes: S=%d G=%d D=%d (S >= 0, G 1..512, D odd 1..31)" % bad


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
    assert reaches(defs, "deeds_register", "rpnet_deeds_register") and reaches(defs, "deeds_register", "rpnet_deeds_workspace_bytes")
    assert reaches(defs, "deeds_warp", "rpnet_deeds_warp") and not reaches(defs, "deeds_warp", "rpnet_deeds_register")
    assert not reaches(defs, "deeds_register", "rpnet_deeds_warp")
    assert not reaches(defs, "demons_register", "rpnet_deeds_register") and not reaches(defs, "affine_warp", "rpnet_deeds_warp")
    for sym in hip.DEEDS_ABI_SYMBOLS[1:]:
        assert reaches(defs, "register_slices", sym) and reaches(defs, "get_registration_field", sym), sym
        assert reaches(defs, "DeviceEvalSource", sym) and reaches(defs, "DeviceEpisodeSource", sym), sym
        assert not reaches(defs, "smooth_image", sym) and not reaches(defs, "DeviceVolumeLoader", sym), sym
    assert not reaches(defs, "deeds_register", "rpnet_demons_register")
    # every new top-level name of the package is new to it: package_defs is keyed by the bare name
    names = [n.name for path in glob.glob(os.path.join(ROOT, "rpnet_amd", "**", "*.py"), recursive=True)
             for n in ast.parse(open(path).read()).body if isinstance(n, (ast.FunctionDef, ast.ClassDef))]
    for name in ("deeds_register", "deeds_warp"):
        assert names.count(name) == 1, name
