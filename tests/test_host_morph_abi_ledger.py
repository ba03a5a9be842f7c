"""No untested morphology entry point: tests/morph_abi_ledger.py names, for every symbol of include/rpnet_morph_abi.h, the GPU test(s)
that exercise it.  The rules and the machinery are those of tests/test_host_abi_ledger.py and its followers (whose headers this
addition leaves as they were); runs without a GPU."""
import ctypes
import os
import re

from rpnet_amd import hip
from tests import morph_abi_ledger as L
from tests.test_host_abi_ledger import ROOT, gpu_tests, header_symbols, package_defs, reaches
from tests.test_host_guard_abi_ledger import _symbols

HEADER = os.path.join(ROOT, "include", "rpnet_morph_abi.h")
EARLIER = (("rpnet_eval_abi.h", hip.EVAL_ABI_SYMBOLS), ("rpnet_optim_abi.h", hip.OPTIM_ABI_SYMBOLS), ("rpnet_guard_abi.h", hip.GUARD_ABI_SYMBOLS),
           ("rpnet_surface_abi.h", hip.SURFACE_ABI_SYMBOLS), ("rpnet_cc_abi.h", hip.CC_ABI_SYMBOLS),
           ("rpnet_surface_spacing_abi.h", hip.SURFACE_SPACING_ABI_SYMBOLS), ("rpnet_ccpost_abi.h", hip.CCPOST_ABI_SYMBOLS))


def test_ledger_keys_are_the_header_symbols_and_the_binding_knows_them():
    syms = _symbols(HEADER)
    assert syms == {"rpnet_morph_abi_version", "rpnet_morph_workspace_bytes", "rpnet_morph_apply", "rpnet_morph_apply_spacing"}
    covered, exempt = set(L.COVERED_BY), set(L.EXEMPT)
    assert not (covered & exempt)
    assert covered | exempt == syms, (sorted(syms - covered - exempt), sorted((covered | exempt) - syms))
    assert set(L.VIA) <= covered
    assert all(isinstance(r, str) and len(r) > 20 for r in L.EXEMPT.values())
    assert set(hip.MORPH_ABI_SYMBOLS) == syms
    # one name, one header: nothing here is also declared in one of the earlier headers, and those still declare what they did
    assert not (syms & header_symbols()) and not (syms & set(hip.ABI_SYMBOLS))
    for other, known in EARLIER:
        theirs = _symbols(os.path.join(ROOT, "include", other))
        assert not (syms & theirs) and theirs == set(known), other
    # the eighth family, bound through one more row of the table
    assert len(hip.SIDE_ABIS) == 8 and hip.SIDE_ABIS[-1][0] == "rpnet_morph_abi.h" and hip.SIDE_ABIS[-1][4] is hip._MORPH_SIGS


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(hip.lib_path())
    for name in _symbols(HEADER):
        assert hasattr(lib, name), f"{name} declared in rpnet_morph_abi.h but not exported"
    hdr = open(HEADER).read()
    lib.rpnet_morph_abi_version.restype = ctypes.c_int
    assert lib.rpnet_morph_abi_version() == hip.MORPH_ABI_VERSION == int(re.search(r"#define RPNET_MORPH_ABI_VERSION (\d+)", hdr).group(1))
    from rpnet_amd import morphology as MO
    macro = lambda n: int(re.search(r"#define RPNET_MORPH_%s (\d+)" % n, hdr).group(1))  # noqa: E731
    assert (MO.STATS_ROW, MO.COUNTS_ROW, MO.MAX_RHO) == (macro("STATS_ROW"), macro("COUNTS_ROW"), macro("MAX_RHO")) == (4, 3, 3 * 1024 * 1024)
    assert (MO.ERODE, MO.DILATE, MO.OPEN, MO.CLOSE) == (macro("ERODE"), macro("DILATE"), macro("OPEN"), macro("CLOSE"))
    cc = open(os.path.join(ROOT, "include", "rpnet_cc_abi.h")).read()
    assert int(re.search(r"#define RPNET_CC_MAX_DIM (\d+)", cc).group(1)) == 1024
    loaded = hip.load()
    assert loaded.rpnet_version() == hip.ABI_VERSION and loaded.rpnet_morph_abi_version() == hip.MORPH_ABI_VERSION
    # the size query needs no GPU: a 64-byte head, 8 bytes and twice 1 byte per voxel, each volume rounded up to 16 bytes
    assert loaded.rpnet_morph_workspace_bytes(2, 3, 5) == 64 + 240 + 2 * 32 and loaded.rpnet_morph_workspace_bytes(1, 1, 1) == 64 + 16 + 32
    assert loaded.rpnet_morph_workspace_bytes(0, 3, 5) == 0 and loaded.rpnet_last_error_string().decode().startswith("morph: D=0")
    assert loaded.rpnet_morph_workspace_bytes(2, 1025, 5) == 0


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
    for fn in ("erode", "dilate", "opening", "closing"):
        assert all(reaches(defs, fn, s) for s in ("rpnet_morph_apply", "rpnet_morph_apply_spacing", "rpnet_morph_workspace_bytes")), fn
    assert reaches(defs, "VolumeSegmenter", "rpnet_morph_apply") and reaches(defs, "VolumeSegmenter", "rpnet_morph_apply_spacing")
    assert not reaches(defs, "morph_figures", "rpnet_morph_apply") and not reaches(defs, "check_radius", "rpnet_morph_apply")
    assert not reaches(defs, "resolve_radius", "rpnet_morph_apply_spacing") and not reaches(defs, "surface_tally", "rpnet_morph_apply")
