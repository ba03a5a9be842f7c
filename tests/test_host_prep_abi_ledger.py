"""No untested preprocessing entry point: tests/prep_abi_ledger.py names, for every symbol of include/rpnet_prep_abi.h, the GPU test(s)
that exercise it.  The rules and the machinery are those of tests/test_host_abi_ledger.py and its followers (whose headers this
addition leaves as they were); runs without a GPU."""
import ctypes
import os
import re

from rpnet_amd import hip
from tests import prep_abi_ledger as L
from tests.test_host_abi_ledger import ROOT, gpu_tests, header_symbols, package_defs, reaches
from tests.test_host_guard_abi_ledger import _symbols

HEADER = os.path.join(ROOT, "include", "rpnet_prep_abi.h")
EARLIER = (("rpnet_eval_abi.h", hip.EVAL_ABI_SYMBOLS), ("rpnet_optim_abi.h", hip.OPTIM_ABI_SYMBOLS), ("rpnet_guard_abi.h", hip.GUARD_ABI_SYMBOLS),
           ("rpnet_surface_abi.h", hip.SURFACE_ABI_SYMBOLS), ("rpnet_cc_abi.h", hip.CC_ABI_SYMBOLS),
           ("rpnet_surface_spacing_abi.h", hip.SURFACE_SPACING_ABI_SYMBOLS), ("rpnet_ccpost_abi.h", hip.CCPOST_ABI_SYMBOLS),
           ("rpnet_morph_abi.h", hip.MORPH_ABI_SYMBOLS))
ENTRY = ("rpnet_prep_threshold", "rpnet_prep_seeded_component", "rpnet_prep_mask_bbox")


def test_ledger_keys_are_the_header_symbols_and_the_binding_knows_them():
    syms = _symbols(HEADER)
    assert syms == {"rpnet_prep_abi_version"} | set(ENTRY) | {e + "_workspace_bytes" for e in ENTRY}
    covered, exempt = set(L.COVERED_BY), set(L.EXEMPT)
    assert not (covered & exempt)
    assert covered | exempt == syms, (sorted(syms - covered - exempt), sorted((covered | exempt) - syms))
    assert set(L.VIA) <= covered
    assert all(isinstance(r, str) and len(r) > 20 for r in L.EXEMPT.values())
    assert set(hip.PREP_ABI_SYMBOLS) == syms
    # one name, one header: nothing here is also declared in one of the earlier headers, and those still declare what they did
    assert not (syms & header_symbols()) and not (syms & set(hip.ABI_SYMBOLS))
    for other, known in EARLIER:
        theirs = _symbols(os.path.join(ROOT, "include", other))
        assert not (syms & theirs) and theirs == set(known), other


def test_the_ninth_family_is_bound_and_checked_like_the_table():
    """the ninth family stands behind the eight rows of SIDE_ABIS, in a table of the same form that load() binds with them; what
    tests/test_host_side_abi_table.py asserts over SIDE_ABIS holds over all nine"""
    assert hip.ALL_SIDE_ABIS == hip.SIDE_ABIS + hip.LATER_SIDE_ABIS and len(hip.ALL_SIDE_ABIS) == 9
    assert hip.ALL_SIDE_ABIS[-1][0] == "rpnet_prep_abi.h" and hip.ALL_SIDE_ABIS[-1][4] is hip._PREP_SIGS
    assert hip.ALL_SIDE_ABIS[-1][3] == hip.PREP_ABI_VERSION and tuple(hip._PREP_SIGS) == hip.PREP_ABI_SYMBOLS
    seen = set(hip.ABI_SYMBOLS)
    for header, words, version_symbol, version, sigs in hip.ALL_SIDE_ABIS:
        path = os.path.join(ROOT, "include", header)
        macro = re.search(r"#define %s (\d+)" % version_symbol.upper(), open(path).read())
        assert macro is not None and int(macro.group(1)) == version, (header, version_symbol)
        assert words and version_symbol in sigs and set(sigs) == _symbols(path), header
        assert not (set(sigs) & seen), (header, sorted(set(sigs) & seen))
        seen |= set(sigs)
    # load() went through all nine: every symbol of the family carries the signature of the binding
    lib = hip.load()
    for name, (res, args) in hip._PREP_SIGS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(hip.lib_path())
    for name in _symbols(HEADER):
        assert hasattr(lib, name), f"{name} declared in rpnet_prep_abi.h but not exported"
    hdr = open(HEADER).read()
    lib.rpnet_prep_abi_version.restype = ctypes.c_int
    assert lib.rpnet_prep_abi_version() == hip.PREP_ABI_VERSION == int(re.search(r"#define RPNET_PREP_ABI_VERSION (\d+)", hdr).group(1))
    from rpnet_amd import preprocess as PP
    macro = lambda n: int(re.search(r"#define RPNET_PREP_%s (\d+)" % n, hdr).group(1))  # noqa: E731
    assert (PP.THRESHOLD_ROW, PP.THRESHOLD_FROW, PP.SEED_ROW, PP.BBOX_ROW) == (macro("THRESHOLD_ROW"), macro("THRESHOLD_FROW"), macro("SEED_ROW"),
                                                                               macro("BBOX_ROW")) == (4, 3, 4, 8)
    assert (PP.FIXED, PP.OTSU, macro("OTSU_BINS")) == (macro("FIXED"), macro("OTSU"), 128)
    import torch
    assert (PP.IMAGE_KINDS[torch.float32], PP.IMAGE_KINDS[torch.int16]) == (macro("F32"), macro("I16"))
    cc = open(os.path.join(ROOT, "include", "rpnet_cc_abi.h")).read()
    assert int(re.search(r"#define RPNET_CC_MAX_DIM (\d+)", cc).group(1)) == 1024
    assert PP.OVERRUN_OFFSET == int(re.search(r"#define RPNET_CC_OVERRUN_OFFSET (\d+)", cc).group(1))
    loaded = hip.load()
    assert loaded.rpnet_version() == hip.ABI_VERSION and loaded.rpnet_prep_abi_version() == hip.PREP_ABI_VERSION
    # the size queries need no GPU: a 64-byte head; 136 uint32 per slice; two int32 volumes rounded up to 16 bytes and 16 bytes per slice
    assert loaded.rpnet_prep_threshold_workspace_bytes(2, 3, 5) == 64 + 2 * 136 * 4
    assert loaded.rpnet_prep_seeded_component_workspace_bytes(2, 3, 5) == 64 + 2 * 128 + 2 * 16
    assert loaded.rpnet_prep_mask_bbox_workspace_bytes(2, 3, 5) == 64
    for e in ENTRY:
        query = getattr(loaded, e + "_workspace_bytes")
        assert query(0, 3, 5) == 0 and loaded.rpnet_last_error_string().decode().startswith(e[6:] + ": D=0")
        assert query(2, 1025, 5) == 0 and query(2, 3, 1025) == 0


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
    assert reaches(defs, "threshold_mask", "rpnet_prep_threshold") and reaches(defs, "threshold_mask", "rpnet_prep_threshold_workspace_bytes")
    assert reaches(defs, "seeded_component", "rpnet_prep_seeded_component") and reaches(defs, "mask_bbox", "rpnet_prep_mask_bbox")
    for sym in ENTRY:
        assert reaches(defs, "clean_volume", sym) and reaches(defs, "clean_volume", sym + "_workspace_bytes"), sym
    assert reaches(defs, "body_mask", "rpnet_morph_apply") and reaches(defs, "body_mask", "rpnet_ccpost_fill_holes")
    assert not reaches(defs, "body_mask", "rpnet_prep_mask_bbox") and not reaches(defs, "threshold_mask", "rpnet_prep_seeded_component")
    assert not reaches(defs, "_check_mask", "rpnet_prep_mask_bbox") and not reaches(defs, "_check_image", "rpnet_prep_threshold")
