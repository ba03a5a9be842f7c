"""rpnet_amd.hip.SIDE_ABIS, the table load() binds the side families from, against the headers it names: asserted once over the whole
table, so that a family added later cannot skip what the per-family ledger tests assert one by one.  Runs without a GPU."""
import os
import re

from rpnet_amd import hip
from tests.test_host_abi_ledger import ROOT
from tests.test_host_guard_abi_ledger import _symbols


def test_every_family_of_the_table_matches_its_header():
    assert len(hip.SIDE_ABIS) >= 7
    seen = set(hip.ABI_SYMBOLS)
    for header, words, version_symbol, version, sigs in hip.SIDE_ABIS:
        path = os.path.join(ROOT, "include", header)
        assert os.path.isfile(path), header
        macro = re.search(r"#define %s (\d+)" % version_symbol.upper(), open(path).read())
        assert macro is not None and int(macro.group(1)) == version, (header, version_symbol)
        assert words and version_symbol in sigs, header
        assert set(sigs) == _symbols(path), (header, sorted(set(sigs) ^ _symbols(path)))
        assert not (set(sigs) & seen), (header, sorted(set(sigs) & seen))          # one name, one family
        seen |= set(sigs)
    # the module-level names the ledger tests read are the table's rows
    for name in ("EVAL", "OPTIM", "GUARD", "SURFACE", "CC", "SURFACE_SPACING", "CCPOST"):
        row = [f for f in hip.SIDE_ABIS if f[4] is getattr(hip, f"_{name}_SIGS")]
        assert len(row) == 1 and row[0][3] == getattr(hip, f"{name}_ABI_VERSION") and tuple(row[0][4]) == getattr(hip, f"{name}_ABI_SYMBOLS")
