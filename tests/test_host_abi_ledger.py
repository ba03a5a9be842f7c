"""No untested entry point: tests/abi_ledger.py names, for every symbol of include/rpnet_abi.h, the GPU test(s) that exercise it
(or why none should).  Runs without a GPU: it reads the header, the ledger and the test sources."""
import ast
import glob
import os
import re

from tests import abi_ledger as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rpnet_abi.h")).read(), flags=re.S)
    return set(re.findall(r"\b(rpnet_\w+)\s*\(", text))


def gpu_tests():
    """{"tests/file.py::test_name": source text} of every test that is marked gpu, by its module or by its own decorator; the
    text of a test includes the helper functions of its own module that it names (run_stp, _run, build, ...)"""
    out, all_tests = {}, set()
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_*.py"))):
        src = open(path).read()
        tree = ast.parse(src)
        helpers = {n.name: ast.get_source_segment(src, n) for n in tree.body
                   if isinstance(n, ast.FunctionDef) and not n.name.startswith("test_")}
        module_gpu = any(isinstance(n, ast.Assign) and any(getattr(t, "id", "") == "pytestmark" for t in n.targets)
                         and "gpu" in ast.get_source_segment(src, n.value) for n in tree.body)
        for n in tree.body:
            if isinstance(n, ast.FunctionDef) and n.name.startswith("test_"):
                tid = f"tests/{os.path.basename(path)}::{n.name}"
                all_tests.add(tid)
                decorated = any("mark.gpu" in ast.get_source_segment(src, d) for d in n.decorator_list)
                if module_gpu or decorated:
                    text = ast.get_source_segment(src, n)
                    out[tid] = text + "".join("\n" + h for name, h in helpers.items() if re.search(r"\b%s\b" % name, text))
    return out, all_tests


def package_defs():
    """{name: source} of the top-level functions and classes of rpnet_amd"""
    defs = {}
    for path in glob.glob(os.path.join(ROOT, "rpnet_amd", "**", "*.py"), recursive=True):
        src = open(path).read()
        for n in ast.parse(src).body:
            if isinstance(n, (ast.FunctionDef, ast.ClassDef)):
                defs[n.name] = ast.get_source_segment(src, n)
    return defs


def reaches(defs, start, symbol):
    """does the function / class `start` hold the call of `symbol`, itself or through the package functions it names"""
    seen, todo = set(), [start]
    while todo:
        name = todo.pop()
        if name in seen:
            continue
        seen.add(name)
        text = defs[name]
        if f'"{symbol}"' in text:
            return True
        todo += [d for d in defs if d not in seen and re.search(r"\b%s\b" % re.escape(d), text)]
    return False


def test_ledger_keys_are_the_header_symbols():
    syms = header_symbols()
    assert len(syms) >= 90
    covered, exempt = set(L.COVERED_BY), set(L.EXEMPT)
    assert not (covered & exempt), sorted(covered & exempt)
    assert covered | exempt == syms, (sorted(syms - covered - exempt), sorted((covered | exempt) - syms))
    assert set(L.VIA) <= covered
    assert all(isinstance(r, str) and len(r) > 20 for r in L.EXEMPT.values())
    # the binding knows the same symbols
    from rpnet_amd import hip
    assert set(hip.ABI_SYMBOLS) == syms


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
            # the name leads to the symbol inside the package: a function / class of that name, or one that holds the name
            # (a module switch such as _CONV1_RECOMP), reaches the call
            ok = any(reaches(defs, d, sym) for v in via for d in defs
                     if d == v or (v not in defs and re.search(r"\b%s\b" % re.escape(v), defs[d])))
            if not ok:
                problems.append(f"{sym}: nothing in rpnet_amd leads from {via} to the symbol")
    assert not problems, "\n".join(problems)


def test_the_check_would_notice():
    defs = package_defs()
    assert reaches(defs, "MaskedPool", "rpnet_masked_pool_fwd") and not reaches(defs, "MaskedPool", "rpnet_seg_tally")
    gpu, every = gpu_tests()
    assert "tests/test_host_abi_ledger.py::test_the_check_would_notice" in every
    assert "tests/test_host_abi_ledger.py::test_the_check_would_notice" not in gpu
