"""The numpy restatement of rpnet_amd.surface_spacing, the spacing of an NRRD header and the ledger of include/rpnet_surface_spacing_abi.h,
without a GPU.

The restatement is what tests/test_gpu_surface_spacing.py compares the kernels with, so it is pinned here three ways: to
scipy.ndimage.distance_transform_edt(sampling=) within 16 ulps of sqrt(d2) (either side makes at most about six roundings, in different
orders; measured on these inputs: below 1 ulp, profiles/surface_spacing.txt), to the integer restatement of rpnet_amd.surface at spacing
(1, 1, 1) exactly, and to an all-pairs computation.  A line-by-line copy of it with the kernel's outward scan then takes seeded
defects, each of which must fail one of those comparisons."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
from scipy import ndimage

from rpnet_amd import hip
from rpnet_amd import surface as SF
from rpnet_amd import surface_spacing as SS
from rpnet_amd.utils import nrrd
from rpnet_amd.utils import volume_reader as VR
from tests import surface_spacing_abi_ledger as L
from tests import surface_spacing_cases as SC
from tests.test_host_abi_ledger import ROOT, gpu_tests, header_symbols, package_defs, reaches
from tests.test_host_guard_abi_ledger import _symbols

HEADER = os.path.join(ROOT, "include", "rpnet_surface_spacing_abi.h")
ULPS = 16
SEEDED = [(5, 7, 9), (9, 33, 20), (17, 40, 36)]


@pytest.mark.parametrize("spacing", SC.SPACINGS)
def test_restatement_against_scipy(spacing):
    worst = 0.0
    for shape in SEEDED:
        for density in (0.02, 0.3):
            border = SF.border_reference(SC.noise(shape, density=density)[0] == 1)
            d2 = SS.transform_reference_spacing(border, SS.spacing_weights(spacing))
            want = ndimage.distance_transform_edt(~border, sampling=spacing)
            worst = max(worst, SC.ulps(np.sqrt(d2), want))
    print(spacing, "largest difference in ulps", worst)
    assert worst <= ULPS


def test_unit_spacing_is_the_integer_restatement():
    for shape in SEEDED + [(1, 16, 16)]:
        for a, b in (SC.noise(shape), SC.boxes(shape), SC.noise(shape, density=0.02)):
            irow, frow = SS.rows_reference_spacing(a, b, (1.0, 1.0, 1.0))
            want_i, want_f = SF.rows_reference(a, b)
            n_a, n_b, d2_k, d2_k1, d2_max, k = want_i.tolist()
            assert irow[:3].tolist() == [n_a, n_b, k] and frow[:3].tolist() == [float(d2_k), float(d2_k1), float(d2_max)]
            # the sums: math.fsum of the roots here, of count * sqrt(bin) there: one rounded product per bin, at most nbins of them
            tol = (sum((s - 1) ** 2 for s in shape) + 1) * 2.0 ** -53
            assert all(abs(g - w_) <= tol * w_ for g, w_ in zip(frow[3:], want_f))
            fig, want = SS.figures_from_rows(irow, frow), SF.surface_from_rows(want_i, want_f)
            assert fig["hd95"] == want["hd95"] and fig["hd"] == want["hd"] and fig["nsd"] is None
            assert abs(fig["assd"] - want["assd"]) <= tol * want["assd"]
    empty = SS.rows_reference_spacing(np.zeros((3, 4, 5)), np.ones((3, 4, 5)), (1, 2, 3))
    assert empty[0].tolist() == [0, 0, -1, 0, 0] and empty[1].tolist() == [0.0] * 5
    assert SS.figures_from_rows(*empty, tau=1.0) == {"hd95": None, "hd": None, "assd": None, "nsd": None}


def anisotropic_case():
    """one prediction voxel; truth voxels one slice away along z and three pixels away along x.  In voxels the z neighbour is nearest
    (1 < 3); at spacing (5, 1, 1) the x neighbour is (3 mm < 5 mm): the millimetre figure is no multiple of the voxel figure"""
    a, b = np.zeros((4, 5, 9), np.uint8), np.zeros((4, 5, 9), np.uint8)
    a[1, 2, 2] = 1
    b[2, 2, 2] = 1
    b[1, 2, 5] = 1
    return a, b


def test_anisotropy_is_not_a_rescaling():
    a, b = anisotropic_case()
    spacing = (5.0, 1.0, 1.0)
    voxels = SS.surface_reference_spacing(a, b, (1.0, 1.0, 1.0))[2]
    mm = SS.surface_reference_spacing(a, b, spacing)[2]
    pooled = SC.brute_force(a, b, spacing)
    assert pooled.tolist() == [3.0, 3.0, 5.0]          # prediction -> x neighbour, x neighbour -> prediction, z neighbour -> prediction
    assert mm["hd95"] == SC.percentile95(pooled) and mm["hd"] == pooled[-1]
    assert abs(mm["assd"] - (pooled[0] + (pooled[1] + pooled[2]) / 2) / 2) <= 4 * 2.0 ** -52 * mm["assd"]
    for factor in spacing:
        assert mm["hd95"] != factor * voxels["hd95"], factor
    assert not any(abs(mm["hd95"] / voxels["hd95"] - f) < 1e-9 for f in spacing)
    # and on seeded volumes the restatement is the all-pairs computation
    for shape in SEEDED[:2]:
        for sp in SC.SPACINGS:
            x, y = SC.noise(shape, density=0.05)
            irow, frow = SS.rows_reference_spacing(x, y, sp)
            pooled = SC.brute_force(x, y, sp)
            k = int(irow[2])
            assert SC.ulps(np.sqrt(frow[:3]), [pooled[k], pooled[min(k + 1, pooled.size - 1)], pooled[-1]]) <= ULPS
            assert abs(SS.figures_from_rows(irow, frow)["hd95"] - SC.percentile95(pooled)) <= ULPS * 2.0 ** -52 * pooled[-1]


# ------------------------------------------------------------------------------------------------- seeded defects
def scan_restatement(pred, truth, spacing, tau=None, defect=None):
    """rows_reference_spacing once more, voxel by voxel with the kernel's outward scan and early exit, with one defect switched on"""
    w = SS.spacing_weights(spacing)
    if defect == "axes":
        w = (w[2], w[1], w[0])

    def combine(a, prod):
        if defect == "fma":                                      # one rounding of the exact a + w * o^2, as a contraction would give
            return float(np.float64(np.longdouble(a) + np.longdouble(prod[0]) * np.longdouble(prod[1])))
        return a + prod[0] * prod[1]

    def transform(border):
        D, H, W = border.shape
        g = np.full(border.shape, SS.NO_SEED)
        for z in range(D):
            for y in range(H):
                for x in range(W):
                    hits = [abs(x - j) for j in range(W) if border[z, y, j]]
                    if hits:
                        g[z, y, x] = w[2] * float(min(hits) ** 2)
        for axis in (1, 0):
            g = np.moveaxis(g, axis, -1)
            out = g.copy()
            L_ = g.shape[-1]
            for idx in np.ndindex(*g.shape[:-1]):
                line = g[idx]
                for i in range(L_):
                    best = line[i]
                    for o in range(1, L_):
                        if (float(o * o) if defect == "exit" else w[axis] * float(o * o)) >= best:
                            break
                        for j in (i - o, i + o):
                            if 0 <= j < L_:
                                best = min(best, combine(line[j], (w[axis], float(o * o))))
                    out[idx + (i,)] = min(best, SS.NO_SEED)
            g = np.moveaxis(out, -1, axis)
        return g

    a, b = SF.border_reference(np.asarray(pred) == 1), SF.border_reference(np.asarray(truth) == 1)
    n_a, n_b = int(a.sum()), int(b.sum())
    d_ab, d_ba = transform(b)[a], transform(a)[b]
    pooled = np.sort(np.concatenate([d_ab, d_ba]))
    n = n_a + n_b
    k = int(math.floor((n - 1) * 0.95))
    k1 = min(k + 1, n - 2) if defect == "clamp" else min(k + 1, n - 1)
    tau2 = SS.tolerance_squared(tau)
    within = (lambda d: int((d < tau2).sum())) if defect == "tau" else (lambda d: int((d <= tau2).sum()))
    irow = np.array([n_a, n_b, k, within(d_ab), within(d_ba)], dtype=np.int64)
    frow = np.array([pooled[k], pooled[k1], pooled[-1], math.fsum(np.sqrt(d_ab).tolist()), math.fsum(np.sqrt(d_ba).tolist())])
    return irow, frow


def defect_cases():
    """(prediction, truth, spacing, tau) on which the comparisons below run: noise under two anisotropic spacings, the pooled count of
    3, far-apart voxels, and a tolerance that coincides with a distance"""
    a, b = SC.noise((4, 9, 10), density=0.08)
    yield a, b, SC.SPACINGS[3], 1.0
    yield a, b, SC.SPACINGS[1], None
    yield (*SC.scattered(1, 2, shape=(3, 6, 7)), SC.SPACINGS[1], None)           # n = 3: k + 1 = n - 1
    yield (*SC.scattered(2, 3, shape=(3, 12, 13)), SC.SPACINGS[3], None)         # offsets of 3 and more: w * o^2 is no longer exact
    yield (*SC.boxes((4, 7, 8)), (2.5, 0.5, 0.5), 2.5)
    corner = np.zeros((4, 9, 10), np.uint8)
    corner[0, 0, 0] = 1
    yield np.ones((4, 9, 10), np.uint8), corner, SC.SPACINGS[3], None           # every offset of the shell to one voxel: many sums
    # two voxels at the first offset (oy, ox) whose wx * ox^2 + wy * oy^2 rounds differently in one rounding than in two (the sums of
    # the cases above absorb such a last-bit difference; a rank that IS such a value cannot)
    w = SS.spacing_weights(SC.SPACINGS[3])
    oy, ox = next((oy, ox) for oy in range(1, 12) for ox in range(1, 12)
                  if w[2] * float(ox * ox) + w[1] * float(oy * oy)
                  != float(np.float64(np.longdouble(w[2] * float(ox * ox)) + np.longdouble(w[1]) * np.longdouble(float(oy * oy)))))
    a, b = np.zeros((1, 12, 12), np.uint8), np.zeros((1, 12, 12), np.uint8)
    a[0, 0, 0] = b[0, oy, ox] = 1
    yield a, b, SC.SPACINGS[3], None


def same_rows(x, y):
    return x[0].tolist() == y[0].tolist() and x[1].tobytes() == y[1].tobytes()


def test_the_scan_copy_is_the_restatement():
    for a, b, spacing, tau in defect_cases():
        assert same_rows(scan_restatement(a, b, spacing, tau), SS.rows_reference_spacing(a, b, spacing, tau=tau)), spacing


@pytest.mark.parametrize("defect", ["axes", "fma", "exit", "clamp", "tau"])
def test_seeded_defects_fail(defect):
    """spacing axes swapped; an FMA-like single rounding; the early exit on o^2 instead of w * o^2; k + 1 clamped to n - 2; tau compared
    with `<`: each changes a row on at least one case, so the bit-for-bit comparison of the GPU tests would catch it"""
    failed = [not same_rows(scan_restatement(a, b, spacing, tau, defect), SS.rows_reference_spacing(a, b, spacing, tau=tau))
              for a, b, spacing, tau in defect_cases()]
    print(defect, failed)
    assert any(failed)


# ------------------------------------------------------------------------------------------------- headers
def test_spacing_from_header():
    f = SS.spacing_from_header
    assert f({"space directions": "(2.5,0,0) (0,0.8,0) (0,0,0.8)"}) == (2.5, 0.8, 0.8)
    assert f({"space directions": "(0.6,0.8,0) (-0.8,0.6,0) (0,0,3)"}) == (1.0, 1.0, 3.0)          # oblique: the norms of the vectors
    assert f({"space directions": "none (1,0,0) (0,2,0) (0,0,3)", "spacings": "nan 9 9 9"}) == (1.0, 2.0, 3.0)
    assert f({"spacings": "0.7 0.7 2.5"}) == (0.7, 0.7, 2.5) and f({"spacings": "nan 1 2 3"}) == (1.0, 2.0, 3.0)
    assert f({"space directions": "(1,0,0) (0,1,0)", "spacings": "1 2 3"}) == (1.0, 2.0, 3.0)       # the first field that gives three
    for header, names in (({}, "neither field is present"), ({"spacings": "1 2"}, "`spacings` gives"),
                          ({"space directions": "(1,0,0) (0,0,0) (0,0,1)"}, "`space directions` gives"), ({"spacings": "1 -2 3"}, "`spacings` gives"),
                          ({"spacings": "1 inf 3"}, "`spacings` gives")):
        with pytest.raises(ValueError, match="three positive spacings in `space directions` .* or in `spacings`.*" + names):
            f(header)


def test_read_header_and_volume_spacing(tmp_path):
    data = np.arange(24, dtype=np.int16).reshape(2, 3, 4)
    path = str(tmp_path / "v.nrrd")
    nrrd.write(path, data, header={"space directions": "(1,0,0) (0,2,0) (0,0,3)", "note": "x"})
    header = nrrd.read_header(path)
    got, want = nrrd.read(path)
    assert np.array_equal(got, data) and sorted(header) == sorted(want)
    assert all(np.array_equal(header[k], want[k]) for k in want)
    with open(path, "r+b") as f:                                   # the payload is not touched: cut it off
        f.truncate(os.path.getsize(path) - 8)
    assert nrrd.read_header(path)["space directions"] == "(1,0,0) (0,2,0) (0,0,3)"
    with pytest.raises(Exception):
        nrrd.read(path)
    # a synthetic data set with and without a spacing
    from tests.reader_cases import config_for
    case = {"data": dict(n_volumes=2, classes=("Liver",), shape=(22, 44, 40), seed=3), "cfg": dict(num_slice=20, num_x=44, num_y=40, crop_size=[32, 32], k=4)}
    for spacing in ((2.5, 0.8, 0.8), None):
        data_dir, set_name, csv_dir = VR.write_synthetic_dataset(str(tmp_path / str(spacing)), spacing=spacing, **case["data"])
        reader = VR.FewshotVolumeReader(data_dir, set_name, config_for(case, csv_dir), mode="eval")
        pid = reader.data_info[0][0]["pid"]
        if spacing:
            assert reader.volume_spacing(pid) == spacing
            assert SS.spacing_from_header(nrrd.read_header(os.path.join(data_dir, f"{pid}_Liver.nrrd"))) == spacing
        else:
            assert "space directions" not in nrrd.read_header(os.path.join(data_dir, f"{pid}_clean.nrrd"))
            with pytest.raises(ValueError, match=f"{pid}_clean.nrrd: spacing_from_header"):
                reader.volume_spacing(pid)


def test_python_checks_without_a_gpu():
    for bad in ((1, 1), (1, 0, 1), (1, float("nan"), 1), "abc", None):
        with pytest.raises(ValueError, match="three finite positive numbers"):
            SS.check_spacing(bad)
    assert SS.spacing_weights((0.5, 2, 3)) == (0.25, 4.0, 9.0) and SS.tolerance_squared(None) == SS.tolerance_squared(-1) == -1.0
    assert SS.tolerance_squared(1.5) == 2.25 and SS.NO_SEED == np.finfo(np.float64).max
    with pytest.raises(ValueError, match="isotropic factor"):      # the integer path still refuses a per-axis spacing, in its own words
        SF.surface_from_rows(np.zeros(6, np.int64), np.zeros(2), spacing=(1, 2, 3))
    assert "surface_spacing" in SF.__doc__


# ------------------------------------------------------------------------------------------------- the ledger
def test_ledger_keys_are_the_header_symbols_and_the_binding_knows_them():
    syms = _symbols(HEADER)
    assert syms == {"rpnet_surface_spacing_abi_version", "rpnet_surface_spacing_workspace_bytes", "rpnet_surface_spacing_tally"}
    covered, exempt = set(L.COVERED_BY), set(L.EXEMPT)
    assert not (covered & exempt)
    assert covered | exempt == syms, (sorted(syms - covered - exempt), sorted((covered | exempt) - syms))
    assert set(L.VIA) <= covered
    assert all(isinstance(r, str) and len(r) > 20 for r in L.EXEMPT.values())
    assert set(hip.SURFACE_SPACING_ABI_SYMBOLS) == syms
    # one name, one header: nothing here is also declared in one of the six earlier headers
    assert not (syms & header_symbols()) and not (syms & set(hip.ABI_SYMBOLS))
    for other, known in (("rpnet_eval_abi.h", hip.EVAL_ABI_SYMBOLS), ("rpnet_optim_abi.h", hip.OPTIM_ABI_SYMBOLS),
                         ("rpnet_guard_abi.h", hip.GUARD_ABI_SYMBOLS), ("rpnet_surface_abi.h", hip.SURFACE_ABI_SYMBOLS),
                         ("rpnet_cc_abi.h", hip.CC_ABI_SYMBOLS)):
        assert not (syms & _symbols(os.path.join(ROOT, "include", other))) and not (syms & set(known)), other


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(hip.lib_path())
    for name in _symbols(HEADER):
        assert hasattr(lib, name), f"{name} declared in rpnet_surface_spacing_abi.h but not exported"
    hdr = open(HEADER).read()
    lib.rpnet_surface_spacing_abi_version.restype = ctypes.c_int
    assert (lib.rpnet_surface_spacing_abi_version() == hip.SURFACE_SPACING_ABI_VERSION
            == int(re.search(r"#define RPNET_SURFACE_SPACING_ABI_VERSION (\d+)", hdr).group(1)))
    surface = open(os.path.join(ROOT, "include", "rpnet_surface_abi.h")).read()
    assert re.search(r"#define RPNET_SURFACE_SPACING_MAX_DIM (\d+)", hdr).group(1) == re.search(r"#define RPNET_SURFACE_MAX_DIM (\d+)", surface).group(1)
    assert int(re.search(r"#define RPNET_SURFACE_SPACING_IROW (\d+)", hdr).group(1)) == SS.IROW
    assert int(re.search(r"#define RPNET_SURFACE_SPACING_FROW (\d+)", hdr).group(1)) == SS.FROW
    loaded = hip.load()
    assert loaded.rpnet_version() == hip.ABI_VERSION and loaded.rpnet_surface_abi_version() == hip.SURFACE_ABI_VERSION
    # the size query and the refusals that come before any launch need no GPU
    assert loaded.rpnet_surface_spacing_workspace_bytes(2, 3, 5) == 66048 + 16 * 30 and loaded.rpnet_surface_spacing_workspace_bytes(0, 3, 5) == 0
    assert loaded.rpnet_last_error_string().decode().startswith("surface_spacing: D=0")
    w = (ctypes.c_double * 3)(1.0, 0.0, 1.0)
    rc = loaded.rpnet_surface_spacing_tally(8, 0, 8, 0, 1, 2, 3, 5, w, -1.0, 8, 0, 8, 0, 1, 16, 1 << 20, None)
    assert rc != 0 and "weight 1 is 0" in loaded.rpnet_last_error_string().decode()


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
    assert reaches(defs, "surface_tally_spacing", "rpnet_surface_spacing_tally")
    assert reaches(defs, "surface_tally_spacing", "rpnet_surface_spacing_workspace_bytes")
    assert reaches(defs, "VolumeSegmenter", "rpnet_surface_spacing_tally") and reaches(defs, "evaluate_dataset", "rpnet_surface_spacing_tally")
    assert not reaches(defs, "surface_tally", "rpnet_surface_spacing_tally") and not reaches(defs, "figures_from_rows", "rpnet_surface_spacing_tally")
    assert not reaches(defs, "transform_reference_spacing", "rpnet_surface_spacing_tally")
