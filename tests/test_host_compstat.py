"""The numpy restatement of the per-component statistics (tests/compstat_cases.py) pinned to scipy.ndimage and to direct computations,
the host functions of rpnet_amd/component_stats.py on its tables, and six seeded defects shown to fail the same checks.  Runs on the
CPU."""
import math

import numpy as np
import pytest
from scipy import ndimage

from rpnet_amd import component_stats as CS
from tests import compstat_cases as CC

SHAPES = [(3, 9, 13), (2, 33, 65), (5, 40, 70), (1, 70, 130)]       # every one but the first holds more than one chunk
DENSITIES = (0.1, 0.31, 0.6)


def structure(connectivity):
    return ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3)


def cases():
    for shape in SHAPES:
        for density in DENSITIES:
            for connectivity in (6, 26):
                yield shape, density, connectivity


def check_numbering(defect=None):
    """the renumbering gives scipy.ndimage.label's own ids, not merely an equivalent labelling"""
    for shape, density, connectivity in cases():
        mask = CC.noise_mask(shape, density, seed=sum(shape) + connectivity)
        want, n = ndimage.label(mask, structure=structure(connectivity))
        dense, C, invalid = CC.rank_restate(CC.sparse_labels(mask, connectivity), defect=defect)
        assert C == n and invalid == 0
        assert np.array_equal(dense, want), (shape, density, connectivity)


def check_table(defect=None, q=4, max_components=None):
    """sum, find_objects and center_of_mass agree with the rows, the moments with a direct computation, the quantised sums with exact
    Python integers, the overlap with a direct count, n_beyond with the voxels of the ids beyond the table"""
    for shape, density, connectivity in list(cases())[::3]:
        mask = CC.noise_mask(shape, density, seed=sum(shape) + connectivity)
        lab, n = ndimage.label(mask, structure=structure(connectivity))
        rng = np.random.RandomState(n)
        image = (np.round(rng.standard_normal(shape) * 64.0) / 32.0 + rng.randint(0, 2, shape) * 2.0 ** -(q + 1)).astype(np.float32)   # ties in plenty
        image.ravel()[::97] = np.nan
        big = rng.choice(np.flatnonzero(mask), 5, replace=False)
        image.ravel()[big] = 2.0 ** 20                       # k = 2^(20 + q): k * k needs its hi word
        other = rng.randint(0, 3, shape).astype(np.uint8)
        M = max_components or n + 3
        dense, C, _ = CC.rank_restate(CC.sparse_labels(mask, connectivity))
        rows, beyond, bad = CC.table_restate(dense, C, image, q, other, 1, M, defect=defect)
        assert bad == 0 and beyond == int((lab > M).sum())
        index = np.arange(1, min(n, M) + 1)
        assert np.array_equal(rows[:len(index), 0], ndimage.sum(np.ones(shape), lab, index).astype(np.int64))
        assert (rows[len(index):] == CC.empty_row(shape)).all()
        for k, box in zip(index, ndimage.find_objects(lab)):
            assert tuple(rows[k - 1, 1:4]) == tuple(s.start for s in box) and tuple(rows[k - 1, 4:7]) == tuple(s.stop - 1 for s in box)
        com = np.array(ndimage.center_of_mass(np.ones(shape), lab, index)).reshape(-1, 3)
        assert np.allclose(rows[:len(index), 7:10] / rows[:len(index), :1], com, rtol=1e-12, atol=1e-12)
        for k in sorted(set(index[:: max(1, len(index) // 40)].tolist()) | (set(lab.ravel()[big].tolist()) & set(index.tolist()))):
            z, y, x = (c.astype(np.int64) for c in np.nonzero(lab == k))
            r = rows[k - 1]
            assert list(r[10:16]) == [(z * z).sum(), (y * y).sum(), (x * x).sum(), (z * y).sum(), (z * x).sum(), (y * x).sum()]
            assert r[23] == np.flatnonzero(lab.ravel() == k)[0]
            assert r[22] == int(((lab == k) & (other == 1)).sum())
            values = image[lab == k].astype(np.float64)
            scaled = [v * 2.0 ** q for v in values.tolist() if math.isfinite(v)]
            ks = [int(round(s)) for s in scaled]                    # Python's round: half to even, on an exact product
            ks = [v for v in ks if abs(v) < 2 ** 31]
            assert r[16] == len(ks) and r[19] == sum(ks) and int(r[20]) + (int(r[21]) << 32) == sum(v * v for v in ks)
            if ks:
                finite = values[np.isfinite(values) & (np.abs(np.rint(values * 2.0 ** q)) < 2.0 ** 31)].astype(np.float32)
                assert CC.key_value([r[17]])[0] == finite.min() and CC.key_value([r[18]])[0] == finite.max()


def test_numbering_is_scipys_own():
    check_numbering()


def test_rows_against_scipy_and_direct_computations():
    check_table()
    check_table(max_components=5)


def test_invalid_labels_and_ids_are_counted_and_enter_nothing():
    shape = (2, 33, 65)
    mask = CC.noise_mask(shape, 0.31, 3)
    labels = CC.sparse_labels(mask)
    n = labels.size
    bad = labels.copy().ravel()
    fg = np.flatnonzero(bad)
    bad[fg[0]] = n + 1                                      # beyond the volume
    bad[fg[1]] = -5
    bad[fg[2]] = 2 ** 31 - 1
    not_root = int(np.flatnonzero(labels.ravel() != np.arange(n) + 1)[0])
    bad[fg[3]] = not_root + 1                               # a voxel whose own label is another value
    dense, C, invalid = CC.rank_restate(bad.reshape(shape))
    assert invalid >= 4 and (dense.ravel()[fg[:4]] == 0).all() and dense.max() <= C
    good, C0, _ = CC.rank_restate(labels)
    odd = good.copy()
    odd.ravel()[fg[5]] = C0 + 1
    odd.ravel()[fg[6]] = -1
    rows, beyond, n_bad = CC.table_restate(odd, C0, max_components=C0)
    assert n_bad == 2 and beyond == 0 and rows[:, 0].sum() == len(fg) - 2


def test_quantisation():
    """ties to even at both parities and both signs, the representability edge, the values that enter nothing"""
    v = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.25, -0.0, 2.0 ** 31, np.nextafter(np.float32(2.0 ** 31), np.float32(0)), -2.0 ** 31,
                  np.nan, np.inf, -np.inf], np.float32)
    k, ok = CC.quantise(v, 0)
    assert list(k[:8]) == [0, 2, 2, 0, -2, -2, 0, 0] and list(ok) == [True] * 8 + [False, True, False, False, False, False]
    assert k[9] == 2 ** 31 - 128
    for q in (16, 30):
        edge = np.array([2.0 ** (31 - q), np.nextafter(np.float32(2.0 ** (31 - q)), np.float32(0)), (3 + 0.5) / 2.0 ** q, (4 + 0.5) / 2.0 ** q], np.float32)
        k, ok = CC.quantise(edge, q)
        assert list(ok) == [False, True, True, True] and list(k[2:]) == [4, 4]
    k, ok = CC.quantise(np.array([-32768, 32767], np.int16), 0)
    assert list(k) == [-32768, 32767] and ok.all()
    assert not CC.quantise(np.array([32767], np.int16), 30)[1].any()


@pytest.mark.parametrize("q", [0, 8, 16])
def test_derived_mean_and_std_within_the_stated_bound(q):
    shape = (2, 33, 65)
    mask = CC.blob_mask(shape, 4)
    image = CC.image_for(shape, 5)
    dense, rows, head = CC.chain_restate(mask.astype(np.uint8), image=image, q=q, other=mask.astype(np.uint8))
    figs = CS.derive_components(rows, spacing=(2.5, 0.8, 0.8), scale_log2=q)
    assert len(figs) == head[0] > 3 and [f["id"] for f in figs] == list(range(1, head[0] + 1))
    bound = 2.0 ** -(q + 1)
    for f in figs:
        values = image[dense == f["id"]].astype(np.float64)
        mean = math.fsum(values) / len(values)
        std = math.sqrt(math.fsum((values - mean) ** 2) / len(values))
        assert abs(f["mean"] - mean) <= bound and abs(f["std"] - std) <= bound, (f["id"], f["mean"] - mean, f["std"] - std)
        assert f["min"] == values.min() and f["max"] == values.max() and f["voxels"] == len(values) and f["n_unsummed"] == 0
        assert f["overlap_fraction"] == 1.0 and f["volume_ml"] == pytest.approx(len(values) * 1.6 / 1000.0)
        z = np.nonzero(dense == f["id"])[0]
        assert f["bbox"][0][0] == z.min() and f["extent_mm"][0] == (z.max() - z.min() + 1) * 2.5 and f["centroid"][0] == pytest.approx(z.mean())


def test_detection_counts_are_the_any_overlap_rule():
    shape = (1, 8, 40)
    truth = np.zeros(shape, np.uint8)
    pred = np.zeros(shape, np.uint8)
    truth[0, 1, 0:10] = 1           # detected by one voxel of ten
    truth[0, 3, 0:4] = 1            # missed
    truth[0, 5, 20:30] = 1          # detected by two fragments
    pred[0, 1, 9:14] = 1            # true positive: 1 of 5 voxels overlap
    pred[0, 5, 18:22] = 1           # true positive: 2 of 4
    pred[0, 5, 26:28] = 1           # true positive: 2 of 2
    pred[0, 7, 30:37] = 1           # false positive, 7 voxels
    rows_p = CC.chain_restate(pred, other=truth)[1]
    rows_t = CC.chain_restate(truth, other=pred)[1]
    got = CS.detection_counts(rows_p, rows_t)
    assert got == {"n_pred": 4, "n_truth": 3, "tp": 3, "fp": 1, "detected": 2, "fn": 1, "fp_voxels": 7, "sensitivity": 2 / 3, "precision": 3 / 4,
                   "f1": 2 * (2 / 3) * (3 / 4) / (2 / 3 + 3 / 4)}
    half = CS.detection_counts(rows_p, rows_t, min_overlap=0.5)         # ceil(0.5 n): the 1-of-5 and the 1-of-10 fall out
    assert (half["tp"], half["fp"], half["detected"], half["fn"]) == (2, 2, 0, 3) and half["fp_voxels"] == 12
    assert CS.detection_counts(rows_p, rows_t, min_overlap=2)["tp"] == 2
    none = CS.detection_counts(rows_p[:0], rows_t)
    assert none["precision"] is None and none["f1"] is None and none["sensitivity"] == 2 / 3
    for bad in (0, -1, 0.0, 1.5):
        with pytest.raises(ValueError):
            CS.detection_counts(rows_p, rows_t, min_overlap=bad)
    heads = np.zeros((2, 1, 4), np.int64)
    heads[:, 0, 0] = 4, 3
    fig = CS.detection_figures(np.stack([rows_p, rows_t])[:, None], heads, spacing=(2.0, 0.5, 0.5))[0]
    assert CS.detection_line_suffix(fig, False) == " comp 4 (3) det 2/3 fp 1 fpvol 7"
    assert CS.detection_line_suffix(fig, True) == " comp 4 (3) det 2/3 fp 1 fpvol 0.0035 mL"
    assert CS.detection_mean_suffix([fig, fig], False) == " comp 4.00 (3.00) det 0.6667 fp 1.00 fpvol 7.0000"
    heads[0, 0, 1] = 1
    with pytest.raises(RuntimeError, match="invalid"):
        CS.detection_figures(np.stack([rows_p, rows_t])[:, None], heads)


@pytest.mark.parametrize("defect", CC.DEFECTS)
def test_seeded_defects_fail_the_checks(defect):
    assert len(CC.DEFECTS) >= 6
    with pytest.raises(AssertionError):
        if defect in ("seam_off_by_one", "inclusive_scan"):
            check_numbering(defect)
        elif defect == "beyond_into_last_row":
            check_table(defect, max_components=5)
        else:
            check_table(defect)


def test_host_layer_refusals_and_layout():
    import torch
    assert CS._compstat_workspace_layout(2, 33, 65) == ((64, 64 + 16), 64 + 16 + 4 * 4290)
    assert CS._compstat_workspace_layout(257, 64, 64) == ((64, 64 + 4 * 260), 64 + 4 * 260 + 4 * 257 * 4096)
    assert CS.components_option(False) == 0 and CS.components_option(True) == 4096 and CS.components_option(7) == 7
    for bad in (0, 65537, 1.5, "8"):
        with pytest.raises(ValueError):
            CS.components_option(bad)
    labels = torch.zeros((2, 3, 4), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CS.rank_components(labels)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CS.tally_components(labels)
    for call in (lambda: CS.rank_components(labels.long()), lambda: CS.rank_components(labels, out=labels),
                 lambda: CS.tally_components(labels, max_components=0), lambda: CS.tally_components(labels, scale_log2=31),
                 lambda: CS.tally_components(labels, image=torch.zeros((2, 3, 4), dtype=torch.float64)),
                 lambda: CS.tally_components(labels, other=torch.zeros((2, 3, 5), dtype=torch.uint8)),
                 lambda: CS.component_table(labels, connectivity=18), lambda: CS.derive_components(np.zeros((3, 20), np.int64))):
        with pytest.raises(ValueError):
            call()
