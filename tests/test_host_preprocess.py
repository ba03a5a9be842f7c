"""tests/preprocess_cases.py, the numpy restatement the GPU tests of rpnet_amd.preprocess compare with, pinned to an exact Otsu in
fractions, to scipy.ndimage and to np.where; every seeded defect must be noticed; the Python-side option parsing.  Runs without a GPU."""
from fractions import Fraction

import numpy as np
import pytest
from scipy import ndimage

from rpnet_amd import preprocess as PP
from tests import morphology_cases as MX
from tests import preprocess_cases as PC

ROUNDING = Fraction(1, 10 ** 12)        # val(k) is three roundings of 2^-53 from the exact quotient: far below this gap


def _exact_scan(counts):
    """the between-class variance of every cut from the class weights and means, in fractions -> (first argmax, {k: variance})"""
    c = [int(v) for v in counts]
    N, total = sum(c), sum(b * v for b, v in enumerate(c))
    out = {}
    for k in range(PC.BINS - 1):
        w0 = sum(c[:k + 1])
        if not 0 < w0 < N:
            continue
        m0 = sum(b * v for b, v in enumerate(c[:k + 1]))
        mu0, mu1 = Fraction(m0, w0), Fraction(total - m0, N - w0)
        out[k] = Fraction(w0, N) * Fraction(N - w0, N) * (mu0 - mu1) ** 2
    best = max(out.values())
    return min(k for k, v in out.items() if v == best), out


def _slices():
    for dtype in (np.float32, np.int16):
        for name, img in PC.threshold_cases(dtype) + [("noise image", PC.noise_image((4, 40, 50), dtype, seed=2)),
                                                       ("phantom", PC.body_phantom((2, 96, 96), dtype)[0])]:
            for z in range(img.shape[0]):
                yield f"{dtype.__name__} {name} {z}", img[z]


def test_otsu_scan_equals_the_exact_one():
    """k* of the float64 scan == the first maximum of the exact between-class variance, on every slice of the case table whose best two
    distinct variances differ by more than rounding (asserted about the inputs); an exact tie between two cuts goes to the first"""
    checked = 0
    for name, s in _slices():
        b, lo, hi, nf = PC.slice_bins(s)
        if b is None:
            continue
        counts = np.bincount(b[b >= 0], minlength=PC.BINS)
        assert counts.sum() == nf and counts[0] > 0 and counts[PC.BINS - 1] > 0, name
        k_exact, exact = _exact_scan(counts)
        ranked = sorted(set(exact.values()), reverse=True)
        assert len(ranked) == 1 or (ranked[0] - ranked[1]) > ROUNDING * ranked[0], name      # about the inputs
        k, vals = PC.otsu_scan(counts)
        assert k == k_exact, (name, k, k_exact)
        assert all((v is None) == (j not in exact) for j, v in enumerate(vals)), name
        for j, v in enumerate(vals):
            if v is not None:
                want = exact[j] * sum(int(c) for c in counts) ** 2          # val(k) = N^2 times the variance
                assert abs(Fraction(float(v)) - want) <= want / 10 ** 14, (name, j)
        checked += 1
    assert checked > 30
    # two bins only: every cut between them has the same variance, exactly; the first one wins
    two = np.zeros(PC.BINS, np.int64)
    two[0], two[127] = 5, 7
    assert PC.otsu_scan(two)[0] == 0 == _exact_scan(two)[0] and PC.otsu_scan(two, "last_maximum")[0] == 126


def test_threshold_rows_and_masks():
    """what the rows say against plain numpy: the clamp of hi to bin 127, bin edges, the empty slices, non-finite voxels, the fixed
    threshold at, below and above a value"""
    cases = dict(PC.threshold_cases(np.float32))
    mask, rows, frows = PC.ref_threshold(cases["bin edges and hi"])
    edges = cases["bin edges and hi"][0]
    b, lo, hi, _ = PC.slice_bins(edges)
    assert (lo, hi) == (0.0, 128.0) and np.array_equal(b, np.minimum(edges.astype(np.int64), 127)) and b.max() == 127
    assert np.array_equal(mask[0], b > rows[0, 1]) and frows[0, 2] == rows[0, 1] + 1.0
    mask, rows, frows = PC.ref_threshold(cases["constant slices"])
    assert not mask.any() and rows.tolist() == [[48, -1, 0, 0]] * 2 and frows.tolist() == [[5.0, 5.0, 5.0], [-7.0, -7.0, -7.0]]
    mask, rows, frows = PC.ref_threshold(cases["non-finite"])
    assert rows[:, 0].tolist() == [45, 42, 24, 0, 48] and rows[3].tolist() == [0, -1, 0, 0] and frows[3].tolist() == [0.0, 0.0, 0.0]
    assert rows[4].tolist() == [48, -1, 0, 0] and not mask[3].any() and not mask[4].any()
    assert not mask[0, 0, 0] and not mask[0, 1, 1] and not mask[0, 2, 2] and not mask[1, :, 0].any() and mask[1].any()
    mask, rows, frows = PC.ref_threshold(cases["two values"])
    assert np.array_equal(mask[0], cases["two values"][0] == 100) and rows[0, 1] == 0
    img = cases["non-finite"]
    for t in PC.fixed_thresholds(img):
        mask, rows, frows = PC.ref_threshold(img, t)
        with np.errstate(invalid="ignore"):
            assert np.array_equal(mask, (img.astype(np.float64) > t).astype(np.uint8)) and (rows[:, 1] == -1).all() and (frows[:, 2] == t).all()
        assert mask[1, :, 0].all() and not mask[3].any()             # +inf is above every threshold, NaN above none
    v = PC.fixed_thresholds(img)[0]
    assert float(img[0, 0, 4]) == v                                 # the value the thresholds bracket (in float64: float32 cannot tell them apart)
    at, below, above = (PC.ref_threshold(img, t)[0][0, 0, 4] for t in PC.fixed_thresholds(img)[:3])
    assert (at, below, above) == (0, 1, 0)
    i16 = dict(PC.threshold_cases(np.int16))["int16 limits"]
    mask, rows, frows = PC.ref_threshold(i16)
    assert frows[0, :2].tolist() == [-32768.0, 32767.0] and np.array_equal(mask[0], i16[0] == 32767)


@pytest.mark.parametrize("connectivity", (4, 8))
def test_seeded_component_equals_scipy_label(connectivity):
    """the flood fill == scipy.ndimage.label of every slice with the 2D structure, followed by the label at the seed"""
    st = ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2)
    for shape in ((3, 9, 11), (5, 33, 65), (4, 20, 7)):
        for name, vol, seed in PC.component_cases(shape):
            for cls, v in ((1, vol), (2, vol * 2 + (vol == 0) * (MX.noise(shape, 0.3, seed=8) * 3))):
                out, rows = PC.ref_seeded(v, cls, seed, connectivity)
                sy, sx = seed or (shape[1] // 2, shape[2] // 2)
                for z in range(shape[0]):
                    lab, n = ndimage.label(v[z] == cls, structure=st)
                    keep = (lab == lab[sy, sx]) & (lab > 0)
                    want = v[z].copy()
                    want[(v[z] == cls) & ~keep] = 0
                    assert np.array_equal(out[z], want), (shape, name, cls, z)
                    assert rows[z].tolist() == [int(lab[sy, sx] > 0), int((v[z] == cls).sum()), int(keep.sum()), n], (shape, name, cls, z)
    diag = dict((n, v) for n, v, _ in PC.component_cases((2, 9, 11)))["diagonal contact"]
    assert PC.ref_seeded(diag, 1, None, 4)[1][0].tolist()[1:] == [5, 1, 2] and PC.ref_seeded(diag, 1, None, 8)[1][0].tolist()[1:] == [5, 5, 1]


def _scipy_chain(vol, radius, connectivity, hole_connectivity, erode_border):
    st2 = MX.structure_of(MX.voxel_ball(int(radius * radius), per_slice=True))[0]
    m = PC.ref_threshold(vol)[0].astype(bool)
    out = np.zeros(m.shape, np.uint8)
    H, W = m.shape[1:]
    for z in range(m.shape[0]):
        s = ndimage.binary_erosion(ndimage.binary_dilation(m[z], structure=st2), structure=st2, border_value=erode_border)
        s = ndimage.binary_dilation(ndimage.binary_erosion(s, structure=st2, border_value=erode_border), structure=st2)
        lab, _ = ndimage.label(s, structure=ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2))
        s = (lab == lab[H // 2, W // 2]) & (lab > 0)
        out[z] = ndimage.binary_fill_holes(s, structure=ndimage.generate_binary_structure(2, 1 if hole_connectivity == 4 else 2))
    return out


def test_chain_equals_the_scipy_pieces():
    """body_mask by the restatements == threshold, binary closing and opening with the ball of tests/morphology_cases.py, label and the
    label at the centre, binary_fill_holes, slice by slice; on the phantom the table and the speck are gone and the pockets filled"""
    img, body, pockets, table, speck = PC.body_phantom()
    for kw in (dict(radius=7), dict(radius=3, connectivity=8, hole_connectivity=8, erode_border=0), dict(radius=2)):
        m, tables = PC.ref_body_mask(img, **kw)
        want = _scipy_chain(img, kw["radius"], kw.get("connectivity", 4), kw.get("hole_connectivity", 4), kw.get("erode_border", 1))
        assert np.array_equal(m, want), kw
        assert tables["voxels"][-1] == m.sum() and tables["voxels"][0] == tables["threshold"][:, 2].sum()
    m, tables = PC.ref_body_mask(img)
    assert not m[table].any() and not m[speck].any() and m[pockets].all() and m[body].mean() > 0.97 and m[~body].mean() < 0.02
    assert (tables["seed"][:, 0] == 1).all() and tables["voxels"][4] >= tables["voxels"][3] >= m[body & ~pockets].sum() - 50
    m1, t1 = PC.ref_body_mask(img, radius=1)                # a ball the table bar survives: the seed stage is what drops it
    assert t1["voxels"][2] - t1["voxels"][3] >= table.sum() // 3 and (t1["seed"][:, 3] >= 2).all()
    assert not m1[table].any() and not m1[speck].any() and m1[pockets].all() and t1["voxels"][4] > t1["voxels"][3]      # holes filled the pockets
    noise = PC.noise_image((3, 40, 50), np.int16, seed=4)
    assert np.array_equal(PC.ref_body_mask(noise, radius=2)[0], _scipy_chain(noise, 2, 4, 4, 1))


def test_box_equals_np_where():
    rng = np.random.default_rng(3)
    for dtype in (np.float32, np.int16):
        img = rng.integers(-1100, 300, (5, 9, 11)).astype(dtype)
        img[2, 3, 4] = -1024
        for name, mask in (("noise", MX.noise(img.shape, 0.2)), ("empty", np.zeros(img.shape, np.uint8)), ("full", np.ones(img.shape, np.uint8)),
                           ("values above 1", MX.noise(img.shape, 0.5, seed=2) * 7)):
            out, row = PC.ref_mask_bbox(img, mask)
            processed = img.copy()
            processed[mask == 0] = -1024
            assert np.array_equal(out, processed) and out.dtype == img.dtype, name
            zz, yy, xx = np.where(processed > -1024)
            if zz.size == 0:
                assert row.tolist() == [-1] * 6 + [0, int((mask != 0).sum())], name
                continue
            assert row.tolist() == [zz.min(), zz.max(), yy.min(), yy.max(), xx.min(), xx.max(), zz.size, int((mask != 0).sum())], name
            y0, y1, x0, x1 = PC.ref_crop(row)
            assert np.array_equal(processed[:, y0:y1, x0:x1], processed[:, yy.min():yy.max(), xx.min():xx.max()])      # the reference's cut
            assert PC.ref_crop(row, False) == (yy.min(), yy.max() + 1, xx.min(), xx.max() + 1)
            assert PP.crop_box(row) == PC.ref_crop(row) and PP.crop_box(row, False) == PC.ref_crop(row, False)
    with pytest.raises(ValueError, match="the box is empty"):
        PP.crop_box(PC.ref_mask_bbox(img, np.zeros(img.shape, np.uint8))[1])
    one = np.zeros(img.shape, np.uint8)
    one[1, 2, 3] = 1
    assert PC.ref_mask_bbox(np.zeros(img.shape, np.float32), one)[1].tolist() == [1, 1, 2, 2, 3, 3, 1, 1]
    with pytest.raises(ValueError, match="half-open crop"):
        PP.crop_box([1, 1, 2, 2, 3, 3, 1, 1])
    assert PP.crop_box([1, 1, 2, 2, 3, 3, 1, 1], False) == (2, 3, 3, 4)
    nan = np.full(img.shape, np.nan, np.float32)
    assert PC.ref_mask_bbox(nan, one)[1].tolist() == [-1] * 6 + [0, 1]              # NaN is not above the fill value


def test_every_seeded_defect_is_noticed():
    """each wrong variant differs from the definition on a case of the tables, and the check that pins the definition fails for it"""
    img = np.stack([np.arange(2000.0).reshape(40, 50), np.arange(2000.0).reshape(40, 50) ** 1.5]).astype(np.float32)   # every bin is populated
    good = PC.ref_threshold(img)
    for defect in PC.THRESHOLD_DEFECTS[:2]:
        bad = PC.ref_threshold(img, defect=defect)
        assert not np.array_equal(bad[0], good[0]) and not np.array_equal(bad[1], good[1]), defect
    # the bin of the cut itself is background: `>=` takes it
    b, _, _, _ = PC.slice_bins(img[0])
    assert (b == good[1][0, 1]).any() and not good[0][0][b == good[1][0, 1]].any()
    assert PC.ref_threshold(img, defect="ge_at_the_bin")[0][0][b == good[1][0, 1]].all()
    # the last maximum: two populated bins tie exactly over every cut between them
    two = dict(PC.threshold_cases(np.int16))["two values"]
    good, bad = PC.ref_threshold(two), PC.ref_threshold(two, defect="last_maximum")
    assert good[1][0, 1] == 0 and bad[1][0, 1] == 126 and good[2][0, 2] != bad[2][0, 2]
    counts = np.bincount(PC.slice_bins(two[0])[0].ravel(), minlength=PC.BINS)
    assert PC.otsu_scan(counts, "last_maximum")[0] != _exact_scan(counts)[0] == PC.otsu_scan(counts)[0]

    shape = (4, 20, 7)                                      # not square: (y, x) and (x, y) are different pixels
    cases = {n: (v, s) for n, v, s in PC.component_cases(shape)}
    leak = cases["no leak across z"][0]
    good, bad = PC.ref_seeded(leak, 1, None, 4), PC.ref_seeded(leak, 1, None, 4, defect="z_link")
    assert good[1][:, 0].tolist() == [1, 0, 1, 0] and not good[0][1::2].any() and bad[0][1::2].any()
    st = ndimage.generate_binary_structure(2, 1)
    lab = ndimage.label(leak[1] == 1, structure=st)[0]
    assert not np.array_equal(bad[0][1], np.where((lab == lab[10, 3]) & (lab > 0), 1, 0))           # the scipy pin fails for it
    col = np.zeros(shape, np.uint8)
    col[:, 10, 3] = 1                                       # only the centre pixel (H // 2, W // 2) = (10, 3)
    good, bad = PC.ref_seeded(col, 1, None, 4), PC.ref_seeded(col, 1, None, 4, defect="seed_swapped")
    assert good[1][:, 0].all() and good[0].sum() == 4 and not bad[1][:, 0].any() and not bad[0].any()

    img = np.zeros((3, 9, 11), np.int16)
    mask = np.zeros(img.shape, np.uint8)
    mask[1, 2:6, 3:8] = 1
    img[1, 5, :] = -1024                                    # a masked row at the fill value: it is not kept
    img[1, 4, 7] = -2000                                    # and one below it
    row = PC.ref_mask_bbox(img, mask)[1]
    assert row.tolist() == [1, 1, 2, 4, 3, 7, 14, 20]
    assert PC.ref_mask_bbox(img, mask, defect="count_at_fill")[1].tolist() == [1, 1, 2, 5, 3, 7, 19, 20]
    processed = np.where(mask != 0, img, -1024)
    _, yy, xx = np.where(processed > -1024)
    assert PC.ref_crop(row) == (yy.min(), yy.max(), xx.min(), xx.max()) != PC.ref_crop(row, defect="inclusive_crop")
    assert processed[:, 2:4, 3:7].shape == processed[:, slice(*PC.ref_crop(row)[:2]), slice(*PC.ref_crop(row)[2:])].shape
    assert len(PC.THRESHOLD_DEFECTS + PC.SEED_DEFECTS + PC.BOX_DEFECTS) == 7


def test_option_parsing_needs_no_gpu():
    assert PP.check_seed(None, 20, 7) == (10, 3) and PP.check_seed((0, 6), 20, 7) == (0, 6)
    for bad in ((20, 0), (0, 7), (-1, 0), (1.0, 2), (1,), "centre", (True, 1)):
        with pytest.raises(ValueError, match="seed must be"):
            PP.check_seed(bad, 20, 7)
    import torch
    with pytest.raises(RuntimeError, match="MI355X only"):
        PP.threshold_mask(torch.zeros((2, 3, 4)))
    with pytest.raises(RuntimeError, match="MI355X only"):
        PP.body_mask(torch.zeros((2, 3, 4), dtype=torch.int16))
    assert PP.STAGES == ("threshold", "closing", "opening", "seed", "holes")
    assert (PP.FIXED, PP.OTSU, PP.IMAGE_KINDS[torch.float32], PP.IMAGE_KINDS[torch.int16]) == (0, 1, 0, 1)
