"""tests/resample_cases.py (the numpy restatement of include/rpnet_resample_abi.h that the GPU tests compare with for equality) pinned to
scipy.ndimage.zoom, the host helpers of rpnet_amd.resample, and the seeded defects of the restatement, each of which must fail.  Runs
without a GPU."""
import numpy as np
import pytest
from scipy import ndimage

from rpnet_amd import resample as RS
from tests import resample_cases as RC

SHAPES = RC.SMALL + (((4, 9, 11), (7, 4, 30)), ((12, 10, 3), (5, 23, 8)))
EPS = 2.0 ** -52


def zoom(v, shape, order, align):
    return ndimage.zoom(v, [m / n for n, m in zip(v.shape, shape)], order=order, mode="nearest", grid_mode=align == "center")


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_linear_restatement_is_scipy_zoom_within_the_rounding_bound(capsys):
    """order 1 under both alignments.  The bound is derived, not measured.  Both routes interpolate the same piecewise linear function
    of the coordinates; they differ in (a) the coordinate: this definition rounds it once or twice and scipy forms it as o * zoom (and
    (o + 0.5) * zoom - 0.5), a few roundings of a number below n, which moves it by at most 2^-52 * n on an axis of input length n, and a
    piecewise linear interpolant changes by at most the value range per unit of coordinate, so 2^-52 * n * range per axis; (b) the
    arithmetic on the result: three roundings per lerp and three lerps on the path of a value here, against scipy's weighted sum, nine
    roundings of a number no larger than max|v|, each 2^-53 relative."""
    worst = 0.0
    for shape_in, shape_out in SHAPES:
        v = RC.noise_image(shape_in, np.float32, seed=2).astype(np.float64)
        vrange, vmax = float(v.max() - v.min()), float(np.abs(v).max())
        bound = EPS * sum(shape_in) * vrange + 9 * 2.0 ** -53 * vmax
        for align in RC.ALIGNS:
            got, want = RC.linear_f64(v, shape_out, align), zoom(v, shape_out, 1, align)
            assert got.shape == want.shape == tuple(shape_out)
            err = float(np.abs(got - want).max())
            worst = max(worst, err / max(vmax, 1e-300))
            with capsys.disabled():
                print(f"\n  linear {shape_in} -> {shape_out} {align}: max|restatement - zoom| = {err:.3e}, bound {bound:.3e}", end="")
            assert err <= bound, (shape_in, shape_out, align, err, bound)
    with capsys.disabled():
        print(f"\n  worst error over max|v|: {worst:.3e}")


def test_nearest_restatement_is_scipy_zoom_where_no_coordinate_is_a_tie():
    """order 0 is compared for equality on grids where no coordinate lies exactly half way between two voxels; the tie rule
    (floor(c + 0.5)) is this project's own, and the case tables do contain ties, which the comparison leaves out by that test alone"""
    compared = skipped = 0
    for shape_in, shape_out in SHAPES:
        v = RC.noise_image(shape_in, np.int16, seed=3)
        for align in RC.ALIGNS:
            if any(RC.has_exact_tie(n, m, align) for n, m in zip(shape_in, shape_out)):
                skipped += 1
                continue
            compared += 1
            assert np.array_equal(RC.ref_image(v, shape_out, 0, align), zoom(v, shape_out, 0, align)), (shape_in, shape_out, align)
    assert compared >= 12 and skipped >= 1
    assert RC.has_exact_tie(2, 3, "corner") and not RC.has_exact_tie(5, 8, "corner") and RC.has_exact_tie(4, 2, "center")
    # the tie of 2 -> 3 under corner (c = 0.5) goes up
    assert RC.nearest_table(2, 3, "corner").tolist() == [0, 1, 1]


def test_identity_is_bit_exact_with_non_finite_voxels():
    v = RC.noise_image((4, 5, 6), np.float32)
    v[0, 0, 0], v[1, 2, 3], v[3, 4, 5], v[2, 2, 2] = np.nan, np.inf, -np.inf, -0.0
    for align in RC.ALIGNS:
        for order in (0, 1):
            assert same_bits(RC.ref_image(v, v.shape, order, align), v), (align, order)
    i16 = RC.noise_image((4, 5, 6), np.int16)
    i16.flat[:2] = (-32768, 32767)
    for align in RC.ALIGNS:
        assert same_bits(RC.ref_image(i16, i16.shape, 1, align), i16)
    # a non-finite neighbour beside a tap of weight zero does not leak: 3 -> 5 under corner has t == 0 at o = 0, 2, 4
    line = np.array([1.0, np.inf, 2.0], np.float32).reshape(1, 1, 3)
    out = RC.ref_image(line, (1, 1, 5), 1, "corner")[0, 0]
    assert out[0] == 1.0 and out[4] == 2.0 and np.isinf(out[2]) and np.isinf(out[1])
    line[0, 0, 1] = np.nan
    out = RC.ref_image(line, (1, 1, 5), 1, "corner")[0, 0]
    assert out[0] == 1.0 and out[4] == 2.0 and np.isnan(out[1:4]).all()


def test_output_shape_and_out_spacing():
    # n * s / s' = 2.5 -> 2 and 3.5 -> 4 (half to even), and never below 1
    assert RS.output_shape((5, 7, 1), (1.0, 1.0, 1.0), (2.0, 2.0, 8.0)) == (2, 4, 1)
    assert RS.output_shape((64, 256, 256), (2.5, 0.8, 0.8), (2, 2, 2)) == (80, 102, 102) == RC.ref_output_shape((64, 256, 256), (2.5, 0.8, 0.8), (2, 2, 2))
    assert RS.out_spacing((64, 256, 256), (80, 102, 102), (2.5, 0.8, 0.8), "center") == (2.5 * 64 / 80, 0.8 * 256 / 102, 0.8 * 256 / 102)
    assert RS.out_spacing((64, 256, 256), (80, 102, 102), (2.5, 0.8, 0.8), "corner") == (2.5 * 63 / 79, 0.8 * 255 / 101, 0.8 * 255 / 101)
    assert RS.out_spacing((5, 7, 9), (1, 7, 3), (2.5, 0.8, 0.7), "corner") == (2.5, 0.8, 0.7 * 8 / 2)
    for align in RC.ALIGNS:
        assert RS.out_spacing((5, 7, 9), (8, 5, 13), (2.5, 0.8, 0.7), align) == RC.ref_out_spacing((5, 7, 9), (8, 5, 13), (2.5, 0.8, 0.7), align)
        assert RS.out_spacing((5, 7, 9), (5, 7, 9), (2.5, 0.8, 0.7), align) == (2.5, 0.8, 0.7)
    # under center the extent is kept, under corner the span of the voxel centres
    assert np.isclose(80 * RS.out_spacing((64, 1, 1), (80, 1, 1), (2.5, 1, 1), "center")[0], 64 * 2.5)
    assert np.isclose(79 * RS.out_spacing((64, 1, 1), (80, 1, 1), (2.5, 1, 1), "corner")[0], 63 * 2.5)
    for bad in ((1, 2), (1, 2, 0), (1, 2, float("nan")), "abc"):
        with pytest.raises(ValueError, match="spacing must be"):
            RS.output_shape((5, 7, 9), bad, (1, 1, 1))
    with pytest.raises(ValueError, match="align must be"):
        RS.out_spacing((5, 7, 9), (5, 7, 9), (1, 1, 1), "edge")
    for bad in ((5, 7), (5, 7, 0), (5, 7, 1025), (5, 7, 2.5)):
        with pytest.raises(ValueError, match="three axis lengths"):
            RS.check_grid(bad, "resample_image")


def test_the_rules_at_their_edges():
    """the int16 conversion (half to even, saturation), the label rule at exactly 0.5, the merge over 0 only"""
    r = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 40000.0, -40000.0, 32767.4, -32768.5])
    assert RC.convert(r, np.int16).tolist() == [0, 2, 2, 0, -2, 32767, -32768, 32767, -32768]
    pair = lambda a, b: np.array([a, b], np.int16).reshape(1, 1, 2)  # noqa: E731
    assert RC.ref_image(pair(0, 1), (1, 1, 3), 1, "corner")[0, 0].tolist() == [0, 0, 1]       # c = 0.5: 0.5 -> 0
    assert RC.ref_image(pair(1, 2), (1, 1, 3), 1, "corner")[0, 0].tolist() == [1, 2, 2]       # 1.5 -> 2
    assert RC.ref_image(pair(-32768, 32767), (1, 1, 3), 1, "corner")[0, 0].tolist() == [-32768, 0, 32767]
    lab = np.array([3, 0], np.uint8).reshape(1, 1, 2)
    out, rows = RC.ref_labels(lab, (1, 1, 3), (3,), "linear", "corner")
    assert out[0, 0].tolist() == [3, 0, 0] and rows.tolist() == [[1, 1, 3, 0]]                  # the indicator is exactly 0.5 at o = 1
    two = np.array([1, 1, 2, 2], np.uint8).reshape(1, 1, 4)
    out, rows = RC.ref_labels(two, (1, 1, 7), (1, 2), "linear", "corner")
    assert out[0, 0].tolist() == [1, 1, 1, 0, 2, 2, 2] and rows.tolist() == [[2, 3, 7, 0], [2, 3, 7, 0]]


def defect_inputs():
    img = RC.noise_image((5, 7, 9), np.float32, seed=5)
    i16 = RC.noise_image((5, 7, 9), np.int16, seed=5)
    lab = RC.label_map((6, 8, 10), seed=1)
    return img, i16, lab


@pytest.mark.parametrize("defect", RC.DEFECTS)
def test_a_seeded_defect_fails(defect):
    """each rule of the definition, switched to a plausible wrong one, changes a result the GPU tests compare for equality"""
    img, i16, lab = defect_inputs()
    d = {defect}
    if defect == "other alignment":
        changed = not same_bits(RC.ref_image(img, (8, 5, 13), 1, "corner", d), RC.ref_image(img, (8, 5, 13), 1, "corner"))
    elif defect == "no far clamp":      # past the last voxel centre under center when the grid grows
        changed = not same_bits(RC.ref_image(img, (8, 9, 13), 1, "center", d), RC.ref_image(img, (8, 9, 13), 1, "center"))
    elif defect == "z before x":        # the same taps, another order of the roundings
        changed = not same_bits(RC.ref_image(img, (8, 5, 13), 1, "corner", d), RC.ref_image(img, (8, 5, 13), 1, "corner"))
    elif defect == "floor for nearest":
        changed = not same_bits(RC.ref_image(img, (8, 5, 13), 0, "corner", d), RC.ref_image(img, (8, 5, 13), 0, "corner"))
    elif defect == "label >=":          # 2 -> 3 under corner: the indicator is exactly 0.5 in the middle
        one = np.array([3, 0], np.uint8).reshape(1, 1, 2)
        changed = not np.array_equal(RC.ref_labels(one, (1, 1, 3), (3,), "linear", "corner", d)[0], RC.ref_labels(one, (1, 1, 3), (3,), "linear")[0])
    elif defect == "int16 truncation":
        changed = not same_bits(RC.ref_image(i16, (8, 5, 13), 1, "corner", d), RC.ref_image(i16, (8, 5, 13), 1, "corner"))
    elif defect == "no saturation":
        r = np.array([40000.0, -40000.0, 12.0])
        changed = RC.convert(r, np.int16, d).tolist() != RC.convert(r, np.int16).tolist()
    else:
        assert defect == "merge over non-zero"
        # the indicators of two classes of one map never both pass 0.5, so the rule shows over what the output held before
        held = RC.ref_labels(RC.label_map((6, 8, 10), seed=2), (9, 5, 13), None, "nearest", "center")[0]
        a = RC.ref_labels(lab, (9, 5, 13), (1, 2, 5), "linear", "center", d, into=held)
        b = RC.ref_labels(lab, (9, 5, 13), (1, 2, 5), "linear", "center", into=held)
        assert np.array_equal(b[0][held != 0], held[held != 0]) and (b[0][held == 0] != 0).any()
        changed = not np.array_equal(a[0], b[0]) and a[1].tolist() != b[1].tolist()
    assert changed, defect


def test_label_restatement_properties():
    """nearest labels are a pick of input voxels; linear labels of a single class equal `zoom(indicator, order=1) > 0.5` away from the
    threshold; the class order decides a contested voxel; the rows count what they say"""
    lab = RC.label_map((6, 8, 10), seed=1)
    assert sorted(np.unique(lab).tolist()) == [0, 1, 2, 5]
    for align in RC.ALIGNS:
        out, rows = RC.ref_labels(lab, (9, 5, 13), (1, 2, 5), "nearest", align)
        assert set(np.unique(out).tolist()) <= {0, 1, 2, 5} and rows[:, 2].tolist() == [9 * 5 * 13] * 3
        assert rows[:, 0].tolist() == [int((lab == c).sum()) for c in (1, 2, 5)] and rows[:, 1].tolist() == [int((out == c).sum()) for c in (1, 2, 5)]
        z = zoom((lab == 2).astype(np.float64), (9, 5, 13), 1, align)
        mine, _ = RC.ref_labels(lab, (9, 5, 13), (2,), "linear", align)
        clear = np.abs(z - 0.5) > 1e-9
        assert clear.mean() > 0.9 and np.array_equal((mine == 2)[clear], (z > 0.5)[clear])
        fwd, _ = RC.ref_labels(lab, (9, 5, 13), (1, 2, 5), "linear", align)
        rev, _ = RC.ref_labels(lab, (9, 5, 13), (5, 2, 1), "linear", align)
        assert set(np.unique(fwd).tolist()) <= {0, 1, 2, 5}
        solo = {c: RC.ref_labels(lab, (9, 5, 13), (c,), "linear", align)[0] == c for c in (1, 2, 5)}
        assert np.array_equal(fwd == 1, solo[1]) and np.array_equal(rev == 5, solo[5])
        assert np.array_equal(fwd == 2, solo[2] & ~solo[1]) and np.array_equal(fwd == 5, solo[5] & ~solo[1] & ~solo[2])
