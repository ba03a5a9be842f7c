"""tests/morphology_cases.py, the numpy restatement the GPU tests of rpnet_amd.morphology compare with, pinned to scipy.ndimage, to the
thresholded distance transform and to the lattice properties; the seeded defects of the kernels' route must be noticed; the Python-side
refusals and the radius parsing.  Runs without a GPU."""
import numpy as np
import pytest
import torch
from scipy import ndimage

from rpnet_amd import morphology as MO
from rpnet_amd import surface_spacing as SS
from tests import morphology_cases as MX

SHAPE = (9, 12, 13)


def _objects(shape=SHAPE):
    return [(n, v.astype(bool)) for n, v in MX.contents(shape)]


@pytest.mark.parametrize("rho", MX.RHOS)
def test_voxel_ball_equals_scipy(rho):
    """dilation, erosion under both border values, opening and closing == scipy.ndimage with the ball as the structure, on noise, boxes
    and objects touching each face; rho = 1, 2, 3 are generate_binary_structure(3, 1 | 2 | 3)"""
    offsets = MX.voxel_ball(rho)
    st = MX.structure_of(offsets)
    assert len(offsets) == int(st.sum()) and st[tuple(s // 2 for s in st.shape)]
    if rho <= 3:
        assert np.array_equal(st, ndimage.generate_binary_structure(3, rho))
    for name, X in _objects():
        assert np.array_equal(MX.dilate_ref(X, offsets), ndimage.binary_dilation(X, structure=st)), name
        for b in (0, 1):
            ero = ndimage.binary_erosion(X, structure=st, border_value=b)
            assert np.array_equal(MX.erode_ref(X, offsets, b), ero), (name, b)
            assert np.array_equal(MX.binary_ref(X, MX.OPEN, offsets, b), ndimage.binary_dilation(ero, structure=st)), (name, b)
            dil = ndimage.binary_dilation(X, structure=st)
            assert np.array_equal(MX.binary_ref(X, MX.CLOSE, offsets, b), ndimage.binary_erosion(dil, structure=st, border_value=b)), (name, b)
        # scipy's own opening and closing are the border_value=0 compositions
        assert np.array_equal(MX.binary_ref(X, MX.OPEN, offsets, 0), ndimage.binary_opening(X, structure=st)), name
        assert np.array_equal(MX.binary_ref(X, MX.CLOSE, offsets, 0), ndimage.binary_closing(X, structure=st)), name
        # the clipped ball of a call on this shape is the same operation
        clipped = MX.voxel_ball(rho, SHAPE)
        assert np.array_equal(MX.erode_ref(X, clipped, 0), MX.erode_ref(X, offsets, 0)) and np.array_equal(MX.dilate_ref(X, clipped),
                                                                                                        MX.dilate_ref(X, offsets))


def test_per_slice_is_the_2d_operation_of_every_slice():
    for rho in (1, 2, 5, 9):
        offsets = MX.voxel_ball(rho, per_slice=True)
        st2 = MX.structure_of(offsets)[0]
        if rho <= 2:
            assert np.array_equal(st2, ndimage.generate_binary_structure(2, rho))
        for name, X in _objects():
            for z in range(X.shape[0]):
                assert np.array_equal(MX.dilate_ref(X, offsets)[z], ndimage.binary_dilation(X[z], structure=st2)), name
                for b in (0, 1):
                    assert np.array_equal(MX.erode_ref(X, offsets, b)[z], ndimage.binary_erosion(X[z], structure=st2, border_value=b)), name


def test_millimetre_ball_equals_scipy():
    """at spacing (1, 1, 1) the millimetre ball is the voxel ball of rho = floor(r^2); at (2.5, 0.8, 0.8) it equals scipy with the
    ellipsoid structure built by the same rule; r = 3 * 0.8 under 0.8 is decided by the rounded products"""
    big = (40, 40, 40)
    for r in (1.0, 1.5, 2.0, 2.9, 3.0, 7.0):
        assert sorted(MX.mm_ball((1.0, 1.0, 1.0), r, big)) == sorted(MX.voxel_ball(int(np.floor(r * r)), big)), r
    for r in (0.5, 0.8, 2.0, 2.4, 2.5, 3 * 0.8, 5.0):
        offsets = MX.mm_ball(MX.MM, r, SHAPE)
        assert (0, 0, 0) in offsets
        st = MX.structure_of(offsets)
        want = [(dz, dy, dx) for dz in range(-9, 10) for dy in range(-12, 13) for dx in range(-13, 14)
                if (0.8 * 0.8 * (dx * dx) + 0.8 * 0.8 * (dy * dy)) + 2.5 * 2.5 * (dz * dz) <= r * r]
        assert sorted(offsets) == sorted(want), r
        for name, X in _objects()[:5]:
            assert np.array_equal(MX.dilate_ref(X, offsets), ndimage.binary_dilation(X, structure=st)), (r, name)
            for b in (0, 1):
                assert np.array_equal(MX.erode_ref(X, offsets, b), ndimage.binary_erosion(X, structure=st, border_value=b)), (r, name, b)
    # 3 * 0.8 along x: fl(fl(0.8 * 0.8) * 9) against fl(fl(3 * 0.8) * fl(3 * 0.8)); whichever way it falls, the rule decides and a
    # radius one ulp larger or smaller brackets it
    w, r = MX.mm_weights(MX.MM), 3 * 0.8
    inside = bool(w[2] * np.float64(9) <= np.float64(r) * np.float64(r))
    assert ((0, 0, 3) in MX.mm_ball(MX.MM, r, SHAPE)) == inside
    assert (0, 0, 3) in MX.mm_ball(MX.MM, 2.41, SHAPE) and (0, 0, 3) not in MX.mm_ball(MX.MM, 2.39, SHAPE)


def test_restatement_equals_the_thresholded_transform():
    """dilate(X) = {d2(v, X) <= rho} and erode(X) = {d2(v, complement) > rho} with d2 the restated distance transform of
    rpnet_amd.surface_spacing: this pins the kernels' route to the definition, for both balls"""
    for name, X in _objects():
        for rho in (1, 3, 4, 9, 50):
            offsets, w = MX.voxel_ball(rho, SHAPE), (1.0, 1.0, 1.0)
            assert np.array_equal(MX.dilate_ref(X, offsets), SS.transform_reference_spacing(X, w) <= float(rho)), (name, rho)
            assert np.array_equal(MX.erode_ref(X, offsets, 1), SS.transform_reference_spacing(~X, w) > float(rho)), (name, rho)
        for r in (2.0, 3 * 0.8, 5.0):
            offsets, w = MX.mm_ball(MX.MM, r, SHAPE), SS.spacing_weights(MX.MM)
            assert np.array_equal(MX.dilate_ref(X, offsets), SS.transform_reference_spacing(X, w) <= r * r), (name, r)
            assert np.array_equal(MX.erode_ref(X, offsets, 1), SS.transform_reference_spacing(~X, w) > r * r), (name, r)


def _route_cases():
    """(volume, class, op, keywords): enough ground for every seeded defect to show"""
    lab = MX.labels((6, 10, 12))
    for vol in (MX.noise(SHAPE, 0.31), MX.noise(SHAPE, 0.9, 2), MX.corners(SHAPE), MX.ties(4, "axis"), lab):
        for op in MX.OPS:
            for kw in (dict(radius=("rho", 4)), dict(radius=("rho", 3), erode_border=0), dict(radius=("rho", 2), per_slice=True),
                       dict(radius=(2.4, "mm"), spacing=MX.MM), dict(radius=(2.5, "mm"), spacing=MX.MM, erode_border=0)):
                yield vol, (2 if vol is lab else 1), op, kw


def test_route_equals_the_restatement_and_seeded_defects_are_noticed():
    """the kernels' route (capped transform, fused threshold, write-back) equals the restatement on every case, and each of the six
    seeded defects fails that same comparison on at least one of them"""
    noticed = {d: 0 for d in MX.DEFECTS}
    for vol, cls, op, kw in _route_cases():
        want, row = MX.ref_apply(vol, cls, op, **kw)
        got, grow = MX.route_apply(vol, cls, op, **kw)
        assert np.array_equal(got, want) and grow.tolist() == row.tolist(), (op, kw)
        assert row[1] == row[0] + row[2] - row[3]
        for d in MX.DEFECTS:
            bad, brow = MX.route_apply(vol, cls, op, defect=d, **kw)
            noticed[d] += not (np.array_equal(bad, want) and brow.tolist() == row.tolist())
    assert len(MX.DEFECTS) >= 6 and all(noticed.values()), noticed


@pytest.mark.parametrize("density", [0.1, 0.5, 0.9])
def test_lattice_properties(density):
    """with erode_border=1: close(X) contains X, open(X) is contained in X, both idempotent; erode and dilate are adjoint duals"""
    X = MX.noise(SHAPE, density, seed=5).astype(bool)
    for offsets in (MX.voxel_ball(1, SHAPE), MX.voxel_ball(5, SHAPE), MX.voxel_ball(3, SHAPE, per_slice=True), MX.mm_ball(MX.MM, 2.5, SHAPE)):
        cl, op = MX.binary_ref(X, MX.CLOSE, offsets), MX.binary_ref(X, MX.OPEN, offsets)
        assert (cl >= X).all() and (op <= X).all()
        assert np.array_equal(MX.binary_ref(cl, MX.CLOSE, offsets), cl) and np.array_equal(MX.binary_ref(op, MX.OPEN, offsets), op)
        assert np.array_equal(MX.erode_ref(X, offsets, 1), ~MX.dilate_ref(~X, offsets))


def test_label_volume_rule():
    """gained voxels take the class only over 0, lost voxels become 0, other classes pass through, and the row says so"""
    lab = MX.labels((6, 10, 12))
    out, row = MX.ref_apply(lab, 1, MX.CLOSE, ("rho", 3))
    gain = MX.binary_ref(lab == 1, MX.CLOSE, MX.voxel_ball(3, lab.shape)) & (lab != 1)
    assert (gain & (lab != 0)).any() and (gain & (lab == 0)).any()
    assert np.array_equal(out[lab > 1], lab[lab > 1]) and (out[gain & (lab == 0)] == 1).all()
    assert row.tolist() == [(lab == 1).sum(), (out == 1).sum(), (gain & (lab == 0)).sum(), 0] and row[2] < gain.sum()
    out, row = MX.ref_apply(lab, 1, MX.OPEN, ("rho", 3))
    assert (out[(lab == 1) & (out != 1)] == 0).all() and row[2] == 0 and row[3] == ((lab == 1) & (out != 1)).sum() > 0
    assert MX.ref_counts(out, lab, 1).tolist() == [(out == 1).sum(), (out == 1).sum(), (lab == 1).sum()]


def test_radius_parsing_and_refusals():
    assert MO.check_radius(1) == ("rho", 1) and MO.check_radius(1.5) == ("rho", 2) and MO.check_radius(7) == ("rho", 49)
    assert MO.check_radius(np.float32(2.0)) == ("rho", 4) and MO.check_radius(("rho", 50)) == ("rho", 50)
    assert MO.check_radius((2.5, "mm")) == ("mm", 2.5) and MO.check_radius([3, "mm"]) == ("mm", 3.0)
    for bad in (0, 0.99, -1, None, True, "7", float("nan"), float("inf"), ("rho", 0), ("rho", 2.5), ("rho", MO.MAX_RHO + 1), (0, "mm"),
                (-1.0, "mm"), (float("inf"), "mm"), (2.0, "cm"), ("rho", "mm"), (1, 2, 3), 1800):
        with pytest.raises(ValueError, match="radius must be"):
            MO.check_radius(bad)
    assert MO.resolve_radius(2, None) == ("rho", 4) and MO.resolve_radius(2, MX.MM) == ("rho", 4)
    kind, w, r2 = MO.resolve_radius((2.4, "mm"), MX.MM)
    assert kind == "mm" and w == SS.spacing_weights(MX.MM) == tuple(float(v) for v in MX.mm_weights(MX.MM)) and r2 == 2.4 * 2.4
    with pytest.raises(ValueError, match="a radius in mm needs a spacing"):
        MO.resolve_radius((2.4, "mm"))
    for spacing in ((1.0, 1.0), (1.0, 0.0, 1.0), (1.0, float("nan"), 1.0), "abc"):
        with pytest.raises(ValueError, match="three finite positive numbers"):
            MO.resolve_radius((2.4, "mm"), spacing)
    vol = torch.zeros((2, 3, 4), dtype=torch.uint8)
    for fn in (MO.erode, MO.dilate, MO.opening, MO.closing):
        with pytest.raises(ValueError, match="radius must be"):
            fn(vol, (1,), 0)
        with pytest.raises(ValueError, match="erode_border must be"):
            fn(vol, (1,), 1, erode_border=2)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(vol, (1,), 1)
    assert MO.morph_figures(np.array([[5, 7, 3, 1], [4, 2, 0, 2]])) == [{"before": 5, "after": 7, "added": 3, "removed": 1},
                                                                        {"before": 4, "after": 2, "added": 0, "removed": 2}]
    f = MO.morph_figures(np.array([[5, 7, 3, 1], [4, 2, 0, 2]]))
    assert MO.line_suffix(f[0], None) == " open -1 +3" and MO.line_suffix(None, f[1]) == " close -2 +0" and MO.line_suffix() == ""
    assert MO.line_suffix(f[0], f[1]) == " open -1 +3 close -2 +0" and MO.mean_suffix(f, None) == " open -1.50 +1.50"
    assert MO.mean_suffix(None, f) == " close -1.50 +1.50" and MO.mean_suffix() == ""
