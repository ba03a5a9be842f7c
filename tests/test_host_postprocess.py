"""The numpy restatement of the two post-processing definitions (tests/postprocess_cases.py) against scipy.ndimage.binary_fill_holes
and scipy.ndimage.label + bincount, seeded defects against the comparison the GPU tests use, that the cases separate the modes, and the
host-side pieces of the feature: min_voxels_from_mm3, the option parsers, the figures and the suffixes.  Runs without a GPU."""
import inspect

import numpy as np
import pytest
from scipy import ndimage

from tests import postprocess_cases as PX


def _hole_cases():
    for shape in PX.SHAPES:
        for name, vol in PX.hole_contents(shape):
            yield shape, name, vol


@pytest.mark.parametrize("conn,per_slice", PX.HOLE_MODES)
def test_ref_fill_holes_is_scipy_binary_fill_holes(conn, per_slice):
    """on every case of the table (one foreground class, no bound): the 3D structures of rank 1 and 3, and per slice the 2D structures
    of rank 1 and 2; the statistics row counts what scipy's result shows"""
    for shape, name, vol in _hole_cases():
        obj = vol == 1
        if per_slice:
            structure = ndimage.generate_binary_structure(2, 1 if conn == 4 else 2)
            want = np.stack([ndimage.binary_fill_holes(obj[z], structure=structure) for z in range(shape[0])])
        else:
            want = ndimage.binary_fill_holes(obj, structure=ndimage.generate_binary_structure(3, 1 if conn == 6 else 3))
        got, row = PX.ref_fill_holes(np.where(obj, 1, 0), 1, conn, per_slice)
        assert got.dtype == np.uint8 and np.array_equal(got == 1, want), (shape, name)
        assert row[2] == want.sum() - obj.sum() and (row[1] == 0) == (row[2] == 0) and row[1] <= row[0], (shape, name)
        assert row[1] == len(PX.hole_sizes(np.where(obj, 1, 0), 1, conn, per_slice))
    # scipy's default structure is the rank-1 one: connectivity 6
    vol = PX.diagonal_chain((5, 33, 65))
    assert np.array_equal(PX.ref_fill_holes(vol, 1, 6)[0] == 1, ndimage.binary_fill_holes(vol == 1))


@pytest.mark.parametrize("conn,rank", [(6, 1), (26, 3)])
def test_ref_remove_small_is_scipy_label_and_bincount(conn, rank):
    structure = ndimage.generate_binary_structure(3, rank)
    for shape in PX.SHAPES:
        for name, vol in PX.small_contents(shape):
            lab, n = ndimage.label(vol == 1, structure=structure)
            sizes = np.bincount(lab.ravel(), minlength=n + 1)
            for m in PX.bounds_around(sizes[1:]):
                drop = sizes < m
                drop[0] = False
                want = vol.copy()
                want[drop[lab]] = 0
                got, row = PX.ref_remove_small(vol, 1, conn, m)
                assert np.array_equal(got, want), (shape, name, m)
                assert row.tolist() == [n, drop.sum(), sizes[drop].sum(), sizes[drop].max() if drop.any() else 0], (shape, name, m)


def _hole_runs(shape):
    """(name, volume, connectivity, per_slice, max_hole) of every comparison the GPU test makes at one extent"""
    for name, vol in PX.hole_contents(shape):
        for conn, per_slice in PX.HOLE_MODES:
            bounds = [None]
            if name in ("hollow box", "shell in cavity", "other class in hole", "noise 0.69"):
                bounds += PX.bounds_around(PX.hole_sizes(vol, 1, conn, per_slice))
            for b in bounds:
                yield name, vol, conn, per_slice, b


@pytest.mark.parametrize("defect", PX.HOLE_DEFECTS)
def test_seeded_hole_defects_fail_the_comparison(defect):
    caught = set()
    for shape in PX.BOX_SHAPES:
        for name, vol, conn, per_slice, b in _hole_runs(shape):
            good, bad = PX.ref_fill_holes(vol, 1, conn, per_slice, b), PX.ref_fill_holes(vol, 1, conn, per_slice, b, defect)
            if not (np.array_equal(good[0], bad[0]) and np.array_equal(good[1], bad[1])):
                caught.add((name, conn, per_slice))
    print(defect, sorted(caught))
    expect = {"face_left_out": ("face 5", 6, False), "z_links_per_slice": ("z channel", 4, True), "conn26_for_6": ("diagonal chain", 6, False),
              "hole_lt": ("hollow box", 6, False), "overwrite_other": ("other class in hole", 6, False)}[defect]
    assert expect in caught
    if defect == "z_links_per_slice":
        assert all(per_slice for _, _, per_slice in caught)
    if defect == "conn26_for_6":
        assert all(conn in (6, 4) for _, conn, _ in caught)
    if defect == "overwrite_other":
        assert all(name == "other class in hole" for name, _, _ in caught)


@pytest.mark.parametrize("defect", PX.SMALL_DEFECTS)
def test_seeded_small_defects_fail_the_comparison(defect):
    caught = set()
    for shape in PX.BOX_SHAPES:
        for name, vol in PX.small_contents(shape):
            for conn in (6, 26):
                for m in PX.bounds_around(PX.component_sizes(vol, 1, conn)):
                    good, bad = PX.ref_remove_small(vol, 1, conn, m), PX.ref_remove_small(vol, 1, conn, m, defect)
                    if not (np.array_equal(good[0], bad[0]) and np.array_equal(good[1], bad[1])):
                        caught.add((name, conn))
    print(defect, sorted(caught))
    expect = {"conn26_for_6": ("noise 0.31", 6), "small_le": ("three blobs", 6), "overwrite_other": ("three blobs", 6)}[defect]
    assert expect in caught
    if defect == "conn26_for_6":
        assert all(conn == 6 for _, conn in caught)
    if defect == "overwrite_other":
        assert all(name == "three blobs" for name, _ in caught)


def test_cases_separate_the_modes():
    for shape in PX.BOX_SHAPES:
        D = shape[0]
        chain = PX.diagonal_chain(shape)
        extra = shape == (10, 66, 130)
        assert PX.ref_fill_holes(chain, 1, 6)[1][1] == 2 + 2 * extra and PX.ref_fill_holes(chain, 1, 26)[1][1] == 0 + extra
        ch = PX.z_channel(shape)
        assert PX.ref_fill_holes(ch, 1, 6)[1].tolist() == [1, 0, 0, 0] and PX.ref_fill_holes(ch, 1, 26)[1][1] == 0
        assert PX.ref_fill_holes(ch, 1, 4, True)[1].tolist() == [D, D, 4 * D, 4] and PX.ref_fill_holes(ch, 1, 8, True)[1][1] == D
        box = PX.hollow_box(shape)
        s = PX.cavity_size(shape)
        for conn, per_slice in PX.HOLE_MODES:
            row = PX.ref_fill_holes(box, 1, conn, per_slice)[1]
            assert row[2] == s and row[1] == (D - 4 if per_slice else 1)
        assert PX.ref_fill_holes(box, 1, 6, False, s - 1)[1][1] == 0 and PX.ref_fill_holes(box, 1, 6, False, s)[1][1] == 1
        for f in range(6):
            row = PX.ref_fill_holes(PX.face_cavity(shape, f), 1, 6)[1]
            assert row.tolist() == [2, 1, 1, 1], f
        for a in range(3):
            row = PX.ref_fill_holes(PX.seam_cavity(shape, a), 1, 6)[1]
            assert row.tolist() == ([1, 1, 8, 8] if extra else [1, 0, 0, 0]), a
        other = PX.other_class_in_hole(shape)
        out, row = PX.ref_fill_holes(other, 1, 6)
        assert np.array_equal(out[other == 2], other[other == 2]) and (other == 2).sum() > 0 and row[1] == 2 and row[2] < row[3] + 2
        nested = PX.ref_fill_holes(PX.shell_in_cavity(shape), 1, 6)[1]
        assert nested[1] == 2
        sizes = sorted(PX.component_sizes(PX.three_blobs(shape)))
        assert sizes == [1, 8, 12, 12]
    assert abs(PX.noise((10, 66, 130), 0.69).mean() - 0.69) < 0.01
    assert PX.TILE == (4, 32, 64) and tuple(t + 1 for t in PX.TILE) in PX.SHAPES and tuple(2 * t + 2 for t in PX.TILE) in PX.SHAPES


def test_min_voxels_from_mm3_and_options():
    from rpnet_amd import postprocess as PP
    assert PP.min_voxels_from_mm3(100.0, (2.5, 0.8, 0.8)) == int(np.ceil(np.float64(100.0) / (np.float64(2.5) * 0.8 * 0.8))) == 63
    assert PP.min_voxels_from_mm3(0, (1, 1, 1)) == 1 and PP.min_voxels_from_mm3(8, (1, 1, 1)) == 8 and PP.min_voxels_from_mm3(8.01, (1, 1, 1)) == 9
    assert PP.min_voxels_from_mm3(1e-9, (3.0, 3.0, 3.0)) == 1
    for bad in ((0, 1, 1), (1, -1, 1), (1, 1, float("inf"))):
        with pytest.raises(ValueError, match="spacing"):
            PP.min_voxels_from_mm3(5, bad)
    with pytest.raises(ValueError, match="volume"):
        PP.min_voxels_from_mm3(-1, (1, 1, 1))
    assert [PP.holes_mode_of(v) for v in (False, None, True, "3d", "slice")] == [None, None, False, False, True]
    with pytest.raises(ValueError, match="fill_holes must be"):
        PP.holes_mode_of("2d")
    assert [PP.hole_connectivity_of(*a) for a in ((None, False), (None, True), (26, False), (8, True), (6, True), (26, True))] == [6, 4, 26, 8, 4, 8]
    for bad in ((8, False), (4, False), (18, True), (True, False), (18, False)):
        with pytest.raises(ValueError, match="hole_connectivity must be"):
            PP.hole_connectivity_of(*bad)
    sig = inspect.signature(PP.fill_holes).parameters
    assert list(sig) == ["mask", "classes", "connectivity", "per_slice", "max_hole", "truth", "out", "counts", "stats"]
    assert sig["connectivity"].default == 6 and sig["per_slice"].default is False and sig["max_hole"].default is None
    sig = inspect.signature(PP.remove_small).parameters
    assert list(sig) == ["mask", "classes", "min_voxels", "connectivity", "truth", "out", "counts", "stats"] and sig["connectivity"].default == 6


def test_figures_and_suffixes():
    import torch

    from rpnet_amd import postprocess as PP
    holes = PP.holes_figures(np.array([[[3, 2, 40, 30]], [[1, 0, 0, 0]]]))
    assert holes == [{"n_complement": 3, "n_holes": 2, "filled": 40, "largest": 30}, {"n_complement": 1, "n_holes": 0, "filled": 0, "largest": 0}]
    small = PP.small_figures(np.array([[5, 4, 9, 3]]))
    assert small == [{"n_components": 5, "n_removed": 4, "removed": 9, "largest": 3}]
    assert PP.line_suffix(holes[0], small[0]) == " holes 2 (40 voxels filled) small 4 (9 voxels removed)"
    assert PP.line_suffix(holes=holes[1]) == " holes 0 (0 voxels filled)" and PP.line_suffix(small=small[0]) == " small 4 (9 voxels removed)"
    assert PP.line_suffix() == "" and PP.mean_suffix() == ""
    assert PP.mean_suffix(holes, small) == " holes 1.00 (20.00 voxels filled) small 4.00 (9.00 voxels removed)"
    for fn in (PP.holes_figures, PP.small_figures):
        with pytest.raises(RuntimeError, match="ran out of its bound"):
            fn(np.array([[-1, 0, 0, 0]]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PP.fill_holes(torch.zeros((2, 2, 2), dtype=torch.uint8), (1,))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PP.remove_small(torch.zeros((2, 2, 2), dtype=torch.uint8), (1,), 2)
