"""The numpy restatement of the connected-component contract (tests/components_cases.py) against scipy.ndimage, the tie rule against
its argmax(bincount) formulation, seeded defects against the comparison the GPU tests use, and the host-side pieces of the feature:
the driver's flag, the defaults of the signatures, VolumeResult.post.  Runs without a GPU."""
import inspect

import numpy as np
import pytest
from scipy import ndimage

from tests import components_cases as CX



def _cases():
    for shape in CX.SHAPES:
        for name, vol in CX.contents(shape):
            yield shape, name, vol
        yield shape, "three classes", CX.three_classes(shape)


@pytest.mark.parametrize("conn,rank", [(6, 1), (26, 3)])
def test_ref_label_is_scipy_label_under_relabelling(conn, rank):
    """on every case of the table: the same partition as scipy.ndimage.label with generate_binary_structure(3, rank) (a bijection
    between the two label sets, background to background), and every label is 1 + the smallest linear index that holds it"""
    structure = ndimage.generate_binary_structure(3, rank)
    for shape, name, vol in _cases():
        for cls in (1, 2) if name == "three classes" else (1,):
            lab, n = ndimage.label(vol == cls, structure=structure)
            ref = CX.ref_label(vol, cls, conn)
            assert ref.dtype == np.int32 and ref.shape == vol.shape
            pairs = np.unique(np.stack([lab.ravel(), ref.ravel()]), axis=1)
            assert pairs.shape[1] == len(np.unique(lab)) == len(np.unique(ref)), (shape, name)
            assert ((pairs[0] == 0) == (pairs[1] == 0)).all()
            values, first = np.unique(ref.ravel(), return_index=True)
            assert all(v == f + 1 for v, f in zip(values, first) if v), (shape, name)
            assert CX.ref_stats(vol, cls, conn)[1] == n


def test_tie_rule_is_argmax_of_bincount():
    """the chosen component is the one np.argmax(np.bincount(lab.ravel())[1:]) names on scipy's labels, whose numbers grow with the
    first voxel in z-major order; the filter keeps exactly its voxels"""
    for shape, name, vol in _cases():
        for conn, rank in ((6, 1), (26, 3)):
            lab, n = ndimage.label(vol == 1, structure=ndimage.generate_binary_structure(3, rank))
            row = CX.ref_stats(vol, 1, conn)
            kept = CX.ref_keep_largest(vol, 1, conn)
            if n == 0:
                assert row.tolist() == [0, 0, 0, -1] and not (kept == 1).any()
                continue
            firsts = ndimage.minimum(np.arange(lab.size).reshape(lab.shape), lab, index=np.arange(1, n + 1))
            assert (np.diff(firsts) > 0).all(), "scipy numbers the components by their first voxel"
            best = 1 + int(np.argmax(np.bincount(lab.ravel())[1:]))
            assert row.tolist() == [(vol == 1).sum(), n, (lab == best).sum(), firsts[best - 1]], (shape, name, conn)
            assert np.array_equal(kept == 1, lab == best) and np.array_equal(kept[vol != 1], vol[vol != 1])
    tie = CX.two_blobs((10, 66, 130))
    assert CX.ref_stats(tie)[3] == 0 and CX.ref_stats(CX.two_blobs((10, 66, 130), later_larger=True))[3] > 0


@pytest.mark.parametrize("defect", CX.DEFECTS)
def test_seeded_defects_fail_the_comparison(defect):
    """each defect, applied to a copy of the restatement, is caught by the exact comparison of labels, filtered mask or statistics row
    on at least one case of the table at the 2 * tile + 2 extent"""
    shape = (10, 66, 130)
    caught = []
    cases = list(CX.contents(shape)) + [("three classes", CX.three_classes(shape))]
    for name, vol in cases:
        for conn in (6, 26):
            same = (np.array_equal(CX.ref_label(vol, 1, conn), CX.ref_label(vol, 1, conn, defect))
                    and np.array_equal(CX.ref_keep_largest(vol, 1, conn), CX.ref_keep_largest(vol, 1, conn, defect))
                    and np.array_equal(CX.ref_stats(vol, 1, conn), CX.ref_stats(vol, 1, conn, defect)))
            if not same:
                caught.append((name, conn))
    print(defect, caught)
    assert caught
    expect = {"no_z_seam": ("full", 6), "no_diagonal_26": ("corner", 26), "tie_last": ("equal blobs", 6), "off_by_one": ("full", 6),
              "zero_other_classes": ("three classes", 6)}[defect]
    assert expect in caught
    if defect == "no_diagonal_26":
        assert all(conn == 26 for _, conn in caught)
    if defect == "zero_other_classes":
        assert all(name == "three classes" for name, _ in caught)


def test_cases_are_what_they_say():
    shape = (10, 66, 130)
    n = int(np.prod(shape))
    assert CX.ref_stats(CX.checkerboard(shape), 1, 6).tolist() == [n // 2, n // 2, 1, 0]
    assert CX.ref_stats(CX.checkerboard(shape), 1, 26)[1] == 1
    s = CX.serpentine(shape)
    assert CX.ref_stats(s, 1, 6)[1] == 1 and ndimage.maximum_filter(s.astype(np.int32), size=2).sum() > 0
    # one voxel wide: no 2 x 2 block of the path in any plane
    assert not (s[:, :-1, :-1] & s[:, 1:, :-1] & s[:, :-1, 1:] & s[:, 1:, 1:]).any()
    u = CX.u_shape(shape)
    assert CX.ref_stats(u, 1, 6)[1] == 1 and CX.ref_stats(u[:, :, :-1], 1, 26)[1] == 2          # the arms join only at x = W - 1
    for corner in (False, True):
        t = CX.touching(shape, corner)
        assert CX.ref_stats(t, 1, 6)[1] == 2 and CX.ref_stats(t, 1, 26)[1] == 1
    assert all(abs(CX.noise(shape, d).mean() - d) < 0.01 for d in CX.DENSITIES)
    assert CX.TILE == (4, 32, 64) and tuple(t + 1 for t in CX.TILE) in CX.SHAPES and tuple(2 * t + 2 for t in CX.TILE) in CX.SHAPES


def test_driver_flag_signatures_and_defaults():
    from rpnet_amd import components as CC
    from rpnet_amd.dataset_eval import evaluate_dataset
    from rpnet_amd.volume import VolumeResult, VolumeSegmenter
    from tools.eval_driver import build_parser, evaluate_on_device
    ap = build_parser()
    assert ap.parse_args([]).keep_largest == 0
    assert ap.parse_args(["--keep-largest"]).keep_largest == 6
    assert ap.parse_args(["--keep-largest", "26", "--surface", "--device-items"]).keep_largest == 26
    assert ap.parse_args(["--keep-largest", "--surface"]).surface is True
    with pytest.raises(SystemExit):
        ap.parse_args(["--keep-largest", "18"])
    assert VolumeResult._fields == ("mask", "counts", "dice") and VolumeResult.post is None and VolumeResult.surface is None
    assert VolumeResult(1, 2, 3).post is None
    for fn in (VolumeSegmenter.__init__, evaluate_dataset, evaluate_on_device):
        assert inspect.signature(fn).parameters["keep_largest"].default is False
    assert inspect.signature(VolumeSegmenter.__call__).parameters["post_out"].default is None
    sig = inspect.signature(CC.keep_largest).parameters
    assert sig["classes"].default == (1,) and sig["connectivity"].default == 6 and all(sig[k].default is None for k in ("truth", "out", "counts", "stats"))
    sig = inspect.signature(CC.label_components).parameters
    assert sig["cls"].default == 1 and sig["connectivity"].default == 6 and sig["row"].default == 0
    assert [CC.connectivity_of(v) for v in (False, True, 6, 26)] == [0, 6, 6, 26]
    for bad in (18, 1, "6", 0):
        with pytest.raises(ValueError, match="keep_largest must be"):
            CC.connectivity_of(bad)


def test_figures_and_suffixes():
    import torch

    from rpnet_amd import components as CC
    figs = CC.components_figures(np.array([[[120, 3, 100, 7]], [[0, 0, 0, -1]]]))
    assert figs == [{"n_components": 3, "kept": 100, "removed": 20}, {"n_components": 0, "kept": 0, "removed": 0}]
    assert CC.line_suffix(0.9, figs[0]) == " lcc 0.9 (3 components, 20 voxels removed)"
    assert CC.line_suffix(None, figs[1], {"hd95": 1.5, "hd": 2.0, "assd": None}) == " lcc None (0 components, 0 voxels removed) lcc hd95 1.5000 assd None"
    assert CC.mean_suffix([0.9, None], figs) == " lcc 0.9000 (1.50 components, 10.00 voxels removed)"
    assert CC.mean_suffix([0.5], figs[:1], [{"hd95": 2.0, "assd": 1.0}]).endswith(" lcc hd95 2.0000 assd 1.0000")
    with pytest.raises(RuntimeError, match="ran out of its bound"):
        CC.components_figures(np.array([[5, -1, 0, -1]]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CC.label_components(torch.zeros((2, 2, 2), dtype=torch.uint8))
