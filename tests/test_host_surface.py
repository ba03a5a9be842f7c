"""Host side of the surface distances (rpnet_amd/surface.py): the numpy restatement `surface_reference`, which is the yardstick of
tests/test_gpu_surface.py, against scipy.ndimage and numpy's own percentile / mean / max; rows -> figures; the loud failures off the GPU
and the refusals of the new arguments."""
import numpy as np
import pytest
import torch

from rpnet_amd import hip
from rpnet_amd import surface as SF
from tests import surface_cases as SC


def _ulps(got, want):
    return abs(got - want) / np.spacing(abs(want)) if want else abs(got)


@pytest.mark.parametrize("shape", SC.SMALL)
def test_reference_equals_scipy(shape):
    """borders equal to M & ~binary_erosion(M, generate_binary_structure(3, 1)) exactly; the square roots of the integer transform
    equal to distance_transform_edt exactly; HD95 / ASSD / HD within 4 ulp of np.percentile / mean / max over scipy's distances"""
    ndi = pytest.importorskip("scipy.ndimage")
    pairs = [SC.random_pair(shape), SC.two_blobs(shape), SC.single_voxels(shape), (np.ones(shape, np.uint8), SC.random_pair(shape, 3)[1])]
    for a, b in pairs:
        borders = []
        for m in (a.astype(bool), b.astype(bool)):
            want = m & ~ndi.binary_erosion(m, ndi.generate_binary_structure(3, 1))
            got = SF.border_reference(m)
            assert np.array_equal(got, want)
            d2 = SF.transform_reference(got)
            assert d2.dtype == np.int64 and d2.max() < SF.NO_SEED
            assert np.array_equal(np.sqrt(d2.astype(np.float64)), ndi.distance_transform_edt(~want))
            borders.append(want)
        ba, bb = borders
        d_ab, d_ba = ndi.distance_transform_edt(~bb)[ba], ndi.distance_transform_edt(~ba)[bb]
        pooled = np.hstack([d_ab, d_ba])
        want = {"hd95": float(np.percentile(pooled, 95)), "hd": float(pooled.max()), "assd": float((d_ab.mean() + d_ba.mean()) / 2)}
        irow, frow, got = SF.surface_reference(a, b)
        assert irow.dtype == np.int64 and irow.shape == (6,) and frow.dtype == np.float64 and frow.shape == (2,)
        assert irow[0] == ba.sum() and irow[1] == bb.sum() and irow[5] == int(np.floor(0.95 * (len(pooled) - 1)))
        worst = {k: _ulps(got[k], want[k]) for k in want}
        print(shape, got, "ulps", worst)
        assert max(worst.values()) <= 4
        assert got["hd95"] <= got["hd"]


def test_reference_details():
    """D == 1: every foreground voxel is a border voxel; a full volume's border is its outer shell; an all-background border
    transforms to NO_SEED everywhere; cls selects the value; an empty side gives the k = -1 row and three Nones"""
    m = np.zeros((1, 6, 6), bool)
    m[0, 1:5, 1:5] = True
    assert np.array_equal(SF.border_reference(m), m)
    full = np.ones((5, 6, 7), bool)
    shell = full.copy()
    shell[1:-1, 1:-1, 1:-1] = False
    assert np.array_equal(SF.border_reference(full), shell)
    assert (SF.transform_reference(np.zeros((3, 4, 5), bool)) == SF.NO_SEED).all()
    a, b = SC.three_valued((5, 7, 9))
    for cls in (1, 2):
        irow, frow, fig = SF.surface_reference(a, b, cls=cls)
        i2, f2, fig2 = SF.surface_reference((a == cls).astype(np.float32), (b == cls).astype(np.int64))
        assert np.array_equal(irow, i2) and np.array_equal(frow, f2) and fig == fig2
    assert not np.array_equal(SF.surface_reference(a, b, 1)[0], SF.surface_reference(a, b, 2)[0])
    zero = np.zeros_like(a)
    for x, y in ((zero, b), (a, zero), (zero, zero)):
        irow, frow, fig = SF.surface_reference(x, y)
        assert irow.tolist() == [0, 0, 0, 0, 0, -1] and frow.tolist() == [0.0, 0.0]
        assert fig == {"hd95": None, "hd": None, "assd": None}
    # identical masks: every distance is 0
    irow, frow, fig = SF.surface_reference(a, a)
    assert irow[2:5].tolist() == [0, 0, 0] and fig == {"hd95": 0.0, "hd": 0.0, "assd": 0.0}


def test_surface_from_rows():
    irow, frow = np.array([3, 1, 4, 9, 25, 2], np.int64), np.array([6.0, 5.0])
    fig = SF.surface_from_rows(irow, frow)
    gamma = 3 * 0.95 - 2
    assert fig["hd"] == 5.0 and fig["assd"] == (6.0 / 3 + 5.0 / 1) / 2
    assert fig["hd95"] == 3.0 - (3.0 - 2.0) * (1 - gamma)          # numpy's _lerp at gamma >= 0.5
    for s in (0.5, 2.0, 3):
        scaled = SF.surface_from_rows(irow, frow, spacing=s)
        assert scaled == {k: v * s for k, v in fig.items()}
    assert SF.surface_from_rows([0, 0, 0, 0, 0, -1], [0.0, 0.0]) == {"hd95": None, "hd": None, "assd": None}
    assert SF.surface_from_rows(torch.tensor([0, 0, 0, 0, 0, -1]), torch.zeros(2, dtype=torch.float64), 2.0)["hd"] is None
    for bad in ((1.0, 1.0, 2.5), [1.0, 1.0, 1.0], np.ones(3)):
        with pytest.raises(ValueError, match="one isotropic factor.*integer.*_clean.nrrd"):
            SF.surface_from_rows(irow, frow, spacing=bad)
    few, aff = SF.surface_figures(np.stack([irow, [0, 0, 0, 0, 0, -1]]), np.stack([frow, [0.0, 0.0]]))
    assert few == fig and aff["hd95"] is None
    assert SF.line_suffix(few, aff) == f" hd95 {fig['hd95']:.4f} (None) assd 3.5000 (None)"
    assert SF.mean_suffix([few, aff, few], [aff, aff]) == f" hd95 {fig['hd95']:.4f} (None) assd 3.5000 (None)"


def test_surface_tally_argument_checks_off_the_gpu():
    """host tensors are refused loudly (there is no CPU fallback); the workspace query needs no GPU"""
    m = torch.zeros(2, 4, 4, dtype=torch.uint8)
    it, ft = torch.zeros(1, 6, dtype=torch.int64), torch.zeros(1, 2, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SF.surface_tally(m, m, it, 0, ft, 0)
    for bad_i, bad_f in ((it.int(), ft), (it, ft.float()), (torch.zeros(1, 5, dtype=torch.int64), ft), (it, torch.zeros(2, 2, dtype=torch.float64)),
                         (torch.zeros(1, 12, dtype=torch.int64)[:, ::2], ft)):
        with pytest.raises(ValueError, match="table"):
            SF.check_surface_tables(bad_i, bad_f)
    q = hip.load().rpnet_surface_workspace_bytes
    nbins = 63 ** 2 + 2 * 255 ** 2 + 1
    assert q(64, 256, 256) == (2 * nbins + 2) * 8 + 2 * 4 * 64 * 256 * 256
    assert q(1, 1, 1) == 32 + 8 and q(1024, 1024, 1024) > 2 ** 33
    for bad in ((0, 4, 4), (4, 1025, 4), (4, 4, -1)):
        assert q(*bad) == 0
        assert hip.load().rpnet_last_error_string().decode().startswith("surface: D=")
    assert SF.MAX_DIM == 1024 and SF.KINDS == {torch.uint8: 0, torch.int32: 1, torch.int64: 2, torch.float32: 3}


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.num_iter = 3

    def forward(self, *a, **kw):
        raise AssertionError("the model must not be called when an argument is refused")


def test_new_arguments_are_refused_as_documented():
    from rpnet_amd.volume import VolumeResult, VolumeSegmenter, check_surface_out
    from tools.eval_driver import evaluate_on_device
    good = (torch.zeros(2, 1, 6, dtype=torch.int64), torch.zeros(2, 1, 2, dtype=torch.float64))
    check_surface_out(good, K=2)
    for bad in (good[0], (good[0], good[1].float()), (good[0][:1], good[1]), (torch.zeros(2, 2, 6, dtype=torch.int64), good[1]),
                (good[0].numpy(), good[1].numpy()), (good[1], good[0])):
        with pytest.raises(ValueError, match="surface_out"):
            check_surface_out(bad, K=2)
    si, fg, qi, appr, ql = [[torch.zeros(2, 1, 16, 16)]], [[torch.zeros(2, 16, 16)]], torch.zeros(2, 1, 16, 16), torch.zeros(2, 16, 16), torch.zeros(2, 16, 16)
    with pytest.raises(ValueError, match=r"surface_out needs VolumeSegmenter\(surface=True\)"):
        VolumeSegmenter(_Net(), batch=2, graphed=False)(si, fg, qi, appr, ql, surface_out=good)
    seg = VolumeSegmenter(_Net(), batch=2, graphed=False, surface=True)
    assert seg.surface and not VolumeSegmenter(_Net(), batch=2, graphed=False).surface
    with pytest.raises(ValueError, match="surface_out needs query_labels"):
        seg(si, fg, qi, appr, None, surface_out=good)
    with pytest.raises(ValueError, match="surface_out must be a pair"):
        seg(si, fg, qi, appr, ql, surface_out=(good[0], good[0]))
    with pytest.raises(ValueError, match=r"needs a VolumeSegmenter\(surface=True\)"):
        evaluate_on_device(_Net(), [], {"eval_classes": ["Liver"]}, segmenter=VolumeSegmenter(_Net(), graphed=False), surface=True)
    # the result type keeps its three fields; `surface` rides beside them and defaults to None
    res = VolumeResult(1, 2, 3)
    assert res.surface is None and tuple(res) == (1, 2, 3)
    res.surface = {"fewshot": []}
    assert VolumeResult(1, 2, 3).surface is None and res.surface == {"fewshot": []}
