"""rpnet_surface_tally (csrc/surface.hip), rpnet_amd.surface, VolumeSegmenter(surface=True) and evaluate_dataset(surface=True) on the
MI355X.

Every comparison is against rpnet_amd.surface.surface_reference (numpy; pinned to scipy.ndimage by tests/test_host_surface.py).  The
int64 row {n_A, n_B, d2_k, d2_k1, d2_max, k} must match EXACTLY.  The two fp64 sums must match to a relative 2 * nbins * 2^-53: a sum
of at most nbins non-negative terms count * sqrt(bin), in any order, lies within nbins * 2^-53 of the exact sum of its terms, and each
term (one correctly rounded square root, one product) within 2 * 2^-53 of its own exact value, which the first bound absorbs for
nbins >= 2; for nbins == 1 the only bin is 0 and the sums are exactly 0."""
import random

import numpy as np
import pytest
import torch

from rpnet_amd import hip
from rpnet_amd import surface as SF
from tests import surface_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL_I, FILL_F = 7, 7.5


def nbins_of(shape):
    return sum((s - 1) ** 2 for s in shape) + 1


def tables(rows=3):
    return (torch.full((rows, SF.IROW), FILL_I, device=DEV, dtype=torch.int64),
            torch.full((rows, SF.FROW), FILL_F, device=DEV, dtype=torch.float64))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def tally(pred, truth, cls=1, row=1, rows=3):
    """one surface_tally into row `row` of fresh, pre-filled tables -> the host tables"""
    it, ft = tables(rows)
    SF.surface_tally(dev(pred), dev(truth), it, row, ft, row, cls=cls)
    torch.cuda.synchronize()
    return it.cpu().numpy(), ft.cpu().numpy()


def check(pred, truth, cls=1, what=""):
    """rpnet_surface_tally (through surface_tally) == surface_reference: the integer row exactly, the sums within the summation bound,
    every other row untouched"""
    irow, frow, fig = SF.surface_reference(pred, truth, cls)
    it, ft = tally(pred, truth, cls)
    tol = 2 * nbins_of(pred.shape) * 2.0 ** -53
    rel = [abs(g - w) / w if w else abs(g) for g, w in zip(ft[1], frow)]
    print(f"{pred.shape} {what}: row {it[1].tolist()} sums {ft[1].tolist()} rel diff {rel} bound {tol:.2e} -> {fig}")
    assert it[1].tolist() == irow.tolist(), what
    assert max(rel) <= tol, what
    assert (it[[0, 2]] == FILL_I).all() and (ft[[0, 2]] == FILL_F).all(), what
    got = SF.surface_from_rows(it[1], ft[1])
    for key, want in fig.items():
        assert (got[key] is None) == (want is None) and (want is None or abs(got[key] - want) <= 2 * tol * want + 0.0), (what, key)
    return it[1], ft[1], got


@pytest.mark.parametrize("shape", SC.SMALL)
def test_tally_equals_the_reference(shape):
    """dilated random masks; identical masks (all distances 0); a single voxel each, far apart; two distant blobs against one (HD95
    below HD); the full volume (the border is the outer shell) against a random mask and against itself"""
    assert hip.query("rpnet_surface_workspace_bytes", *shape) == (2 * nbins_of(shape) + 2) * 8 + 8 * int(np.prod(shape))
    a, b = SC.random_pair(shape)
    irow, _, fig = check(a, b, what="random")
    assert irow[0] > 0 and irow[1] > 0 and fig["hd"] > 0
    irow, frow, fig = check(a, a, what="identical")
    assert irow[2:5].tolist() == [0, 0, 0] and frow.tolist() == [0.0, 0.0] and fig == {"hd95": 0.0, "hd": 0.0, "assd": 0.0}
    irow, _, fig = check(*SC.single_voxels(shape), what="single voxels")
    assert irow.tolist() == [1, 1, nbins_of(shape) - 1, nbins_of(shape) - 1, nbins_of(shape) - 1, 0]
    irow, _, fig = check(*SC.two_blobs(shape), what="two blobs")
    assert fig["hd95"] < fig["hd"]
    full = np.ones(shape, np.uint8)
    irow, _, _ = check(full, b, what="full volume")
    shell = int(np.prod(shape)) - int(np.prod([max(s - 2, 0) for s in shape]))
    assert irow[0] == shell
    check(full, full, what="full against full")


@pytest.mark.parametrize("shape", SC.LONG + SC.LIMIT)
def test_long_lines_and_the_axis_limit(shape):
    """a long line on each axis (300: several tiles of the x pass's 1024 voxels, the narrowest y / z tiles) and the axis limit, 1024,
    on each axis; a single voxel at either end of the long axis puts the largest possible squared distance into the last bin"""
    assert max(shape) in (300, SF.MAX_DIM)
    check(*SC.random_pair(shape), what="random")
    irow, _, _ = check(*SC.single_voxels(shape), what="single voxels")
    assert irow[4] == nbins_of(shape) - 1
    check(*SC.two_blobs(shape), what="two blobs")


@pytest.mark.parametrize("shape", [(1, 16, 16), (9, 33, 20), (2, 3, 300)])
def test_empty_borders_give_the_k_minus_one_row(shape):
    """an empty prediction, an empty truth, both empty: the row {0, 0, 0, 0, 0, -1} and {0.0, 0.0}, no fault, the other rows untouched"""
    a, b = SC.random_pair(shape)
    zero = np.zeros(shape, np.uint8)
    for x, y, what in ((zero, b, "empty prediction"), (a, zero, "empty truth"), (zero, zero, "both empty")):
        irow, frow, fig = check(x, y, what=what)
        assert irow.tolist() == [0, 0, 0, 0, 0, -1] and frow.tolist() == [0.0, 0.0] and fig == {"hd95": None, "hd": None, "assd": None}
    # a class that neither volume holds
    check(a, b, cls=3, what="absent class")


def test_every_element_kind_and_class():
    """cls = 1 and cls = 2 on three-valued masks; every accepted element kind, for either argument, gives the same rows"""
    a, b = SC.three_valued((9, 33, 20))
    rows = {}
    for cls in (1, 2):
        want_i, want_f, _ = check(a, b, cls=cls, what=f"cls {cls}")
        rows[cls] = want_i
        for pk, tk in ((np.uint8, np.int32), (np.int32, np.int64), (np.int64, np.float32), (np.float32, np.uint8), (np.float32, np.float32)):
            it, ft = tally(a.astype(pk), b.astype(tk), cls=cls)
            assert np.array_equal(it[1], want_i) and np.array_equal(ft[1].view(np.int64), want_f.view(np.int64)), (cls, pk, tk)
    assert not np.array_equal(rows[1], rows[2])
    with pytest.raises(ValueError, match="uint8, int32, int64 and float32"):
        SF.surface_tally(dev(a.astype(np.float64)), dev(b), *sum(((t, 0) for t in tables()), ()))
    with pytest.raises(ValueError, match="differ in shape"):
        SF.surface_tally(dev(a[:, :, :10]), dev(b), *sum(((t, 0) for t in tables()), ()))
    with pytest.raises(ValueError, match="contiguous"):
        SF.surface_tally(dev(a)[:, :, ::2], dev(b)[:, :, ::2], *sum(((t, 0) for t in tables()), ()))


def test_runs_are_byte_identical_and_rows_are_kept():
    """the same tally twice into fresh tables is byte-identical; writing row r leaves the rows != r as they were, for every r"""
    a, b = SC.random_pair((17, 40, 36), seed=5)
    first = tally(a, b)
    again = tally(a, b)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    for r in range(3):
        it, ft = tally(a, b, row=r)
        keep = [q for q in range(3) if q != r]
        assert np.array_equal(it[r], first[0][1]) and np.array_equal(ft[r].view(np.int64), first[1][1].view(np.int64))
        assert (it[keep] == FILL_I).all() and (ft[keep] == FILL_F).all()
    # the two tables may use different rows
    it, ft = tables()
    SF.surface_tally(dev(a), dev(b), it, 0, ft, 2)
    torch.cuda.synchronize()
    assert np.array_equal(it[0].cpu().numpy(), first[0][1]) and (it[1:] == FILL_I).all()
    assert np.array_equal(ft[2].cpu().numpy(), first[1][1]) and (ft[:2] == FILL_F).all()


def test_refusals_launch_nothing():
    """a bad row, a too-small workspace, an over-limit dimension, a null pointer and an unknown kind return a status and a message;
    the tables hold what they held"""
    a, b = (dev(x) for x in SC.random_pair((5, 7, 9)))
    it, ft = tables()
    p = hip.ptr
    need = hip.query("rpnet_surface_workspace_bytes", 5, 7, 9)
    ws = torch.empty(need, device=DEV, dtype=torch.uint8)
    for row in (3, -1):
        with pytest.raises(RuntimeError, match=f"rows {row} and 0 of tables of 3 rows"):
            SF.surface_tally(a, b, it, row, ft, 0)
        with pytest.raises(RuntimeError, match=f"rows 0 and {row} of tables of 3 rows"):
            SF.surface_tally(a, b, it, 0, ft, row)

    def raw(pred=p(a), pk=0, truth=p(b), tk=0, dims=(5, 7, 9), itab=p(it), ftab=p(ft), work=p(ws), nbytes=need):
        hip.call("rpnet_surface_tally", pred, pk, truth, tk, 1, *dims, itab, 0, ftab, 0, 3, work, nbytes)
    with pytest.raises(RuntimeError, match=f"workspace of {need - 1} bytes, {need} needed"):
        raw(nbytes=need - 1)
    for dims in ((1025, 1, 1), (5, 1025, 9), (5, 7, 0)):
        with pytest.raises(RuntimeError, match="every extent 1..1024"):
            raw(dims=dims)
        assert hip.query("rpnet_surface_workspace_bytes", *dims) == 0
    for kw in (dict(pred=None), dict(truth=None), dict(itab=None), dict(ftab=None), dict(work=None)):
        with pytest.raises(RuntimeError, match="null pointer"):
            raw(**kw)
    with pytest.raises(RuntimeError, match="element kinds 4, 0"):
        raw(pk=4)
    with pytest.raises(RuntimeError, match="aligned"):
        raw(work=p(ws) + 4, nbytes=need)
    assert hip.load().rpnet_last_error_string().decode().startswith("surface_tally: volumes must be aligned")
    torch.cuda.synchronize()
    assert (it == FILL_I).all() and (ft == FILL_F).all()
    raw()
    torch.cuda.synchronize()
    assert it[0].cpu().numpy().tolist() == SF.surface_reference(a.cpu().numpy(), b.cpu().numpy())[0].tolist()


# ------------------------------------------------------------------------------------------------ end to end
def test_volume_segmenter_surface():
    """a small synthetic episode (the sizes of tests/test_gpu_volume.py), f32 convolutions, eager, one net: res.surface equals
    surface_reference applied to res.mask / the affine baseline and the labels; counts, mask and dice are byte-identical to a
    surface=False run; with surface_out nothing is returned and the caller's tables hold the same rows"""
    import rpnet_amd.functional as RF
    from rpnet_amd.volume import VolumeSegmenter
    from tests.test_gpu_volume import build_net, eval_cfg, reader, segment
    RF.set_conv_math("f32")              # restored by tests/conftest.py
    cfg = eval_cfg()
    item = reader(cfg, 6, 64)[0]
    net = build_net(cfg)
    plain = segment(VolumeSegmenter(net, batch=4, graphed=False), item)
    res = segment(VolumeSegmenter(net, batch=4, graphed=False, surface=True), item)
    assert plain.surface is None
    assert torch.equal(res.mask, plain.mask) and res.counts.tobytes() == plain.counts.tobytes() and res.dice == plain.dice
    labels, mask = item["query_labels"].numpy(), res.mask.cpu().numpy()
    appr = item["appr_query_labels"].numpy()
    want = {"fewshot": SF.surface_reference(mask, labels), "affine": SF.surface_reference(appr, labels)}
    print("surface", res.surface, "\nreference", {k: v[2] for k, v in want.items()})
    assert want["affine"][2]["hd95"] is not None, "the synthetic episode has an organ and a baseline"
    assert sorted(res.surface) == ["affine", "fewshot"]
    tol = 2 * nbins_of(mask.shape) * 2.0 ** -53
    for key, (irow, frow, fig) in want.items():
        (got,) = res.surface[key]
        for name, w in fig.items():
            assert (got[name] is None) == (w is None) and (w is None or abs(got[name] - w) <= 2 * tol * w), (key, name)
    # the caller's tables: exact rows, nothing returned
    it = torch.full((2, 1, SF.IROW), FILL_I, device=DEV, dtype=torch.int64)
    ft = torch.full((2, 1, SF.FROW), FILL_F, device=DEV, dtype=torch.float64)
    seg = VolumeSegmenter(net, batch=4, graphed=False, surface=True)
    out = seg(item["support_images"], item["support_labels"], item["query_images"], item["appr_query_labels"], item["query_labels"],
              surface_out=(it, ft))
    assert out.surface is None and torch.equal(out.mask, plain.mask) and np.array_equal(out.counts, plain.counts)
    for s, key in enumerate(("fewshot", "affine")):
        assert it[s, 0].cpu().numpy().tolist() == want[key][0].tolist(), key
        assert np.abs(ft[s, 0].cpu().numpy() - want[key][1]).max() <= tol * want[key][1].max(), key
    # without labels there is nothing to measure against: the flag is ignored
    bare = seg(item["support_images"], item["support_labels"], item["query_images"], item["appr_query_labels"])
    assert bare.surface is None and bare.counts is None and torch.equal(bare.mask, plain.mask)


def test_evaluate_dataset_surface(tmp_path, capsys):
    """the small synthetic NRRD set of tests/test_gpu_dataset_eval.py, f32 convolutions, eager: the three returned dictionaries and the
    tally tables equal those of the surface=False run; every printed line is the surface=False line plus exactly the documented suffix;
    out["surface_i"] / out["surface_f"] match surface_reference per item (the masks come back through save_pred)"""
    import os

    from rpnet_amd import dataset_eval as DE
    from rpnet_amd.utils import nrrd
    from tests.test_gpu_dataset_eval import _build_net, _dataset, _driver_lines, _eval_cfg, _plain
    data_dir, set_name, cfg = _dataset(tmp_path / "data", do_deformable=False)
    cfg = _eval_cfg(cfg)
    src = DE.DeviceEvalSource(data_dir, set_name, cfg, DEV)
    src.warm()
    pred_dir = str(tmp_path / "pred")
    random.seed(77)
    capsys.readouterr()
    t0, t1 = {}, {}
    want = _plain(DE.evaluate_dataset(_build_net(cfg, "f32"), src, cfg, batch=8, graphed=False, out=t0))
    lines0 = _driver_lines(capsys.readouterr().out)
    random.seed(77)
    got = _plain(DE.evaluate_dataset(_build_net(cfg, "f32"), src, cfg, batch=8, graphed=False, out=t1, surface=True, save_pred=pred_dir))
    lines1 = _driver_lines(capsys.readouterr().out)
    assert got == want
    assert sorted(t0) == ["counts", "ncc"] and sorted(t1) == ["counts", "ncc", "surface_f", "surface_i"]
    assert np.array_equal(t0["counts"], t1["counts"]) and t0["ncc"].tobytes() == t1["ncc"].tobytes()
    si, sf = t1["surface_i"], t1["surface_f"]
    assert si.shape == (3, 2, 1, SF.IROW) and si.dtype == np.int64 and sf.shape == (3, 2, 1, SF.FROW) and sf.dtype == np.float64
    assert len(lines0) == len(lines1) == 4
    few, aff = [], []
    random.seed(77)
    for j in range(3):
        s = src.item(j)
        labels, appr = s["query_labels"].cpu().numpy(), s["appr_query_labels"].cpu().numpy()
        mask, _ = nrrd.read(os.path.join(pred_dir, f"{s['pid']}_Liver.nrrd"))
        tol = 2 * nbins_of(mask.shape) * 2.0 ** -53
        for r, pred in enumerate((mask, appr)):
            irow, frow, _ = SF.surface_reference(pred, labels)
            assert si[j, r, 0].tolist() == irow.tolist(), (j, r)
            assert np.abs(sf[j, r, 0] - frow).max() <= tol * frow.max(), (j, r)
        f, a = SF.surface_figures(si[j, :, 0], sf[j, :, 0])
        few.append(f)
        aff.append(a)
        suffix = f" hd95 {SF.fmt(f['hd95'])} ({SF.fmt(a['hd95'])}) assd {SF.fmt(f['assd'])} ({SF.fmt(a['assd'])})"
        assert lines1[j] == lines0[j] + suffix, (lines0[j], lines1[j])
    assert any(a["hd95"] is not None for a in aff)
    assert lines1[3] == lines0[3] + SF.mean_suffix(few, aff) and " hd95 " in lines1[3] and " assd " in lines1[3]
