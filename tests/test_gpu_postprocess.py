"""rpnet_ccpost_fill_holes and rpnet_ccpost_remove_small (csrc/cc_post.hip), rpnet_amd.postprocess and the clean-up chain of
VolumeSegmenter on the MI355X.

Every comparison is exact integer equality with tests/postprocess_cases.py:ref_fill_holes / ref_remove_small (numpy; pinned to
scipy.ndimage by tests/test_host_postprocess.py): results, statistics rows and counts rows.  There is no tolerance.  After every call the
`overrun` word of the workspace must be 0."""
import numpy as np
import pytest
import torch

from rpnet_amd import hip
from rpnet_amd import postprocess as PP
from tests import components_cases as CX
from tests import postprocess_cases as PX

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 7


def dev(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(DEV)


def table(rows, cols):
    return torch.full((rows, cols), FILL, device=DEV, dtype=torch.int64)


def check(kind, vol, what, truth=None, in_place=False, cls=1, **kw):
    """fill_holes (kind 'holes': connectivity, per_slice, max_hole) or remove_small (kind 'small': connectivity, min_voxels) of one class
    == the restatement: the result, the statistics row and the counts row (added to FILL); the input untouched out of place; no overrun"""
    src = dev(vol)
    out = src if in_place else torch.full(vol.shape, FILL, device=DEV, dtype=torch.uint8)
    counts = None if truth is None else table(1, PP.COUNTS_ROW)
    stats = table(1, PP.STATS_ROW)
    tr = None if truth is None else dev(truth)
    if kind == "holes":
        got = PP.fill_holes(src, (cls,), truth=tr, out=out, counts=counts, stats=stats, **kw)
        want, row = PX.ref_fill_holes(vol, cls, kw["connectivity"], kw.get("per_slice", False), kw.get("max_hole"))
    else:
        got = PP.remove_small(src, (cls,), truth=tr, out=out, counts=counts, stats=stats, **kw)
        want, row = PX.ref_remove_small(vol, cls, kw["connectivity"], kw["min_voxels"])
    torch.cuda.synchronize()
    assert PP.post_overrun(DEV, vol.shape) == 0, what
    assert got[0] is out and got[1] is counts and got[2] is stats
    assert np.array_equal(out.cpu().numpy(), want), what
    if not in_place:
        assert np.array_equal(src.cpu().numpy(), vol), what
    assert stats.cpu().numpy()[0].tolist() == row.tolist(), what
    if truth is not None:
        assert (counts.cpu().numpy()[0] - FILL).tolist() == PX.ref_counts(want, truth, cls).tolist(), what
    return out, row


def hole_bounds(name, vol, conn, per_slice):
    """None (no bound) and, for the contents with holes of known sizes, one below, at and one above those sizes"""
    if name in ("hollow box", "shell in cavity", "other class in hole", "noise 0.69"):
        return [None] + PX.bounds_around(PX.hole_sizes(vol, 1, conn, per_slice))
    return [None]


@pytest.mark.parametrize("shape", PX.SHAPES)
def test_fill_holes_equals_the_restatement(shape):
    """every content of the table at every extent under the four modes, max_hole one below, at and one above the sizes of the holes:
    alternately out of place without a truth and in place with one"""
    assert hip.query("rpnet_ccpost_workspace_bytes", *shape) == 64 + 2 * ((4 * int(np.prod(shape)) + 15) // 16 * 16)
    truth = CX.noise(shape, 0.5, seed=9)
    k, rows = 0, {}
    for name, vol in PX.hole_contents(shape):
        for conn, per_slice in PX.HOLE_MODES:
            for b in hole_bounds(name, vol, conn, per_slice):
                k += 1
                _, row = check("holes", vol, f"{shape} {name} {conn} {per_slice} {b}", truth=truth if k % 2 else None, in_place=bool(k % 2),
                               connectivity=conn, per_slice=per_slice, max_hole=b)
                rows[(name, conn, per_slice, b)] = row.tolist()
    if shape in PX.BOX_SHAPES:
        D, s = shape[0], PX.cavity_size(shape)
        assert rows[("hollow box", 6, False, None)][1:] == [1, s, s] and rows[("hollow box", 6, False, s - 1)][1:] == [0, 0, 0]
        assert rows[("hollow box", 6, False, s)][1:] == [1, s, s] and rows[("hollow box", 4, True, None)][1] == D - 4
        assert rows[("z channel", 6, False, None)] == [1, 0, 0, 0] and rows[("z channel", 4, True, None)] == [D, D, 4 * D, 4]
        assert rows[("diagonal chain", 6, False, None)][1] >= 2 and rows[("diagonal chain", 26, False, None)][1] <= 1
        assert all(rows[(f"face {f}", 6, False, None)] == [2, 1, 1, 1] for f in range(6))
        assert rows[("full", 6, False, None)] == [0, 0, 0, 0] and rows[("empty", 26, False, None)] == [1, 0, 0, 0]


@pytest.mark.parametrize("shape", PX.SHAPES)
def test_remove_small_equals_the_restatement(shape):
    """every content of the table at every extent and both connectivities, min_voxels one below, at and one above the smallest, the
    largest and (for the blobs) every size, ties included: alternately out of place without a truth and in place with one"""
    truth = CX.noise(shape, 0.5, seed=9)
    k, rows = 0, {}
    for name, vol in PX.small_contents(shape):
        for conn in (6, 26):
            for m in PX.bounds_around(PX.component_sizes(vol, 1, conn), most=4):
                k += 1
                _, row = check("small", vol, f"{shape} {name} {conn} {m}", truth=truth if k % 2 else None, in_place=bool(k % 2),
                               connectivity=conn, min_voxels=m)
                rows[(name, conn, m)] = row.tolist()
    if shape in PX.BOX_SHAPES:
        assert rows[("three blobs", 6, 12)] == [4, 2, 9, 8] and rows[("three blobs", 6, 13)] == [4, 4, 33, 12]          # the tie goes together
        assert rows[("three blobs", 6, 8)] == [4, 1, 1, 1] and rows[("three blobs", 6, 1)] == [4, 0, 0, 0]
    n = int(np.prod(shape))
    assert rows[("full", 6, n)] == [1, 0, 0, 0] and rows[("full", 6, n + 1)] == [1, 1, n, n]


def test_every_element_kind_and_three_classes():
    """a three-class volume: every accepted element kind of the input and of the truth gives the restatement's result and rows; the
    other classes pass through untouched; several classes in one call equal the restatement applied class by class; counts are added"""
    shape = (5, 33, 65)
    vol, truth = CX.three_classes(shape), CX.three_classes(shape, seed=4)
    dense = np.where(CX.noise(shape, 0.8, seed=2) == 1, np.uint8(2), CX.three_classes(shape, seed=5))      # class 2 with holes in it
    for cls in (1, 2, 3):
        for kind, tk in ((np.uint8, np.int32), (np.int32, np.int64), (np.int64, np.float32), (np.float32, np.uint8)):
            out, _ = check("small", vol.astype(kind), f"small {cls} {kind}", truth=truth.astype(tk), cls=cls, connectivity=26, min_voxels=3)
            assert out.dtype == torch.uint8
    for kind, tk in ((np.uint8, np.int32), (np.int32, np.int64), (np.int64, np.float32), (np.float32, np.uint8)):
        for conn, per_slice in PX.HOLE_MODES:
            _, row = check("holes", dense.astype(kind), f"holes {kind} {conn}", truth=truth.astype(tk), cls=2, connectivity=conn, per_slice=per_slice)
        assert row[1] > 0 and row[2] > 0
    want, rows = vol, []
    for cls in (1, 2, 3):
        want, row = PX.ref_remove_small(want, cls, 6, 4)
        rows.append(row.tolist())
    counts = torch.full((3, PP.COUNTS_ROW), 5, device=DEV, dtype=torch.int64)
    out, counts, stats = PP.remove_small(dev(vol), (1, 2, 3), 4, truth=dev(truth), counts=counts)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want) and stats.cpu().numpy().tolist() == rows
    assert (counts.cpu().numpy() - 5).tolist() == [PX.ref_counts(want, truth, c).tolist() for c in (1, 2, 3)]
    want, rows = dense, []
    for cls in (2, 1):
        want, row = PX.ref_fill_holes(want, cls, 6)
        rows.append(row.tolist())
    out, counts, stats = PP.fill_holes(dev(dense), (2, 1))
    torch.cuda.synchronize()
    assert counts is None and np.array_equal(out.cpu().numpy(), want) and stats.cpu().numpy().tolist() == rows
    # per slice, 6 / 26 stand for 4 / 8
    out, _, stats = PP.fill_holes(dev(dense), (2,), connectivity=26, per_slice=True)
    assert np.array_equal(out.cpu().numpy(), PX.ref_fill_holes(dense, 2, 8, True)[0])
    with pytest.raises(ValueError, match="uint8, int32, int64 and float32"):
        PP.fill_holes(dev(vol.astype(np.float64)), (1,))
    with pytest.raises(ValueError, match="contiguous"):
        PP.remove_small(dev(vol)[:, :, ::2], (1,), 2)
    with pytest.raises(ValueError, match="counts need a truth"):
        PP.fill_holes(dev(vol), (1,), counts=table(1, 3))
    with pytest.raises(ValueError, match="max_hole must be"):
        PP.fill_holes(dev(vol), (1,), max_hole=0)


def test_graph_replay_and_guard_words():
    """both calls through the C ABI with a workspace of exactly the size asked for, guard bytes behind it: captured with
    torch.cuda.graph and replayed twice they give identical bits, equal to an eager call and to the restatement; the guard bytes and
    the other rows of the tables hold what they held; the overrun word is 0"""
    shape = (10, 66, 130)
    vol, truth = CX.noise(shape, 0.69), CX.noise(shape, 0.5, seed=9)
    src, tr = dev(vol), dev(truth)
    need = hip.query("rpnet_ccpost_workspace_bytes", *shape)
    ws = torch.full((need + 64,), 0xA5, device=DEV, dtype=torch.uint8)
    outs = [torch.empty(shape, device=DEV, dtype=torch.uint8) for _ in range(2)]
    stats, counts = table(3, PP.STATS_ROW), table(3, PP.COUNTS_ROW)
    p = hip.ptr

    def both():
        hip.call("rpnet_ccpost_fill_holes", p(src), 0, p(outs[0]), 1, *shape, 26, 0, 0, p(tr), 0, p(counts), 0, p(stats), 0, 3, p(ws), need)
        hip.call("rpnet_ccpost_remove_small", p(src), 0, p(outs[1]), 1, *shape, 6, 3, p(tr), 0, p(counts), 2, p(stats), 2, 3, p(ws), need)

    def snapshot():
        torch.cuda.synchronize()
        assert int(ws[PP.OVERRUN_OFFSET:PP.OVERRUN_OFFSET + 4].view(torch.int32).item()) == 0 and (ws[need:] == 0xA5).all()
        return [t.cpu().numpy().copy() for t in (*outs, stats, counts)]

    both()
    eager = snapshot()
    want_h, row_h = PX.ref_fill_holes(vol, 1, 26)
    want_s, row_s = PX.ref_remove_small(vol, 1, 6, 3)
    assert np.array_equal(eager[0], want_h) and np.array_equal(eager[1], want_s) and row_h[1] > 0 and row_s[1] > 0
    assert eager[2].tolist() == [row_h.tolist(), [FILL] * 4, row_s.tolist()]
    assert (eager[3] - FILL).tolist() == [PX.ref_counts(want_h, truth).tolist(), [0] * 3, PX.ref_counts(want_s, truth).tolist()]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    runs = []
    for _ in range(2):
        for t in (*outs, stats, counts):
            t.fill_(FILL)
        graph.replay()
        runs.append(snapshot())
    for a, b, c in zip(eager, runs[0], runs[1]):
        assert a.tobytes() == b.tobytes() == c.tobytes()


def test_refusals_launch_nothing():
    """every refusal of include/rpnet_ccpost_abi.h returns its status with a message; the output and the tables hold what they held"""
    shape = (5, 7, 9)
    host = CX.noise(shape, 0.6)
    vol = dev(host)
    vol32 = vol.to(torch.int32)
    out = torch.full(shape, FILL, device=DEV, dtype=torch.uint8)
    stats, counts = table(3, PP.STATS_ROW), table(3, PP.COUNTS_ROW)
    p = hip.ptr
    need = hip.query("rpnet_ccpost_workspace_bytes", *shape)
    ws = torch.empty(need + 16, device=DEV, dtype=torch.uint8)

    def holes(src=p(vol), kind=0, dst=p(out), cls=1, dims=shape, conn=6, per_slice=0, bound=0, truth=p(vol), tk=0, cnt=p(counts), crow=0,
              st=p(stats), srow=0, work=p(ws), nbytes=need):
        hip.call("rpnet_ccpost_fill_holes", src, kind, dst, cls, *dims, conn, per_slice, bound, truth, tk, cnt, crow, st, srow, 3, work, nbytes)

    def small(src=p(vol), kind=0, dst=p(out), cls=1, dims=shape, conn=6, bound=2, truth=p(vol), tk=0, cnt=p(counts), crow=0, st=p(stats), srow=0,
              work=p(ws), nbytes=need):
        hip.call("rpnet_ccpost_remove_small", src, kind, dst, cls, *dims, conn, bound, truth, tk, cnt, crow, st, srow, 3, work, nbytes)

    for fn in (holes, small):
        for kw in (dict(src=None), dict(dst=None), dict(st=None), dict(work=None)):
            with pytest.raises(RuntimeError, match="null pointer"):
                fn(**kw)
        with pytest.raises(RuntimeError, match="kinds 4, 0"):
            fn(kind=4)
        with pytest.raises(RuntimeError, match="kinds 0, 7"):
            fn(tk=7)
        for conn in (0, 18, 4, 8):
            with pytest.raises(RuntimeError, match=f"connectivity {conn} "):
                fn(conn=conn)
        for cls in (0, 256, -1):
            with pytest.raises(RuntimeError, match=f"class {cls} "):
                fn(cls=cls)
        for srow in (3, -1):
            with pytest.raises(RuntimeError, match=f"and {srow} of tables of 3 rows"):
                fn(srow=srow)
        with pytest.raises(RuntimeError, match="rows 3 and 0"):
            fn(crow=3)
        for dims in ((1025, 1, 1), (5, 1025, 9), (5, 7, 0)):
            with pytest.raises(RuntimeError, match="every extent 1..1024"):
                fn(dims=dims)
            assert hip.query("rpnet_ccpost_workspace_bytes", *dims) == 0
            assert hip.load().rpnet_last_error_string().decode().startswith("ccpost: D=")
        with pytest.raises(RuntimeError, match=f"workspace of {need - 1} bytes, {need} needed"):
            fn(nbytes=need - 1)
        with pytest.raises(RuntimeError, match="aligned"):
            fn(work=p(ws) + 4)
        with pytest.raises(RuntimeError, match="truth and counts come together"):
            fn(truth=None)
        with pytest.raises(RuntimeError, match="truth and counts come together"):
            fn(cnt=None)
        with pytest.raises(RuntimeError, match="out overlaps in"):
            fn(src=p(vol32), kind=1, dst=p(vol32))
        with pytest.raises(RuntimeError, match="out overlaps in"):
            fn(dst=p(vol) + 1)
    for conn in (6, 26, 0):
        with pytest.raises(RuntimeError, match=f"connectivity {conn} \\(4 or 8 per slice\\)"):
            holes(conn=conn, per_slice=1)
    with pytest.raises(RuntimeError, match="max_hole_voxels -1"):
        holes(bound=-1)
    for m in (0, -3):
        with pytest.raises(RuntimeError, match=f"min_voxels {m} "):
            small(bound=m)
    assert hip.load().rpnet_last_error_string().decode().startswith("ccpost_remove_small: min_voxels -3")
    torch.cuda.synchronize()
    assert (out == FILL).all() and (stats == FILL).all() and (counts == FILL).all()
    assert np.array_equal(vol32.cpu().numpy(), host) and np.array_equal(vol.cpu().numpy(), host)
    # the same calls with nothing wrong, without truth and counts; per slice with 8
    holes(truth=None, cnt=None, conn=8, per_slice=1, srow=1)
    torch.cuda.synchronize()
    want, row = PX.ref_fill_holes(host, 1, 8, True)
    assert np.array_equal(out.cpu().numpy(), want) and stats[1].tolist() == row.tolist()
    small(truth=None, cnt=None, srow=2, bound=1 << 40)
    torch.cuda.synchronize()
    want, row = PX.ref_remove_small(host, 1, 6, 1 << 40)
    assert np.array_equal(out.cpu().numpy(), want) and stats[2].tolist() == row.tolist() and not want.any()
    assert (stats[0] == FILL).all() and (counts == FILL).all()


# ------------------------------------------------------------------------------------------------ end to end
def test_volume_segmenter_chain():
    """a 64^2 net with T = 2, a volume of 5 slices at batch 2, f32 convolutions, eager.  With the new options off the result equals,
    byte for byte and key for key, that of a VolumeSegmenter made without naming them.  With all three stages on, post['mask'] is the
    three host steps composed in the fixed order remove small -> keep largest -> fill holes on res.mask, the statistics are those of
    each step on its own input, and counts / dice describe the end of the chain; the device-table form fills the caller's tables."""
    import rpnet_amd.functional as RF
    from rpnet_amd.volume import VolumeSegmenter, dice_from_counts
    from tests.test_gpu_volume import build_net, eval_cfg, reader, segment
    RF.set_conv_math("f32")              # restored by tests/conftest.py
    cfg = eval_cfg()
    cfg["n_iter_refinement"] = 2
    item = reader(cfg, 5, 64)[0]
    net = build_net(cfg)
    labels = item["query_labels"].numpy()
    plain = segment(VolumeSegmenter(net, batch=2, graphed=False, keep_largest=26), item)
    off = segment(VolumeSegmenter(net, batch=2, graphed=False, keep_largest=26, fill_holes=False, hole_connectivity=None, max_hole=None,
                                  min_component=None), item)
    assert torch.equal(off.mask, plain.mask) and off.counts.tobytes() == plain.counts.tobytes() and off.dice == plain.dice
    assert list(off.post) == list(plain.post) == ["mask", "counts", "dice", "components", "surface"]
    assert torch.equal(off.post["mask"], plain.post["mask"]) and off.post["counts"].tobytes() == plain.post["counts"].tobytes()
    assert off.post["dice"] == plain.post["dice"] and off.post["components"] == plain.post["components"] and off.post["surface"] is None
    assert segment(VolumeSegmenter(net, batch=2, graphed=False, fill_holes=False, min_component=None), item).post is None
    mask = plain.mask.cpu().numpy()
    # all three stages on, twice: 3D holes without a bound, then per-slice holes with 8-connected background and a bound
    for m, mode, hconn, bound in ((3, True, None, None), (2, "slice", 8, 50)):
        per_slice = mode == "slice"
        res = segment(VolumeSegmenter(net, batch=2, graphed=False, keep_largest=26, fill_holes=mode, hole_connectivity=hconn, max_hole=bound,
                                      min_component=m), item)
        assert torch.equal(res.mask, plain.mask) and res.counts.tobytes() == plain.counts.tobytes() and res.dice == plain.dice
        assert sorted(res.post) == ["components", "counts", "dice", "holes", "mask", "small", "surface"]
        s1, row_s = PX.ref_remove_small(mask, 1, 26, m)
        s2, row_l = CX.ref_keep_largest(s1, 1, 26), CX.ref_stats(s1, 1, 26)
        s3, row_h = PX.ref_fill_holes(s2, 1, hconn or (4 if per_slice else 6), per_slice, bound)
        assert np.array_equal(res.post["mask"].cpu().numpy(), s3)
        assert res.post["small"] == PP.small_figures(row_s) and res.post["holes"] == PP.holes_figures(row_h)
        assert res.post["components"] == [{"n_components": int(row_l[1]), "kept": int(row_l[2]), "removed": int(row_l[0] - row_l[2])}]
        assert res.post["counts"].tolist() == [PX.ref_counts(s3, labels).tolist()] and res.post["dice"] == dice_from_counts(res.post["counts"])
        assert PP.post_overrun(DEV, mask.shape) == 0
    assert row_l[0] > 0, "the synthetic episode predicts an organ"
    # the model calls replayed from captured graphs: the chain runs behind them on the same stream and describes that run's own mask
    res = segment(VolumeSegmenter(net, batch=2, graphed=True, keep_largest=26, fill_holes=True, min_component=3), item)
    gmask = res.mask.cpu().numpy()
    s1, row_s = PX.ref_remove_small(gmask, 1, 26, 3)
    s3, row_h = PX.ref_fill_holes(CX.ref_keep_largest(s1, 1, 26), 1, 6)
    assert np.array_equal(res.post["mask"].cpu().numpy(), s3) and res.post["small"] == PP.small_figures(row_s)
    assert res.post["holes"] == PP.holes_figures(row_h) and res.post["counts"].tolist() == [PX.ref_counts(s3, labels).tolist()]
    # stages alone: 'components' is None without keep_largest; min_component in mm3 under a spacing
    res = segment(VolumeSegmenter(net, batch=2, graphed=False, fill_holes="slice"), item)
    want, row = PX.ref_fill_holes(mask, 1, 4, True)
    assert np.array_equal(res.post["mask"].cpu().numpy(), want) and res.post["components"] is None and res.post["small"] is None
    assert res.post["holes"] == PP.holes_figures(row) and res.post["counts"].tolist() == [PX.ref_counts(want, labels).tolist()]
    seg = VolumeSegmenter(net, batch=2, graphed=False, min_component=(40.0, "mm3"), spacing=(2.5, 1.0, 2.0))
    res = segment(seg, item)
    want, row = PX.ref_remove_small(mask, 1, 6, 8)
    assert PP.min_voxels_from_mm3(40.0, (2.5, 1.0, 2.0)) == 8 and np.array_equal(res.post["mask"].cpu().numpy(), want)
    assert res.post["small"] == PP.small_figures(row) and res.post["holes"] is None
    args = (item["support_images"], item["support_labels"], item["query_images"], item["appr_query_labels"])
    with pytest.raises(ValueError, match="mm3 needs a spacing"):
        VolumeSegmenter(net, batch=2, graphed=False, min_component=(40.0, "mm3"))(*args, item["query_labels"])
    # the caller's tables
    tabs = (torch.zeros((1, 3), device=DEV, dtype=torch.int64), table(1, 4))
    wide = table(1, 8)
    seg = VolumeSegmenter(net, batch=2, graphed=False, keep_largest=26, fill_holes=True, min_component=3)
    out = seg(*args, item["query_labels"], post_out=tabs, post_stats_out=wide)
    s1, row_s = PX.ref_remove_small(mask, 1, 26, 3)
    s2 = CX.ref_keep_largest(s1, 1, 26)
    s3, row_h = PX.ref_fill_holes(s2, 1, 6)
    assert np.array_equal(out.post["mask"].cpu().numpy(), s3) and all(out.post[k] is None for k in out.post if k != "mask")
    assert tabs[0].cpu().numpy().tolist() == [PX.ref_counts(s3, labels).tolist()] and tabs[1].cpu().numpy().tolist() == [CX.ref_stats(s1, 1, 26).tolist()]
    assert wide.cpu().numpy().tolist() == [row_h.tolist() + row_s.tolist()]
    with pytest.raises(ValueError, match="post_stats_out needs post_out"):
        seg(*args, item["query_labels"], post_stats_out=wide)
    with pytest.raises(ValueError, match="post_stats_out must be a contiguous int64 \\[1, 8\\]"):
        seg(*args, item["query_labels"], post_out=tabs, post_stats_out=table(1, 4))
    with pytest.raises(ValueError, match="need fill_holes"):
        VolumeSegmenter(net, batch=2, graphed=False, max_hole=5)
    with pytest.raises(ValueError, match="min_component must be"):
        VolumeSegmenter(net, batch=2, graphed=False, min_component=0)


def _chain_reference(mask, labels, conn, m, hconn, per_slice, bound):
    """the three host steps composed in the documented order -> (end of the chain, lcc row, holes row, small row)"""
    s1, row_s = PX.ref_remove_small(mask, 1, conn, m)
    s2, row_l = CX.ref_keep_largest(s1, 1, conn), CX.ref_stats(s1, 1, conn)
    s3, row_h = PX.ref_fill_holes(s2, 1, hconn, per_slice, bound)
    return s3, row_l, row_h, row_s


def test_evaluate_dataset_chain(tmp_path, capsys):
    """a synthetic NRRD set with spacing (2.5, 0.8, 0.8) in its headers, f32 convolutions, eager.  With the new options off (named with
    their defaults) every printed character, table and dictionary is that of a call that does not know them.  With the chain on
    (min_component in mm3 resolved from each header, keep_largest 26, per-slice holes) the dictionaries and earlier tables do not
    change, every line is the plain line plus the documented suffixes, out["post_stats"] and the other tables equal the three host steps
    composed on the plain run's saved masks, and save_pred holds the end of the chain.  New stages without keep_largest: no lcc fields."""
    import os
    import random

    from rpnet_amd import components as CC
    from rpnet_amd import dataset_eval as DE
    from rpnet_amd.utils import nrrd
    from rpnet_amd.volume import dice_from_counts
    from tests.test_gpu_dataset_eval import _build_net, _driver_lines, _plain
    from tests.test_gpu_surface_spacing import MM, _mm_dataset
    data_dir, set_name, cfg = _mm_dataset(tmp_path / "data", MM)
    src = DE.DeviceEvalSource(data_dir, set_name, cfg, DEV)
    src.warm()
    dirs = {k: str(tmp_path / k) for k in ("plain", "off", "chain", "bare")}
    m = PP.min_voxels_from_mm3(16.0, MM)
    assert m == 10
    runs = {}
    for name, kw in (("plain", {}), ("off", dict(fill_holes=False, hole_connectivity=None, max_hole=None, min_component=None)),
                     ("chain", dict(keep_largest=26, fill_holes="slice", hole_connectivity=8, max_hole=40, min_component=(16.0, "mm3"),
                                    spacing="header")),
                     ("bare", dict(fill_holes=True, min_component=m))):
        random.seed(77)
        capsys.readouterr()
        tabs = {}
        dicts = _plain(DE.evaluate_dataset(_build_net(cfg, "f32"), src, cfg, batch=8, graphed=False, out=tabs, save_pred=dirs[name], **kw))
        runs[name] = (dicts, tabs, capsys.readouterr().out)
    (d0, t0, o0), (d1, t1, o1), (d2, t2, o2), (d3, t3, o3) = (runs[k] for k in ("plain", "off", "chain", "bare"))
    assert o1 == o0 and d1 == d0 and sorted(t1) == sorted(t0) == ["counts", "ncc"] and all(t1[k].tobytes() == t0[k].tobytes() for k in t0)
    assert d2 == d0 and d3 == d0 and all(t2[k].tobytes() == t0[k].tobytes() == t3[k].tobytes() for k in t0)
    assert sorted(t2) == ["components", "counts", "ncc", "post_counts", "post_stats"] and sorted(t3) == ["counts", "ncc", "post_counts", "post_stats"]
    assert t2["post_stats"].shape == (3, 1, 8) and t2["post_stats"].dtype == np.int64
    l0, l2, l3 = _driver_lines(o0), _driver_lines(o2), _driver_lines(o3)
    assert len(l0) == len(l2) == len(l3) == 4
    figs = {k: [] for k in ("dice", "lcc", "holes", "small", "holes3", "small3")}
    random.seed(77)
    for j in range(3):
        s = src.item(j)
        labels = s["query_labels"].cpu().numpy()
        mask, _ = nrrd.read(os.path.join(dirs["plain"], f"{s['pid']}_Liver.nrrd"))
        same, _ = nrrd.read(os.path.join(dirs["off"], f"{s['pid']}_Liver.nrrd"))
        assert np.array_equal(same, mask)
        end, row_l, row_h, row_s = _chain_reference(mask, labels, 26, m, 8, True, 40)
        got, _ = nrrd.read(os.path.join(dirs["chain"], f"{s['pid']}_Liver.nrrd"))
        assert np.array_equal(got, end), j
        assert t2["post_stats"][j, 0].tolist() == row_h.tolist() + row_s.tolist() and t2["components"][j, 0].tolist() == row_l.tolist(), j
        assert t2["post_counts"][j, 0].tolist() == PX.ref_counts(end, labels).tolist(), j
        d, lcc = dice_from_counts(t2["post_counts"][j])[0], CC.components_figures(t2["components"][j])[0]
        h, sm = PP.holes_figures(row_h)[0], PP.small_figures(row_s)[0]
        assert l2[j] == (l0[j] + f" lcc {d} ({lcc['n_components']} components, {lcc['removed']} voxels removed)"
                         + f" holes {h['n_holes']} ({h['filled']} voxels filled) small {sm['n_removed']} ({sm['removed']} voxels removed)"), j
        s1, row_s3 = PX.ref_remove_small(mask, 1, 6, m)
        end3, row_h3 = PX.ref_fill_holes(s1, 1, 6)
        got3, _ = nrrd.read(os.path.join(dirs["bare"], f"{s['pid']}_Liver.nrrd"))
        assert np.array_equal(got3, end3) and t3["post_stats"][j, 0].tolist() == row_h3.tolist() + row_s3.tolist(), j
        assert t3["post_counts"][j, 0].tolist() == PX.ref_counts(end3, labels).tolist(), j
        assert l3[j] == l0[j] + PP.line_suffix(PP.holes_figures(row_h3)[0], PP.small_figures(row_s3)[0]) and " lcc " not in l3[j]
        for k, v in (("dice", d), ("lcc", lcc), ("holes", h), ("small", sm), ("holes3", PP.holes_figures(row_h3)[0]), ("small3", PP.small_figures(row_s3)[0])):
            figs[k].append(v)
    assert l2[3] == l0[3] + CC.mean_suffix(figs["dice"], figs["lcc"]) + PP.mean_suffix(figs["holes"], figs["small"])
    assert l3[3] == l0[3] + PP.mean_suffix(figs["holes3"], figs["small3"]) and " holes " in l3[3] and " small " in l3[3]
    # mm3 without a spacing and a spacing without a use are refused before any launch
    with pytest.raises(ValueError, match="mm3 needs a spacing"):
        DE.evaluate_dataset(None, src, cfg, min_component=(5.0, "mm3"))
    with pytest.raises(ValueError, match="give surface=True"):
        DE.evaluate_dataset(None, src, cfg, spacing=MM, min_component=5)


def test_driver_on_device_chain(tmp_path, capsys):
    """tools.eval_driver.evaluate_on_device over the host reader on one item of the same set: with the new options named at their
    defaults the output is byte-identical to a call that does not know them; with the chain on (mm3 under spacing="header", which the
    driver resolves per item) the line is the plain line plus the documented suffixes, the figures those of the three host steps on
    the plain run's saved mask, and save_pred holds the end of the chain.  The command-line forms parse."""
    import os
    import random

    from rpnet_amd.utils import nrrd
    from rpnet_amd.utils import volume_reader as VR
    from rpnet_amd.volume import VolumeSegmenter
    from tests.test_gpu_dataset_eval import _build_net, _driver_lines, _plain
    from tests.test_gpu_surface_spacing import MM, _mm_dataset
    from tools.eval_driver import build_parser, evaluate_on_device, parse_min_component
    data_dir, set_name, cfg = _mm_dataset(tmp_path / "data", MM)
    host = VR.FewshotRegReader(data_dir, set_name, cfg, mode="eval")
    outs = {}
    for name, kw in (("plain", {}), ("off", dict(fill_holes=False, hole_connectivity=None, max_hole=None, min_component=None)),
                     ("chain", dict(keep_largest=6, fill_holes="3d", min_component=(16.0, "mm3"), spacing="header", surface=True))):
        random.seed(5)
        capsys.readouterr()
        d = _plain(evaluate_on_device(_build_net(cfg, "f32"), host, cfg, 1, batch_size=8, graphed=False, save_pred=str(tmp_path / name),
                                      **dict(dict(surface=True), **kw)))
        outs[name] = (d, capsys.readouterr().out)
    assert outs["off"] == outs["plain"] and outs["chain"][0] == outs["plain"][0]
    random.seed(5)
    item = host[0]
    labels = item["query_labels"].numpy()
    mask, _ = nrrd.read(os.path.join(str(tmp_path / "plain"), f"{item['pid']}_Liver.nrrd"))
    end, row_l, row_h, row_s = _chain_reference(mask, labels, 6, 10, 6, False, None)
    got, _ = nrrd.read(os.path.join(str(tmp_path / "chain"), f"{item['pid']}_Liver.nrrd"))
    assert np.array_equal(got, end)
    lines = _driver_lines(outs["chain"][1])
    h, sm = PP.holes_figures(row_h)[0], PP.small_figures(row_s)[0]
    suffix = f" holes {h['n_holes']} ({h['filled']} voxels filled) small {sm['n_removed']} ({sm['removed']} voxels removed)"
    assert len(lines) == 2 and lines[0].endswith(suffix) and f" lcc " in lines[0] and f"({int(row_l[1])} components, " in lines[0]
    assert lines[1].endswith(PP.mean_suffix([h], [sm]))
    with pytest.raises(ValueError, match="made with the same options"):
        evaluate_on_device(None, host, cfg, 1, segmenter=VolumeSegmenter(_build_net(cfg, "f32"), batch=8, graphed=False), fill_holes=True)
    with pytest.raises(ValueError, match="mm3 needs a spacing"):
        evaluate_on_device(None, host, cfg, 1, min_component=(16.0, "mm3"))
    ap = build_parser()
    a = ap.parse_args([])
    assert a.fill_holes is None and a.max_hole is None and a.min_component is None
    assert ap.parse_args(["--fill-holes"]).fill_holes == "3d" and ap.parse_args(["--fill-holes", "slice", "--max-hole", "40"]).max_hole == 40
    assert parse_min_component(ap.parse_args(["--min-component", "16mm3"]).min_component) == (16.0, "mm3")
    assert parse_min_component("12") == 12 and parse_min_component(None) is None
    with pytest.raises(SystemExit):
        ap.parse_args(["--fill-holes", "2d"])
    with pytest.raises(ValueError, match="a number of voxels or <x>mm3"):
        parse_min_component("big")
