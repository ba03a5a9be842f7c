"""rpnet_cc_label and rpnet_cc_keep_largest (csrc/components.hip), rpnet_amd.components, VolumeSegmenter(keep_largest=...) and
evaluate_dataset(keep_largest=...) on the MI355X.

Every comparison is exact integer equality with tests/components_cases.py:ref_label and its companions (numpy; pinned to
scipy.ndimage.label by tests/test_host_components.py): labels, filtered masks, statistics rows and counts rows.  There is no tolerance.
After every call the `overrun` word of the workspace must be 0."""
import os
import random

import numpy as np
import pytest
import torch

from rpnet_amd import components as CC
from rpnet_amd import hip
from rpnet_amd import surface as SF
from tests import components_cases as CX

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 7


def dev(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(DEV)


def table(rows, cols):
    return torch.full((rows, cols), FILL, device=DEV, dtype=torch.int64)


def check_label(vol, cls, conn, what):
    """rpnet_cc_label (through label_components) == ref_label and ref_stats, the other rows untouched, no overrun"""
    stats = table(3, CC.STATS_ROW)
    labels, _ = CC.label_components(dev(vol), cls=cls, connectivity=conn, stats=stats, row=1)
    torch.cuda.synchronize()
    assert CC.overrun(DEV, vol.shape) == 0, what
    assert np.array_equal(labels.cpu().numpy(), CX.ref_label(vol, cls, conn)), what
    got = stats.cpu().numpy()
    assert got[1].tolist() == CX.ref_stats(vol, cls, conn).tolist(), what
    assert (got[[0, 2]] == FILL).all(), what
    return labels, got[1]


def check_keep(vol, cls, conn, what, truth=None, in_place=False):
    """rpnet_cc_keep_largest (through keep_largest) == ref_keep_largest, ref_stats and ref_counts; no overrun"""
    src = dev(vol)
    out = src if in_place else torch.full(vol.shape, FILL, device=DEV, dtype=torch.uint8)
    got_out, counts, stats = CC.keep_largest(src, classes=(cls,), connectivity=conn, truth=None if truth is None else dev(truth), out=out)
    torch.cuda.synchronize()
    assert CC.overrun(DEV, vol.shape) == 0, what
    want = CX.ref_keep_largest(vol, cls, conn)
    assert got_out is out and np.array_equal(out.cpu().numpy(), want), what
    if not in_place:
        assert np.array_equal(src.cpu().numpy(), vol), what
    assert stats.cpu().numpy()[0].tolist() == CX.ref_stats(vol, cls, conn).tolist(), what
    if truth is None:
        assert counts is None
    else:
        assert counts.cpu().numpy()[0].tolist() == CX.ref_counts(want, truth, cls).tolist(), what
    return out


@pytest.mark.parametrize("shape", CX.SHAPES)
def test_labels_equal_the_reference(shape):
    """every content of the table at every extent, both connectivities: labels and the statistics row, exactly"""
    assert hip.query("rpnet_cc_workspace_bytes", *shape) == 64 + 2 * ((4 * int(np.prod(shape)) + 15) // 16 * 16)
    seen = {}
    for name, vol in CX.contents(shape):
        for conn in (6, 26):
            _, row = check_label(vol, 1, conn, f"{shape} {name} {conn}")
            seen[(name, conn)] = row
    if min(shape) >= 5:
        n = int(np.prod(shape))
        assert seen[("full", 6)].tolist() == [n, 1, n, 0] and seen[("empty", 26)].tolist() == [0, 0, 0, -1]
        assert seen[("checkerboard", 6)][1] == (n + 1) // 2 and seen[("checkerboard", 26)][1] == 1
        assert seen[("serpentine", 6)][1] == 1 and seen[("u", 6)][1] == 1
        assert seen[("equal blobs", 6)][1] == 2 and seen[("equal blobs", 6)][3] == 0
        assert seen[("later blob larger", 6)][3] > 0
        assert seen[("edge", 6)][1] == 2 and seen[("edge", 26)][1] == 1 and seen[("corner", 6)][1] == 2 and seen[("corner", 26)][1] == 1


@pytest.mark.parametrize("shape", CX.SHAPES)
def test_keep_largest_equals_the_reference(shape):
    """the filter at every extent and content: out of place without a truth, in place with one (noise of another seed)"""
    truth = CX.noise(shape, 0.5, seed=9)
    for name, vol in CX.contents(shape):
        for conn in (6, 26):
            check_keep(vol, 1, conn, f"{shape} {name} {conn}")
            check_keep(vol, 1, conn, f"{shape} {name} {conn} in place", truth=truth, in_place=True)


def test_every_element_kind_and_three_classes():
    """a three-class volume: every accepted element kind of the input and of the truth gives the same labels, filtered mask and rows;
    the other classes pass through untouched; keep_largest over (1, 2, 3) equals the reference applied class by class; counts are
    added to what the table holds"""
    shape = (5, 33, 65)
    vol, truth = CX.three_classes(shape), CX.three_classes(shape, seed=4)
    for cls in (1, 2, 3):
        want = CX.ref_keep_largest(vol, cls, 26)
        assert np.array_equal(want[vol != cls], vol[vol != cls])
        for kind, tk in ((np.uint8, np.int32), (np.int32, np.int64), (np.int64, np.float32), (np.float32, np.uint8)):
            labels, _ = check_label(vol.astype(kind), cls, 26, f"label {cls} {kind}")
            out = check_keep(vol.astype(kind), cls, 26, f"keep {cls} {kind}", truth=truth.astype(tk))
            assert out.dtype == torch.uint8
    for conn in (6, 26):
        want, rows, cnts = vol, [], []
        for cls in (1, 2, 3):
            rows.append(CX.ref_stats(vol, cls, conn).tolist())
            want = CX.ref_keep_largest(want, cls, conn)
        cnts = [CX.ref_counts(want, truth, cls).tolist() for cls in (1, 2, 3)]
        counts = torch.full((3, CC.COUNTS_ROW), 5, device=DEV, dtype=torch.int64)
        out, counts, stats = CC.keep_largest(dev(vol), classes=(1, 2, 3), connectivity=conn, truth=dev(truth), counts=counts)
        torch.cuda.synchronize()
        assert CC.overrun(DEV, shape) == 0
        assert np.array_equal(out.cpu().numpy(), want) and stats.cpu().numpy().tolist() == rows
        assert (counts.cpu().numpy() - 5).tolist() == cnts
    with pytest.raises(ValueError, match="uint8, int32, int64 and float32"):
        CC.label_components(dev(vol.astype(np.float64)))
    with pytest.raises(ValueError, match="contiguous"):
        CC.keep_largest(dev(vol)[:, :, ::2])
    with pytest.raises(ValueError, match="counts need a truth"):
        CC.keep_largest(dev(vol), counts=table(1, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CC.keep_largest(torch.from_numpy(vol))


def test_runs_are_bit_identical():
    """noise at the density with the most merges, twice: the same labels, masks and rows, byte for byte"""
    vol = CX.noise((10, 66, 130), 0.31)
    runs = []
    for _ in range(2):
        labels, stats = CC.label_components(dev(vol), connectivity=26)
        out, counts, kstats = CC.keep_largest(dev(vol), connectivity=26, truth=dev(CX.noise(vol.shape, 0.5, seed=9)))
        torch.cuda.synchronize()
        assert CC.overrun(DEV, vol.shape) == 0
        runs.append([t.cpu().numpy().tobytes() for t in (labels, stats, out, counts, kstats)])
    assert runs[0] == runs[1]


def test_refusals_launch_nothing():
    """every refusal of include/rpnet_cc_abi.h returns its status with a message; the output and the tables hold what they held"""
    shape = (5, 7, 9)
    vol = dev(CX.noise(shape, 0.4))
    vol32 = vol.to(torch.int32)
    out = torch.full(shape, FILL, device=DEV, dtype=torch.uint8)
    labels = torch.full(shape, FILL, device=DEV, dtype=torch.int32)
    stats, counts = table(3, CC.STATS_ROW), table(3, CC.COUNTS_ROW)
    p = hip.ptr
    need = hip.query("rpnet_cc_workspace_bytes", *shape)
    ws = torch.empty(need + 16, device=DEV, dtype=torch.uint8)

    def keep(src=p(vol), kind=0, dst=p(out), cls=1, dims=shape, conn=6, truth=p(vol), tk=0, cnt=p(counts), crow=0, st=p(stats), srow=0,
             work=p(ws), nbytes=need):
        hip.call("rpnet_cc_keep_largest", src, kind, dst, cls, *dims, conn, truth, tk, cnt, crow, st, srow, 3, work, nbytes)

    def label(src=p(vol), kind=0, cls=1, dims=shape, conn=6, lab=p(labels), st=p(stats), srow=0, work=p(ws), nbytes=need):
        hip.call("rpnet_cc_label", src, kind, cls, *dims, conn, lab, st, srow, 3, work, nbytes)

    for fn in (keep, label):
        for kw in (dict(src=None), dict(st=None), dict(work=None)):
            with pytest.raises(RuntimeError, match="null pointer"):
                fn(**kw)
        with pytest.raises(RuntimeError, match="kind"):
            fn(kind=4)
        for conn in (0, 18, 8):
            with pytest.raises(RuntimeError, match=f"connectivity {conn}"):
                fn(conn=conn)
        for srow in (3, -1):
            with pytest.raises(RuntimeError, match=f"{srow} of "):
                fn(srow=srow)
        for dims in ((1025, 1, 1), (5, 1025, 9), (5, 7, 0)):
            with pytest.raises(RuntimeError, match="every extent 1..1024"):
                fn(dims=dims)
            assert hip.query("rpnet_cc_workspace_bytes", *dims) == 0
            assert hip.load().rpnet_last_error_string().decode().startswith("components: D=")
        with pytest.raises(RuntimeError, match=f"workspace of {need - 1} bytes, {need} needed"):
            fn(nbytes=need - 1)
        with pytest.raises(RuntimeError, match="aligned"):
            fn(work=p(ws) + 4)
    with pytest.raises(RuntimeError, match="null pointer"):
        keep(dst=None)
    with pytest.raises(RuntimeError, match="null pointer"):
        label(lab=None)
    with pytest.raises(RuntimeError, match="truth and counts come together"):
        keep(truth=None)
    with pytest.raises(RuntimeError, match="truth and counts come together"):
        keep(cnt=None)
    with pytest.raises(RuntimeError, match="kinds 0, 7"):
        keep(tk=7)
    for cls in (0, 256, -1):
        with pytest.raises(RuntimeError, match=f"class {cls} "):
            keep(cls=cls)
    with pytest.raises(RuntimeError, match="rows 3 and 0"):
        keep(crow=3)
    with pytest.raises(RuntimeError, match="out overlaps in"):
        keep(src=p(vol32), kind=1, dst=p(vol32))
    with pytest.raises(RuntimeError, match="out overlaps in"):
        keep(dst=p(vol) + 1)
    assert hip.load().rpnet_last_error_string().decode().startswith("cc_keep_largest: out overlaps in")
    torch.cuda.synchronize()
    assert (out == FILL).all() and (labels == FILL).all() and (stats == FILL).all() and (counts == FILL).all()
    assert np.array_equal(vol32.cpu().numpy(), vol.cpu().numpy())
    # the same calls with nothing wrong; without truth and counts
    keep(truth=None, cnt=None)
    label(srow=2)
    torch.cuda.synchronize()
    host = vol.cpu().numpy()
    assert np.array_equal(out.cpu().numpy(), CX.ref_keep_largest(host)) and np.array_equal(labels.cpu().numpy(), CX.ref_label(host))
    assert stats[0].tolist() == stats[2].tolist() == CX.ref_stats(host).tolist() and (stats[1] == FILL).all() and (counts == FILL).all()


# ------------------------------------------------------------------------------------------------ end to end
def test_volume_segmenter_keep_largest():
    """a 64^2 net with T = 2, a volume of 5 slices at batch 2 (the last batch holds a filler slice), f32 convolutions, eager:
    mask, counts and dice equal those of a segmenter without the option; post['mask'] equals ref_keep_largest of res.mask (so the
    filler did not enter the components: they are those of the 5 slices), post['counts'] numpy's; post_out fills the caller's tables and
    leaves the post values None.  The same on a mask with an island, through keep_largest itself on res.mask with the island added."""
    import rpnet_amd.functional as RF
    from rpnet_amd.volume import VolumeSegmenter, dice_from_counts
    from tests.test_gpu_volume import build_net, eval_cfg, reader, segment
    RF.set_conv_math("f32")              # restored by tests/conftest.py
    cfg = eval_cfg()
    cfg["n_iter_refinement"] = 2
    item = reader(cfg, 5, 64)[0]
    net = build_net(cfg)
    plain = segment(VolumeSegmenter(net, batch=2, graphed=False), item)
    assert plain.post is None
    labels = item["query_labels"].numpy()
    for option, conn in ((True, 6), (26, 26)):
        res = segment(VolumeSegmenter(net, batch=2, graphed=False, keep_largest=option), item)
        assert torch.equal(res.mask, plain.mask) and res.counts.tobytes() == plain.counts.tobytes() and res.dice == plain.dice
        assert res.surface is None and sorted(res.post) == ["components", "counts", "dice", "mask", "surface"]
        mask = res.mask.cpu().numpy()
        want = CX.ref_keep_largest(mask, 1, conn)
        assert res.post["mask"].shape == (5, 64, 64) and np.array_equal(res.post["mask"].cpu().numpy(), want)
        row = CX.ref_stats(mask, 1, conn)
        assert res.post["components"] == [{"n_components": int(row[1]), "kept": int(row[2]), "removed": int(row[0] - row[2])}]
        assert res.post["counts"].tolist() == [CX.ref_counts(want, labels).tolist()]
        assert res.post["dice"] == dice_from_counts(res.post["counts"]) and res.post["surface"] is None
        assert CC.overrun(DEV, mask.shape) == 0
    assert row[0] > 0, "the synthetic episode predicts an organ"
    # an island far from the organ: the filter removes exactly it
    island = mask.copy()
    from scipy import ndimage
    free = np.argwhere(ndimage.maximum_filter(mask, size=3, mode="constant") == 0)      # background with a background neighbourhood
    z, y, x = free[0]
    island[z, y, x] = 1
    out, _, stats = CC.keep_largest(dev(island), connectivity=6)
    assert np.array_equal(out.cpu().numpy(), CX.ref_keep_largest(island)) and stats[0, 1].item() == CX.ref_stats(island)[1]
    # with surface: one more tally of the filtered mask per class, equal to surface_tally by hand
    res = segment(VolumeSegmenter(net, batch=2, graphed=False, surface=True, keep_largest=6), item)
    assert res.surface == segment(VolumeSegmenter(net, batch=2, graphed=False, surface=True), item).surface
    it = torch.zeros((1, SF.IROW), device=DEV, dtype=torch.int64)
    ft = torch.zeros((1, SF.FROW), device=DEV, dtype=torch.float64)
    SF.surface_tally(res.post["mask"], dev(labels.astype(np.int32)), it, 0, ft, 0)
    assert res.post["surface"] == SF.surface_figures(it.cpu().numpy(), ft.cpu().numpy())
    # the caller's tables
    tabs = (torch.zeros((1, 3), device=DEV, dtype=torch.int64), table(1, 4), (table(1, SF.IROW), torch.zeros((1, SF.FROW), device=DEV, dtype=torch.float64)))
    seg = VolumeSegmenter(net, batch=2, graphed=False, surface=True, keep_largest=6)
    out = seg(item["support_images"], item["support_labels"], item["query_images"], item["appr_query_labels"], item["query_labels"], post_out=tabs)
    want = CX.ref_keep_largest(mask, 1, 6)
    assert np.array_equal(out.post["mask"].cpu().numpy(), want)
    assert all(out.post[k] is None for k in ("counts", "dice", "components", "surface"))
    assert tabs[0].cpu().numpy().tolist() == [CX.ref_counts(want, labels).tolist()] and tabs[1].cpu().numpy().tolist() == [CX.ref_stats(mask).tolist()]
    assert torch.equal(tabs[2][0], it) and torch.equal(tabs[2][1], ft)
    with pytest.raises(ValueError, match="post_out needs VolumeSegmenter"):
        VolumeSegmenter(net, batch=2, graphed=False)(item["support_images"], item["support_labels"], item["query_images"],
                                                     item["appr_query_labels"], item["query_labels"], post_out=tabs[:2])
    with pytest.raises(ValueError, match="post_out needs query_labels"):
        seg(item["support_images"], item["support_labels"], item["query_images"], item["appr_query_labels"], post_out=tabs)
    with pytest.raises(ValueError, match="post_out must be contiguous tensors"):
        seg(item["support_images"], item["support_labels"], item["query_images"], item["appr_query_labels"], item["query_labels"], post_out=tabs[:2])
    # without labels: the filtered mask and the components alone
    bare = VolumeSegmenter(net, batch=2, graphed=False, keep_largest=6)(item["support_images"], item["support_labels"], item["query_images"],
                                                                        item["appr_query_labels"])
    assert bare.counts is None and bare.post["counts"] is None and bare.post["dice"] is None
    assert np.array_equal(bare.post["mask"].cpu().numpy(), want) and bare.post["components"][0]["kept"] == int(CX.ref_stats(mask)[2])


def test_evaluate_dataset_keep_largest(tmp_path, capsys):
    """the small synthetic NRRD set of tests/test_gpu_dataset_eval.py, f32 convolutions, eager: the three returned dictionaries and the
    earlier tables equal those of a run without the option; every printed line is that run's line plus exactly the documented suffix;
    the new `out` tables match the reference per item (the unfiltered masks come from the plain run's save_pred, the filtered ones
    from this run's); with surface=True the third tally equals surface_tally called by hand on the filtered mask"""
    from rpnet_amd import dataset_eval as DE
    from rpnet_amd.utils import nrrd
    from rpnet_amd.volume import dice_from_counts
    from tests.test_gpu_dataset_eval import _build_net, _dataset, _driver_lines, _eval_cfg, _plain
    data_dir, set_name, cfg = _dataset(tmp_path / "data", do_deformable=False)
    cfg = _eval_cfg(cfg)
    src = DE.DeviceEvalSource(data_dir, set_name, cfg, DEV)
    src.warm()
    dir0, dir1 = str(tmp_path / "pred0"), str(tmp_path / "pred1")
    random.seed(77)
    capsys.readouterr()
    t0, t1 = {}, {}
    want = _plain(DE.evaluate_dataset(_build_net(cfg, "f32"), src, cfg, batch=8, graphed=False, out=t0, surface=True, save_pred=dir0))
    lines0 = _driver_lines(capsys.readouterr().out)
    random.seed(77)
    got = _plain(DE.evaluate_dataset(_build_net(cfg, "f32"), src, cfg, batch=8, graphed=False, out=t1, surface=True, save_pred=dir1,
                                     keep_largest=26))
    lines1 = _driver_lines(capsys.readouterr().out)
    assert got == want
    assert sorted(t1) == sorted(list(t0) + ["components", "post_counts", "post_surface_f", "post_surface_i"])
    for key in t0:
        assert t0[key].tobytes() == t1[key].tobytes(), key
    assert t1["post_counts"].shape == (3, 1, 3) and t1["components"].shape == (3, 1, 4) and t1["post_surface_i"].shape == (3, 1, SF.IROW)
    assert t1["post_surface_f"].shape == (3, 1, SF.FROW) and t1["post_counts"].dtype == t1["components"].dtype == np.int64
    assert len(lines0) == len(lines1) == 4
    dices, figs, surfs = [], [], []
    random.seed(77)
    for j in range(3):
        s = src.item(j)
        labels = s["query_labels"].cpu().numpy()
        mask, _ = nrrd.read(os.path.join(dir0, f"{s['pid']}_Liver.nrrd"))
        kept, _ = nrrd.read(os.path.join(dir1, f"{s['pid']}_Liver.nrrd"))
        assert np.array_equal(kept, CX.ref_keep_largest(mask, 1, 26)), j
        assert t1["components"][j, 0].tolist() == CX.ref_stats(mask, 1, 26).tolist(), j
        assert t1["post_counts"][j, 0].tolist() == CX.ref_counts(kept, labels).tolist(), j
        it = torch.zeros((1, SF.IROW), device=DEV, dtype=torch.int64)
        ft = torch.zeros((1, SF.FROW), device=DEV, dtype=torch.float64)
        SF.surface_tally(dev(kept), s["query_labels"], it, 0, ft, 0)
        assert np.array_equal(it.cpu().numpy(), t1["post_surface_i"][j]) and ft.cpu().numpy().tobytes() == t1["post_surface_f"][j].tobytes()
        d, fig = dice_from_counts(t1["post_counts"][j])[0], CC.components_figures(t1["components"][j])[0]
        (surf,) = SF.surface_figures(t1["post_surface_i"][j], t1["post_surface_f"][j])
        suffix = (f" lcc {d} ({fig['n_components']} components, {fig['removed']} voxels removed)"
                  f" lcc hd95 {SF.fmt(surf['hd95'])} assd {SF.fmt(surf['assd'])}")
        assert lines1[j] == lines0[j] + suffix, (lines0[j], lines1[j])
        dices.append(d), figs.append(fig), surfs.append(surf)
    assert lines1[3] == lines0[3] + CC.mean_suffix(dices, figs, surfs) and " lcc " in lines1[3] and " components, " in lines1[3]
    # without surface: the shorter suffix, and only the two new tables
    random.seed(77)
    t2 = {}
    DE.evaluate_dataset(_build_net(cfg, "f32"), src, cfg, batch=8, graphed=False, out=t2, keep_largest=True, n_items=1)
    line = _driver_lines(capsys.readouterr().out)[0]
    assert sorted(t2) == ["components", "counts", "ncc", "post_counts"] and " lcc hd95 " not in line and line.endswith(" voxels removed)")


def test_driver_on_device_keep_largest(tmp_path, capsys):
    """tools.eval_driver.evaluate_on_device(keep_largest=26) on one synthetic item: the same dictionaries, the line of a run without
    the option plus the documented suffix, the filtered mask under save_pred; a segmenter handed in must have been made with the option"""
    from rpnet_amd.utils import nrrd
    from rpnet_amd.volume import VolumeSegmenter
    from tests.test_gpu_dataset_eval import _driver_lines, _plain
    from tests.test_gpu_volume import OneItem, build_net, eval_cfg, reader, segment
    from tools.eval_driver import evaluate_on_device
    cfg = eval_cfg()
    cfg["n_iter_refinement"] = 2
    item = reader(cfg, 3, 64)[0]
    capsys.readouterr()
    want = _plain(evaluate_on_device(build_net(cfg), OneItem(item), cfg, batch_size=2, graphed=False))
    lines0 = _driver_lines(capsys.readouterr().out)
    got = _plain(evaluate_on_device(build_net(cfg), OneItem(item), cfg, batch_size=2, graphed=False, save_pred=str(tmp_path), keep_largest=26))
    lines1 = _driver_lines(capsys.readouterr().out)
    assert got == want and len(lines0) == len(lines1) == 2
    res = segment(VolumeSegmenter(build_net(cfg), batch=2, graphed=False, keep_largest=26), item)
    fig = res.post["components"][0]
    assert lines1[0] == lines0[0] + f" lcc {res.post['dice'][0]} ({fig['n_components']} components, {fig['removed']} voxels removed)"
    assert lines1[1] == lines0[1] + CC.mean_suffix(res.post["dice"], res.post["components"])
    data, _ = nrrd.read(os.path.join(str(tmp_path), f"{item['pid']}_Liver.nrrd"))
    assert np.array_equal(data, res.post["mask"].cpu().numpy()) and np.array_equal(data, CX.ref_keep_largest(res.mask.cpu().numpy(), 1, 26))
    with pytest.raises(ValueError, match="needs a VolumeSegmenter\\(keep_largest=6\\)"):
        evaluate_on_device(None, OneItem(item), cfg, segmenter=VolumeSegmenter(build_net(cfg), batch=2, graphed=False), keep_largest=6)
