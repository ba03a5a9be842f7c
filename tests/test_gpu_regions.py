"""Region statistics on the device (csrc/regions.hip through include/rpnet_region_abi.h and rpnet_amd/regions.py) against the numpy
restatement of tests/regions_cases.py: the integer rows EQUAL, the float64 sums bit for bit, the n_outside word equal.  Every call is
made twice into tables prefilled with sentinels, with guard words behind the tables and the workspace, and gives the same bits."""
import json
import random
import sys

import numpy as np
import pytest
import torch

from rpnet_amd import hip
from rpnet_amd import regions as R
from tests import regions_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TORCH = {"u8": torch.uint8, "i32": torch.int32, "i64": torch.int64, "f32": torch.float32, "i16": torch.int16}
FILL_I, GUARD = -7, 0x5A


def dev(a, dtype, offset=0):
    """`a` on the device as `dtype`; offset: that many ELEMENTS into a larger allocation"""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    if not offset:
        return t.to(DEV)
    buf = torch.zeros((t.numel() + offset + 16,), dtype=dtype, device=DEV)
    view = buf[offset:offset + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() - buf.data_ptr() == offset * t.element_size()
    return view


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def run_stats(labels, image=None, lo=1, L=2, kind="u8", ikind="f32", loff=0, ioff=0, row=1, n_rows=3):
    """R.region_stats twice on the device against RC.restate: everything equal; the other rows, the words behind the tables and behind
    the workspace untouched -> (rows_i, rows_f, n_outside) of the restatement"""
    labels = np.asarray(labels)
    cast = labels.astype({"u8": np.uint8, "i32": np.int32, "i64": np.int64, "f32": np.float32}[kind])
    want_i, want_f, want_out = RC.restate(cast, image, lo=lo, L=L)
    d_labels = dev(cast, TORCH[kind], loff)
    d_image = None if image is None else dev(image, TORCH[ikind], ioff)
    need = hip.query("rpnet_region_workspace_bytes", *labels.shape, L)
    assert need == R._workspace_layout(*labels.shape, L)[1]
    runs = []
    for fill in (0, 0xFF):              # whatever the workspace holds before the call
        ws = torch.full((need + 64,), GUARD, dtype=torch.uint8, device=DEV)
        ws[:need] = fill
        bi = torch.full((n_rows * L * R.IROW + 8,), FILL_I, dtype=torch.int64, device=DEV)
        bf = torch.full((n_rows * L * R.FROW + 8,), float("nan"), dtype=torch.float64, device=DEV)
        ri, rf = bi[:n_rows * L * R.IROW].view(n_rows, L, R.IROW), bf[:n_rows * L * R.FROW].view(n_rows, L, R.FROW)
        got = R.region_stats(d_labels, d_image, n_labels=L, skip_background=bool(lo), out=(ri, rf), row=row, workspace=ws[:need])
        assert got[0] is ri and got[1] is rf
        assert (ws[need:] == GUARD).all() and (bi[n_rows * L * R.IROW:] == FILL_I).all() and torch.isnan(bf[n_rows * L * R.FROW:]).all()
        for other in range(n_rows):
            if other != row:
                assert (ri[other] == FILL_I).all() and torch.isnan(rf[other]).all()
        runs.append((ri[row].cpu().numpy(), rf[row].cpu().numpy(), int(R.region_outside(ws).item())))
    (a_i, a_f, a_o), (b_i, b_f, b_o) = runs
    assert a_i.tobytes() == b_i.tobytes() and a_f.tobytes() == b_f.tobytes() and a_o == b_o, "two runs differ"
    assert np.array_equal(a_i, want_i), (np.argwhere(a_i != want_i)[:8], a_i[a_i != want_i][:8], want_i[a_i != want_i][:8])
    assert np.array_equal(bits(a_f), bits(want_f)), (a_f, want_f)
    assert a_o == want_out
    return want_i, want_f, want_out


@pytest.mark.parametrize("shape", RC.SHAPES)
def test_shapes(shape):
    """one voxel; the lane edge; lanes that straddle a row end and a slice end; the chunk edge; each axis of length 1; a line of 1024
    along each axis: smooth regions (wave-uniform runs with mixed borders) and independent labels, lo = 0 and lo = 1"""
    image = RC.image_for(shape, sum(shape))
    want_i, _, _ = run_stats(RC.blob_labels(shape, 4, sum(shape) + 1), image, lo=1, L=4)
    run_stats(RC.noise_labels(shape, 5, sum(shape) + 2, outside=1), image, lo=0, L=5)
    run_stats(np.ones(shape, np.uint8), image, lo=1, L=2)               # every wave holds one label
    if shape in ((1024, 1, 1), (1, 1024, 1), (1, 1, 1024)):
        axis = shape.index(1024)
        full = run_stats(np.ones(shape, np.uint8), None, lo=1, L=2)[0][1]
        assert full[4 + axis] == 1023 and full[10 + axis] == sum(v * v for v in range(1024))


def test_second_trip_of_a_block():
    """more than 1024 chunks: blocks 0 .. 2 make a second trip, the last lanes of which lie beyond the volume"""
    shape = RC.TWO_TRIPS
    assert -(-shape[0] * shape[1] * shape[2] // 4096) > 1024
    run_stats(RC.blob_labels(shape, 4, 3), RC.image_for(shape, 9), lo=1, L=4, n_rows=1, row=0)


def test_label_counts():
    """L = 1 (with lo = 1 one empty row); L = 256 with every label in every wave; values that are no label"""
    shape = (1, 4, 1024)
    every = (np.arange(4096) % 256).astype(np.uint8).reshape(shape)
    image = RC.image_for(shape, 1)
    for lo in (0, 1):
        want_i, _, out = run_stats(every, image, lo=lo, L=256)
        assert out == 0 and (want_i[lo:, 0] == 16).all()
        want_i, _, out = run_stats(every, image, lo=lo, L=1)
        assert out == 4096 - 16 and want_i[0, 0] == (0 if lo else 16)
        want_i, _, out = run_stats(every, image, lo=lo, L=100)
        assert out == 16 * 156
    mixed = np.array([0, 1, 2, 3, -1, -2, 4, 300, 2 ** 31 - 1, -2 ** 31] * 7, np.int64).reshape(1, 7, 10)
    for kind in ("i32", "i64"):
        assert run_stats(mixed, RC.image_for(mixed.shape, 2), lo=1, L=4, kind=kind)[2] == 6 * 7
    big = mixed.copy()
    big[0, 0, :2] = (2 ** 40 + 1, -2 ** 40)         # an int64 whose low 32 bits are a label
    assert run_stats(big, None, lo=0, L=4, kind="i64")[2] == 6 * 7 + 2
    floats = np.array([0.0, -0.0, 1.0, 2.0, 3.0, 0.5, 2.5, -1.0, np.nan, np.inf, -np.inf, 4.0, 255.0, 256.0, 1e9, 1e-42] * 5, np.float32).reshape(1, 5, 16)
    assert run_stats(floats, RC.image_for(floats.shape, 3), lo=0, L=4, kind="f32")[2] == 11 * 5
    assert run_stats(floats, None, lo=1, L=256, kind="f32")[2] == 9 * 5


@pytest.mark.parametrize("kind", ["u8", "i32", "i64", "f32"])
def test_every_label_kind_both_image_kinds_and_offset_pointers(kind):
    """pointers one element into an allocation take the element-wise path (a uint8 volume at an odd address, an int16 image on a 2-byte
    boundary); 16 elements in, the 16-byte path from a base that torch did not align"""
    shape = (2, 17, 241)
    labels = RC.blob_labels(shape, 3, 5)
    for ikind in ("f32", "i16"):
        image = RC.image_for(shape, 6, ikind)
        for loff, ioff in ((0, 0), (1, 0), (0, 1), (1, 1), (16, 16)):
            run_stats(labels, image, lo=1, L=3, kind=kind, ikind=ikind, loff=loff, ioff=ioff)
    run_stats(labels, None, lo=0, L=3, kind=kind, loff=1)


def test_image_values():
    """both ends of the int16 range; +-FLT_MAX, subnormals and -0.0; NaN and +-inf beside finite values; a label whose image values are
    all non-finite; no image"""
    shape = (3, 9, 13)
    labels = RC.noise_labels(shape, 4, 8)
    assert all((labels == l).sum() > 8 for l in range(4))
    ends = RC.image_for(shape, 1, "i16")
    ends.ravel()[::5] = -32768
    ends.ravel()[1::7] = 32767
    want_i, _, _ = run_stats(labels, ends, lo=0, L=4, ikind="i16")
    assert (RC.key_value(want_i[:, 17]) == -32768.0).all() and (RC.key_value(want_i[:, 18]) == 32767.0).all()
    big = np.finfo(np.float32).max
    special = RC.image_for(shape, 2)
    special.ravel()[::3] = np.resize(np.array([big, -big, 1e-42, -1e-42, -0.0, 0.0, np.nan, np.inf, -np.inf], np.float32), special.ravel()[::3].size)
    special[labels == 3] = np.resize(np.array([np.nan, np.inf, -np.inf], np.float32), int((labels == 3).sum()))
    want_i, want_f, _ = run_stats(labels, special, lo=0, L=4)
    assert want_i[3, 0] > 0 and want_i[3, 16] == 0 and want_i[3, 17] == 0xFFFFFFFF and want_i[3, 18] == 0 and (want_f[3] == 0).all()
    assert (want_i[:3, 16] < want_i[:3, 0]).all() and np.isfinite(want_f).all()
    tiny = np.full(shape, -0.0, np.float32)
    tiny[labels == 1] = -1e-42
    tiny[labels == 2] = 1e-45
    want_i, _, _ = run_stats(labels, tiny, lo=0, L=4)
    assert want_i[0, 17] == want_i[0, 18] == 0x80000000         # -0.0 is taken as +0.0
    want_i, want_f, _ = run_stats(labels, None, lo=1, L=4)
    assert (want_i[:, 16] == 0).all() and (want_f == 0).all()
    # rows_f may be absent without an image
    d = dev(labels, torch.uint8)
    ri = torch.full((1, 4, R.IROW), FILL_I, dtype=torch.int64, device=DEV)
    got_i, got_f = R.region_stats(d, None, n_labels=4, out=(ri, None))
    assert got_f is None and np.array_equal(got_i[0].cpu().numpy(), want_i)
    # the default workspace, tables and label count: uint8 labels without n_labels are tallied over 256 labels
    got_i, got_f = R.region_stats(d, dev(special, torch.float32))
    assert got_i.shape == (256, R.IROW) and got_f.shape == (256, R.FROW)
    ref_i, ref_f, _ = RC.restate(labels, special, lo=1, L=256)
    assert np.array_equal(got_i.cpu().numpy(), ref_i) and np.array_equal(bits(got_f.cpu().numpy()), bits(ref_f))
    assert int(R.region_outside(R.region_workspace(shape, 256, DEV)).item()) == 0


def test_captured_graph_of_region_stats_replayed_twice():
    shape = (3, 37, 41)
    labels, image = RC.blob_labels(shape, 4, 11), RC.image_for(shape, 12)
    want_i, want_f, _ = RC.restate(labels, image, lo=1, L=4)
    d_labels, d_image = dev(labels, torch.uint8), dev(image, torch.float32)
    ri = torch.zeros((1, 4, R.IROW), dtype=torch.int64, device=DEV)
    rf = torch.zeros((1, 4, R.FROW), dtype=torch.float64, device=DEV)
    R.region_stats(d_labels, d_image, n_labels=4, out=(ri, rf))             # the workspace is allocated before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            R.region_stats(d_labels, d_image, n_labels=4, out=(ri, rf))
    for replay in range(2):
        ri.fill_(FILL_I)
        rf.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(ri[0].cpu().numpy(), want_i) and np.array_equal(bits(rf[0].cpu().numpy()), bits(want_f)), replay


def raw_stats(labels, rows_i, rows_f, ws, image=None, label_kind=0, image_kind=0, dims=None, lo=1, L=2, row=0, n_rows=2, ws_bytes=None):
    """rpnet_region_stats itself -> (status, error string)"""
    lib = hip.load()
    D, H, W = dims or (labels.shape if torch.is_tensor(labels) else (3, 9, 13))
    p = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())  # noqa: E731
    rc = lib.rpnet_region_stats(p(labels), label_kind, p(image), image_kind, D, H, W, lo, L, p(rows_i), p(rows_f), row, n_rows, p(ws),
                                (ws.numel() if torch.is_tensor(ws) else 0) if ws_bytes is None else ws_bytes, hip.stream())
    return rc, lib.rpnet_last_error_string().decode()


def test_refusals_launch_nothing():
    shape = (3, 9, 13)
    labels = dev(RC.blob_labels(shape, 2, 1), torch.uint8)
    image = dev(RC.image_for(shape, 2), torch.float32)
    need = hip.query("rpnet_region_workspace_bytes", *shape, 2)
    ws = torch.full((need + 16,), GUARD, dtype=torch.uint8, device=DEV)
    ri = torch.full((2, 2, R.IROW), FILL_I, dtype=torch.int64, device=DEV)
    rf = torch.full((2, 2, R.FROW), -5.0, dtype=torch.float64, device=DEV)
    base = dict(labels=labels, rows_i=ri, rows_f=rf, ws=ws, image=image)
    rc, err = raw_stats(**dict(base, ws_bytes=need))
    assert rc == 0, err
    ri.fill_(FILL_I)
    rf.fill_(-5.0)
    ws.fill_(GUARD)
    torch.cuda.synchronize()
    bad = [dict(labels=None), dict(rows_i=None), dict(ws=None), dict(rows_f=None), dict(label_kind=4), dict(label_kind=-1), dict(image_kind=2),
           dict(image_kind=-1), dict(lo=2), dict(lo=-1), dict(L=0), dict(L=257), dict(L=1, lo=0, image=None, rows_f=None, labels=None),
           dict(lo=1, L=1, ws=None), dict(dims=(0, 9, 13)), dict(dims=(3, 1025, 13)), dict(dims=(3, 9, -1)), dict(row=2), dict(row=-1),
           dict(n_rows=0), dict(ws_bytes=need - 1), dict(ws=ws.data_ptr() + 8, ws_bytes=need), dict(labels=labels.data_ptr() + 1, label_kind=1),
           dict(labels=labels.data_ptr() + 4, label_kind=2), dict(labels=labels.data_ptr() + 2, label_kind=3), dict(image=image.data_ptr() + 2),
           dict(image=image.data_ptr() + 1, image_kind=1), dict(rows_i=ri.data_ptr() + 4), dict(rows_f=rf.data_ptr() + 4)]
    for over in bad:
        rc, err = raw_stats(**dict(base, **over))
        assert rc != 0 and err.startswith("region_stats:"), (over, rc, err)
    for q in ((0, 9, 13, 2), (3, 9, 13, 0), (3, 9, 13, 257), (3, 9, 1025, 2)):
        assert hip.query("rpnet_region_workspace_bytes", *q) == 0
        assert hip.load().rpnet_last_error_string().decode().startswith("region_workspace_bytes:")
    torch.cuda.synchronize()
    assert (ri == FILL_I).all() and (rf == -5.0).all() and (ws == GUARD).all()
    # lo = L = 1 is accepted and writes one empty row
    one = torch.full((1, 1, R.IROW), FILL_I, dtype=torch.int64, device=DEV)
    rc, err = raw_stats(labels, one, None, ws, lo=1, L=1, n_rows=1)
    assert rc == 0, err
    assert np.array_equal(one[0, 0].cpu().numpy(), RC.empty_row(shape))
    # the Python layer on device tensors
    for kw in (dict(n_labels=0), dict(n_labels=257), dict(image=image[:2]), dict(image=image.double()), dict(row=1),
               dict(n_labels=2, out=(ri, rf), row=2), dict(n_labels=3, out=(ri, rf)), dict(workspace=ws[:need - 16]),
               dict(n_labels=2, workspace=ws[8:8 + need])):
        with pytest.raises(ValueError):
            R.region_stats(labels, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.region_stats(labels.cpu())
    with pytest.raises(ValueError):
        R.region_stats(labels.to(torch.int32))


# ----------------------------------------------------------------------------------------------------------------- end to end
MM = (2.5, 0.8, 0.8)


def mm_dataset(tmp_path):
    from rpnet_amd.utils import volume_reader as VR
    from tests.test_gpu_dataset_eval import CASE, _eval_cfg, config_for
    data_dir, set_name, csv_dir = VR.write_synthetic_dataset(str(tmp_path), spacing=MM, **CASE["data"])
    return data_dir, set_name, _eval_cfg(dict(config_for(CASE, csv_dir), use_registration_mask=False, do_deformable=False))


def item_image(item):
    return item["query_images"][:, 0].contiguous().cpu().numpy()


def test_volume_segmenter_regions_eager_and_graphed(tmp_path):
    """VolumeSegmenter(regions=True) on an item of the synthetic data set: its tables equal the restatement applied to the mask it returns
    (the end of the clean-up chain where one is on) and to the labels, eagerly and through the captured graph, into the caller's tables
    without a host synchronisation; mask, counts and dice are those of regions=False"""
    from rpnet_amd import dataset_eval as DE
    from rpnet_amd.volume import VolumeSegmenter
    from tests.test_gpu_dataset_eval import _build_net
    data_dir, set_name, cfg = mm_dataset(tmp_path)
    src = DE.DeviceEvalSource(data_dir, set_name, cfg, DEV)
    src.warm()
    net = _build_net(cfg, "f32")
    random.seed(3)
    item = src.item(0)
    args = (item["support_images"], item["support_labels"], item["query_images"], item["appr_query_labels"], item["query_labels"])
    image, labels = item_image(item), item["query_labels"].cpu().numpy().astype(np.int32)
    for graphed in (False, True):
        plain = VolumeSegmenter(net, batch=8, graphed=graphed)(*args)
        assert plain.regions is None
        for chain in ({}, dict(keep_largest=6, fill_holes=True)):
            res = VolumeSegmenter(net, batch=8, graphed=graphed, regions=True, **chain)(*args, spacing=MM)
            assert torch.equal(res.mask, plain.mask) and np.array_equal(res.counts, plain.counts) and res.dice == plain.dice
            final = (res.post["mask"] if chain else res.mask).cpu().numpy()
            for s, vol in enumerate((final, labels)):
                want_i, want_f, _ = RC.restate(vol, image, lo=1, L=2)
                assert np.array_equal(res.regions["rows_i"][s], want_i) and np.array_equal(bits(res.regions["rows_f"][s]), bits(want_f)), (graphed, s)
            fig = res.regions["figures"][0]
            p, t = R.derive(res.regions["rows_i"][0], res.regions["rows_f"][0], MM)[1], R.derive(res.regions["rows_i"][1], res.regions["rows_f"][1], MM)[1]
            assert fig["rvd"] == R.compare(p, t)["rvd"] and fig["unit"] == "mm" and t["voxels"] == int((labels == 1).sum()) > 0
            assert res.regions["pred"][1]["voxels"] == int((final == 1).sum())
        seg = VolumeSegmenter(net, batch=8, graphed=graphed, regions=True)
        it = torch.full((2, 2, R.IROW), FILL_I, dtype=torch.int64, device=DEV)
        ft = torch.full((2, 2, R.FROW), float("nan"), dtype=torch.float64, device=DEV)
        counts = torch.zeros((net.num_iter + 2, 1, 3), dtype=torch.int64, device=DEV)
        seg(*args, counts_out=counts, regions_out=(it, ft))                 # shapes seen, workspaces made
        it.fill_(FILL_I)
        out = seg(*args, counts_out=counts, regions_out=(it, ft))
        assert out.regions is None and torch.equal(out.mask, plain.mask)
        for s, vol in enumerate((plain.mask.cpu().numpy(), labels)):
            want_i, want_f, _ = RC.restate(vol, image, lo=1, L=2)
            assert np.array_equal(it[s].cpu().numpy(), want_i) and np.array_equal(bits(ft[s].cpu().numpy()), bits(want_f))
        # what the option adds makes no host synchronisation: every synchronising torch call raises under the debug mode
        d_labels, d_image = dev(labels, torch.int32), dev(image, torch.float32)
        it2, ft2 = torch.zeros_like(it), torch.zeros_like(ft)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            assert seg._regions(plain.mask, d_labels, d_image, 2, (it2, ft2)) is None
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.equal(it2, it) and torch.equal(ft2.view(torch.int64), ft.view(torch.int64))
        with pytest.raises(ValueError, match="regions_out needs"):
            VolumeSegmenter(net, batch=8, graphed=graphed)(*args, regions_out=(it, ft))
        with pytest.raises(ValueError, match="regions_out must be"):
            seg(*args, regions_out=(it[:1], ft))
    # without labels: the prediction's row alone
    res = VolumeSegmenter(net, batch=8, graphed=False, regions=True)(*args[:4])
    assert res.regions["figures"] is None and res.regions["truth"] is None and (res.regions["rows_i"][1] == 0).all()
    assert np.array_equal(res.regions["rows_i"][0], RC.restate(res.mask.cpu().numpy(), image, lo=1, L=2)[0])


def test_evaluate_dataset_regions_and_the_driver(tmp_path, capsys, monkeypatch):
    """evaluate_dataset(regions=True, spacing="header"): out["regions_*"] equal the per-item restatement on the kept masks, the printed
    vol / rvd / cdist fields equal derive + compare of those tables, and everything else is the run without the option; regions=False
    prints and returns what a run with the option absent does; tools/eval_driver.py --regions end to end"""
    import yaml

    from rpnet_amd import dataset_eval as DE
    from tests.helpers import load_cfg
    from tests.test_gpu_dataset_eval import _build_net, _plain
    data_dir, set_name, cfg = mm_dataset(tmp_path / "data")
    src = DE.DeviceEvalSource(data_dir, set_name, cfg, DEV)
    src.warm()
    net = _build_net(cfg, "f32")
    runs = {}
    for name, kw in (("absent", {}), ("off", dict(regions=False)), ("voxels", dict(regions=True, keep_masks=True)),
                     ("header", dict(regions=True, spacing="header", keep_masks=True, keep_largest=6))):
        random.seed(77)
        capsys.readouterr()
        tabs = {}
        dicts = _plain(DE.evaluate_dataset(net, src, cfg, batch=8, graphed=False, out=tabs, **kw))
        runs[name] = (dicts, tabs, capsys.readouterr().out.splitlines())
    (d0, t0, l0), (d1, t1, l1) = runs["absent"], runs["off"]
    assert d1 == d0 and l1 == l0 and sorted(t1) == sorted(t0) == ["counts", "ncc"] and all(t1[k].tobytes() == t0[k].tobytes() for k in t0)
    for name in ("voxels", "header"):
        d, t, lines = runs[name]
        mm = name == "header"
        assert d == d0 and t["counts"].tobytes() == t0["counts"].tobytes() and t["ncc"].tobytes() == t0["ncc"].tobytes()
        assert t["regions_i"].shape == (3, 2, 2, R.IROW) and t["regions_f"].shape == (3, 2, 2, R.FROW) and len(lines) == len(l0) == 4
        assert (t.get("spacing") == [MM] * 3) if mm else ("spacing" not in t)
        figs = []
        for j in range(3):
            c, qv = src.reader.indices[j]
            image, truth = (v.cpu().numpy() for v in src.volume(c, qv))
            for s, vol in enumerate((t["masks"][j].cpu().numpy(), truth.astype(np.int32))):
                want_i, want_f, _ = RC.restate(vol, image, lo=1, L=2)
                assert np.array_equal(t["regions_i"][j, s], want_i) and np.array_equal(bits(t["regions_f"][j, s]), bits(want_f)), (name, j, s)
            p = R.derive(t["regions_i"][j, 0], t["regions_f"][j, 0], MM if mm else None)[1]
            q = R.derive(t["regions_i"][j, 1], t["regions_f"][j, 1], MM if mm else None)[1]
            cmp_ = R.compare(p, q)
            figs.append(cmp_)
            if mm:
                tail = f" vol {p['volume_ml']:.4f} ({q['volume_ml']:.4f}) ml rvd {cmp_['rvd']:.4f} cdist {cmp_['centroid_distance']:.4f} mm"
                assert lines[j].startswith(l0[j]) and " lcc " in lines[j]
            else:
                tail = f" vol {p['voxels']} ({q['voxels']}) rvd {cmp_['rvd']:.4f} cdist {cmp_['centroid_distance']:.4f}"
                assert lines[j] == l0[j] + tail
            assert lines[j].endswith(tail) and cmp_["rvd"] is not None and cmp_["centroid_distance"] is not None, (lines[j], tail)
        mean_rvd, mean_cd = np.mean([f["rvd"] for f in figs]), np.mean([f["centroid_distance"] for f in figs])
        assert lines[3].startswith(l0[3]) and lines[3].endswith(f" rvd {mean_rvd:.4f} cdist {mean_cd:.4f}" + (" mm" if mm else "")) and " vol " in lines[3]
    with pytest.raises(ValueError, match="give surface=True"):
        DE.evaluate_dataset(net, src, cfg, batch=8, graphed=False, spacing="header")
    # the driver
    from tools import eval_driver
    y = dict(load_cfg(), **cfg)
    y.update(data_dir=data_dir, eval_set_name=set_name)
    path = str(tmp_path / "regions.yml")
    with open(path, "w") as fh:
        yaml.safe_dump(json.loads(json.dumps(y)), fh)
    monkeypatch.setattr(sys, "argv", ["eval_driver.py", "--yaml", path, "--device-items", "--items", "2", "--regions"])
    random.seed(8)
    capsys.readouterr()
    eval_driver.main()
    text = capsys.readouterr().out.splitlines()
    assert len(text) == 3 and all(" vol " in l and " rvd " in l and " cdist " in l and " ml " not in l for l in text)
    monkeypatch.setattr(sys, "argv", ["eval_driver.py", "--yaml", path, "--regions"])
    with pytest.raises(SystemExit):
        eval_driver.main()
