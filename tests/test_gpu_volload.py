"""The volume-loading entry points (csrc/volload.hip, include/rpnet_volload_abi.h), rpnet_amd.volume_load and the device_load options on
the MI355X.

Every comparison is exact equality with tests/volload_cases.py (numpy: the definitions of the header operation by operation; pinned to
FewshotVolumeReader.load_image_and_mask and numpy.percentile by tests/test_host_volload.py), bit for bit; a NaN is compared as a NaN, and
a zero the selection returns by its value.  There is no tolerance."""
import os
import random

import numpy as np
import pytest
import torch

from rpnet_amd import hip
from rpnet_amd import volume_load as VL
from rpnet_amd.utils import volume_reader as VR
from tests import volload_cases as VC
from tests.test_host_volload import bare_reader, write_pair

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
NP_KIND = {np.dtype(np.float32): 0, np.dtype(np.int16): 1, np.dtype(np.uint8): 2}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def file_order(a):
    """[D,H,W] array -> the device view of its file payload (z fastest), as DeviceVolumeLoader uploads it"""
    return VL.upload_payload(np.ascontiguousarray(a.reshape(-1, order="F")), a.shape, DEV)


def select_raw(x_dev, n, ranks, ptr=None):
    """rpnet_volload_select through the C ABI: stats and a workspace of exactly the size asked for, guard words behind both"""
    need = hip.query("rpnet_volload_select_workspace_bytes", n)
    assert need == 64 + 4 * 2 * 256 * 4
    ws = torch.full((need + 64,), 0xA5, device=DEV, dtype=torch.uint8)
    stats = torch.full((8,), -7, device=DEV, dtype=torch.int32)
    hip.call("rpnet_volload_select", hip.ptr(x_dev) if ptr is None else ptr, n, ranks[0], ranks[1], hip.ptr(stats), hip.ptr(ws), need)
    torch.cuda.synchronize()
    assert (ws[need:] == 0xA5).all() and (stats[4:] == -7).all() and stats[3] == 0
    return stats[:2].view(torch.float32).cpu().numpy(), int(stats[2])


def check_select(x, what):
    n = x.size
    k0, k1, g = VL.percentile_rank(n, 99.5)
    assert (k0, k1, g) == VC.ref_rank(n)
    a, b, n_nan = VC.ref_select(x, (k0, k1))
    xd = dev(x)
    for _ in range(2):                                                   # every call twice with equal bits
        got, nan = select_raw(xd, n, (k0, k1))
        assert VC.same_bits_nan(got, np.array([a, b], F)) and nan == n_nan, (what, got, a, b)
    s = np.sort(x)
    assert VC.same_bits_nan(got, np.array([s[k0], s[k1]], F), zeros_by_value=True), what
    st = VL.order_statistics(xd, (k0, k1))
    assert VC.same_bits_nan(st[:2].view(torch.float32).cpu().numpy(), got) and int(st[2]) == n_nan
    with np.errstate(invalid="ignore"):
        want = np.percentile(x, 99.5)
    assert VC.same_bits_nan(VL.percentile_f32(xd, 99.5).cpu().numpy(), want, zeros_by_value=True), what
    assert VC.same_bits_nan(VL.percentile_f32(xd, 99.5).cpu().numpy(), VC.ref_percentile(x)), what


def test_selection_cases_equal_the_restatement_and_numpy():
    """n = 1, 2, 200, 201, 202; all equal; ties across the rank; values that differ in the lowest digit only; negative and mixed data;
    zeros of both signs; subnormals; infinities at the rank (the lerp makes numpy's NaN); one NaN, of either sign; a CT-like volume that
    is 60 % -1024.  rpnet_volload_select, order_statistics and percentile_f32 against the restatement and numpy.percentile"""
    cases = VC.selection_cases()
    assert {"n1", "n2", "n200", "n201", "n202", "all_equal", "ties_straddle", "lowest_digit", "negative", "mixed", "zeros", "subnormals",
            "pos_inf_at_rank", "neg_inf_at_rank", "inf_next", "one_nan", "negative_nan", "ct_like"} <= set(cases)
    assert [VC.ref_rank(n)[:2] for n in (1, 2, 200, 201, 202)] == [(0, 0), (0, 1), (198, 199), (199, 200), (199, 200)]
    assert (cases["ct_like"] == -1024).mean() > 0.55
    with np.errstate(invalid="ignore"):
        assert np.isnan(np.percentile(cases["pos_inf_at_rank"], 99.5)) and np.isnan(np.percentile(cases["one_nan"], 99.5))
    for name, x in cases.items():
        check_select(x, name)
    # any two ranks, not only neighbours: the ranks part in the first digit
    x = cases["mixed"]
    got, _ = select_raw(dev(x), x.size, (3, 1000))
    assert VC.same_bits_nan(got, np.sort(x)[[3, 1000]])


def test_selection_past_one_sweep_unaligned_and_ragged():
    """n one value past one full sweep of the counting pass (1024 blocks * 256 lanes * 4 values: 4 MiB), so the last block strides a second
    time for one value; a pointer 16 bytes and one 4 bytes into an allocation; n not a multiple of 4"""
    n = VL.SELECT_SWEEP + 1
    assert VL.SELECT_SWEEP == 1024 * 256 * 4
    gen = torch.Generator(device=DEV).manual_seed(3)
    big = torch.randn(n + 8, device=DEV, generator=gen) * 300
    big[n + 3] = 1e9                                                     # the one value of the second stride is the largest
    k0, k1, _ = VL.percentile_rank(n, 99.5)
    for off in (4, 1):
        x = big[off:off + n]
        assert x.data_ptr() % 16 == (16 * (off == 4) + 4 * (off == 1)) % 16
        s = torch.sort(x).values
        for ranks in ((k0, k1), (n - 2, n - 1)):
            got, nan = select_raw(x, n, ranks)
            assert VC.same_bits_nan(got, s[list(ranks)].cpu().numpy()) and nan == 0, (off, ranks)
    assert float(big[4:4 + n].max()) == 1e9
    for m in (5, 1023, 4097):
        x = (torch.randn(m + 1, device=DEV, generator=gen) * 50)[1:]
        check_select(x.cpu().numpy(), f"ragged {m}")


@pytest.mark.parametrize("bounds", [(-1024, 3072), (0.25, 0.75), (0.1, 2.3), (-1024, 3076)], ids=str)
def test_clip_and_map_equals_the_restatement(bounds):
    """HU_range [-1024, 3072]; a range below 1 (the max(1, .) branch); bounds float32 does not hold; values exactly at top, minimum and
    maximum; in place and out=; outputs prefilled with NaN, guard words behind them; twice with equal bits"""
    mn, mx = bounds
    rs = np.random.RandomState(8)
    x = (rs.normal((mn + mx) / 2, (mx - mn), 4099)).astype(F)
    tie = F(np.sort(x)[-41])                                             # the top 40 values and one more are one value: the percentile
    x[np.argsort(x)[-40:]] = tie
    x[:5] = [F(mn), F(mx), np.nextafter(F(mn), F(-np.inf)), np.nextafter(F(mx), F(np.inf)), np.nextafter(F(mn), F(np.inf))]
    top = VC.ref_percentile(x)
    assert top == tie and (x == top).sum() >= 30 and (x == F(mn)).any() and (x == F(mx)).any()
    want = VC.ref_normalize(x, mn, mx)
    assert VC.bits(want).tobytes() == VC.bits(VR.normalize(x, mn, mx)).tobytes()
    if mx - mn < 1:
        assert want.max() < 1
    xd = dev(x)
    buf = torch.full((x.size + 16,), float("nan"), device=DEV)
    out = buf[:x.size]
    for _ in range(2):
        buf.fill_(float("nan"))
        assert VL.window_normalize(xd, mn, mx, out=out) is out
        assert VC.same_bits_nan(out.cpu().numpy(), want) and torch.isnan(buf[x.size:]).all()
    assert VC.same_bits_nan(VL.window_normalize(xd, mn, mx).cpu().numpy(), want) and VC.same_bits_nan(xd.cpu().numpy(), x)
    inplace = xd.clone()
    assert VL.window_normalize(inplace, mn, mx, out=inplace) is inplace and VC.same_bits_nan(inplace.cpu().numpy(), want)
    # a NaN in the volume: numpy's percentile is a NaN and clips nothing; the NaN voxel stays one
    x[77] = np.nan
    with np.errstate(invalid="ignore"):
        want = VR.normalize(x, mn, mx)
    assert VC.same_bits_nan(VC.ref_normalize(x, mn, mx), want) and VC.same_bits_nan(VL.window_normalize(dev(x), mn, mx).cpu().numpy(), want)
    # an unaligned, ragged view
    y = dev(x[:1001])[1:]
    assert VC.same_bits_nan(VL.window_normalize(y, mn, mx, out=y).cpu().numpy(), VC.ref_normalize(x[1:1001], mn, mx))


def test_graph_of_window_normalize_replayed_with_new_input():
    """the select + clip pair captured with torch.cuda.graph and replayed twice, the input rewritten in between"""
    rs = np.random.RandomState(12)
    a, b = (VC.file_volume((6, 40, 40), np.float32, s).ravel() for s in (1, 2))
    x = dev(a)
    out = torch.empty_like(x)
    VL.window_normalize(x, *VC.HU, out=out)                              # the workspace exists before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        VL.window_normalize(x, *VC.HU, out=out)
    for src in (a, b, a):
        x.copy_(dev(src))
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert VC.same_bits_nan(out.cpu().numpy(), VC.ref_normalize(src, *VC.HU))
    assert rs is not None and not VC.same_bits_nan(VC.ref_normalize(a, *VC.HU), VC.ref_normalize(b, *VC.HU))


@pytest.mark.parametrize("row", VC.GEOMETRY_ROWS, ids=lambda r: "%s-%s-%s" % r)
def test_gather_and_range_equal_the_restatement(row):
    """file shapes (1,1,1), (17,33,31), (22,44,40), (16,300,280) under crop_size [32,32], [256,256] and the odd [33,47]: crop and pad on
    each axis, both pad parities, num_slice / num_y / num_x below and above the extents; annotations in the first slice, the last slice,
    a single slice, and two slices (depth 1); every image and mask kind, both source orders; a float mask with fractional values passes
    through; outputs prefilled with NaN with a guard behind them; every call twice"""
    shape, window, crop = row
    cfg = VC.config(window, crop)
    geom = VL.load_geometry(cfg, shape)
    g = VC.ref_geometry(shape, window, crop)
    nz = g["nz"]
    spans = [(0, 0)] if nz == 1 else [(0, nz - 1), (nz // 2, nz // 2), (0, 1), (nz - 2, nz - 1)]
    for j, (zf, zl) in enumerate(spans):
        for mk in (np.uint8, np.int16, np.float32):
            mask = VC.file_mask(shape, mk, zf, zl, seed=j)
            if mk is np.float32:
                mask[zf, 0, 0] = np.nan if shape != (1, 1, 1) else mask[zf, 0, 0]      # outside or inside the window: the restatement decides
            want = VC.ref_range(mask, g)
            for src in (dev(mask), file_order(mask)):
                row_buf = torch.full((8,), -9, device=DEV, dtype=torch.int32)
                for _ in range(2):
                    hip.call("rpnet_volload_range", hip.ptr(src), NP_KIND[mask.dtype], int(not src.is_contiguous()), *shape, *window, hip.ptr(row_buf))
                    assert tuple(row_buf[:4].tolist()) == want and (row_buf[4:] == -9).all(), (row, j, mk)
                assert tuple(VL.annotated_range(src, geom).tolist()) == want
            lo, hi = (zf, zl) if zl > zf else (zf, zf + 1)
            n = (hi - lo) * crop[0] * crop[1]
            buf = torch.full((n + 16,), float("nan"), device=DEV)
            out = buf[:n].view(hi - lo, *crop)
            for src in (dev(mask), file_order(mask)):
                buf.fill_(float("nan"))
                assert VL.gather_volume(src, geom, lo, hi, 0.0, out=out) is out
                assert VC.same_bits_nan(out.cpu().numpy(), VC.ref_gather(mask, g, lo, hi, 0.0)) and torch.isnan(buf[n:]).all(), (row, j, mk)
            if mk is np.float32 and zl > zf:
                got = out.cpu().numpy()
                assert ((got > 0) & (got < 1)).any()
        for ik in (np.int16, np.float32):
            image = VC.file_volume(shape, ik, seed=j)
            want = VC.ref_gather(image, g, lo, hi, -1024)
            for src in (dev(image), file_order(image)):
                a = VL.gather_volume(src, geom, lo, hi, -1024).cpu().numpy()
                b = VL.gather_volume(src, geom, lo, hi, -1024).cpu().numpy()
                assert VC.same_bits_nan(a, want) and a.tobytes() == b.tobytes(), (row, j, ik)
    empty = np.zeros(shape, np.uint8)
    assert tuple(VL.annotated_range(dev(empty), geom).tolist()) == (-1, -1, 0, 0)


def test_refusals_launch_nothing():
    """every refusal of include/rpnet_volload_abi.h returns its status with a message; the Python layer and DeviceVolumeLoader refuse what
    the kernels do not serve and name the host reader"""
    shape, window = (6, 20, 24), (6, 20, 24)
    mask, img = dev(VC.file_mask(shape, np.uint8, 1, 4)), dev(VC.file_volume(shape, np.int16))
    row = torch.full((4,), -9, device=DEV, dtype=torch.int32)
    out = torch.full((3, 16, 16), 7.0, device=DEV)
    x = torch.randn(100, device=DEV)
    p = hip.ptr

    def rng(src=p(mask), kind=2, layout=0, dims=shape, win=window, dst=p(row)):
        hip.call("rpnet_volload_range", src, kind, layout, *dims, *win, dst)

    def gat(src=p(img), kind=1, layout=0, dims=shape, win=window, lo=1, hi=4, crop=(16, 16), dst=p(out)):
        hip.call("rpnet_volload_gather", src, kind, layout, *dims, *win, lo, hi, *crop, -1024.0, dst)

    for fn, name in ((rng, "volload_range"), (gat, "volload_gather")):
        for null in ("src", "dst"):
            with pytest.raises(RuntimeError, match=f"{name}: null pointer"):
                fn(**{null: None})
        for kind in (-1, 3):
            with pytest.raises(RuntimeError, match=f"element kind {kind} "):
                fn(kind=kind)
        with pytest.raises(RuntimeError, match="layout 2 "):
            fn(layout=2)
        for dims in ((0, 20, 24), (6, 1025, 24), (6, 20, -1)):
            with pytest.raises(RuntimeError, match="every extent 1..1024"):
                fn(dims=dims)
        with pytest.raises(RuntimeError, match="each at least 1"):
            fn(win=(0, 20, 24))
        with pytest.raises(RuntimeError, match="is empty"):
            fn(win=(6, 1, 24))
    with pytest.raises(RuntimeError, match="aligned to its element"):
        gat(src=p(img) + 1)
    with pytest.raises(RuntimeError, match="row must be aligned to 16"):
        rng(dst=p(row) + 4)
    for lo, hi in ((-1, 3), (3, 3), (4, 3), (0, 7)):
        with pytest.raises(RuntimeError, match="0 <= lo < hi <= 6"):
            gat(lo=lo, hi=hi)
    for crop in ((0, 16), (16, 1025)):
        with pytest.raises(RuntimeError, match="each 1..1024"):
            gat(crop=crop)
    with pytest.raises(RuntimeError, match="out must be aligned to 4"):
        gat(dst=p(out) + 2)
    need = hip.query("rpnet_volload_select_workspace_bytes", 100)
    ws, st = torch.zeros(need + 16, device=DEV, dtype=torch.uint8), torch.full((4,), -9, device=DEV, dtype=torch.int32)

    def sel(src=p(x), n=100, k0=3, k1=4, stats=p(st), work=p(ws), nbytes=need):
        hip.call("rpnet_volload_select", src, n, k0, k1, stats, work, nbytes)

    def nrm(src=p(x), dst=p(x), n=100, stats=p(st), g=0.5, mn=0.0, mx=1.0, den=1.0):
        hip.call("rpnet_volload_normalize", src, dst, n, stats, g, mn, mx, den)

    for null in ("src", "stats", "work"):
        with pytest.raises(RuntimeError, match="volload_select: null pointer"):
            sel(**{null: None})
    for n in (0, (1 << 30) + 1):
        with pytest.raises(RuntimeError, match="1..1073741824 values"):
            sel(n=n)
        assert hip.query("rpnet_volload_select_workspace_bytes", n) == 0
        assert hip.load().rpnet_last_error_string().decode().startswith(f"volload_select: n={n} ")
    for k0, k1 in ((5, 4), (3, 100)):
        with pytest.raises(RuntimeError, match="k0 <= k1 <= n - 1"):
            sel(k0=k0, k1=k1)
    with pytest.raises(RuntimeError, match=f"workspace of {need - 1} bytes, {need} needed"):
        sel(nbytes=need - 1)
    for bad in (dict(src=p(x) + 2), dict(stats=p(st) + 4), dict(work=p(ws) + 8)):
        with pytest.raises(RuntimeError, match="aligned to 4 bytes, stats and the workspace to 16"):
            sel(**bad)
    for null in ("src", "dst", "stats"):
        with pytest.raises(RuntimeError, match="volload_normalize: null pointer"):
            nrm(**{null: None})
    with pytest.raises(RuntimeError, match="1..1073741824 values"):
        nrm(n=0)
    with pytest.raises(RuntimeError, match="aligned to 4 bytes, stats to 16"):
        nrm(dst=p(x) + 2)
    with pytest.raises(RuntimeError, match="partly overlaps"):
        nrm(dst=p(x) + 8, n=50)
    for bad in (dict(mn=2.0), dict(den=0.5), dict(g=1.0), dict(g=-0.1), dict(g=float("nan")), dict(mx=float("nan"))):
        with pytest.raises(RuntimeError, match="minimum <= maximum, denominator >= 1, 0 <= g < 1"):
            nrm(**bad)
    torch.cuda.synchronize()
    assert (row == -9).all() and (out == 7).all() and (st == -9).all() and (ws == 0).all()
    # the Python layer
    geom = VL.load_geometry(VC.config(window, [16, 16]), shape)
    with pytest.raises(ValueError, match="are accepted .*load_image_and_mask"):
        VL.annotated_range(mask.double(), geom)
    with pytest.raises(ValueError, match="must be contiguous, or the transposed view"):
        VL.annotated_range(mask.transpose(1, 2), VL.load_geometry(VC.config(window, [16, 16]), (6, 24, 20)))
    with pytest.raises(ValueError, match="not the file shape"):
        VL.gather_volume(img[:5], geom, 1, 3)
    with pytest.raises(ValueError, match="0 <= lo < hi <= 6"):
        VL.gather_volume(img, geom, 3, 3)
    with pytest.raises(RuntimeError, match="MI355X only"):
        VL.window_normalize(x.cpu(), 0, 1)
    with pytest.raises(ValueError, match="contiguous float32 tensor"):
        VL.window_normalize(x.double(), 0, 1)
    with pytest.raises(ValueError, match="out must be a contiguous float32 tensor of shape"):
        VL.window_normalize(x, 0, 1, out=x[:50])
    with pytest.raises(ValueError, match="finite and ordered"):
        VL.window_normalize(x, 2, 1)
    with pytest.raises(ValueError, match="0 <= k0 <= k1 <= n - 1"):
        VL.order_statistics(x, (5, 100))


def test_loader_refusals_name_the_host_reader(tmp_path):
    shape, window = (8, 20, 24), (8, 20, 24)
    image, mask = VC.file_volume(shape, np.int16), VC.file_mask(shape, np.uint8, 2, 5)
    loader = VL.DeviceVolumeLoader(bare_reader(tmp_path, VC.config(window, [16, 16])), DEV)
    flat = lambda a: np.ascontiguousarray(a.reshape(-1, order="F"))  # noqa: E731
    ok = loader.load_arrays(flat(image), flat(mask), shape, shape)
    assert ok[0].shape == ok[1].shape == (3, 16, 16)
    with pytest.raises(ValueError, match="the image is int32.*load_image_and_mask"):
        loader.load_arrays(flat(image.astype(np.int32)), flat(mask), shape, shape)
    with pytest.raises(ValueError, match="the mask is int64.*load_image_and_mask"):
        loader.load_arrays(flat(image), flat(mask.astype(np.int64)), shape, shape)
    with pytest.raises(ValueError, match="the mask is empty.*load_image_and_mask"):
        loader.load_arrays(flat(image), flat(mask * 0), shape, shape)
    with pytest.raises(ValueError, match="one annotated slice.*load_image_and_mask"):
        loader.load_arrays(flat(image), flat(VC.file_mask(shape, np.uint8, 3, 3)), shape, shape)
    for pad in (-1024.5, 40000):
        loader.reader.cfg = VC.config(window, [16, 16], pad_value=pad)
        with pytest.raises(ValueError, match="pad_value .* is not held exactly.*load_image_and_mask"):
            loader.load_arrays(flat(image), flat(mask), shape, shape)
    loader.reader.cfg = VC.config(window, [16, 16], pad_value=0.1)
    with pytest.raises(ValueError, match="pad_value 0.1 is not held exactly.*load_image_and_mask"):
        loader.load_arrays(flat(image.astype(np.float32)), flat(mask), shape, shape)


# ---------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("kinds", [(np.int16, np.uint8), (np.float32, np.float32)], ids=lambda k: k[0].__name__)
def test_loader_equals_the_host_reader(tmp_path, kinds):
    """DeviceVolumeLoader.load against FewshotVolumeReader.load_image_and_mask, bit for bit: a write_synthetic_dataset data set, and files
    of every geometry row with a real depth"""
    data_dir, _, _ = VR.write_synthetic_dataset(str(tmp_path / "syn"), n_volumes=2, shape=(22, 72, 72), seed=11)
    rows = [((22, 72, 72), (20, 72, 72), [64, 64], data_dir, ("case000", "case001"))]
    for j, (shape, window, crop) in enumerate(VC.GEOMETRY_ROWS[3:]):
        d = str(tmp_path / f"row{j}")
        nz = min(shape[0], window[0])
        write_pair(d, "p", VC.file_volume(shape, kinds[0], j), VC.file_mask(shape, kinds[1], 1, nz - 1, j))
        rows.append((shape, window, crop, d, ("p",)))
    for shape, window, crop, d, pids in rows if kinds[0] is np.int16 else rows[1:]:
        rd = bare_reader(d, VC.config(window, crop))
        loader = VL.DeviceVolumeLoader(rd, DEV)
        for pid in pids:
            want = rd.load_image_and_mask(pid, "Liver")
            image, mask = loader.load(pid, "Liver")
            assert image.dtype == mask.dtype == torch.float32 and image.is_cuda and loader.last_read_seconds > 0
            assert tuple(image.shape) == want["image"][0].shape == tuple(mask.shape)
            assert VC.bits(image.cpu().numpy()).tobytes() == VC.bits(want["image"][0]).tobytes(), (shape, window, crop, pid)
            assert VC.bits(mask.cpu().numpy()).tobytes() == VC.bits(want["mask"][0]).tobytes(), (shape, window, crop, pid)


def test_episode_items_are_the_same_with_device_load(tmp_path):
    """DeviceEpisodeSource(device_load=True).item equals the device_load=False item bit for bit under equal seeds, cache_volumes off"""
    from rpnet_amd.episodes import DeviceEpisodeSource
    from tests import augment_cases as AC
    from tests.test_gpu_augment import _dataset
    data_dir, set_name, cfg = _dataset(tmp_path, do_elastic=True, do_deformable=False)
    items = []
    for on in (False, True):
        src = DeviceEpisodeSource(data_dir, set_name, cfg, DEV, cache_volumes=False, elastic_random_state=np.random.RandomState(5), device_load=on)
        assert (src.loader is not None) == on
        got = []
        for idx in range(3):
            AC.seed_all(60 + idx)
            got.append(src.item(idx))
        items.append(got)
    for a, b in zip(*items):
        assert a["pid"] == b["pid"] and a["supp_pids"] == b["supp_pids"]
        for key in DeviceEpisodeSource.FIELDS:
            assert torch.equal(a[key], b[key]), key
        assert torch.equal(a["registration_field"], b["registration_field"])


def test_dataset_evaluation_and_drivers_with_device_load(tmp_path, capsys, monkeypatch):
    """evaluate_dataset(device_load=True) gives the tables and lines of device_load=False; train_rpnet.train runs on a source built as
    --device_load builds it; both drivers know their flag and refuse it without what it needs"""
    import sys
    from rpnet_amd import dataset_eval as DE
    from tests.test_gpu_dataset_eval import _build_net, _dataset, _driver_lines, _eval_cfg, _plain
    data_dir, set_name, cfg = _dataset(tmp_path / "data", do_deformable=False)
    cfg = _eval_cfg(cfg)
    results = []
    for on in (False, True):
        src = DE.DeviceEvalSource(data_dir, set_name, cfg, DEV, cache_volumes=False)
        tables = {}
        random.seed(77)
        capsys.readouterr()
        dicts = _plain(DE.evaluate_dataset(_build_net(cfg, "f32"), src, cfg, batch=8, graphed=False, out=tables, device_load=on))
        assert (src.loader is not None) == on
        results.append((dicts, tables, _driver_lines(capsys.readouterr().out)))
    (d0, t0, l0), (d1, t1, l1) = results
    assert d0 == d1 and l0 == l1 and len(l0) == 4
    assert np.array_equal(t0["counts"], t1["counts"]) and t0["ncc"].tobytes() == t1["ncc"].tobytes()
    assert DE.DeviceEvalSource(data_dir, set_name, cfg, DEV, device_load=True).loader is not None

    from rpnet_amd.episodes import DeviceEpisodeSource
    from tests.test_gpu_augment import _dataset as train_dataset
    import train_rpnet
    from tools import eval_driver
    tdir, tset, tcfg = train_dataset(tmp_path / "train", do_elastic=False, do_deformable=False)
    from tests.helpers import load_cfg
    source = DeviceEpisodeSource(tdir, tset, tcfg, torch.device(DEV), cache_volumes=False, device_load=True)
    _, hist = train_rpnet.train(dict(load_cfg(2), **tcfg), steps=2, batch=4, size=64, dev=torch.device(DEV), lr=1e-3, log_every=0, source=source)
    assert len(hist) == 2 and all(np.isfinite(hist))
    capsys.readouterr()
    assert eval_driver.build_parser().parse_args(["--device-items", "--device-load"]).device_load is True
    monkeypatch.setattr(sys, "argv", ["eval_driver.py", "--device-load"])
    with pytest.raises(SystemExit, match="--device-load needs --device-items"):
        eval_driver.main()
    monkeypatch.setattr(sys, "argv", ["train_rpnet.py", "--device_load"])
    with pytest.raises(SystemExit):
        train_rpnet.main()
    assert "--device_load needs --data_dir" in capsys.readouterr().err
