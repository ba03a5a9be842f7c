"""rpnet_resample_image and rpnet_resample_labels (csrc/resample.hip), rpnet_amd.resample and tools/preprocess_volumes.py --resample on
the MI355X.

Every comparison is exact equality with tests/resample_cases.py (numpy: the definitions of include/rpnet_resample_abi.h operation by
operation; pinned to scipy.ndimage.zoom by tests/test_host_resample.py): images bit for bit, label maps and statistics rows equal.
There is no tolerance."""
import os

import numpy as np
import pytest
import torch

from rpnet_amd import hip
from rpnet_amd import resample as RS
from tests import resample_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 7
DTYPES = (np.float32, np.int16)


def dev(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(DEV)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_bits_or_both_nan(a, b):
    """same_bits, except that a NaN matches a NaN: IEEE 754 leaves the sign and payload of a NaN that an operation makes (inf - inf) to
    the processor, and the host and the device choose differently; everything that is not a NaN is compared bit for bit"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    keep = ~np.isnan(a)
    return a[keep].tobytes() == b[keep].tobytes()


def check_image(img, shape, what, same_bits=same_bits):
    """both orders and both alignments of one image == the restatement, bit for bit; the input untouched"""
    src = dev(img)
    for align in RC.ALIGNS:
        for order in (1, 0):
            got = RS.resample_image(src, shape, order=order, align=align)
            want = RC.ref_image(img, shape, order, align)
            res = got.cpu().numpy()
            assert same_bits(res, want), (what, align, order, int((res.view(np.uint8) != want.view(np.uint8)).sum()))
    assert same_bits(src.cpu().numpy(), img), what


@pytest.mark.parametrize("shapes", RC.SMALL)
def test_small_grids_equal_the_restatement(shapes):
    """one voxel to one voxel, 1 -> 5, 5 -> 1, each axis of length 1 in turn, the identity, 5x7x9 -> 8x5x13 and back; both alignments,
    both orders, both image kinds"""
    shape_in, shape_out = shapes
    assert hip.query("rpnet_resample_workspace_bytes", *shape_in, *shape_out) == 64 + 16 * sum(shape_out)
    for dtype in DTYPES:
        img = RC.noise_image(shape_in, dtype, seed=1)
        check_image(img, shape_out, f"{shape_in} -> {shape_out} {dtype.__name__}")
        if shape_in == shape_out:
            for align in RC.ALIGNS:
                assert same_bits(RS.resample_image(dev(img), shape_out, align=align).cpu().numpy(), img)


@pytest.mark.parametrize("dtype", DTYPES + (np.uint8,))
def test_lane_runs_and_unaligned_rows(dtype):
    """output rows of one lane run + 1 and of two runs + 2 voxels, and rows whose first address is not 16-byte aligned, in every kind"""
    for shape_in, shape_out in RC.run_shapes(dtype):
        r = RC.RUN[np.dtype(dtype)]
        assert RS.RUN[getattr(torch, np.dtype(dtype).name)] == r
        assert any((row * shape_out[2] * np.dtype(dtype).itemsize) % 16 for row in range(shape_out[0] * shape_out[1]))
        if dtype is np.uint8:
            check_labels(RC.label_map(shape_in), shape_out, f"{shape_in} -> {shape_out}")
        else:
            check_image(RC.noise_image(shape_in, dtype, seed=2), shape_out, f"{shape_in} -> {shape_out} {dtype.__name__}")


@pytest.mark.parametrize("shapes", RC.LINES)
def test_a_line_of_1024_along_each_axis(shapes):
    shape_in, shape_out = shapes
    for dtype in DTYPES:
        check_image(RC.noise_image(shape_in, dtype, seed=3), shape_out, f"{shape_in} -> {shape_out} {dtype.__name__}")
    check_labels(RC.label_map(shape_in), shape_out, f"{shape_in} -> {shape_out}", aligns=("center",))


def test_ties_saturation_and_non_finite_neighbours():
    """2 -> 3 under corner has c = 0.5: the int16 half-even tie (0, 1) -> 0 and (1, 2) -> 2, the ends of the int16 range, the nearest
    tie, an indicator of exactly 0.5 left out; NaN and inf beside a tap of weight zero; the identity with non-finite voxels"""
    pair = lambda a, b, dtype: np.array([a, b], dtype).reshape(1, 1, 2)  # noqa: E731
    run = lambda img, **kw: RS.resample_image(dev(img), (1, 1, 3), **kw).cpu().numpy()[0, 0].tolist()  # noqa: E731
    assert run(pair(0, 1, np.int16)) == [0, 0, 1] and run(pair(1, 2, np.int16)) == [1, 2, 2]
    assert run(pair(-1, 0, np.int16)) == [-1, 0, 0] and run(pair(-2, -1, np.int16)) == [-2, -2, -1]
    assert run(pair(-32768, 32767, np.int16)) == [-32768, 0, 32767] and run(pair(32767, 32767, np.int16)) == [32767] * 3
    assert run(pair(-32768, -32768, np.int16)) == [-32768] * 3 and run(pair(32766, 32767, np.int16)) == [32766, 32766, 32767]
    assert run(pair(10, 20, np.int16), order=0) == [10, 20, 20] and run(pair(1.5, 2.5, np.float32), order=0) == [1.5, 2.5, 2.5]
    lab = np.array([3, 0], np.uint8).reshape(1, 1, 2)
    out, stats = RS.resample_labels(dev(lab), (1, 1, 3), (3,), mode="linear")
    assert out.cpu().numpy()[0, 0].tolist() == [3, 0, 0] and stats.cpu().numpy().tolist() == [[1, 1, 3, 0]]
    out, _ = RS.resample_labels(dev(lab[:, :, ::-1]), (1, 1, 3), (3,), mode="linear")
    assert out.cpu().numpy()[0, 0].tolist() == [0, 0, 3]
    for bad in (np.inf, -np.inf, np.nan):
        line = np.array([1.0, bad, 2.0], np.float32).reshape(1, 1, 3)
        for shape_in in ((1, 1, 3), (1, 3, 1), (3, 1, 1)):
            img = line.reshape(shape_in)
            shape_out = tuple(5 if s == 3 else 1 for s in shape_in)
            got = RS.resample_image(dev(img), shape_out).cpu().numpy()
            assert same_bits_or_both_nan(got, RC.ref_image(img, shape_out, 1, "corner")) and got.flat[0] == 1.0 and got.flat[4] == 2.0
            assert not np.isfinite(got.flat[1:4]).any()
    v = RC.noise_image((4, 5, 6), np.float32)
    v[0, 0, 0], v[1, 2, 3], v[3, 4, 5], v[2, 2, 2] = np.nan, np.inf, -np.inf, -0.0
    for align in RC.ALIGNS:
        for order in (0, 1):
            assert same_bits(RS.resample_image(dev(v), v.shape, order=order, align=align).cpu().numpy(), v)
        check_image(v, (7, 5, 9), "non-finite voxels", same_bits_or_both_nan)


def check_labels(lab, shape, what, classes=(1, 2, 5), aligns=RC.ALIGNS):
    src = dev(lab)
    for align in aligns:
        for mode in ("nearest", "linear"):
            for order in (classes, classes[::-1]):
                out = torch.full(shape, FILL, device=DEV, dtype=torch.uint8)
                stats = torch.full((len(order), RS.STATS_ROW), FILL, device=DEV, dtype=torch.int64)
                got = RS.resample_labels(src, shape, order, mode=mode, align=align, out=out, stats=stats)
                want, rows = RC.ref_labels(lab, shape, order, mode, align)
                assert got[0] is out and got[1] is stats
                res = out.cpu().numpy()
                assert np.array_equal(res, want), (what, align, mode, order, int((res != want).sum()))
                assert stats.cpu().numpy().tolist() == rows.tolist(), (what, align, mode, order, stats.cpu().numpy().tolist(), rows.tolist())
        plain, none = RS.resample_labels(src, shape, align=align)
        assert none is None and np.array_equal(plain.cpu().numpy(), RC.ref_labels(lab, shape, None, "nearest", align)[0]), (what, align)
    assert np.array_equal(src.cpu().numpy(), lab), what


def test_label_maps_with_three_classes():
    """both modes, both class orders, the statistics rows; merge over what the output held: only voxels that hold 0 are taken"""
    lab = RC.label_map((6, 8, 10), seed=1)
    for shape in ((9, 5, 13), (3, 11, 37), (6, 8, 10)):
        check_labels(lab, shape, f"(6, 8, 10) -> {shape}")
    shape = (9, 5, 13)
    held = RC.ref_labels(RC.label_map((6, 8, 10), seed=2), shape, None, "nearest", "center")[0]
    out = dev(held)
    got, stats = RS.resample_labels(dev(lab), shape, (1, 2, 5), mode="linear", align="center", out=out, merge=True)
    want, rows = RC.ref_labels(lab, shape, (1, 2, 5), "linear", "center", into=held)
    res = got.cpu().numpy()
    assert got is out and np.array_equal(res, want) and stats.cpu().numpy().tolist() == rows.tolist()
    assert np.array_equal(res[held != 0], held[held != 0]) and (res[held == 0] != 0).any()
    with pytest.raises(ValueError, match="merge lays the classes over"):
        RS.resample_labels(dev(lab), shape, (1,), mode="linear", merge=True)


def test_guard_words_out_given_and_graph_replay():
    """calls through the C ABI with a workspace of exactly the size asked for and guard bytes behind it and behind the outputs; a second
    identical call gives the same bits; resample_to_spacing captured with torch.cuda.graph and replayed twice gives identical bits, equal
    to the eager call and to the restatement"""
    shape_in, shape_out = (6, 21, 33), (9, 13, 41)
    n_out = int(np.prod(shape_out))
    img, lab = RC.noise_image(shape_in, np.float32, seed=4), RC.label_map(shape_in, seed=4)
    src, m_in = dev(img), dev(lab)
    p = hip.ptr
    need = hip.query("rpnet_resample_workspace_bytes", *shape_in, *shape_out)
    assert need == 64 + 16 * sum(shape_out)
    ws = torch.full((need + 64,), 0xA5, device=DEV, dtype=torch.uint8)
    outf = torch.full((n_out + 16,), float(FILL), device=DEV, dtype=torch.float32)
    out8 = torch.full((n_out + 64,), FILL, device=DEV, dtype=torch.uint8)
    stats = torch.full((3, 4), FILL, device=DEV, dtype=torch.int64)

    def calls():
        hip.call("rpnet_resample_image", p(src), 0, *shape_in, p(outf), *shape_out, 1, 1, p(ws), need)
        hip.call("rpnet_resample_labels", p(m_in), *shape_in, p(out8), *shape_out, 2, 0, 1, 0, p(stats), 1, 3, p(ws), need)

    def snapshot():
        torch.cuda.synchronize()
        assert (ws[need:] == 0xA5).all() and (outf[n_out:] == FILL).all() and (out8[n_out:] == FILL).all()
        return [t.cpu().numpy().copy() for t in (outf, out8, stats)]

    calls()
    eager = snapshot()
    want_l, rows = RC.ref_labels(lab, shape_out, (2,), "linear", "corner")
    assert same_bits(eager[0][:n_out].reshape(shape_out), RC.ref_image(img, shape_out, 1, "center"))
    assert np.array_equal(eager[1][:n_out].reshape(shape_out), want_l) and eager[2].tolist() == [[FILL] * 4, rows[0].tolist(), [FILL] * 4]
    outf.fill_(FILL), out8.fill_(FILL), stats.fill_(FILL)
    calls()
    for a, b in zip(eager, snapshot()):
        assert a.tobytes() == b.tobytes()

    # the public calls, captured: the cache holds its workspace after the eager call
    spacing, new_spacing = (2.5, 0.8, 0.7), (2.0, 1.1, 0.9)
    grid = RS.output_shape(shape_in, spacing, new_spacing)
    assert grid == RC.ref_output_shape(shape_in, spacing, new_spacing) and grid != shape_in
    given = torch.empty(grid, device=DEV, dtype=torch.float32)

    def chain():
        a, sa = RS.resample_to_spacing(src, spacing, new_spacing, align="center", out=given)
        b, sb = RS.resample_to_spacing(m_in, spacing, new_spacing, classes=(1, 2, 5), mode="linear")
        c = RS.resample_like(b, shape_in, classes=(1, 2, 5), mode="nearest")
        assert a is given and sa == RC.ref_out_spacing(shape_in, grid, spacing, "center") and sb == RC.ref_out_spacing(shape_in, grid, spacing, "corner")
        return [a, b, c]

    first = [t.cpu().numpy().copy() for t in chain()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = chain()
    runs = []
    for _ in range(2):
        for t in held:
            t.fill_(FILL)
        graph.replay()
        torch.cuda.synchronize()
        runs.append([t.cpu().numpy().copy() for t in held])
    for a, b, c in zip(first, runs[0], runs[1]):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    want_b = RC.ref_labels(lab, grid, (1, 2, 5), "linear", "corner")[0]
    assert same_bits(first[0], RC.ref_image(img, grid, 1, "center")) and np.array_equal(first[1], want_b)
    assert np.array_equal(first[2], RC.ref_labels(want_b, shape_in, None, "nearest", "corner")[0])


def test_refusals_launch_nothing():
    """every refusal of include/rpnet_resample_abi.h returns its status with a message and the outputs hold what they held; the Python
    layer refuses kind, contiguity, device, shape and option before the library is reached"""
    si, so = (5, 7, 9), (8, 5, 13)
    n_in, n_out = int(np.prod(si)), int(np.prod(so))
    img, i16, lab = dev(RC.noise_image(si, np.float32)), dev(RC.noise_image(si, np.int16)), dev(RC.label_map(si))
    outf = torch.full(so, float(FILL), device=DEV, dtype=torch.float32)
    out8 = torch.full(so, FILL, device=DEV, dtype=torch.uint8)
    stats = torch.full((2, 4), FILL, device=DEV, dtype=torch.int64)
    big = torch.zeros(4 * (n_in + n_out) + 64, device=DEV, dtype=torch.uint8)
    p = hip.ptr
    need = hip.query("rpnet_resample_workspace_bytes", *si, *so)
    ws = torch.empty(need + 16, device=DEV, dtype=torch.uint8)

    def image(src=p(img), kind=0, di=si, dst=p(outf), do=so, align=0, order=1, work=p(ws), nbytes=need):
        hip.call("rpnet_resample_image", src, kind, *di, dst, *do, align, order, work, nbytes)

    def labels(src=p(lab), di=si, dst=p(out8), do=so, cls=1, align=0, mode=1, merge=0, st=p(stats), row=0, rows=2, work=p(ws), nbytes=need):
        hip.call("rpnet_resample_labels", src, *di, dst, *do, cls, align, mode, merge, st, row, rows, work, nbytes)

    for fn, name in ((image, "resample_image"), (labels, "resample_labels")):
        for null in ("src", "dst", "work"):
            with pytest.raises(RuntimeError, match="null pointer"):
                fn(**{null: None})
        for key, dims in (("di", (0, 7, 9)), ("di", (5, 1025, 9)), ("di", (5, 7, -1)), ("do", (1025, 5, 13)), ("do", (8, 0, 13)), ("do", (8, 5, 1025))):
            with pytest.raises(RuntimeError, match=f"{name}: D=.*every extent 1..1024"):
                fn(**{key: dims})
        for align in (-1, 2):
            with pytest.raises(RuntimeError, match=f"align {align} "):
                fn(align=align)
        with pytest.raises(RuntimeError, match=f"workspace of {need - 1} bytes, {need} needed"):
            fn(nbytes=need - 1)
        with pytest.raises(RuntimeError, match="aligned"):
            fn(work=p(ws) + 8)
    for kind in (-1, 2, 3):
        with pytest.raises(RuntimeError, match=f"element kind {kind} "):
            image(kind=kind)
    for order in (-1, 2, 3):
        with pytest.raises(RuntimeError, match=f"order {order} "):
            image(order=order)
        with pytest.raises(RuntimeError, match=f"mode {order} "):
            labels(mode=order)
    with pytest.raises(RuntimeError, match="aligned"):
        image(src=p(img) + 2)
    with pytest.raises(RuntimeError, match="aligned"):
        image(kind=1, src=p(i16), dst=p(outf) + 1)
    with pytest.raises(RuntimeError, match="out overlaps in"):
        image(src=p(big), dst=p(big) + 4 * n_in - 4)
    with pytest.raises(RuntimeError, match="out overlaps in"):
        labels(src=p(big) + n_out - 1, dst=p(big))
    for cls in (0, 256, -1):
        with pytest.raises(RuntimeError, match=f"class {cls} "):
            labels(cls=cls)
    for cls in (256, -1):
        with pytest.raises(RuntimeError, match=f"class {cls} "):
            labels(cls=cls, mode=0)
    for merge in (2, -1):
        with pytest.raises(RuntimeError, match=f"merge {merge} "):
            labels(merge=merge)
    for row, rows in ((2, 2), (-1, 2), (0, 0)):
        with pytest.raises(RuntimeError, match=f"row {row} of a table of {rows} rows"):
            labels(row=row, rows=rows)
    with pytest.raises(RuntimeError, match="aligned"):
        labels(st=p(stats) + 4)
    for dims in ((0, 7, 9, 8, 5, 13), (5, 7, 9, 8, 5, 1025)):
        assert hip.query("rpnet_resample_workspace_bytes", *dims) == 0
        assert hip.load().rpnet_last_error_string().decode().startswith(f"resample: D={dims[0]} ")
    torch.cuda.synchronize()
    assert (outf == FILL).all() and (out8 == FILL).all() and (stats == FILL).all() and (big == 0).all()
    # the same calls with nothing wrong: class 0 is counted under NEAREST, and a null table forms no statistics
    host = lab.cpu().numpy()
    labels(cls=0, mode=0, row=1)
    labels(dst=p(big), st=None, rows=0)
    image(kind=1, src=p(i16), dst=p(outf), align=1)
    torch.cuda.synchronize()
    want, rows = RC.ref_labels(host, so, (0,), "nearest", "corner")
    assert np.array_equal(out8.cpu().numpy(), want) and stats.cpu().numpy().tolist() == [[FILL] * 4, rows[0].tolist()]
    assert np.array_equal(big[:n_out].cpu().numpy().reshape(so), RC.ref_labels(host, so, (1,), "linear", "corner")[0]) and (big[n_out:] == 0).all()
    assert same_bits(outf.cpu().numpy().view(np.int16).reshape(-1)[:n_out].reshape(so), RC.ref_image(i16.cpu().numpy(), so, 1, "center"))
    # the Python layer
    with pytest.raises(ValueError, match="float32 and int16 volumes are accepted"):
        RS.resample_image(img.double(), so)
    with pytest.raises(ValueError, match="float32 and int16 volumes are accepted"):
        RS.resample_image(lab, so)
    with pytest.raises(ValueError, match="uint8 volumes are accepted"):
        RS.resample_labels(img, so)
    with pytest.raises(ValueError, match=r"contiguous \[D,H,W\] tensor"):
        RS.resample_image(img.transpose(1, 2), so)
    with pytest.raises(ValueError, match=r"contiguous \[D,H,W\] tensor"):
        RS.resample_image(img[0], so)
    with pytest.raises(RuntimeError, match="MI355X only"):
        RS.resample_image(img.cpu(), so)
    with pytest.raises(RuntimeError, match="MI355X only"):
        RS.resample_labels(lab, so, out=torch.empty(so, dtype=torch.uint8))
    for bad in ((0, 5, 13), (8, 5, 1025), (8, 5), (8, 5, 2.5)):
        with pytest.raises(ValueError, match="three axis lengths"):
            RS.resample_image(img, bad)
        with pytest.raises(ValueError, match="three axis lengths"):
            RS.resample_labels(lab, bad)
    with pytest.raises(ValueError, match="three axis lengths"):
        RS.resample_image(torch.zeros((1, 1, 1025), device=DEV), so)
    for bad in ("edge", None, 0):
        with pytest.raises(ValueError, match="align must be"):
            RS.resample_image(img, so, align=bad)
    for bad in (2, -1, "linear", True):
        with pytest.raises(ValueError, match="order must be"):
            RS.resample_image(img, so, order=bad)
    for bad in ("cubic", 1, None):
        with pytest.raises(ValueError, match="mode must be"):
            RS.resample_labels(lab, so, (1,), mode=bad)
    with pytest.raises(ValueError, match="needs the classes"):
        RS.resample_labels(lab, so, mode="linear")
    for bad in ((), (0,), (1, 256)):
        with pytest.raises(ValueError, match="classes must be"):
            RS.resample_labels(lab, so, bad, mode="linear")
    with pytest.raises(ValueError, match="out must be a contiguous float32 tensor of shape"):
        RS.resample_image(img, so, out=torch.empty((8, 5, 12), device=DEV))
    with pytest.raises(ValueError, match="out must be a contiguous uint8 tensor of shape"):
        RS.resample_labels(lab, so, out=outf)
    with pytest.raises(ValueError, match="stats must be"):
        RS.resample_labels(lab, so, (1, 2, 5), stats=stats)
    with pytest.raises(ValueError, match="needs the classes it counts"):
        RS.resample_labels(lab, so, stats=stats)


def write_raw(raw, spacing, seed0=0):
    """two phantoms in the raw layout (axes x, y, z) with an anisotropic spacing -> {pid: (image, organ)}"""
    from rpnet_amd.utils import nrrd
    from tests import preprocess_cases as PC
    phantoms = {}
    for i, pid in enumerate(("p0", "p1")):
        img = PC.body_phantom((6, 96, 96), np.int16, seed=seed0 + i)[0]
        organ = np.zeros(img.shape, np.uint8)
        organ[1:5, 30:50, 35:60] = 1
        phantoms[pid] = (img, organ)
        os.makedirs(raw / pid / "structures")
        hdr = {"space": "left-posterior-superior", "space directions": f"({spacing[2]!r},0,0) (0,{spacing[1]!r},0) (0,0,{spacing[0]!r})"}
        nrrd.write(str(raw / pid / "img.nrrd"), np.swapaxes(img, 0, -1), header=hdr)
        nrrd.write(str(raw / pid / "structures" / "Liver.nrrd"), np.swapaxes(organ, 0, -1), header=hdr)
    return phantoms


def expected_files(save, phantoms, spacing, radius, resample=None, align="corner", interp="linear"):
    """the files the driver must write, formed from the restatements alone -> {pid: (shape, spacing of the output grid)}"""
    from rpnet_amd.utils import nrrd
    from tests import preprocess_cases as PC
    os.makedirs(save, exist_ok=True)
    grids = {}
    for pid, (img, organ) in phantoms.items():
        sp = spacing
        if resample is not None:
            grid = RC.ref_output_shape(img.shape, spacing, resample)
            sp = RC.ref_out_spacing(img.shape, grid, spacing, align)
            img = RC.ref_image(img, grid, 1, align)
            organ = RC.ref_labels(organ, grid, (1,), "linear", align)[0] if interp == "linear" else RC.ref_labels(organ, grid, None, "nearest", align)[0]
        mask = PC.ref_body_mask(img, radius=radius)[0]
        masked, row = PC.ref_mask_bbox(img, mask, -1024)
        y0, y1, x0, x1 = PC.ref_crop(row, True)
        hdr = {"space": "left-posterior-superior", "space directions": f"({sp[0]!r},0,0) (0,{sp[1]!r},0) (0,0,{sp[2]!r})"}
        nrrd.write(str(save / f"{pid}_clean.nrrd"), masked[:, y0:y1, x0:x1], header=hdr)
        nrrd.write(str(save / f"{pid}_Liver.nrrd"), organ[:, y0:y1, x0:x1], header=hdr)
        np.save(str(save / f"{pid}_bbox.npy"), np.array([[0, y0, x0], [img.shape[0], y1, x1]]))
        grids[pid] = (img.shape, sp)
    return grids


def same_directory(a, b):
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and len(names) == 6
    for name in names:
        assert open(a / name, "rb").read() == open(b / name, "rb").read(), name


def test_driver_end_to_end_with_resample(tmp_path, capsys):
    """tools/preprocess_volumes.py --resample on a synthetic raw directory: the image and the structure are resampled before the body
    mask and the crop; shapes from output_shape; the headers carry the spacing of the new grid, read back through
    FewshotVolumeReader.volume_spacing; bbox.npy is formed from the resampled shape; both alignments and both mask rules; every file
    byte for byte what the restatements give"""
    from rpnet_amd.utils.volume_reader import FewshotVolumeReader
    from tools import preprocess_volumes as TP
    raw = tmp_path / "raw"
    spacing, target = (2.5, 0.8, 0.7), (2.0, 1.1, 1.0)
    phantoms = write_raw(raw, spacing)
    for align, interp in (("corner", "linear"), ("center", "nearest")):
        save, want_dir = tmp_path / f"got_{align}", tmp_path / f"want_{align}"
        argv = ["--raw-dir", str(raw), "--save-dir", str(save), "--radius", "3", "--rois", "Liver", "--resample", "2.0,1.1,1.0"]
        results = TP.main(argv + (["--resample-align", align, "--mask-interp", interp] if align == "center" else []))
        capsys.readouterr()
        grids = expected_files(want_dir, phantoms, spacing, 3, target, align, interp)
        same_directory(save, want_dir)
        split = tmp_path / f"split_{align}"
        os.makedirs(split / "classes")
        (split / "all.csv").write_text("p0\np1\n")
        (split / "classes" / "Liver.csv").write_text("pid,z_start,z_end\np0,1,4\np1,1,4\n")
        cfg = {"class_csv_dir": str(split / "classes"), "train_classes": ["Liver"], "eval_classes": ["Liver"], "n_shot": 1, "n_way": 1, "num_slice": 6,
               "num_x": 96, "num_y": 96, "pad_value": -1024, "HU_range": [-1024, 3076], "crop_size": [96, 96], "do_elastic": False}
        reader = FewshotVolumeReader(str(save), str(split / "all.csv"), cfg, mode="eval")
        for r in results:
            grid, sp = grids[r["pid"]]
            assert grid == RS.output_shape((6, 96, 96), spacing, target) == (8, 70, 67) and r["shape"][0] == 8
            assert r["bbox"][1][0] == 8 and r["bbox"][1][1] <= 70 and r["bbox"][1][2] <= 67
            assert reader.volume_spacing(r["pid"]) == sp == RS.out_spacing((6, 96, 96), grid, spacing, align)


def test_driver_without_resample_writes_what_it_wrote(tmp_path, capsys):
    """the same raw directory without --resample: every file byte for byte what preprocess_one gave before the option existed (the
    masked, cropped restatement under the input's own spacing), through main() and through preprocess_one with its defaults"""
    from tools import preprocess_volumes as TP
    raw = tmp_path / "raw"
    spacing = (2.5, 0.8, 0.7)
    phantoms = write_raw(raw, spacing)
    expected_files(tmp_path / "want", phantoms, spacing, 3)
    TP.main(["--raw-dir", str(raw), "--save-dir", str(tmp_path / "main"), "--radius", "3", "--rois", "Liver"])
    for pid in phantoms:
        TP.preprocess_one(pid, str(raw), str(tmp_path / "one"), DEV, radius=3, rois=["Liver"])
    capsys.readouterr()
    same_directory(tmp_path / "main", tmp_path / "want")
    same_directory(tmp_path / "one", tmp_path / "want")
