"""rpnet_smooth_image (csrc/smooth.hip), rpnet_amd.smooth, the `antialias` option of rpnet_amd.resample and tools/preprocess_volumes.py
--antialias on the MI355X.

Every comparison is exact equality with tests/smooth_cases.py (numpy: the definition of include/rpnet_smooth_abi.h operation by operation;
pinned to scipy.ndimage.gaussian_filter by tests/test_host_smooth.py), bit for bit; a NaN that an operation makes is compared as a NaN.
There is no tolerance."""
import itertools
import os

import numpy as np
import pytest
import torch

from rpnet_amd import hip
from rpnet_amd import resample as RS
from rpnet_amd import smooth as SM
from tests import resample_cases as RC
from tests import smooth_cases as SC
from tests.test_gpu_resample import dev, same_bits, same_bits_or_both_nan, same_directory, write_raw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 7
DTYPES = (np.float32, np.int16)


def check_smooth(vol, sigmas, what, same=same_bits):
    """both borders of one volume == the restatement, bit for bit, twice; the input untouched"""
    src = dev(vol)
    for mode in SC.MODES:
        want = SC.ref_smooth(vol, sigmas, mode)
        got = SM.smooth_image(src, sigmas, mode=mode).cpu().numpy()
        again = SM.smooth_image(src, sigmas, mode=mode).cpu().numpy()
        assert same(got, want), (what, mode, int((got.view(np.uint8) != want.view(np.uint8)).sum()))
        assert got.tobytes() == again.tobytes(), (what, mode)
    assert same_bits(src.cpu().numpy(), vol), what


@pytest.mark.parametrize("case", SC.SMALL)
def test_small_volumes_equal_the_restatement(case):
    """one voxel with radius 3, each axis of length 1 with a radius on it, lines of 2 and 3 under radius 7, 5 x 7 x 9 with three sigmas, a
    radius on one axis only, on two, and on none (the identity bit for bit); both kinds, both borders"""
    shape, sigmas = case
    rz, ry, rx = SC.radii(sigmas)
    buffers = min(2, max(0, (rz != 0) + (ry != 0) + (rx != 0) - 1))
    assert hip.query("rpnet_smooth_workspace_bytes", *shape, rz, ry, rx) == 64 + 16 * ((int(np.prod(shape)) + 1) // 2) * buffers
    for dtype in DTYPES:
        vol = SC.noise_image(shape, dtype, seed=1)
        check_smooth(vol, sigmas, f"{shape} {sigmas} {dtype.__name__}")
        if not any(sigmas):
            v = vol.copy()
            if dtype is np.float32:
                v.flat[:4] = (np.nan, np.inf, -np.inf, -0.0)
            assert same_bits(SM.smooth_image(dev(v), 0.0).cpu().numpy(), v)


@pytest.mark.parametrize("dtype", DTYPES)
def test_tiles_runs_and_unaligned_rows(dtype):
    """every tile extent of csrc/smooth.hip + 1 and 2 * tile + 2 with a radius that crosses the seam; rows of one lane run + 1, and rows
    whose first address is not 16-byte aligned: by their length, and by a view 1 element into an allocation for input and output"""
    t = getattr(torch, np.dtype(dtype).name)
    d = np.dtype(dtype)
    assert (SM.LANE_RUN[t], SM.X_TILE[t], SM.X_ROWS, SM.AXIS_SEG[t]) == (SC.LANE_RUN[d], SC.X_TILE[d], SC.X_ROWS, SC.AXIS_SEG[d])
    for shape, sigmas in SC.tile_shapes(dtype):
        check_smooth(SC.noise_image(shape, dtype, seed=2), sigmas, f"{shape} {sigmas} {d.name}")
    shape = (5, 9, 4 * SC.LANE_RUN[d])
    n = int(np.prod(shape))
    vol = SC.noise_image(shape, dtype, seed=3)
    flat_in = torch.zeros(n + 1, device=DEV, dtype=t)
    flat_out = torch.full((n + 2,), FILL, device=DEV, dtype=t)
    src, out = flat_in[1:].view(shape), flat_out[1:n + 1].view(shape)
    src.copy_(dev(vol))
    assert src.data_ptr() % 16 == d.itemsize == out.data_ptr() % 16
    for sigmas in ((0.75, 1.0, 0.5), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 0.0, 0.0)):
        got = SM.smooth_image(src, sigmas, out=out)
        assert got is out and same_bits(got.cpu().numpy(), SC.ref_smooth(vol, sigmas)), sigmas
        assert flat_out[0] == FILL and flat_out[n + 1] == FILL


@pytest.mark.parametrize("case", SC.LINES + SC.WIDE)
def test_lines_of_1024_and_radius_255(case):
    """a line of 1024 along each axis with the other two axes 2, and radius 255 on a line of 300 along each axis"""
    shape, sigmas = case
    if case in SC.WIDE:
        assert max(SC.radii(sigmas)) == 255 == SM.MAX_RADIUS
    for dtype in DTYPES:
        check_smooth(SC.noise_image(shape, dtype, seed=4), sigmas, f"{shape} {sigmas} {dtype.__name__}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_more_lanes_than_one_sweep(dtype):
    """65 x 1024 x 1024: the y pass, the z pass and the copy of the identity each have more lanes than 8192 blocks of 256 hold, so a
    block sweeps more than once (a lane is (block * sweeps + sweep) * 256 + thread: every stretch of the volume holds lanes of every
    sweep).  A pass along an axis filters every line of that axis on its own, so the restatement of a strided set of whole lines, the
    first and the last among them, is compared bit for bit; the identity is compared over the whole volume on the device"""
    shape = (65, 1024, 1024)
    t = getattr(torch, np.dtype(dtype).name)
    run, seg = SM.LANE_RUN[t], SM.AXIS_SEG[t]
    one_sweep = 8192 * 256
    assert 65 * (1024 // seg) * (1024 // run) > one_sweep and -(-65 // seg) * (1024 * 1024 // run) > one_sweep
    assert int(np.prod(shape)) * np.dtype(dtype).itemsize // 16 > one_sweep
    gen = torch.Generator(device=DEV).manual_seed(11)
    if dtype is np.int16:
        vol = torch.randint(-1024, 3000, shape, device=DEV, dtype=torch.int16, generator=gen)
    else:
        vol = torch.randn(shape, device=DEV, generator=gen) * 400.0 - 200.0
    out = torch.empty_like(vol)
    some = torch.tensor(sorted(set(range(0, 1024, 61)) | {1023}), device=DEV)
    planes = torch.tensor([0, 1, 31, 32, 63, 64], device=DEV)
    assert SM.smooth_image(vol, 0.0, out=out) is out and torch.equal(out, vol)
    SM.smooth_image(vol, (0.75, 0.0, 0.0), mode="nearest", out=out)
    lines = vol[:, some][:, :, some].cpu().numpy()                  # whole z lines
    assert same_bits(out[:, some][:, :, some].cpu().numpy(), SC.ref_smooth(lines, (0.75, 0.0, 0.0), "nearest"))
    SM.smooth_image(vol, (0.0, 0.75, 0.0), mode="reflect", out=out)
    lines = vol[planes][:, :, some].cpu().numpy()                   # whole y lines
    assert same_bits(out[planes][:, :, some].cpu().numpy(), SC.ref_smooth(lines, (0.0, 0.75, 0.0), "reflect"))


def call_tables(vol, tables, border, out=None):
    """rpnet_smooth_image through the C ABI with weight tables of the test's own: ((wz, rz), (wy, ry), (wx, rx))"""
    src = dev(vol)
    out = torch.empty_like(src) if out is None else out
    held = [(None, 0) if r == 0 else (dev(np.asarray(w, np.float64)), r) for w, r in tables]
    radii = [r for _, r in held]
    need = hip.query("rpnet_smooth_workspace_bytes", *vol.shape, *radii)
    ws = torch.empty(need, device=DEV, dtype=torch.uint8)
    args = [a for w, r in held for a in (hip.ptr(w), r)]
    hip.call("rpnet_smooth_image", hip.ptr(src), SM.VOLUME_KINDS[src.dtype], *vol.shape, hip.ptr(out), *args, border, hip.ptr(ws), need)
    return out.cpu().numpy()


def test_ties_saturation_impulses_and_non_finite():
    """int16 ties at exactly .5 above even and above odd integers from the weights (0.25, 0.5, 0.25); both ends of the int16 range,
    saturating under weights that sum to 3; an impulse at each corner and at the centre gives the outer product of the weights; a NaN and
    an infinity spread over their ball"""
    quarter = ((None, 0), (None, 0), (np.array([0.25, 0.5, 0.25]), 1))
    v = np.array([[[1, 0, 1, 0, 1, 2, 3, 2, 3, -1, 0, -1, -2, -3, -2]]], np.int16)
    f = SC.smooth_f64(v, None, "nearest", tables=quarter)
    ties = np.abs(f - np.trunc(f)) == 0.5
    assert ties.sum() >= 6 and {int(x) % 2 for x in np.floor(f[ties])} == {0, 1}
    for border, mode in enumerate(SC.MODES):
        got = call_tables(v, quarter, border)
        assert same_bits(got, SC.ref_smooth(v, None, mode, tables=quarter)) and np.all(got[ties] % 2 == 0)
    for axis in range(3):
        tables = [(None, 0)] * 3
        tables[axis] = (np.array([1.0, 1.0, 1.0]), 1)
        big = np.array([32767, 32767, -32768, -32768, 100], np.int16).reshape([5 if a == axis else 1 for a in range(3)])
        got = call_tables(big, tables, SM.CLAMP)
        assert got.reshape(-1).tolist() == [32767, 32766, -32768, -32768, -32568] and same_bits(got, SC.ref_smooth(big, None, "nearest", tables=tables))
    shape, sigmas = (7, 9, 11), (0.5, 0.75, 1.0)
    wz, wy, wx = (SC.weights(s)[0] for s in sigmas)
    rz, ry, rx = SC.radii(sigmas)
    corners = tuple(itertools.product((0, 6), (0, 8), (0, 10)))
    assert len(corners) == 8
    for at in corners + ((3, 4, 5),):
        v = np.zeros(shape, np.float32)
        v[at] = 1.0
        check_smooth(v, sigmas, f"impulse at {at}")
    got = SM.smooth_image(dev(v), sigmas).cpu().numpy()              # the centre: no border in reach
    outer = ((wx[None, None, :] * np.ones((1, 2 * ry + 1, 1))) * wy[None, :, None]) * wz[:, None, None]
    assert same_bits(got[3 - rz:4 + rz, 4 - ry:5 + ry, 5 - rx:6 + rx], outer.astype(np.float32))
    assert np.count_nonzero(got) == outer.size
    for bad in (np.nan, np.inf, -np.inf):
        v = SC.noise_image(shape, np.float32, seed=5)
        v[3, 4, 5] = bad
        v[0, 0, 0] = -bad
        check_smooth(v, sigmas, f"{bad} in the volume", same_bits_or_both_nan)
        got = SM.smooth_image(dev(v), sigmas).cpu().numpy()
        assert not np.isfinite(got[3 - rz:4 + rz, 4 - ry:5 + ry, 5 - rx:6 + rx]).any() and np.isfinite(got[6, 8, 10])


def test_guard_words_out_given_and_graph_replay():
    """calls through the C ABI with `out` and the workspace prefilled with a pattern, the workspace of exactly the size asked for, guard
    words behind both intact; a second identical call gives the same bits; smooth_image and resample_to_spacing(antialias=True) captured
    with torch.cuda.graph and replayed twice give identical bits, equal to the eager call and to the restatement"""
    shape, sigmas = (6, 21, 33), (0.75, 1.0, 1.5)
    n = int(np.prod(shape))
    vol = SC.noise_image(shape, np.float32, seed=6)
    src = dev(vol)
    tables = [SM.smooth_device_weights(s, 4.0, src.device) for s in sigmas]
    radii = [r for _, r in tables]
    need = hip.query("rpnet_smooth_workspace_bytes", *shape, *radii)
    assert need == 64 + 16 * ((n + 1) // 2) * 2
    ws = torch.full((need + 64,), 0xA5, device=DEV, dtype=torch.uint8)
    out = torch.full((n + 16,), float("nan"), device=DEV, dtype=torch.float32)
    args = [a for w, r in tables for a in (hip.ptr(w), r)]
    runs = []
    for _ in range(2):
        ws.fill_(0xA5), out.fill_(float("nan"))
        hip.call("rpnet_smooth_image", hip.ptr(src), 0, *shape, hip.ptr(out), *args, SM.REFLECT, hip.ptr(ws), need)
        torch.cuda.synchronize()
        assert (ws[need:] == 0xA5).all() and torch.isnan(out[n:]).all()
        runs.append(out[:n].cpu().numpy().reshape(shape).copy())
    assert same_bits(runs[0], SC.ref_smooth(vol, sigmas)) and runs[0].tobytes() == runs[1].tobytes()

    spacing, new_spacing = (2.5, 0.8, 0.7), (2.0, 2.0, 1.5)
    grid = RS.output_shape(shape, spacing, new_spacing)
    assert grid == (8, 8, 15)
    given, given_s = torch.empty(grid, device=DEV, dtype=torch.float32), torch.empty(shape, device=DEV, dtype=torch.float32)

    def chain():
        a = SM.smooth_image(src, 1.5, spacing=(3.0, 1.5, 0.75), mode="nearest", out=given_s)
        b, sb = RS.resample_to_spacing(src, spacing, new_spacing, align="center", out=given, antialias=True)
        assert a is given_s and b is given and sb == RC.ref_out_spacing(shape, grid, spacing, "center")
        return [a, b]

    first = [t.cpu().numpy().copy() for t in chain()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = chain()
    replays = []
    for _ in range(2):
        for t in held:
            t.fill_(FILL)
        graph.replay()
        torch.cuda.synchronize()
        replays.append([t.cpu().numpy().copy() for t in held])
    for a, b, c in zip(first, replays[0], replays[1]):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    assert same_bits(first[0], SC.ref_smooth(vol, (0.5, 1.0, 2.0), "nearest")) and same_bits(first[1], SC.ref_antialiased(vol, grid, "center"))


def test_refusals_launch_nothing():
    """every refusal of include/rpnet_smooth_abi.h returns its status with a message and the output holds what it held; the Python layer
    refuses kind, contiguity, device, shape and option before the library is reached"""
    shape = (5, 7, 9)
    n = int(np.prod(shape))
    img, i16 = dev(SC.noise_image(shape, np.float32)), dev(SC.noise_image(shape, np.int16))
    out = torch.full(shape, float(FILL), device=DEV, dtype=torch.float32)
    big = torch.zeros(8 * n + 64, device=DEV, dtype=torch.uint8)
    w = dev(np.full(16, 1.0 / 3))
    p = hip.ptr
    need = hip.query("rpnet_smooth_workspace_bytes", *shape, 1, 1, 1)
    assert need == 64 + 16 * ((n + 1) // 2) * 2
    ws = torch.empty(need + 16, device=DEV, dtype=torch.uint8)

    def image(src=p(img), kind=0, dims=shape, dst=p(out), wz=p(w), rz=1, wy=p(w), ry=1, wx=p(w), rx=1, border=0, work=p(ws), nbytes=need):
        hip.call("rpnet_smooth_image", src, kind, *dims, dst, wz, rz, wy, ry, wx, rx, border, work, nbytes)

    for null in ("src", "dst", "work"):
        with pytest.raises(RuntimeError, match="smooth_image: null pointer"):
            image(**{null: None})
    for axis in ("z", "y", "x"):
        with pytest.raises(RuntimeError, match="a weight table is null exactly when its radius is 0"):
            image(**{"w" + axis: None})
        with pytest.raises(RuntimeError, match="a weight table is null exactly when its radius is 0"):
            image(**{"r" + axis: 0})
        for r in (-1, 256):
            with pytest.raises(RuntimeError, match=f"radii .*{axis}={r}.*every radius 0..255"):
                image(**{"r" + axis: r})
        with pytest.raises(RuntimeError, match="weight tables must be aligned to 8 bytes"):
            image(**{"w" + axis: p(w) + 4})
    for kind in (-1, 2, 3):
        with pytest.raises(RuntimeError, match=f"element kind {kind} "):
            image(kind=kind)
    for border in (-1, 2):
        with pytest.raises(RuntimeError, match=f"border {border} "):
            image(border=border)
    for dims in ((0, 7, 9), (5, 1025, 9), (5, 7, -1), (5, 7, 1025)):
        with pytest.raises(RuntimeError, match="smooth_image: D=.*every extent 1..1024"):
            image(dims=dims)
    with pytest.raises(RuntimeError, match=f"workspace of {need - 1} bytes, {need} needed"):
        image(nbytes=need - 1)
    with pytest.raises(RuntimeError, match="workspace to 16 bytes"):
        image(work=p(ws) + 8)
    with pytest.raises(RuntimeError, match="aligned to their element"):
        image(src=p(img) + 2)
    with pytest.raises(RuntimeError, match="aligned to their element"):
        image(kind=1, src=p(i16), dst=p(out) + 1)
    with pytest.raises(RuntimeError, match="out overlaps in"):
        image(src=p(big), dst=p(big) + 4 * n - 4)
    with pytest.raises(RuntimeError, match="the workspace overlaps a volume"):
        image(src=p(ws) + 16)
    with pytest.raises(RuntimeError, match="the workspace overlaps a volume"):
        image(dst=p(ws) + need - 16)
    for bad in ((0, 7, 9, 1, 1, 1), (5, 7, 1025, 1, 1, 1), (5, 7, 9, -1, 1, 1), (5, 7, 9, 1, 1, 256)):
        assert hip.query("rpnet_smooth_workspace_bytes", *bad) == 0
        text = hip.load().rpnet_last_error_string().decode()
        assert text.startswith(f"smooth: D={bad[0]} H=7 W={bad[2]}, radii z={bad[3]} y=1 x={bad[5]}") and "every radius 0..255" in text
    torch.cuda.synchronize()
    assert (out == FILL).all() and (big == 0).all()
    # the same call with nothing wrong, and with one table absent
    third = np.full(3, 1.0 / 3)
    image()
    assert same_bits(out.cpu().numpy(), SC.ref_smooth(img.cpu().numpy(), None, "reflect", tables=[(third, 1)] * 3))
    image(wy=None, ry=0, border=1)
    assert same_bits(out.cpu().numpy(), SC.ref_smooth(img.cpu().numpy(), None, "nearest", tables=[(third, 1), (None, 0), (third, 1)]))
    # the Python layer
    lab = torch.zeros(shape, device=DEV, dtype=torch.uint8)
    for bad in (img.double(), lab):
        with pytest.raises(ValueError, match="float32 and int16 volumes are accepted"):
            SM.smooth_image(bad, 1.0)
    for bad in (img.transpose(1, 2), img[0], torch.zeros((1, 1, 1025), device=DEV)):
        with pytest.raises(ValueError, match=r"contiguous \[D,H,W\] tensor"):
            SM.smooth_image(bad, 1.0)
    with pytest.raises(RuntimeError, match="MI355X only"):
        SM.smooth_image(img.cpu(), 1.0)
    with pytest.raises(RuntimeError, match="MI355X only"):
        SM.smooth_image(img, 1.0, out=torch.empty(shape))
    for bad in ("mirror", None, 0):
        with pytest.raises(ValueError, match="mode must be"):
            SM.smooth_image(img, 1.0, mode=bad)
    for bad in ((1, 2), "a", float("inf")):
        with pytest.raises(ValueError, match="sigma must be"):
            SM.smooth_image(img, bad)
    with pytest.raises(ValueError, match="spacing must be"):
        SM.smooth_image(img, 1.0, spacing=(1, 1))
    with pytest.raises(ValueError, match=r"of the y axis gives radius 256"):
        SM.smooth_image(img, (1.0, 64.0, 1.0))
    with pytest.raises(ValueError, match="out must be a contiguous float32 tensor of shape"):
        SM.smooth_image(img, 1.0, out=torch.empty((5, 7, 8), device=DEV))
    with pytest.raises(ValueError, match="out must be a contiguous float32 tensor of shape"):
        SM.smooth_image(img, 1.0, out=i16)


def test_antialiased_resample_equals_the_composed_restatement():
    """resample_image(antialias=False) is the plain call on the rows of tests/resample_cases.py; antialias=True equals smooth (border
    nearest, the kind of the volume) followed by the linear rule, at 8 x 20 x 20 -> 8 x 8 x 8 and 5 x 7 x 9 -> 8 x 5 x 13, where only the
    shrinking y axis is filtered; no axis shrinking is the plain call; a label map is refused"""
    for shape_in, shape_out in RC.SMALL:
        for dtype in DTYPES:
            img = RC.noise_image(shape_in, dtype, seed=1)
            for align in RC.ALIGNS:
                plain = RS.resample_image(dev(img), shape_out, align=align, antialias=False).cpu().numpy()
                assert same_bits(plain, RS.resample_image(dev(img), shape_out, align=align).cpu().numpy())
                assert same_bits(plain, RC.ref_image(img, shape_out, 1, align))
    for shape_in, shape_out in (((8, 20, 20), (8, 8, 8)), ((5, 7, 9), (8, 5, 13)), ((5, 7, 9), (5, 7, 9)), ((5, 7, 9), (6, 7, 12))):
        sig = SM.antialias_sigma(shape_in, shape_out)
        assert sig == SC.antialias_sigmas(shape_in, shape_out) and all((s > 0) == (m < n) for s, n, m in zip(sig, shape_in, shape_out))
        for dtype in DTYPES:
            img = SC.noise_image(shape_in, dtype, seed=7)
            src = dev(img)
            for align in RC.ALIGNS:
                got = RS.resample_image(src, shape_out, align=align, antialias=True).cpu().numpy()
                assert same_bits(got, SC.ref_antialiased(img, shape_out, align)), (shape_in, shape_out, dtype.__name__, align)
                if not any(sig):
                    assert same_bits(got, RC.ref_image(img, shape_out, 1, align))
                elif dtype is np.float32:           # (7 -> 5 is sigma 0.2, weights (4e-6, 1, 4e-6): an int16 volume comes back as it was)
                    assert not same_bits(got, RC.ref_image(img, shape_out, 1, align))
            assert same_bits(src.cpu().numpy(), img)
    got, sp = RS.resample_to_spacing(dev(img), (1.0, 1.0, 1.0), (1.0, 2.0, 2.0), antialias=True)
    assert same_bits(got.cpu().numpy(), SC.ref_antialiased(img, (5, 4, 4))) and sp == RC.ref_out_spacing((5, 7, 9), (5, 4, 4), (1.0,) * 3, "corner")
    lab = dev(RC.label_map((5, 7, 9)))
    with pytest.raises(ValueError, match="a uint8 label map keeps the indicator rule"):
        RS.resample_to_spacing(lab, (1.0, 1.0, 1.0), (1.0, 2.0, 2.0), antialias=True)
    with pytest.raises(ValueError, match="a uint8 label map keeps the indicator rule"):
        RS.resample_like(lab, (5, 4, 4), antialias=True)
    with pytest.raises(ValueError, match="float32 and int16 volumes are accepted"):
        RS.resample_image(lab, (5, 4, 4), antialias=True)
    assert np.array_equal(RS.resample_like(lab, (5, 4, 4), antialias=False).cpu().numpy(), RC.ref_labels(lab.cpu().numpy(), (5, 4, 4))[0])


def expected_antialiased_files(save, phantoms, spacing, radius, target):
    """the files tools/preprocess_volumes.py --resample --antialias must write, formed from the restatements alone"""
    from rpnet_amd.utils import nrrd
    from tests import preprocess_cases as PC
    os.makedirs(save, exist_ok=True)
    for pid, (img, organ) in phantoms.items():
        grid = RC.ref_output_shape(img.shape, spacing, target)
        sp = RC.ref_out_spacing(img.shape, grid, spacing, "corner")
        img = SC.ref_antialiased(img, grid, "corner")
        organ = RC.ref_labels(organ, grid, (1,), "linear", "corner")[0]
        mask = PC.ref_body_mask(img, radius=radius)[0]
        masked, row = PC.ref_mask_bbox(img, mask, -1024)
        y0, y1, x0, x1 = PC.ref_crop(row, True)
        hdr = {"space": "left-posterior-superior", "space directions": f"({sp[0]!r},0,0) (0,{sp[1]!r},0) (0,0,{sp[2]!r})"}
        nrrd.write(str(save / f"{pid}_clean.nrrd"), masked[:, y0:y1, x0:x1], header=hdr)
        nrrd.write(str(save / f"{pid}_Liver.nrrd"), organ[:, y0:y1, x0:x1], header=hdr)
        np.save(str(save / f"{pid}_bbox.npy"), np.array([[0, y0, x0], [img.shape[0], y1, x1]]))


def test_driver_with_and_without_antialias(tmp_path, capsys):
    """tools/preprocess_volumes.py --resample ... --antialias on a synthetic raw directory: every file byte for byte what the
    restatements give (the image smoothed, then resampled, then masked and cropped); the structures resampled exactly as without the
    flag; without the flag, with and without --resample, the files are byte for byte what the driver wrote before the flag existed;
    the flag without --resample is refused"""
    from tests.test_gpu_resample import expected_files
    from tools import preprocess_volumes as TP
    raw = tmp_path / "raw"
    spacing, target = (2.5, 0.8, 0.7), (2.0, 1.7, 1.6)
    phantoms = write_raw(raw, spacing)
    argv = ["--raw-dir", str(raw), "--radius", "3", "--rois", "Liver"]
    res_aa = TP.main(argv + ["--save-dir", str(tmp_path / "aa"), "--resample", "2.0,1.7,1.6", "--antialias"])
    res_plain = TP.main(argv + ["--save-dir", str(tmp_path / "plain"), "--resample", "2.0,1.7,1.6"])
    TP.main(argv + ["--save-dir", str(tmp_path / "none")])
    capsys.readouterr()
    expected_antialiased_files(tmp_path / "want_aa", phantoms, spacing, 3, target)
    expected_files(tmp_path / "want_plain", phantoms, spacing, 3, target)
    expected_files(tmp_path / "want_none", phantoms, spacing, 3)
    same_directory(tmp_path / "aa", tmp_path / "want_aa")
    same_directory(tmp_path / "plain", tmp_path / "want_plain")
    same_directory(tmp_path / "none", tmp_path / "want_none")
    grid = RC.ref_output_shape((6, 96, 96), spacing, target)
    for pid, (img, organ) in phantoms.items():
        # the flag changes the image and leaves the structure's resampling alone
        assert not same_bits(SC.ref_antialiased(img, grid), RC.ref_image(img, grid, 1, "corner"))
        for name in (f"{pid}_Liver.nrrd", f"{pid}_bbox.npy"):
            assert open(tmp_path / "aa" / name, "rb").read() == open(tmp_path / "plain" / name, "rb").read(), name
        assert open(tmp_path / "aa" / f"{pid}_clean.nrrd", "rb").read() != open(tmp_path / "plain" / f"{pid}_clean.nrrd", "rb").read()
    assert [r["rois"] for r in res_aa] == [r["rois"] for r in res_plain] == [["Liver"], ["Liver"]]
    with pytest.raises(SystemExit, match="--antialias is read with --resample"):
        TP.main(argv + ["--save-dir", str(tmp_path / "bad"), "--antialias"])
