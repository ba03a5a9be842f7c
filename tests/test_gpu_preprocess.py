"""rpnet_prep_threshold, rpnet_prep_seeded_component and rpnet_prep_mask_bbox (csrc/prep.hip), rpnet_amd.preprocess and
tools/preprocess_volumes.py on the MI355X.

Every comparison is exact equality with tests/preprocess_cases.py (numpy: the definitions of include/rpnet_prep_abi.h operation by
operation; pinned to an exact Otsu, scipy.ndimage and np.where by tests/test_host_preprocess.py): masks, every table and the box; the
masked image bit for bit.  There is no tolerance."""
import os

import numpy as np
import pytest
import torch

from rpnet_amd import hip
from rpnet_amd import preprocess as PP
from tests import morphology_cases as MX
from tests import preprocess_cases as PC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 7
KINDS = ((np.float32, 0), (np.int16, 1))


def dev(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(DEV)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_threshold(img, threshold, what):
    """one public call == the restatement: the mask and both tables; the image untouched"""
    src = dev(img)
    out = torch.full(img.shape, FILL, device=DEV, dtype=torch.uint8)
    got = PP.threshold_mask(src, threshold, out=out)
    want = PC.ref_threshold(img, threshold)
    torch.cuda.synchronize()
    assert got[0] is out and same_bits(src.cpu().numpy(), img), what
    res = out.cpu().numpy()
    assert np.array_equal(res, want[0]), (what, int((res != want[0]).sum()))
    assert got[1].cpu().numpy().tolist() == want[1].tolist(), (what, got[1].cpu().numpy().tolist(), want[1].tolist())
    assert same_bits(got[2].cpu().numpy(), want[2]), (what, got[2].cpu().numpy().tolist(), want[2].tolist())
    return want


@pytest.mark.parametrize("shape", PC.SHAPES)
def test_threshold_equals_the_restatement(shape):
    """one voxel, each axis of length 1, the labelling tile plus one and twice the tile plus two (slices of 2145 and 8580 pixels: lanes
    that are not whole, slices that start off a 16-byte boundary), a line of 1024 along each axis; both element kinds; Otsu and a fixed
    threshold; slices with their own lo and hi"""
    assert hip.query("rpnet_prep_threshold_workspace_bytes", *shape) == 64 + shape[0] * 136 * 4
    for dtype, _ in KINDS:
        img = PC.noise_image(shape, dtype, seed=1)
        _, rows, frows = check_threshold(img, "otsu", f"{shape} {dtype.__name__} otsu")
        if shape[1] * shape[2] > 100:
            assert (rows[:, 1] >= 0).all() and (rows[:, 2] > 0).all() and len(set(frows[:, 0].tolist())) == shape[0]
        for t in (-400.0, float(img.flat[0])):
            check_threshold(img, t, f"{shape} {dtype.__name__} fixed {t}")


def test_threshold_cases():
    """a constant slice, two values, a voxel equal to hi (bin 127), values on bin edges, negative values, int16 at both limits, NaN and
    both infinities in a float slice and a slice of NaN only, zeros of both signs, different lo / hi in neighbouring slices; the fixed
    threshold at, just below and just above a voxel value"""
    for dtype, _ in KINDS:
        for name, img in PC.threshold_cases(dtype):
            check_threshold(img, "otsu", f"{dtype.__name__} {name}")
            for t in PC.fixed_thresholds(img):
                check_threshold(img, t, f"{dtype.__name__} {name} fixed {t!r}")
    f = dict(PC.threshold_cases(np.float32))
    mask, rows, frows = PP.threshold_mask(dev(f["non-finite"]))
    assert rows[:, 0].tolist() == [45, 42, 24, 0, 48] and rows[3:, 1].tolist() == [-1, -1] and not mask[3:].any()
    mask, rows, frows = PP.threshold_mask(dev(f["bin edges and hi"]))
    assert frows[0].tolist()[:2] == [0.0, 128.0] and bool(mask[0].flatten()[-1]) and frows[0, 2].item() == rows[0, 1].item() + 1.0
    for bad in ("mean", None, float("nan"), True):
        with pytest.raises(ValueError, match="threshold must be"):
            PP.threshold_mask(dev(f["negative"]), bad)
    with pytest.raises(ValueError, match="float32 and int16"):
        PP.threshold_mask(dev(f["negative"].astype(np.float64)))


def check_seeded(vol, cls, seed, conn, what, in_place=False):
    src = dev(vol)
    out = src if in_place else torch.full(vol.shape, FILL, device=DEV, dtype=torch.uint8)
    stats = torch.full((1, vol.shape[0], PP.SEED_ROW), FILL, device=DEV, dtype=torch.int64)
    got = PP.seeded_component(src, (cls,), seed=seed, connectivity=conn, out=out, stats=stats)
    want, rows = PC.ref_seeded(vol, cls, seed, conn)
    torch.cuda.synchronize()
    assert got[0] is out and got[1] is stats
    res = out.cpu().numpy()
    assert np.array_equal(res, want), (what, int((res != want).sum()))
    if not in_place:
        assert np.array_equal(src.cpu().numpy(), vol), what
    assert stats.cpu().numpy()[0].tolist() == rows.tolist(), (what, stats.cpu().numpy()[0].tolist(), rows.tolist())
    assert PP.seed_overrun(DEV, vol.shape) == 0, what
    return res, rows


@pytest.mark.parametrize("shape", PC.SHAPES)
def test_seeded_component_equals_the_restatement(shape):
    """the seed on background and on the class, a component that crosses the tile seams in x and in y, the same blob in the neighbouring
    slice (nothing leaks across z), a diagonal contact under 4 and 8, a seed at each corner, noise; a label volume whose other classes
    pass through; in place and out of place; the overrun word 0 after every call"""
    D, H, W = shape
    n = D * H * W
    assert hip.query("rpnet_prep_seeded_component_workspace_bytes", *shape) == 64 + 2 * ((4 * n + 15) // 16 * 16) + 16 * D
    k = 0
    for name, vol, seed in PC.component_cases(shape):
        for conn in (4, 8):
            k += 1
            res, rows = check_seeded(vol, 1, seed, conn, f"{shape} {name} {conn}", in_place=bool(k % 2))
            if name.startswith("snake"):
                assert rows.tolist() == [[1, int(vol[0].sum()), int(vol[0].sum()), 1]] * D
            if name == "no leak across z" and H > 4 and W > 4:
                assert rows[:, 0].tolist() == [1 - z % 2 for z in range(D)] and not res[1::2].any() and res[0::2].any()
            if name == "diagonal contact" and H > 2 and W > 2 and H // 2 + 1 < H and W // 2 + 1 < W:
                assert rows[0, 2] == (1 if conn == 4 else rows[0, 1]) and rows[0, 3] == (2 if conn == 4 else 1)
    lab = (MX.noise(shape, 0.55) * 2 + (MX.noise(shape, 0.3, seed=5) == 1) * (MX.noise(shape, 0.55) == 0) * 5).astype(np.uint8)
    for conn in (4, 8):
        res, _ = check_seeded(lab, 2, None, conn, f"{shape} labels {conn}")
        assert np.array_equal(res[lab == 5], lab[lab == 5]) and not res[lab == 0].any()
    # two classes in sequence: the second reads the result of the first
    want, rows2 = PC.ref_seeded(lab, 2, None, 4)
    want, rows5 = PC.ref_seeded(want, 5, None, 4)
    out, stats = PP.seeded_component(dev(lab), (2, 5))
    assert np.array_equal(out.cpu().numpy(), want) and stats.cpu().numpy().tolist() == [rows2.tolist(), rows5.tolist()]


def box_cases(shape, dtype):
    """(name, image, mask): an empty mask, a mask touching each face, a single kept voxel, mask voxels at and below the fill value"""
    D, H, W = shape
    rng = np.random.default_rng(sum(shape))
    img = rng.integers(-1000, 2000, shape).astype(dtype)
    out = [("empty", img, np.zeros(shape, np.uint8)), ("full", img, np.full(shape, 3, np.uint8)), ("noise", img, MX.noise(shape, 0.4))]
    for f in range(6):
        m = np.zeros(shape, np.uint8)
        idx = [slice(s // 3, s // 3 + max(1, s // 4)) for s in shape]
        idx[f // 2] = slice(0, 1) if f % 2 == 0 else slice(shape[f // 2] - 1, shape[f // 2])
        m[tuple(idx)] = 1
        out.append((f"face {f}", img, m))
    one = np.zeros(shape, np.uint8)
    one[D // 2, H // 2, W - 1] = 1
    at_fill = np.full(shape, -1024, dtype)
    at_fill[0, 0, 0] = -1025
    at_fill[D // 2, H // 2, W - 1] = -1023                      # the one voxel above the fill value (it may be voxel 0)
    out.append(("single voxel", img, one))
    out.append(("at and below the fill value", at_fill, np.ones(shape, np.uint8)))
    low = img.copy()
    low[MX.noise(shape, 0.5, seed=4) == 1] = -1024
    low[MX.noise(shape, 0.2, seed=6) == 1] = -1500
    out.append(("mixed", low, MX.noise(shape, 0.6, seed=2)))
    if dtype is np.float32:
        nan = low.copy()
        nan[MX.noise(shape, 0.3, seed=7) == 1] = np.nan
        nan.flat[0] = np.float32(-0.0)
        nan.flat[-1] = np.inf
        out.append(("NaN and infinities", nan, MX.noise(shape, 0.7, seed=3)))
    return out


@pytest.mark.parametrize("shape", PC.SHAPES)
def test_mask_bbox_equals_the_restatement(shape):
    """both image kinds, in place and out of place: the masked image bit for bit and the box row equal"""
    assert hip.query("rpnet_prep_mask_bbox_workspace_bytes", *shape) == 64
    k = 0
    for dtype, _ in KINDS:
        for name, img, mask in box_cases(shape, dtype):
            k += 1
            for fill in (-1024, 0):
                src, m = dev(img), dev(mask)
                out = src if k % 2 else torch.full(img.shape, FILL, device=DEV, dtype=src.dtype)
                rows = torch.full((3, PP.BBOX_ROW), FILL, device=DEV, dtype=torch.int64)
                got = PP.mask_bbox(src, m, fill, out=out, rows=rows, row=1)
                want, row = PC.ref_mask_bbox(img, mask, fill)
                torch.cuda.synchronize()
                what = f"{shape} {dtype.__name__} {name} {fill}"
                assert got[0] is out and got[1] is rows and same_bits(out.cpu().numpy(), want), what
                assert rows.cpu().numpy().tolist() == [[FILL] * 8, row.tolist(), [FILL] * 8], (what, rows[1].tolist(), row.tolist())
                assert np.array_equal(m.cpu().numpy(), mask) and (k % 2 or same_bits(src.cpu().numpy(), img)), what
                if name == "empty":
                    assert row.tolist() == [-1] * 6 + [0, 0]
                if name == "single voxel" and fill == -1024:
                    assert row.tolist() == [shape[0] // 2] * 2 + [shape[1] // 2] * 2 + [shape[2] - 1] * 2 + [1, 1]
                if name == "at and below the fill value" and fill == -1024:
                    assert row[6] == 1 and row[7] == int(np.prod(shape))


def test_guard_words_graph_replay_and_repeatability():
    """calls through the C ABI with workspaces of exactly the size asked for and guard bytes behind them: a second identical call gives
    the same bits and the guard bytes hold; body_mask and the masking pass captured with torch.cuda.graph and replayed twice give
    identical bits, equal to the eager call and to the restatement"""
    shape = (10, 66, 130)
    D = shape[0]
    img = PC.noise_image(shape, np.float32, seed=3)
    lab = MX.noise(shape, 0.6)
    src, m_in = dev(img), dev(lab)
    p = hip.ptr
    needs = [hip.query(f"rpnet_prep_{e}_workspace_bytes", *shape) for e in ("threshold", "seeded_component", "mask_bbox")]
    wss = [torch.full((n + 64,), 0xA5, device=DEV, dtype=torch.uint8) for n in needs]
    mask, comp, masked = (torch.empty(shape, device=DEV, dtype=torch.uint8), torch.empty(shape, device=DEV, dtype=torch.uint8),
                          torch.empty(shape, device=DEV, dtype=torch.float32))
    rows_i = torch.full((D, 4), FILL, device=DEV, dtype=torch.int64)
    rows_f = torch.full((D, 3), float(FILL), device=DEV, dtype=torch.float64)
    stats = torch.full((D, 4), FILL, device=DEV, dtype=torch.int64)
    box = torch.full((2, 8), FILL, device=DEV, dtype=torch.int64)
    tensors = (mask, comp, masked, rows_i, rows_f, stats, box)

    def calls():
        hip.call("rpnet_prep_threshold", p(src), 0, p(mask), *shape, PP.OTSU, 0.0, p(rows_i), p(rows_f), p(wss[0]), needs[0])
        hip.call("rpnet_prep_seeded_component", p(m_in), p(comp), 1, *shape, 33, 65, 8, p(stats), p(wss[1]), needs[1])
        hip.call("rpnet_prep_mask_bbox", p(src), 0, p(comp), p(masked), -1024.0, *shape, p(box), 1, 2, p(wss[2]), needs[2])

    def snapshot():
        torch.cuda.synchronize()
        for ws, n in zip(wss, needs):
            assert (ws[n:] == 0xA5).all()
        assert wss[1][PP.OVERRUN_OFFSET:PP.OVERRUN_OFFSET + 4].view(torch.int32).item() == 0
        return [t.cpu().numpy().copy() for t in tensors]

    def refill():
        for t in tensors:
            t.fill_(FILL)

    calls()
    eager = snapshot()
    want_t = PC.ref_threshold(img)
    want_c = PC.ref_seeded(lab, 1, (33, 65), 8)
    want_b = PC.ref_mask_bbox(img, want_c[0])
    assert np.array_equal(eager[0], want_t[0]) and eager[3].tolist() == want_t[1].tolist() and same_bits(eager[4], want_t[2])
    assert np.array_equal(eager[1], want_c[0]) and eager[5].tolist() == want_c[1].tolist()
    assert same_bits(eager[2], want_b[0]) and eager[6].tolist() == [[FILL] * 8, want_b[1].tolist()]
    refill()
    calls()
    again = snapshot()
    for a, b in zip(eager, again):
        assert a.tobytes() == b.tobytes()

    # the public chain, captured: the caches hold their workspaces after the eager call
    phantom = PC.body_phantom((6, 96, 96))[0]
    vol = dev(phantom)
    want_m, want_tables = PC.ref_body_mask(phantom, radius=3)

    def chain():
        m, tables = PP.body_mask(vol, radius=3)
        out, rows = PP.mask_bbox(vol, m)
        return [m, out, rows] + [tables[k] for k in sorted(tables)]

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
    assert np.array_equal(first[0], want_m) and same_bits(first[1], PC.ref_mask_bbox(phantom, want_m)[0])
    assert first[2][0].tolist() == PC.ref_mask_bbox(phantom, want_m)[1].tolist()
    for k, got in zip(sorted(want_tables), first[3:]):
        assert same_bits(got, want_tables[k]), k


def test_refusals_launch_nothing():
    """every refusal of include/rpnet_prep_abi.h returns its status with a message; the outputs and the tables hold what they held"""
    shape = (5, 7, 9)
    n = int(np.prod(shape))
    img = dev(PC.noise_image(shape, np.float32))
    i16 = dev(PC.noise_image(shape, np.int16))
    m8 = dev(MX.noise(shape, 0.6))
    out8 = torch.full(shape, FILL, device=DEV, dtype=torch.uint8)
    outf = torch.full(shape, float(FILL), device=DEV, dtype=torch.float32)
    ti, tf = torch.full((5, 4), FILL, device=DEV, dtype=torch.int64), torch.full((5, 3), float(FILL), device=DEV, dtype=torch.float64)
    box = torch.full((3, 8), FILL, device=DEV, dtype=torch.int64)
    big = torch.zeros(4 * n + 64, device=DEV, dtype=torch.uint8)
    p = hip.ptr
    need = {e: hip.query(f"rpnet_prep_{e}_workspace_bytes", *shape) for e in ("threshold", "seeded_component", "mask_bbox")}
    ws = torch.empty(max(need.values()) + 16, device=DEV, dtype=torch.uint8)

    def thr(src=p(img), kind=0, dst=p(out8), dims=shape, mode=PP.OTSU, t=0.0, ri=p(ti), rf=p(tf), work=p(ws), nbytes=need["threshold"]):
        hip.call("rpnet_prep_threshold", src, kind, dst, *dims, mode, t, ri, rf, work, nbytes)

    def seed(src=p(m8), dst=p(out8), cls=1, dims=shape, sy=3, sx=4, conn=4, st=p(ti), work=p(ws), nbytes=need["seeded_component"]):
        hip.call("rpnet_prep_seeded_component", src, dst, cls, *dims, sy, sx, conn, st, work, nbytes)

    def bbox(src=p(img), kind=0, mask=p(m8), dst=p(outf), fill=-1024.0, dims=shape, rows=p(box), row=0, n_rows=3, work=p(ws),
             nbytes=need["mask_bbox"]):
        hip.call("rpnet_prep_mask_bbox", src, kind, mask, dst, fill, *dims, rows, row, n_rows, work, nbytes)

    for fn, nulls in ((thr, ("src", "dst", "ri", "rf", "work")), (seed, ("src", "dst", "st", "work")), (bbox, ("src", "mask", "dst", "rows", "work"))):
        for name in nulls:
            with pytest.raises(RuntimeError, match="null pointer"):
                fn(**{name: None})
        for dims in ((1025, 1, 1), (5, 1025, 9), (5, 7, 0)):
            with pytest.raises(RuntimeError, match="every extent 1..1024"):
                fn(dims=dims)
        with pytest.raises(RuntimeError, match="workspace of 48 bytes"):
            fn(nbytes=48)
        with pytest.raises(RuntimeError, match="aligned"):
            fn(work=p(ws) + 8)
    for e, fn in (("threshold", thr), ("seeded_component", seed)):
        with pytest.raises(RuntimeError, match=f"workspace of {need[e] - 1} bytes, {need[e]} needed"):
            fn(nbytes=need[e] - 1)
        for dims in ((1025, 1, 1), (5, 7, 0)):
            assert hip.query(f"rpnet_prep_{e}_workspace_bytes", *dims) == 0
            assert hip.load().rpnet_last_error_string().decode().startswith(f"prep_{e}: D=")
    for fn in (thr, bbox):
        for kind in (-1, 2, 3):
            with pytest.raises(RuntimeError, match=f"element kind {kind} "):
                fn(kind=kind)
    for mode in (-1, 2):
        with pytest.raises(RuntimeError, match=f"mode {mode} "):
            thr(mode=mode)
    with pytest.raises(RuntimeError, match="the threshold is NaN"):
        thr(mode=PP.FIXED, t=float("nan"))
    with pytest.raises(RuntimeError, match="mask overlaps img"):
        thr(src=p(big), dst=p(big) + 4 * n - 1)
    with pytest.raises(RuntimeError, match="aligned"):
        thr(src=p(img) + 2)
    with pytest.raises(RuntimeError, match="aligned"):
        thr(kind=1, src=p(i16) + 1)
    with pytest.raises(RuntimeError, match="aligned"):
        thr(rf=p(tf) + 4)
    for cls in (0, 256, -1):
        with pytest.raises(RuntimeError, match=f"class {cls} "):
            seed(cls=cls)
    for conn in (6, 26, 0, 5):
        with pytest.raises(RuntimeError, match=f"connectivity {conn} "):
            seed(conn=conn)
    for sy, sx in ((7, 4), (-1, 4), (3, 9), (3, -1)):
        with pytest.raises(RuntimeError, match="outside the 7 x 9 slice"):
            seed(sy=sy, sx=sx)
    with pytest.raises(RuntimeError, match="out overlaps in"):
        seed(src=p(big), dst=p(big) + 1)
    for row, n_rows in ((3, 3), (-1, 3), (0, 0)):
        with pytest.raises(RuntimeError, match=f"row {row} of a table of {n_rows} rows"):
            bbox(row=row, n_rows=n_rows)
    for fill in (float("nan"), float("inf"), 0.1):
        with pytest.raises(RuntimeError, match="is not a value of element kind 0"):
            bbox(fill=fill)
    for fill in (0.5, 40000.0, -32769.0, float("nan")):
        with pytest.raises(RuntimeError, match="is not a value of element kind 1"):
            bbox(kind=1, src=p(i16), fill=fill)
    with pytest.raises(RuntimeError, match="out overlaps img or mask"):
        bbox(src=p(big), dst=p(big) + 4)
    with pytest.raises(RuntimeError, match="out overlaps img or mask"):
        bbox(mask=p(big) + 4 * n - 1, dst=p(big))
    torch.cuda.synchronize()
    assert (out8 == FILL).all() and (outf == FILL).all() and (ti == FILL).all() and (tf == FILL).all() and (box == FILL).all()
    assert (big == 0).all()
    # the same calls with nothing wrong
    host = m8.cpu().numpy()
    seed(sy=0, sx=8, conn=8)
    torch.cuda.synchronize()
    want, rows = PC.ref_seeded(host, 1, (0, 8), 8)
    assert np.array_equal(out8.cpu().numpy(), want) and ti.cpu().numpy().tolist() == rows.tolist()
    bbox(kind=1, src=p(i16), dst=p(i16), fill=-5.0, row=2)
    torch.cuda.synchronize()
    want, row = PC.ref_mask_bbox(PC.noise_image(shape, np.int16), host, -5)
    assert same_bits(i16.cpu().numpy(), want) and box.cpu().numpy().tolist() == [[FILL] * 8] * 2 + [row.tolist()]
    thr(mode=PP.FIXED, t=-100.0)
    torch.cuda.synchronize()
    want = PC.ref_threshold(img.cpu().numpy(), -100.0)
    assert np.array_equal(out8.cpu().numpy(), want[0]) and ti.cpu().numpy().tolist() == want[1].tolist() and same_bits(tf.cpu().numpy(), want[2])
    # the Python layer refuses before the library is reached
    for bad, msg in (((7, 4), "seed must be"), ((3, 9), "seed must be")):
        with pytest.raises(ValueError, match=msg):
            PP.seeded_component(m8, (1,), seed=bad)
    with pytest.raises(ValueError, match="connectivity must be 4 or 8"):
        PP.seeded_component(m8, (1,), connectivity=6)
    with pytest.raises(ValueError, match="uint8"):
        PP.mask_bbox(img, img)
    with pytest.raises(ValueError, match="shape the body mask and a mask was handed in"):
        PP.clean_volume(img, mask=m8, radius=2)


def test_phantom_body_mask_and_clean_volume():
    """a body on a table: an ellipse with air pockets, a detached table bar and a speck.  body_mask and clean_volume == the restated
    chain, every table included; the table and the speck are gone, the pockets filled and the box tight; both crop modes; both kinds"""
    for dtype, radius in ((np.float32, 7), (np.int16, 1)):
        img, body, pockets, table, speck = PC.body_phantom((6, 96, 96), dtype)
        want_m, want_tables = PC.ref_body_mask(img, radius=radius)
        m, tables = PP.body_mask(dev(img), radius=radius)
        torch.cuda.synchronize()
        got = m.cpu().numpy()
        assert np.array_equal(got, want_m) and sorted(tables) == sorted(want_tables)
        for k in want_tables:
            assert same_bits(tables[k].cpu().numpy(), want_tables[k]), (k, tables[k].cpu().numpy().tolist(), want_tables[k].tolist())
        assert not got[table].any() and not got[speck].any() and got[pockets].all() and got[body].mean() > 0.97
        structures = {"Liver": (body & ~pockets).astype(np.uint8), "Table": table.astype(np.uint8) * 3}
        want_img, want_row = PC.ref_mask_bbox(img, want_m, -1024)
        ys, xs = np.nonzero(want_m.any(axis=0))
        assert want_row.tolist()[:6] == [0, 5, ys.min(), ys.max(), xs.min(), xs.max()] and want_row[6] == want_row[7] == want_m.sum()     # tight
        for reference_crop in (True, False):
            res = PP.clean_volume(dev(img), {k: dev(v) for k, v in structures.items()}, reference_crop=reference_crop, radius=radius)
            torch.cuda.synchronize()
            y0, y1, x0, x1 = PC.ref_crop(want_row, reference_crop)
            assert res["box"] == (y0, y1, x0, x1) and res["bbox"].cpu().numpy()[0].tolist() == want_row.tolist()
            assert same_bits(res["masked"].cpu().numpy(), want_img) and np.array_equal(res["mask"].cpu().numpy(), want_m)
            assert same_bits(res["image"].cpu().numpy(), want_img[:, y0:y1, x0:x1]) and res["image"].shape[0] == 6
            for k, v in structures.items():
                assert np.array_equal(res["structures"][k].cpu().numpy(), v[:, y0:y1, x0:x1]), k
            assert same_bits(res["tables"]["voxels"].cpu().numpy(), want_tables["voxels"])
        assert res["image"].shape[1] == ys.max() - ys.min() + 1 and res["image"].shape[2] == xs.max() - xs.min() + 1
    # a mask handed in; a fixed threshold; an empty box raises
    res = PP.clean_volume(dev(img), mask=dev(want_m), fill=-1024)
    assert res["tables"] is None and same_bits(res["masked"].cpu().numpy(), want_img)
    m, _ = PP.body_mask(dev(img), radius=2, threshold=-500)
    assert np.array_equal(m.cpu().numpy(), PC.ref_body_mask(img, radius=2, threshold=-500)[0])
    with pytest.raises(ValueError, match="the box is empty"):
        PP.clean_volume(dev(np.full((2, 20, 20), -1024, np.int16)))


def test_driver_end_to_end(tmp_path, capsys):
    """tools/preprocess_volumes.py (one clean_volume per volume) on two phantoms written as NRRD in the raw layout (axes x, y, z) with an anisotropic spacing: the files
    load through FewshotVolumeReader, volume_spacing returns the input spacing, the bbox file has the reference's form, both crop modes"""
    from rpnet_amd.utils import nrrd
    from rpnet_amd.utils.volume_reader import FewshotVolumeReader
    from tools import preprocess_volumes as TP
    raw = tmp_path / "raw"
    spacing = (2.5, 0.8, 0.7)                                       # (sz, sy, sx)
    phantoms = {}
    for i, pid in enumerate(("p0", "p1")):
        img, body, pockets, table, speck = PC.body_phantom((6, 96, 96), np.int16, seed=i)
        organ = np.zeros(img.shape, np.uint8)
        organ[1:5, 30:50, 35:60] = 1
        phantoms[pid] = (img, organ)
        os.makedirs(raw / pid / "structures")
        hdr = {"space": "left-posterior-superior", "space directions": f"({spacing[2]!r},0,0) (0,{spacing[1]!r},0) (0,0,{spacing[0]!r})"}
        nrrd.write(str(raw / pid / "img.nrrd"), np.swapaxes(img, 0, -1), header=hdr)
        nrrd.write(str(raw / pid / "structures" / "Liver.nrrd"), np.swapaxes(organ, 0, -1), header=hdr)
    for inclusive in (False, True):
        save = tmp_path / ("inclusive" if inclusive else "reference")
        results = TP.main(["--raw-dir", str(raw), "--save-dir", str(save), "--radius", "3", "--rois", "Liver", "Kidney L"]
                          + (["--inclusive-crop"] if inclusive else []))
        lines = capsys.readouterr().out.strip().split("\n")
        assert [r["pid"] for r in results] == ["p0", "p1"] and sum("does not have Kidney L" in ln for ln in lines) == 2
        split = tmp_path / f"split{int(inclusive)}"
        os.makedirs(split / "classes")
        (split / "all.csv").write_text("p0\np1\n")
        (split / "classes" / "Liver.csv").write_text("pid,z_start,z_end\np0,1,4\np1,1,4\n")
        cfg = {"class_csv_dir": str(split / "classes"), "train_classes": ["Liver"], "eval_classes": ["Liver"], "n_shot": 1, "n_way": 1, "num_slice": 6,
               "num_x": 96, "num_y": 96, "pad_value": -1024, "HU_range": [-1024, 3076], "crop_size": [96, 96], "do_elastic": False}
        reader = FewshotVolumeReader(str(save), str(split / "all.csv"), cfg, mode="eval")
        for pid, (img, organ) in phantoms.items():
            want_m, tables = PC.ref_body_mask(img, radius=3)
            want_img, row = PC.ref_mask_bbox(img, want_m, -1024)
            y0, y1, x0, x1 = PC.ref_crop(row, not inclusive)
            clean, header = nrrd.read(str(save / f"{pid}_clean.nrrd"))
            assert same_bits(clean, want_img[:, y0:y1, x0:x1]) and header["type"] == "int16"
            liver, _ = nrrd.read(str(save / f"{pid}_Liver.nrrd"))
            assert liver.dtype == np.uint8 and np.array_equal(liver, organ[:, y0:y1, x0:x1])
            bbox = np.load(str(save / f"{pid}_bbox.npy"))
            assert bbox.tolist() == [[0, y0, x0], [6, y1, x1]]
            assert bbox[1].tolist() == ([6, row[3], row[5]] if not inclusive else [6, row[3] + 1, row[5] + 1])    # the reference's yy.max(), xx.max()
            assert reader.volume_spacing(pid) == spacing
            assert not os.path.exists(save / f"{pid}_Kidney L.nrrd")
            line = [ln for ln in lines if ln.startswith(pid + " (")][0]
            assert f"box y {y0}:{y1} x {x0}:{x1}" in line and all(f"{s} {v}" in line for s, v in zip(PP.STAGES, tables["voxels"].tolist()))
        item = reader[0]
        assert item["query_images"][0][0].shape[-2:] == (96, 96) and item["query_labels"][0][0].sum() > 0
