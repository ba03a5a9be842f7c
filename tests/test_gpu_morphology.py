"""rpnet_morph_apply and rpnet_morph_apply_spacing (csrc/morph.hip), rpnet_amd.morphology and the opening / closing stages of the
clean-up chain of VolumeSegmenter on the MI355X.

Every comparison is exact equality with tests/morphology_cases.py:ref_apply (numpy: the ball offset by offset, an explicit OR / AND over
shifted copies; pinned to scipy.ndimage by tests/test_host_morphology.py): results, statistics rows and counts rows.  There is no
tolerance."""
import numpy as np
import pytest
import torch

from rpnet_amd import hip
from rpnet_amd import morphology as MO
from tests import morphology_cases as MX

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 7


def dev(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(DEV)


def table(rows, cols):
    return torch.full((rows, cols), FILL, device=DEV, dtype=torch.int64)


def check(vol, op, radius, what, truth=None, in_place=False, cls=1, want=None, **kw):
    """one public call on one class == the restatement: the result, the statistics row and the counts row (added to FILL); the input
    untouched out of place -> (result on the host, statistics row)"""
    src = dev(vol)
    out = src if in_place else torch.full(vol.shape, FILL, device=DEV, dtype=torch.uint8)
    counts = None if truth is None else table(1, MO.COUNTS_ROW)
    stats = table(1, MO.STATS_ROW)
    fn = {MX.ERODE: MO.erode, MX.DILATE: MO.dilate, MX.OPEN: MO.opening, MX.CLOSE: MO.closing}[op]
    got = fn(src, (cls,), radius, truth=None if truth is None else dev(truth), out=out, counts=counts, stats=stats, **kw)
    want, row = want if want is not None else MX.ref_apply(vol, cls, op, radius, **kw)
    torch.cuda.synchronize()
    assert got[0] is out and got[1] is counts and got[2] is stats
    res = out.cpu().numpy()
    assert np.array_equal(res, want), (what, int((res != want).sum()))
    if not in_place:
        assert np.array_equal(src.cpu().numpy(), vol), what
    assert stats.cpu().numpy()[0].tolist() == row.tolist(), (what, stats.cpu().numpy()[0].tolist(), row.tolist())
    if truth is not None:
        assert (counts.cpu().numpy()[0] - FILL).tolist() == MX.ref_counts(want, truth, cls).tolist(), what
    return res, row


# the ball of every shape of the table: a small and a larger voxel ball under either border rule, the millimetre ball, per slice
CONFIGS = [dict(radius=("rho", 2)), dict(radius=("rho", 5), erode_border=0), dict(radius=(5.0, "mm"), spacing=MX.MM),
           dict(radius=("rho", 4), per_slice=True), dict(radius=(2.4, "mm"), spacing=MX.MM, per_slice=True, erode_border=0)]


@pytest.mark.parametrize("shape", MX.ONE + MX.LINES + MX.TILES_VOX + MX.TILES_MM + MX.LIMIT + MX.SMALL)
def test_every_shape_equals_the_restatement(shape):
    """one voxel, each axis of length 1, one column more than a tile and two more than two tiles for both metrics' tile widths, a line
    of 1024 along each axis, the 513-long line of the 64 KiB fp64 tile: every operation under every ball of CONFIGS, on noise, on
    blocks in the corners and on the full volume, alternately out of place without a truth and in place with one"""
    assert hip.query("rpnet_morph_workspace_bytes", *shape) == 64 + (8 * int(np.prod(shape)) + 15) // 16 * 16 + 2 * ((int(np.prod(shape)) + 15) // 16 * 16)
    truth = MX.noise(shape, 0.5, seed=9)
    k = 0
    for name in ("noise 0.31", "corners", "full"):
        vol = dict(MX.contents(shape))[name]
        for op in MX.OPS:
            for kw in CONFIGS:
                k += 1
                check(vol, op, kw["radius"], f"{shape} {name} {MX.OP_NAMES[op]} {kw}", truth=truth if k % 2 else None, in_place=bool(k % 2),
                      **{a: b for a, b in kw.items() if a != "radius"})


def test_borders_and_contents():
    """objects touching each face and corner, noise at three densities, a box, full and empty, under both erode_border values, 3D and
    per slice (against the 2D restatement of every slice), for both balls"""
    shape = MX.SMALL[0]
    rows = {}
    for name, vol in MX.contents(shape):
        for op in MX.OPS:
            for per_slice in (False, True):
                for b in (0, 1):
                    for radius, spacing in ((("rho", 3), None), (1, None), ((2.5, "mm"), MX.MM)):
                        _, row = check(vol, op, radius, f"{name} {MX.OP_NAMES[op]} {per_slice} {b} {radius}", spacing=spacing, per_slice=per_slice,
                                       erode_border=b)
                        rows[(name, op, per_slice, b, radius)] = row.tolist()
    n = int(np.prod(shape))
    assert rows[("full", MX.ERODE, False, 1, 1)] == [n, n, 0, 0] and rows[("full", MX.ERODE, False, 0, 1)] == [n, 4 * 7 * 8, 0, n - 4 * 7 * 8]
    assert rows[("full", MX.ERODE, True, 0, 1)] == [n, 6 * 7 * 8, 0, n - 6 * 7 * 8] and rows[("empty", MX.DILATE, False, 1, 1)] == [0, 0, 0, 0]
    assert rows[("face 0", MX.CLOSE, False, 1, ("rho", 3))][3] == 0 and rows[("face 0", MX.CLOSE, False, 0, ("rho", 3))][3] > 0


def test_ball_larger_than_the_volume():
    """rho above the squared diagonal: one voxel dilates to everything; with erode_border=0 everything erodes, with 1 only a full
    volume survives; the largest accepted rho and a millimetre radius beyond the volume do the same"""
    shape = (4, 5, 6)
    n = int(np.prod(shape))
    one = np.zeros(shape, np.uint8)
    one[1, 2, 3] = 1
    full = np.ones(shape, np.uint8)
    for radius, spacing in ((("rho", 200), None), (("rho", MO.MAX_RHO), None), (40, None), ((100.0, "mm"), MX.MM)):
        assert check(one, MX.DILATE, radius, "dilate", spacing=spacing)[1].tolist() == [1, n, n - 1, 0]
        assert check(one, MX.CLOSE, radius, "close", spacing=spacing)[1].tolist() == [1, n, n - 1, 0]
        assert check(full, MX.ERODE, radius, "erode 1", spacing=spacing)[1].tolist() == [n, n, 0, 0]
        assert check(full, MX.ERODE, radius, "erode 0", spacing=spacing, erode_border=0)[1].tolist() == [n, 0, 0, n]
        assert check(full, MX.OPEN, radius, "open 0", spacing=spacing, erode_border=0)[1].tolist() == [n, 0, 0, n]
        full[0, 0, 0] = 0
        assert check(full, MX.ERODE, radius, "erode holed", spacing=spacing)[1].tolist() == [n - 1, 0, 0, n - 1]
        full[0, 0, 0] = 1
        res, _ = check(one, MX.DILATE, radius, "dilate per slice", spacing=spacing, per_slice=True)
        assert res[1].all() and not res[0].any() and not res[2:].any()


def test_ties_at_the_threshold():
    """voxel ball: from one object voxel, the voxels at squared distance exactly rho are gained and those at rho + 1 are not, along an
    axis, a face diagonal and a space diagonal, and the ball one smaller loses them; millimetre ball: r = 3 * 0.8 under spacing 0.8,
    where the rounded products decide, bracketed by radii just below and above"""
    for rho, kind in MX.TIES:
        vol = MX.ties(rho, kind)
        c = vol.shape[0] // 2
        k = {"axis": (int(round(rho ** 0.5)), 0, 0), "face": (int(round((rho / 2) ** 0.5)),) * 2 + (0,), "space": (int(round((rho / 3) ** 0.5)),) * 3}[kind]
        at, _ = check(vol, MX.DILATE, ("rho", rho), f"ties {rho} {kind}")
        below, _ = check(vol, MX.DILATE, ("rho", rho - 1), f"ties {rho - 1} {kind}")
        for perm in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
            o = tuple(k[p] for p in perm)
            assert sum(v * v for v in o) == rho and at[c + o[0], c + o[1], c + o[2]] == 1 and at[c - o[0], c - o[1], c - o[2]] == 1
            assert below[c + o[0], c + o[1], c + o[2]] == 0
            far = list(o)
            far[([i for i, v in enumerate(o) if v == 0] or [0])[0]] += 1           # rho + 1 where a coordinate is 0
            assert sum(v * v for v in far) > rho and at[c + far[0], c + far[1], c + far[2]] == 0
        inv = (1 - vol).astype(np.uint8)
        for op in (MX.ERODE, MX.OPEN, MX.CLOSE):
            check(inv, op, ("rho", rho), f"ties inverse {rho} {kind}")
            check(inv, op, ("rho", rho + 1), f"ties inverse {rho + 1} {kind}")
    vol = MX.ties(16, "axis")
    for spacing in ((0.8, 0.8, 0.8), MX.MM, (0.8, 2.5, 0.8)):
        for r in (3 * 0.8, np.nextafter(3 * 0.8, 0.0), np.nextafter(3 * 0.8, 9.0), 2.39, 2.41, 0.8, 0.79):
            for op in MX.OPS:
                check(vol if op == MX.DILATE else MX.noise(vol.shape, 0.6), op, (float(r), "mm"), f"mm ties {spacing} {r!r} {op}", spacing=spacing)


def test_label_volumes_and_element_kinds():
    """a label volume with another class adjacent to and inside what the closing of class 1 gains; every element kind of the input and
    of the truth; in place and out of place; two classes processed in sequence equal the restatement applied class by class, the
    second reading the result of the first; counts are added to what the rows hold"""
    lab, truth = MX.labels((6, 33, 65)), MX.labels((6, 33, 65), seed=11)
    for kind, tk in ((np.uint8, np.int32), (np.int32, np.int64), (np.int64, np.float32), (np.float32, np.uint8)):
        for op in MX.OPS:
            for cls in (1, 3):
                res, row = check(lab.astype(kind), op, ("rho", 3), f"{kind} {op} {cls}", truth=truth.astype(tk), cls=cls,
                                 in_place=kind is np.uint8 and op % 2 == 0)
                assert np.array_equal(res[(lab != cls) & (lab != 0)], lab[(lab != cls) & (lab != 0)])
    _, row = check(lab, MX.CLOSE, ("rho", 3), "closing over classes")
    gain = MX.binary_ref(lab == 1, MX.CLOSE, MX.voxel_ball(3, lab.shape)) & (lab != 1)
    assert 0 < row[2] == int((gain & (lab == 0)).sum()) < int(gain.sum())
    for fn, op, kw in ((MO.closing, MX.CLOSE, dict(radius=("rho", 2))), (MO.opening, MX.OPEN, dict(radius=(2.5, "mm"), spacing=MX.MM)),
                       (MO.dilate, MX.DILATE, dict(radius=1, per_slice=True)), (MO.erode, MX.ERODE, dict(radius=1.5, erode_border=0))):
        want, rows = lab, []
        for cls in (2, 1, 3):
            want, row = MX.ref_apply(want, cls, op, **kw)
            rows.append(row.tolist())
        counts = torch.full((3, MO.COUNTS_ROW), 5, device=DEV, dtype=torch.int64)
        out, counts, stats = fn(dev(lab), (2, 1, 3), truth=dev(truth), counts=counts, **kw)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want) and stats.cpu().numpy().tolist() == rows, kw
        assert (counts.cpu().numpy() - 5).tolist() == [MX.ref_counts(want, truth, c).tolist() for c in (2, 1, 3)]
    out, counts, stats = MO.closing(dev(lab), (1,), 2)
    assert counts is None and out.dtype == torch.uint8 and stats.shape == (1, 4)
    with pytest.raises(ValueError, match="uint8, int32, int64 and float32"):
        MO.closing(dev(lab.astype(np.float64)), (1,), 2)
    with pytest.raises(ValueError, match="counts need a truth"):
        MO.opening(dev(lab), (1,), 2, counts=table(1, 3))
    with pytest.raises(ValueError, match="a radius in mm needs a spacing"):
        MO.opening(dev(lab), (1,), (2.0, "mm"))


def test_graph_replay_guard_words_and_repeatability():
    """calls through the C ABI with a workspace of exactly the size asked for, guard bytes behind it: a second identical call gives the
    same bits; captured with torch.cuda.graph and replayed twice they give identical bits, equal to the eager call and to the
    restatement; the guard bytes and the other rows of the tables hold what they held"""
    import ctypes
    shape = (10, 66, 130)
    vol, truth = MX.noise(shape, 0.31), MX.noise(shape, 0.5, seed=9)
    src, tr = dev(vol), dev(truth)
    need = hip.query("rpnet_morph_workspace_bytes", *shape)
    ws = torch.full((need + 64,), 0xA5, device=DEV, dtype=torch.uint8)
    outs = [torch.empty(shape, device=DEV, dtype=torch.uint8) for _ in range(4)]
    stats, counts = table(5, MO.STATS_ROW), table(5, MO.COUNTS_ROW)
    p = hip.ptr
    w = (ctypes.c_double * 3)(*MO.resolve_radius((2.5, "mm"), MX.MM)[1])

    def calls():
        hip.call("rpnet_morph_apply", p(src), 0, p(outs[0]), 1, *shape, MX.CLOSE, 9, 0, 1, p(tr), 0, p(counts), 0, p(stats), 0, 5, p(ws), need)
        hip.call("rpnet_morph_apply", p(src), 0, p(outs[1]), 1, *shape, MX.OPEN, 2, 1, 0, p(tr), 0, p(counts), 2, p(stats), 2, 5, p(ws), need)
        hip.call("rpnet_morph_apply_spacing", p(src), 0, p(outs[2]), 1, *shape, MX.ERODE, w, 2.5 * 2.5, 0, 1, p(tr), 0, p(counts), 3, p(stats), 3,
                 5, p(ws), need)
        hip.call("rpnet_morph_apply_spacing", p(src), 0, p(outs[3]), 1, *shape, MX.DILATE, w, 2.5 * 2.5, 0, 1, None, 0, None, 0, p(stats), 4, 5,
                 p(ws), need)

    def snapshot():
        torch.cuda.synchronize()
        assert (ws[need:] == 0xA5).all()
        return [t.cpu().numpy().copy() for t in (*outs, stats, counts)]

    def refill():
        for t in (*outs, stats, counts):
            t.fill_(FILL)

    calls()
    eager = snapshot()
    wants = [MX.ref_apply(vol, 1, MX.CLOSE, ("rho", 9)), MX.ref_apply(vol, 1, MX.OPEN, ("rho", 2), per_slice=True, erode_border=0),
             MX.ref_apply(vol, 1, MX.ERODE, (2.5, "mm"), MX.MM), MX.ref_apply(vol, 1, MX.DILATE, (2.5, "mm"), MX.MM)]
    for got, (want, _) in zip(eager, wants):
        assert np.array_equal(got, want)
    assert eager[4].tolist() == [wants[0][1].tolist(), [FILL] * 4, wants[1][1].tolist(), wants[2][1].tolist(), wants[3][1].tolist()]
    assert (eager[5] - FILL).tolist() == [MX.ref_counts(wants[0][0], truth).tolist(), [0] * 3, MX.ref_counts(wants[1][0], truth).tolist(),
                                          MX.ref_counts(wants[2][0], truth).tolist(), [0] * 3]
    refill()
    calls()
    again = snapshot()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        calls()
    runs = []
    for _ in range(2):
        refill()
        graph.replay()
        runs.append(snapshot())
    for a, b, c, d in zip(eager, again, runs[0], runs[1]):
        assert a.tobytes() == b.tobytes() == c.tobytes() == d.tobytes()


def test_refusals_launch_nothing():
    """every refusal of include/rpnet_morph_abi.h returns its status with a message; the output and the tables hold what they held"""
    import ctypes
    shape = (5, 7, 9)
    host = MX.noise(shape, 0.6)
    vol = dev(host)
    vol32 = vol.to(torch.int32)
    out = torch.full(shape, FILL, device=DEV, dtype=torch.uint8)
    stats, counts = table(3, MO.STATS_ROW), table(3, MO.COUNTS_ROW)
    p = hip.ptr
    need = hip.query("rpnet_morph_workspace_bytes", *shape)
    ws = torch.empty(need + 16, device=DEV, dtype=torch.uint8)

    def vox(src=p(vol), kind=0, dst=p(out), cls=1, dims=shape, op=MX.CLOSE, rho=2, per_slice=0, border=1, truth=p(vol), tk=0, cnt=p(counts),
            crow=0, st=p(stats), srow=0, work=p(ws), nbytes=need):
        hip.call("rpnet_morph_apply", src, kind, dst, cls, *dims, op, rho, per_slice, border, truth, tk, cnt, crow, st, srow, 3, work, nbytes)

    def mm(src=p(vol), kind=0, dst=p(out), cls=1, dims=shape, op=MX.CLOSE, w=(6.25, 0.64, 0.64), r2=4.0, per_slice=0, border=1, truth=p(vol),
           tk=0, cnt=p(counts), crow=0, st=p(stats), srow=0, work=p(ws), nbytes=need):
        wp = None if w is None else (ctypes.c_double * 3)(*w)
        hip.call("rpnet_morph_apply_spacing", src, kind, dst, cls, *dims, op, wp, r2, per_slice, border, truth, tk, cnt, crow, st, srow, 3, work,
                 nbytes)

    for fn in (vox, mm):
        for kw in (dict(src=None), dict(dst=None), dict(st=None), dict(work=None)):
            with pytest.raises(RuntimeError, match="null pointer"):
                fn(**kw)
        with pytest.raises(RuntimeError, match="kinds 4, 0"):
            fn(kind=4)
        with pytest.raises(RuntimeError, match="kinds 0, 7"):
            fn(tk=7)
        for op in (-1, 4):
            with pytest.raises(RuntimeError, match=f"op {op} "):
                fn(op=op)
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
            assert hip.query("rpnet_morph_workspace_bytes", *dims) == 0
            assert hip.load().rpnet_last_error_string().decode().startswith("morph: D=")
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
    for rho in (0, -5, MO.MAX_RHO + 1):
        with pytest.raises(RuntimeError, match=f"rho {rho} "):
            vox(rho=rho)
    with pytest.raises(RuntimeError, match="null pointer"):
        mm(w=None)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        for at in range(3):
            w = [6.25, 0.64, 0.64]
            w[at] = bad
            with pytest.raises(RuntimeError, match=f"weight {at} is"):
                mm(w=w)
        with pytest.raises(RuntimeError, match="r2 is"):
            mm(r2=bad)
    assert hip.load().rpnet_last_error_string().decode().startswith("morph_apply_spacing: r2 is inf")
    torch.cuda.synchronize()
    assert (out == FILL).all() and (stats == FILL).all() and (counts == FILL).all()
    assert np.array_equal(vol32.cpu().numpy(), host) and np.array_equal(vol.cpu().numpy(), host)
    # the same calls with nothing wrong, without truth and counts
    vox(truth=None, cnt=None, srow=1, op=MX.OPEN, rho=3, border=0)
    torch.cuda.synchronize()
    want, row = MX.ref_apply(host, 1, MX.OPEN, ("rho", 3), erode_border=0)
    assert np.array_equal(out.cpu().numpy(), want) and stats[1].tolist() == row.tolist()
    mm(truth=None, cnt=None, srow=2, op=MX.DILATE, per_slice=1, w=MO.resolve_radius((2.0, "mm"), MX.MM)[1])
    torch.cuda.synchronize()
    want, row = MX.ref_apply(host, 1, MX.DILATE, (2.0, "mm"), MX.MM, per_slice=True)
    assert np.array_equal(out.cpu().numpy(), want) and stats[2].tolist() == row.tolist()
    assert (stats[0] == FILL).all() and (counts == FILL).all()


# ------------------------------------------------------------------------------------------------ end to end
def _chain_by_hand(mask, opening=None, closing=None, per_slice=False, spacing=None, m=None, conn=None, holes=False):
    """open -> remove small -> keep largest -> close -> fill holes, each stage that is on, by the host restatements -> (end, rows)"""
    from tests import components_cases as CX
    from tests import postprocess_cases as PX
    rows, s = {}, mask
    if opening is not None:
        s, rows["opening"] = MX.ref_apply(s, 1, MX.OPEN, opening, spacing, per_slice)
    if m is not None:
        s, rows["small"] = PX.ref_remove_small(s, 1, conn or 6, m)
    if conn:
        rows["largest"] = CX.ref_stats(s, 1, conn)
        s = CX.ref_keep_largest(s, 1, conn)
    if closing is not None:
        s, rows["closing"] = MX.ref_apply(s, 1, MX.CLOSE, closing, spacing, per_slice)
    if holes:
        s, rows["holes"] = PX.ref_fill_holes(s, 1, 6)
    return s, rows


def test_volume_segmenter_morphology():
    """a 64^2 net with T = 2, a volume of 5 slices at batch 2, f32 convolutions.  With opening and closing None the result equals, byte
    for byte and key for key, that of a VolumeSegmenter made without naming them.  With the stages on, eager and graphed, post['mask'] is
    the host restatements chained by hand in the fixed order open -> remove small -> keep largest -> close -> fill holes, the figures are
    those of each stage on its own input, counts / dice describe the end of the chain, and morph_stats_out takes the two rows."""
    import rpnet_amd.functional as RF
    from rpnet_amd import postprocess as PP
    from rpnet_amd.volume import VolumeSegmenter, dice_from_counts
    from tests.test_gpu_volume import build_net, eval_cfg, reader, segment
    RF.set_conv_math("f32")              # restored by tests/conftest.py
    cfg = eval_cfg()
    cfg["n_iter_refinement"] = 2
    item = reader(cfg, 5, 64)[0]
    net = build_net(cfg)
    labels = item["query_labels"].numpy()
    plain = segment(VolumeSegmenter(net, batch=2, graphed=False, keep_largest=26, fill_holes=True), item)
    off = segment(VolumeSegmenter(net, batch=2, graphed=False, keep_largest=26, fill_holes=True, opening=None, closing=None, morph_per_slice=False),
                  item)
    assert torch.equal(off.mask, plain.mask) and off.counts.tobytes() == plain.counts.tobytes() and off.dice == plain.dice
    assert list(off.post) == list(plain.post) and torch.equal(off.post["mask"], plain.post["mask"])
    assert off.post["counts"].tobytes() == plain.post["counts"].tobytes() and off.post["holes"] == plain.post["holes"]
    assert segment(VolumeSegmenter(net, batch=2, graphed=False, opening=None, closing=None), item).post is None
    mask = plain.mask.cpu().numpy()
    assert mask.any(), "the synthetic episode predicts an organ"
    for graphed in (False, True):
        for kw, hand in ((dict(opening=1, closing=("rho", 5), keep_largest=26, fill_holes=True, min_component=3),
                          dict(opening=1, closing=("rho", 5), conn=26, holes=True, m=3)),
                         (dict(opening=(2.0, "mm"), closing=(3.0, "mm"), spacing=(2.5, 0.8, 0.8), keep_largest=6),
                          dict(opening=(2.0, "mm"), closing=(3.0, "mm"), spacing=(2.5, 0.8, 0.8), conn=6)),
                         (dict(closing=2, morph_per_slice=True), dict(closing=2, per_slice=True)), (dict(opening=1.5), dict(opening=1.5))):
            res = segment(VolumeSegmenter(net, batch=2, graphed=graphed, **kw), item)
            base = res.mask.cpu().numpy()           # a graphed run describes its own mask
            assert graphed or (np.array_equal(base, mask) and res.counts.tobytes() == plain.counts.tobytes() and res.dice == plain.dice)
            end, rows = _chain_by_hand(base, **hand)
            assert np.array_equal(res.post["mask"].cpu().numpy(), end), (graphed, kw)
            assert ("opening" in res.post and "closing" in res.post), kw
            assert res.post["opening"] == (MO.morph_figures(rows["opening"]) if "opening" in rows else None), kw
            assert res.post["closing"] == (MO.morph_figures(rows["closing"]) if "closing" in rows else None), kw
            if "holes" in rows:
                assert res.post["holes"] == PP.holes_figures(rows["holes"]) and res.post["small"] == PP.small_figures(rows["small"])
            else:
                assert "holes" not in res.post and "small" not in res.post
            assert res.post["counts"].tolist() == [MX.ref_counts(end, labels).tolist()] and res.post["dice"] == dice_from_counts(res.post["counts"])
    # the caller's tables, eager and graphed
    args = (item["support_images"], item["support_labels"], item["query_images"], item["appr_query_labels"])
    for graphed in (False, True):
        seg = VolumeSegmenter(net, batch=2, graphed=graphed, opening=1, closing=2, keep_largest=26)
        tabs, wide = (torch.zeros((1, 3), device=DEV, dtype=torch.int64), table(1, 4)), table(1, 8)
        out = seg(*args, item["query_labels"], post_out=tabs, morph_stats_out=wide)
        end, rows = _chain_by_hand(out.mask.cpu().numpy(), opening=1, closing=2, conn=26)
        assert np.array_equal(out.post["mask"].cpu().numpy(), end) and all(out.post[k] is None for k in out.post if k != "mask")
        assert tabs[0].cpu().numpy().tolist() == [MX.ref_counts(end, labels).tolist()] and tabs[1].cpu().numpy().tolist() == [rows["largest"].tolist()]
        assert wide.cpu().numpy().tolist() == [rows["opening"].tolist() + rows["closing"].tolist()]
    seg = VolumeSegmenter(net, batch=2, graphed=False, closing=2)
    wide = table(1, 8)
    seg(*args, item["query_labels"], post_out=(torch.zeros((1, 3), device=DEV, dtype=torch.int64), table(1, 4)), morph_stats_out=wide)
    assert (wide[:, :4] == FILL).all() and wide[0, 4].item() >= 0 and wide[0, 7].item() == 0
    with pytest.raises(ValueError, match="morph_stats_out needs post_out"):
        seg(*args, item["query_labels"], morph_stats_out=wide)
    with pytest.raises(ValueError, match="morph_stats_out must be a contiguous int64 \\[1, 8\\]"):
        seg(*args, item["query_labels"], post_out=(torch.zeros((1, 3), device=DEV, dtype=torch.int64), table(1, 4)), morph_stats_out=table(1, 4))
    with pytest.raises(ValueError, match="radius in mm needs a spacing"):
        VolumeSegmenter(net, batch=2, graphed=False, closing=(2.0, "mm"))(*args, item["query_labels"])
    with pytest.raises(ValueError, match="radius must be"):
        VolumeSegmenter(net, batch=2, graphed=False, opening=0)
    with pytest.raises(ValueError, match="morph_per_slice needs opening or closing"):
        VolumeSegmenter(net, batch=2, graphed=False, morph_per_slice=True)


def test_evaluate_dataset_morphology(tmp_path, capsys):
    """a synthetic NRRD set with spacing (2.5, 0.8, 0.8) in its headers, f32 convolutions, eager.  With the options named at their
    defaults every printed character, table and dictionary is that of a call that does not know them.  With opening (voxels) and closing
    (mm, resolved from each header) around keep_largest, the dictionaries and earlier tables do not change, every line is the plain line
    plus the documented suffixes, out["morph_stats"] equals the chain by hand on the plain run's saved masks, and save_pred holds the end
    of the chain."""
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
    dirs = {k: str(tmp_path / k) for k in ("plain", "off", "morph")}
    runs = {}
    for name, kw in (("plain", {}), ("off", dict(opening=None, closing=None, morph_per_slice=False)),
                     ("morph", dict(keep_largest=26, opening=1, closing=(3.0, "mm"), spacing="header"))):
        random.seed(77)
        capsys.readouterr()
        tabs = {}
        dicts = _plain(DE.evaluate_dataset(_build_net(cfg, "f32"), src, cfg, batch=8, graphed=False, out=tabs, save_pred=dirs[name], **kw))
        runs[name] = (dicts, tabs, capsys.readouterr().out)
    (d0, t0, o0), (d1, t1, o1), (d2, t2, o2) = (runs[k] for k in ("plain", "off", "morph"))
    assert o1 == o0 and d1 == d0 and sorted(t1) == sorted(t0) == ["counts", "ncc"] and all(t1[k].tobytes() == t0[k].tobytes() for k in t0)
    assert d2 == d0 and all(t2[k].tobytes() == t0[k].tobytes() for k in t0)
    assert sorted(t2) == ["components", "counts", "morph_stats", "ncc", "post_counts"]
    assert t2["morph_stats"].shape == (3, 1, 8) and t2["morph_stats"].dtype == np.int64
    l0, l2 = _driver_lines(o0), _driver_lines(o2)
    assert len(l0) == len(l2) == 4
    figs = {k: [] for k in ("dice", "lcc", "open", "close")}
    random.seed(77)
    for j in range(3):
        s = src.item(j)
        labels = s["query_labels"].cpu().numpy()
        mask, _ = nrrd.read(os.path.join(dirs["plain"], f"{s['pid']}_Liver.nrrd"))
        same, _ = nrrd.read(os.path.join(dirs["off"], f"{s['pid']}_Liver.nrrd"))
        assert np.array_equal(same, mask)
        end, rows = _chain_by_hand(mask, opening=1, closing=(3.0, "mm"), spacing=MM, conn=26)
        got, _ = nrrd.read(os.path.join(dirs["morph"], f"{s['pid']}_Liver.nrrd"))
        assert np.array_equal(got, end), j
        assert t2["morph_stats"][j, 0].tolist() == rows["opening"].tolist() + rows["closing"].tolist(), j
        assert t2["components"][j, 0].tolist() == rows["largest"].tolist() and t2["post_counts"][j, 0].tolist() == MX.ref_counts(end, labels).tolist()
        d, lcc = dice_from_counts(t2["post_counts"][j])[0], CC.components_figures(t2["components"][j])[0]
        op, cl = MO.morph_figures(rows["opening"])[0], MO.morph_figures(rows["closing"])[0]
        assert l2[j] == (l0[j] + f" lcc {d} ({lcc['n_components']} components, {lcc['removed']} voxels removed)"
                         + f" open -{op['removed']} +{op['added']} close -{cl['removed']} +{cl['added']}"), j
        for k, v in (("dice", d), ("lcc", lcc), ("open", op), ("close", cl)):
            figs[k].append(v)
    assert l2[3] == l0[3] + CC.mean_suffix(figs["dice"], figs["lcc"]) + MO.mean_suffix(figs["open"], figs["close"])
    with pytest.raises(ValueError, match="radius in mm needs a spacing"):
        DE.evaluate_dataset(None, src, cfg, closing=(3.0, "mm"))


def test_driver_morphology(tmp_path, capsys):
    """tools.eval_driver.evaluate_on_device over the host reader on one item of the same set: with the options named at their defaults the
    output is byte-identical to a call that does not know them; with a per-slice opening and closing the line is the plain line plus the
    documented suffix, the figures those of the chain by hand on the plain run's saved mask, and save_pred holds the end of the chain.
    The command-line forms parse."""
    import os
    import random

    from rpnet_amd.utils import nrrd
    from rpnet_amd.utils import volume_reader as VR
    from rpnet_amd.volume import VolumeSegmenter
    from tests.test_gpu_dataset_eval import _build_net, _driver_lines, _plain
    from tests.test_gpu_surface_spacing import MM, _mm_dataset
    from tools.eval_driver import build_parser, evaluate_on_device, parse_radius
    data_dir, set_name, cfg = _mm_dataset(tmp_path / "data", MM)
    host = VR.FewshotRegReader(data_dir, set_name, cfg, mode="eval")
    outs = {}
    for name, kw in (("plain", {}), ("off", dict(opening=None, closing=None, morph_per_slice=False)),
                     ("morph", dict(opening=(1.0, "mm"), closing=2, morph_per_slice=True, spacing="header", surface=True))):
        random.seed(5)
        capsys.readouterr()
        d = _plain(evaluate_on_device(_build_net(cfg, "f32"), host, cfg, 1, batch_size=8, graphed=False, save_pred=str(tmp_path / name), **kw))
        outs[name] = (d, capsys.readouterr().out)
    assert outs["off"] == outs["plain"] and outs["morph"][0] == outs["plain"][0]
    random.seed(5)
    item = host[0]
    mask, _ = nrrd.read(os.path.join(str(tmp_path / "plain"), f"{item['pid']}_Liver.nrrd"))
    end, rows = _chain_by_hand(mask, opening=(1.0, "mm"), closing=2, per_slice=True, spacing=MM)
    got, _ = nrrd.read(os.path.join(str(tmp_path / "morph"), f"{item['pid']}_Liver.nrrd"))
    assert np.array_equal(got, end)
    lines = _driver_lines(outs["morph"][1])
    op, cl = MO.morph_figures(rows["opening"])[0], MO.morph_figures(rows["closing"])[0]
    assert len(lines) == 2 and lines[0].endswith(MO.line_suffix(op, cl)) and lines[1].endswith(MO.mean_suffix([op], [cl]))
    with pytest.raises(ValueError, match="made with the same options"):
        evaluate_on_device(None, host, cfg, 1, segmenter=VolumeSegmenter(_build_net(cfg, "f32"), batch=8, graphed=False), closing=2)
    with pytest.raises(ValueError, match="radius in mm needs a spacing"):
        evaluate_on_device(None, host, cfg, 1, opening=(1.0, "mm"))
    ap = build_parser()
    a = ap.parse_args([])
    assert a.opening is None and a.closing is None and a.morph_slice is False
    a = ap.parse_args(["--opening", "2", "--closing", "2.5mm", "--morph-slice"])
    assert parse_radius(a.opening) == 2.0 and parse_radius(a.closing, "--closing") == (2.5, "mm") and a.morph_slice is True
    assert parse_radius(None) is None
    with pytest.raises(ValueError, match="a radius in voxels or <x>mm"):
        parse_radius("wide")
