"""rpnet_surface_spacing_tally (csrc/surface_spacing.hip), rpnet_amd.surface_spacing, VolumeSegmenter(surface=True, spacing=...) and
evaluate_dataset(surface=True, spacing=...) on the MI355X.

Every comparison is against rpnet_amd.surface_spacing.rows_reference_spacing (numpy; pinned to scipy.ndimage and to an all-pairs
computation by tests/test_host_surface_spacing.py).  The int64 row {n_A, n_B, k, within_A, within_B} and d2_k, d2_k1, d2_max must match
bit for bit: the kernel and the restatement perform the same separately rounded operations.  The two sums must match within
n * 2^-52 * sum (tests/surface_spacing_cases.py:check_rows states the derivation)."""
import ctypes

import numpy as np
import pytest
import torch

from rpnet_amd import hip
from rpnet_amd import surface as SF
from rpnet_amd import surface_spacing as SS
from tests import surface_spacing_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL_I, FILL_F = 7, 7.5
HEAD_BYTES = 66048          # counters, radix histograms and partial sums in front of the two fp64 volumes


def tables(rows=3):
    return (torch.full((rows, SS.IROW), FILL_I, device=DEV, dtype=torch.int64),
            torch.full((rows, SS.FROW), FILL_F, device=DEV, dtype=torch.float64))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def tally(pred, truth, spacing, cls=1, tau=None, row=1, rows=3):
    """one surface_tally_spacing into row `row` of fresh, pre-filled tables -> the host tables; the other rows must keep their fill"""
    it, ft = tables(rows)
    SS.surface_tally_spacing(dev(pred), dev(truth), spacing, it, row, ft, row, cls=cls, tau=tau)
    torch.cuda.synchronize()
    it, ft = it.cpu().numpy(), ft.cpu().numpy()
    keep = [r for r in range(rows) if r != row]
    assert (it[keep] == FILL_I).all() and (ft[keep] == FILL_F).all()
    return it[row], ft[row]


def check(pred, truth, spacing, what, cls=1, tau=None, want=None):
    """rpnet_surface_spacing_tally (through SS.surface_tally_spacing in `tally`) == rows_reference_spacing under check_rows"""
    want_i, want_f = want if want is not None else SS.rows_reference_spacing(pred, truth, spacing, cls=cls, tau=tau)
    got_i, got_f = tally(pred, truth, spacing, cls=cls, tau=tau)
    print(f"{pred.shape} {spacing} {what}: {got_i.tolist()} {got_f.tolist()}")
    SC.check_rows(got_i, got_f, want_i, want_f, what=(pred.shape, spacing, what))
    return got_i, got_f


@pytest.mark.parametrize("shape", SC.SHAPES)
def test_rows_equal_the_restatement(shape):
    """every shape of the table, every content family, every spacing; the workspace query is the head plus two fp64 volumes"""
    assert hip.query("rpnet_surface_spacing_workspace_bytes", *shape) == HEAD_BYTES + 16 * int(np.prod(shape))
    for name in SC.CONTENTS:
        a, b = SC.content(shape, name)
        for spacing in SC.SPACINGS:
            got_i, got_f = check(a, b, spacing, name, want=SC.reference(shape, name, spacing))
            if name.startswith("empty"):
                assert got_i.tolist() == [0, 0, -1, 0, 0] and got_f.tolist() == [0.0] * 5
            else:
                assert got_i[0] > 0 and got_i[1] > 0 and got_i[2] >= 0


@pytest.mark.parametrize("shape", SC.SHAPES)
def test_unit_spacing_equals_the_integer_path(shape):
    """at spacing (1, 1, 1) the rows are what rpnet_surface_tally writes for the same volumes: its d2 columns converted to double, the same
    n_A, n_B and k, and the same sums within the bound of either test"""
    for name in SC.CONTENTS:
        a, b = SC.content(shape, name)
        got_i, got_f = tally(a, b, (1.0, 1.0, 1.0))
        it = torch.full((1, SF.IROW), FILL_I, device=DEV, dtype=torch.int64)
        ft = torch.full((1, SF.FROW), FILL_F, device=DEV, dtype=torch.float64)
        SF.surface_tally(dev(a), dev(b), it, 0, ft, 0)
        torch.cuda.synchronize()
        n_a, n_b, d2_k, d2_k1, d2_max, k = it[0].cpu().numpy().tolist()
        sums = ft[0].cpu().numpy()
        assert got_i[:3].tolist() == [n_a, n_b, k], (shape, name)
        assert got_f[:3].tolist() == [float(d2_k), float(d2_k1), float(d2_max)], (shape, name)
        # either sum against the exact one: n * 2^-53 here (check_rows), 2 * nbins * 2^-53 there (tests/test_gpu_surface.py)
        nbins = sum((s - 1) ** 2 for s in shape) + 1
        for col, n in ((3, n_a), (4, n_b)):
            assert abs(got_f[col] - sums[col - 3]) <= (n + 2 * nbins) * 2.0 ** -53 * sums[col - 3], (shape, name, col)


@pytest.mark.parametrize("counts", SC.COUNTS)
def test_small_pooled_counts(counts):
    """pooled counts of 2, 3, 21 and 22: k = 0, k + 1 clamped to n - 1, (n - 1) * 0.95 next to a whole number, interpolation at 0.95"""
    a, b = SC.scattered(*counts)
    for spacing in SC.SPACINGS:
        got_i, got_f = check(a, b, spacing, f"scattered {counts}")
        n = sum(counts)
        assert got_i[:3].tolist() == [counts[0], counts[1], SC.rank(n)]
        fig = SS.figures_from_rows(got_i, got_f)
        want = SC.percentile95(SC.brute_force(a, b, spacing))
        assert abs(fig["hd95"] - want) <= 16 * 2.0 ** -52 * want, (counts, spacing, fig["hd95"], want)


def test_ties_across_the_rank_and_low_bits():
    """two parallel planes (one distance nearly everywhere); distances whose doubles differ only in low bits, so that the last digits
    of the radix selection decide between rank k and rank k + 1"""
    a, b = SC.planes()
    for spacing in SC.SPACINGS:
        got_i, got_f = check(a, b, spacing, "planes")
        assert got_f[0] == got_f[1] < got_f[2]
    a, b, shape = SC.low_bits()
    for spacing in SC.LOW_BIT_SPACINGS:
        got_i, got_f = check(a, b, spacing, "low bits")
        assert got_i[:3].tolist() == [1, 20, 19]
        w = SS.spacing_weights(spacing)
        assert got_f[0] == 100.0 and got_f[1] == got_f[2] == w[1] * 100.0 and got_f[1] != got_f[0]
    lo, hi = (np.float64(v).view(np.uint64) for v in (100.0, SS.spacing_weights(SC.LOW_BIT_SPACINGS[0])[1] * 100.0))
    assert lo >> np.uint64(8) == hi >> np.uint64(8) and lo != hi, "the first pair differs in the last radix digit only"


def test_every_element_kind_and_class():
    """cls = 1 and cls = 2 on three-valued masks; every accepted element kind, for either argument, gives the same bits"""
    from tests.surface_cases import three_valued
    a, b = three_valued((9, 33, 20))
    for spacing in SC.SPACINGS:
        for cls in (1, 2):
            want_i, want_f = check(a, b, spacing, f"cls {cls}", cls=cls, tau=1.5)
            for pk, tk in ((np.uint8, np.int32), (np.int32, np.int64), (np.int64, np.float32), (np.float32, np.uint8), (np.float32, np.float32)):
                got_i, got_f = tally(a.astype(pk), b.astype(tk), spacing, cls=cls, tau=1.5)
                assert got_i.tobytes() == want_i.tobytes() and got_f.tobytes() == want_f.tobytes(), (spacing, cls, pk, tk)


def test_nsd_counts():
    """tau = 0 counts the coinciding border voxels; a tau whose square equals an occurring squared distance counts it (`<=`, where `<`
    would not); tau unset leaves both columns 0 and nsd None"""
    a, b = SC.boxes((6, 12, 13))
    for spacing, tau in (((1.0, 1.0, 1.0), 1.0), ((2.5, 0.5, 0.5), 2.5), ((2.5, 0.5, 0.5), 0.5)):
        w = SS.spacing_weights(spacing)
        from rpnet_amd.surface import border_reference
        d_ab = SS.transform_reference_spacing(border_reference(b == 1), w)[border_reference(a == 1)]
        assert (d_ab == tau * tau).any(), "the tolerance must coincide with an occurring distance"
        got_i, got_f = check(a, b, spacing, f"tau {tau}", tau=tau)
        assert got_i[3] == int((d_ab <= tau * tau).sum()) > int((d_ab < tau * tau).sum())
        fig = SS.figures_from_rows(got_i, got_f, tau)
        assert fig["nsd"] == (got_i[3] + got_i[4]) / (got_i[0] + got_i[1]) and 0 < fig["nsd"] < 1
        zero_i, zero_f = check(a, b, spacing, "tau 0", tau=0.0)
        assert zero_i[3] == int((d_ab == 0).sum()) and 0 < zero_i[3] < got_i[3]
        none_i, none_f = check(a, b, spacing, "no tau")
        assert none_i[3:].tolist() == [0, 0] and SS.figures_from_rows(none_i, none_f)["nsd"] is None
        assert none_f.tobytes() == got_f.tobytes() and none_i[:3].tolist() == got_i[:3].tolist()


def test_workspace_guard_determinism_and_graph_replay():
    """the workspace is exactly as long as its query says (guard words behind it keep their bits); a second identical call gives the
    same bits; captured in a graph, two replays into refilled tables give those bits again"""
    shape, spacing = (9, 40, 36), SC.SPACINGS[3]
    a, b = SC.noise(shape)
    want = SS.rows_reference_spacing(a, b, spacing, tau=1.0)
    da, db = dev(a), dev(b)
    need = hip.query("rpnet_surface_spacing_workspace_bytes", *shape)
    ws = torch.full((need + 64,), 0xA5, device=DEV, dtype=torch.uint8)
    w = (ctypes.c_double * 3)(*SS.spacing_weights(spacing))

    def raw(it, ft):
        hip.call("rpnet_surface_spacing_tally", hip.ptr(da), 0, hip.ptr(db), 0, 1, *shape, w, 1.0, hip.ptr(it), 1, hip.ptr(ft), 1, 3, hip.ptr(ws), need)
    runs = []
    for _ in range(2):
        it, ft = tables()
        raw(it, ft)
        torch.cuda.synchronize()
        runs.append((it.cpu().numpy(), ft.cpu().numpy()))
        assert (ws[need:] == 0xA5).all()
    SC.check_rows(runs[0][0][1], runs[0][1][1], *want, what="raw")
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    assert (runs[0][0][[0, 2]] == FILL_I).all() and (runs[0][1][[0, 2]] == FILL_F).all()

    it, ft = tables()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        raw(it, ft)
    for _ in range(2):
        it.fill_(FILL_I)
        ft.fill_(FILL_F)
        graph.replay()
        torch.cuda.synchronize()
        assert it.cpu().numpy().tobytes() == runs[0][0].tobytes() and ft.cpu().numpy().tobytes() == runs[0][1].tobytes()
    assert (ws[need:] == 0xA5).all()


def test_refusals_launch_nothing():
    """every refusal of the ABI returns a status and a message and leaves the tables as they were; every refusal of the Python layer
    raises before a call"""
    a, b = (dev(x) for x in SC.noise((5, 7, 9)))
    it, ft = tables()
    p = hip.ptr
    need = hip.query("rpnet_surface_spacing_workspace_bytes", 5, 7, 9)
    ws = torch.empty(need, device=DEV, dtype=torch.uint8)
    good = (ctypes.c_double * 3)(1.0, 1.0, 1.0)

    def raw(pred=p(a), pk=0, truth=p(b), tk=0, dims=(5, 7, 9), w=good, tau2=-1.0, itab=p(it), irow=0, ftab=p(ft), frow=0, work=p(ws), nbytes=need):
        hip.call("rpnet_surface_spacing_tally", pred, pk, truth, tk, 1, *dims, w, tau2, itab, irow, ftab, frow, 3, work, nbytes)
    for row in (3, -1):
        with pytest.raises(RuntimeError, match=f"rows {row} and 0 of tables of 3 rows"):
            raw(irow=row)
        with pytest.raises(RuntimeError, match=f"rows 0 and {row} of tables of 3 rows"):
            raw(frow=row)
    with pytest.raises(RuntimeError, match=f"workspace of {need - 1} bytes, {need} needed"):
        raw(nbytes=need - 1)
    for dims in ((1025, 1, 1), (5, 1025, 9), (5, 7, 0)):
        with pytest.raises(RuntimeError, match="every extent 1..1024"):
            raw(dims=dims)
        assert hip.query("rpnet_surface_spacing_workspace_bytes", *dims) == 0
        assert hip.load().rpnet_last_error_string().decode().startswith("surface_spacing: D=")
    for kw in (dict(pred=None), dict(truth=None), dict(itab=None), dict(ftab=None), dict(work=None), dict(w=None)):
        with pytest.raises(RuntimeError, match="null pointer"):
            raw(**kw)
    with pytest.raises(RuntimeError, match="element kinds 4, 0"):
        raw(pk=4)
    with pytest.raises(RuntimeError, match="element kinds 0, -1"):
        raw(tk=-1)
    with pytest.raises(RuntimeError, match="aligned"):
        raw(work=p(ws) + 8, nbytes=need)
    for axis, bad in ((0, 0.0), (1, -1.0), (2, float("inf")), (1, float("nan"))):
        w = (ctypes.c_double * 3)(1.0, 1.0, 1.0)
        w[axis] = bad
        with pytest.raises(RuntimeError, match=f"weight {axis} is .* finite and > 0"):
            raw(w=w)
    with pytest.raises(RuntimeError, match="tau2 is NaN"):
        raw(tau2=float("nan"))
    # the Python layer
    args = (it, 0, ft, 0)
    with pytest.raises(ValueError, match="uint8, int32, int64 and float32"):
        SS.surface_tally_spacing(a.double(), b, (1, 1, 1), *args)
    with pytest.raises(ValueError, match="differ in shape"):
        SS.surface_tally_spacing(a[:, :, :4].contiguous(), b, (1, 1, 1), *args)
    with pytest.raises(ValueError, match="contiguous"):
        SS.surface_tally_spacing(a[:, :, ::2], b[:, :, ::2], (1, 1, 1), *args)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        SS.surface_tally_spacing(a.cpu(), b, (1, 1, 1), *args)
    old_i = torch.zeros((3, SF.IROW), device=DEV, dtype=torch.int64)
    old_f = torch.zeros((3, SF.FROW), device=DEV, dtype=torch.float64)
    with pytest.raises(ValueError, match=r"int64 \[n, 5\] tensor \(the widths under a spacing\)"):
        SS.surface_tally_spacing(a, b, (1, 1, 1), old_i, 0, ft, 0)
    with pytest.raises(ValueError, match=r"float64 \[n, 5\] tensor \(the widths under a spacing\)"):
        SS.surface_tally_spacing(a, b, (1, 1, 1), it, 0, old_f, 0)
    with pytest.raises(ValueError, match="4 and 3 rows"):
        SS.surface_tally_spacing(a, b, (1, 1, 1), torch.zeros((4, 5), device=DEV, dtype=torch.int64), 0, ft, 0)
    for bad in ((1, 1), (1, 0, 1), (1, -2, 1), (1, float("inf"), 1), (float("nan"), 1, 1), 2.0, "1,1,1", None):
        with pytest.raises(ValueError, match="three finite positive numbers"):
            SS.surface_tally_spacing(a, b, bad, *args)
    with pytest.raises(ValueError, match="tau is NaN"):
        SS.surface_tally_spacing(a, b, (1, 1, 1), *args, tau=float("nan"))
    with pytest.raises(RuntimeError, match="rows 3 and 0"):
        SS.surface_tally_spacing(a, b, (1, 1, 1), it, 3, ft, 0)
    torch.cuda.synchronize()
    assert (it == FILL_I).all() and (ft == FILL_F).all()
    raw()
    torch.cuda.synchronize()
    want = SS.rows_reference_spacing(a.cpu().numpy(), b.cpu().numpy(), (1, 1, 1))
    SC.check_rows(it[0].cpu().numpy(), ft[0].cpu().numpy(), *want, what="after the refusals")


# ------------------------------------------------------------------------------------------------ end to end
MM, TAU = (2.5, 0.8, 0.8), 2.0


def _figures_match(got, want, n_border):
    """figures of device rows against figures of the restatement's rows: hd95, hd and nsd come from equal bits; assd within the bound of
    its two sums"""
    for key in ("hd95", "hd", "nsd"):
        assert got[key] == want[key], (key, got[key], want[key])
    assert (got["assd"] is None) == (want["assd"] is None)
    assert want["assd"] is None or abs(got["assd"] - want["assd"]) <= n_border * 2.0 ** -52 * want["assd"]


def test_volume_segmenter_spacing():
    """a small synthetic episode, f32 convolutions, eager: under a spacing res.surface and res.post['surface'] equal the restatement
    applied to the masks; mask, counts and dice are those of a run without the argument; surface_out takes the new widths and its check
    says so when handed the old ones; spacing=None gives what the integer path gives"""
    import rpnet_amd.functional as RF
    from rpnet_amd.volume import VolumeSegmenter
    from tests.test_gpu_volume import build_net, eval_cfg, reader, segment
    RF.set_conv_math("f32")              # restored by tests/conftest.py
    cfg = eval_cfg()
    item = reader(cfg, 6, 64)[0]
    net = build_net(cfg)
    plain = segment(VolumeSegmenter(net, batch=4, graphed=False, surface=True, keep_largest=6), item)
    res = segment(VolumeSegmenter(net, batch=4, graphed=False, surface=True, keep_largest=6, spacing=MM, surface_tolerance=TAU), item)
    assert torch.equal(res.mask, plain.mask) and res.counts.tobytes() == plain.counts.tobytes() and res.dice == plain.dice
    assert torch.equal(res.post["mask"], plain.post["mask"]) and sorted(plain.surface["fewshot"][0]) == ["assd", "hd", "hd95"]
    labels, appr = item["query_labels"].numpy(), item["appr_query_labels"].numpy()
    for got, pred in ((res.surface["fewshot"][0], res.mask), (res.surface["affine"][0], torch.from_numpy(appr)),
                      (res.post["surface"][0], res.post["mask"])):
        irow, _, want = SS.surface_reference_spacing(pred.cpu().numpy(), labels, MM, tau=TAU)
        print("got", got, "want", want)
        assert want["hd95"] is not None and 0 < want["nsd"] <= 1
        _figures_match(got, want, int(irow[0] + irow[1]))
    # the same segmenter with the spacing given per call, and the caller's tables
    seg = VolumeSegmenter(net, batch=4, graphed=False, surface=True, surface_tolerance=TAU)
    it = torch.full((2, 1, SS.IROW), FILL_I, device=DEV, dtype=torch.int64)
    ft = torch.full((2, 1, SS.FROW), FILL_F, device=DEV, dtype=torch.float64)
    args = (item["support_images"], item["support_labels"], item["query_images"], item["appr_query_labels"], item["query_labels"])
    out = seg(*args, surface_out=(it, ft), spacing=MM)
    assert out.surface is None and torch.equal(out.mask, plain.mask)
    for s, pred in enumerate((res.mask.cpu().numpy(), appr)):
        SC.check_rows(it[s, 0].cpu().numpy(), ft[s, 0].cpu().numpy(), *SS.rows_reference_spacing(pred, labels, MM, tau=TAU), what=s)
    old = (torch.zeros((2, 1, SF.IROW), device=DEV, dtype=torch.int64), torch.zeros((2, 1, SF.FROW), device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"int64 \[2, 1, 5\], float64 \[2, 1, 5\]\) \(the widths under a spacing"):
        seg(*args, surface_out=old, spacing=MM)
    with pytest.raises(ValueError, match="give spacing= as well"):
        seg(*args)
    with pytest.raises(ValueError, match="three finite positive numbers"):
        VolumeSegmenter(net, surface=True, spacing=(1, 0, 1))
    none = segment(VolumeSegmenter(net, batch=4, graphed=False, surface=True, keep_largest=6, spacing=None), item)
    assert none.surface == plain.surface and none.post["surface"] == plain.post["surface"]


def _mm_dataset(tmp_path, spacing):
    from rpnet_amd.utils import volume_reader as VR
    from tests.test_gpu_dataset_eval import CASE, _eval_cfg, config_for
    data_dir, set_name, csv_dir = VR.write_synthetic_dataset(str(tmp_path), spacing=spacing, **CASE["data"])
    return data_dir, set_name, _eval_cfg(dict(config_for(CASE, csv_dir), use_registration_mask=False, do_deformable=False))


def test_evaluate_dataset_spacing_from_the_header(tmp_path, capsys):
    """a synthetic NRRD set written with spacing (2.5, 0.8, 0.8), f32 convolutions, eager.  spacing="header": the dictionaries and tally
    tables of a run without the new arguments; every line is that run's line with the surface fields in mm and the nsd field; the rows
    equal the restatement on the saved masks.  spacing=None: tables and lines of a run made without the argument.  A set without a
    spacing raises before any launch."""
    import os
    import random

    from rpnet_amd import dataset_eval as DE
    from rpnet_amd.utils import nrrd
    from tests.test_gpu_dataset_eval import _build_net, _driver_lines, _plain
    data_dir, set_name, cfg = _mm_dataset(tmp_path / "data", MM)
    src = DE.DeviceEvalSource(data_dir, set_name, cfg, DEV)
    src.warm()
    assert src.reader.volume_spacing(src.reader.data_info[0][0]["pid"]) == MM
    pred_dir = str(tmp_path / "pred")
    runs = {}
    for name, kw in (("before", {}), ("none", dict(spacing=None, surface_tolerance=None)),
                     ("header", dict(spacing="header", surface_tolerance=TAU, save_pred=pred_dir))):
        random.seed(77)
        capsys.readouterr()
        tabs = {}
        dicts = _plain(DE.evaluate_dataset(_build_net(cfg, "f32"), src, cfg, batch=8, graphed=False, out=tabs, surface=True, **kw))
        runs[name] = (dicts, tabs, _driver_lines(capsys.readouterr().out))
    (d0, t0, l0), (d1, t1, l1), (d2, t2, l2) = runs["before"], runs["none"], runs["header"]
    assert d1 == d0 and l1 == l0 and sorted(t1) == sorted(t0) == ["counts", "ncc", "surface_f", "surface_i"]
    assert all(t1[k].tobytes() == t0[k].tobytes() for k in t0)
    assert d2 == d0 and sorted(t2) == ["counts", "ncc", "spacing", "surface_mm_f", "surface_mm_i"] and t2["spacing"] == [MM] * 3
    assert t2["counts"].tobytes() == t0["counts"].tobytes() and t2["ncc"].tobytes() == t0["ncc"].tobytes()
    si, sf = t2["surface_mm_i"], t2["surface_mm_f"]
    assert si.shape == (3, 2, 1, SS.IROW) and si.dtype == np.int64 and sf.shape == (3, 2, 1, SS.FROW) and sf.dtype == np.float64
    assert len(l0) == len(l2) == 4
    few, aff = [], []
    random.seed(77)
    for j in range(3):
        s = src.item(j)
        labels, appr = s["query_labels"].cpu().numpy(), s["appr_query_labels"].cpu().numpy()
        mask, _ = nrrd.read(os.path.join(pred_dir, f"{s['pid']}_Liver.nrrd"))
        figs = []
        for r, pred in enumerate((mask, appr)):
            irow, frow, want = SS.surface_reference_spacing(pred, labels, MM, tau=TAU)
            SC.check_rows(si[j, r, 0], sf[j, r, 0], irow, frow, what=(j, r))
            got = SS.figures_from_rows(si[j, r, 0], sf[j, r, 0], TAU)
            _figures_match(got, want, int(irow[0] + irow[1]))
            figs.append(got)
        few.append(figs[0])
        aff.append(figs[1])
        head = l0[j][:l0[j].index(" hd95 ")]
        mm = lambda v: SF.fmt(v) + ("mm" if v is not None else "")      # noqa: E731
        assert l2[j] == (head + f" hd95 {mm(figs[0]['hd95'])} ({mm(figs[1]['hd95'])}) assd {mm(figs[0]['assd'])} ({mm(figs[1]['assd'])})"
                         + f" nsd {SF.fmt(figs[0]['nsd'])} ({SF.fmt(figs[1]['nsd'])})"), (l0[j], l2[j])
    assert any(a["hd95"] is not None for a in aff) and "mm" in l2[0]
    assert l2[3] == l0[3][:l0[3].index(" hd95 ")] + SS.mean_suffix_mm(few, aff, True)
    # no spacing on disk: "header" raises while the headers are read, before the first item is built
    bare_dir, bare_set, bare_cfg = _mm_dataset(tmp_path / "bare", None)
    bare = DE.DeviceEvalSource(bare_dir, bare_set, bare_cfg, DEV)
    built = []
    bare.item = lambda j: built.append(j)
    with pytest.raises(ValueError, match="_clean.nrrd: spacing_from_header: .* neither field is present"):
        DE.evaluate_dataset(_build_net(cfg, "f32"), bare, bare_cfg, batch=8, graphed=False, surface=True, spacing="header")
    assert built == []
    with pytest.raises(ValueError, match="give surface=True"):
        DE.evaluate_dataset(None, src, cfg, spacing=MM)
    with pytest.raises(ValueError, match="give spacing= as well"):
        DE.evaluate_dataset(None, src, cfg, surface=True, surface_tolerance=1.0)


def test_driver_spacing(tmp_path, capsys):
    """tools.eval_driver.evaluate_on_device over the host reader with spacing="header" on one item of the same set: the dictionaries of
    a run without it; the item line carries the figures of the restatement on the saved mask, in mm; the command-line forms parse"""
    import os
    import random

    from rpnet_amd.utils import nrrd
    from rpnet_amd.utils import volume_reader as VR
    from tests.test_gpu_dataset_eval import _build_net, _driver_lines, _plain
    from tools.eval_driver import build_parser, evaluate_on_device, parse_spacing
    data_dir, set_name, cfg = _mm_dataset(tmp_path / "data", MM)
    host = VR.FewshotRegReader(data_dir, set_name, cfg, mode="eval")
    random.seed(5)
    capsys.readouterr()
    want = _plain(evaluate_on_device(_build_net(cfg, "f32"), host, cfg, 1, batch_size=8, graphed=False, surface=True))
    lines0 = _driver_lines(capsys.readouterr().out)
    random.seed(5)
    got = _plain(evaluate_on_device(_build_net(cfg, "f32"), host, cfg, 1, batch_size=8, graphed=False, surface=True, save_pred=str(tmp_path / "p"),
                                    spacing="header", surface_tolerance=TAU))
    lines1 = _driver_lines(capsys.readouterr().out)
    assert got == want and len(lines0) == len(lines1) == 2
    random.seed(5)
    item = host[0]
    mask, _ = nrrd.read(os.path.join(str(tmp_path / "p"), f"{item['pid']}_Liver.nrrd"))
    labels = item["query_labels"].numpy()
    few = SS.surface_reference_spacing(mask, labels, MM, tau=TAU)[2]
    aff = SS.surface_reference_spacing(item["appr_query_labels"].numpy(), labels, MM, tau=TAU)[2]
    head = lines0[0][:lines0[0].index(" hd95 ")]
    assert lines1[0].startswith(head + f" hd95 {SF.fmt(few['hd95'])}mm ({SF.fmt(aff['hd95'])}mm) assd ")
    assert lines1[0].endswith(f" nsd {SF.fmt(few['nsd'])} ({SF.fmt(aff['nsd'])})")
    assert parse_spacing("header") == "header" and parse_spacing("2.5,0.8,0.8") == MM and parse_spacing([2.5, 0.8, 0.8]) == MM
    with pytest.raises(ValueError, match="three numbers Z,Y,X"):
        parse_spacing("1,2")
    a = build_parser().parse_args(["--spacing", "header", "--surface-tolerance", "2"])
    assert a.spacing == "header" and a.surface_tolerance == 2.0
