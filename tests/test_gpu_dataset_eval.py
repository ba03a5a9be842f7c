"""Evaluation items assembled on the device and the data-set loop over them (csrc/evalitem.hip, rpnet_amd/dataset_eval.py, the
counts_out argument of rpnet_amd.volume.VolumeSegmenter) on the MI355X, against numpy and against this repository's host reader
(rpnet_amd/utils/volume_reader.py, pinned to the reference by tests/golden/volume_reader.npz) and host-item driver
(tools/eval_driver.py:evaluate_on_device)."""
import os
import random

import numpy as np
import pytest
import torch

from rpnet_amd import dataset_eval as DE
from rpnet_amd import hip
from rpnet_amd.utils import volume_reader as VR
from tests import augment_cases as AC
from tests.helpers import load_cfg
from tests.reader_cases import config_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------------------- gather
def _volumes(seed, Ds, S, H, W):
    rs = np.random.RandomState(seed)
    s_img, q_img = [rs.uniform(-1, 1, (d, H, W)).astype(np.float32) for d in (Ds, S)]
    s_msk, q_msk = [(rs.rand(d, H, W) < 0.3).astype(np.float32) for d in (Ds, S)]
    s_img.flat[:3], q_img.flat[:3] = [-1.0, 1.0, 1e-30], [-1.0, 1.0, -1e-30]
    return s_img, s_msk, q_img, q_msk, rs.randint(0, Ds, size=S).astype(np.int32)


@pytest.mark.parametrize("Ds,S,H,W", [(7, 9, 12, 40), (5, 6, 10, 44), (6, 4, 5, 63), (9, 1, 7, 63), (4, 3, 256, 256), (3, 1, 16, 256), (1, 5, 3, 2)])
def test_gather_matches_numpy_indexing(Ds, S, H, W):
    """rpnet_eval_item_gather against numpy indexing: the four copies and the two (x + 1) / 2 planes, bit for bit, for W a multiple of
    4 or not (a scalar tail per row, rows on 4-byte boundaries), S = 1, and volumes that start on a 4-byte boundary only"""
    s_img, s_msk, q_img, q_msk, table = _volumes(100 + W + S, Ds, S, H, W)
    want = [s_img[table], s_msk[table], q_img, q_msk, (s_img[table] + 1) / 2, (q_img + 1) / 2]
    assert all(w.dtype == np.float32 for w in want)
    got = DE.eval_item_gather(_dev(s_img), _dev(s_msk), _dev(q_img), _dev(q_msk), table)
    torch.cuda.synchronize()
    for g, w, what in zip(got, want, ("support image", "support label", "query image", "query label", "support [0,1]", "query [0,1]")):
        assert tuple(g.shape) == (S, H, W) and g.dtype == torch.float32
        assert torch.equal(g.cpu(), torch.from_numpy(w)), what
        assert np.array_equal(g.cpu().numpy().view(np.uint32), w.view(np.uint32)), what
    # the same volumes one float into a larger allocation: base pointers on a 4-byte boundary only
    pad = lambda a: _dev(np.concatenate([[0.0], a.ravel()]).astype(np.float32))[1:].view(a.shape)  # noqa: E731
    again = DE.eval_item_gather(pad(s_img), pad(s_msk), pad(q_img), pad(q_msk), torch.from_numpy(table))
    for g, w in zip(again, want):
        assert torch.equal(g.cpu(), torch.from_numpy(w))


def test_gather_error_returns():
    """a null pointer and S = 0 are refused by the entry point, a slice number outside the support volume by the host-side check of
    the table before it is uploaded; nothing is launched in any of these"""
    s_img, s_msk, q_img, q_msk, table = _volumes(5, 4, 3, 8, 12)
    d = [_dev(a) for a in (s_img, s_msk, q_img, q_msk)]
    outs = [torch.empty(3, 8, 12, device=DEV) for _ in range(6)]
    tab = _dev(table)
    p = hip.ptr
    with pytest.raises(RuntimeError, match="null pointer"):
        hip.call("rpnet_eval_item_gather", p(d[0]), None, p(d[2]), p(d[3]), p(tab), *[p(t) for t in outs], 4, 3, 8, 12)
    with pytest.raises(RuntimeError, match="null pointer"):
        hip.call("rpnet_eval_item_gather", *[p(t) for t in d], None, *[p(t) for t in outs], 4, 3, 8, 12)
    with pytest.raises(RuntimeError, match="empty volume or item is refused"):
        hip.call("rpnet_eval_item_gather", *[p(t) for t in d], p(tab), *[p(t) for t in outs], 4, 0, 8, 12)
    with pytest.raises(RuntimeError, match="empty volume or item is refused"):
        DE.eval_item_gather(d[0], d[1], d[2][:0], d[3][:0], np.zeros(0, np.int32))
    with pytest.raises(RuntimeError, match="in place"):
        hip.call("rpnet_eval_item_gather", *[p(t) for t in d], p(tab), p(d[2]), *[p(t) for t in outs[1:]], 4, 3, 8, 12)
    assert hip.load().rpnet_last_error_string().decode().startswith("eval_item_gather: a gather cannot run in place")
    for bad in ([0, 4, 1], [0, -1, 1]):
        with pytest.raises(ValueError, match=r"outside the support volume's \[0, 4\)"):
            DE.eval_item_gather(*d, np.asarray(bad, np.int32))
    with pytest.raises(ValueError, match="2 table entries for 3 query slices"):
        DE.eval_item_gather(*d, np.zeros(2, np.int32))
    with pytest.raises(TypeError, match="host memory"):
        DE.eval_item_gather(*d, tab)
    with pytest.raises(NotImplementedError, match="differ in size"):
        DE.eval_item_gather(d[0], d[1], d[2][:, :, :8].contiguous(), d[3][:, :, :8].contiguous(), table)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- NCC
U = 2.0 ** -53


def ncc_with_bound(moving, fixed):
    """net.registration.NCC (net/registration.py:16-20) in float64 numpy, and the bound on what ANY fp64 evaluation of that formula
    may differ from the exact value by: every sum of N terms in any order is within N * 2^-53 * sum|term| of the exact sum of its
    terms (recursive summation, Higham, Accuracy and Stability of Numerical Algorithms, 4.2; the rounding of a single term, 2^-53
    of it, is inside that since N >> 1), a mean is therefore within 2^-53 * sum|x| of the exact mean, which moves sum f m by at most
    |dmean_f| sum|m| + |dmean_m| sum|f| and sum f^2 by 2 |dmean_f| sum|f|; the three bounds go through v = -A / sqrt(B C + 1e-10) to
    first order: |dv| <= dA / D + |A| (dB C + B dC) / (2 D^3)."""
    m, f = moving.astype(np.float64).ravel(), fixed.astype(np.float64).ravel()
    N = m.size
    fc, mc = f - f.mean(), m - m.mean()
    A, B, C = np.sum(fc * mc), np.sum(fc ** 2), np.sum(mc ** 2)
    D = np.sqrt(B * C + 1e-10)
    dmf, dmm = U * np.abs(f).sum(), U * np.abs(m).sum()
    dA = N * U * np.abs(fc * mc).sum() + dmf * np.abs(mc).sum() + dmm * np.abs(fc).sum()
    dB = N * U * B + 2 * dmf * np.abs(fc).sum()
    dC = N * U * C + 2 * dmm * np.abs(mc).sum()
    return -1.0 * A / D, dA / D + abs(A) * (dB * C + B * dC) / (2 * D ** 3)


def _ncc_images(seed, shape):
    rs = np.random.RandomState(seed)
    q = rs.uniform(-1, 1, shape).astype(np.float32)
    w = (0.8 * q + 0.2 * rs.uniform(-1, 1, shape)).astype(np.float32)
    a = (0.3 * q + 0.7 * rs.uniform(-1, 1, shape) + 0.1).astype(np.float32)
    return q, w, a


@pytest.mark.parametrize("shape", [(5, 1, 37, 51), (8, 1, 64, 64), (1, 1, 3, 1), (64, 1, 256, 256)])
def test_ncc_pairs_against_float64_numpy(shape):
    """rpnet_ncc_pairs against the float64 numpy evaluation of the reference formula, within the summation bound the test computes
    from its own data (ncc_with_bound: no chosen constant); 16-byte and scalar loads (an element count that is no multiple of 4,
    tensors that start on a 4-byte boundary); the row of the table that was asked for and no other; two runs give the same bits.
    rpnet_ncc_pairs_workspace_bytes sizes the workspace (through ncc_pairs)."""
    q, w, a = _ncc_images(sum(shape), shape)
    (want_w, tol_w), (want_a, tol_a) = ncc_with_bound(q, w), ncc_with_bound(q, a)
    table = torch.full((3, 2), 7.0, device=DEV, dtype=torch.float64)
    dq, dw, da = _dev(q), _dev(w[:, 0]), _dev(a)               # the warped support comes as [S,H,W], as the item holds it
    DE.ncc_pairs(dq, dw, da, table, 1)
    DE.ncc_pairs(dq, dw, da, table, 2)
    got = table.cpu().numpy()
    print(f"{shape}: NCC(q, warped) {got[1, 0]:.12f} want {want_w:.12f} |diff| {abs(got[1, 0] - want_w):.3e} bound {tol_w:.3e}; "
          f"NCC(q, affine) {got[1, 1]:.12f} want {want_a:.12f} |diff| {abs(got[1, 1] - want_a):.3e} bound {tol_a:.3e}")
    assert got[0].tolist() == [7.0, 7.0]
    assert 0 < tol_w < 1e-6 and 0 < tol_a < 1e-6
    assert abs(got[1, 0] - want_w) <= tol_w and abs(got[1, 1] - want_a) <= tol_a
    if q.size > 1000:
        assert want_w < -0.9 and -0.9 < want_a < -0.1           # the two figures are told apart
    assert np.array_equal(got[1].view(np.int64), got[2].view(np.int64))
    # scalar path: the same elements one float into a larger allocation
    off = lambda x: _dev(np.concatenate([x.ravel()[:1], x.ravel()]))[1:]  # noqa: E731
    DE.ncc_pairs(off(q), off(w), off(a), table, 0)
    got0 = table[0].cpu().numpy()
    assert abs(got0[0] - want_w) <= tol_w and abs(got0[1] - want_a) <= tol_a
    assert hip.query("rpnet_ncc_pairs_workspace_bytes", q.size) >= 2 * 8 * 8


def test_ncc_pairs_constant_image_and_refusals():
    """a constant image: f - mean f is exactly zero (the fp64 sum of n equal fp32 values is exact), the numerator is zero and the
    denominator is the 1e-10 term alone, so the figure is (minus) zero exactly, as in numpy; the other pair of the same call is
    within its bound"""
    shape = (6, 1, 40, 44)
    q, w, a = _ncc_images(3, shape)
    const = np.full(shape, np.float32(0.3), dtype=np.float32)
    table = torch.full((2, 2), 7.0, device=DEV, dtype=torch.float64)
    DE.ncc_pairs(_dev(q), _dev(const), _dev(a), table, 0)
    DE.ncc_pairs(_dev(const), _dev(w), _dev(const), table, 1)
    got = table.cpu().numpy()
    want_c, _ = ncc_with_bound(q, const)
    want_a, tol_a = ncc_with_bound(q, a)
    print("constant image:", got.tolist(), "numpy", want_c, want_a)
    assert want_c == 0.0 and got[0, 0] == 0.0 and abs(got[0, 1] - want_a) <= tol_a
    assert got[1].tolist() == [0.0, 0.0]
    d = _dev(q)
    with pytest.raises(RuntimeError, match="row 2 of a table of 2 rows"):
        DE.ncc_pairs(d, d, d, table, 2)
    with pytest.raises(RuntimeError, match="row -1"):
        DE.ncc_pairs(d, d, d, table, -1)
    with pytest.raises(RuntimeError, match="empty tensors"):
        DE.ncc_pairs(d[:0], d[:0], d[:0], table, 0)
    with pytest.raises(RuntimeError, match="null pointer"):
        hip.call("rpnet_ncc_pairs", hip.ptr(d), None, hip.ptr(d), d.numel(), hip.ptr(table), 0, 2, hip.ptr(d), 1 << 20)
    with pytest.raises(RuntimeError, match="workspace of 8 bytes"):
        hip.call("rpnet_ncc_pairs", hip.ptr(d), hip.ptr(d), hip.ptr(d), d.numel(), hip.ptr(table), 0, 2, hip.ptr(d), 8)
    with pytest.raises(ValueError, match="float64"):
        DE.ncc_pairs(d, d, d, table.float(), 0)
    with pytest.raises(ValueError, match="elements"):
        DE.ncc_pairs(d, d[:1], d, table, 0)
    torch.cuda.synchronize()


# -------------------------------------------------------------------------------------------------------------- items
CASE = {"data": dict(n_volumes=3, classes=("Liver",), shape=(22, 72, 72), seed=11),
        "cfg": dict(num_slice=20, num_x=72, num_y=72, crop_size=[64, 64], k=4)}


def _dataset(tmp_path, **over):
    data_dir, set_name, csv_dir = VR.write_synthetic_dataset(str(tmp_path), **CASE["data"])
    return data_dir, set_name, dict(config_for(CASE, csv_dir), use_registration_mask=False, **over)


@pytest.mark.parametrize("deformable", [False, True])
def test_device_item_matches_host_reader(tmp_path, deformable):
    """DeviceEvalSource.item(idx) against FewshotRegReader(mode="eval")[idx] for every idx, `random` seeded alike before each side
    (one reader and one source over all items, so that k sticks alike).  The gathered fields, the support choice and the generator's
    final state are equal.  Affine registration only: the registered fields are equal too, bit for bit (the same launches on equal
    inputs).  With the demons stage, whose backward scatters with fp32 atomics in an order that changes from run to run, the
    tolerances are those tests/test_registration.py::test_hip_deformable_registration_vs_reference_golden holds the same path to on
    one host (theta 1e-3, flow 5e-3, warped images 1e-2), and no label pixel may flip."""
    data_dir, set_name, cfg = _dataset(tmp_path, do_deformable=deformable)
    host = VR.FewshotRegReader(data_dir, set_name, cfg, mode="eval")
    src = DE.DeviceEvalSource(data_dir, set_name, cfg, DEV)
    src.warm()
    assert len(src) == len(host) == 3
    supports = set()
    for idx in range(len(host)):
        AC.seed_all(40 + idx)
        h = host[idx]
        h_state = AC.rng_state()
        AC.seed_all(40 + idx)
        d = src.item(idx)
        assert AC.rng_state() == h_state
        assert src.k == host.fewshot_reader.k
        assert d["pid"] == h["pid"] and d["supp_pids"] == h["supp_pids"] and d["class_id"] == h["class_id"]
        supports.add(d["supp_pids"][0])
        pre = src.pre
        h_pre = {"support_images": h["original_support_images"][0][0][:, [0]], "support_labels": h["original_support_labels"][0][0],
                 "query_images": h["query_images"], "query_labels": h["query_labels"]}
        for key, hv in h_pre.items():
            assert tuple(pre[key].shape) == tuple(hv.shape) and pre[key].dtype == hv.dtype == torch.float32 and pre[key].is_cuda, key
            assert torch.equal(pre[key].cpu(), hv), (idx, key)
        assert torch.equal(d["query_images"], pre["query_images"]) and torch.equal(d["query_labels"], pre["query_labels"])
        got = {"support_images": d["support_images"][0][0], "support_labels": d["support_labels"][0][0],
               "appr_query_labels": d["appr_query_labels"], "warped_supp": d["warped_supp"]}
        want = {"support_images": h["support_images"][0][0], "support_labels": h["support_labels"][0][0],
                "appr_query_labels": h["appr_query_labels"], "warped_supp": h["warped_supp"]}
        for key in got:
            assert tuple(got[key].shape) == tuple(want[key].shape) and got[key].dtype == want[key].dtype and got[key].is_cuda, key
        if not deformable:
            for key in got:
                assert torch.equal(got[key].cpu(), want[key]), (idx, key)
            assert torch.equal(d["registration_field"].cpu(), h["registration_field"])
        else:
            (th, fl), (hth, hfl) = d["registration_field"], h["registration_field"]
            diffs = {"theta": (th.cpu() - hth).abs().max().item(), "flow": (fl.cpu() - hfl).abs().max().item(),
                     "support_images": (got["support_images"].cpu() - want["support_images"]).abs().max().item(),
                     "warped_supp": (got["warped_supp"].cpu() - want["warped_supp"]).abs().max().item()}
            flips = {key: int((got[key].cpu() != want[key]).sum().item()) for key in ("support_labels", "appr_query_labels")}
            print(f"item {idx} deformable: max |diff| {diffs}, label flips {flips}")
            assert diffs["theta"] < 1e-3 and diffs["flow"] < 5e-3                       # tests/test_registration.py:206-208
            assert diffs["support_images"] < 1e-2 and diffs["warped_supp"] < 1e-2        # tests/test_registration.py:206,209
            assert flips == {"support_labels": 0, "appr_query_labels": 0}
    assert len(supports) > 1, "the seeds must exercise the support choice"


def test_item_makes_no_host_synchronisation(tmp_path):
    """after warm-up an item copies nothing back: checked with torch.cuda.set_sync_debug_mode("error") around the call (every
    synchronising torch call — .cpu(), .item(), a blocking copy — raises under it), for both registration settings"""
    for deformable in (False, True):
        data_dir, set_name, cfg = _dataset(tmp_path, do_deformable=deformable)
        src = DE.DeviceEvalSource(data_dir, set_name, cfg, DEV)
        src.warm()
        random.seed(3)
        for idx in range(len(src)):
            src.item(idx)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for idx in range(len(src)):
                src.item(idx)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------- data set
def _eval_cfg(cfg):
    model = dict(load_cfg(), **cfg)
    model["n_iter_refinement"] = model["n_test_iter_refinement"]
    return model


def _build_net(cfg, conv_math=None):
    from rpnet_amd.modules import RP_Net
    from rpnet_amd.utils.seeding import seed_module_
    net = RP_Net(cfg={"align": True, "backbone": "UNet"}, backbone_cfg=cfg).to(DEV)
    seed_module_(net)
    net.schedule.conv_math = conv_math
    return net.eval()


def _plain(dicts):
    aff, few, ref = dicts
    return dict(aff), dict(few), {name: dict(v) for name, v in ref.items()}


def _recording_segmenter(net, batch, graphed):
    """a VolumeSegmenter that keeps every result (the parent path hands its tallies to nobody)"""
    from rpnet_amd.volume import VolumeSegmenter

    class Rec(VolumeSegmenter):
        results = []

        def __call__(self, *a, **kw):
            res = super().__call__(*a, **kw)
            self.results.append(res)
            return res
    return Rec(net, batch=batch, graphed=graphed)


def _driver_lines(text):
    return [l for l in text.splitlines() if l[:1].isdigit() or l.startswith("Liver,")]


def _dice_values(dicts):
    aff, few, ref = dicts
    return [v for d in (aff, few) for vs in d.values() for v in vs] + [v for r in ref.values() for vs in r.values() for v in vs]


def test_dataset_evaluation_equals_the_host_item_path(tmp_path, capsys):
    """evaluate_dataset against tools.eval_driver.evaluate_on_device over the host reader, same seeded data set and `random` seed,
    affine registration only.  f32 convolutions (a Schedule on the net), eager, batch 8 on both sides: the three dictionaries are
    EQUAL and the tally tables equal integer for integer; the counts_out=None path (the parent's, recorded here) gives what it gave;
    the masks written by save_pred are the same files' contents; the printed lines differ only in the second similarity figure, and
    both figures equal net.registration.NCC to 4 decimals.  Default arithmetic through the captured graph, each side on a fresh net:
    the largest Dice difference is at most 1e-3 (the bar of tests/test_gpu_volume.py between call histories)."""
    from net.registration import NCC
    from rpnet_amd.utils import nrrd
    from tools.eval_driver import evaluate_on_device
    data_dir, set_name, cfg = _dataset(tmp_path / "data", do_deformable=False)
    cfg = _eval_cfg(cfg)
    T = cfg["n_iter_refinement"]
    host = VR.FewshotRegReader(data_dir, set_name, cfg, mode="eval")
    src = DE.DeviceEvalSource(data_dir, set_name, cfg, DEV)
    src.warm()
    dir_a, dir_b = str(tmp_path / "pred_host"), str(tmp_path / "pred_device")

    rec = _recording_segmenter(_build_net(cfg, "f32"), 8, False)
    random.seed(77)
    capsys.readouterr()
    want = _plain(evaluate_on_device(rec.net, host, cfg, batch_size=8, save_pred=dir_a, graphed=False, segmenter=rec))
    lines_a = _driver_lines(capsys.readouterr().out)
    tables = {}
    random.seed(77)
    got = _plain(DE.evaluate_dataset(_build_net(cfg, "f32"), src, cfg, batch=8, graphed=False, save_pred=dir_b, out=tables))
    lines_b = _driver_lines(capsys.readouterr().out)
    print("host items  ", want, "\ndevice items", got)
    assert got == want
    assert len(want[1]["Liver"]) == 3 and sorted(want[2]["Liver"]) == list(range(T)) and all(v is not None and v > 0 for v in want[0]["Liver"])
    assert tables["counts"].shape == (3, T + 2, 1, 3) and tables["counts"].dtype == np.int64 and tables["ncc"].shape == (3, 2)
    assert len(rec.results) == 3
    for j, res in enumerate(rec.results):
        assert res.counts.dtype == np.int64 and np.array_equal(res.counts, tables["counts"][j]), j
        assert res.dice["fewshot"] == [got[1]["Liver"][j]] and res.dice["affine"] == [got[0]["Liver"][j]]
    files = sorted(os.listdir(dir_a))
    assert files == sorted(os.listdir(dir_b)) and len(files) == 3
    for f in files:
        a, b = nrrd.read(os.path.join(dir_a, f)), nrrd.read(os.path.join(dir_b, f))
        assert a[0].dtype == np.uint8 and b[1]["encoding"] == "gzip" and np.array_equal(a[0], b[0]), f
    # the printed lines: "j pid affine (ncc) ..." against "j pid affine (ncc, ncc2) ..."
    assert len(lines_a) == len(lines_b) == 4 and lines_a[3] == lines_b[3]
    random.seed(77)
    for j in range(3):
        head_a, tail_a = lines_a[j].split(") ", 1)
        head_b, tail_b = lines_b[j].split(") ", 1)
        (start_a, fig_a), (start_b, figs_b) = head_a.rsplit("(", 1), head_b.rsplit("(", 1)
        assert tail_a == tail_b and start_a == start_b
        t = tables["ncc"][j]
        assert figs_b == f"{t[0]:.4f}, {t[1]:.4f}"
        # the parent prints torch's fp32 figure to 4 decimals: half a unit of the print (5e-5) plus fp32 summation error (relative
        # 1e-5 at most over 8e4 elements of magnitude <= 1) is below 1e-4
        assert abs(float(fig_a) - t[0]) < 1e-4
        s = host[j]
        qi = s["query_images"].to(DEV)
        ncc = [NCC(qi, s["warped_supp"].unsqueeze(1).to(DEV)).item(), NCC(qi, s["support_images"][0][0].to(DEV)).item()]
        assert np.abs(t - ncc).max() < 1e-4 and t[0] != t[1], (lines_b[j], ncc)

    random.seed(77)
    want_g = _plain(evaluate_on_device(_build_net(cfg), host, cfg, batch_size=8, graphed=True))
    random.seed(77)
    got_g = _plain(DE.evaluate_dataset(_build_net(cfg), src, cfg, batch=8, graphed=True))
    va, vb = _dice_values(want_g), _dice_values(got_g)
    worst = max(abs(x - y) for x, y in zip(va, vb))
    print(f"default arithmetic, graphed: largest Dice difference {worst:.2e} over {len(va)} values")
    assert len(va) == len(vb) == 3 * (T + 2) and worst <= 1e-3
