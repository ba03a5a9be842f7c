"""Label fusion on the device (csrc/fusion.hip through include/rpnet_fusion_abi.h and rpnet_amd/fusion.py) against the numpy restatement
of tests/fusion_cases.py: every mask, pattern volume, histogram, label / w table, statistics row, rater row and iteration count EQUAL,
the float64 values bit for bit, the probability plane equal to float32(w).  Every call is made twice and gives the same bits."""
import ctypes
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

from rpnet_amd import dataset_eval as DE
from rpnet_amd import fusion as F
from rpnet_amd import hip
from rpnet_amd.utils import volume_reader as VR
from tests import augment_cases as AC
from tests import fusion_cases as FC
from tests.helpers import load_cfg
from tests.reader_cases import config_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TORCH = {"u8": torch.uint8, "i32": torch.int32, "i64": torch.int64, "f32": torch.float32}


def dev(a, dtype=torch.uint8, offset=0):
    """`a` on the device as `dtype`; offset: that many bytes into a larger allocation"""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    if not offset:
        return t.to(DEV)
    n, item = t.numel(), t.element_size()
    buf = torch.zeros((n + offset // item + 16,), dtype=dtype, device=DEV)
    view = buf[offset // item:offset // item + n].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() - buf.data_ptr() == offset
    return view


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def run_fuse(raters, kind="u8", truth=None, truth_kind="i32", offset=0, **kw):
    """F.fuse twice on the device against FC.fuse: everything equal; -> (FusionResult, restatement)"""
    want = FC.fuse(raters, truth=truth, **kw)
    d_raters = [dev(r, TORCH[kind], offset) for r in raters]
    d_truth = None if truth is None else dev(truth, TORCH[truth_kind], offset)
    R, shape = len(raters), raters[0].shape
    runs = []
    for _ in range(2):
        res = F.fuse(d_raters, truth=d_truth, prob=True, **kw)
        hist, w, label, patterns = (t.cpu().numpy() for t in F._last_table(shape, R, DEV))
        runs.append(dict(mask=res.mask.cpu().numpy(), prob=res.prob.cpu().numpy(), stats=res.stats.cpu().numpy(), rater_f=res.rater_f.cpu().numpy(),
                         rater_i=res.rater_i.cpu().numpy(), counts=None if truth is None else res.counts.cpu().numpy(), hist=hist, w=w,
                         label=label, patterns=patterns))
    a, b = runs
    for key in a:
        if a[key] is not None:
            assert a[key].tobytes() == b[key].tobytes(), f"{key}: two runs differ"
    assert np.array_equal(a["mask"], want["mask"])
    assert np.array_equal(a["patterns"].astype(np.uint16), want["patterns"][-1]) and np.array_equal(a["hist"], want["hist"][-1])
    assert np.array_equal(a["label"], want["label"][-1]) and np.array_equal(bits(a["w"]), bits(want["w"][-1]))
    assert np.array_equal(a["stats"], want["stats"]), (a["stats"], want["stats"])
    assert np.array_equal(a["rater_i"], want["rater_i"])
    assert np.array_equal(bits(a["rater_f"]), bits(want["rater_f"])), (a["rater_f"], want["rater_f"])
    assert a["prob"].dtype == np.float32 and np.array_equal(a["prob"].view(np.int32), want["prob"].view(np.int32))
    if truth is not None:
        assert np.array_equal(a["counts"], want["counts"])
    return res, want


METHOD_KW = [dict(method="vote"), dict(method="weighted"), dict(method="staple"), dict(method="staple", consensus=False)]


def with_weights(kw, R):
    return dict(kw, weights=[0.25 + 0.5 * r for r in range(R)]) if kw["method"] == "weighted" else kw


@pytest.mark.parametrize("shape", FC.SHAPES)
@pytest.mark.parametrize("R", FC.RATER_COUNTS)
def test_shapes_and_rater_counts(shape, R):
    truth, raters = FC.raters_for(shape, R, seed=sum(shape) + R)
    for kw in METHOD_KW:
        run_fuse(raters, truth=truth, **with_weights(kw, R))
    d = [dev(r) for r in raters]
    for _ in range(2):
        patterns, hist = F.pattern_histogram(d, 1)
        assert np.array_equal(patterns.cpu().numpy().astype(np.uint16), FC.patterns_of(raters, 1))
        assert np.array_equal(hist.cpu().numpy(), FC.histogram(FC.patterns_of(raters, 1), R))


def test_second_trip_of_a_block():
    """more voxels than 1024 blocks of 4096: every block makes a second trip, the last lanes of which lie beyond the volume"""
    shape = FC.TWO_TRIPS
    assert shape[0] * shape[1] * shape[2] > 1024 * 4096
    truth = FC.blob(shape, 5)
    raters = [FC.perturbed(truth, 0.2, 0.01, 60), FC.perturbed(truth, 0.1, 0.02, 61), FC.perturbed(truth, 0.3, 0.01, 62)]
    run_fuse(raters, truth=truth, method="staple")
    run_fuse(raters[:2], truth=truth, method="vote", truth_kind="u8")


def special_inputs():
    shape = (3, 9, 13)
    z, o, b = np.zeros(shape, np.uint8), np.ones(shape, np.uint8), FC.blob(shape, 4)
    one = b.copy()
    one[1, 4, 6] ^= 1
    return {"empty": [z] * 5, "full": [o] * 5, "same": [b] * 5, "complement": [b, b, b, 1 - b], "one_disputed": [b, b, one, b],
            "even_split": [b, 1 - b], "empty12": [z] * 12, "full1": [o]}


@pytest.mark.parametrize("name", sorted(special_inputs()))
def test_special_inputs(name):
    raters = special_inputs()[name]
    for kw in METHOD_KW:
        res, want = run_fuse(raters, truth=raters[0], **with_weights(kw, len(raters)))
    if name == "one_disputed":
        assert want["stats"][0, 3] == 1
    if name == "even_split":
        assert not run_fuse(raters, method="vote")[1]["mask"].any()


@pytest.mark.parametrize("kind", ["u8", "i32", "i64", "f32"])
def test_every_element_kind_offset_pointers_and_a_truth_of_another_kind(kind):
    truth, raters = FC.raters_for((2, 17, 241), 5, seed=9, labels=2)
    other = {"u8": "i64", "i32": "f32", "i64": "u8", "f32": "i32"}[kind]
    item = {"u8": 1, "i32": 4, "i64": 8, "f32": 4}
    for offset in (0, 16, 8 if 8 in (item[kind], item[other]) else 20):
        # 0 and 16: the 16-byte paths; 8 or 20: aligned to the elements only, so whole lanes take the element-wise path
        run_fuse(raters, kind=kind, truth=truth, truth_kind=other, offset=offset, method="staple", classes=(2,))
        run_fuse(raters, kind=kind, truth=truth, truth_kind=other, offset=offset, method="vote", classes=(1, 2))


def test_vote_and_weighted_options():
    truth, raters = FC.raters_for((3, 9, 13), 5, seed=1)
    for k in (1, 2, 3, 5):
        run_fuse(raters, truth=truth, method="vote", min_votes=k)
    _, two = FC.raters_for((3, 9, 13), 2, seed=2)
    for k in (1, 2):
        run_fuse(two, method="vote", min_votes=k)
    run_fuse(raters, method="weighted", weights=[0.5, 1.0, 1.5, 2.0, 0.0])                   # a zero weight
    tie = [np.array([[[0, 1, 0, 1, 1]]], np.uint8), np.array([[[0, 0, 1, 1, 1]]], np.uint8), np.array([[[1, 0, 0, 0, 1]]], np.uint8)]
    res, want = run_fuse(tie, method="weighted", weights=[1.0, 1.0, 2.0])                     # 2 s == total exactly on patterns 0b100 and 0b011
    assert want["label"][0][4] == 0 and want["w"][0][4] == 0.5 and list(want["mask"].ravel()) == [0, 0, 0, 0, 1]


def test_staple_options():
    truth, raters = FC.phantom()
    full, want = run_fuse(raters, truth=truth, method="staple", consensus=False)
    its = int(want["stats"][0, 4])
    assert want["stats"][0, 5] == 1 and 2 < its < 100                      # tol reached at a known iteration of the restatement
    _, cut = run_fuse(raters, method="staple", consensus=False, max_iter=its - 1)
    assert list(cut["stats"][0, 4:]) == [its - 1, 0]
    _, one = run_fuse(raters, method="staple", max_iter=1)
    assert list(one["stats"][0, 4:]) == [1, 0]
    run_fuse(raters, method="staple", tol=0.0, max_iter=7)
    run_fuse(raters, method="staple", tol=1e-3)
    perfect = [truth] + [FC.perturbed(truth, 0.3, 0.02, 40 + i) for i in range(3)]
    _, clamped = run_fuse(perfect, method="staple", max_iter=60)
    assert FC.HI in clamped["rater_f"][0, 0]                               # the clamp reached, with a perfect rater under consensus


def test_three_classes_out_given_counts_added_sentinels_and_guards():
    truth, raters = FC.raters_for((3, 9, 13), 3, seed=2, labels=3)
    want = FC.fuse(raters, classes=(1, 2, 3), method="staple", truth=truth, counts=np.full((3, 3), 1000, np.int64))
    d = [dev(r) for r in raters]
    n = truth.size
    guard = 64
    out_buf = torch.full((n + 2 * guard,), 0xA5, dtype=torch.uint8, device=DEV)
    out = out_buf[guard:guard + n].view(truth.shape)
    counts = torch.full((3, 3), 1000, dtype=torch.int64, device=DEV)
    tabs = {"stats": (torch.int64, (3, 6)), "rater_f": (torch.float64, (3, 3, 2)), "rater_i": (torch.int64, (3, 3, 3))}
    bufs = {k: torch.full((int(np.prod(s)) + 16,), -7, dtype=dt, device=DEV) for k, (dt, s) in tabs.items()}
    views = {k: bufs[k][8:8 + int(np.prod(s))].view(s) for k, (dt, s) in tabs.items()}
    res = F.fuse(d, classes=(1, 2, 3), method="staple", truth=dev(truth, torch.int64), counts=counts, out=out, **views)
    assert res.mask.data_ptr() == out.data_ptr() and res.counts is counts
    assert np.array_equal(out.cpu().numpy(), want["mask"]) and np.array_equal(counts.cpu().numpy(), want["counts"])
    assert (out_buf[:guard] == 0xA5).all() and (out_buf[guard + n:] == 0xA5).all()
    for k in tabs:
        assert (bufs[k][:8] == -7).all() and (bufs[k][8 + views[k].numel():] == -7).all(), k
    assert np.array_equal(views["stats"].cpu().numpy(), want["stats"]) and np.array_equal(views["rater_i"].cpu().numpy(), want["rater_i"])
    assert np.array_equal(bits(views["rater_f"].cpu().numpy()), bits(want["rater_f"]))
    assert set(np.unique(want["mask"])) <= {0, 1, 2, 3} and (want["mask"] == 3).any()


def test_merge_keeps_the_first_class_where_two_classes_win_a_voxel():
    """min_votes = 1 of raters that disagree between the classes: both class 1 and class 2 win such a voxel on their own; written in
    the order (1, 2) it keeps 1, in the order (2, 1) it keeps 2.  A pass 2 that overwrote non-zero voxels under merge would give the
    other class there."""
    _, raters = FC.raters_for((3, 9, 13), 3, seed=2, labels=3)
    stack = np.stack(raters)
    both = (stack == 1).any(0) & (stack == 2).any(0)
    assert both.sum() >= 5
    for method, kw in (("vote", dict(min_votes=1)), ("weighted", dict(weights=[1.0, 1.0, 1.0]))):
        for order in ((1, 2), (2, 1), (1, 2, 3)):
            res, want = run_fuse(raters, method=method, classes=order, **kw)
            if method == "vote":
                assert (res.mask.cpu().numpy()[both] == order[0]).all() and (want["mask"][both] == order[0]).all()
    # every class written alone wins those voxels: the restatement's merge is what keeps the first
    assert (FC.fuse(raters, method="vote", min_votes=1, classes=(2,))["mask"][both] == 2).all()


@pytest.mark.parametrize("shape", [(1, 1, 17), (1, 17, 241), (3, 9, 13)])
def test_guard_words_behind_prob_counts_and_unaligned_outputs(shape):
    """prob, counts and out in buffers of sentinels, at byte offsets that are no multiple of 16 (out at an odd one), the volumes' tails
    no multiple of 16 voxels: the words before and behind every output stay"""
    truth, raters = FC.raters_for(shape, 5, seed=13)
    want = FC.fuse(raters, method="staple", truth=truth, counts=np.full((1, 3), 7, np.int64))
    n = truth.size
    d = [dev(r, torch.uint8, 1 + 2 * i) for i, r in enumerate(raters)]       # uint8 raters at odd addresses
    prob_buf = torch.full((n + 64,), -3.0, dtype=torch.float32, device=DEV)
    out_buf = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    cnt_buf = torch.full((3 + 8,), 7, dtype=torch.int64, device=DEV)
    for p_off, o_off in ((3, 5), (5, 16), (7, 33)):
        prob_buf.fill_(-3.0)
        out_buf.fill_(0xA5)
        cnt_buf.fill_(7)
        prob = prob_buf[p_off:p_off + n].view(shape)
        out = out_buf[o_off:o_off + n].view(shape)
        counts = cnt_buf[3:6].view(1, 3)
        res = F.fuse(d, method="staple", truth=dev(truth, torch.float32), counts=counts, out=out, prob=prob)
        assert res.prob.data_ptr() == prob.data_ptr() and prob.data_ptr() % 16 != 0
        assert np.array_equal(out.cpu().numpy(), want["mask"]) and np.array_equal(counts.cpu().numpy(), want["counts"])
        assert np.array_equal(prob.cpu().numpy().view(np.int32), want["prob"].view(np.int32))
        assert (prob_buf[:p_off] == -3.0).all() and (prob_buf[p_off + n:] == -3.0).all()
        assert (out_buf[:o_off] == 0xA5).all() and (out_buf[o_off + n:] == 0xA5).all()
        assert (cnt_buf[:3] == 7).all() and (cnt_buf[6:] == 7).all()


def raw_fuse(raters, out, stats, rater_f, rater_i, ws, ws_bytes=None, R=None, kind=0, cls=1, dims=None, method=2, min_votes=1, weights=None,
             consensus=1, max_iter=10, tol=1e-9, merge=0, prob=None, truth=None, truth_kind=0, counts=None, counts_row=0, row=0, n_rows=1):
    """rpnet_fusion_fuse itself -> (status, error string)"""
    lib = hip.load()
    R = len(raters) if R is None else R
    D, H, W = dims or raters[0].shape
    arr = (ctypes.c_void_p * max(len(raters), 1))(*[None if t is None else t.data_ptr() for t in raters])
    wts = None if weights is None else (ctypes.c_double * len(weights))(*weights)
    p = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())  # noqa: E731
    rc = lib.rpnet_fusion_fuse(arr, R, kind, cls, D, H, W, method, min_votes, wts, consensus, max_iter, tol, p(out), merge, p(prob), p(truth),
                               truth_kind, p(counts), counts_row, p(stats), p(rater_f), p(rater_i), row, n_rows, p(ws),
                               (ws.numel() if torch.is_tensor(ws) else 0) if ws_bytes is None else ws_bytes, hip.stream())
    return rc, lib.rpnet_last_error_string().decode()


def test_workspace_guard_and_raw_entry_points():
    """the C ABI called directly: a guard word behind the workspace and behind patterns and hist stays; the workspace size is the header's"""
    truth, raters = FC.raters_for((2, 17, 241), 5, seed=3)
    d = [dev(r) for r in raters]
    n = truth.size
    need = hip.query("rpnet_fusion_workspace_bytes", 2, 17, 241, 5)
    assert need == F._workspace_layout(5, n)[1] == 64 + 16 * 32 + 32 + (2 * n + 15) // 16 * 16
    ws = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    out = torch.empty(truth.shape, dtype=torch.uint8, device=DEV)
    stats = torch.zeros((1, 6), dtype=torch.int64, device=DEV)
    rf, ri = torch.zeros((1, 5, 2), dtype=torch.float64, device=DEV), torch.zeros((1, 5, 3), dtype=torch.int64, device=DEV)
    rc, err = raw_fuse(d, out, stats, rf, ri, ws, ws_bytes=need, max_iter=100)
    assert rc == 0, err
    want = FC.fuse(raters, method="staple")
    assert np.array_equal(out.cpu().numpy(), want["mask"]) and (ws[need:] == 0x5A).all()
    pat_buf = torch.full((n + 32,), -3, dtype=torch.int16, device=DEV)
    hist_buf = torch.full((32 + 8,), -3, dtype=torch.int64, device=DEV)
    arr = (ctypes.c_void_p * 5)(*[t.data_ptr() for t in d])
    hip.call("rpnet_fusion_patterns", arr, 5, 0, 1, 2, 17, 241, pat_buf[16:].data_ptr(), hist_buf[4:].data_ptr())
    assert np.array_equal(pat_buf[16:16 + n].cpu().numpy().astype(np.uint16), want["patterns"][0].ravel())
    assert np.array_equal(hist_buf[4:36].cpu().numpy(), want["hist"][0])
    assert (pat_buf[:16] == -3).all() and (pat_buf[16 + n:] == -3).all() and (hist_buf[:4] == -3).all() and (hist_buf[36:] == -3).all()


def test_captured_graph_of_fuse_replayed_twice():
    truth, raters = FC.phantom()
    d = [dev(r) for r in raters]
    d_truth = dev(truth, torch.float32)
    want = FC.fuse(raters, method="staple", truth=truth, counts=np.zeros((1, 3), np.int64))
    counts = torch.zeros((1, 3), dtype=torch.int64, device=DEV)
    out = torch.empty(truth.shape, dtype=torch.uint8, device=DEV)
    F.fuse(d, method="staple", truth=d_truth, counts=counts, out=out, prob=True)            # the workspace is allocated before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            res = F.fuse(d, method="staple", truth=d_truth, counts=counts, out=out, prob=True)
    for replay in range(2):
        counts.zero_()
        out.fill_(9)
        res.prob.fill_(-1.0)
        res.stats.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want["mask"]) and np.array_equal(counts.cpu().numpy(), want["counts"]), replay
        assert np.array_equal(res.stats.cpu().numpy(), want["stats"]) and np.array_equal(bits(res.rater_f.cpu().numpy()), bits(want["rater_f"]))
        assert np.array_equal(res.prob.cpu().numpy().view(np.int32), want["prob"].view(np.int32))


def test_refusals_launch_nothing():
    truth, raters = FC.raters_for((3, 9, 13), 3, seed=5)
    d = [dev(r) for r in raters]
    need = hip.query("rpnet_fusion_workspace_bytes", 3, 9, 13, 3)
    ws = torch.full((need + 16,), 0x5A, dtype=torch.uint8, device=DEV)
    out = torch.full(truth.shape, 77, dtype=torch.uint8, device=DEV)
    stats = torch.full((2, 6), -5, dtype=torch.int64, device=DEV)
    rf, ri = torch.full((2, 3, 2), -5.0, dtype=torch.float64, device=DEV), torch.full((2, 3, 3), -5, dtype=torch.int64, device=DEV)
    counts = torch.full((2, 3), -5, dtype=torch.int64, device=DEV)
    t = dev(truth)
    base = dict(raters=d, out=out, stats=stats, rater_f=rf, rater_i=ri, ws=ws, n_rows=2)
    nan, inf = float("nan"), float("inf")
    bad = [dict(out=None), dict(stats=None), dict(rater_f=None), dict(rater_i=None), dict(ws=None), dict(raters=[d[0], None, d[2]]),
           dict(R=0), dict(R=13), dict(kind=4), dict(kind=-1), dict(method=3), dict(method=-1), dict(cls=0), dict(cls=256),
           dict(min_votes=0), dict(min_votes=4), dict(method=1), dict(method=1, weights=[1.0, -1.0, 1.0]), dict(method=1, weights=[1.0, nan, 1.0]),
           dict(method=1, weights=[1.0, inf, 1.0]), dict(method=1, weights=[0.0, 0.0, 0.0]), dict(max_iter=0), dict(tol=-1e-9), dict(tol=nan),
           dict(row=2), dict(row=-1), dict(truth=t, counts=counts, counts_row=2), dict(truth=t), dict(counts=counts),
           dict(truth=t, counts=counts, truth_kind=7), dict(dims=(0, 9, 13)), dict(dims=(3, 1025, 13)), dict(ws_bytes=need - 1),
           dict(ws=ws.data_ptr() + 8, ws_bytes=need), dict(out=d[1]), dict(out=d[2].data_ptr() + 5), dict(stats=stats.data_ptr() + 4)]
    for over in bad:
        rc, err = raw_fuse(**dict(base, **over))
        assert rc != 0 and err.startswith("fusion_fuse:"), (over, rc, err)
    pat = torch.full(truth.shape, -3, dtype=torch.int16, device=DEV)
    hist = torch.full((8,), -3, dtype=torch.int64, device=DEV)
    lib = hip.load()
    arr = (ctypes.c_void_p * 3)(*[x.data_ptr() for x in d])
    for args in ((arr, 0, 0, 1, 3, 9, 13, pat.data_ptr(), hist.data_ptr()), (arr, 3, 9, 1, 3, 9, 13, pat.data_ptr(), hist.data_ptr()),
                 (arr, 3, 0, 0, 3, 9, 13, pat.data_ptr(), hist.data_ptr()), (arr, 3, 0, 1, 3, 9, 2000, pat.data_ptr(), hist.data_ptr()),
                 (arr, 3, 0, 1, 3, 9, 13, None, hist.data_ptr()), (arr, 3, 0, 1, 3, 9, 13, pat.data_ptr(), None),
                 (arr, 3, 0, 1, 3, 9, 13, pat.data_ptr(), hist.data_ptr() + 4), (None, 3, 0, 1, 3, 9, 13, pat.data_ptr(), hist.data_ptr())):
        assert lib.rpnet_fusion_patterns(*args, hip.stream()) != 0 and lib.rpnet_last_error_string().decode().startswith("fusion_patterns:")
    for q in ((0, 9, 13, 3), (3, 9, 13, 0), (3, 9, 13, 13), (3, 9, 1025, 3)):
        assert hip.query("rpnet_fusion_workspace_bytes", *q) == 0
    torch.cuda.synchronize()
    assert (out == 77).all() and (stats == -5).all() and (rf == -5.0).all() and (ri == -5).all() and (counts == -5).all()
    assert (ws == 0x5A).all() and (pat == -3).all() and (hist == -3).all()
    for r in range(3):
        assert np.array_equal(d[r].cpu().numpy(), raters[r])
    # the Python layer
    cpu = [torch.from_numpy(r) for r in raters]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.fuse(cpu)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.pattern_histogram(cpu)
    for kw in (dict(method="median"), dict(min_votes=0), dict(min_votes=4), dict(method="weighted"), dict(method="weighted", weights=[1, 1]),
               dict(method="weighted", weights=[0, 0, 0]), dict(weights=[1, 1, 1]), dict(max_iter=0), dict(tol=-1.0), dict(classes=()),
               dict(classes=(0,)), dict(classes=(256,)), dict(counts=counts[:1]), dict(out=torch.empty((3, 9, 12), dtype=torch.uint8, device=DEV)),
               dict(truth=dev(truth[:2]))):
        with pytest.raises(ValueError):
            F.fuse(d, **kw)
    with pytest.raises(ValueError):
        F.fuse(d + [dev(raters[0], torch.int32)])
    with pytest.raises(ValueError):
        F.fuse(d * 5)


# -------------------------------------------------------------------------------------------------------- evaluation over runs
CASE = {"data": dict(n_volumes=3, classes=("Liver",), shape=(22, 72, 72), seed=11),
        "cfg": dict(num_slice=20, num_x=72, num_y=72, crop_size=[64, 64], k=4)}


def dataset(tmp_path, **over):
    data_dir, set_name, csv_dir = VR.write_synthetic_dataset(str(tmp_path), **CASE["data"])
    return data_dir, set_name, dict(config_for(CASE, csv_dir), use_registration_mask=False, **over)


def eval_cfg(cfg):
    model = dict(load_cfg(), **cfg)
    model["n_iter_refinement"] = model["n_test_iter_refinement"]
    return model


def build_net(cfg):
    from rpnet_amd.modules import RP_Net
    from rpnet_amd.utils.seeding import seed_module_
    net = RP_Net(cfg={"align": True, "backbone": "UNet"}, backbone_cfg=cfg).to(DEV)
    seed_module_(net)
    net.schedule.conv_math = "f32"
    return net.eval()


def test_item_with_a_given_support_matches_the_host_reader(tmp_path):
    """DeviceEvalSource.item(idx, support=s) against the host volume reader's __getitem__(idx, supp_idx=s): the same support, the same
    gathered tensors, and the `random` generator in the same state afterwards (the draw is made, then overridden)"""
    data_dir, set_name, cfg = dataset(tmp_path, do_deformable=False)
    src = DE.DeviceEvalSource(data_dir, set_name, cfg, DEV)
    src.warm()
    host = VR.FewshotVolumeReader(data_dir, set_name, cfg, mode="eval")
    for idx in range(len(src)):
        for s in range(3):
            if s == host.indices[idx][1]:
                continue
            AC.seed_all(5 + idx)
            h = host.__getitem__(idx, supp_idx=s)
            state = AC.rng_state()
            AC.seed_all(5 + idx)
            d = src.item(idx, support=s)
            assert AC.rng_state() == state
            assert d["supp_pids"] == h["supp_pids"] == [(0, s)] and d["pid"] == h["pid"]
            table = np.asarray(src.pre["support_slices"]).ravel()
            assert torch.equal(src.pre["support_images"][:, 0].cpu(), h["support_images"][0][0][0][table])
            assert torch.equal(src.pre["support_labels"].cpu(), h["support_labels"][0][0][0][table])
            assert torch.equal(src.pre["query_images"][:, 0].cpu(), h["query_images"][0][0][0])
    AC.seed_all(1)
    a = src.item(0)
    state = AC.rng_state()
    AC.seed_all(1)
    b = src.item(0, support=None)
    assert AC.rng_state() == state and a["supp_pids"] == b["supp_pids"]
    with pytest.raises(ValueError):
        src.item(0, support=3)


def plain(dicts):
    aff, few, ref = dicts
    return dict(aff), dict(few), {name: dict(v) for name, v in ref.items()}


def test_evaluate_runs_equals_plain_calls_and_fuses_their_masks(tmp_path, capsys):
    """n_runs = 2 under one seed: run r's tables and lines are those of the r-th of two plain evaluate_dataset calls; the fused Dice
    table, statistics and rater rows equal the restatement applied to out["masks"] with the cached query mask as the truth"""
    data_dir, set_name, cfg = dataset(tmp_path, do_deformable=False)
    cfg = eval_cfg(cfg)
    src = DE.DeviceEvalSource(data_dir, set_name, cfg, DEV)
    src.warm()
    net = build_net(cfg)
    random.seed(31)
    capsys.readouterr()
    want, want_out = [], []
    for r in range(2):
        o = {}
        want.append(plain(DE.evaluate_dataset(net, src, cfg, batch=8, graphed=False, out=o)))
        want_out.append(o)
    lines_plain = capsys.readouterr().out.splitlines()
    assert all("masks" not in o for o in want_out)
    for fuse in ("staple", "vote"):
        random.seed(31)
        results, outs, tables = F.evaluate_runs(net, src, dict(cfg, n_runs=2), fuse=fuse, batch=8, graphed=False)
        text = capsys.readouterr().out.splitlines()
        assert [plain(r) for r in results] == want
        for r in range(2):
            assert np.array_equal(outs[r]["counts"], want_out[r]["counts"]) and np.array_equal(outs[r]["ncc"], want_out[r]["ncc"])
        half = len(lines_plain) // 2
        assert text[0] == "1 / 2" and text[1:1 + half] == lines_plain[:half] and text[1 + half] == "2 / 2"
        assert text[2 + half:2 + 2 * half] == lines_plain[half:] and text[2 + 2 * half] == "=======Average performance========="
        few = np.array([want[0][1]["Liver"], want[1][1]["Liver"]])
        aff = np.array([want[0][0]["Liver"], want[1][0]["Liver"]])
        assert text[3 + 2 * half] == (f"Liver, affine {aff.mean(1).mean()} + {aff.mean(1).std()}, fewshot {few.mean(1).mean()} + "
                                      f"{few.mean(1).std()} ")
        assert tables["counts"].shape == (3, 1, 3) and tables["stats"].shape == (3, 1, 6) and tables["rater_f"].shape == (3, 1, 2, 2)
        fused_lines = [l for l in text if " fused " in l]
        assert len(fused_lines) == 4 and fused_lines[-1].startswith("Liver, fused ")
        for j in range(3):
            masks = [outs[r]["masks"][j].cpu().numpy() for r in range(2)]
            c, qv = src.reader.indices[j]
            truth = src.volume(c, qv)[1].cpu().numpy()
            ref = FC.fuse(masks, method=fuse, truth=truth)
            assert np.array_equal(tables["counts"][j], ref["counts"]) and np.array_equal(tables["stats"][j], ref["stats"]), j
            assert np.array_equal(tables["rater_i"][j], ref["rater_i"]) and np.array_equal(bits(tables["rater_f"][j]), bits(ref["rater_f"]))
            assert np.array_equal(tables["masks"][j].cpu().numpy(), ref["mask"])
            assert f" fused {DE.dice_from_counts(ref['counts'])[0]} (runs " in fused_lines[j]
    random.seed(31)
    results, outs, tables = F.evaluate_runs(net, src, cfg, n_runs=None, batch=8, graphed=False, n_items=1)      # the yaml's n_runs
    assert len(results) == cfg.get("n_runs", 1) and tables is None and "masks" not in outs[0]
    capsys.readouterr()


def test_driver_with_runs_fuse_and_save_pred(tmp_path, capsys, monkeypatch):
    import yaml
    from rpnet_amd.utils import nrrd
    from tools import eval_driver
    data_dir, set_name, cfg = dataset(tmp_path / "data", do_deformable=False)
    y = dict(load_cfg(), **cfg)
    y.update(data_dir=data_dir, eval_set_name=set_name)
    path = str(tmp_path / "runs.yml")
    with open(path, "w") as fh:
        yaml.safe_dump(json.loads(json.dumps(y)), fh)
    pred = str(tmp_path / "pred")
    monkeypatch.setattr(sys, "argv", ["eval_driver.py", "--yaml", path, "--device-items", "--items", "2", "--runs", "2", "--fuse", "staple",
                                      "--save-pred", pred])
    random.seed(8)
    capsys.readouterr()
    eval_driver.main()
    text = capsys.readouterr().out
    assert "1 / 2" in text and "2 / 2" in text and "=======Average performance=========" in text and text.count(" fused ") == 3
    files = sorted(os.listdir(pred))
    assert len(files) == 2 and all(f.endswith("_Liver.nrrd") for f in files)
    vol, header = nrrd.read(os.path.join(pred, files[0]))
    assert vol.dtype == np.uint8 and header["encoding"] == "gzip" and set(np.unique(vol)) <= {0, 1}
    for argv in (["--runs", "2"], ["--device-items", "--fuse", "vote"]):
        monkeypatch.setattr(sys, "argv", ["eval_driver.py", "--yaml", path] + argv)
        with pytest.raises(SystemExit):
            eval_driver.main()
