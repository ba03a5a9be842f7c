"""Per-component statistics on the device (csrc/compstat.hip through include/rpnet_compstat_abi.h and rpnet_amd/component_stats.py)
against the numpy restatement of tests/compstat_cases.py: the renumbered volume, every int64 row and every head word EQUAL.  Every call
is made twice into outputs prefilled with sentinels, with guard words behind the volume, the rows and the workspace, and gives the same
bits."""
import json
import random
import sys

import numpy as np
import pytest
import torch

from rpnet_amd import component_stats as CS
from rpnet_amd import hip
from tests import compstat_cases as CC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TORCH = {"u8": torch.uint8, "i32": torch.int32, "i64": torch.int64, "f32": torch.float32, "i16": torch.int16}
FILL, GUARD = -7, 0x5A


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


def run_chain(labels, image=None, q=0, other=None, other_cls=1, max_components=64, ikind="f32", okind="u8", loff=0, ioff=0, ooff=0, row=1, n_rows=2,
              want_invalid=0):
    """rpnet_compstat_rank and rpnet_compstat_table (through CS.rank_components and CS.tally_components) twice on sparse int32 labels
    against the restatement: dense, the statistics row, the rows and the head equal; the other rows of the tables and the words behind
    the volume, the tables and the workspace untouched -> (dense, rows, head) of the restatement"""
    labels = np.asarray(labels, np.int32)
    shape = labels.shape
    n = labels.size
    want_dense, C, invalid = CC.rank_restate(labels)
    want_rows, beyond, bad = CC.table_restate(want_dense, C, image, q, other, other_cls, max_components)
    assert invalid == want_invalid and bad == 0
    d_labels = dev(labels, torch.int32, loff)
    d_image = None if image is None else dev(image, TORCH[ikind], ioff)
    d_other = None if other is None else dev(other, TORCH[okind], ooff)
    need = hip.query("rpnet_compstat_workspace_bytes", *shape, max_components)
    assert need == CS._compstat_workspace_layout(*shape)[1]
    entries = n_rows * max_components * CS.COMP_ROW
    runs = []
    for fill in (0, 0xFF):              # whatever the workspace holds before the calls
        ws = torch.full((need + 64,), GUARD, dtype=torch.uint8, device=DEV)
        ws[:need] = fill
        vol = torch.full((n + 16,), FILL, dtype=torch.int32, device=DEV)
        stats = torch.full((n_rows * CS.COMP_STATS_ROW + 4,), FILL, dtype=torch.int64, device=DEV)
        table = torch.full((entries + 8,), FILL, dtype=torch.int64, device=DEV)
        dense = vol[:n].view(shape)
        st = stats[:n_rows * CS.COMP_STATS_ROW].view(n_rows, CS.COMP_STATS_ROW)
        rows = table[:entries].view(n_rows, max_components, CS.COMP_ROW)
        got = CS.rank_components(d_labels, out=dense, stats=st, row=row, workspace=ws[:need])
        assert got[0] is dense and got[1] is st
        assert CS.tally_components(dense, d_image, d_other, other_cls, max_components, q, out=rows, row=row, workspace=ws[:need]) is rows
        assert (ws[need:] == GUARD).all() and (vol[n:] == FILL).all() and (stats[n_rows * CS.COMP_STATS_ROW:] == FILL).all()
        assert (table[entries:] == FILL).all()
        for r in range(n_rows):
            if r != row:
                assert (rows[r] == FILL).all() and (st[r] == FILL).all()
        runs.append((dense.cpu().numpy(), rows[row].cpu().numpy(), CS.component_head(ws).cpu().numpy(), st[row].cpu().numpy()))
    (a_d, a_r, a_h, a_s), (b_d, b_r, b_h, b_s) = runs
    assert a_d.tobytes() == b_d.tobytes() and a_r.tobytes() == b_r.tobytes() and a_h.tobytes() == b_h.tobytes() and a_s.tobytes() == b_s.tobytes()
    assert np.array_equal(a_d, want_dense), np.argwhere(a_d != want_dense)[:8]
    assert np.array_equal(a_r, want_rows), (np.argwhere(a_r != want_rows)[:8], a_r[a_r != want_rows][:8], want_rows[a_r != want_rows][:8])
    assert list(a_h) == [C, invalid, beyond, 0] and list(a_s) == [C, invalid, 0, 0]
    return want_dense, want_rows, a_h


def sparse(mask, connectivity=6):
    return CC.sparse_labels(np.asarray(mask, bool), connectivity)


@pytest.mark.parametrize("shape", CC.SHAPES)
def test_shapes(shape):
    """one voxel; each axis of length 1; one tile + 1 (two chunks); 2 * tile + 2; a line of 1024 along each axis: a smooth organ with
    islands, noise under both connectivities, with an image and the overlap volume"""
    image = CC.image_for(shape, sum(shape))
    other = CC.noise_mask(shape, 0.5, 1).astype(np.uint8)
    run_chain(sparse(CC.blob_mask(shape, sum(shape) + 1)), image, 16, other, max_components=256)
    for connectivity in (6, 26):
        run_chain(sparse(CC.noise_mask(shape, 0.31, 2), connectivity), image, 4, other, max_components=512)
    if 1024 in shape:
        axis = shape.index(1024)
        _, rows, _ = run_chain(sparse(np.ones(shape, bool)), None, max_components=1)
        assert rows[0, 4 + axis] == 1023 and rows[0, 10 + axis] == sum(v * v for v in range(1024)) and rows[0, 23] == 0


def test_empty_full_and_the_scan_past_its_block():
    """no component at all; one id in every chunk; 257 chunks, one more than the scan block has threads, with a root in every chunk, in
    the last voxel, and many in the chunks on either side of the seam between the scan's tiles"""
    shape = (2, 33, 65)
    _, rows, head = run_chain(np.zeros(shape, np.int32), CC.image_for(shape, 1), 16, np.ones(shape, np.uint8), max_components=3)
    assert head[0] == 0 and (rows == CC.empty_row(shape)).all()
    _, rows, head = run_chain(sparse(np.ones(shape, bool)), CC.image_for(shape, 1), 16, np.ones(shape, np.uint8), max_components=3)
    assert head[0] == 1 and rows[0, 0] == rows[0, 22] == 2 * 33 * 65
    shape = CC.SCAN_SHAPE
    assert shape[0] * shape[1] * shape[2] == 257 * CC.CHUNK
    mask = np.zeros(shape, bool)
    mask[0::2, 0, 0] = True                                 # one voxel in every chunk (a slice is a chunk), no two of them neighbours
    mask[1::2, 2, 2] = True
    mask[-1, -1, -1] = True
    mask[255, 10, 1::2] = True                              # 32 more roots in the last chunk of the scan's first tile
    mask[256, 12, 1::2] = True                              # and in the one chunk of its second tile
    _, rows, head = run_chain(sparse(mask), None, max_components=512, n_rows=1, row=0)
    assert head[0] == int(mask.sum()) == 257 + 1 + 64 and head[2] == 0 and (rows[:322, 0] == 1).all()
    assert list(rows[[0, 256 + 32, 321], 23]) == [0, 256 * 4096, 257 * 4096 - 1]
    big = sparse(np.ones(shape, bool))
    _, rows, head = run_chain(big, None, other=np.ones(shape, np.uint8), max_components=2, n_rows=1, row=0)
    assert head[0] == 1 and rows[0, 0] == 257 * CC.CHUNK and rows[0, 10] == sum(z * z for z in range(257)) * 4096


@pytest.mark.parametrize("max_components", [5000, 7])
def test_checkerboard_more_ids_than_slots(max_components):
    """2048 ids in every whole chunk against 128 slots: most runs go to their rows directly; with max_components = 7 nearly every voxel
    is beyond the table"""
    shape = (2, 33, 65)
    board = CC.checkerboard(shape)
    _, rows, head = run_chain(sparse(board), CC.image_for(shape, 3, "i16"), 0, board.astype(np.uint8), max_components=max_components, ikind="i16")
    assert head[0] == int(board.sum()) == 2145 and head[2] == max(0, 2145 - max_components)
    assert (rows[:min(2145, max_components), 0] == 1).all()
    dense, _, head = run_chain(sparse(board, 26), None, max_components=max_components)
    assert head[0] == 1 and head[2] == 0


def test_component_count_at_and_one_above_the_table():
    shape = (1, 9, 13)
    mask = np.zeros(shape, bool)
    mask[0, ::2, ::2] = True                                # 35 components of one voxel
    C = int(mask.sum())
    other = np.zeros(shape, np.uint8)
    other[0, 4] = 3
    for M, beyond in ((C, 0), (C - 1, 1), (C + 1, 0)):
        _, rows, head = run_chain(sparse(mask), CC.image_for(shape, 2), 16, other, other_cls=3, max_components=M)
        assert list(head) == [C, 0, beyond, 0] and rows[:, 0].sum() == C - beyond and rows[:, 22].sum() == min(int((mask & (other == 3)).sum()), M)


@pytest.mark.parametrize("kind", ["u8", "i32", "i64", "f32"])
def test_every_label_kind_both_connectivities_and_offset_pointers(kind):
    """component_table on every kind rpnet_cc_label takes, under both connectivities, equal to the chain of the restatement; `other` of
    every kind; volumes 4 and 16 bytes into an allocation (int32 at an address that is no multiple of 16, an int16 image on a 2-byte
    boundary, a uint8 volume at an odd address)"""
    shape = (3, 37, 41)
    vol = (CC.noise_mask(shape, 0.35, 5) * 2).astype(np.int64)         # class 2 is the foreground; class 1 a few voxels beside it
    vol[CC.noise_mask(shape, 0.05, 6)] = 1
    image = CC.image_for(shape, 7)
    other = CC.noise_mask(shape, 0.5, 8).astype(np.int64) * 2
    d_vol, d_image = dev(vol, TORCH[kind]), dev(image, torch.float32)
    cast = vol.astype({"u8": np.uint8, "i32": np.int32, "i64": np.int64, "f32": np.float32}[kind])
    for connectivity in (6, 26):
        want_dense, want_rows, want_head = CC.chain_restate(cast, 2, connectivity, image, 16, other, 2, 700)
        for _ in range(2):
            got = CS.component_table(d_vol, cls=2, connectivity=connectivity, image=d_image, other=dev(other, TORCH[kind]), max_components=700)
            assert got.scale_log2 == 16 and got.rows.shape == (700, CS.COMP_ROW)
            assert np.array_equal(got.dense.cpu().numpy(), want_dense) and np.array_equal(got.rows.cpu().numpy(), want_rows)
            assert np.array_equal(got.head.cpu().numpy(), want_head) and want_head[0] > (20 if connectivity == 6 else 1)
    labels = sparse(vol == 2)
    small = CC.image_for(shape, 9, "i16")
    for loff, ioff, ooff in ((1, 0, 0), (0, 1, 1), (4, 8, 16), (1, 1, 1)):
        run_chain(labels, small, 0, other, 2, 700, ikind="i16", okind=kind, loff=loff, ioff=ioff, ooff=ooff)
        run_chain(labels, image, 16, other, 2, 700, ikind="f32", okind=kind, loff=loff, ioff=ioff, ooff=ooff)


@pytest.mark.parametrize("q", [0, 16, 30])
def test_image_values(q):
    """both ends of the int16 range; NaN, +-inf and -0.0; ties at k + 0.5 of both parities and both signs; values at and one ulp below
    the representability edge 2^31 / 2^q, of both signs; other given with a class it does not hold, and null"""
    shape = (3, 9, 13)
    mask = CC.blob_mask(shape, 2)
    labels = sparse(mask)
    n_fg = int(mask.sum())
    edge = np.float32(2.0 ** (31 - q))
    below = np.nextafter(edge, np.float32(0))
    unit = 2.0 ** -q
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 2.5 * unit, 3.5 * unit, -2.5 * unit, -3.5 * unit, 0.5 * unit, edge, below, -edge, -below,
                        1.0, -1.0], np.float32)
    assert (special[5:10].astype(np.float64) / unit * 2 % 2 == 1).all()           # the ties are ties in float32
    image = np.zeros(shape, np.float32)
    image[mask] = np.resize(special, n_fg)
    other = np.zeros(shape, np.uint8)
    _, rows, _ = run_chain(labels, image, q, other, other_cls=1, max_components=40)
    assert rows[:, 22].sum() == 0 and 0 < rows[:, 16].sum() < n_fg
    k, ok = CC.quantise(special, q)
    assert list(ok) == [False] * 3 + [True] * 7 + [False, True, False, True, True, True] and list(k[5:10]) == [2, 4, -2, -4, 0]
    run_chain(labels, image, q, None, max_components=40)
    ends = CC.image_for(shape, 1, "i16")
    ends.ravel()[::5] = -32768
    ends.ravel()[1::7] = 32767
    _, rows, _ = run_chain(labels, ends, q, other, max_components=40, ikind="i16")
    assert (rows[:, 16].sum() == n_fg) if q == 0 else (rows[:, 16].sum() < n_fg)      # -32768 * 2^16 is -2^31: not representable; at q = 30 only -1, 0 and 1 are
    whole = np.ones(shape, bool)
    allnan = np.full(shape, np.nan, np.float32)
    _, rows, _ = run_chain(sparse(whole), allnan, q, max_components=2)
    assert rows[0, 0] == 351 and rows[0, 16] == 0 and rows[0, 17] == 0xFFFFFFFF and rows[0, 18] == 0 and (rows[0, 19:22] == 0).all()


def test_invalid_labels_set_the_word_and_write_nothing_out_of_bounds():
    """a hand-made labels volume with values beyond the volume, negative ones, INT_MAX and labels that name a voxel that is no root: they
    give 0, are counted, and the guards behind every output stay intact (run_chain asserts them); a dense volume with ids outside
    0..C sets the table's invalid word"""
    shape = (2, 33, 65)
    mask = CC.noise_mask(shape, 0.31, 3)
    labels = sparse(mask).ravel()
    n = labels.size
    fg = np.flatnonzero(labels)
    bad = labels.copy()
    bad[fg[::7]] = np.resize(np.array([n + 1, -5, 2 ** 31 - 1, -2 ** 31, n + 4096, 2], np.int32), len(fg[::7]))
    _, _, invalid = CC.rank_restate(bad.reshape(shape))
    assert invalid >= len(fg[::7]) - 1
    run_chain(bad.reshape(shape), CC.image_for(shape, 1), 16, mask.astype(np.uint8), max_components=2000, want_invalid=invalid)
    good, C, _ = CC.rank_restate(labels.reshape(shape))
    odd = good.copy().ravel()
    odd[fg[:6]] = (C + 1, -1, 2 ** 31 - 1, -2 ** 31, C + 70000, 65537 + C)
    want_rows, beyond, n_bad = CC.table_restate(odd.reshape(shape), C, max_components=C)
    assert n_bad == 6 and beyond == 0
    d_odd = dev(odd.reshape(shape), torch.int32)
    need = CS._compstat_workspace_layout(*shape)[1]
    ws = torch.full((need + 64,), GUARD, dtype=torch.uint8, device=DEV)
    CS.component_head(ws)[:] = torch.tensor([C, 0, FILL, FILL], device=DEV)
    table = torch.full((C * CS.COMP_ROW + 8,), FILL, dtype=torch.int64, device=DEV)
    rows = table[:C * CS.COMP_ROW].view(1, C, CS.COMP_ROW)
    CS.tally_components(d_odd, max_components=C, out=rows, workspace=ws[:need])
    assert np.array_equal(rows[0].cpu().numpy(), want_rows) and list(CS.component_head(ws).cpu().numpy()) == [C, 0, 0, 6]
    assert (table[C * CS.COMP_ROW:] == FILL).all() and (ws[need:] == GUARD).all() and (ws[32:need] == GUARD).all()


def test_captured_graph_of_component_table_replayed_twice():
    shape = (3, 37, 41)
    vol, image = CC.blob_mask(shape, 11).astype(np.uint8), CC.image_for(shape, 12)
    other = CC.noise_mask(shape, 0.5, 13).astype(np.uint8)
    want_dense, want_rows, want_head = CC.chain_restate(vol, 1, 26, image, 16, other, 1, 300)
    d_vol, d_image, d_other = dev(vol, torch.uint8), dev(image, torch.float32), dev(other, torch.uint8)
    rows = torch.zeros((1, 300, CS.COMP_ROW), dtype=torch.int64, device=DEV)
    head = torch.zeros((CS.HEAD_WORDS,), dtype=torch.int64, device=DEV)
    labels, dense = (torch.zeros(shape, dtype=torch.int32, device=DEV) for _ in range(2))
    kw = dict(cls=1, connectivity=26, image=d_image, other=d_other, max_components=300, out=rows, head_out=head, labels=labels, dense=dense)
    CS.component_table(d_vol, **kw)                         # the workspaces are allocated before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            CS.component_table(d_vol, **kw)
    for replay in range(2):
        rows.fill_(FILL)
        head.fill_(FILL)
        dense.fill_(FILL)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(rows[0].cpu().numpy(), want_rows) and np.array_equal(head.cpu().numpy(), want_head), replay
        assert np.array_equal(dense.cpu().numpy(), want_dense)


def raw_rank(labels, dense, ws, stats=None, dims=(3, 9, 13), row=0, n_rows=1, ws_bytes=None):
    """rpnet_compstat_rank itself -> (status, error string)"""
    lib = hip.load()
    p = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())  # noqa: E731
    rc = lib.rpnet_compstat_rank(p(labels), *dims, p(dense), p(stats), row, n_rows, p(ws),
                                 (ws.numel() if torch.is_tensor(ws) else 0) if ws_bytes is None else ws_bytes, hip.stream())
    return rc, lib.rpnet_last_error_string().decode()


def raw_table(dense, rows, ws, image=None, image_kind=0, q=0, other=None, other_kind=0, dims=(3, 9, 13), M=4, row=0, n_rows=1, ws_bytes=None):
    """rpnet_compstat_table itself -> (status, error string)"""
    lib = hip.load()
    p = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())  # noqa: E731
    rc = lib.rpnet_compstat_table(p(dense), p(image), image_kind, q, p(other), other_kind, 1, *dims, M, p(rows), row, n_rows, p(ws),
                                  (ws.numel() if torch.is_tensor(ws) else 0) if ws_bytes is None else ws_bytes, hip.stream())
    return rc, lib.rpnet_last_error_string().decode()


def test_refusals_launch_nothing():
    shape = (3, 9, 13)
    labels = dev(sparse(CC.blob_mask(shape, 1)), torch.int32)
    image = dev(CC.image_for(shape, 2), torch.float32)
    need = hip.query("rpnet_compstat_workspace_bytes", *shape, 4)
    ws = torch.full((need + 16,), GUARD, dtype=torch.uint8, device=DEV)
    dense = torch.full(shape, FILL, dtype=torch.int32, device=DEV)
    stats = torch.full((1, CS.COMP_STATS_ROW), FILL, dtype=torch.int64, device=DEV)
    rows = torch.full((1, 4, CS.COMP_ROW), FILL, dtype=torch.int64, device=DEV)
    base = dict(labels=labels, dense=dense, ws=ws, stats=stats)
    assert raw_rank(**dict(base, ws_bytes=need))[0] == 0
    tbase = dict(dense=dense, rows=rows, ws=ws, image=image, other=labels, other_kind=1)
    rc, err = raw_table(**dict(tbase, ws_bytes=need))
    assert rc == 0, err
    dense.fill_(FILL)
    stats.fill_(FILL)
    rows.fill_(FILL)
    ws.fill_(GUARD)
    torch.cuda.synchronize()
    for over in (dict(labels=None), dict(dense=None), dict(ws=None), dict(dense=labels), dict(dims=(0, 9, 13)), dict(dims=(3, 1025, 13)),
                 dict(dims=(3, 9, -1)), dict(row=1), dict(row=-1), dict(n_rows=0), dict(ws_bytes=need - 1), dict(ws=ws.data_ptr() + 8, ws_bytes=need),
                 dict(labels=labels.data_ptr() + 2), dict(dense=dense.data_ptr() + 1), dict(stats=stats.data_ptr() + 4)):
        rc, err = raw_rank(**dict(base, **over))
        assert rc != 0 and err.startswith("compstat_rank:"), (over, rc, err)
    assert raw_rank(**dict(base, dense=labels))[1] == "compstat_rank: dense may not alias labels"
    for over in (dict(dense=None), dict(rows=None), dict(ws=None), dict(image_kind=2), dict(image_kind=-1), dict(q=-1), dict(q=31), dict(other_kind=4),
                 dict(other_kind=-1), dict(M=0), dict(M=65537), dict(dims=(0, 9, 13)), dict(dims=(3, 9, 1025)), dict(row=1), dict(row=-1), dict(n_rows=0),
                 dict(ws_bytes=need - 1), dict(ws=ws.data_ptr() + 8, ws_bytes=need), dict(dense=dense.data_ptr() + 2), dict(image=image.data_ptr() + 2),
                 dict(image=image.data_ptr() + 1, image_kind=1), dict(other=labels.data_ptr() + 2), dict(other=labels.data_ptr() + 4, other_kind=2),
                 dict(rows=rows.data_ptr() + 4)):
        rc, err = raw_table(**dict(tbase, **over))
        assert rc != 0 and err.startswith("compstat_table:"), (over, rc, err)
    assert raw_table(**dict(tbase, q=31))[1] == "compstat_table: scale_log2=31 (0..30)"
    for bad in ((0, 9, 13, 4), (3, 9, 13, 0), (3, 9, 13, 65537), (3, 9, 1025, 4)):
        assert hip.query("rpnet_compstat_workspace_bytes", *bad) == 0
        assert hip.load().rpnet_last_error_string().decode() == (
            "compstat_workspace_bytes: D=%d H=%d W=%d max_components=%d (every extent 1..1024, max_components 1..65536)" % bad)
    torch.cuda.synchronize()
    assert (dense == FILL).all() and (stats == FILL).all() and (rows == FILL).all() and (ws == GUARD).all()
    # a null stats table, a null image with any kind and scale, a null other with any kind are accepted
    assert raw_rank(labels, dense, ws)[0] == 0
    assert raw_table(dense, rows, ws, image_kind=9, q=99, other_kind=9)[0] == 0
    # the Python layer on device tensors
    for call in (lambda: CS.rank_components(labels, out=labels), lambda: CS.rank_components(labels, stats=stats, row=1),
                 lambda: CS.rank_components(labels, workspace=ws[:need - 16]), lambda: CS.rank_components(labels, workspace=ws[8:8 + need]),
                 lambda: CS.tally_components(dense, image=image[:2]), lambda: CS.tally_components(dense, out=rows, max_components=5),
                 lambda: CS.tally_components(dense, out=rows, max_components=4, row=1), lambda: CS.tally_components(dense, image, scale_log2=31),
                 lambda: CS.component_table(labels, head_out=stats)):
        with pytest.raises(ValueError):
            call()


# ----------------------------------------------------------------------------------------------------------------- end to end
MM = (2.5, 0.8, 0.8)


def mm_dataset(tmp_path):
    from rpnet_amd.utils import volume_reader as VR
    from tests.test_gpu_dataset_eval import CASE, _eval_cfg, config_for
    data_dir, set_name, csv_dir = VR.write_synthetic_dataset(str(tmp_path), spacing=MM, **CASE["data"])
    return data_dir, set_name, _eval_cfg(dict(config_for(CASE, csv_dir), use_registration_mask=False, do_deformable=False))


def want_tables(final, labels, image, M):
    """the two tables and heads VolumeSegmenter(components=M) forms of a final mask and the labels"""
    p = CC.chain_restate(final, 1, 6, image, 16, labels, 1, M)
    t = CC.chain_restate(labels, 1, 6, image, 16, final, 1, M)
    return np.stack([p[1], t[1]])[:, None], np.stack([p[2], t[2]])[:, None]


def test_volume_segmenter_components_eager_and_graphed(tmp_path):
    """VolumeSegmenter(components=True) on an item of the synthetic data set, 8 slices of 64 x 64: its tables equal the restatement applied
    to the mask it returns (the end of the clean-up chain where one is on) and to the labels, eagerly and through the captured graph,
    into the caller's tables without a host synchronisation; mask, counts and dice are those of components=False"""
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
    image = item["query_images"][:, 0].contiguous().cpu().numpy()
    labels = item["query_labels"].cpu().numpy().astype(np.int32)
    assert image.shape[1:] == (64, 64)
    for graphed in (False, True):
        plain = VolumeSegmenter(net, batch=8, graphed=graphed)(*args)
        assert plain.components is None
        for chain, M in (({}, True), (dict(keep_largest=6, fill_holes=True), 5)):
            res = VolumeSegmenter(net, batch=8, graphed=graphed, components=M, **chain)(*args, spacing=MM)
            assert torch.equal(res.mask, plain.mask) and np.array_equal(res.counts, plain.counts) and res.dice == plain.dice
            final = (res.post["mask"] if chain else res.mask).cpu().numpy()
            want_rows, want_head = want_tables(final, labels, image, 4096 if M is True else M)
            assert np.array_equal(res.components["rows"], want_rows) and np.array_equal(res.components["head"], want_head), graphed
            fig = res.components["figures"][0]
            assert fig == dict(CS.detection_counts(want_rows[0, 0], want_rows[1, 0]), components_pred=int(want_head[0, 0, 0]),
                               components_truth=int(want_head[1, 0, 0]), fp_volume_ml=fig["fp_voxels"] * 1.6 / 1000.0)
            assert res.components["scale_log2"] == 16 and want_head[1, 0, 0] >= 1
        seg = VolumeSegmenter(net, batch=8, graphed=graphed, components=9)
        rows = torch.full((2, 1, 9, CS.COMP_ROW), FILL, dtype=torch.int64, device=DEV)
        heads = torch.full((2, 1, CS.HEAD_WORDS), FILL, dtype=torch.int64, device=DEV)
        counts = torch.zeros((net.num_iter + 2, 1, 3), dtype=torch.int64, device=DEV)
        seg(*args, counts_out=counts, components_out=(rows, heads))            # shapes seen, workspaces made
        rows.fill_(FILL)
        out = seg(*args, counts_out=counts, components_out=(rows, heads))
        assert out.components is None and torch.equal(out.mask, plain.mask)
        want_rows, want_head = want_tables(plain.mask.cpu().numpy(), labels, image, 9)
        assert np.array_equal(rows.cpu().numpy(), want_rows) and np.array_equal(heads.cpu().numpy(), want_head)
        # what the option adds makes no host synchronisation: every synchronising torch call raises under the debug mode
        d_labels, d_image = dev(labels, torch.int32), dev(image, torch.float32)
        rows2, heads2 = torch.zeros_like(rows), torch.zeros_like(heads)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            assert seg._components(plain.mask, d_labels, d_image, 2, (rows2, heads2)) is None
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.equal(rows2, rows) and torch.equal(heads2, heads)
        with pytest.raises(ValueError, match="components_out needs"):
            VolumeSegmenter(net, batch=8, graphed=graphed)(*args, components_out=(rows, heads))
        with pytest.raises(ValueError, match="components_out must be"):
            seg(*args, components_out=(rows[:1], heads))
    # without labels: the prediction's tables alone, with no overlap
    res = VolumeSegmenter(net, batch=8, graphed=False, components=6)(*args[:4])
    assert res.components["figures"] is None and (res.components["rows"][1] == 0).all() and (res.components["head"][1] == 0).all()
    dense, want, head = CC.chain_restate(res.mask.cpu().numpy(), image=image, q=16, max_components=6)
    assert np.array_equal(res.components["rows"][0, 0], want) and np.array_equal(res.components["head"][0, 0], head)


def test_evaluate_dataset_components_and_the_driver(tmp_path, capsys, monkeypatch):
    """evaluate_dataset(components=...): out["components_*"] equal the per-item restatement on the kept masks, the printed comp / det /
    fp / fpvol fields equal detection_figures of those tables, and everything else is the run without the option; components=False prints
    and returns what a run with the option absent does; tools/eval_driver.py --components end to end, byte for byte the old lines in
    front of the new fields"""
    import yaml

    from rpnet_amd import dataset_eval as DE
    from tests.helpers import load_cfg
    from tests.test_gpu_dataset_eval import _build_net, _plain
    data_dir, set_name, cfg = mm_dataset(tmp_path / "data")
    src = DE.DeviceEvalSource(data_dir, set_name, cfg, DEV)
    src.warm()
    net = _build_net(cfg, "f32")
    runs = {}
    for name, kw in (("absent", {}), ("off", dict(components=False)), ("voxels", dict(components=True, keep_masks=True)),
                     ("header", dict(components=50, spacing="header", keep_masks=True, keep_largest=6))):
        random.seed(77)
        capsys.readouterr()
        tabs = {}
        dicts = _plain(DE.evaluate_dataset(net, src, cfg, batch=8, graphed=False, out=tabs, **kw))
        runs[name] = (dicts, tabs, capsys.readouterr().out.splitlines())
    (d0, t0, l0), (d1, t1, l1) = runs["absent"], runs["off"]
    assert d1 == d0 and l1 == l0 and sorted(t1) == sorted(t0) == ["counts", "ncc"] and all(t1[k].tobytes() == t0[k].tobytes() for k in t0)
    for name, M in (("voxels", 4096), ("header", 50)):
        d, t, lines = runs[name]
        mm = name == "header"
        assert d == d0 and t["counts"].tobytes() == t0["counts"].tobytes() and t["ncc"].tobytes() == t0["ncc"].tobytes()
        assert t["components_rows"].shape == (3, 2, 1, M, CS.COMP_ROW) and t["components_head"].shape == (3, 2, 1, CS.HEAD_WORDS) and len(lines) == len(l0) == 4
        assert (t.get("spacing") == [MM] * 3) if mm else ("spacing" not in t)
        figs = []
        for j in range(3):
            c, qv = src.reader.indices[j]
            image, truth = (v.cpu().numpy() for v in src.volume(c, qv))
            want_rows, want_head = want_tables(t["masks"][j].cpu().numpy(), truth.astype(np.int32), image, M)
            assert np.array_equal(t["components_rows"][j], want_rows) and np.array_equal(t["components_head"][j], want_head), (name, j)
            fig = CS.detection_figures(want_rows, want_head, MM if mm else None)[0]
            figs.append(fig)
            tail = (f" comp {fig['components_pred']} ({fig['components_truth']}) det {fig['detected']}/{fig['components_truth']} fp {fig['fp']} fpvol "
                    + (f"{fig['fp_volume_ml']:.4f} mL" if mm else f"{fig['fp_voxels']}"))
            assert lines[j].endswith(tail), (lines[j], tail)
            assert (lines[j].startswith(l0[j]) and " lcc " in lines[j]) if mm else lines[j] == l0[j] + tail
        assert lines[3].startswith(l0[3]) and lines[3].endswith(CS.detection_mean_suffix(figs, mm)) and " comp " in lines[3]
    # the driver
    from tools import eval_driver
    y = dict(load_cfg(), **cfg)
    y.update(data_dir=data_dir, eval_set_name=set_name)
    path = str(tmp_path / "components.yml")
    with open(path, "w") as fh:
        yaml.safe_dump(json.loads(json.dumps(y)), fh)
    texts = {}
    for name, extra in (("off", []), ("on", ["--components"]), ("n", ["--components", "3"])):
        monkeypatch.setattr(sys, "argv", ["eval_driver.py", "--yaml", path, "--device-items", "--items", "2"] + extra)
        random.seed(8)
        torch.manual_seed(8)                                # the driver builds its net from the generator: the same weights in every run
        capsys.readouterr()
        eval_driver.main()
        texts[name] = capsys.readouterr().out
    assert " comp " not in texts["off"] and len(texts["off"].splitlines()) == 3
    for name in ("on", "n"):
        new = texts[name].splitlines()
        assert len(new) == 3 and all(" comp " in l and " det " in l and " fpvol " in l and " mL" not in l for l in new)
        assert all(l.startswith(old) for l, old in zip(new, texts["off"].splitlines()))
        assert [l[:l.index(" comp ")] for l in new] == texts["off"].splitlines()
    monkeypatch.setattr(sys, "argv", ["eval_driver.py", "--yaml", path, "--components"])
    with pytest.raises(SystemExit):
        eval_driver.main()
