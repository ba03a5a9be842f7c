"""Host side of the device evaluation path (rpnet_amd/dataset_eval.py, the counts_out argument of rpnet_amd.volume.VolumeSegmenter):
the slice pairing against the host reader's own loop, the loud failures off the GPU and on unsupported configurations, the shape
checks of the tally table, and the host expression the gather kernel restates."""
import ctypes

import numpy as np
import pytest
import torch

from rpnet_amd import dataset_eval as DE
from rpnet_amd import hip
from rpnet_amd.utils import volume_reader as VR

DEPTHS = range(1, 41)
KS = [1, 3, 12, 50]


class _IndexVolumes:
    """stands in for FewshotVolumeReader: volumes whose every pixel holds its own slice number"""

    def __init__(self, n_support, n_query):
        self.depths = (n_support, n_query)

    def __len__(self):
        return 1

    def __getitem__(self, idx):
        def vol(n):
            return torch.arange(n, dtype=torch.float32).view(1, n, 1, 1).expand(1, n, 2, 2).clone()
        s, q = vol(self.depths[0]), vol(self.depths[1])
        return {"support_images": [[s]], "support_labels": [[s.clone()]], "query_images": [[q]], "query_labels": [[q.clone()]],
                "class_id": 0, "pid": "q", "supp_pids": [(0, 1)]}


def _slice_reader(k):
    """a FewshotSliceReader in eval mode without files behind it (and without the registration: nothing here touches a GPU)"""
    rd = object.__new__(VR.FewshotSliceReader)
    rd.cfg, rd.k, rd.mode = {"n_shot": 1, "use_registration_loss": False}, k, "eval"
    return rd


def _host_pairing(rd, n_support, n_query):
    """(support slice per paired query slice, the query slices) as the reader's own eval branch produces them"""
    rd.fewshot_volume_reader = _IndexVolumes(n_support, n_query)
    item = rd[0]
    sup_i, sup_l = item["support_images"][0][0], item["support_labels"][0][0]
    assert torch.equal(sup_i[:, 0, 0, 0], sup_l[:, 0, 0])
    return sup_i[:, 0, 0, 0].numpy().astype(np.int32), item["query_images"][:, 0, 0, 0].numpy().astype(np.int32)


@pytest.mark.parametrize("k", KS)
def test_slice_table_is_the_host_readers_pairing(k):
    """support / query depths 1 .. 40 each, k smaller and larger than either: the table equals, entry for entry, the support
    slices FewshotSliceReader's eval loop stacks, and k_effective is the k the reader keeps.  Where the loop pairs fewer slices
    than the query has (np.arange gives k + 1 block edges) the table is as short as the loop's stack."""
    ragged = 0
    for ns in DEPTHS:
        for nq in DEPTHS:
            rd = _slice_reader(k)
            want, query = _host_pairing(rd, ns, nq)
            k_eff, table = DE.eval_slice_table(ns, nq, k)
            assert k_eff == rd.k == min(k, ns, nq), (ns, nq, k)
            assert table.dtype == np.int32 and np.array_equal(table, want), (ns, nq, k, table, want)
            assert np.array_equal(query, np.arange(nq))
            assert table.min() >= 0 and table.max() < ns
            ragged += len(table) != nq
    print(f"k = {k}: {ragged} of {len(DEPTHS) ** 2} depth pairs where the reader's loop pairs fewer slices than the query has")
    assert ragged < 0.02 * len(DEPTHS) ** 2


def test_k_sticks_across_items():
    """the reader keeps min(k, depths) for later items; feeding k_effective back in follows it"""
    rd, k = _slice_reader(12), 12
    for ns, nq in [(30, 40), (22, 9), (40, 40), (5, 33), (17, 17), (3, 2), (40, 31)]:
        want, _ = _host_pairing(rd, ns, nq)
        k, table = DE.eval_slice_table(ns, nq, k)
        assert k == rd.k and np.array_equal(table, want), (ns, nq, k)
    assert k == 2


def test_unit_map_is_one_add_and_one_multiply():
    """(x + 1) / 2 in fp32, as the host forms the registration's inputs (numpy and torch), is bit for bit a single fp32 add followed
    by a single fp32 multiply by 0.5 — the two operations csrc/evalitem.hip issues (unit_map)"""
    rs = np.random.RandomState(0)
    x = np.concatenate([rs.uniform(-1, 1, 1 << 16), rs.standard_normal(1 << 12) * 1e-30, [-1.0, 1.0, 0.0, -0.0, 1e-45, -1e-45, 3e38, -1 + 2 ** -24]])
    x = x.astype(np.float32)
    want = (x + 1) / 2
    assert want.dtype == np.float32
    two_ops = (x + np.float32(1)) * np.float32(0.5)
    assert np.array_equal(want.view(np.uint32), two_ops.view(np.uint32))
    assert np.array_equal(((torch.from_numpy(x) + 1) / 2.0).numpy().view(np.uint32), want.view(np.uint32))


CFG = dict(n_way=1, n_shot=1, k=4, use_registration_loss=True, class_csv_dir="nowhere", eval_classes=["Liver"])


def test_no_cpu_fallback():
    with pytest.raises(RuntimeError, match="MI355X only"):
        DE.DeviceEvalSource("nowhere", "nothing.csv", CFG, "cpu")
    z = torch.zeros(2, 8, 8)
    with pytest.raises(RuntimeError, match="MI355X only"):
        DE.eval_item_gather(z, z, z, z, np.zeros(2, np.int32))
    with pytest.raises(RuntimeError, match="MI355X only"):
        DE.ncc_pairs(z, z, z, torch.zeros(1, 2, dtype=torch.float64), 0)


@pytest.mark.parametrize("over,exc,match", [
    (dict(test_shot=2), NotImplementedError, "test_shot"),
    (dict(use_registration_mask=True), NotImplementedError, "use_registration_mask"),
    (dict(n_shot=2), NotImplementedError, "one way, one shot"),
    (dict(n_way=2), NotImplementedError, "one way, one shot"),
    (dict(use_registration_loss=False), TypeError, "use_registration_loss"),
])
def test_unsupported_configurations_raise(over, exc, match):
    """refused before any file or the device is touched"""
    with pytest.raises(exc, match=match):
        DE.DeviceEvalSource("nowhere", "nothing.csv", dict(CFG, **over), "cuda:0")


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.num_iter = 3

    def forward(self, *a, **kw):
        raise AssertionError("the model must not be called when counts_out is refused")


def test_counts_out_shape_checks():
    from rpnet_amd.volume import VolumeSegmenter, check_counts_out
    check_counts_out(torch.zeros(5, 1, 3, dtype=torch.int64), K=2, T=3)
    check_counts_out(torch.zeros(12, 1, 3, dtype=torch.int64), K=2)
    for bad in (torch.zeros(5, 1, 3, dtype=torch.int32), torch.zeros(4, 1, 3, dtype=torch.int64), torch.zeros(5, 2, 3, dtype=torch.int64),
                torch.zeros(5, 3, dtype=torch.int64), torch.zeros(5, 1, 6, dtype=torch.int64)[:, :, ::2], np.zeros((5, 1, 3), np.int64)):
        with pytest.raises(ValueError, match="counts_out"):
            check_counts_out(bad, K=2, T=3)
    seg = VolumeSegmenter(_Net(), batch=2, graphed=False)
    si, fg, qi, appr, ql = [[torch.zeros(2, 1, 16, 16)]], [[torch.zeros(2, 16, 16)]], torch.zeros(2, 1, 16, 16), torch.zeros(2, 16, 16), torch.zeros(2, 16, 16)
    with pytest.raises(ValueError, match=r"\[5, 1, 3\]"):
        seg(si, fg, qi, appr, ql, counts_out=torch.zeros(12, 1, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="needs query_labels"):
        seg(si, fg, qi, appr, None, counts_out=torch.zeros(5, 1, 3, dtype=torch.int64))


def test_library_exports_the_evaluation_entry_points():
    lib = ctypes.CDLL(hip.lib_path())
    for name in ("rpnet_eval_item_gather", "rpnet_ncc_pairs_workspace_bytes", "rpnet_ncc_pairs"):
        assert name in hip.EVAL_ABI_SYMBOLS and name not in hip.ABI_SYMBOLS and hasattr(lib, name), name
    # the workspace holds two partial tables of at most 1024 rows of 8 doubles, whatever the element count
    q = hip.load().rpnet_ncc_pairs_workspace_bytes
    assert q(1) == 2 * 8 * 8 and q(64 * 256 * 256) == q(1 << 28) == 2 * 1024 * 8 * 8
