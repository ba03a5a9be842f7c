"""CPU tests of rpnet_amd.volume: the new entry point is declared, exported and bound; the counts -> Dice helper gives the
numbers of the driver's `dice_score_seperate`; host tensors are refused (no fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_seg_tally_is_declared_exported_and_bound():
    from rpnet_amd import hip
    hdr = open(os.path.join(ROOT, "include", "rpnet_abi.h")).read()
    assert re.search(r"\bint rpnet_seg_tally\s*\(", hdr)
    assert os.path.exists(hip.lib_path()), "build librpnet_hip.so first (__graft_entry__.build())"
    assert hasattr(ctypes.CDLL(hip.lib_path()), "rpnet_seg_tally")
    assert "rpnet_seg_tally" in hip.ABI_SYMBOLS
    assert hip.ABI_VERSION >= 110
    assert hip.load().rpnet_version() == hip.ABI_VERSION


def test_package_exports_the_volume_segmenter():
    import rpnet_amd
    from rpnet_amd.volume import VolumeResult, VolumeSegmenter, dice_from_counts, seg_tally  # noqa: F401
    assert rpnet_amd.VolumeSegmenter is VolumeSegmenter
    assert VolumeResult._fields == ("mask", "counts", "dice")


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_dice_from_counts_equals_dice_score_seperate(seed):
    """seeded random binary volumes of three classes, the last one absent from the ground truth (-> None); predictions as the
    driver hands them over (fp32 and int32 arrays against int64 labels)"""
    from rpnet_amd.volume import dice_from_counts
    from utils.util import dice_score_seperate
    rs = np.random.RandomState(seed)
    shape = (3, 7, 48, 80)
    true = (rs.rand(*shape) < np.array([0.3, 0.02, 0.0]).reshape(3, 1, 1, 1)).astype(np.int64)
    for dtype in (np.float32, np.int32):
        pred = (rs.rand(*shape) < np.array([0.35, 0.5, 0.1]).reshape(3, 1, 1, 1)).astype(dtype)
        want = dice_score_seperate(pred, true, num_class=3)
        assert want[2] is None and want[0] is not None and want[1] is not None
        counts = np.array([[int((pred[c] * true[c]).sum()), int(pred[c].sum()), int(true[c].sum())] for c in range(3)], dtype=np.int64)
        assert dice_from_counts(counts) == want
    assert dice_from_counts(np.array([[0, 0, 5]])) == [0.0]                 # empty prediction of a present class
    assert dice_from_counts(np.array([[0, 9, 0]])) == [None]


def test_seg_tally_refuses_host_tensors():
    from rpnet_amd.volume import seg_tally
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        seg_tally([torch.zeros(1, 2, 16, 16)], [0], torch.ones(1, dtype=torch.int32), mask=torch.zeros(1, 16, 16, dtype=torch.uint8))
