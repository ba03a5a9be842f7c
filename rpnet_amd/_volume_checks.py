"""The host layer the volume metrics share (surface, surface_spacing, components, postprocess): the checks of a volume, a table and the
devices, the workspace cache, and the helpers of their figures and evaluation lines.  No entry point of the library is named here:
the public function that makes a call names it, and hands its workspace query to the cache."""
import math

import numpy as np
import torch

from . import hip

KINDS = {torch.uint8: 0, torch.int32: 1, torch.int64: 2, torch.float32: 3}      # RPNET_SURFACE_U8 / I32 / I64 / F32 (= RPNET_CC_*)


def check_volume(t, what, fn):
    """`t` is a contiguous [D,H,W] tensor of one of the four element kinds"""
    if t.dtype not in KINDS:
        raise ValueError(f"{fn}: {what} is {t.dtype}; uint8, int32, int64 and float32 volumes are accepted")
    if t.dim() != 3 or not t.is_contiguous():
        raise ValueError(f"{fn}: {what} must be a contiguous [D,H,W] tensor, got {tuple(t.shape)}")


def check_table(t, rows, cols, dtype, what, fn, note=""):
    """`t` is a contiguous `dtype` [rows, cols] tensor; rows None: any number of rows"""
    if not torch.is_tensor(t) or t.dtype != dtype or t.dim() != 2 or t.shape[1] != cols or not t.is_contiguous() or (
            rows is not None and t.shape[0] != rows):
        raise ValueError(f"{fn}: {what} must be a contiguous {str(dtype)[6:]} [{'n' if rows is None else rows}, {cols}] tensor{note}")


def one_device(fn, *tensors, what="the volumes and the tables"):
    if len({t.device for t in tensors if t is not None}) != 1:
        raise ValueError(f"{fn}: {what} must be on one device")


class WorkspaceCache:
    """uint8 workspaces that stay allocated: a call allocates nothing once its shape has been seen.  by_shape False: one buffer per
    device, grown on demand; True: one per (device, shape), so that a word a call left in it can be read back afterwards."""

    def __init__(self, by_shape):
        self.by_shape, self.buffers = by_shape, {}

    def get(self, query_symbol, device, shape):
        """(workspace, the bytes `query_symbol` asks for a volume of `shape`)"""
        shape = tuple(int(s) for s in shape)
        key = (device, shape) if self.by_shape else device
        ws = self.buffers.get(key)
        if ws is not None and self.by_shape:
            return ws, ws.numel()
        nbytes = hip.query(query_symbol, *shape)
        if nbytes == 0:
            raise RuntimeError(f"{query_symbol} failed: {hip.load().rpnet_last_error_string().decode()}")
        if ws is None or ws.numel() < nbytes:
            ws = self.buffers[key] = torch.empty((nbytes,), device=device, dtype=torch.uint8)
        return ws, nbytes


def prepare_class_filter(fn, verb, mask, classes, truth, out, counts, stats, stats_cols, counts_cols):
    """the argument checks and the tables of a per-class filter of a volume (one row per class) -> (classes, out, counts, stats)"""
    hip.require_gpu(mask, truth, out, counts, stats)
    check_volume(mask, "mask", fn)
    classes = [int(c) for c in classes]
    if not classes:
        raise ValueError(f"{fn}: no class to {verb}")
    if truth is not None:
        check_volume(truth, "truth", fn)
        if truth.shape != mask.shape:
            raise ValueError(f"{fn}: mask {tuple(mask.shape)} and truth {tuple(truth.shape)} differ in shape")
    elif counts is not None:
        raise ValueError(f"{fn}: counts need a truth volume (there is nothing to tally without the ground truth)")
    if out is None:
        out = torch.empty(mask.shape, device=mask.device, dtype=torch.uint8)
    elif out.dtype != torch.uint8 or out.shape != mask.shape or not out.is_contiguous():
        raise ValueError(f"{fn}: out must be a contiguous uint8 tensor of shape {tuple(mask.shape)}")
    if stats is None:
        stats = torch.zeros((len(classes), stats_cols), device=mask.device, dtype=torch.int64)
    check_table(stats, len(classes), stats_cols, torch.int64, "stats", fn)
    if truth is not None:
        if counts is None:
            counts = torch.zeros((len(classes), counts_cols), device=mask.device, dtype=torch.int64)
        check_table(counts, len(classes), counts_cols, torch.int64, "counts", fn)
    one_device(fn, mask, truth, out, counts, stats)
    return classes, out, counts, stats


def fmt(v):
    """a figure as the evaluation lines print it"""
    return "None" if v is None else f"{v:.4f}"


def mean_of(rows, key=None):
    """the mean of r[key] (of r itself without a key) over the rows where it is not None; None where there is none"""
    vals = [v for v in (rows if key is None else (r[key] for r in rows)) if v is not None]
    return float(np.mean(vals)) if vals else None


def hd95_from(d2_k, d2_k1, n, k):
    """np.percentile(., 95) of n pooled distances from the squares of the order statistics k = floor((n - 1) * 0.95) and k + 1"""
    def _lerp(a, b, t):
        """numpy's interpolation between two order statistics (numpy/lib/_function_base_impl.py:_lerp)"""
        d = b - a
        return b - d * (1 - t) if t >= 0.5 else a + d * t
    return _lerp(math.sqrt(d2_k), math.sqrt(d2_k1), (n - 1) * 0.95 - k)     # numpy: virtual index (n - 1) * q, q = 95 / 100
