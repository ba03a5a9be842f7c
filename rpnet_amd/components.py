"""Connected components of a segmented volume and the filter that keeps the largest one per class (csrc/components.hip,
include/rpnet_cc_abi.h): the post-processing step every user of a slice-by-slice segmenter applies before measuring surface distances
(a stray island a few voxels large decides HD and moves HD95), without the round trip through scipy.ndimage.label on the host.

Definition.  Foreground is `value == cls`; two foreground voxels are neighbours when they share a face (connectivity 6) or a face, an
edge or a corner (26); voxels outside the volume are background.  labels (int32 [D,H,W]): background 0, a foreground voxel
1 + the smallest linear index z*H*W + y*W + x of its component, whatever the order in which blocks ran.  The largest component is the
one with the most voxels and, among equals, the one whose first voxel comes first: np.argmax(np.bincount(lab.ravel())[1:]) on a
scipy.ndimage.label result.  A statistics row is int64 {n_foreground, n_components, size_largest, first_index_largest} (0, 0, 0, -1 for
an empty class), a counts row int64 {|P and T|, |P|, |T|} of the filtered class.  Everything is integer work: two runs give the same
bits.  tests/components_cases.py:ref_label restates the contract in numpy and is what the GPU tests compare with.
"""
import numpy as np
import torch

from . import hip
from .surface import KINDS

STATS_ROW, COUNTS_ROW = 4, 3        # RPNET_CC_STATS_ROW, RPNET_CC_COUNTS_ROW
MAX_DIM = 1024                      # RPNET_CC_MAX_DIM
OVERRUN_OFFSET = 24                 # RPNET_CC_OVERRUN_OFFSET
_workspaces = {}                    # (device, (D, H, W)) -> uint8 tensor: a call allocates nothing once its shape has been seen


def connectivity_of(keep_largest):
    """the `keep_largest` option of VolumeSegmenter / evaluate_dataset -> 0 (off), 6 or 26; True means 6"""
    if keep_largest is False or keep_largest is None:
        return 0
    if keep_largest is True:
        return 6
    if isinstance(keep_largest, (int, np.integer)) and int(keep_largest) in (6, 26):
        return int(keep_largest)
    raise ValueError(f"keep_largest must be False, True (connectivity 6), 6 or 26, got {keep_largest!r}")


def _cc_workspace(device, shape):
    key = (device, tuple(int(s) for s in shape))
    ws = _workspaces.get(key)
    if ws is None:
        nbytes = hip.query("rpnet_cc_workspace_bytes", *key[1])
        if nbytes == 0:
            raise RuntimeError(f"rpnet_cc_workspace_bytes failed: {hip.load().rpnet_last_error_string().decode()}")
        ws = _workspaces[key] = torch.empty((nbytes,), device=device, dtype=torch.uint8)
    return ws


def overrun(device, shape):
    """the `overrun` word the last call on a volume of this shape left in its workspace (0 unless a bounded loop ran out of its bound);
    a device-to-host copy: for tests and diagnosis, the product path reads the same fact from the statistics row (n_components -1)"""
    ws = _cc_workspace(torch.device(device), shape)
    return int(ws[OVERRUN_OFFSET:OVERRUN_OFFSET + 4].view(torch.int32).item())


def _cc_volume(t, what, fn):
    if t.dtype not in KINDS:
        raise ValueError(f"{fn}: {what} is {t.dtype}; uint8, int32, int64 and float32 volumes are accepted")
    if t.dim() != 3 or not t.is_contiguous():
        raise ValueError(f"{fn}: {what} must be a contiguous [D,H,W] tensor, got {tuple(t.shape)}")


def _cc_table(t, rows, cols, what, fn):
    if not torch.is_tensor(t) or t.dtype != torch.int64 or t.dim() != 2 or t.shape[1] != cols or not t.is_contiguous() or (
            rows is not None and t.shape[0] != rows):
        raise ValueError(f"{fn}: {what} must be a contiguous int64 [{'n' if rows is None else rows}, {cols}] tensor")


def label_components(vol, cls=1, connectivity=6, labels=None, stats=None, row=0):
    """One `rpnet_cc_label` on the current stream -> (labels int32 [D,H,W], stats int64 [n,4]) with the statistics of class `cls` in
    stats[row].  vol: a contiguous [D,H,W] GPU tensor of uint8, int32, int64 or float32, every extent 1..1024.  Launches only: nothing is
    copied or synchronised."""
    hip.require_gpu(vol, labels, stats)
    _cc_volume(vol, "vol", "label_components")
    if labels is None:
        labels = torch.empty(vol.shape, device=vol.device, dtype=torch.int32)
    elif labels.dtype != torch.int32 or labels.shape != vol.shape or not labels.is_contiguous():
        raise ValueError(f"label_components: labels must be a contiguous int32 tensor of shape {tuple(vol.shape)}")
    if stats is None:
        stats = torch.zeros((int(row) + 1, STATS_ROW), device=vol.device, dtype=torch.int64)
    _cc_table(stats, None, STATS_ROW, "stats", "label_components")
    if len({vol.device, labels.device, stats.device}) != 1:
        raise ValueError("label_components: the volume, the labels and the table must be on one device")
    D, H, W = vol.shape
    ws = _cc_workspace(vol.device, (D, H, W))
    hip.call("rpnet_cc_label", hip.ptr(vol), KINDS[vol.dtype], int(cls), D, H, W, int(connectivity), hip.ptr(labels), hip.ptr(stats), int(row),
             stats.shape[0], hip.ptr(ws), ws.numel())
    return labels, stats


def keep_largest(mask, classes=(1,), connectivity=6, truth=None, out=None, counts=None, stats=None):
    """Keep the largest component of every class in `classes`, one `rpnet_cc_keep_largest` call per class on the current stream ->
    (out uint8 [D,H,W], counts int64 [len(classes), 3] or None, stats int64 [len(classes), 4]); row r belongs to classes[r].  Voxels
    of a listed class outside its largest component become 0; every other value passes through (as uint8).  out may be `mask` itself
    when that is uint8 (in place).  truth (a volume of any accepted kind): the Dice counts |P and T|, |P|, |T| of each filtered class
    are ADDED to counts (made of zeros when not handed in).  Launches only: nothing is copied or synchronised."""
    hip.require_gpu(mask, truth, out, counts, stats)
    _cc_volume(mask, "mask", "keep_largest")
    classes = [int(c) for c in classes]
    if not classes:
        raise ValueError("keep_largest: no class to filter")
    if truth is not None:
        _cc_volume(truth, "truth", "keep_largest")
        if truth.shape != mask.shape:
            raise ValueError(f"keep_largest: mask {tuple(mask.shape)} and truth {tuple(truth.shape)} differ in shape")
    elif counts is not None:
        raise ValueError("keep_largest: counts need a truth volume (there is nothing to tally without the ground truth)")
    if out is None:
        out = torch.empty(mask.shape, device=mask.device, dtype=torch.uint8)
    elif out.dtype != torch.uint8 or out.shape != mask.shape or not out.is_contiguous():
        raise ValueError(f"keep_largest: out must be a contiguous uint8 tensor of shape {tuple(mask.shape)}")
    if stats is None:
        stats = torch.zeros((len(classes), STATS_ROW), device=mask.device, dtype=torch.int64)
    _cc_table(stats, len(classes), STATS_ROW, "stats", "keep_largest")
    if truth is not None:
        if counts is None:
            counts = torch.zeros((len(classes), COUNTS_ROW), device=mask.device, dtype=torch.int64)
        _cc_table(counts, len(classes), COUNTS_ROW, "counts", "keep_largest")
    if len({t.device for t in (mask, truth, out, counts, stats) if t is not None}) != 1:
        raise ValueError("keep_largest: the volumes and the tables must be on one device")
    D, H, W = mask.shape
    ws = _cc_workspace(mask.device, (D, H, W))
    src = mask
    for r, c in enumerate(classes):
        hip.call("rpnet_cc_keep_largest", hip.ptr(src), KINDS[src.dtype], hip.ptr(out), c, D, H, W, int(connectivity), hip.ptr(truth),
                 KINDS[truth.dtype] if truth is not None else 0, hip.ptr(counts), r, hip.ptr(stats), r, len(classes), hip.ptr(ws), ws.numel())
        src = out                       # the classes filtered so far are in `out`; the next one is filtered there in place
    return out, counts, stats


def components_figures(stats_host):
    """per row of a host table [..., 4]: {'n_components', 'kept' (voxels of the largest component), 'removed' (the other foreground
    voxels)} -> a flat list.  A row with n_components -1 says that a bounded loop of the kernels ran out of its bound: raised here,
    where the table has crossed to the host anyway."""
    rows = np.asarray(stats_host).reshape(-1, STATS_ROW)
    if (rows[:, 1] < 0).any():
        raise RuntimeError("rpnet_cc: a bounded loop of the component kernels ran out of its bound (the workspace's overrun word is set)")
    return [{"n_components": int(r[1]), "kept": int(r[2]), "removed": int(r[0] - r[2])} for r in rows]


def _cc_fmt(v):
    return "None" if v is None else f"{v:.4f}"


def _cc_unit(v, unit):
    return _cc_fmt(v) + (unit if v is not None else "")


def line_suffix(dice, figures, surface=None, unit=""):
    """what an item line gains: ` lcc <dice> (<n_components> components, <removed> voxels removed)`, then ` lcc hd95 <v> assd <v>`
    where the surface distances of the filtered mask were measured (each followed by `unit`: `mm` under a voxel spacing)"""
    s = f" lcc {dice} ({figures['n_components']} components, {figures['removed']} voxels removed)"
    if surface is not None:
        s += f" lcc hd95 {_cc_unit(surface['hd95'], unit)} assd {_cc_unit(surface['assd'], unit)}"
    return s


def mean_suffix(dices, figures, surfaces=None, unit=""):
    """what a class line gains: the same figures as means over the items (Dice and distances over the items where they are not None)"""
    def mean(vals):
        vals = [v for v in vals if v is not None]
        return float(np.mean(vals)) if vals else None
    s = (f" lcc {_cc_fmt(mean(dices))} ({np.mean([f['n_components'] for f in figures]):.2f} components, "
         f"{np.mean([f['removed'] for f in figures]):.2f} voxels removed)")
    if surfaces is not None:
        s += f" lcc hd95 {_cc_unit(mean([r['hd95'] for r in surfaces]), unit)} assd {_cc_unit(mean([r['assd'] for r in surfaces]), unit)}"
    return s
