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
from ._volume_checks import KINDS, WorkspaceCache, check_table, check_volume, fmt, mean_of, one_device, prepare_class_filter

STATS_ROW, COUNTS_ROW = 4, 3        # RPNET_CC_STATS_ROW, RPNET_CC_COUNTS_ROW
MAX_DIM = 1024                      # RPNET_CC_MAX_DIM
OVERRUN_OFFSET = 24                 # RPNET_CC_OVERRUN_OFFSET
_workspaces = WorkspaceCache(by_shape=True)     # overrun() reads the word a call left in the buffer of its shape


def connectivity_of(keep_largest):
    """the `keep_largest` option of VolumeSegmenter / evaluate_dataset -> 0 (off), 6 or 26; True means 6"""
    if keep_largest is False or keep_largest is None:
        return 0
    if keep_largest is True:
        return 6
    if isinstance(keep_largest, (int, np.integer)) and int(keep_largest) in (6, 26):
        return int(keep_largest)
    raise ValueError(f"keep_largest must be False, True (connectivity 6), 6 or 26, got {keep_largest!r}")


def overrun(device, shape):
    """the `overrun` word the last call on a volume of this shape left in its workspace (0 unless a bounded loop ran out of its bound);
    a device-to-host copy: for tests and diagnosis, the product path reads the same fact from the statistics row (n_components -1)"""
    ws, _ = _workspaces.get("rpnet_cc_workspace_bytes", torch.device(device), shape)
    return int(ws[OVERRUN_OFFSET:OVERRUN_OFFSET + 4].view(torch.int32).item())


def label_components(vol, cls=1, connectivity=6, labels=None, stats=None, row=0):
    """One `rpnet_cc_label` on the current stream -> (labels int32 [D,H,W], stats int64 [n,4]) with the statistics of class `cls` in
    stats[row].  vol: a contiguous [D,H,W] GPU tensor of uint8, int32, int64 or float32, every extent 1..1024.  Launches only: nothing is
    copied or synchronised."""
    hip.require_gpu(vol, labels, stats)
    check_volume(vol, "vol", "label_components")
    if labels is None:
        labels = torch.empty(vol.shape, device=vol.device, dtype=torch.int32)
    elif labels.dtype != torch.int32 or labels.shape != vol.shape or not labels.is_contiguous():
        raise ValueError(f"label_components: labels must be a contiguous int32 tensor of shape {tuple(vol.shape)}")
    if stats is None:
        stats = torch.zeros((int(row) + 1, STATS_ROW), device=vol.device, dtype=torch.int64)
    check_table(stats, None, STATS_ROW, torch.int64, "stats", "label_components")
    one_device("label_components", vol, labels, stats, what="the volume, the labels and the table")
    D, H, W = vol.shape
    ws, _ = _workspaces.get("rpnet_cc_workspace_bytes", vol.device, (D, H, W))
    hip.call("rpnet_cc_label", hip.ptr(vol), KINDS[vol.dtype], int(cls), D, H, W, int(connectivity), hip.ptr(labels), hip.ptr(stats), int(row),
             stats.shape[0], hip.ptr(ws), ws.numel())
    return labels, stats


def keep_largest(mask, classes=(1,), connectivity=6, truth=None, out=None, counts=None, stats=None):
    """Keep the largest component of every class in `classes`, one `rpnet_cc_keep_largest` call per class on the current stream ->
    (out uint8 [D,H,W], counts int64 [len(classes), 3] or None, stats int64 [len(classes), 4]); row r belongs to classes[r].  Voxels
    of a listed class outside its largest component become 0; every other value passes through (as uint8).  out may be `mask` itself
    when that is uint8 (in place).  truth (a volume of any accepted kind): the Dice counts |P and T|, |P|, |T| of each filtered class
    are ADDED to counts (made of zeros when not handed in).  Launches only: nothing is copied or synchronised."""
    classes, out, counts, stats = prepare_class_filter("keep_largest", "filter", mask, classes, truth, out, counts, stats, STATS_ROW, COUNTS_ROW)
    D, H, W = mask.shape
    ws, _ = _workspaces.get("rpnet_cc_workspace_bytes", mask.device, (D, H, W))
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


def _cc_unit(v, unit):
    return fmt(v) + (unit if v is not None else "")


def line_suffix(dice, figures, surface=None, unit=""):
    """what an item line gains: ` lcc <dice> (<n_components> components, <removed> voxels removed)`, then ` lcc hd95 <v> assd <v>`
    where the surface distances of the filtered mask were measured (each followed by `unit`: `mm` under a voxel spacing)"""
    s = f" lcc {dice} ({figures['n_components']} components, {figures['removed']} voxels removed)"
    if surface is not None:
        s += f" lcc hd95 {_cc_unit(surface['hd95'], unit)} assd {_cc_unit(surface['assd'], unit)}"
    return s


def mean_suffix(dices, figures, surfaces=None, unit=""):
    """what a class line gains: the same figures as means over the items (Dice and distances over the items where they are not None)"""
    s = (f" lcc {fmt(mean_of(dices))} ({np.mean([f['n_components'] for f in figures]):.2f} components, "
         f"{np.mean([f['removed'] for f in figures]):.2f} voxels removed)")
    if surfaces is not None:
        s += f" lcc hd95 {_cc_unit(mean_of(surfaces, 'hd95'), unit)} assd {_cc_unit(mean_of(surfaces, 'assd'), unit)}"
    return s
