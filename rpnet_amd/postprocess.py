"""Hole filling and the small-component filter of a segmented volume (csrc/cc_post.hip, include/rpnet_ccpost_abi.h): with
components.keep_largest the clean-up chain every slice-by-slice abdominal pipeline ends with, without the round trip through
scipy.ndimage.binary_fill_holes / label on the host.

Definitions.  A volume [D,H,W], a class cls; the object is `value == cls`.

Holes.  The complement is `value != cls`; its voxels are neighbours under background connectivity 6 or 26
(structure=generate_binary_structure(3, 1) or (3, 3) of scipy.ndimage.binary_fill_holes; 6 is scipy's default).  per_slice: the background
connectivity is 4 or 8 (generate_binary_structure(2, 1) or (2, 2)), every z slice is its own 2D image with no link across z, and the border
is the slice's own four edges.  A complement component is a hole when none of its voxels lies on the border of the volume (of its slice)
and its size is <= max_hole (None: no bound).  Filling writes cls to the voxels of a hole whose value is 0; voxels of other classes inside
a hole pass through unchanged.  With one foreground class, the only case the evaluation reaches, and no bound this is exactly
scipy.ndimage.binary_fill_holes.

Small components.  The components of `value == cls` under connectivity 6 or 26, with the labels of components.label_components.  A
component is removed (its voxels set to 0) when its size is < min_voxels; other classes pass through unchanged.

A statistics row is int64: holes {n_complement_components, n_holes, voxels_filled, largest_hole}, small {n_components, n_removed,
voxels_removed, largest_removed}; a counts row is int64 {|P and T|, |P|, |T|} of the class in the result, ADDED to what the row holds.
A first statistics column of -1 says that a bounded loop of the kernels ran out of its bound.  Everything is integer work: two runs give
the same bits.  tests/postprocess_cases.py restates both definitions in numpy and is what the GPU tests compare with.
"""
import math

import numpy as np
import torch

from . import hip
from ._volume_checks import KINDS, WorkspaceCache, prepare_class_filter

STATS_ROW, COUNTS_ROW = 4, 3        # RPNET_CCPOST_STATS_ROW, RPNET_CCPOST_COUNTS_ROW
OVERRUN_OFFSET = 24                 # RPNET_CCPOST_OVERRUN_OFFSET
_post_workspaces = WorkspaceCache(by_shape=True)    # post_overrun() reads the word a call left in the buffer of its shape


def holes_mode_of(fill_holes):
    """the `fill_holes` option of VolumeSegmenter / evaluate_dataset -> None (off), False (3D) or True (per slice)"""
    if fill_holes is False or fill_holes is None:
        return None
    if fill_holes is True or fill_holes == "3d":
        return False
    if fill_holes == "slice":
        return True
    raise ValueError(f"fill_holes must be False, True (3D), '3d' or 'slice', got {fill_holes!r}")


def hole_connectivity_of(hole_connectivity, per_slice):
    """the background connectivity of fill_holes -> 6 or 26, per slice 4 or 8.  None means the faces only (6, per slice 4); per slice
    6 and 26 are accepted too and stand for their in-plane subsets 4 and 8.  The one rule for `connectivity` of fill_holes and for
    `hole_connectivity` of VolumeSegmenter / evaluate_dataset."""
    allowed = (4, 8) if per_slice else (6, 26)
    if hole_connectivity is None:
        return allowed[0]
    if isinstance(hole_connectivity, (int, np.integer)) and not isinstance(hole_connectivity, bool):
        conn = int(hole_connectivity)
        if per_slice:
            conn = {6: 4, 26: 8}.get(conn, conn)
        if conn in allowed:
            return conn
    raise ValueError(f"hole_connectivity must be None, {allowed[0]} or {allowed[1]}{' (or 6, 26 for them) per slice' if per_slice else ''}, "
                     f"got {hole_connectivity!r}")


def min_voxels_from_mm3(volume_mm3, spacing):
    """the smallest voxel count whose volume reaches `volume_mm3` under the voxel spacing (sz, sy, sx) in mm: ceil(v / (sz*sy*sx)) in
    float64, at least 1"""
    sz, sy, sx = (float(s) for s in spacing)
    if not (sz > 0 and sy > 0 and sx > 0) or not all(math.isfinite(s) for s in (sz, sy, sx)):
        raise ValueError(f"min_voxels_from_mm3: the spacing must be three positive finite numbers, got {tuple(spacing)!r}")
    v = float(volume_mm3)
    if not (v >= 0 and math.isfinite(v)):
        raise ValueError(f"min_voxels_from_mm3: the volume must be a finite number >= 0, got {volume_mm3!r}")
    return max(1, int(math.ceil(v / (sz * sy * sx))))


def post_overrun(device, shape):
    """the `overrun` word the last call on a volume of this shape left in its workspace (0 unless a bounded loop ran out of its bound);
    a device-to-host copy: for tests and diagnosis, the product path reads the same fact from the statistics row (first column -1)"""
    ws, _ = _post_workspaces.get("rpnet_ccpost_workspace_bytes", torch.device(device), shape)
    return int(ws[OVERRUN_OFFSET:OVERRUN_OFFSET + 4].view(torch.int32).item())


def fill_holes(mask, classes, connectivity=6, per_slice=False, max_hole=None, truth=None, out=None, counts=None, stats=None):
    """Fill the holes of every class in `classes`, one `rpnet_ccpost_fill_holes` call per class on the current stream ->
    (out uint8 [D,H,W], counts int64 [len(classes), 3] or None, stats int64 [len(classes), 4]); row r belongs to classes[r].
    connectivity: of the background, 6 or 26; per_slice: 4 or 8, and 6 / 26 stand for their in-plane subsets 4 / 8.  max_hole: the largest hole (in voxels) that is filled, None for no
    bound.  Voxels of value 0 inside a hole of a listed class become that class; every other value passes through (as uint8).  out may be
    `mask` itself when that is uint8 (in place).  truth: the Dice counts of each class in the result are ADDED to counts (made of zeros
    when not handed in).  Launches only: nothing is copied or synchronised."""
    classes, out, counts, stats = prepare_class_filter("fill_holes", "process", mask, classes, truth, out, counts, stats, STATS_ROW, COUNTS_ROW)
    if max_hole is None:
        bound = 0
    else:
        bound = int(max_hole)
        if bound < 1:
            raise ValueError(f"fill_holes: max_hole must be None (no bound) or at least 1 voxel, got {max_hole!r}")
    conn = hole_connectivity_of(connectivity, bool(per_slice))
    D, H, W = mask.shape
    ws, _ = _post_workspaces.get("rpnet_ccpost_workspace_bytes", mask.device, (D, H, W))
    src = mask
    for r, c in enumerate(classes):
        hip.call("rpnet_ccpost_fill_holes", hip.ptr(src), KINDS[src.dtype], hip.ptr(out), c, D, H, W, conn, int(bool(per_slice)), bound,
                 hip.ptr(truth), KINDS[truth.dtype] if truth is not None else 0, hip.ptr(counts), r, hip.ptr(stats), r, len(classes), hip.ptr(ws),
                 ws.numel())
        src = out                       # the classes filled so far are in `out`; the next one is filled there in place
    return out, counts, stats


def remove_small(mask, classes, min_voxels, connectivity=6, truth=None, out=None, counts=None, stats=None):
    """Remove the components of fewer than `min_voxels` voxels of every class in `classes`, one `rpnet_ccpost_remove_small` call per class
    on the current stream -> (out, counts, stats) as fill_holes gives them.  connectivity: 6 or 26.  Voxels of a removed component
    become 0; every other value passes through (as uint8)."""
    classes, out, counts, stats = prepare_class_filter("remove_small", "process", mask, classes, truth, out, counts, stats, STATS_ROW, COUNTS_ROW)
    D, H, W = mask.shape
    ws, _ = _post_workspaces.get("rpnet_ccpost_workspace_bytes", mask.device, (D, H, W))
    src = mask
    for r, c in enumerate(classes):
        hip.call("rpnet_ccpost_remove_small", hip.ptr(src), KINDS[src.dtype], hip.ptr(out), c, D, H, W, int(connectivity), int(min_voxels),
                 hip.ptr(truth), KINDS[truth.dtype] if truth is not None else 0, hip.ptr(counts), r, hip.ptr(stats), r, len(classes), hip.ptr(ws),
                 ws.numel())
        src = out
    return out, counts, stats


def _post_rows(stats_host):
    rows = np.asarray(stats_host).reshape(-1, STATS_ROW)
    if (rows[:, 0] < 0).any():
        raise RuntimeError("rpnet_ccpost: a bounded loop of the component kernels ran out of its bound (the workspace's overrun word is set)")
    return rows


def holes_figures(stats_host):
    """per row of a host table [..., 4]: {'n_complement', 'n_holes', 'filled', 'largest'} -> a flat list.  A first column of -1 is
    raised here, where the table has crossed to the host anyway."""
    return [{"n_complement": int(r[0]), "n_holes": int(r[1]), "filled": int(r[2]), "largest": int(r[3])} for r in _post_rows(stats_host)]


def small_figures(stats_host):
    """per row of a host table [..., 4]: {'n_components', 'n_removed', 'removed', 'largest'} -> a flat list"""
    return [{"n_components": int(r[0]), "n_removed": int(r[1]), "removed": int(r[2]), "largest": int(r[3])} for r in _post_rows(stats_host)]


def line_suffix(holes=None, small=None):
    """what an item line gains: ` holes <n> (<filled> voxels filled)` and ` small <n> (<removed> voxels removed)`, each for the stage
    that ran"""
    s = ""
    if holes is not None:
        s += f" holes {holes['n_holes']} ({holes['filled']} voxels filled)"
    if small is not None:
        s += f" small {small['n_removed']} ({small['removed']} voxels removed)"
    return s


def mean_suffix(holes=None, small=None):
    """what a class line gains: the same figures as means over the items (lists of figures)"""
    s = ""
    if holes is not None:
        s += f" holes {np.mean([f['n_holes'] for f in holes]):.2f} ({np.mean([f['filled'] for f in holes]):.2f} voxels filled)"
    if small is not None:
        s += f" small {np.mean([f['n_removed'] for f in small]):.2f} ({np.mean([f['removed'] for f in small]):.2f} voxels removed)"
    return s
