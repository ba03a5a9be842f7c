"""Per-component statistics of a segmented volume on the device (csrc/compstat.hip, include/rpnet_compstat_abi.h): how many islands a
class has, how big each is, where it sits, what the image holds inside it and whether it touches a class of a second volume, without
the round trip through scipy.ndimage.label and six more scipy calls on the host.

`rank_components` renumbers the sparse labels of rpnet_amd.components.label_components (0, or 1 + the smallest linear index of the
component) to the ids 1 .. C by the rank of each component's first voxel in z-major order: scipy.ndimage.label's own numbering.
`component_table` chains labelling, renumbering and one tally pass and leaves an int64 table on the device, row k - 1 for the id k:
n | min z y x | max z y x | sum z y x | sum zz yy xx | sum zy zx yx | n_summed | smallest and largest order-preserving key | S1 = SUM k |
SUM (k*k & 0xFFFFFFFF) | SUM (k*k >> 32) | n_overlap | first index, where k = rint(v * 2^scale_log2), ties to even, in float64, of the
image value v.  Every entry is an exact integer (integer atomics only), so two runs, and the numpy restatement of
tests/compstat_cases.py, give the same words; the mean and the standard deviation `derive_components` forms are those of the
quantised values, within 2^-(scale_log2 + 1) of those of the values themselves.  `detection_counts` turns the tables of a prediction
and of the labels into lesion-wise TP / FN / FP counts under the any-overlap rule.

Limits: one class at a time; max_components <= 65536 (the components beyond it are counted, not tallied); extents up to 1024; no
pair-wise overlap table and no one-to-one matching; no order statistics of the intensity; no surface area; a spacing per axis.
"""
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np
import torch

from . import hip
from ._volume_checks import KINDS, WorkspaceCache, check_table, check_volume, fmt, mean_of, one_device
from .components import label_components
from .regions import IMAGE_KINDS, key_to_float

MAX_COMPONENTS = 65536               # RPNET_COMPSTAT_MAX_COMPONENTS
COMP_ROW, COMP_STATS_ROW = 24, 4     # RPNET_COMPSTAT_ROW, RPNET_COMPSTAT_STATS_ROW
COMP_CHUNK = 4096                    # RPNET_COMPSTAT_CHUNK
COMP_HEAD_BYTES = 64                 # RPNET_COMPSTAT_HEAD_BYTES
# RPNET_COMPSTAT_COUNT_OFFSET, _INVALID_OFFSET, _BEYOND_OFFSET, _TABLE_INVALID_OFFSET: the four int64 words of the head
COUNT_OFFSET, INVALID_OFFSET, BEYOND_OFFSET, TABLE_INVALID_OFFSET = 0, 8, 16, 24
HEAD_WORDS = 4
MAX_SCALE_LOG2 = 30                  # RPNET_COMPSTAT_MAX_SCALE_LOG2
MAX_DIM = 1024                       # RPNET_CC_MAX_DIM
DEFAULT_MAX_COMPONENTS = 4096
_workspaces = WorkspaceCache(by_shape=True)

ComponentTable = namedtuple("ComponentTable", ["rows", "dense", "head", "scale_log2"])


def _compstat_workspace_layout(D, H, W):
    """byte offsets of (the chunk counts int32 [nc rounded up to 4], the rank volume int32 [n]) inside the workspace, and its size"""
    nc = (D * H * W + COMP_CHUNK - 1) // COMP_CHUNK
    counts = 4 * ((nc + 3) // 4 * 4)
    return (COMP_HEAD_BYTES, COMP_HEAD_BYTES + counts), COMP_HEAD_BYTES + counts + 4 * D * H * W


def check_max_components(max_components, fn):
    if isinstance(max_components, bool) or not isinstance(max_components, (int, np.integer)) or not 1 <= int(max_components) <= MAX_COMPONENTS:
        raise ValueError(f"{fn}: max_components is an integer 1..{MAX_COMPONENTS}, got {max_components!r}")
    return int(max_components)


def components_option(components):
    """the `components` option of the volume segmenter and the data-set evaluation -> 0 (off) or max_components; True means 4096"""
    if components is False or components is None:
        return 0
    if components is True:
        return DEFAULT_MAX_COMPONENTS
    return check_max_components(components, "components")


def component_workspace(shape, device, max_components=DEFAULT_MAX_COMPONENTS):
    """the workspace the calls of this module keep for volumes of `shape` on `device` (made on first use)"""
    D, H, W = (int(s) for s in shape)
    return _workspaces.get("rpnet_compstat_workspace_bytes", torch.device(device), (D, H, W, check_max_components(max_components, "component_workspace")))[0]


def component_head(workspace):
    """the four int64 words the last calls left in the head of `workspace`, a view on the device: n_components C and the `invalid` count
    of the renumbering, n_beyond (voxels whose id exceeds max_components) and the `invalid` count of the tally"""
    return workspace[:8 * HEAD_WORDS].view(torch.int64)


def _check_extents(fn, t, what):
    if any(not 1 <= int(s) <= MAX_DIM for s in t.shape):
        raise ValueError(f"{fn}: {what} is {tuple(t.shape)}; every extent is 1..{MAX_DIM}")


def rank_components(labels, out=None, stats=None, row=0, workspace=None):
    """One `rpnet_compstat_rank` on the current stream -> (dense int32 [D,H,W], stats int64 [n, 4]): dense holds 0 for background and
    otherwise the id 1 .. C of the voxel's component, C in stats[row][0] (and in `component_head` of the workspace).  labels: the
    contiguous int32 labels of `label_components`.  A label that is neither 0 nor 1 + the index of a voxel that holds that same label
    gives 0 and is counted in stats[row][1].  out may not be `labels`.  Launches only: nothing is copied or synchronised."""
    fn = "rank_components"
    if not torch.is_tensor(labels) or labels.dtype != torch.int32 or labels.dim() != 3 or not labels.is_contiguous():
        raise ValueError(f"{fn}: labels must be a contiguous int32 [D,H,W] tensor")
    _check_extents(fn, labels, "labels")
    if out is not None:
        if not torch.is_tensor(out) or out.dtype != torch.int32 or out.shape != labels.shape or not out.is_contiguous():
            raise ValueError(f"{fn}: out must be a contiguous int32 tensor of shape {tuple(labels.shape)}")
        if out.data_ptr() == labels.data_ptr():
            raise ValueError(f"{fn}: out may not be labels")
    hip.require_gpu(labels, out, stats, workspace)
    if out is None:
        out = torch.empty(labels.shape, device=labels.device, dtype=torch.int32)
    if isinstance(row, bool) or not isinstance(row, (int, np.integer)) or int(row) < 0:
        raise ValueError(f"{fn}: row is a non-negative integer, got {row!r}")
    if stats is None:
        stats = torch.zeros((int(row) + 1, COMP_STATS_ROW), device=labels.device, dtype=torch.int64)
    check_table(stats, None, COMP_STATS_ROW, torch.int64, "stats", fn)
    if int(row) >= stats.shape[0]:
        raise ValueError(f"{fn}: row {row} of a table of {stats.shape[0]} rows")
    D, H, W = (int(s) for s in labels.shape)
    workspace, nbytes = _take_workspace(fn, workspace, labels.device, (D, H, W))
    one_device(fn, labels, out, stats, workspace)
    hip.call("rpnet_compstat_rank", hip.ptr(labels), D, H, W, hip.ptr(out), hip.ptr(stats), int(row), stats.shape[0], hip.ptr(workspace), nbytes)
    return out, stats


def _take_workspace(fn, workspace, device, dims):
    if workspace is None:
        return _workspaces.get("rpnet_compstat_workspace_bytes", device, dims + (DEFAULT_MAX_COMPONENTS,))
    need = _compstat_workspace_layout(*dims)[1]
    if not torch.is_tensor(workspace) or workspace.dtype != torch.uint8 or workspace.dim() != 1 or not workspace.is_contiguous():
        raise ValueError(f"{fn}: workspace must be a contiguous 1-d uint8 tensor")
    if workspace.numel() < need:
        raise ValueError(f"{fn}: workspace of {workspace.numel()} bytes, {need} needed")
    if workspace.is_cuda and workspace.data_ptr() % 16:
        raise ValueError(f"{fn}: workspace must be aligned to 16 bytes")
    return workspace, workspace.numel()


def default_scale_log2(image):
    """0 for an int16 image (the values enter as they are), 16 for a float32 one (a step of 2^-16; values up to 32768 in magnitude)"""
    return 0 if image is None or image.dtype == torch.int16 else 16


def tally_components(dense, image=None, other=None, other_cls=1, max_components=DEFAULT_MAX_COMPONENTS, scale_log2=None, out=None, row=0,
                     workspace=None):
    """One `rpnet_compstat_table` on the current stream -> rows int64 [n, max_components, 24] with the table of `dense` in rows[row].
    dense: the int32 volume of the renumbering; the workspace is the one that call used (its head holds C).  image: None, or a
    contiguous float32 or int16 volume of the same shape; other: None, or a volume of any of the four label kinds, of which the voxels
    equal to other_cls count as overlap.  The rows are WRITTEN, all max_components of them.  Launches only."""
    fn = "tally_components"
    if not torch.is_tensor(dense) or dense.dtype != torch.int32 or dense.dim() != 3 or not dense.is_contiguous():
        raise ValueError(f"{fn}: dense must be a contiguous int32 [D,H,W] tensor")
    _check_extents(fn, dense, "dense")
    max_components = check_max_components(max_components, fn)
    if image is not None:
        if not torch.is_tensor(image) or image.dtype not in IMAGE_KINDS:
            raise ValueError(f"{fn}: image must be a float32 or int16 tensor")
        if image.shape != dense.shape or not image.is_contiguous():
            raise ValueError(f"{fn}: image must be a contiguous tensor of the volume's shape {tuple(dense.shape)}, got {tuple(image.shape)}")
    if scale_log2 is None:
        scale_log2 = default_scale_log2(image)
    if isinstance(scale_log2, bool) or not isinstance(scale_log2, (int, np.integer)) or not 0 <= int(scale_log2) <= MAX_SCALE_LOG2:
        raise ValueError(f"{fn}: scale_log2 is an integer 0..{MAX_SCALE_LOG2}, got {scale_log2!r}")
    if other is not None:
        if not torch.is_tensor(other):
            raise ValueError(f"{fn}: other must be a tensor")
        check_volume(other, "other", fn)
        if other.shape != dense.shape:
            raise ValueError(f"{fn}: other must have the volume's shape {tuple(dense.shape)}, got {tuple(other.shape)}")
    if isinstance(row, bool) or not isinstance(row, (int, np.integer)) or int(row) < 0:
        raise ValueError(f"{fn}: row is a non-negative integer, got {row!r}")
    hip.require_gpu(dense, image, other, out, workspace)
    if out is None:
        out = torch.empty((int(row) + 1, max_components, COMP_ROW), device=dense.device, dtype=torch.int64)
    elif (not torch.is_tensor(out) or out.dtype != torch.int64 or out.dim() != 3 or tuple(out.shape[1:]) != (max_components, COMP_ROW)
          or not out.is_contiguous()):
        raise ValueError(f"{fn}: out must be a contiguous int64 [n, {max_components}, {COMP_ROW}] tensor")
    if int(row) >= out.shape[0]:
        raise ValueError(f"{fn}: row {row} of a table of {out.shape[0]} rows")
    D, H, W = (int(s) for s in dense.shape)
    workspace, nbytes = _take_workspace(fn, workspace, dense.device, (D, H, W))
    one_device(fn, dense, image, other, out, workspace)
    hip.call("rpnet_compstat_table", hip.ptr(dense), hip.ptr(image), IMAGE_KINDS[image.dtype] if image is not None else 0, int(scale_log2),
             hip.ptr(other), KINDS[other.dtype] if other is not None else 0, int(other_cls), D, H, W, max_components, hip.ptr(out), int(row),
             out.shape[0], hip.ptr(workspace), nbytes)
    return out


def component_table(vol, cls=1, connectivity=6, image=None, other=None, other_cls=None, max_components=DEFAULT_MAX_COMPONENTS, scale_log2=None,
                    out=None, row=0, head_out=None, labels=None, dense=None):
    """`label_components` -> `rank_components` -> `tally_components` on the current stream for the class `cls` of `vol` (a contiguous
    [D,H,W] volume of uint8, int32, int64 or float32) -> ComponentTable(rows, dense, head, scale_log2), all on the device:
      rows   int64 [max_components, 24], row k - 1 of the component k (out=: the table [n, max_components, 24] handed in, written at `row`)
      dense  int32 [D,H,W], the ids 1 .. C in scipy.ndimage.label's order
      head   int64 [4]: the number of components C (which may exceed max_components), the labels the renumbering found invalid (0 after
             label_components), n_beyond (the voxels of the components beyond max_components, which enter no row) and the ids the tally
             found invalid (0); head_out=: an int64 [4] tensor to receive them
    image, other, scale_log2: as in `tally_components`; scale_log2 None is 0 for an int16 image and 16 for a float32 one; other_cls None
    is `cls`.  labels=, dense=: int32 volumes to use instead of new ones.  Launches and device copies only: nothing crosses to the host,
    so the chain can be captured in a graph once its workspaces exist."""
    fn = "component_table"
    if not torch.is_tensor(vol):
        raise ValueError(f"{fn}: vol must be a tensor")
    check_volume(vol, "vol", fn)
    _check_extents(fn, vol, "vol")
    if connectivity not in (6, 26):
        raise ValueError(f"{fn}: connectivity is 6 or 26, got {connectivity!r}")
    max_components = check_max_components(max_components, fn)
    if scale_log2 is None:
        scale_log2 = default_scale_log2(image)
    if head_out is not None and (not torch.is_tensor(head_out) or head_out.dtype != torch.int64 or tuple(head_out.shape) != (HEAD_WORDS,)):
        raise ValueError(f"{fn}: head_out must be an int64 [{HEAD_WORDS}] tensor")
    labels, _ = label_components(vol, cls=cls, connectivity=connectivity, labels=labels)
    dense, _ = rank_components(labels, out=dense)
    rows = tally_components(dense, image, other, cls if other_cls is None else other_cls, max_components, scale_log2, out=out, row=row)
    head = component_head(component_workspace(vol.shape, vol.device))
    if head_out is None:
        head_out = head.clone()
    else:
        head_out.copy_(head)
    return ComponentTable(rows[0] if out is None else rows, dense, head_out, int(scale_log2))


def derive_components(rows, spacing=None, scale_log2=0):
    """The figures of every component from a table of this module's chain, once it has crossed to the host: rows int64 [N, 24], spacing
    None or (sz, sy, sx), scale_log2 the one the table was made with -> a list with one dict per row that holds voxels (the ids 1, 2,
    ... in order):
      id, voxels, first_index, bbox ((z0, y0, x0), (z1, y1, x1)) inclusive, centroid (z, y, x) in voxels, extent (voxels of the box)
      volume_mm3, volume_ml, centroid_mm, extent_mm           None without a spacing
      mean, std (population), min, max, n_unsummed            of the image inside the component; None for a table made without an image.
                                                              mean and std are those of the quantised values k / 2^scale_log2, formed
                                                              from exact integers: within 2^-(scale_log2 + 1) of those of the values;
                                                              min and max are values of the image itself
      overlap, overlap_fraction                               voxels of the component inside the class of `other`, and n_overlap / n"""
    r_all = np.asarray(rows)
    if r_all.ndim != 2 or r_all.shape[1] != COMP_ROW:
        raise ValueError(f"derive_components: rows must be [N, {COMP_ROW}], got {r_all.shape}")
    if spacing is not None:
        from .surface_spacing import check_spacing
        spacing = check_spacing(spacing, "derive_components")
    unit = 1 << int(scale_log2)
    out = []
    for i in np.flatnonzero(r_all[:, 0] > 0):
        r = [int(v) for v in r_all[i]]
        n = r[0]
        fig = dict(id=int(i) + 1, voxels=n, first_index=r[23], bbox=(tuple(r[1:4]), tuple(r[4:7])), centroid=tuple(r[7 + a] / n for a in range(3)),
                   extent=tuple(r[4 + a] - r[1 + a] + 1 for a in range(3)), volume_mm3=None, volume_ml=None, centroid_mm=None, extent_mm=None,
                   mean=None, std=None, min=None, max=None, n_unsummed=n - r[16], overlap=r[22], overlap_fraction=r[22] / n)
        if spacing is not None:
            fig["volume_mm3"] = n * spacing[0] * spacing[1] * spacing[2]
            fig["volume_ml"] = fig["volume_mm3"] / 1000.0
            fig["centroid_mm"] = tuple(fig["centroid"][a] * spacing[a] for a in range(3))
            fig["extent_mm"] = tuple(fig["extent"][a] * spacing[a] for a in range(3))
        ns = r[16]
        if ns:
            s1, s2 = r[19], r[20] + (r[21] << 32)
            fig["mean"] = s1 / (ns * unit)                                          # integers: one rounding
            fig["std"] = math.sqrt((ns * s2 - s1 * s1) / (ns * ns * unit * unit))   # the cancellation happens before anything is rounded
            lo_hi = key_to_float([r[17], r[18]])
            fig["min"], fig["max"] = float(lo_hi[0]), float(lo_hi[1])
        out.append(fig)
    return out


def _detected(rows, min_overlap):
    r = np.asarray(rows)
    r = r[r[:, 0] > 0]
    n, ov = r[:, 0].astype(object), r[:, 22]
    if isinstance(min_overlap, (int, np.integer)) and not isinstance(min_overlap, bool):
        if int(min_overlap) < 1:
            raise ValueError(f"detection_counts: min_overlap is a voxel count >= 1 or a fraction in (0, 1], got {min_overlap!r}")
        need = np.full(len(r), int(min_overlap), np.int64)
    else:
        theta = Fraction(float(min_overlap))
        if not 0 < theta <= 1:
            raise ValueError(f"detection_counts: min_overlap is a voxel count >= 1 or a fraction in (0, 1], got {min_overlap!r}")
        need = np.array([max(1, math.ceil(theta * int(v))) for v in n], np.int64).reshape(len(r))
    return r, ov >= need


def detection_counts(rows_pred, rows_truth, min_overlap=1):
    """Lesion-wise detection from the table of the prediction (made with other = the labels) and the table of the labels (made with
    other = the prediction), both on the host.  A truth component is DETECTED, and a predicted component is a TRUE POSITIVE, when its
    n_overlap >= max(1, ceil(theta * n)) with theta = min_overlap as a fraction in (0, 1] of its own voxels; min_overlap as an integer
    (the default 1: any overlap) is that many voxels.  This is the any-overlap rule: a component is judged by its overlap with the WHOLE
    class of the other volume.  It is not a one-to-one matching: one large predicted component can detect several truth components, and
    several predicted fragments of one truth component are all true positives.
    -> {'n_pred', 'n_truth' (components that hold rows), 'tp' (predicted components that overlap), 'fp' (those that do not), 'detected',
    'fn' (truth components), 'fp_voxels' (the voxels of the false positives), 'sensitivity' detected / n_truth, 'precision' tp / n_pred,
    'f1' their harmonic mean; a ratio without a denominator is None}"""
    p, hit_p = _detected(rows_pred, min_overlap)
    t, hit_t = _detected(rows_truth, min_overlap)
    tp, detected = int(hit_p.sum()), int(hit_t.sum())
    sens = detected / len(t) if len(t) else None
    prec = tp / len(p) if len(p) else None
    f1 = None if sens is None or prec is None else (2 * sens * prec / (sens + prec) if sens + prec else 0.0)
    return {"n_pred": len(p), "n_truth": len(t), "tp": tp, "fp": len(p) - tp, "detected": detected, "fn": len(t) - detected,
            "fp_voxels": int(p[~hit_p, 0].sum()), "sensitivity": sens, "precision": prec, "f1": f1}


def check_components_out(components_out, K, max_components):
    """the tables a caller hands to the volume segmenter under its components option: (int64 [2, K-1, max_components, 24], int64 [2, K-1, 4]), both
    contiguous: the rows and the head words of the final mask, then of the labels, per foreground class"""
    ok = isinstance(components_out, (tuple, list)) and len(components_out) == 2 and all(torch.is_tensor(t) and t.is_contiguous() for t in components_out)
    if ok:
        rt, ht = components_out
        ok = (rt.dtype == torch.int64 and tuple(rt.shape) == (2, K - 1, max_components, COMP_ROW) and ht.dtype == torch.int64
              and tuple(ht.shape) == (2, K - 1, HEAD_WORDS))
    if not ok:
        raise ValueError(f"components_out must be a pair of contiguous tensors (int64 [2, {K - 1}, {max_components}, {COMP_ROW}], "
                         f"int64 [2, {K - 1}, {HEAD_WORDS}]): the rows and the head words of the final mask and of the labels")


def detection_figures(rows, heads, spacing=None, min_overlap=1):
    """tables [2, K-1, N, 24] and heads [2, K-1, 4] of a volume (prediction, labels) -> per foreground class the dict of
    `detection_counts` with 'components_pred' and 'components_truth' (the true counts C of the heads) and, under a spacing,
    'fp_volume_ml'.  A head with an invalid word says that a volume did not hold what the chain expects: raised here, where the tables
    have crossed to the host anyway."""
    rows, heads = np.asarray(rows), np.asarray(heads)
    if (heads[..., 1] != 0).any() or (heads[..., 3] != 0).any():
        raise RuntimeError("rpnet_compstat: the renumbering or the tally met a value that is no label of its volume (the head's invalid words)")
    figs = []
    for c in range(rows.shape[1]):
        fig = detection_counts(rows[0, c], rows[1, c], min_overlap)
        fig["components_pred"], fig["components_truth"] = int(heads[0, c, 0]), int(heads[1, c, 0])
        fig["fp_volume_ml"] = None if spacing is None else fig["fp_voxels"] * float(spacing[0]) * float(spacing[1]) * float(spacing[2]) / 1000.0
        figs.append(fig)
    return figs


def detection_line_suffix(fig, mm):
    """the fields an item line of a data-set evaluation gains under the components option: the components of the prediction (of the labels), the truth
    components detected, the false-positive components and their volume in voxels or, under a spacing, in mL"""
    vol = f"{fmt(fig['fp_volume_ml'])} mL" if mm else f"{fig['fp_voxels']}"
    return f" comp {fig['components_pred']} ({fig['components_truth']}) det {fig['detected']}/{fig['components_truth']} fp {fig['fp']} fpvol {vol}"


def detection_mean_suffix(figs, mm):
    """the means of those fields over the items (the detected fraction over the items that have a truth component)"""
    key = "fp_volume_ml" if mm else "fp_voxels"
    return (f" comp {np.mean([f['components_pred'] for f in figs]):.2f} ({np.mean([f['components_truth'] for f in figs]):.2f})"
            f" det {fmt(mean_of(figs, 'sensitivity'))} fp {np.mean([f['fp'] for f in figs]):.2f} fpvol {fmt(mean_of([float(f[key]) for f in figs]))}"
            f"{' mL' if mm else ''}")
