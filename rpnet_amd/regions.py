"""Region statistics of a segmented volume on the device (csrc/regions.hip, include/rpnet_region_abi.h): per label, from ONE pass over the
label volume and an image, the voxel count, the bounding box, the first and second coordinate moments (all exact integers) and the
float64 sums S1 = SUM v, S2 = SUM v * v, the extrema and the count of the finite image values inside the label.  What a user of an organ
segmenter asks first follows on the host from those two small tables (`derive`): volume, centroid, extent, principal axes, mean and
standard deviation of the intensity; and from two of them (`compare`) the relative volume difference and the centroid distance of a
prediction against the labels.

A row of the integer table is int64 [20]: n | min z y x | max z y x | sum z y x | sum zz yy xx | sum zy zx yx | n_finite | the smallest
and the largest order-preserving key of the float32 pattern (rpnet_volload_abi.h) | 0.  An empty label holds min = (D, H, W), max = -1,
keys 0xFFFFFFFF and 0.  A row of the float table is float64 [2]: S1, S2, summed in the fixed order the header states (a lane of 16
voxels, a tree over the 256 lanes of a chunk of 4096, the chunks of a block in ascending order, the blocks by the SUM of
rpnet_fusion_abi.h), so that two runs, and the numpy restatement of tests/regions_cases.py, give the same bits.  Integer atomics only.

Limits: dense labels 0 .. L-1 with L <= 256 (the sparse labels of rpnet_amd.components.label would first need a renumbering); no order
statistics of the intensity; no surface area; a spacing per axis; extents up to 1024.
"""
import math

import numpy as np
import torch

from . import hip
from ._volume_checks import KINDS, WorkspaceCache, check_volume, fmt, mean_of, one_device

MAX_LABELS = 256                     # RPNET_REGION_MAX_LABELS
IROW, FROW = 20, 2                   # RPNET_REGION_IROW, RPNET_REGION_FROW
CHUNK, MAX_BLOCKS = 4096, 1024       # RPNET_REGION_CHUNK, RPNET_REGION_MAX_BLOCKS
HEAD_BYTES, OUTSIDE_OFFSET = 64, 0   # RPNET_REGION_HEAD_BYTES, RPNET_REGION_OUTSIDE_OFFSET
MAX_DIM = 1024                       # RPNET_CC_MAX_DIM
IMAGE_KINDS = {torch.float32: 0, torch.int16: 1}        # RPNET_PREP_F32, RPNET_PREP_I16
_workspaces = WorkspaceCache(by_shape=True)


def _region_workspace_layout(D, H, W, L):
    """byte offsets of (the accumulators int64 [L, 20], the partials float64 [G, L, 2]) inside the workspace of a call, and its size"""
    G = min((D * H * W + CHUNK - 1) // CHUNK, MAX_BLOCKS)
    return (HEAD_BYTES, HEAD_BYTES + 8 * IROW * L), HEAD_BYTES + 8 * IROW * L + 16 * G * L


_workspace_layout = _region_workspace_layout


def region_workspace(shape, n_labels, device):
    """the workspace `region_stats` keeps for volumes of `shape` with `n_labels` labels on `device` (made on first use)"""
    D, H, W = (int(s) for s in shape)
    return _workspaces.get("rpnet_region_workspace_bytes", torch.device(device), (D, H, W, int(n_labels)))[0]


def region_outside(workspace):
    """n_outside of the last call that used `workspace`: an int64 device scalar, a view of the workspace's head"""
    return workspace[OUTSIDE_OFFSET:OUTSIDE_OFFSET + 8].view(torch.int64)[0]


def check_region_labels(fn, labels, n_labels, skip_background):
    """-> (lo, L) of a call; ValueError for what the C side refuses too"""
    if not torch.is_tensor(labels):
        raise ValueError(f"{fn}: labels must be a tensor")
    check_volume(labels, "labels", fn)
    if any(not 1 <= int(s) <= MAX_DIM for s in labels.shape):
        raise ValueError(f"{fn}: labels are {tuple(labels.shape)}; every extent is 1..{MAX_DIM}")
    if n_labels is None:
        if labels.dtype != torch.uint8:
            raise ValueError(f"{fn}: n_labels is needed for {labels.dtype} labels (only a uint8 volume has a range known without reading it)")
        n_labels = MAX_LABELS
    if isinstance(n_labels, bool) or not isinstance(n_labels, (int, np.integer)) or not 1 <= int(n_labels) <= MAX_LABELS:
        raise ValueError(f"{fn}: n_labels is an integer 1..{MAX_LABELS}, got {n_labels!r}")
    return (1 if skip_background else 0), int(n_labels)


def region_stats(labels, image=None, n_labels=None, skip_background=True, out=None, row=0, workspace=None):
    """One `rpnet_region_stats` call on the current stream -> (rows_i int64 [L, 20], rows_f float64 [L, 2]) on the device, row l of label l.
    labels: a contiguous [D,H,W] volume (uint8, int32, int64 or float32) of labels 0 .. L-1 with L = n_labels (None: 256 for uint8
    labels); a voxel that holds anything else enters no row and is counted in n_outside (`region_outside(region_workspace(shape, L,
    device))`, or of the workspace handed in).  skip_background: label 0 is not tallied and its row is an empty row.  image: None, or a
    contiguous float32 or int16 volume of the same shape; without one the intensity columns are those of an empty row and rows_f is
    zero.  out: (rows_i int64 [n, L, 20], rows_f float64 [n, L, 2] or None without an image) to write row `row` of, returned as they
    are.  workspace: a uint8 tensor of at least rpnet_region_workspace_bytes, 16-byte aligned, instead of the cached one.
    The rows are WRITTEN, not added to.  Launches only: nothing is copied or synchronised.  CPU tensors raise: there is no host route."""
    fn = "region_stats"
    lo, L = check_region_labels(fn, labels, n_labels, skip_background)
    shape = labels.shape
    if image is not None:
        if not torch.is_tensor(image) or image.dtype not in IMAGE_KINDS:
            raise ValueError(f"{fn}: image must be a float32 or int16 tensor")
        if image.shape != shape or not image.is_contiguous():
            raise ValueError(f"{fn}: image must be a contiguous tensor of the labels' shape {tuple(shape)}, got {tuple(image.shape)}")
    if isinstance(row, bool) or not isinstance(row, (int, np.integer)):
        raise ValueError(f"{fn}: row is an integer, got {row!r}")
    if out is not None:
        ok = isinstance(out, (tuple, list)) and len(out) == 2 and torch.is_tensor(out[0]) and (torch.is_tensor(out[1]) or (out[1] is None and image is None))
        if ok:
            ri, rf = out
            ok = ri.dtype == torch.int64 and ri.dim() == 3 and tuple(ri.shape[1:]) == (L, IROW) and ri.is_contiguous()
            ok = ok and (rf is None or (rf.dtype == torch.float64 and tuple(rf.shape) == (ri.shape[0], L, FROW) and rf.is_contiguous()))
        if not ok:
            raise ValueError(f"{fn}: out must be (a contiguous int64 [n, {L}, {IROW}] tensor, a contiguous float64 [n, {L}, {FROW}] tensor"
                             " or None without an image)")
        if not 0 <= int(row) < ri.shape[0]:
            raise ValueError(f"{fn}: row {row} of tables of {ri.shape[0]} rows")
    elif int(row) != 0:
        raise ValueError(f"{fn}: row {row} needs out=")
    if workspace is not None:
        need = _region_workspace_layout(*(int(s) for s in shape), L)[1]
        if not torch.is_tensor(workspace) or workspace.dtype != torch.uint8 or workspace.dim() != 1 or not workspace.is_contiguous():
            raise ValueError(f"{fn}: workspace must be a contiguous 1-d uint8 tensor")
        if workspace.numel() < need:
            raise ValueError(f"{fn}: workspace of {workspace.numel()} bytes, {need} needed")
    hip.require_gpu(labels, image, workspace, *(out or ()))
    one_device(fn, labels, image, workspace, *(out or ()))
    if workspace is not None and workspace.data_ptr() % 16:
        raise ValueError(f"{fn}: workspace must be aligned to 16 bytes")
    D, H, W = (int(s) for s in shape)
    dev = labels.device
    if out is None:
        ri = torch.empty((1, L, IROW), device=dev, dtype=torch.int64)
        rf = torch.empty((1, L, FROW), device=dev, dtype=torch.float64)
    if workspace is None:
        workspace, nbytes = _workspaces.get("rpnet_region_workspace_bytes", dev, (D, H, W, L))
    else:
        nbytes = workspace.numel()
    hip.call("rpnet_region_stats", hip.ptr(labels), KINDS[labels.dtype], hip.ptr(image), IMAGE_KINDS[image.dtype] if image is not None else 0,
             D, H, W, lo, L, hip.ptr(ri), hip.ptr(rf), int(row), ri.shape[0], hip.ptr(workspace), nbytes)
    return (ri[0], rf[0]) if out is None else (ri, rf)


def key_to_float(keys):
    """the float32 values of order-preserving keys (rpnet_volload_abi.h): a set top bit is a value >= 0, a clear one the complement of a
    negative value's pattern"""
    k = np.asarray(keys).astype(np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def derive(rows_i, rows_f=None, spacing=None):
    """The figures of every label from the tables of `region_stats`, once they have crossed to the host (numpy, float64):
    rows_i int64 [L, 20], rows_f float64 [L, 2] or None (no image), spacing None or (sz, sy, sx) -> a list of L dicts with
      voxels        n
      bbox          ((z0, y0, x0), (z1, y1, x1)), inclusive
      centroid      (z, y, x) in voxels
      volume_mm3, volume_ml, centroid_mm (index x spacing), extent_mm (of the box), covariance_mm2 (3x3, population, from the integer
      moments), axes_mm (the square roots of its eigenvalues, ascending: the standard deviations along the principal axes)
      mean, std (population), min, max of the finite image values inside the label, n_nonfinite
    A figure that does not exist is None: those of an empty label, the millimetre figures without a spacing, the intensity figures
    without an image, mean .. max of a label without a finite voxel."""
    ri = np.asarray(rows_i)
    if ri.ndim != 2 or ri.shape[1] != IROW:
        raise ValueError(f"derive: rows_i must be [L, {IROW}], got {ri.shape}")
    rf = None if rows_f is None else np.asarray(rows_f, np.float64)
    if rf is not None and rf.shape != (ri.shape[0], FROW):
        raise ValueError(f"derive: rows_f must be [{ri.shape[0]}, {FROW}], got {rf.shape}")
    if spacing is not None:
        from .surface_spacing import check_spacing
        spacing = check_spacing(spacing, "derive")
    out = []
    for l in range(ri.shape[0]):
        r = [int(v) for v in ri[l]]
        n = r[0]
        fig = dict(voxels=n, bbox=None, centroid=None, volume_mm3=None, volume_ml=None, centroid_mm=None, extent_mm=None, covariance_mm2=None,
                   axes_mm=None, mean=None, std=None, min=None, max=None, n_nonfinite=None)
        if spacing is not None:
            fig["volume_mm3"] = n * spacing[0] * spacing[1] * spacing[2]
            fig["volume_ml"] = fig["volume_mm3"] / 1000.0
        if n:
            fig["bbox"] = (tuple(r[1:4]), tuple(r[4:7]))
            fig["centroid"] = tuple(r[7 + a] / n for a in range(3))
            if spacing is not None:
                fig["centroid_mm"] = tuple(fig["centroid"][a] * spacing[a] for a in range(3))
                fig["extent_mm"] = tuple((r[4 + a] - r[1 + a] + 1) * spacing[a] for a in range(3))
                second = {(0, 0): r[10], (1, 1): r[11], (2, 2): r[12], (0, 1): r[13], (0, 2): r[14], (1, 2): r[15]}
                cov = np.zeros((3, 3), np.float64)
                for (a, b), sab in second.items():
                    # n * sum ab - sum a * sum b is an exact integer: the cancellation happens before anything is rounded
                    cov[a, b] = cov[b, a] = (n * sab - r[7 + a] * r[7 + b]) / (n * n) * (spacing[a] * spacing[b])
                fig["covariance_mm2"] = cov
                fig["axes_mm"] = tuple(float(math.sqrt(max(v, 0.0))) for v in np.linalg.eigvalsh(cov))
        if rf is not None:
            nf = r[16]
            fig["n_nonfinite"] = n - nf
            if nf:
                mean = float(rf[l, 0]) / nf
                fig["mean"] = mean
                fig["std"] = math.sqrt(max(float(rf[l, 1]) / nf - mean * mean, 0.0))
                lo_hi = key_to_float([r[17], r[18]])
                fig["min"], fig["max"] = float(lo_hi[0]), float(lo_hi[1])
        out.append(fig)
    return out


def compare(pred, truth):
    """The two figures that stand beside Dice in an evaluation, from one label's `derive` dict of the prediction and of the labels ->
    {'rvd': (V_pred - V_truth) / V_truth (None where the truth is empty), 'centroid_distance': the Euclidean distance of the centroids,
    in millimetres where both were derived under a spacing, else in voxels (None where either is empty), 'unit': 'mm' or 'voxels'}"""
    vt, vp = truth["voxels"], pred["voxels"]
    mm = pred["centroid_mm"] is not None and truth["centroid_mm"] is not None
    a, b = (pred["centroid_mm"], truth["centroid_mm"]) if mm else (pred["centroid"], truth["centroid"])
    both_mm = pred["volume_mm3"] is not None and truth["volume_mm3"] is not None
    dist = None if a is None or b is None else math.sqrt(sum((a[k] - b[k]) ** 2 for k in range(3)))
    return {"rvd": (vp - vt) / vt if vt else None, "centroid_distance": dist, "unit": "mm" if (mm or both_mm) else "voxels"}


def check_regions_out(regions_out, K):
    """the tables a caller hands to VolumeSegmenter(regions=True): (int64 [2, K, 20], float64 [2, K, 2]), both contiguous: the rows of
    the final mask, then of the labels, per label 0 .. K-1"""
    ok = isinstance(regions_out, (tuple, list)) and len(regions_out) == 2 and all(torch.is_tensor(t) and t.is_contiguous() for t in regions_out)
    if ok:
        it, ft = regions_out
        ok = it.dtype == torch.int64 and tuple(it.shape) == (2, K, IROW) and ft.dtype == torch.float64 and tuple(ft.shape) == (2, K, FROW)
    if not ok:
        raise ValueError(f"regions_out must be a pair of contiguous tensors (int64 [2, {K}, {IROW}], float64 [2, {K}, {FROW}]): "
                         "the rows of the final mask and of the labels")


def region_figures(rows_i, rows_f, spacing=None):
    """tables [2, K, .] of a volume (prediction, labels) -> per foreground class {'pred', 'truth': the `derive` dicts, and the figures of
    `compare`}"""
    p, t = derive(rows_i[0], rows_f[0], spacing), derive(rows_i[1], rows_f[1], spacing)
    return [dict(compare(p[c], t[c]), pred=p[c], truth=t[c]) for c in range(1, len(p))]


def _volume_of(fig, mm):
    return fig["volume_ml"] if mm else fig["voxels"]


def region_line_suffix(fig, mm):
    """the fields an item line of evaluate_dataset(regions=True) gains: the volume of the prediction (of the labels), in voxels or, under
    a spacing, in ml; the relative volume difference; the centroid distance in voxels or mm"""
    vp, vt = _volume_of(fig["pred"], mm), _volume_of(fig["truth"], mm)
    if mm:
        return f" vol {fmt(vp)} ({fmt(vt)}) ml rvd {fmt(fig['rvd'])} cdist {fmt(fig['centroid_distance'])} mm"
    return f" vol {vp} ({vt}) rvd {fmt(fig['rvd'])} cdist {fmt(fig['centroid_distance'])}"


def region_mean_suffix(figs, mm):
    """the means of those fields over the items where the figure is not None"""
    vp = mean_of([float(_volume_of(f["pred"], mm)) for f in figs])
    vt = mean_of([float(_volume_of(f["truth"], mm)) for f in figs])
    return (f" vol {fmt(vp)} ({fmt(vt)}){' ml' if mm else ''} rvd {fmt(mean_of(figs, 'rvd'))} cdist {fmt(mean_of(figs, 'centroid_distance'))}"
            f"{' mm' if mm else ''}")
