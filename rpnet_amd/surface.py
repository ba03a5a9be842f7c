"""Surface distances of an evaluated volume: HD95, HD and ASSD beside the Dice score (csrc/surface.hip, include/rpnet_surface_abi.h).

Definition (the common medpy / MONAI one, in voxel units).  For a binary volume M [D,H,W], border(M) = M & ~erode(M) with the
6-neighbourhood, voxels outside the volume counting as background.  For a prediction A and a truth B, d_AB are the Euclidean distances
from every voxel of border(A) to the nearest voxel of border(B) and d_BA the reverse; HD = max(d_AB u d_BA), HD95 =
np.percentile(hstack(d_AB, d_BA), 95) and ASSD = (mean(d_AB) + mean(d_BA)) / 2; all three are None when either border is empty.

With unit spacing every squared distance is an integer, so the device forms everything but two sums of square roots in integers:
`surface_tally` leaves one int64 row {n_A, n_B, d2_k, d2_k1, d2_max, k} and one fp64 row {sum_A sqrt(d2), sum_B sqrt(d2)} in tables
that stay on the device; `surface_from_rows` turns a pair of rows into the three figures on the host; `surface_reference` restates
the definition in numpy and is what the GPU tests compare with (tests/test_host_surface.py pins it to scipy.ndimage).

Millimetres on a grid with a per-axis voxel spacing, and the normalised surface Dice: rpnet_amd.surface_spacing (a float64 transform
and a radix selection beside this integer path, which stays the yardstick for it at spacing (1, 1, 1)).
"""
import math

import numpy as np
import torch

from . import hip
from ._volume_checks import KINDS, WorkspaceCache, check_table, check_volume, fmt, hd95_from, mean_of, one_device  # noqa: F401  (KINDS, fmt: public)

IROW, FROW = 6, 2           # RPNET_SURFACE_IROW, RPNET_SURFACE_FROW
MAX_DIM = 1024              # RPNET_SURFACE_MAX_DIM
NO_SEED = 1 << 29           # the transform of a volume without a border voxel
_NONE = {"hd95": None, "hd": None, "assd": None}
_workspaces = WorkspaceCache(by_shape=False)


def check_surface_tables(itable, ftable, what="surface_tally"):
    """the two tables of surface rows: a contiguous int64 [n, 6] and a contiguous float64 [n, 2] tensor"""
    check_table(itable, None, IROW, torch.int64, "the integer table", what)
    check_table(ftable, None, FROW, torch.float64, "the sum table", what)
    if itable.shape[0] != ftable.shape[0]:
        raise ValueError(f"{what}: the tables have {itable.shape[0]} and {ftable.shape[0]} rows")


def surface_tally(pred, truth, itable, irow, ftable, frow, cls=1):
    """One `rpnet_surface_tally` on the current stream: the rows of prediction `pred` against `truth` for class `cls` (foreground is
    `value == cls`) into itable[irow] and ftable[frow].  pred, truth: contiguous [D,H,W] GPU tensors of uint8, int32, int64 or float32
    (each its own kind), every extent 1..1024; itable int64 [n,6], ftable float64 [n,2] on the same device.  Launches only: nothing is
    copied or synchronised."""
    hip.require_gpu(pred, truth, itable, ftable)
    check_volume(pred, "pred", "surface_tally")
    check_volume(truth, "truth", "surface_tally")
    if pred.shape != truth.shape:
        raise ValueError(f"surface_tally: pred {tuple(pred.shape)} and truth {tuple(truth.shape)} differ in shape")
    check_surface_tables(itable, ftable)
    one_device("surface_tally", pred, truth, itable, ftable)
    D, H, W = pred.shape
    ws, nbytes = _workspaces.get("rpnet_surface_workspace_bytes", pred.device, (D, H, W))
    hip.call("rpnet_surface_tally", hip.ptr(pred), KINDS[pred.dtype], hip.ptr(truth), KINDS[truth.dtype], int(cls), D, H, W,
             hip.ptr(itable), int(irow), hip.ptr(ftable), int(frow), itable.shape[0], hip.ptr(ws), nbytes)


def surface_from_rows(irow, frow, spacing=1.0):
    """{"hd95", "hd", "assd"} of one pair of rows, on the host; three Nones for the row of an empty border (k = -1).  spacing: ONE
    isotropic factor applied to the final figures."""
    if np.ndim(spacing) != 0:
        raise ValueError("surface_from_rows: spacing is one isotropic factor.  The tally is exact because every squared distance is an "
                         "integer number of voxels; a per-axis spacing would need a transform and a histogram in floating point, and the "
                         "preprocessed _clean.nrrd volumes carry no spacing anyway")
    n_a, n_b, d2_k, d2_k1, d2_max, k = (int(v) for v in irow)
    if k < 0 or n_a == 0 or n_b == 0:
        return dict(_NONE)
    hd95 = hd95_from(d2_k, d2_k1, n_a + n_b, k)
    assd = (float(frow[0]) / n_a + float(frow[1]) / n_b) / 2
    s = float(spacing)
    return {"hd95": hd95 * s, "hd": math.sqrt(d2_max) * s, "assd": assd * s}


def surface_figures(itable, ftable, spacing=1.0):
    """surface_from_rows over the rows of two host tables [..., 6] and [..., 2] -> a flat list"""
    it, ft = np.asarray(itable).reshape(-1, IROW), np.asarray(ftable).reshape(-1, FROW)
    return [surface_from_rows(i, f, spacing) for i, f in zip(it, ft)]


def line_suffix(fewshot, affine):
    """what an item line gains: ` hd95 <fewshot> (<affine>) assd <fewshot> (<affine>)`"""
    return f" hd95 {fmt(fewshot['hd95'])} ({fmt(affine['hd95'])}) assd {fmt(fewshot['assd'])} ({fmt(affine['assd'])})"


def mean_suffix(fewshot, affine):
    """what a class line gains: the same four figures as means over the items where they are not None"""
    return line_suffix({k: mean_of(fewshot, k) for k in ("hd95", "assd")}, {k: mean_of(affine, k) for k in ("hd95", "assd")})


# ------------------------------------------------------------------------------------------------- the numpy restatement
def border_reference(m):
    """M & ~erode(M) of a boolean [D,H,W] array, 6-neighbourhood, outside = background, by shifted arrays"""
    m = np.asarray(m, dtype=bool)
    p = np.pad(m, 1, constant_values=False)
    core = (slice(1, -1),) * 3
    eroded = m.copy()
    for axis in range(3):
        for shift in (-1, 1):
            eroded &= np.roll(p, shift, axis=axis)[core]
    return m & ~eroded


def transform_reference(border):
    """squared Euclidean distance of every voxel to the nearest True voxel of `border`, int64; NO_SEED everywhere when there is none:
    the separable min-plus transform out[i] = min_j (in[j] + (i - j)^2) along x, then y, then z, by brute force"""
    g = np.where(np.asarray(border, dtype=bool), 0, NO_SEED).astype(np.int64)
    for axis in (2, 1, 0):
        L = g.shape[axis]
        g = np.moveaxis(g, axis, -1)
        out = g.copy()
        pos = np.arange(L)
        for j in range(L):
            np.minimum(out, g[..., j:j + 1] + (pos - j) ** 2, out=out)
        g = np.moveaxis(np.minimum(out, NO_SEED), -1, axis)
    return np.ascontiguousarray(g)


def rows_reference(pred, truth, cls=1):
    """the rows `surface_tally` writes, from numpy: (int64 [6], float64 [2]); the sums of square roots by math.fsum"""
    a, b = border_reference(np.asarray(pred) == cls), border_reference(np.asarray(truth) == cls)
    n_a, n_b = int(a.sum()), int(b.sum())
    if n_a == 0 or n_b == 0:
        return np.array([0, 0, 0, 0, 0, -1], dtype=np.int64), np.zeros(2, dtype=np.float64)
    d_ab, d_ba = transform_reference(b)[a], transform_reference(a)[b]
    pooled = np.sort(np.concatenate([d_ab, d_ba]))
    n = n_a + n_b
    k = int(math.floor((n - 1) * 0.95))
    irow = np.array([n_a, n_b, pooled[k], pooled[min(k + 1, n - 1)], pooled[-1], k], dtype=np.int64)

    def root_sum(d2):
        bins, counts = np.unique(d2, return_counts=True)
        return math.fsum(float(c) * math.sqrt(float(v)) for v, c in zip(bins, counts))
    return irow, np.array([root_sum(d_ab), root_sum(d_ba)], dtype=np.float64)


def surface_reference(pred, truth, cls=1):
    """numpy-only restatement of the definition at the top: (irow, frow, {"hd95", "hd", "assd"}) of `pred` against `truth` (arrays
    [D,H,W] of any dtype) for class `cls`"""
    irow, frow = rows_reference(pred, truth, cls)
    return irow, frow, surface_from_rows(irow, frow)
