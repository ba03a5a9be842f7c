"""Surface distances of an evaluated volume in millimetres: HD95, HD, ASSD and the normalised surface Dice (NSD) on a grid with a
per-axis voxel spacing (csrc/surface_spacing.hip, include/rpnet_surface_spacing_abi.h).

Definition: that of rpnet_amd.surface (6-neighbourhood border, outside = background, distances pooled over border(A) -> border(B) and
back), with the distance between two voxels sqrt(sz^2 dz^2 + sy^2 dy^2 + sx^2 dx^2) for a spacing (sz, sy, sx) given in the order of
the tensor's axes [D, H, W].  NSD at a tolerance tau is the fraction of the pooled border voxels within tau of the other border.

The squared distances are no longer integers.  The weights w = s * s are formed once, here, in float64; the device evaluates
((wx dx^2 + wy dy^2) + wz dz^2) with every product and every sum rounded separately and minimises it over the border voxels, so
`transform_reference_spacing`, which performs the same operations in numpy, gets the same bits.  `surface_tally_spacing` leaves one int64
row {n_A, n_B, k, within_A, within_B} and one fp64 row {d2_k, d2_k1, d2_max, sum_A sqrt(d2), sum_B sqrt(d2)} in tables that stay on the
device; `figures_from_rows` turns a pair of rows into the four figures on the host; `rows_reference_spacing` restates the rows in
numpy and is what the GPU tests compare with (tests/test_host_surface_spacing.py pins it to scipy.ndimage).

Out of scope: an oblique grid is measured by the norms of its axis vectors only (`spacing_from_header`), and nothing is resampled here
(rpnet_amd.resample takes a volume to another spacing).
"""
import ctypes
import math
import re

import numpy as np
import torch

from . import hip
from ._volume_checks import KINDS, WorkspaceCache, check_table, check_volume, fmt, hd95_from, mean_of, one_device
from .surface import MAX_DIM, border_reference  # noqa: F401  MAX_DIM: the extent limit is that of the integer path

IROW, FROW = 5, 5           # RPNET_SURFACE_SPACING_IROW, RPNET_SURFACE_SPACING_FROW
NO_SEED = float(np.finfo(np.float64).max)       # the transform of a volume without a border voxel (DBL_MAX)
_NONE = {"hd95": None, "hd": None, "assd": None, "nsd": None}
_workspaces = WorkspaceCache(by_shape=False)


def check_spacing(spacing, what="surface_tally_spacing"):
    """a spacing as a tuple of three floats; ValueError unless it is three finite positive numbers"""
    try:
        s = tuple(float(v) for v in spacing)
    except (TypeError, ValueError):
        s = ()
    if len(s) != 3 or not all(math.isfinite(v) and v > 0 for v in s):
        raise ValueError(f"{what}: spacing must be three finite positive numbers (sz, sy, sx) in the order of the axes [D, H, W], got {spacing!r}")
    return s


def spacing_weights(spacing):
    """w = s * s in float64: the three doubles both the kernel and the restatement use"""
    return tuple(s * s for s in check_spacing(spacing))


def tolerance_squared(tau):
    """tau^2 as the one double the stored squared distances are compared with; -1.0 ("not asked") for None or a negative tau"""
    if tau is None or tau < 0:
        return -1.0
    return float(tau) * float(tau)


def check_spacing_tables(itable, ftable, what="surface_tally_spacing"):
    """the two tables of spacing rows: a contiguous int64 [n, 5] and a contiguous float64 [n, 5] tensor"""
    check_table(itable, None, IROW, torch.int64, "the integer table", what, " (the widths under a spacing)")
    check_table(ftable, None, FROW, torch.float64, "the float table", what, " (the widths under a spacing)")
    if itable.shape[0] != ftable.shape[0]:
        raise ValueError(f"{what}: the tables have {itable.shape[0]} and {ftable.shape[0]} rows")


def surface_tally_spacing(pred, truth, spacing, itable, irow, ftable, frow, cls=1, tau=None):
    """One `rpnet_surface_spacing_tally` on the current stream: the rows of prediction `pred` against `truth` for class `cls` under the
    spacing (sz, sy, sx) into itable[irow] and ftable[frow].  pred, truth: as for rpnet_amd.surface.surface_tally; itable int64 [n,5],
    ftable float64 [n,5] on the same device; tau: the NSD tolerance in the unit of the spacing, None for none.  Launches only: nothing is
    copied or synchronised."""
    hip.require_gpu(pred, truth, itable, ftable)
    check_volume(pred, "pred", "surface_tally_spacing")
    check_volume(truth, "truth", "surface_tally_spacing")
    if pred.shape != truth.shape:
        raise ValueError(f"surface_tally_spacing: pred {tuple(pred.shape)} and truth {tuple(truth.shape)} differ in shape")
    check_spacing_tables(itable, ftable)
    one_device("surface_tally_spacing", pred, truth, itable, ftable)
    w = (ctypes.c_double * 3)(*spacing_weights(spacing))
    if tau is not None and math.isnan(tau):
        raise ValueError("surface_tally_spacing: tau is NaN")
    D, H, W = pred.shape
    ws, nbytes = _workspaces.get("rpnet_surface_spacing_workspace_bytes", pred.device, (D, H, W))
    hip.call("rpnet_surface_spacing_tally", hip.ptr(pred), KINDS[pred.dtype], hip.ptr(truth), KINDS[truth.dtype], int(cls), D, H, W, w,
             tolerance_squared(tau), hip.ptr(itable), int(irow), hip.ptr(ftable), int(frow), itable.shape[0], hip.ptr(ws), nbytes)


def figures_from_rows(irow, frow, tau=None):
    """{"hd95", "hd", "assd", "nsd"} of one pair of rows, on the host, in the unit of the spacing; the first three are None for the row
    of an empty border (k = -1).  tau: the tolerance the tally was made with; "nsd" is None when none was asked (None or negative: both
    `within` columns are then 0, which the rows alone cannot tell from a tolerance that nothing met)"""
    n_a, n_b, k, within_a, within_b = (int(v) for v in irow)
    if k < 0 or n_a == 0 or n_b == 0:
        return dict(_NONE)
    d2_k, d2_k1, d2_max, sum_a, sum_b = (float(v) for v in frow)
    n = n_a + n_b
    hd95 = hd95_from(d2_k, d2_k1, n, k)
    nsd = (within_a + within_b) / n if tolerance_squared(tau) >= 0 else None
    return {"hd95": hd95, "hd": math.sqrt(d2_max), "assd": (sum_a / n_a + sum_b / n_b) / 2, "nsd": nsd}


def spacing_figures(itable, ftable, tau=None):
    """figures_from_rows over the rows of two host tables [..., 5] and [..., 5] -> a flat list"""
    it, ft = np.asarray(itable).reshape(-1, IROW), np.asarray(ftable).reshape(-1, FROW)
    return [figures_from_rows(i, f, tau) for i, f in zip(it, ft)]


def line_suffix_mm(fewshot, affine, nsd):
    """what an item line gains under a spacing: the fields of rpnet_amd.surface.line_suffix, each followed by `mm`, and with a tolerance
    ` nsd <fewshot> (<affine>)`"""
    def mm(v):
        return fmt(v) + ("mm" if v is not None else "")
    line = f" hd95 {mm(fewshot['hd95'])} ({mm(affine['hd95'])}) assd {mm(fewshot['assd'])} ({mm(affine['assd'])})"
    return line + (f" nsd {fmt(fewshot['nsd'])} ({fmt(affine['nsd'])})" if nsd else "")


def mean_suffix_mm(fewshot, affine, nsd):
    """what a class line gains: the same figures as means over the items where they are not None"""
    keys = ("hd95", "assd", "nsd")
    return line_suffix_mm({k: mean_of(fewshot, k) for k in keys}, {k: mean_of(affine, k) for k in keys}, nsd)


# ------------------------------------------------------------------------------------------------- the numpy restatement
def transform_reference_spacing(border, w):
    """weighted squared distance of every voxel to the nearest True voxel of `border`, float64, with the kernel's operations: along x
    w[2] * o^2 for the nearest border voxel of the line (NO_SEED without one), then out[i] = min_j (in[j] + w * (i - j)^2) along y
    (w[1]) and z (w[0]), product and sum rounded separately, by brute force; NO_SEED everywhere when there is no border voxel"""
    border = np.asarray(border, dtype=bool)
    g = np.full(border.shape, NO_SEED, dtype=np.float64)
    pos = np.arange(border.shape[2])
    for j in range(border.shape[2]):
        cand = np.where(border[..., j:j + 1], np.float64(w[2]) * ((pos - j) ** 2).astype(np.float64), NO_SEED)
        np.minimum(g, cand, out=g)
    with np.errstate(over="ignore"):
        for axis in (1, 0):
            L = g.shape[axis]
            g = np.moveaxis(g, axis, -1)
            out = g.copy()
            pos = np.arange(L)
            for j in range(L):
                prod = np.float64(w[axis]) * ((pos - j) ** 2).astype(np.float64)
                np.minimum(out, g[..., j:j + 1] + prod, out=out)
            g = np.moveaxis(np.minimum(out, NO_SEED), -1, axis)
    return np.ascontiguousarray(g)


def rows_reference_spacing(pred, truth, spacing, cls=1, tau=None):
    """the rows `surface_tally_spacing` writes, from numpy: (int64 [5], float64 [5]); the sums of square roots by math.fsum"""
    w = spacing_weights(spacing)
    a, b = border_reference(np.asarray(pred) == cls), border_reference(np.asarray(truth) == cls)
    n_a, n_b = int(a.sum()), int(b.sum())
    if n_a == 0 or n_b == 0:
        return np.array([0, 0, -1, 0, 0], dtype=np.int64), np.zeros(FROW, dtype=np.float64)
    d_ab, d_ba = transform_reference_spacing(b, w)[a], transform_reference_spacing(a, w)[b]
    pooled = np.sort(np.concatenate([d_ab, d_ba]))
    n = n_a + n_b
    k = int(math.floor((n - 1) * 0.95))
    tau2 = tolerance_squared(tau)
    irow = np.array([n_a, n_b, k, int((d_ab <= tau2).sum()), int((d_ba <= tau2).sum())], dtype=np.int64)
    frow = np.array([pooled[k], pooled[min(k + 1, n - 1)], pooled[-1], math.fsum(np.sqrt(d_ab).tolist()), math.fsum(np.sqrt(d_ba).tolist())],
                    dtype=np.float64)
    return irow, frow


def surface_reference_spacing(pred, truth, spacing, cls=1, tau=None):
    """numpy-only restatement: (irow, frow, {"hd95", "hd", "assd", "nsd"}) of `pred` against `truth` (arrays [D,H,W] of any dtype) for
    class `cls` under the spacing (sz, sy, sx)"""
    irow, frow = rows_reference_spacing(pred, truth, spacing, cls, tau)
    return irow, frow, figures_from_rows(irow, frow, tau)


# ------------------------------------------------------------------------------------------------- the spacing of an NRRD header
def _vector_numbers(vector):
    return [float(v) for v in str(vector).strip().strip("()").split(",")]


def spacing_from_header(header):
    """(s0, s1, s2) of the three spatial axes of an NRRD header in the array's axis order: the norms of the `space directions` vectors,
    else `spacings`; axes marked `none` and `nan` entries are non-spatial and are skipped.  ValueError, naming the fields, when neither
    gives three finite positive numbers: there is no silent fall-back to voxels."""
    found = []
    directions = header.get("space directions")
    if directions is not None:
        vectors = re.findall(r"none|\([^)]*\)", directions, flags=re.I) if isinstance(directions, str) else directions
        norms = []
        for v in vectors:
            if v is None or (isinstance(v, str) and v.strip().lower() == "none"):
                continue
            vals = _vector_numbers(v) if isinstance(v, str) else [float(x) for x in np.asarray(v, dtype=np.float64).ravel()]
            if any(math.isnan(x) for x in vals):
                continue
            norms.append(math.sqrt(math.fsum(x * x for x in vals)))
        found.append(("space directions", norms))
    spacings = header.get("spacings")
    if spacings is not None:
        vals = [float(v) for v in (spacings.split() if isinstance(spacings, str) else np.asarray(spacings, dtype=np.float64).ravel())]
        found.append(("spacings", [v for v in vals if not math.isnan(v)]))
    for _, vals in found:
        if len(vals) == 3 and all(math.isfinite(v) and v > 0 for v in vals):
            return tuple(vals)
    seen = "; ".join(f"`{name}` gives {vals}" for name, vals in found) or "neither field is present"
    raise ValueError("spacing_from_header: the header must carry three positive spacings in `space directions` (vector norms) or in "
                     f"`spacings`: {seen}")
