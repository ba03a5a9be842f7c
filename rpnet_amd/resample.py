"""Resampling of a volume or a label map to another grid on the device (csrc/resample.hip, include/rpnet_resample_abi.h): the
`resample(image, spacing, new_spacing)` stage of the reference's utils/preprocess_abd_110.py, which that script calls on the image and on
every structure (followed by `> 0.5` on the structures) and imports from a module the reference does not ship.  The definition is therefore
this project's own, pinned to scipy.ndimage.zoom by tests/test_host_resample.py; parity with the missing module is not claimed.
tools/preprocess_volumes.py --resample is the driver.

Definitions (word for word those of include/rpnet_resample_abi.h; tests/resample_cases.py restates them in numpy, bit for bit).  An image
is [D,H,W] float32 or int16, a label map uint8; every axis length, input and output, is 1..1024.  fl(.) is one float64 rounding.

Coordinates, for output index o on an axis of input length n and output length m.  align "corner": c = fl((o (n - 1)) / (m - 1)), and
c = 0 when m == 1 (scipy's zoom(grid_mode=False)).  align "center": c = fl(fl(((2o + 1) n) / (2m)) - 0.5), clamped to [0, n - 1]
(grid_mode=True, mode='nearest'; torch's align_corners=False).  i0 = min(floor(c), n - 1), i1 = min(i0 + 1, n - 1), t = c - i0.
Linear: lerp(a, b, t) = a when t == 0 (a tap of weight zero is not used: an identity resample is bit-exact and a non-finite neighbour
does not leak), otherwise fl(a + fl(t * fl(b - a))); four lerps along x, then two along y, then one along z, on the voxels widened to
float64; one conversion to the output kind (float32 rounds to nearest; int16 rounds half to even and saturates).
Nearest: i = clamp(floor(fl(c + 0.5)), 0, n - 1) per axis.
Labels, nearest: the label at the nearest voxel.  Labels, linear, one class per call: the linear rule on the indicator (v == cls); the
voxel is of the class when the result is > 0.5 (exactly 0.5 is not); the first class writes cls or 0, every further class takes only the
voxels that hold 0 (merge).  The statistics row of a class: int64 {voxels_in, voxels_out, out_voxels_total, 0}.

Anti-aliasing (`antialias=True` of resample_image and resample_to_spacing): the image is first smoothed by rpnet_amd.smooth with the sigmas
of smooth.antialias_sigma (an axis that shrinks from n to m voxels: (n / m - 1) / 2 voxels; this project's own rule) under the border
"nearest", the border the coordinate clamp above implies, and the smoothed copy is resampled.  Label maps keep the indicator rule.

Not done: no oblique grids, no spline order above 1.
"""
import numpy as np
import torch

from . import hip, smooth
from ._volume_checks import WorkspaceCache, check_table, one_device
from .surface_spacing import check_spacing

IMAGE_KINDS = {torch.float32: 0, torch.int16: 1}    # RPNET_PREP_F32, RPNET_PREP_I16
ALIGNS = {"corner": 0, "center": 1}                 # RPNET_RESAMPLE_CORNER, RPNET_RESAMPLE_CENTER
NEAREST, LINEAR = 0, 1                              # RPNET_RESAMPLE_NEAREST, RPNET_RESAMPLE_LINEAR
MODES = {"nearest": NEAREST, "linear": LINEAR}
STATS_ROW = 4                                       # RPNET_RESAMPLE_STATS_ROW
MAX_DIM = 1024                                      # RPNET_CC_MAX_DIM
RUN = {torch.float32: 4, torch.int16: 8, torch.uint8: 16}      # output x positions of a lane: 16 bytes
_workspaces = WorkspaceCache(by_shape=False)
_smoothed = {}                                      # (device, dtype) -> the flat intermediate an anti-aliased resample smooths into


def check_grid(shape, fn, what="shape"):
    """a grid as a tuple of three ints, each 1..1024"""
    try:
        s = tuple(int(v) for v in shape)
        whole = all(int(v) == v for v in shape)
    except (TypeError, ValueError):
        s, whole = (), False
    if len(s) != 3 or not whole or not all(1 <= v <= MAX_DIM for v in s):
        raise ValueError(f"{fn}: {what} must be three axis lengths (D, H, W), each 1..{MAX_DIM}, got {shape!r}")
    return s


def check_align(align, fn):
    if align not in ALIGNS:
        raise ValueError(f"{fn}: align must be 'corner' or 'center', got {align!r}")
    return ALIGNS[align]


def output_shape(shape, spacing, new_spacing):
    """the grid a volume of `shape` and `spacing` has at `new_spacing`: max(1, round-half-even(n * s / s')) per axis (np.round, as the
    common `resample` helper forms it)"""
    s, t = check_spacing(spacing, "output_shape"), check_spacing(new_spacing, "output_shape")
    return tuple(max(1, int(np.round(int(n) * a / b))) for n, a, b in zip(shape, s, t))


def out_spacing(shape, new_shape, spacing, align="corner"):
    """the spacing of the resampled grid: s * n / m under "center" (the extent n * s is kept), s * (n - 1) / (m - 1) under "corner" (the
    first and the last voxel centres are kept); under "corner" an output axis of length 1 keeps its own spacing, and an axis whose
    length does not change keeps its spacing to the bit under both"""
    check_align(align, "out_spacing")
    s = check_spacing(spacing, "out_spacing")
    if align == "center":
        return tuple(a if int(m) == int(n) else a * int(n) / int(m) for a, n, m in zip(s, shape, new_shape))
    return tuple(a if int(m) in (1, int(n)) else a * (int(n) - 1) / (int(m) - 1) for a, n, m in zip(s, shape, new_shape))


def _resample_volume_check(t, dtypes, what, fn):
    if not torch.is_tensor(t) or t.dtype not in dtypes:
        names = " and ".join(str(d)[6:] for d in dtypes)
        raise ValueError(f"{fn}: {what} is {getattr(t, 'dtype', type(t))}; {names} volumes are accepted")
    if t.dim() != 3 or not t.is_contiguous():
        raise ValueError(f"{fn}: {what} must be a contiguous [D,H,W] tensor, got {tuple(t.shape)}")
    check_grid(t.shape, fn, f"the shape of {what}")


def _resample_out(out, vol, shape, fn):
    if out is None:
        return torch.empty(shape, device=vol.device, dtype=vol.dtype)
    if not torch.is_tensor(out) or out.dtype != vol.dtype or tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError(f"{fn}: out must be a contiguous {str(vol.dtype)[6:]} tensor of shape {shape}")
    return out


def _antialiased(vol, shape):
    """`vol` smoothed for a resample to `shape` into the cached intermediate of its kind; `vol` itself where no axis shrinks.  The
    intermediate is one buffer per device and kind, grown on demand (as the workspaces are: a captured graph holds the one it was
    captured with, so capture after the largest volume has been seen)."""
    sigma = smooth.antialias_sigma(vol.shape, shape)
    if not any(sigma):
        return vol
    key = (vol.device, vol.dtype)
    if key not in _smoothed or _smoothed[key].numel() < vol.numel():
        _smoothed[key] = torch.empty(vol.numel(), device=vol.device, dtype=vol.dtype)
    return smooth.smooth_image(vol, sigma, mode="nearest", out=_smoothed[key][:vol.numel()].view(vol.shape))


def resample_image(vol, shape, order=1, align="corner", out=None, antialias=False):
    """`vol` (float32 or int16 [D,H,W]) on the grid `shape`, one `rpnet_resample_image` call on the current stream -> out, of the kind of
    `vol`.  order: 1 trilinear, 0 nearest neighbour.  align: "corner" or "center" (the definitions above).  antialias: smooth the axes
    that shrink first (one more call, into an intermediate that stays allocated).  Launches only: nothing is copied or synchronised."""
    fn = "resample_image"
    hip.require_gpu(vol, out)
    _resample_volume_check(vol, IMAGE_KINDS, "vol", fn)
    shape = check_grid(shape, fn)
    if order not in (0, 1) or isinstance(order, bool):
        raise ValueError(f"{fn}: order must be 0 (nearest) or 1 (linear), got {order!r}")
    a = check_align(align, fn)
    out = _resample_out(out, vol, shape, fn)
    one_device(fn, vol, out, what="the volumes")
    if antialias:
        vol = _antialiased(vol, shape)
    dims = tuple(vol.shape) + shape
    ws, nbytes = _workspaces.get("rpnet_resample_workspace_bytes", vol.device, dims)
    hip.call("rpnet_resample_image", hip.ptr(vol), IMAGE_KINDS[vol.dtype], *dims[:3], hip.ptr(out), *shape, a, int(order), hip.ptr(ws), nbytes)
    return out


def resample_labels(mask, shape, classes=None, mode="nearest", align="corner", out=None, stats=None, merge=False):
    """The label map `mask` (uint8 [D,H,W]) on the grid `shape`, `rpnet_resample_labels` calls on the current stream -> (out uint8,
    stats int64 [len(classes), 4] {voxels_in, voxels_out, out_voxels_total, 0} per class, None without classes).

    mode "nearest": the label at the nearest voxel, whatever `classes` says; one call, and one more per further class, which writes the
    same output again and fills the row of that class.  mode "linear": `classes` is needed; one call per class in the order given, each
    the linear rule on the indicator of the class with `> 0.5`; the first writes cls or 0 everywhere, the others take only voxels that
    hold 0.  merge=True (linear mode, `out` given): the first class too takes only the voxels of `out` that hold 0, so the classes are
    laid over what `out` held.  Launches only: nothing is copied or synchronised."""
    fn = "resample_labels"
    hip.require_gpu(mask, out, stats)
    _resample_volume_check(mask, (torch.uint8,), "mask", fn)
    shape = check_grid(shape, fn)
    if mode not in MODES:
        raise ValueError(f"{fn}: mode must be 'nearest' or 'linear', got {mode!r}")
    a = check_align(align, fn)
    classes = None if classes is None else [int(c) for c in classes]
    low = 1 if mode == "linear" else 0
    if classes is not None and (not classes or not all(low <= c <= 255 for c in classes)):
        raise ValueError(f"{fn}: classes must be a non-empty sequence of values {low}..255, got {classes!r}")
    if classes is None and mode == "linear":
        raise ValueError(f"{fn}: mode 'linear' resamples one indicator per class and needs the classes")
    if merge and (mode != "linear" or out is None):
        raise ValueError(f"{fn}: merge lays the classes over what `out` holds: it needs mode 'linear' and an `out`")
    if classes is None and stats is not None:
        raise ValueError(f"{fn}: a statistics table needs the classes it counts")
    out = _resample_out(out, mask, shape, fn)
    if classes is not None:
        if stats is None:
            stats = torch.zeros((len(classes), STATS_ROW), device=mask.device, dtype=torch.int64)
        check_table(stats, len(classes), STATS_ROW, torch.int64, "stats", fn)
    one_device(fn, mask, out, stats)
    dims = tuple(mask.shape) + shape
    ws, nbytes = _workspaces.get("rpnet_resample_workspace_bytes", mask.device, dims)
    if classes is None:
        hip.call("rpnet_resample_labels", hip.ptr(mask), *dims[:3], hip.ptr(out), *shape, 0, a, NEAREST, 0, None, 0, 0, hip.ptr(ws), nbytes)
        return out, None
    for r, c in enumerate(classes):
        hip.call("rpnet_resample_labels", hip.ptr(mask), *dims[:3], hip.ptr(out), *shape, c, a, MODES[mode], int(r > 0 or bool(merge)), hip.ptr(stats), r,
                 len(classes), hip.ptr(ws), nbytes)
    return out, stats


def resample_like(x, ref_shape, **options):
    """`x` on the grid `ref_shape`, e.g. a prediction taken back to the native grid of its volume: resample_labels for a uint8 tensor
    (options: classes, mode, align, out, stats; the statistics are dropped), resample_image otherwise (options: order, align, out,
    antialias).  A label map is not smoothed: antialias=True with one is refused."""
    if torch.is_tensor(x) and x.dtype == torch.uint8:
        if options.pop("antialias", False):
            raise ValueError("resample_like: antialias smooths an image; a uint8 label map keeps the indicator rule")
        return resample_labels(x, ref_shape, **options)[0]
    return resample_image(x, ref_shape, **options)


def resample_to_spacing(vol, spacing, new_spacing, align="corner", **options):
    """`vol` with the per-axis `spacing` (sz, sy, sx) taken to `new_spacing` -> (out, out_spacing).  The grid is output_shape(vol.shape,
    spacing, new_spacing); `out_spacing` is what that grid really has (the lengths are whole numbers, so it is close to `new_spacing`,
    not equal): out_spacing(...) above.  A uint8 tensor is a label map (options of resample_labels), anything else an image (options
    of resample_image, antialias=True among them: the axes that shrink are smoothed first).  Launches only."""
    if not torch.is_tensor(vol) or vol.dim() != 3:
        raise ValueError("resample_to_spacing: vol must be a [D,H,W] tensor")
    shape = output_shape(vol.shape, spacing, new_spacing)
    return resample_like(vol, shape, align=align, **options), out_spacing(vol.shape, shape, spacing, align)
