"""Binary morphology of a segmented volume with a ball: erosion, dilation, opening and closing on the device (csrc/morph.hip,
include/rpnet_morph_abi.h), without the round trip through scipy.ndimage.binary_closing / binary_opening on the host.

Definitions.  A volume [D,H,W] (the set of its voxels is Omega), a class cls; the object is X = (value == cls).

Voxel ball.  A squared radius rho, an integer >= 1: B = {(dz,dy,dx) : dz^2 + dy^2 + dx^2 <= rho}.  rho = 1, 2, 3 are
scipy.ndimage.generate_binary_structure(3, 1 | 2 | 3), the 6-, 18- and 26-neighbourhoods.  A radius r in voxels means rho = floor(r^2).
per_slice takes dz = 0 only: every z slice is its own 2D image, as fill_holes='slice' does.

Millimetre ball.  A spacing (sz, sy, sx) and a radius r in its unit.  With the weights w = s * s rounded once (surface_spacing.
spacing_weights), B = {o : fl(fl(fl(wx dx^2) + fl(wy dy^2)) + fl(wz dz^2)) <= fl(r * r)}: the operations of the spacing transform
in the order its x, y and z passes apply them, so tests/morphology_cases.py, which restates them in numpy, gets the same set bit for bit.

Operations on Omega.
  dilate(X) = {v in Omega : there is s in X with v - s in B}; outside Omega is background.
  erode(X)  = {v in Omega : for every o in B, v + o in X or v + o not in Omega}; outside Omega counts as object: border_value=1 of
              scipy.ndimage.binary_erosion.  The adjoint pair makes closing = erode . dilate extensive and idempotent and
              opening = dilate . erode anti-extensive and idempotent on a bounded volume.
  erode_border=0: outside Omega counts as background in every erosion of the call, scipy's default border_value=0 (with it scipy's and
              this closing eat objects that touch the border).  In closed form: a voxel whose distance to the outside along any axis
              is within the ball is eroded as well.
The kernels take the route of the distance transform: dilate(X) = {d2(v, X) <= rho}, erode(X) = {d2(v, Omega \\ X) > rho}.

Writing back into a label volume (the rule of postprocess.fill_holes).  Voxels gained take cls only where the value is 0; voxels lost
become 0; every other value passes through as uint8; the object of a later class is read from the result so far.

A statistics row is int64 {voxels_before, voxels_after, voxels_added, voxels_removed} of the class (on a label volume `added` can be
smaller than the binary operation's gain); a counts row is int64 {|P and T|, |P|, |T|} of the class in the result, ADDED to what the row
holds.  Everything is integer or separately rounded fp64 work with integer atomics only: two runs give the same bits.

Not claimed: parity with SimpleITK's BinaryBall, which ITK rasterises as an ellipsoid by its own rule.
"""
import ctypes
import math

import numpy as np
import torch

from . import hip
from ._volume_checks import KINDS, WorkspaceCache, prepare_class_filter
from .surface_spacing import check_spacing, spacing_weights

STATS_ROW, COUNTS_ROW = 4, 3        # RPNET_MORPH_STATS_ROW, RPNET_MORPH_COUNTS_ROW
ERODE, DILATE, OPEN, CLOSE = 0, 1, 2, 3     # RPNET_MORPH_ERODE .. RPNET_MORPH_CLOSE
MAX_RHO = 3 * 1024 * 1024           # RPNET_MORPH_MAX_RHO
_workspaces = WorkspaceCache(by_shape=False)


def _is_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def check_radius(radius, what="morphology"):
    """the `radius` option -> ('rho', n) for a voxel ball or ('mm', x) for a millimetre ball, not yet resolved under a spacing.
    radius: a number of voxels (rho = floor(r^2), at least 1), ('rho', n) with an integer n >= 1, or (x, 'mm') with a finite x > 0"""
    if isinstance(radius, (tuple, list)) and len(radius) == 2:
        if radius[0] == "rho" and isinstance(radius[1], (int, np.integer)) and not isinstance(radius[1], bool) and 1 <= int(radius[1]) <= MAX_RHO:
            return ("rho", int(radius[1]))
        if not isinstance(radius[0], str) and radius[1] == "mm" and _is_number(radius[0]) and math.isfinite(radius[0]) and radius[0] > 0:
            return ("mm", float(radius[0]))
    elif _is_number(radius) and math.isfinite(radius) and radius >= 1 and math.floor(float(radius) * float(radius)) <= MAX_RHO:
        return ("rho", int(math.floor(float(radius) * float(radius))))
    raise ValueError(f"{what}: radius must be a number of voxels >= 1, ('rho', n) with an integer 1 <= n <= {MAX_RHO} or (x, 'mm') with "
                     f"x > 0, got {radius!r}")


def resolve_radius(radius, spacing=None, what="morphology"):
    """('rho', n) or ('mm', (wz, wy, wx), r2): the ball of a call.  The 'mm' form needs a spacing (sz, sy, sx); a voxel ball ignores one"""
    kind, value = check_radius(radius, what)
    if kind == "rho":
        return ("rho", value)
    if spacing is None:
        raise ValueError(f"{what}: a radius in mm needs a spacing (sz, sy, sx)")
    return ("mm", spacing_weights(check_spacing(spacing, what)), value * value)


def _apply(fn, op, mask, classes, radius, spacing, per_slice, erode_border, truth, out, counts, stats):
    ball = resolve_radius(radius, spacing, fn)
    if erode_border not in (0, 1, False, True):
        raise ValueError(f"{fn}: erode_border must be 1 (outside counts as object) or 0 (as background), got {erode_border!r}")
    classes, out, counts, stats = prepare_class_filter(fn, "process", mask, classes, truth, out, counts, stats, STATS_ROW, COUNTS_ROW)
    D, H, W = mask.shape
    ws, nbytes = _workspaces.get("rpnet_morph_workspace_bytes", mask.device, (D, H, W))
    src = mask
    for r, c in enumerate(classes):
        tail = (int(bool(per_slice)), int(erode_border), hip.ptr(truth), KINDS[truth.dtype] if truth is not None else 0, hip.ptr(counts), r,
                hip.ptr(stats), r, len(classes), hip.ptr(ws), nbytes)
        if ball[0] == "rho":
            hip.call("rpnet_morph_apply", hip.ptr(src), KINDS[src.dtype], hip.ptr(out), c, D, H, W, op, ball[1], *tail)
        else:
            hip.call("rpnet_morph_apply_spacing", hip.ptr(src), KINDS[src.dtype], hip.ptr(out), c, D, H, W, op, (ctypes.c_double * 3)(*ball[1]),
                     ball[2], *tail)
        src = out                       # the classes processed so far are in `out`; the next one is read there and written in place
    return out, counts, stats


def erode(mask, classes, radius, spacing=None, per_slice=False, erode_border=1, truth=None, out=None, counts=None, stats=None):
    """Erode every class in `classes` by the ball, one `rpnet_morph_apply` (voxel ball) or `rpnet_morph_apply_spacing` (millimetre ball)
    call per class on the current stream -> (out uint8 [D,H,W], counts int64 [len(classes), 3] or None, stats int64 [len(classes), 4]);
    row r belongs to classes[r].  radius: voxels, ('rho', n) or (x, 'mm') under `spacing` (sz, sy, sx).  per_slice: every z slice on its
    own.  erode_border: 1 outside counts as object, 0 as background.  Voxels lost become 0, voxels gained take the class only where the
    value is 0; out may be `mask` itself when that is uint8.  truth: the Dice counts of each class in the result are ADDED to counts
    (made of zeros when not handed in).  Launches only: nothing is copied or synchronised."""
    return _apply("erode", ERODE, mask, classes, radius, spacing, per_slice, erode_border, truth, out, counts, stats)


def dilate(mask, classes, radius, spacing=None, per_slice=False, erode_border=1, truth=None, out=None, counts=None, stats=None):
    """Dilate every class in `classes` by the ball; arguments and results as `erode` (erode_border has no erosion to act on)"""
    return _apply("dilate", DILATE, mask, classes, radius, spacing, per_slice, erode_border, truth, out, counts, stats)


def opening(mask, classes, radius, spacing=None, per_slice=False, erode_border=1, truth=None, out=None, counts=None, stats=None):
    """Open (dilate . erode) every class in `classes` by the ball; arguments and results as `erode`"""
    return _apply("opening", OPEN, mask, classes, radius, spacing, per_slice, erode_border, truth, out, counts, stats)


def closing(mask, classes, radius, spacing=None, per_slice=False, erode_border=1, truth=None, out=None, counts=None, stats=None):
    """Close (erode . dilate) every class in `classes` by the ball; arguments and results as `erode`"""
    return _apply("closing", CLOSE, mask, classes, radius, spacing, per_slice, erode_border, truth, out, counts, stats)


def morph_figures(stats_host):
    """per row of a host table [..., 4]: {'before', 'after', 'added', 'removed'} -> a flat list"""
    return [{"before": int(r[0]), "after": int(r[1]), "added": int(r[2]), "removed": int(r[3])}
            for r in np.asarray(stats_host).reshape(-1, STATS_ROW)]


def line_suffix(opening=None, closing=None):
    """what an item line gains: ` open -<removed> +<added>` and ` close -<removed> +<added>` voxels, each for the stage that ran"""
    s = ""
    for word, f in (("open", opening), ("close", closing)):
        if f is not None:
            s += f" {word} -{f['removed']} +{f['added']}"
    return s


def mean_suffix(opening=None, closing=None):
    """what a class line gains: the same figures as means over the items (lists of figures)"""
    s = ""
    for word, fs in (("open", opening), ("close", closing)):
        if fs is not None:
            s += f" {word} -{np.mean([f['removed'] for f in fs]):.2f} +{np.mean([f['added'] for f in fs]):.2f}"
    return s
