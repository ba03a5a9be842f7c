"""Separable Gaussian smoothing of a volume on the device (csrc/smooth.hip, include/rpnet_smooth_abi.h): the device form of
scipy.ndimage.gaussian_filter, to which tests/test_host_smooth.py pins it, and the prefilter of a shrinking resample
(rpnet_amd.resample: `antialias=True`; tools/preprocess_volumes.py --antialias).

Definitions (word for word those of include/rpnet_smooth_abi.h; tests/smooth_cases.py restates them in numpy, bit for bit).  A volume is
[D,H,W] float32 or int16; every axis length is 1..1024, every radius 0..255.  fl(.) is one float64 rounding.

Weights: scipy's kernel, radius = int(truncate * sigma + 0.5), exp(-0.5 / sigma^2 * k^2) for k = -radius .. radius, divided by its sum;
built on the host in float64.  sigma <= 0 gives radius 0.
Passes: the voxels widened to float64; x first, then y, then z; a pass with radius 0 is skipped, it is not a multiplication by 1.  One
pass along an axis of length n: s = 0; for k = -r .. r ascending: s = fl(s + fl(w[k + r] * v[fold(i + k)])).  mode "reflect":
j = (i + k) mod 2n taken non-negative, fold = 2n - 1 - j where j >= n and j elsewhere (d c b a | a b c d | d c b a, any radius).  mode
"nearest": fold = clamp(i + k, 0, n - 1).  Nothing is rounded to a narrower type between passes.
Result: one conversion to the kind of the volume (float32 rounds to nearest; int16 rounds half to even and saturates).  With all radii 0
the output is the input bit for bit.  A NaN or an infinity is not special-cased: it spreads over its ball.

Anti-aliasing: an axis that shrinks from n to m voxels is prefiltered with sigma = (n / m - 1) / 2 voxels, an axis that does not shrink
with none.  That rule is this project's own: scipy.ndimage.zoom has no prefilter for order 1, and the reference ships none.
"""
import functools

import numpy as np
import torch

from . import hip
from ._volume_checks import WorkspaceCache, one_device

VOLUME_KINDS = {torch.float32: 0, torch.int16: 1}   # RPNET_PREP_F32, RPNET_PREP_I16
REFLECT, CLAMP = 0, 1                               # RPNET_SMOOTH_REFLECT, RPNET_SMOOTH_NEAREST
BORDERS = {"reflect": REFLECT, "nearest": CLAMP}
MAX_RADIUS = 255                                    # RPNET_SMOOTH_MAX_RADIUS
MAX_EXTENT = 1024                                   # RPNET_CC_MAX_DIM
# the tiles of csrc/smooth.hip: x positions of a lane (16 bytes), x positions and rows of a block of the x pass, and outputs of a lane
# along the axis of the y and z passes
LANE_RUN = {torch.float32: 4, torch.int16: 8}
X_TILE = {torch.float32: 256, torch.int16: 512}
X_ROWS = 4
AXIS_SEG = {torch.float32: 8, torch.int16: 4}
AXES = ("z", "y", "x")
# one workspace per device, grown on demand, as rpnet_amd.resample keeps its own: a workspace is up to 16 bytes per voxel, and one per
# shape would stay allocated for every shape a process has ever smoothed.  A captured graph holds the workspace it was captured with by
# its address: capture after the largest volume of the process has been seen, or the buffer it holds is freed when a larger one comes.
_workspaces = WorkspaceCache(by_shape=False)


def smooth_radius(sigma, truncate=4.0, axis=None):
    """scipy's radius of the kernel of `sigma`: int(truncate * sigma + 0.5), 0 for sigma <= 0 (the pass is skipped).  A radius above 255
    is refused; axis: the name that error gives the axis."""
    sigma, truncate = float(sigma), float(truncate)
    if not (np.isfinite(sigma) and np.isfinite(truncate)) or truncate < 0:
        raise ValueError(f"smooth_weights: sigma {sigma!r} and truncate {truncate!r} must be finite, truncate not negative")
    radius = 0 if sigma <= 0 else int(truncate * sigma + 0.5)
    if radius > MAX_RADIUS:
        where = "" if axis is None else f" of the {axis} axis"
        raise ValueError(f"smooth_weights: sigma {sigma!r}{where} gives radius {radius} at truncate {truncate!r}; the largest is {MAX_RADIUS}")
    return radius


def smooth_weights(sigma, truncate=4.0, axis=None):
    """the 1-D kernel of scipy.ndimage.gaussian_filter(sigma, truncate=truncate) -> (float64 weights [2 * radius + 1], radius of
    smooth_radius)"""
    radius = smooth_radius(sigma, truncate, axis)
    if radius == 0:
        return np.ones(1, np.float64), 0
    sigma = float(sigma)
    k = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    return phi / phi.sum(), radius


@functools.lru_cache(maxsize=None)
def smooth_device_weights(sigma, truncate, device):
    """(the weights of smooth_weights on `device`, radius), one table per (sigma, truncate, device) whatever the axis; (None, 0) for a
    pass that is skipped.  The cache is not bounded: a table is at most 4 KiB, and a captured graph holds it by its address, so a table
    that has been handed out is never freed."""
    w, radius = smooth_weights(sigma, truncate)
    return (torch.from_numpy(w).to(device), radius) if radius else (None, 0)


def _smooth_sigmas(sigma, spacing, fn):
    """(sz, sy, sx) in voxels from a number or three, in millimetres where a spacing is given"""
    try:
        s = tuple(float(v) for v in sigma) if np.ndim(sigma) else (float(sigma),) * 3
    except (TypeError, ValueError):
        s = ()
    if len(s) != 3 or not all(np.isfinite(v) for v in s):
        raise ValueError(f"{fn}: sigma must be a finite number or three (sz, sy, sx), got {sigma!r}")
    if spacing is not None:
        try:
            sp = tuple(float(v) for v in spacing)
        except (TypeError, ValueError):
            sp = ()
        if len(sp) != 3 or not all(np.isfinite(v) and v > 0 for v in sp):
            raise ValueError(f"{fn}: spacing must be three positive finite numbers (sz, sy, sx), got {spacing!r}")
        s = tuple(a / b for a, b in zip(s, sp))
    return s


def antialias_sigma(shape, new_shape):
    """the sigma, in voxels of `shape`, that a resample to `new_shape` is prefiltered with: max(0, (n / m - 1) / 2) per axis, so a shrink
    by f gets (f - 1) / 2 and an axis that does not shrink gets none (this project's own rule)"""
    return tuple(max(0.0, (int(n) / int(m) - 1) / 2) for n, m in zip(shape, new_shape))


def smooth_image(vol, sigma, spacing=None, mode="reflect", truncate=4.0, out=None):
    """`vol` (float32 or int16 [D,H,W]) filtered with a Gaussian of `sigma` voxels (a number or (sz, sy, sx); millimetres where `spacing`
    (sz, sy, sx) is given), one `rpnet_smooth_image` call on the current stream -> out, of the kind of `vol`.  mode: "reflect" or
    "nearest", scipy's borders of those names.  Launches only: nothing is copied or synchronised once the weights of a sigma are on the
    device."""
    fn = "smooth_image"
    hip.require_gpu(vol, out)
    if not torch.is_tensor(vol) or vol.dtype not in VOLUME_KINDS:
        raise ValueError(f"{fn}: vol is {getattr(vol, 'dtype', type(vol))}; float32 and int16 volumes are accepted")
    if vol.dim() != 3 or not vol.is_contiguous() or not all(1 <= n <= MAX_EXTENT for n in vol.shape):
        raise ValueError(f"{fn}: vol must be a contiguous [D,H,W] tensor with every axis 1..{MAX_EXTENT}, got {tuple(vol.shape)}")
    if mode not in BORDERS:
        raise ValueError(f"{fn}: mode must be 'reflect' or 'nearest', got {mode!r}")
    sig = _smooth_sigmas(sigma, spacing, fn)
    if out is None:
        out = torch.empty_like(vol)
    elif not torch.is_tensor(out) or out.dtype != vol.dtype or out.shape != vol.shape or not out.is_contiguous():
        raise ValueError(f"{fn}: out must be a contiguous {str(vol.dtype)[6:]} tensor of shape {tuple(vol.shape)}")
    one_device(fn, vol, out, what="the volumes")
    for s, a in zip(sig, AXES):
        smooth_radius(s, truncate, a)               # the refusal of a radius above 255 names its axis
    tables = [smooth_device_weights(s, float(truncate), vol.device) for s in sig]
    radii = tuple(r for _, r in tables)
    ws, nbytes = _workspaces.get("rpnet_smooth_workspace_bytes", vol.device, tuple(vol.shape) + radii)
    args = [a for w, r in tables for a in (hip.ptr(w), r)]
    hip.call("rpnet_smooth_image", hip.ptr(vol), VOLUME_KINDS[vol.dtype], *vol.shape, hip.ptr(out), *args, BORDERS[mode], hip.ptr(ws), nbytes)
    return out
