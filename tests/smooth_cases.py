"""A numpy restatement of rpnet_amd.smooth (include/rpnet_smooth_abi.h) and the case tables shared by tests/test_host_smooth.py (which pins
it to scipy.ndimage.gaussian_filter and shows that seeded defects fail) and tests/test_gpu_smooth.py (which compares the device with it
for equality).  One pass is an explicit loop over k ascending, s = s + w[k + r] * v[..., fold(idx + k)] on float64 arrays, every operation
rounded on its own; the passes run x, y, z; then comes the one conversion (that of tests/resample_cases.py).

Every function takes `defect`, a set of names: each name switches one rule to a plausible wrong one, so that the host tests can show
that the comparison notices it.  The GPU tests never pass one."""
import numpy as np

from tests.resample_cases import convert, linear_f64, noise_image  # noqa: F401  (re-exported for the two test files)

DEFECTS = ("mirror", "clamp for reflect", "radius without half", "unnormalised", "z and x swapped", "int16 truncation",
           "float32 between passes", "radius 0 multiplies")
MODES = ("reflect", "nearest")
U = 2.0 ** -53                                      # unit roundoff of float64


def weights(sigma, truncate=4.0, defect=()):
    """(float64 weights, radius): scipy's kernel (scipy/ndimage/_filters.py:_gaussian_kernel1d with gaussian_filter1d's radius)"""
    sigma = float(sigma)
    if sigma <= 0:
        return np.ones(1), 0
    radius = int(truncate * sigma) if "radius without half" in defect else int(truncate * sigma + 0.5)
    k = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    return (phi if "unnormalised" in defect else phi / phi.sum()), radius


def fold(idx, n, mode, defect=()):
    """the index of the line that stands for idx"""
    idx = np.asarray(idx, np.int64)
    if mode == "nearest" or "clamp for reflect" in defect:
        return np.clip(idx, 0, n - 1)
    assert mode == "reflect", mode
    if "mirror" in defect:                          # d c b | a b c d | c b a: the edge voxel is not repeated
        if n == 1:
            return np.zeros_like(idx)
        j = np.mod(idx, 2 * n - 2)
        return np.where(j >= n, 2 * n - 2 - j, j)
    j = np.mod(idx, 2 * n)                          # non-negative
    return np.where(j >= n, 2 * n - 1 - j, j)


def one_pass(v, w, r, axis, mode, defect=()):
    """s = 0; for k ascending: s = fl(s + fl(w[k + r] * v[fold(i + k)])) along `axis`"""
    n = v.shape[axis]
    idx = np.arange(n)
    s = np.zeros_like(v)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(-r, r + 1):
            s = s + w[k + r] * np.take(v, fold(idx + k, n, mode, defect), axis=axis)
    return s


def radii(sigmas, truncate=4.0):
    return tuple(weights(s, truncate)[1] for s in sigmas)


def smooth_f64(vol, sigmas, mode="reflect", truncate=4.0, defect=(), tables=None):
    """the float64 result before its conversion.  sigmas: (sz, sy, sx) in voxels.  tables: ((wz, rz), (wy, ry), (wx, rx)) instead of
    the kernels of the sigmas.  With no pass at all the input is returned as it is (not widened)."""
    vol = np.asarray(vol)
    if tables is None:
        if "z and x swapped" in defect:
            sigmas = tuple(sigmas)[::-1]
        tables = [weights(s, truncate, defect) for s in sigmas]
    v, widened = vol, False
    for axis in (2, 1, 0):
        w, r = tables[axis]
        if r == 0 and "radius 0 multiplies" not in defect:
            continue
        if not widened:
            v, widened = vol.astype(np.float64), True
        v = one_pass(v, np.asarray(w, np.float64), r, axis, mode, defect)
        if "float32 between passes" in defect:
            v = v.astype(np.float32).astype(np.float64)
    return v


def ref_smooth(vol, sigmas, mode="reflect", truncate=4.0, defect=(), tables=None):
    vol = np.asarray(vol)
    r = smooth_f64(vol, sigmas, mode, truncate, defect, tables)
    if r.dtype == vol.dtype:                        # no pass ran: the input bit for bit
        return np.ascontiguousarray(vol).copy()
    return np.ascontiguousarray(convert(r, vol.dtype, defect))


def error_bound(vol, sigmas, mode="reflect", truncate=4.0):
    """What |restatement - exact| can be, voxel by voxel, derived: a sum of 2r + 1 products formed one rounding at a time is off by at most
    (2r + 2) u sum|w||v| (2r + 1 additions and one product per term, to first order; u = 2^-53), and an error a pass inherits goes through
    the later passes by the same filter, whose weights are positive.  The magnitudes the later passes see are bounded by the filtered
    magnitudes plus that error."""
    a = np.abs(np.asarray(vol).astype(np.float64))
    e = np.zeros_like(a)
    for axis in (2, 1, 0):
        w, r = weights(sigmas[axis], truncate)
        if r == 0:
            continue
        fa = one_pass(a, w, r, axis, mode)
        e = one_pass(e, w, r, axis, mode) + (2 * r + 2) * U * (fa + e)
        a = fa + e
    return e


def antialias_sigmas(shape, new_shape):
    return tuple(max(0.0, (n / m - 1) / 2) for n, m in zip(shape, new_shape))


def ref_antialiased(vol, shape, align="corner", defect=()):
    """smooth (border nearest, the sigmas of the shrink) to the kind of the volume, then the linear rule of tests/resample_cases.py"""
    vol = np.asarray(vol)
    smoothed = ref_smooth(vol, antialias_sigmas(vol.shape, shape), "nearest", defect=defect)
    return np.ascontiguousarray(convert(linear_f64(smoothed, shape, align), vol.dtype, defect))


# ---------------------------------------------------------------------------------------------------------------- cases
# the tiles of csrc/smooth.hip (rpnet_amd.smooth exports the same numbers, and tests/test_host_smooth_abi_ledger.py compares them)
LANE_RUN = {np.dtype(np.float32): 4, np.dtype(np.int16): 8}
X_TILE = {np.dtype(np.float32): 256, np.dtype(np.int16): 512}
X_ROWS = 4
AXIS_SEG = {np.dtype(np.float32): 8, np.dtype(np.int16): 4}

# (shape, (sz, sy, sx)): one voxel with radius 3; each axis of length 1 with a radius on it; lines of 2 and 3 with radius 7 (sigma 1.75:
# the reflection folds more than once); 5 x 7 x 9 with three sigmas; a radius on one axis only; no radius at all
SMALL = (((1, 1, 1), (0.75, 0.75, 0.75)), ((1, 6, 7), (1.0, 0.5, 0.75)), ((6, 1, 7), (0.5, 1.0, 0.75)), ((6, 7, 1), (0.5, 0.75, 1.0)),
         ((2, 3, 2), (1.75, 1.75, 1.75)), ((3, 2, 3), (1.75, 1.75, 1.75)), ((5, 7, 9), (0.5, 1.0, 1.5)), ((5, 7, 9), (1.0, 0.0, 0.0)),
         ((5, 7, 9), (0.0, 1.0, 0.0)), ((5, 7, 9), (0.0, 0.0, 1.0)), ((5, 7, 9), (0.0, 0.0, 0.0)), ((4, 5, 6), (0.0, 1.0, 0.6)),
         ((4, 5, 6), (0.7, 0.0, 1.0)), ((4, 5, 6), (0.7, 1.0, 0.0)))
# a line of 1024 along each axis, the other two axes 2
LINES = (((1024, 2, 2), (1.0, 0.5, 0.5)), ((2, 1024, 2), (0.5, 1.0, 0.5)), ((2, 2, 1024), (0.5, 0.5, 1.0)))
# radius 255 (sigma 63.75) on a line of 300, one axis at a time
WIDE = (((300, 1, 3), (63.75, 0.0, 0.0)), ((1, 300, 3), (0.0, 63.75, 0.0)), ((1, 2, 300), (0.0, 0.0, 63.75)))


def tile_shapes(dtype):
    """every tile extent + 1 and 2 * tile + 2, with a radius (3, sigma 0.75) that crosses the seam: the segment of a lane along y and z,
    the rows of a block of the x pass, the x positions of a block of the x pass, the run of a lane.  Two int16 tiles of the x pass are
    the longest row there is, 1024: that case stands for 2 * tile + 2, which no volume has"""
    d = np.dtype(dtype)
    seg, xt, run = AXIS_SEG[d], X_TILE[d], LANE_RUN[d]
    s = (0.75, 0.75, 0.75)
    return (((seg + 1, 2 * seg + 2, run + 1), s), ((2 * seg + 2, seg + 1, 2 * run + 2), s), ((1, X_ROWS + 1, xt + 1), s),
            ((2, X_ROWS + 1, min(2 * xt + 2, 1024)), (0.0, 0.75, 2.0)), ((1, 2 * X_ROWS + 2, 3 * run + run // 2), s))
