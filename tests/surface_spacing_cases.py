"""Case tables and checks shared by tests/test_host_surface_spacing.py and tests/test_gpu_surface_spacing.py (numpy only).

The y / z tile table of csrc/surface_spacing.hip: 32 columns for lines up to 128 voxels, 16 up to 256, 8 up to 1024, the LDS of a tile
passing 32 KiB above 512.  The shapes below are the smallest at which each mechanism can go wrong: one voxel; lines with a single axis;
one more column than each tile width with a line length on either side of every threshold, along y and along z; the axis limit on each
axis beside 3 and 5.  A reference row costs a brute-force transform, so every (shape, spacing, content) row is computed once and kept."""
import functools
import math

import numpy as np

SPACINGS = [(1.0, 1.0, 1.0), (2.5, 0.7, 0.7), (5.0, 0.78125, 0.78125), (1 / 3, 1.1, 0.9)]

ONE = [(1, 1, 1)]
LINES = [(1, 1, 37), (37, 1, 1), (1, 37, 1)]
# (D, H, W): y lines of H voxels, z lines of D voxels, W one more than the tile width the longer of them selects
TILES = [(4, 128, 33), (4, 129, 33), (3, 129, 17), (3, 256, 17), (3, 257, 17), (3, 257, 9), (2, 512, 9), (2, 513, 9),
         (128, 3, 33), (129, 4, 17), (257, 2, 9)]
LIMIT = [(1024, 3, 5), (3, 1024, 5), (3, 5, 1024)]
SHAPES = ONE + LINES + TILES + LIMIT
CONTENTS = ["boxes", "noise", "full", "empty", "empty_pred", "empty_truth"]


def boxes(shape):
    """a box against the same box shifted by one voxel where the axis has room (many equal distances: ties across the 95 % rank)"""
    a, b = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    lo = [s // 4 for s in shape]
    hi = [max(l + 1, s - s // 4 - 1) for l, s in zip(lo, shape)]
    a[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 1
    sh = [1 if h < s else 0 for h, s in zip(hi, shape)]
    b[lo[0] + sh[0]:hi[0] + sh[0], lo[1] + sh[1]:hi[1] + sh[1], lo[2] + sh[2]:hi[2] + sh[2]] = 1
    return a, b


def noise(shape, seed=0, density=0.3):
    """(prediction, truth) of independent noise; one voxel of each is set so that neither border is empty at the smallest shapes"""
    rs = np.random.RandomState(4000 + seed + sum(shape))
    a, b = (rs.rand(*shape) < density).astype(np.uint8), (rs.rand(*shape) < density).astype(np.uint8)
    a.flat[0] = b.flat[-1] = 1
    return a, b


def content(shape, name):
    """(prediction, truth) uint8 of one family"""
    zero = np.zeros(shape, np.uint8)
    if name == "boxes":
        return boxes(shape)
    if name == "noise":
        return noise(shape)
    if name == "full":
        return np.ones(shape, np.uint8), noise(shape, 1)[1] | boxes(shape)[1]
    if name == "empty":
        return zero, zero
    if name == "empty_pred":
        return zero, boxes(shape)[1]
    if name == "empty_truth":
        return boxes(shape)[0], zero
    raise KeyError(name)


def scattered(n_a, n_b, shape=(7, 24, 25), seed=0):
    """n_a and n_b isolated voxels (each is its own border: no two share a face), so the pooled count is n_a + n_b exactly"""
    rs = np.random.RandomState(seed)
    grid = [(z, y, x) for z in range(0, shape[0], 2) for y in range(0, shape[1], 2) for x in range(0, shape[2], 2)]
    pick = rs.permutation(len(grid))[:n_a + n_b]
    a, b = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    for i, g in enumerate(pick):
        (a if i < n_a else b)[grid[g]] = 1
    return a, b


# pooled counts of 2 (k = 0, k + 1 = n - 1), 3, 21 ((n - 1) * 0.95 is a whole number up to rounding) and 22 (interpolation at 0.95)
COUNTS = [(1, 1), (1, 2), (1, 20), (2, 20)]


def planes(shape=(6, 9, 10)):
    """two parallel planes one apart along y and one stray voxel: every distance but a few is the same number (ties across the rank)"""
    a, b = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    a[:, 2, :] = 1
    b[:, 3, :] = 1
    a[0, 8, 0] = 1
    return a, b


def low_bits(m=10):
    """(prediction, truth, shape): one prediction voxel at the centre, truth voxels at the offsets 1..m along x and along y.  Under a
    spacing (1, 1 + e, 1) the pooled distances come in pairs o^2 and o^2 * (1 + e)^2 whose doubles differ in the low bits only; with
    n = 2m + 1 = 21 the ranks k = 19 and k + 1 = 20 are the two values of the largest pair, so the last radix digit that differs between
    them decides, after every digit above it agreed"""
    shape = (1, 2 * m + 1, 2 * m + 1)
    a, b = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    a[0, m, m] = 1
    for o in range(1, m + 1):
        b[0, m, m + o] = 1
        b[0, m - o, m] = 1
    return a, b, shape                              # D == 1: every foreground voxel is a border voxel


# spacings whose y weight differs from 1 in the lowest byte, in a middle byte and in a high byte of the mantissa
LOW_BIT_SPACINGS = [(1.0, 1.0 + 2.0 ** -52, 1.0), (1.0, 1.0 + 2.0 ** -30, 1.0), (1.0, 1.0 + 2.0 ** -9, 1.0)]


@functools.lru_cache(maxsize=None)
def reference(shape, name, spacing, tau=None):
    """(irow, frow) of rows_reference_spacing for one table entry, computed once"""
    from rpnet_amd import surface_spacing as SS
    a, b = content(shape, name)
    irow, frow = SS.rows_reference_spacing(a, b, spacing, tau=tau)
    irow.setflags(write=False)
    frow.setflags(write=False)
    return irow, frow


def check_rows(got_i, got_f, want_i, want_f, what=""):
    """the int64 row and d2_k, d2_k1, d2_max bit for bit; the two sums within n * 2^-52 * sum.  Derivation: either side adds n
    non-negative terms sqrt(d2), each one correctly rounded square root (relative 2^-53) of the same double; the device adds them in its
    fixed order with one rounding per addition, so its sum lies within (n - 1) * 2^-53 relative of the exact sum of its terms (all terms
    are >= 0, so the partial sums never exceed the total), plus 2^-53 for the roots: n * 2^-53.  math.fsum of the restatement is the exact
    sum of the same rounded roots, rounded once: 2^-53 more.  Together below n * 2^-52 for every n >= 1."""
    got_i, got_f = np.asarray(got_i), np.asarray(got_f)
    assert got_i.tolist() == np.asarray(want_i).tolist(), (what, got_i.tolist(), np.asarray(want_i).tolist())
    assert got_f[:3].view(np.int64).tolist() == np.asarray(want_f)[:3].view(np.int64).tolist(), (what, got_f[:3].tolist(), list(want_f[:3]))
    for col, n in ((3, int(want_i[0])), (4, int(want_i[1]))):
        bound = n * 2.0 ** -52 * float(want_f[col])
        assert abs(float(got_f[col]) - float(want_f[col])) <= bound, (what, col, float(got_f[col]), float(want_f[col]), bound)


def brute_force(pred, truth, spacing, cls=1):
    """all-pairs restatement of the definition, independent of any transform: sorted pooled distances (not squared), by
    sqrt(sum_axis (s * d)^2) over every pair of border voxels"""
    from rpnet_amd.surface import border_reference
    pa = np.argwhere(border_reference(np.asarray(pred) == cls)).astype(np.float64)
    pb = np.argwhere(border_reference(np.asarray(truth) == cls)).astype(np.float64)
    s = np.asarray(spacing, dtype=np.float64)
    d = np.sqrt((((pa[:, None, :] - pb[None, :, :]) * s) ** 2).sum(-1))
    return np.sort(np.concatenate([d.min(1), d.min(0)]))


def ulps(a, b):
    """largest relative difference of two positive arrays in units of 2^-52"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    m = np.maximum(np.abs(a), np.abs(b))
    return float(np.max(np.where(m > 0, np.abs(a - b) / np.where(m > 0, m, 1.0), 0.0)) / 2.0 ** -52) if a.size else 0.0


def percentile95(sorted_values):
    return float(np.percentile(sorted_values, 95))


def rank(n):
    return int(math.floor((n - 1) * 0.95))
