"""A numpy restatement of rpnet_amd.resample (include/rpnet_resample_abi.h) and the case tables shared by tests/test_host_resample.py (which
pins it to scipy.ndimage.zoom and shows that seeded defects fail) and tests/test_gpu_resample.py (which compares the device with it for
equality).  Separable: x, then y, then z, every float64 operation rounded on its own, which is the same sequence of operations per
voxel as the eight-tap order of the header (four lerps along x, two along y, one along z).

Every function takes `defect`, a set of names: each name switches one rule to a plausible wrong one, so that the host tests can show
that the comparison notices it.  The GPU tests never pass one."""
import numpy as np

DEFECTS = ("other alignment", "no far clamp", "z before x", "floor for nearest", "label >=", "int16 truncation", "no saturation",
           "merge over non-zero")


def coords(n, m, align, defect=()):
    """c of every output index of an axis: float64 [m]"""
    if "other alignment" in defect:
        align = "center" if align == "corner" else "corner"
    o = np.arange(m, dtype=np.int64)
    if align == "corner":
        return np.zeros(m) if m == 1 else (o * (n - 1)).astype(np.float64) / np.float64(m - 1)
    assert align == "center", align
    c = ((2 * o + 1) * n).astype(np.float64) / np.float64(2 * m) - 0.5
    return np.clip(c, 0.0, None if "no far clamp" in defect else float(n - 1))


def linear_table(n, m, align, defect=()):
    """(i0, i1, t) of every output index"""
    c = coords(n, m, align, defect)
    i0 = np.minimum(np.floor(c).astype(np.int64), n - 1)
    i1 = (i0 + 1) % n if "no far clamp" in defect else np.minimum(i0 + 1, n - 1)       # the defect reads voxel 0 past the far edge
    return i0, i1, c - i0


def nearest_table(n, m, align, defect=()):
    c = coords(n, m, align, defect)
    return np.clip(np.floor(c if "floor for nearest" in defect else c + 0.5).astype(np.int64), 0, n - 1)


def lerp(a, b, t):
    """a where t == 0 (the other tap is not used), a + t * (b - a) in three roundings elsewhere"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(t == 0, a, a + t * (b - a))


def linear_f64(vol, shape, align, defect=()):
    """the float64 result of the linear rule before its conversion"""
    v = np.asarray(vol).astype(np.float64)
    axes = (0, 1, 2) if "z before x" in defect else (2, 1, 0)
    for ax in axes:
        i0, i1, t = linear_table(v.shape[ax], shape[ax], align, defect)
        tb = t.reshape([-1 if k == ax else 1 for k in range(3)])
        v = lerp(np.take(v, i0, axis=ax), np.take(v, i1, axis=ax), tb)
    return v


def convert(r, dtype, defect=()):
    """the one conversion of a float64 result to the output kind"""
    dtype = np.dtype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        if dtype == np.float32:
            return r.astype(np.float32)
        assert dtype == np.int16, dtype
        q = np.trunc(r) if "int16 truncation" in defect else np.rint(r)
        if "no saturation" in defect:
            return q.astype(np.int64).astype(np.int16)              # wraps
        return np.clip(q, -32768.0, 32767.0).astype(np.int16)


def ref_image(vol, shape, order=1, align="corner", defect=()):
    vol = np.asarray(vol)
    if order == 0:
        iz, iy, ix = (nearest_table(n, m, align, defect) for n, m in zip(vol.shape, shape))
        return np.ascontiguousarray(vol[np.ix_(iz, iy, ix)])
    return np.ascontiguousarray(convert(linear_f64(vol, shape, align, defect), vol.dtype, defect))


def ref_labels(mask, shape, classes=None, mode="nearest", align="corner", defect=(), into=None):
    """(out uint8, stats int64 [len(classes), 4] or None).  into (linear mode): what the output holds before the first class, which then
    merges as the later ones do (merge = 1 from the first call on)"""
    mask = np.asarray(mask)
    assert mask.dtype == np.uint8
    total = int(np.prod(shape))
    if mode == "nearest":
        out = ref_image(mask, shape, 0, align, defect)
        if classes is None:
            return out, None
        return out, np.array([[int((mask == c).sum()), int((out == c).sum()), total, 0] for c in classes], np.int64)
    out, rows = (np.zeros(shape, np.uint8) if into is None else np.array(into, np.uint8)), []
    for k, c in enumerate(classes):
        r = linear_f64(mask == c, shape, align, defect)
        hit = (r >= 0.5) if "label >=" in defect else (r > 0.5)
        if k == 0 and into is None:
            out = np.where(hit, c, 0).astype(np.uint8)
        else:
            out = np.where(hit if "merge over non-zero" in defect else hit & (out == 0), c, out).astype(np.uint8)
        rows.append([int((mask == c).sum()), int((out == c).sum()), total, 0])
    return out, np.array(rows, np.int64)


def ref_output_shape(shape, spacing, new_spacing):
    return tuple(max(1, int(np.round(n * s / t))) for n, s, t in zip(shape, spacing, new_spacing))


def ref_out_spacing(shape, new_shape, spacing, align):
    if align == "center":
        return tuple(s if m == n else s * n / m for s, n, m in zip(spacing, shape, new_shape))
    return tuple(s if m in (1, n) else s * (n - 1) / (m - 1) for s, n, m in zip(spacing, shape, new_shape))


# ---------------------------------------------------------------------------------------------------------------- cases
RUN = {np.dtype(np.float32): 4, np.dtype(np.int16): 8, np.dtype(np.uint8): 16}       # output x positions of a lane of the gather
ALIGNS = ("corner", "center")
# (input shape, output shape): one voxel; 1 -> 5 and 5 -> 1; each axis of length 1 in turn; the identity; 5x7x9 <-> 8x5x13
SMALL = (((1, 1, 1), (1, 1, 1)), ((1, 1, 1), (5, 5, 5)), ((5, 5, 5), (1, 1, 1)), ((1, 6, 7), (1, 9, 4)), ((6, 1, 7), (4, 1, 9)),
         ((6, 7, 1), (9, 4, 1)), ((1, 6, 7), (3, 6, 7)), ((5, 7, 9), (5, 7, 9)), ((5, 7, 9), (8, 5, 13)), ((8, 5, 13), (5, 7, 9)),
         ((3, 2, 4), (1, 3, 2)))
# a line of 1024 along each axis, as input and as output, the other axes <= 3
LINES = (((1024, 2, 3), (7, 3, 2)), ((2, 1024, 3), (3, 9, 2)), ((3, 2, 1024), (2, 3, 11)), ((5, 2, 3), (1024, 3, 2)), ((2, 7, 3), (3, 1024, 2)),
         ((3, 2, 6), (2, 3, 1024)), ((2, 3, 1024), (2, 3, 1024)))


def run_shapes(dtype):
    """output x lengths of one lane run + 1 and two runs + 2 (with 3 output rows an odd length also makes rows whose first address is
    not 16-byte aligned), and an even length whose rows start off a 16-byte boundary"""
    r = RUN[np.dtype(dtype)]
    return (((3, 4, 6), (2, 3, r + 1)), ((3, 4, 40), (3, 2, 2 * r + 2)), ((2, 3, 9), (2, 3, 3 * r + r // 2)))


def noise_image(shape, dtype, seed=0):
    """CT-like values; float32 images carry fractions so that no product is exact by luck"""
    rng = np.random.default_rng(seed + 1000 * int(np.prod(shape)))
    if np.dtype(dtype) == np.int16:
        return rng.integers(-1024, 3000, shape).astype(np.int16)
    return (rng.standard_normal(shape) * 400.0 - 200.0).astype(np.float32)


def label_map(shape, seed=0):
    """three classes (1, 2, 5) in blocks of a few voxels over background, so that interpolated indicators pass and miss 0.5 and two
    classes meet"""
    rng = np.random.default_rng(seed + 7 * int(np.prod(shape)))
    coarse = rng.choice(np.array([0, 1, 2, 5], np.uint8), size=[(s + 1) // 2 for s in shape], p=[0.4, 0.25, 0.2, 0.15])
    for ax in range(3):
        coarse = np.repeat(coarse, 2, axis=ax)
    return np.ascontiguousarray(coarse[:shape[0], :shape[1], :shape[2]])


def has_exact_tie(n, m, align):
    """does any coordinate of the axis lie exactly half way between two voxels (where the nearest rule is this project's own)"""
    from fractions import Fraction
    for o in range(m):
        if align == "corner":
            c = Fraction(0) if m == 1 else Fraction(o * (n - 1), m - 1)
        else:
            c = min(max(Fraction((2 * o + 1) * n, 2 * m) - Fraction(1, 2), Fraction(0)), Fraction(n - 1))
        if (c - Fraction(1, 2)).denominator == 1:
            return True
    return False
