"""A numpy restatement of rpnet_amd.morphology and the case tables shared by tests/test_host_morphology.py and
tests/test_gpu_morphology.py (numpy only).

The restatement is the definition, not the kernels' route: the ball is built offset by offset by its rule, a dilation is an explicit OR
and an erosion an explicit AND over the shifted copies of the object, with the stated values outside the volume.  tests/
test_host_morphology.py pins it to scipy.ndimage and to the thresholded distance transform; the GPU tests compare with it for equality.

`route_apply` restates the kernels' route instead (the capped separable transform, the fused threshold, the write-back rule) and takes
a `defect`: the host tests seed the mistakes that route can make and require the checks to notice each of them."""
import functools
import math

import numpy as np

ERODE, DILATE, OPEN, CLOSE = 0, 1, 2, 3
OPS = (ERODE, DILATE, OPEN, CLOSE)
OP_NAMES = {ERODE: "erode", DILATE: "dilate", OPEN: "opening", CLOSE: "closing"}

# tile widths of the y / z passes (csrc/morph.hip): the voxel ball in int32 64 columns for lines up to 128 voxels (32 to 256, 16 to 512,
# 8 to 1024), the millimetre ball in fp64 32 columns up to 128 (16 to 256, 8 to 1024, the LDS of a tile passing 32 KiB above 512)
ONE = [(1, 1, 1)]
LINES = [(1, 1, 37), (37, 1, 1), (1, 37, 1), (1, 9, 11), (7, 1, 11), (7, 9, 1)]
TILES_VOX = [(3, 5, 65), (3, 5, 130), (2, 129, 33), (2, 257, 17)]
TILES_MM = [(3, 5, 33), (3, 5, 66), (2, 129, 17), (2, 257, 9), (2, 513, 9), (513, 2, 9)]
LIMIT = [(1024, 3, 5), (3, 1024, 5), (3, 5, 1024)]
SMALL = [(6, 9, 10)]
RHOS = [1, 2, 3, 4, 5, 8, 9, 50]
MM = (2.5, 0.8, 0.8)


# ------------------------------------------------------------------------------------------------- the ball
def _clip(reach, n):
    """offsets beyond the extent add nothing: an offset of n voxels points outside from every voxel, and the ball holds it whenever it
    holds a longer one along the same axis"""
    return min(int(reach), int(n)) if n is not None else int(reach)


def voxel_ball(rho, shape=None, per_slice=False):
    """the offsets (dz, dy, dx) with dz^2 + dy^2 + dx^2 <= rho (per slice: dz = 0), clipped to the extents of `shape`"""
    r = math.isqrt(int(rho))
    rz, ry, rx = (_clip(r, n) for n in (shape or (None, None, None)))
    rz = 0 if per_slice else rz
    return [(dz, dy, dx) for dz in range(-rz, rz + 1) for dy in range(-ry, ry + 1) for dx in range(-rx, rx + 1)
            if dz * dz + dy * dy + dx * dx <= rho]


def mm_weights(spacing):
    """w = s * s, rounded once"""
    return tuple(np.float64(s) * np.float64(s) for s in spacing)


def mm_cost(w, dz, dy, dx):
    """fl(fl(fl(wx dx^2) + fl(wy dy^2)) + fl(wz dz^2)): every numpy float64 operation is one rounding"""
    return (w[2] * np.float64(dx * dx) + w[1] * np.float64(dy * dy)) + w[0] * np.float64(dz * dz)


def mm_ball(spacing, r, shape, per_slice=False):
    """the offsets whose rounded cost is <= fl(r * r) under the spacing (sz, sy, sx)"""
    w, r2 = mm_weights(spacing), np.float64(r) * np.float64(r)
    reach = []
    for a, n in enumerate(shape):
        o = 0
        while o < n and w[a] * np.float64((o + 1) * (o + 1)) <= r2:
            o += 1
        reach.append(o)
    if per_slice:
        reach[0] = 0
    return [(dz, dy, dx) for dz in range(-reach[0], reach[0] + 1) for dy in range(-reach[1], reach[1] + 1)
            for dx in range(-reach[2], reach[2] + 1) if mm_cost(w, dz, dy, dx) <= r2]


def structure_of(offsets):
    """the offsets as a centred boolean structuring element for scipy.ndimage"""
    r = [max(abs(o[a]) for o in offsets) for a in range(3)]
    s = np.zeros([2 * v + 1 for v in r], dtype=bool)
    for dz, dy, dx in offsets:
        s[dz + r[0], dy + r[1], dx + r[2]] = True
    return s


# ------------------------------------------------------------------------------------------------- the operations
def _shifted(X, offsets, outside):
    """yield, for every offset o, the array v -> X[v + o] with `outside` beyond the volume"""
    r = [max(abs(o[a]) for o in offsets) for a in range(3)]
    P = np.pad(X, [(v, v) for v in r], constant_values=outside)
    D, H, W = X.shape
    for dz, dy, dx in offsets:
        yield P[r[0] + dz:r[0] + dz + D, r[1] + dy:r[1] + dy + H, r[2] + dx:r[2] + dx + W]


def dilate_ref(X, offsets):
    """{v : some s in X with v - s in B}: the ball is symmetric, so this is the OR over o of X[v + o]; outside is background"""
    X = np.asarray(X, dtype=bool)
    out = np.zeros(X.shape, dtype=bool)
    for s in _shifted(X, offsets, False):
        out |= s
    return out


def erode_ref(X, offsets, border=1):
    """{v : every o in B has v + o in X or outside}: the AND over o of X[v + o] with `border` outside"""
    X = np.asarray(X, dtype=bool)
    out = np.ones(X.shape, dtype=bool)
    for s in _shifted(X, offsets, bool(border)):
        out &= s
    return out


def binary_ref(X, op, offsets, border=1):
    if op == ERODE:
        return erode_ref(X, offsets, border)
    if op == DILATE:
        return dilate_ref(X, offsets)
    if op == OPEN:
        return dilate_ref(erode_ref(X, offsets, border), offsets)
    return erode_ref(dilate_ref(X, offsets), offsets, border)


def write_back(vol, cls, result):
    """the label-volume rule -> (uint8 volume, int64 {before, after, added, removed})"""
    vol = np.asarray(vol)
    was = vol == cls
    gain, loss = result & ~was & (vol == 0), was & ~result
    out = vol.astype(np.int64).astype(np.uint8)
    out[gain] = cls
    out[loss] = 0
    return out, np.array([was.sum(), (out == cls).sum(), gain.sum(), loss.sum()], dtype=np.int64)


def ball_of(radius, shape, spacing=None, per_slice=False):
    """the offsets of a `radius` option of rpnet_amd.morphology: voxels, ('rho', n) or (x, 'mm')"""
    if isinstance(radius, tuple) and radius[1] == "mm":
        return mm_ball(spacing, radius[0], shape, per_slice)
    rho = radius[1] if isinstance(radius, tuple) else int(math.floor(float(radius) * float(radius)))
    return voxel_ball(rho, shape, per_slice)


def ref_apply(vol, cls, op, radius, spacing=None, per_slice=False, erode_border=1):
    """one call of rpnet_amd.morphology on one class -> (uint8 volume, statistics row)"""
    vol = np.asarray(vol)
    offsets = ball_of(radius, vol.shape, spacing, per_slice)
    return write_back(vol, cls, binary_ref(vol == cls, op, offsets, erode_border))


def ref_counts(out, truth, cls=1):
    p, t = np.asarray(out) == cls, np.asarray(truth) == cls
    return np.array([(p & t).sum(), p.sum(), t.sum()], dtype=np.int64)


# ------------------------------------------------------------------------------------------------- the kernels' route
def _capped_transform(seeds, w, lim, cap, per_slice, defect):
    """min(cap, min over seeds of the rounded cost), pass by pass as csrc/morph.hip runs them: x (the nearest seed of the line within
    the ball, else cap), then y and z as out[i] = min(in[i], min_j (in[j] + w (i - j)^2))"""
    g = np.full(seeds.shape, cap, dtype=np.float64)
    pos = np.arange(seeds.shape[2])
    for j in range(seeds.shape[2]):
        c = w[2] * ((pos - j) ** 2).astype(np.float64)
        np.minimum(g, np.where(seeds[..., j:j + 1] & (c < cap), c, cap), out=g)
    for axis in (1, 0):
        if seeds.shape[axis] == 1 or (axis == 0 and (per_slice or defect == "no z pass")):
            continue
        g = np.moveaxis(g, axis, -1)
        out, pos = g.copy(), np.arange(g.shape[-1])
        for j in range(g.shape[-1]):
            c = w[axis] * ((pos - j) ** 2).astype(np.float64)
            np.minimum(out, np.where(c < cap, g[..., j:j + 1] + c, cap), out=out)
        g = np.moveaxis(out, -1, axis)
    return np.ascontiguousarray(g)


def route_apply(vol, cls, op, radius, spacing=None, per_slice=False, erode_border=1, defect=None):
    """the same call by the kernels' route, with one seeded `defect` (None: none): '< for <=', 'outside is background', 'no z pass',
    'cap off by one', 'overwrite classes', 'swap added removed'"""
    vol = np.asarray(vol)
    if isinstance(radius, tuple) and radius[1] == "mm":
        w, lim = mm_weights(spacing), np.float64(radius[0]) * np.float64(radius[0])
        cap = np.nextafter(lim, np.inf)
    else:
        rho = radius[1] if isinstance(radius, tuple) else int(math.floor(float(radius) * float(radius)))
        w, lim = (np.float64(1.0),) * 3, np.float64(rho)
        cap = lim + 1.0
    if defect == "cap off by one":
        cap = lim
    inside = (lambda d: d < lim) if defect == "< for <=" else (lambda d: d <= lim)

    def reach(a):
        o = 0
        while o < vol.shape[a] and w[a] * np.float64((o + 1) * (o + 1)) <= lim:
            o += 1
        return o

    def dil(X):
        return inside(_capped_transform(X, w, lim, cap, per_slice, defect))

    def ero(X):
        out = ~inside(_capped_transform(~X, w, lim, cap, per_slice, defect))
        if not erode_border or defect == "outside is background":
            idx = np.indices(vol.shape)
            for a in ((1, 2) if per_slice else (0, 1, 2)):
                o = reach(a)
                out &= (idx[a] >= o) & (vol.shape[a] - 1 - idx[a] >= o)
        return out

    X = vol == cls
    res = {ERODE: lambda: ero(X), DILATE: lambda: dil(X), OPEN: lambda: dil(ero(X)), CLOSE: lambda: ero(dil(X))}[op]()
    if defect == "overwrite classes":
        out = vol.astype(np.int64).astype(np.uint8)
        gain, loss = res & ~X, X & ~res
        out[gain] = cls
        out[loss] = 0
        return out, np.array([X.sum(), (out == cls).sum(), gain.sum(), loss.sum()], dtype=np.int64)
    out, row = write_back(vol, cls, res)
    if defect == "swap added removed":
        row = row[[0, 1, 3, 2]]
    return out, row


DEFECTS = ["< for <=", "outside is background", "no z pass", "cap off by one", "overwrite classes", "swap added removed"]


# ------------------------------------------------------------------------------------------------- contents
def noise(shape, density=0.31, seed=0):
    rs = np.random.RandomState(7000 + seed + sum(shape))
    return (rs.rand(*shape) < density).astype(np.uint8)


def box(shape):
    """a box in the middle, away from every face where the axis has room"""
    a = np.zeros(shape, np.uint8)
    lo = [s // 4 for s in shape]
    hi = [max(l + 1, s - s // 4) for l, s in zip(lo, shape)]
    a[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 1
    return a


def face(shape, f):
    """a slab of two voxels (one where the axis is short) on face f of 0..5: -z, +z, -y, +y, -x, +x"""
    a = np.zeros(shape, np.uint8)
    axis, far = f // 2, f % 2
    t = min(2, shape[axis])
    sl = [slice(None)] * 3
    sl[axis] = slice(shape[axis] - t, None) if far else slice(0, t)
    a[tuple(sl)] = 1
    return a


def corners(shape):
    """a 2 x 2 x 2 block (clipped) in each of the eight corners and one voxel in the middle"""
    a = np.zeros(shape, np.uint8)
    for cz in (slice(0, 2), slice(-2, None)):
        for cy in (slice(0, 2), slice(-2, None)):
            for cx in (slice(0, 2), slice(-2, None)):
                a[cz, cy, cx] = 1
    a[shape[0] // 2, shape[1] // 2, shape[2] // 2] = 1
    return a


def contents(shape):
    """[(name, uint8 volume of one class)]"""
    rows = [("noise 0.31", noise(shape)), ("noise 0.05", noise(shape, 0.05, 1)), ("noise 0.9", noise(shape, 0.9, 2)), ("box", box(shape)),
            ("corners", corners(shape)), ("full", np.ones(shape, np.uint8)), ("empty", np.zeros(shape, np.uint8))]
    return rows + [(f"face {f}", face(shape, f)) for f in range(6)]


def ties(rho, kind):
    """one object voxel in the middle of a volume just large enough: the voxels at squared distance exactly rho and rho + 1 along an axis
    (kind 'axis', rho a square), a face diagonal ('face', rho = 2 k^2) or a space diagonal ('space', rho = 3 k^2) decide"""
    k = {"axis": math.isqrt(rho), "face": math.isqrt(rho // 2), "space": math.isqrt(rho // 3)}[kind]
    assert {"axis": k * k, "face": 2 * k * k, "space": 3 * k * k}[kind] == rho
    n = 2 * (k + 2) + 1
    a = np.zeros((n, n, n), np.uint8)
    a[n // 2, n // 2, n // 2] = 1
    return a


TIES = [(4, "axis"), (9, "axis"), (2, "face"), (8, "face"), (3, "space"), (12, "space")]


def labels(shape, seed=3):
    """a label volume of classes 0..3 in blocks with noise holes: another class adjacent to and inside what a closing of class 1 gains"""
    rs = np.random.RandomState(seed + sum(shape))
    a = np.zeros(shape, np.uint8)
    a[:, : shape[1] // 2, : shape[2] // 2] = 1
    a[:, shape[1] // 2:, : shape[2] // 2] = 2
    a[:, :, shape[2] // 2:] = np.where(rs.rand(shape[0], shape[1], shape[2] - shape[2] // 2) < 0.5, 3, 1)
    hole = rs.rand(*shape)
    a[hole < 0.15] = 0
    a[(hole >= 0.15) & (hole < 0.22)] = 2
    return a


@functools.lru_cache(maxsize=None)
def reference(shape, name, op, radius, spacing=None, per_slice=False, erode_border=1):
    """(volume, statistics row) of ref_apply on one content of the table, computed once"""
    vol = dict(contents(shape))[name]
    out, row = ref_apply(vol, 1, op, radius, spacing, per_slice, erode_border)
    out.setflags(write=False)
    row.setflags(write=False)
    return out, row
