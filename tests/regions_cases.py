"""The numpy restatement of include/rpnet_region_abi.h (not product code): the integer rows, the order-preserving key, and the float64 sums
in the chunk, lane, tree, trip and fold order of the header, so that `restate` gives the bits the device must give.  Vectorised over
chunks and lanes with a loop over the labels present.  `defect=` seeds one of the mistakes tests/test_host_regions.py shows its checks
would catch.  The case tables of tests/test_gpu_regions.py stand at the end."""
import numpy as np

CHUNK, LANES, LANE, MAX_BLOCKS, IROW, FROW = 4096, 256, 16, 1024, 20, 2
DEFECTS = ("lane8", "tree_reversed", "trips_reversed", "keys_swapped", "zy_zx_exchanged", "nonfinite_in_s1")


def float_key(v):
    """the key of rpnet_volload_abi.h of float32 values (finite ones): -0.0 as +0.0; a set sign bit gives ~u, a clear one u | 2^31"""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).copy()
    u[u == np.uint32(0x80000000)] = 0
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key_value(k):
    k = np.asarray(k).astype(np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def codes_of(labels, L):
    """per voxel the label 0 .. L-1 it holds, -1 where it holds anything else (float labels: value == float(l) for no l)"""
    flat = np.asarray(labels).ravel()
    if flat.dtype.kind == "f":
        with np.errstate(invalid="ignore"):
            ok = (flat >= 0) & (flat < L)
            whole = np.where(ok, flat, 0).astype(np.int64)
            ok &= whole.astype(flat.dtype) == flat
    else:
        whole = flat.astype(np.int64)
        ok = (whole >= 0) & (whole < L)
    return np.where(ok, whole, -1)


def tree(a, reverse=False):
    """a[..., t] = a[..., t] + a[..., t + s] for t < s, s = 128, 64, ..., 1 over the last axis of 256 -> a[..., 0]"""
    a = a.copy()
    strides = [128, 64, 32, 16, 8, 4, 2, 1]
    if reverse:         # the seeded defect: neighbours first.  a[t] += a[t + s] for t a multiple of 2 s
        for s in strides[::-1]:
            a[..., 0::2 * s] = a[..., 0::2 * s] + a[..., s::2 * s]
        return a[..., 0]
    for s in strides:
        a[..., :s] = a[..., :s] + a[..., s:2 * s]
    return a[..., 0]


def ordered_sum(terms, defect=None):
    """SUM of the header over `terms`, float64 [n] in linear order with 0.0 where a voxel does not take part"""
    n = terms.shape[0]
    lane = 8 if defect == "lane8" else LANE
    chunk = LANES * lane
    n_chunks = (n + chunk - 1) // chunk
    padded = np.zeros(n_chunks * chunk, np.float64)
    padded[:n] = terms
    per = padded.reshape(n_chunks, LANES, lane)
    a = np.zeros((n_chunks, LANES), np.float64)
    for j in range(lane):
        a = a + per[:, :, j]
    values = tree(a, reverse=defect == "tree_reversed")
    G = min(n_chunks, MAX_BLOCKS)
    iters = (n_chunks + G - 1) // G
    trips = np.zeros(iters * G, np.float64)
    trips[:n_chunks] = values
    trips = trips.reshape(iters, G)
    P = np.zeros(G, np.float64)
    for it in (range(iters - 1, -1, -1) if defect == "trips_reversed" else range(iters)):
        P = P + trips[it]
    rounds = (G + LANES - 1) // LANES
    folded = np.zeros(rounds * LANES, np.float64)
    folded[:G] = P
    folded = folded.reshape(rounds, LANES)
    a = np.zeros(LANES, np.float64)
    for r in range(rounds):
        a = a + folded[r]
    return tree(a, reverse=defect == "tree_reversed")


def empty_row(shape):
    D, H, W = shape
    return np.array([0, D, H, W, -1, -1, -1] + [0] * 10 + [0xFFFFFFFF, 0, 0], np.int64)


def restate(labels, image=None, lo=1, L=2, defect=None):
    """-> (rows_i int64 [L, 20], rows_f float64 [L, 2], n_outside) of a label volume [D, H, W] and an image (None, float32 or int16)"""
    labels = np.asarray(labels)
    D, H, W = labels.shape
    code = codes_of(labels, L)
    rows_i = np.stack([empty_row(labels.shape) for _ in range(L)])
    rows_f = np.zeros((L, FROW), np.float64)
    values = None if image is None else np.asarray(image).ravel().astype(np.float32)
    for l in sorted(set(np.unique(code).tolist()) - {-1}):
        if l < lo:
            continue
        at = np.flatnonzero(code == l)
        z, y, x = (c.astype(np.int64) for c in np.unravel_index(at, (D, H, W)))
        row = rows_i[l]
        row[0] = at.size
        row[1:4] = z.min(), y.min(), x.min()
        row[4:7] = z.max(), y.max(), x.max()
        row[7:10] = z.sum(), y.sum(), x.sum()
        row[10:13] = (z * z).sum(), (y * y).sum(), (x * x).sum()
        zy, zx = (z * y).sum(), (z * x).sum()
        row[13:16] = (zx, zy, (y * x).sum()) if defect == "zy_zx_exchanged" else (zy, zx, (y * x).sum())
        if values is None:
            continue
        inside = values[at]
        finite = np.isfinite(inside)
        row[16] = int(finite.sum())
        if finite.any():
            keys = float_key(inside[finite])
            if defect == "keys_swapped":        # the order of the raw patterns: right for values >= 0, reversed below
                raw = inside[finite].view(np.uint32)
                keys = np.array([float_key(inside[finite][[np.argmin(raw)]])[0], float_key(inside[finite][[np.argmax(raw)]])[0]], np.uint32)
                row[17], row[18] = int(keys[0]), int(keys[1])
            else:
                row[17], row[18] = int(keys.min()), int(keys.max())
        take = np.zeros(code.shape, bool)
        take[at[finite]] = True
        dv = values.astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            s1_terms = np.where(take | ((code == l) & (defect == "nonfinite_in_s1")), dv, 0.0)
            rows_f[l, 0] = ordered_sum(s1_terms, defect)
            rows_f[l, 1] = ordered_sum(np.where(take, dv * dv, 0.0), defect)
    return rows_i, rows_f, int((code == -1).sum())


# ------------------------------------------------------------------------------------------------------------------ case tables
def blob_labels(shape, L, seed):
    """a label map of smooth regions: label 0 the background, labels 1 .. L-1 nested ellipsoids around a seeded centre, so that most
    waves hold one label and the borders hold several"""
    rng = np.random.RandomState(seed)
    grid = np.indices(shape).astype(np.float64)
    centre = [(s - 1) * (0.35 + 0.3 * rng.rand()) for s in shape]
    r2 = sum(((grid[a] - centre[a]) / max(shape[a] * 0.45, 1.0)) ** 2 for a in range(3))
    out = np.zeros(shape, np.uint8)
    for l in range(1, L):
        out[r2 < (1.0 - (l - 1) / max(L - 1, 1)) ** 2] = l
    return out


def noise_labels(shape, L, seed, outside=0):
    """every voxel an independent label 0 .. L-1 (+ `outside` further values that are no label)"""
    return np.random.RandomState(seed).randint(0, L + outside, size=shape).astype(np.uint8 if L + outside <= 256 else np.int32)


def image_for(shape, seed, kind="f32"):
    rng = np.random.RandomState(seed)
    if kind == "i16":
        return rng.randint(-1024, 3072, size=shape).astype(np.int16)
    return (rng.standard_normal(shape) * 300.0 + 40.0).astype(np.float32)


# the smallest shapes at which the pass can go wrong: one voxel; the lane edge (15, 16, 17); a lane that straddles a row end and a slice
# end (W = 17, H * W = 51); the chunk edge (4095, 4096, 4097); each axis of length 1; a line of 1024 along each axis
SHAPES = [(1, 1, 1), (1, 1, 15), (1, 1, 16), (1, 1, 17), (5, 3, 17), (1, 5, 819), (1, 4, 1024), (1, 17, 241), (1, 9, 13), (7, 1, 19), (6, 11, 1),
          (1024, 1, 1), (1, 1024, 1), (1, 1, 1024), (3, 37, 41)]
TWO_TRIPS = (5, 1024, 821)          # 1027 chunks: blocks 0, 1 and 2 make a second trip
