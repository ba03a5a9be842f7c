"""The numpy restatement of include/rpnet_compstat_abi.h (not product code): the dense renumbering of the sparse component labels and
the per-component table, the quantisation of the image included, in exact integers, so that `rank_restate` and `table_restate` give the
words the device must give.  `defect=` seeds one of the mistakes tests/test_host_compstat.py shows its checks would catch.  The case
tables of tests/test_gpu_compstat.py stand at the end."""
import numpy as np

CHUNK, ROW, SCAN_THREADS, SLOTS = 4096, 24, 256, 128
DEFECTS = ("seam_off_by_one", "inclusive_scan", "ties_away", "lost_hi_word", "overlap_wrong_class", "beyond_into_last_row")


def float_key(v):
    """the key of rpnet_volload_abi.h of float32 values (finite ones): -0.0 as +0.0; a set sign bit gives ~u, a clear one u | 2^31"""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).copy()
    u[u == np.uint32(0x80000000)] = 0
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key_value(k):
    k = np.asarray(k).astype(np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def sparse_labels(mask, connectivity=6):
    """the labels of rpnet_cc_label of a boolean volume: 0, or 1 + the smallest linear index of the voxel's component"""
    from scipy import ndimage
    lab, n = ndimage.label(mask, structure=ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3))
    flat = lab.ravel()
    first = np.full(n + 1, flat.size, np.int64)
    np.minimum.at(first, flat, np.arange(flat.size))
    out = np.where(flat > 0, first[flat] + 1, 0).astype(np.int32)
    return out.reshape(mask.shape)


def rank_restate(labels, defect=None):
    """-> (dense int32 [D, H, W], C, invalid): the roots are the voxels with labels[i] == i + 1, the id of a root is 1 + the number of
    roots below it, formed as the header forms it: roots counted per chunk of 4096, an exclusive scan over the chunk counts, the rank
    inside the chunk added; a label that names no root gives 0 and is counted"""
    labels = np.asarray(labels)
    flat = labels.ravel().astype(np.int64)
    n = flat.size
    root = flat == np.arange(n) + 1
    nc = (n + CHUNK - 1) // CHUNK
    padded = np.zeros(nc * CHUNK, np.int64)
    padded[:n] = root
    per = padded.reshape(nc, CHUNK)
    counts = per.sum(1)
    offsets = np.cumsum(counts) - (0 if defect == "inclusive_scan" else counts)
    inside = np.cumsum(per, 1)                              # 1-based rank of a root inside its chunk
    if defect == "seam_off_by_one":
        offsets = offsets + (np.arange(nc) > 0)             # every chunk after the first starts one too high
    rank = (offsets[:, None] + inside).ravel()[:n]
    inb = (flat >= 1) & (flat <= n)
    at = np.where(inb, flat - 1, 0)
    valid = inb & (flat[at] == flat)
    dense = np.where(valid, rank[at], 0)
    invalid = int(((flat != 0) & ~valid).sum())
    return dense.astype(np.int32).reshape(labels.shape), int(counts.sum()), invalid


def quantise(values, q, defect=None):
    """-> (k int64, summed bool): k = rint(float64(v) * 2^q), ties to even; summed where v is finite and |k| < 2^31"""
    p = np.asarray(values).astype(np.float64) * float(1 << q)          # exact: a float32 or int16 value times a power of two
    with np.errstate(invalid="ignore"):
        if defect == "ties_away":
            k = np.where(np.isfinite(p), np.sign(p) * np.floor(np.abs(p) + 0.5), p)
        else:
            k = np.rint(p)
        ok = np.isfinite(k) & (np.abs(k) < 2147483648.0)
    return np.where(ok, k, 0).astype(np.int64), ok


def empty_row(shape):
    D, H, W = shape
    return np.array([0, D, H, W, -1, -1, -1] + [0] * 10 + [0xFFFFFFFF, 0, 0, 0, 0, 0, -1], np.int64)


def group_sum(ids, values, size):
    """exact int64 sums of `values` per id (np.bincount would go through float64)"""
    out = np.zeros(size, np.int64)
    if ids.size:
        order = np.argsort(ids, kind="stable")
        sid, sval = ids[order], np.asarray(values, np.int64)[order]
        starts = np.flatnonzero(np.r_[True, sid[1:] != sid[:-1]])
        out[sid[starts]] = np.add.reduceat(sval, starts)
    return out


def overlap_of(other, other_cls):
    other = np.asarray(other).ravel()
    return other == (np.float32(other_cls) if other.dtype.kind == "f" else other_cls)


def table_restate(dense, C, image=None, q=0, other=None, other_cls=1, max_components=4096, defect=None):
    """-> (rows int64 [max_components, 24], n_beyond, invalid) of a renumbered volume whose head holds C"""
    dense = np.asarray(dense)
    D, H, W = dense.shape
    flat = dense.ravel().astype(np.int64)
    M = int(max_components)
    rows = np.stack([empty_row(dense.shape)] * M)
    bad = (flat < 0) | (flat > C)
    beyond = ~bad & (flat > M)
    take = ~bad & ~beyond & (flat > 0)
    ids_all = flat.copy()
    if defect == "beyond_into_last_row":
        take = take | beyond
        ids_all = np.minimum(ids_all, M)
    at = np.flatnonzero(take)
    ids = ids_all[at] - 1
    z, y, x = (c.astype(np.int64) for c in np.unravel_index(at, (D, H, W)))
    n = group_sum(ids, np.ones(at.size, np.int64), M)
    has = n > 0
    rows[:, 0] = n
    for col, c in ((1, z), (2, y), (3, x)):
        lo = np.full(M, 1 << 40, np.int64)
        np.minimum.at(lo, ids, c)
        hi = np.full(M, -1, np.int64)
        np.maximum.at(hi, ids, c)
        rows[has, col], rows[has, col + 3] = lo[has], hi[has]
    for col, term in ((7, z), (8, y), (9, x), (10, z * z), (11, y * y), (12, x * x), (13, z * y), (14, z * x), (15, y * x)):
        rows[:, col] = group_sum(ids, term, M)
    first = np.full(M, 1 << 40, np.int64)
    np.minimum.at(first, ids, at)
    rows[has, 23] = first[has]
    if image is not None:
        values = np.asarray(image).ravel()[at]
        k, ok = quantise(values, q, defect)
        rows[:, 16] = group_sum(ids, ok.astype(np.int64), M)
        keys = float_key(values[ok].astype(np.float32)).astype(np.int64)
        kmin = np.full(M, 1 << 40, np.int64)
        np.minimum.at(kmin, ids[ok], keys)
        kmax = np.full(M, -1, np.int64)
        np.maximum.at(kmax, ids[ok], keys)
        summed = rows[:, 16] > 0
        rows[summed, 17], rows[summed, 18] = kmin[summed], kmax[summed]
        k_ok = k[ok]
        rows[:, 19] = group_sum(ids[ok], k_ok, M)
        kk = (k_ok * k_ok).astype(np.uint64)                # |k| < 2^31: below 2^62
        rows[:, 20] = group_sum(ids[ok], (kk & np.uint64(0xFFFFFFFF)).astype(np.int64), M)
        rows[:, 21] = 0 if defect == "lost_hi_word" else group_sum(ids[ok], (kk >> np.uint64(32)).astype(np.int64), M)
    if other is not None:
        cls = other_cls + 1 if defect == "overlap_wrong_class" else other_cls
        rows[:, 22] = group_sum(ids, overlap_of(other, cls)[at].astype(np.int64), M)
    return rows, int(beyond.sum()), int(bad.sum())


def chain_restate(vol, cls=1, connectivity=6, image=None, q=0, other=None, other_cls=None, max_components=4096):
    """label -> rank -> table of the class `cls` of a volume -> (dense, rows, head [C, invalid, n_beyond, invalid of the table])"""
    vol = np.asarray(vol)
    mask = vol == (np.float32(cls) if vol.dtype.kind == "f" else cls)
    dense, C, inv = rank_restate(sparse_labels(mask, connectivity))
    rows, beyond, bad = table_restate(dense, C, image, q, other, cls if other_cls is None else other_cls, max_components)
    return dense, rows, np.array([C, inv, beyond, bad], np.int64)


# ------------------------------------------------------------------------------------------------------------------ case tables
def noise_mask(shape, density, seed):
    return np.random.RandomState(seed).rand(*shape) < density


def blob_mask(shape, seed):
    """a smooth organ around a seeded centre with a few islands beside it"""
    rng = np.random.RandomState(seed)
    grid = np.indices(shape).astype(np.float64)
    centre = [(s - 1) * (0.35 + 0.3 * rng.rand()) for s in shape]
    r2 = sum(((grid[a] - centre[a]) / max(shape[a] * 0.3, 1.0)) ** 2 for a in range(3))
    mask = r2 < 1.0
    mask |= rng.rand(*shape) < 0.01
    return mask


def checkerboard(shape):
    """every foreground voxel a 6-connected component of its own: 2048 ids in a whole chunk"""
    return (np.indices(shape).sum(0) % 2) == 0


def image_for(shape, seed, kind="f32"):
    rng = np.random.RandomState(seed)
    if kind == "i16":
        return rng.randint(-1024, 3072, size=shape).astype(np.int16)
    return (rng.standard_normal(shape) * 300.0 + 40.0).astype(np.float32)


# the smallest shapes at which the launches can go wrong: one voxel; each axis of length 1; one tile of rpnet_cc_label (4 x 32 x 64) + 1
# along y and x, which is also two chunks; 2 * tile + 2; a line of 1024 along each axis
SHAPES = [(1, 1, 1), (1, 9, 13), (7, 1, 19), (6, 11, 1), (2, 33, 65), (10, 66, 130), (1024, 1, 1), (1, 1024, 1), (1, 1, 1024)]
# one more chunk than the scan block has threads (the second tile of the scan holds one chunk): 256 * 4096 + 1 voxels in 257 chunks
SCAN_SHAPE = (257, 64, 64)
