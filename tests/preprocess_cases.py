"""A numpy restatement of rpnet_amd.preprocess (include/rpnet_prep_abi.h) and the case tables shared by tests/test_host_preprocess.py
and tests/test_gpu_preprocess.py.

The restatement is the definition, not the kernels' route: the Otsu scan operation by operation in float64 and int64 (every numpy
float64 operation is one rounding), the seeded component as a flood fill from the seed inside each slice, the box from the kept voxels.
tests/test_host_preprocess.py pins it to an exact Otsu in fractions, to scipy.ndimage.label and to np.where; the GPU tests compare with
it for equality.  Every function takes a `defect`: a deliberately wrong variant that the host tests require the checks to notice."""
import numpy as np
from scipy import ndimage

from tests import morphology_cases as MX
from tests import postprocess_cases as PX

BINS = 128
SHAPES = [(1, 1, 1), (1, 9, 11), (7, 1, 11), (7, 9, 1), (5, 33, 65), (10, 66, 130), (1, 1, 1024), (2, 1024, 1), (1024, 1, 2)]
TILE_SHAPES = [(5, 33, 65), (10, 66, 130)]
THRESHOLD_DEFECTS = ("ge_at_the_bin", "kstar_off_by_one", "last_maximum")
SEED_DEFECTS = ("z_link", "seed_swapped")
BOX_DEFECTS = ("inclusive_crop", "count_at_fill")


# --------------------------------------------------------------------------------------------------------------- threshold
def otsu_scan(counts, defect=None):
    """steps 6 to 8 on the 128 int64 counts -> (k*, [val(k) or None for k in 0..126])"""
    c = np.asarray(counts, dtype=np.int64)
    N, w, m = int(c.sum()), np.cumsum(c), np.cumsum(np.arange(BINS, dtype=np.int64) * c)
    best, ks, vals = -1.0, -1, []
    for k in range(BINS - 1):
        if not 0 < int(w[k]) < N:
            vals.append(None)
            continue
        num = np.float64(int(m[BINS - 1]) * int(w[k]) - int(m[k]) * N)           # exact: below 2^53
        val = (num * num) / (np.float64(int(w[k])) * np.float64(N - int(w[k])))
        vals.append(val)
        if val > best or (defect == "last_maximum" and val == best):
            best, ks = val, k
    return ks, vals


def slice_bins(s):
    """steps 1 to 5 of one slice -> (bins int64 with -1 for non-finite voxels, lo, hi, n_finite); bins is None without a scan"""
    v = np.asarray(s).astype(np.float64)
    fin = np.isfinite(v)
    nf = int(fin.sum())
    if nf == 0:
        return None, np.float64(0.0), np.float64(0.0), 0
    lo, hi = v[fin].min() + 0.0, v[fin].max() + 0.0                                 # a zero of either sign is +0
    if hi == lo:
        return None, lo, hi, nf
    scale = np.float64(BINS) / (hi - lo)
    b = np.full(v.shape, -1, dtype=np.int64)
    b[fin] = np.minimum(BINS - 1, ((v[fin] - lo) * scale).astype(np.int64))
    return b, lo, hi, nf


def ref_threshold(vol, threshold="otsu", defect=None):
    """threshold_mask -> (uint8 mask, int64 [D,4], float64 [D,3])"""
    vol = np.asarray(vol)
    D = vol.shape[0]
    mask, rows, frows = np.zeros(vol.shape, np.uint8), np.zeros((D, 4), np.int64), np.zeros((D, 3), np.float64)
    for z in range(D):
        b, lo, hi, nf = slice_bins(vol[z])
        k = -1
        if threshold != "otsu":
            with np.errstate(invalid="ignore"):
                mask[z] = vol[z].astype(np.float64) > np.float64(threshold)
            thr = np.float64(threshold)
        else:
            if b is not None:
                k, _ = otsu_scan(np.bincount(b[b >= 0], minlength=BINS), defect)
                cut = k + 1 if defect == "kstar_off_by_one" else k
                mask[z] = (b >= cut) & (b >= 0) if defect == "ge_at_the_bin" else b > cut
            thr = lo + np.float64(k + 1) * ((hi - lo) / np.float64(BINS))
        rows[z] = (nf, k, int(mask[z].sum()), 0)
        frows[z] = (lo, hi, thr)
    return mask, rows, frows


# -------------------------------------------------------------------------------------------------------- seeded component
def flood(obj, seed, connectivity, z_link=False):
    """the pixels of the boolean volume `obj` connected to the seed pixel of their own slice: grown from the seed one neighbour step at
    a time until nothing is gained"""
    sy, sx = seed
    region = np.zeros(obj.shape, bool)
    region[:, sy, sx] = obj[:, sy, sx]
    steps = [(0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    if connectivity == 8:
        steps += [(0, 1, 1), (0, 1, -1), (0, -1, 1), (0, -1, -1)]
    if z_link:
        steps += [(1, 0, 0), (-1, 0, 0)]
    while True:
        P = np.pad(region, 1)
        grown = region.copy()
        for dz, dy, dx in steps:
            grown |= P[1 + dz:1 + dz + obj.shape[0], 1 + dy:1 + dy + obj.shape[1], 1 + dx:1 + dx + obj.shape[2]]
        grown &= obj
        if (grown == region).all():
            return region
        region = grown


def ref_seeded(mask, cls=1, seed=None, connectivity=4, defect=None):
    """seeded_component on one class -> (uint8 volume, int64 [D,4] {seed_hit, voxels_before, voxels_kept, n_components})"""
    mask = np.asarray(mask)
    D, H, W = mask.shape
    sy, sx = (H // 2, W // 2) if seed is None else seed
    if defect == "seed_swapped":
        sy, sx = min(sx, H - 1), min(sy, W - 1)
    obj = mask == cls
    keep = flood(obj, (sy, sx), connectivity, z_link=defect == "z_link")
    out = mask.copy()
    out[obj & ~keep] = 0
    structure = ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2)
    rows = np.array([[int(obj[z, sy, sx]), int(obj[z].sum()), int(keep[z].sum()), ndimage.label(obj[z], structure=structure)[1]] for z in range(D)],
                    np.int64).reshape(D, 4)
    return out, rows


# ------------------------------------------------------------------------------------------------------------ mask and box
def ref_mask_bbox(img, mask, fill=-1024, defect=None):
    """mask_bbox -> (masked image, int64 [8] {zmin, zmax, ymin, ymax, xmin, xmax, n_kept, n_mask})"""
    img, m = np.asarray(img), np.asarray(mask) != 0
    out = np.where(m, img, np.asarray(fill, dtype=img.dtype))
    with np.errstate(invalid="ignore"):
        above = img.astype(np.float64) >= np.float64(fill) if defect == "count_at_fill" else img.astype(np.float64) > np.float64(fill)
    kept = m & above
    row = np.full(8, -1, np.int64)
    if kept.any():
        row[0:6] = [f(kept.nonzero()[a]) for a in range(3) for f in (np.min, np.max)]
    row[6], row[7] = kept.sum(), m.sum()
    return out, row


def ref_crop(row, reference_crop=True, defect=None):
    """(y0, y1, x0, x1) of the crop: half-open at ymax / xmax as the reference cuts, or including them"""
    extra = 0 if reference_crop and defect != "inclusive_crop" else 1
    return int(row[2]), int(row[3]) + extra, int(row[4]), int(row[5]) + extra


# --------------------------------------------------------------------------------------------------------------- the chain
def ref_body_mask(vol, radius=7, threshold="otsu", seed=None, connectivity=4, hole_connectivity=4, erode_border=1):
    """body_mask by the restatements of its stages -> (mask, tables as numpy arrays)"""
    m, rows, frows = ref_threshold(vol, threshold)
    m, closing = MX.ref_apply(m, 1, MX.CLOSE, radius, None, True, erode_border)
    m, opening = MX.ref_apply(m, 1, MX.OPEN, radius, None, True, erode_border)
    m, seeds = ref_seeded(m, 1, seed, connectivity)
    m, holes = PX.ref_fill_holes(m, 1, hole_connectivity, True)
    kept = int(seeds[:, 2].sum())
    voxels = np.array([rows[:, 2].sum(), closing[1], opening[1], kept, kept + holes[2]], np.int64)
    return m, {"threshold": rows, "threshold_f": frows, "closing": closing[None], "opening": opening[None], "seed": seeds, "holes": holes[None],
               "voxels": voxels}


# ------------------------------------------------------------------------------------------------------------------- cases
def noise_image(shape, dtype=np.float32, seed=0):
    """two populations (air and tissue) with noise, a different offset and spread in every slice"""
    rng = np.random.default_rng(seed)
    D = shape[0]
    tissue = rng.random(shape) < 0.45
    base = np.where(tissue, 60.0, -950.0) + rng.normal(0, 25, shape)
    base = base * (1.0 + 0.1 * np.arange(D)).reshape(D, 1, 1) + 37.0 * np.arange(D).reshape(D, 1, 1)
    return np.clip(np.round(base * 4) / 4, -32768, 32767).astype(dtype)


def threshold_cases(dtype):
    """(name, image) of the threshold table for one element kind, every image [D, 6, 8]"""
    H, W = 6, 8
    n = H * W
    ramp = np.arange(n, dtype=np.float64).reshape(H, W)
    out = []
    const = np.full((2, H, W), 5, dtype)
    const[1] = -7
    out.append(("constant slices", const))
    two = np.where(ramp % 3 == 0, 100, -100).astype(dtype)
    out.append(("two values", np.stack([two, -two, two + 5])))
    # hi clamps to bin 127; 0, 1, .., 128 over lo = 0, hi = 128: scale is exactly 1 and every value sits on a bin edge
    edges = (np.arange(n) * 128 // (n - 1)).reshape(H, W)
    out.append(("bin edges and hi", np.stack([edges, edges * 2 - 128, (edges - 128) * 3]).astype(dtype)))
    out.append(("negative", np.stack([-(ramp ** 2) - 3, -ramp - 1000]).astype(dtype)))
    out.append(("different lo / hi per slice", np.stack([ramp * (z + 1) - 40 * z for z in range(4)]).astype(dtype)))
    out.append(("noise", noise_image((3, H, W), dtype, seed=5)))
    if dtype is np.int16:
        ext = np.where(ramp % 2 == 0, -32768, 32767).astype(np.int16)
        ext2 = ext.copy()
        ext2[1, :] = 0
        ext2[2, :3] = 32766
        out.append(("int16 limits", np.stack([ext, ext2])))
    else:
        f = np.stack([ramp, ramp, ramp, np.full((H, W), np.nan), ramp]).astype(np.float32)
        f[0, 0, 0], f[0, 1, 1], f[0, 2, 2] = np.nan, np.inf, -np.inf
        f[1, :, 0] = np.inf
        f[2, :3] = np.nan
        f[4] = np.where(ramp % 2 == 0, -0.0, 0.0)                   # zeros of both signs: hi == lo by value
        out.append(("non-finite", f))
        out.append(("fractions", np.stack([ramp * 0.1 - 1.7, np.exp(ramp / 7) * 1e-3, -ramp * 1e6]).astype(np.float32)))
    return out


def fixed_thresholds(img):
    """a fixed threshold at, just below and just above a voxel value of the image"""
    v = np.float64(np.asarray(img).astype(np.float64)[np.isfinite(np.asarray(img).astype(np.float64))].flat[3])
    return [float(v), float(np.nextafter(v, -np.inf)), float(np.nextafter(v, np.inf)), float(v) - 0.5, float(v) + 0.5]


def snake(shape, vertical=False):
    """one component per slice that winds through the whole slice in rows (or columns) two apart, joined at alternating ends: it
    crosses every tile seam in x and in y"""
    D, H, W = shape
    v = np.zeros(shape, np.uint8)
    if vertical:
        v[:, :, ::2] = 1
        for i, x in enumerate(range(1, W, 2)):
            v[:, 0 if i % 2 else H - 1, x] = 1
    else:
        v[:, ::2, :] = 1
        for i, y in enumerate(range(1, H, 2)):
            v[:, y, 0 if i % 2 else W - 1] = 1
    return v


def component_cases(shape):
    """(name, uint8 volume, seed or None) of the component table at one extent"""
    D, H, W = shape
    cy, cx = H // 2, W // 2
    out = [("empty", np.zeros(shape, np.uint8), None), ("full", np.ones(shape, np.uint8), None),
           ("noise 0.6", MX.noise(shape, 0.6), None), ("noise 0.45", MX.noise(shape, 0.45, seed=3), None)]
    if H * W <= 33 * 65:                            # the flood fill of the restatement walks a snake pixel by pixel
        out += [("snake", snake(shape), (0, 0)), ("snake vertical", snake(shape, True), (0, 0))]         # row 0 and column 0 are on it
    # the same blob in neighbouring slices, the seed on it in the even ones only: nothing may leak across z
    leak = np.zeros(shape, np.uint8)
    leak[:, max(0, cy - 2):cy + 3, max(0, cx - 2):cx + 3] = 1
    leak[1::2, cy, cx] = 0
    if H > 4 and W > 4:
        leak[1::2, max(0, cy - 1):cy + 2, max(0, cx - 1):cx + 2] = 0
    out.append(("no leak across z", leak, None))
    # a diagonal contact: one component under 8, two under 4
    diag = np.zeros(shape, np.uint8)
    diag[:, cy, cx] = 1
    if cy + 1 < H and cx + 1 < W:
        diag[:, cy + 1, cx + 1] = 1
        diag[:, cy + 1:, cx + 1] = 1
    out.append(("diagonal contact", diag, None))
    corners = np.zeros(shape, np.uint8)
    corners[:, :max(1, H // 3), :max(1, W // 3)] = 1
    corners[:, H - max(1, H // 3):, W - max(1, W // 3):] = 1
    corners[:, 0, W - 1] = corners[:, H - 1, 0] = 1
    for seed in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        out.append((f"corner seed {seed}", corners, seed))
    return out


def body_phantom(shape=(6, 96, 96), dtype=np.float32, seed=0):
    """a body on a table: an ellipse of tissue with air pockets, a detached table bar below it and a speck in a corner, in air; every
    slice a little different.  -> (image, the ellipse, the pockets, the table, the speck) as boolean volumes"""
    D, H, W = shape
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    cy, cx = 0.44 * H, 0.5 * W
    ry, rx = (0.28 + 0.004 * zz) * H, (0.38 - 0.004 * zz) * W
    body = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1
    pockets = np.zeros(shape, bool)
    for py, px, pr in ((cy - 0.1 * H, cx - 0.15 * W, 3.2), (cy + 0.08 * H, cx + 0.2 * W, 2.4), (cy, cx + 0.02 * W, 1.5)):
        pockets |= (yy - py) ** 2 + (xx - px - zz) ** 2 < pr * pr
    pockets &= body
    table = (yy >= H - 6) & (yy < H - 3) & (xx >= W // 10) & (xx < W - W // 10)
    speck = (yy >= 2) & (yy < 4) & (xx >= 3) & (xx < 5)
    img = np.where(body & ~pockets, 45.0, -1000.0) + rng.normal(0, 10, shape)
    img = np.where(table, 250.0, img)
    img = np.where(speck, 400.0, img)
    img = np.where(pockets, -930.0 + rng.normal(0, 10, shape), img)
    return np.round(img).astype(dtype), body, pockets, table, speck
