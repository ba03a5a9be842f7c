"""The definitions of include/rpnet_volload_abi.h restated in numpy, and the case tables of tests/test_host_volload.py and
tests/test_gpu_volload.py.  Nothing here calls the reader: the restatement is the kernels' index arithmetic and float32 operation
sequence, and tests/test_host_volload.py pins it to FewshotVolumeReader.load_image_and_mask and to numpy.percentile bit for bit.

The percentile is numpy's method 'linear' as numpy 2.2.6 computes it for a float32 array (the version the host test ran against): the
virtual index (n - 1) * (q / 100) is formed in float32, q / 100 included, so at the size of a real volume it is a multiple of 0.5 and
its floor or its fraction differ from those of the float64 index (n - 1) * 0.995; the host reader calls that numpy, and the device must give the reader's bits."""
import numpy as np

NUMPY_PINNED = "2.2.6"
F = np.float32

# every defect a test can switch on: each must make at least one row of tests/test_host_volload.py fail
DEFECTS = ("rank_not_clamped", "round_not_floor", "lerp_f64", "fused_map", "extra_pixel_near", "hi_inclusive", "index_f64")

# (file shape, num_slice, num_y, num_x): crop and pad on each axis, both odd pad parities, num_slice below and above D, num_x / num_y
# below and above W / H
FILE_SHAPES = ((1, 1, 1), (17, 33, 31), (22, 44, 40), (16, 300, 280))
# the padded extents are multiples of 16, so an odd pad (the extra pixel at the far end) arises only under an odd crop_size: [33, 47]
CROPS = ([32, 32], [256, 256], [33, 47])
WINDOWS = {(1, 1, 1): ((4, 8, 8),),
           (17, 33, 31): ((40, 64, 64), (12, 20, 18)),
           (22, 44, 40): ((20, 40, 40), (30, 30, 50)),
           (16, 300, 280): ((16, 512, 512), (10, 270, 100))}
GEOMETRY_ROWS = tuple((shape, win, crop) for shape in FILE_SHAPES for win in WINDOWS[shape] for crop in CROPS)
HU = (-1024, 3072)


def config(window, crop, pad_value=-1024, hu=HU):
    ns, ny, nx = window
    return {"num_slice": ns, "num_y": ny, "num_x": nx, "crop_size": list(crop), "pad_value": pad_value, "HU_range": list(hu)}


# ------------------------------------------------------------------------------------------------------------- geometry
def ref_geometry(shape, window, crop, defect=None):
    D, H, W = shape
    ns, ny, nx = window
    ch, cw = crop
    g = {"nz": min(D, ns), "y1": max(0, H // 2 - ny // 2), "y2": min(H, H // 2 + ny // 2), "x1": max(0, W // 2 - nx // 2),
         "x2": min(W, W // 2 + nx // 2), "ch": ch, "cw": cw}
    g["pD"], g["pH"], g["pW"] = (-(-n // 16) * 16 for n in (g["nz"], g["y2"] - g["y1"], g["x2"] - g["x1"]))
    g["rh"], g["rw"] = min(ch, g["pH"]), min(cw, g["pW"])
    g["cy"], g["cx"] = g["pH"] // 2 - g["rh"] // 2, g["pW"] // 2 - g["rw"] // 2
    g["pt"], g["pl"] = (ch - g["rh"]) // 2, (cw - g["rw"]) // 2
    if defect == "extra_pixel_near":
        g["pt"], g["pl"] = (ch - g["rh"]) - g["pt"], (cw - g["rw"]) - g["pl"]
    return g


def ref_range(mask, shape_window):
    """(first, last, count) of the non-zero voxels inside the window; (-1, -1, 0) where there is none.  mask [D,H,W]"""
    g = shape_window
    win = mask[:g["nz"], g["y1"]:g["y2"], g["x1"]:g["x2"]]
    zs = np.nonzero(win)[0]
    return (int(zs.min()), int(zs.max()), int(zs.size), 0) if zs.size else (-1, -1, 0, 0)


def ref_gather(src, g, lo, hi, pad_value):
    """float32 [hi - lo, ch, cw] by the index arithmetic of the header, one output voxel at a time (vectorised over the axes)"""
    out = np.full((hi - lo, g["ch"], g["cw"]), F(pad_value), np.float32)
    oy, ox = np.arange(g["ch"]), np.arange(g["cw"])
    ry, rx = oy - g["pt"], ox - g["pl"]
    py, px = ry + g["cy"], rx + g["cx"]
    ok_y = (ry >= 0) & (ry < g["rh"]) & (py < g["y2"] - g["y1"])
    ok_x = (rx >= 0) & (rx < g["rw"]) & (px < g["x2"] - g["x1"])
    sy, sx = (g["y1"] + py)[ok_y], (g["x1"] + px)[ok_x]
    block = src[lo:hi][:, sy][:, :, sx].astype(np.float32)
    out[np.ix_(np.arange(hi - lo), oy[ok_y], ox[ok_x])] = block
    return out


# ----------------------------------------------------------------------------------------------------------- selection
def ref_key(x):
    """the order-preserving uint32 key of float32 values: NaN -> 0xFFFFFFFF, -0.0 as +0.0, negatives inverted, the sign flipped"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).copy()
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    u[u == 0x80000000] = 0
    neg = (u & 0x80000000) != 0
    key = np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    key[nan] = 0xFFFFFFFF
    return key


def ref_unkey(key):
    key = np.asarray(key, np.uint32)
    return np.where(key & 0x80000000, key & 0x7FFFFFFF, ~key).astype(np.uint32).view(np.float32)


def ref_select(x, ranks):
    """(value of rank k0, value of rank k1, number of NaNs) by the radix selection of the header: four passes of 8 bits over the keys"""
    key = ref_key(np.ravel(x))
    vals = []
    for k in ranks:
        rem, prefix, keep = int(k), 0, key
        for shift in (24, 16, 8, 0):
            hist = np.bincount((keep >> shift) & 255, minlength=256)
            cum = np.cumsum(hist)
            digit = int(np.searchsorted(cum, rem, side="right"))
            rem -= int(cum[digit] - hist[digit])
            prefix = (prefix << 8) | digit
            keep = keep[((keep >> shift) & 255) == digit]
        vals.append(ref_unkey(np.array([prefix], np.uint32))[0])
    return vals[0], vals[1], int((key == 0xFFFFFFFF).sum())


def ref_rank(n, q=99.5, defect=None):
    """(k0, k1, g) of numpy.percentile(x, q) for a float32 x of n values: numpy >= 2 forms the virtual index in float32"""
    if defect == "index_f64":
        v = (n - 1) * (q / 100.0)
    else:
        qq = F(q) / F(100)
        v = F(n - 1) * qq
    if v >= n - 1 and defect != "rank_not_clamped":
        return n - 1, n - 1, F(0)
    if v < 0:
        return 0, 0, F(0)
    k = np.round(v) if defect == "round_not_floor" else np.floor(v)
    return int(k), int(k) + 1, F(v - k)          # v < n - 1, so k + 1 <= n - 1: the clamp is the branch above


def ref_top(a, b, g, n_nan, defect=None):
    """numpy's _lerp in float32, and its rule that one NaN makes the percentile a NaN"""
    with np.errstate(invalid="ignore", over="ignore"):
        if defect == "lerp_f64":
            a64, b64, g64 = float(a), float(b), float(g)
            top = F(b64 - (b64 - a64) * (1 - g64) if g64 >= 0.5 else a64 + (b64 - a64) * g64)
        else:
            a, b, g = F(a), F(b), F(g)
            d = F(b - a)
            top = F(b - F(d * F(F(1) - g))) if g >= F(0.5) else F(a + F(d * g))
    return F(np.nan) if n_nan else top


def ref_percentile(x, q=99.5, defect=None):
    x = np.ravel(np.asarray(x, np.float32))
    k0, k1, g = ref_rank(x.size, q, defect)
    s = np.sort(x)                                  # numpy's sort: NaNs last; ref_select gives the same values (tested)
    a, b = s[k0] + F(0), s[k1] + F(0)               # a zero is +0.0, as the selection returns it; the defect that does not clamp k + 1 reads past the end here
    return ref_top(a, b, g, int(np.isnan(x).sum()), defect)


def ref_map(x, top, minimum, maximum, defect=None):
    """v > top -> top; v > maximum -> maximum; v < minimum -> minimum; ((v - minimum) / max(1, maximum - minimum)) * 2 - 1, float32"""
    mn, mx, den = F(minimum), F(maximum), F(max(1, maximum - minimum))
    v = np.array(x, np.float32, copy=True)
    with np.errstate(invalid="ignore"):
        v[v > top] = top
        v[v > mx] = mx
        v[v < mn] = mn
        r = ((v - mn) / den).astype(np.float32)
        if defect == "fused_map":
            return (r.astype(np.float64) * 2 - 1).astype(np.float32)        # one rounding, as an FMA gives
        return (r * F(2)).astype(np.float32) - F(1)


def ref_normalize(x, minimum, maximum, top_percent=0.5, defect=None):
    return ref_map(x, ref_percentile(x, 100.0 - top_percent, defect), minimum, maximum, defect)


def ref_load(image, mask, cfg, defect=None):
    """(image, mask) float32 [d, ch, cw] as the reader's load_image_and_mask gives them for the file arrays `image` and `mask` [D,H,W]"""
    window = (cfg["num_slice"], cfg["num_y"], cfg["num_x"])
    g = ref_geometry(image.shape, window, cfg["crop_size"], defect)
    first, last, count, _ = ref_range(mask, g)
    if count == 0:
        raise ValueError("empty mask")
    hi = last + 1 if defect == "hi_inclusive" else last
    out_mask = ref_gather(mask, g, first, hi, 0.0)
    out_image = ref_gather(image, g, first, hi, cfg["pad_value"])
    if out_image.size == 0:
        return out_image, out_mask
    return ref_normalize(out_image, cfg["HU_range"][0], cfg["HU_range"][1], defect=defect), out_mask


# ---------------------------------------------------------------------------------------------------------------- data
def file_volume(shape, dtype, seed=0):
    """a CT-like volume: 60 % of the voxels -1024, soft tissue, a few outliers above the HU window"""
    rs = np.random.RandomState(seed)
    v = rs.normal(40.0, 60.0, shape)
    v[rs.rand(*shape) < 0.6] = -1024.0
    v[rs.rand(*shape) > 0.997] = 3500.0
    if np.dtype(dtype) == np.int16:
        return np.clip(np.rint(v), -1024, 4000).astype(np.int16)
    return (v + rs.rand(*shape) * 0.5).astype(np.float32)


def file_mask(shape, dtype, z_first, z_last, seed=0):
    """a mask whose annotated slices are z_first .. z_last (both hold a voxel inside every window of the tables: the centre voxel);
    a float mask holds fractional values"""
    D, H, W = shape
    rs = np.random.RandomState(seed + 100)
    m = np.zeros(shape, np.float32)
    m[z_first:z_last + 1] = rs.rand(z_last + 1 - z_first, H, W) < 0.3
    m[z_first, H // 2 - (H > 1), W // 2 - (W > 1)] = 1
    m[z_last, H // 2 - (H > 1), W // 2 - (W > 1)] = 1
    if np.dtype(dtype) == np.float32:
        return (m * (0.25 + 0.5 * rs.rand(*shape))).astype(np.float32)
    return (m * (1 if np.dtype(dtype) == np.uint8 else 3)).astype(dtype)


def selection_cases():
    """{name: float32 array}: the rows of the selection tests"""
    rs = np.random.RandomState(5)
    c = {}
    for n in (1, 2, 200, 201, 202):
        c[f"n{n}"] = rs.normal(0, 100, n).astype(np.float32)
    c["all_equal"] = np.full(777, 3.25, np.float32)
    ties = np.sort(rs.randint(0, 4, 1000)).astype(np.float32)
    ties[990:] = 7.0
    ties[985:996] = 5.0                             # the 99.5th percentile of 1000 values stands between ranks 994 and 995: inside a tie
    c["ties_straddle"] = rs.permutation(ties)
    low = np.full(600, 1.0, np.float32).view(np.uint32) + rs.randint(0, 256, 600).astype(np.uint32)
    c["lowest_digit"] = low.view(np.float32)
    c["negative"] = -np.abs(rs.normal(0, 50, 999)).astype(np.float32) - 1
    c["mixed"] = rs.normal(0, 1e3, 1003).astype(np.float32)
    z = np.zeros(403, np.float32)
    z[::2] = -0.0
    z[:5] = [-1, -2, 1, 2, -3]
    c["zeros"] = z
    c["zeros_on_top"] = np.concatenate([-np.abs(rs.normal(0, 1, 300)).astype(np.float32) - 1, np.array([-0.0, 0.0, -0.0, 0.0], np.float32)])
    sub = (rs.randint(1, 1 << 22, 500).astype(np.uint32) | (rs.randint(0, 2, 500).astype(np.uint32) << 31)).view(np.float32)
    c["subnormals"] = sub
    for name, v in (("pos_inf", np.inf), ("neg_inf", -np.inf)):
        a = rs.normal(0, 1, 400).astype(np.float32)
        a[:5 if v > 0 else 399] = v                  # +inf: ranks 397, 398 are 0.x and inf ... ; -inf: all but one
        c[name + "_at_rank"] = rs.permutation(a)
    a = rs.normal(0, 1, 400).astype(np.float32)
    a[:2] = np.inf                                   # ranks 397 and 398: finite and inf -> the lerp makes inf or NaN as numpy does
    c["inf_next"] = rs.permutation(a)
    a = rs.normal(0, 1, 401).astype(np.float32)
    a[137] = np.nan
    c["one_nan"] = a
    a = rs.normal(0, 1, 64).astype(np.float32)
    a[3] = np.float32(np.nan).view(np.uint32).__or__(np.uint32(0x80000000)).view(np.float32)     # a NaN with the sign bit set
    c["negative_nan"] = a
    c["ct_like"] = file_volume((6, 40, 40), np.int16, 3).astype(np.float32).ravel()
    return c


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits_nan(a, b, zeros_by_value=False):
    """equal bit for bit, a NaN compared as a NaN; zeros_by_value: -0.0 equals +0.0 (what a selection returns for a zero)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    same = (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))
    if zeros_by_value:
        same |= (a == 0) & (b == 0)
    return a.shape == b.shape and bool(np.all(same))
