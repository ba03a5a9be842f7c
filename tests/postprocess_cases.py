"""Case tables of the post-processing tests and the numpy restatement of the two definitions of include/rpnet_ccpost_abi.h that the GPU
tests compare with (tests/test_host_postprocess.py pins it to scipy.ndimage.binary_fill_holes and to label + bincount, and shows that
seeded defects fail the same comparison).

The tile of the shared labelling phases is 4 x 32 x 64 voxels (z, y, x): the extents are one voxel, one past a tile in every axis
(tile + 1), 2 * tile + 2, and a line of the axis limit along each axis."""
import numpy as np
from scipy import ndimage

from tests.components_cases import TILE, noise, two_blobs

SHAPES = [(1, 1, 1), (5, 33, 65), (10, 66, 130), (1, 1, 1024), (1, 1024, 1), (1024, 1, 1)]
BOX_SHAPES = [(5, 33, 65), (10, 66, 130)]           # the extents at which the geometric cases have room
HOLE_MODES = [(6, False), (26, False), (4, True), (8, True)]          # (background connectivity, per_slice)
HOLE_DEFECTS = ("face_left_out", "z_links_per_slice", "conn26_for_6", "hole_lt", "overwrite_other")
SMALL_DEFECTS = ("conn26_for_6", "small_le", "overwrite_other")


# ------------------------------------------------------------------------------------------------------- the restatement
def _label(mask, connectivity, per_slice):
    """int64 labels 1..n of a boolean volume (0 elsewhere) and n; per_slice: every z slice labelled on its own in 2D"""
    if not per_slice:
        lab, n = ndimage.label(mask, structure=ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3))
        return lab.astype(np.int64), n
    structure = ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2)
    lab, n = np.zeros(mask.shape, np.int64), 0
    for z in range(mask.shape[0]):
        part, k = ndimage.label(mask[z], structure=structure)
        lab[z] = np.where(part > 0, part + n, 0)
        n += k
    return lab, n


def _border(shape, per_slice, defect=None):
    b = np.zeros(shape, bool)
    if not per_slice:
        b[0] = b[-1] = True
    b[:, 0] = b[:, -1] = True
    b[:, :, 0] = True
    if defect != "face_left_out":
        b[:, :, -1] = True
    return b


def ref_fill_holes(vol, cls=1, connectivity=6, per_slice=False, max_hole=None, defect=None):
    """(uint8 result, int64 statistics row {n_complement_components, n_holes, voxels_filled, largest_hole}).  defect: one of
    HOLE_DEFECTS, a deliberately wrong variant for tests/test_host_postprocess.py (None: the definition)."""
    vol = np.asarray(vol)
    comp = vol != cls
    if defect == "conn26_for_6" and connectivity in (6, 4):
        connectivity = 26 if connectivity == 6 else 8
    if defect == "z_links_per_slice" and per_slice:
        lab, n = _label(comp, 6 if connectivity == 4 else 26, False)
    else:
        lab, n = _label(comp, connectivity, per_slice)
    sizes = np.bincount(lab.ravel(), minlength=n + 1)
    hole = np.ones(n + 1, bool)
    hole[0] = False
    hole[np.unique(lab[_border(vol.shape, per_slice, defect) & comp])] = False
    if max_hole is not None:
        hole &= (sizes < max_hole) if defect == "hole_lt" else (sizes <= max_hole)
    inside = hole[lab]
    fill = inside & ((vol == 0) if defect != "overwrite_other" else comp)
    out = vol.astype(np.uint8)
    out[fill] = cls
    return out, np.array([n, hole.sum(), fill.sum(), sizes[hole].max() if hole.any() else 0], np.int64)


def ref_remove_small(vol, cls=1, connectivity=6, min_voxels=1, defect=None):
    """(uint8 result, int64 statistics row {n_components, n_removed, voxels_removed, largest_removed})"""
    vol = np.asarray(vol)
    lab, n = _label(vol == cls, 26 if defect == "conn26_for_6" else connectivity, False)
    sizes = np.bincount(lab.ravel(), minlength=n + 1)
    small = (sizes <= min_voxels) if defect == "small_le" else (sizes < min_voxels)
    small[0] = False
    out = vol.astype(np.uint8)
    out[small[lab]] = 0
    if defect == "overwrite_other":
        out[vol != cls] = 0
    return out, np.array([n, small.sum(), sizes[small].sum(), sizes[small].max() if small.any() else 0], np.int64)


def ref_counts(result, truth, cls=1):
    """int64 {|P and T|, |P|, |T|}"""
    p, t = np.asarray(result) == cls, np.asarray(truth) == cls
    return np.array([(p & t).sum(), p.sum(), t.sum()], np.int64)


# ------------------------------------------------------------------------------------------------------------- contents
def _set(v, zs, ys, xs, value):
    """v[zs, ys, xs] = value for inclusive index ranges (lo, hi); an empty or out-of-range box is skipped"""
    sl = []
    for (lo, hi), s in zip((zs, ys, xs), v.shape):
        lo, hi = max(lo, 0), min(hi, s - 1)
        if lo > hi:
            return
        sl.append(slice(lo, hi + 1))
    v[tuple(sl)] = value


def hollow_box(shape):
    """a box one voxel inside the volume with a cavity one voxel inside the box: one hole under every mode"""
    D, H, W = shape
    v = np.zeros(shape, np.uint8)
    _set(v, (1, D - 2), (1, H - 2), (1, W - 2), 1)
    _set(v, (2, D - 3), (2, H - 3), (2, W - 3), 0)
    return v


def cavity_size(shape):
    return max(0, shape[0] - 4) * max(0, shape[1] - 4) * max(0, shape[2] - 4)


def face_cavity(shape, face):
    """a full volume with a 2 x 2 x 2 cavity that touches face `face` (0..5: z low, z high, y low, y high, x low, x high) and so is
    no hole in 3D, and a single-voxel cavity well inside, which is one"""
    D, H, W = shape
    v = np.ones(shape, np.uint8)
    at = [(D // 2, D // 2 + 1), (H // 2, H // 2 + 1), (W // 2, W // 2 + 1)]
    axis, high = face // 2, face % 2
    at[axis] = (shape[axis] - 2, shape[axis] - 1) if high else (0, 1)
    _set(v, *at, 0)
    _set(v, (1, 1), (1, 1), (1, 1), 0)
    return v


def seam_cavity(shape, axis):
    """a full volume with a cavity over the last voxel of the first tile and the first of the second along `axis`, two voxels wide in
    the other axes: a hole where the volume goes on behind it (2 * tile + 2), open where that voxel is the volume's last (tile + 1)"""
    v = np.ones(shape, np.uint8)
    at = [(1, 2), (1, 2), (1, 2)]
    at[axis] = (TILE[axis] - 1, TILE[axis])
    _set(v, *at, 0)
    return v


def diagonal_chain(shape):
    """a full volume with single-voxel cavities on a diagonal from the corner voxel inward: (1,1,1) and (2,2,2) are 2 holes under
    connectivity 6 and none under 26, which links them to (0,0,0) on the border.  Where there is room a second chain of two crosses
    the corner where the first tiles of all three axes meet: 2 holes under 6, one of 2 voxels under 26."""
    v = np.ones(shape, np.uint8)
    for k in range(3):
        _set(v, (k, k), (k, k), (k, k), 0)
    if all(s > t + 1 for s, t in zip(shape, TILE)):
        for k in (-1, 0):
            v[TILE[0] + k, TILE[1] + k, TILE[2] + k] = 0
    return v


def z_channel(shape):
    """a full volume with a channel of 2 x 2 voxels through every slice, away from the in-plane edges: open at both ends in 3D (no
    hole), closed in every plane (one hole per slice in per-slice mode)"""
    D, H, W = shape
    v = np.ones(shape, np.uint8)
    _set(v, (0, D - 1), (H // 2, H // 2 + 1), (W // 2, W // 2 + 1), 0)
    return v


def shell_in_cavity(shape):
    """a hollow box whose cavity holds a smaller hollow box: two nested holes where the extent allows it"""
    D, H, W = shape
    v = hollow_box(shape)
    _set(v, (3, D - 4), (5, H - 6), (5, W - 6), 1)
    _set(v, (4, D - 5), (8, H - 9), (8, W - 9), 0)
    if D < 9:                                     # too thin to nest in z: a ring in the middle slice closes the inner hole
        _set(v, (D // 2, D // 2), (5, H - 6), (5, W - 6), 1)
        _set(v, (D // 2, D // 2), (8, H - 9), (8, W - 9), 0)
    return v


def other_class_in_hole(shape):
    """a full volume with a cavity that holds voxels of class 2 (they pass through, the zeros around them are filled) and a single
    voxel of class 2 elsewhere: a hole with nothing to fill"""
    v = np.ones(shape, np.uint8)
    _set(v, (2, 2), (4, 8), (4, 12), 0)
    _set(v, (2, 2), (5, 6), (5, 8), 2)
    _set(v, (1, 1), (1, 1), (1, 1), 2)
    return v


def hole_contents(shape):
    """(name, uint8 volume) of every content of the hole table at one extent"""
    out = [("empty", np.zeros(shape, np.uint8)), ("full", np.ones(shape, np.uint8)), ("noise 0.31", noise(shape, 0.31)),
           ("noise 0.69", noise(shape, 0.69))]
    if shape in BOX_SHAPES:
        out += [("hollow box", hollow_box(shape))] + [(f"face {f}", face_cavity(shape, f)) for f in range(6)]
        out += [(f"seam {a}", seam_cavity(shape, a)) for a in range(3)]
        out += [("diagonal chain", diagonal_chain(shape)), ("z channel", z_channel(shape)), ("shell in cavity", shell_in_cavity(shape)),
                ("other class in hole", other_class_in_hole(shape))]
    return out


def three_blobs(shape):
    """boxes of 8, 12 and 12 voxels (a tie) and a single voxel, apart from each other, and a box of class 2"""
    v = np.zeros(shape, np.uint8)
    _set(v, (0, 1), (0, 1), (0, 1), 1)
    _set(v, (0, 1), (4, 5), (4, 6), 1)
    _set(v, (3, 4), (20, 21), (40, 42), 1)
    _set(v, (2, 2), (30, 30), (60, 60), 1)
    _set(v, (0, 1), (10, 12), (10, 12), 2)
    return v


def small_contents(shape):
    """(name, uint8 volume) of every content of the size-filter table at one extent"""
    out = [("empty", np.zeros(shape, np.uint8)), ("full", np.ones(shape, np.uint8)), ("noise 0.31", noise(shape, 0.31)),
           ("noise 0.69", noise(shape, 0.69))]
    if shape in BOX_SHAPES:
        out += [("three blobs", three_blobs(shape)), ("equal blobs", two_blobs(shape)), ("later blob larger", two_blobs(shape, later_larger=True))]
    return out


def bounds_around(sizes, most=3):
    """one below, at and one above the smallest, the largest and up to `most` sizes in all (of components or of holes), without
    values below 1: the thresholds at which a `<` / `<=` mistake shows"""
    sizes = sorted(set(int(s) for s in sizes))
    picked = sizes[:most - 1] + sizes[-1:] if len(sizes) > most else sizes
    return sorted({b for s in picked for b in (s - 1, s, s + 1) if b >= 1}) or [1]


def component_sizes(vol, cls=1, connectivity=6):
    lab, n = _label(np.asarray(vol) == cls, connectivity, False)
    return np.bincount(lab.ravel(), minlength=n + 1)[1:]


def hole_sizes(vol, cls=1, connectivity=6, per_slice=False):
    """sizes of the complement components that do not reach the border"""
    vol = np.asarray(vol)
    lab, n = _label(vol != cls, connectivity, per_slice)
    inner = np.setdiff1d(np.arange(1, n + 1), lab[_border(vol.shape, per_slice) & (vol != cls)])
    return np.bincount(lab.ravel(), minlength=n + 1)[inner]
