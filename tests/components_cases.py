"""Case tables of the connected-component tests and the numpy restatement of the contract of include/rpnet_cc_abi.h that the GPU tests
compare with (tests/test_host_components.py pins it to scipy.ndimage.label and shows that seeded defects fail the same comparison).

The tile of csrc/components.hip is 4 x 32 x 64 voxels (z, y, x): the extents are one voxel, D == 1, one past a tile in every axis
(tile + 1), 2 * tile + 2, a few whole tiles, and a line of the axis limit along x and along z."""
import numpy as np
from scipy import ndimage

TILE = (4, 32, 64)
SHAPES = [(1, 1, 1), (1, 7, 9), (5, 33, 65), (10, 66, 130), (17, 64, 64), (1, 1, 1024), (1024, 1, 1)]
DENSITIES = (0.2, 0.31, 0.6)
DEFECTS = ("no_z_seam", "no_diagonal_26", "tie_last", "off_by_one", "zero_other_classes")


# ------------------------------------------------------------------------------------------------------- the restatement
def ref_label(vol, cls=1, connectivity=6, defect=None):
    """int32 labels of `vol == cls`: background 0, a foreground voxel 1 + the smallest linear index of its component.  defect: one of
    DEFECTS, a deliberately wrong variant for tests/test_host_components.py (None: the contract)."""
    fg = np.asarray(vol) == cls
    rank = 1 if connectivity == 6 or defect == "no_diagonal_26" else 3
    structure = ndimage.generate_binary_structure(3, rank)
    if defect == "no_z_seam":                               # every slab of TILE[0] slices on its own
        out = np.zeros(fg.shape, np.int32)
        plane = fg.shape[1] * fg.shape[2]
        for z0 in range(0, fg.shape[0], TILE[0]):
            part = ref_label(fg[z0:z0 + TILE[0]], True, connectivity)
            out[z0:z0 + TILE[0]] = np.where(part > 0, part + z0 * plane, 0)
        return out
    lab, n = ndimage.label(fg, structure=structure)
    flat = lab.ravel()
    values, first = np.unique(flat, return_index=True)      # first[k]: the smallest linear index that holds values[k]
    table = np.zeros(n + 1, np.int64)
    table[values] = first + (0 if defect == "off_by_one" else 1)
    table[0] = 0
    return table[flat].reshape(fg.shape).astype(np.int32)


def ref_stats(vol, cls=1, connectivity=6, defect=None):
    """the statistics row: int64 {n_foreground, n_components, size_largest, first_index_largest}; (0, 0, 0, -1) for an empty class.
    The largest size wins, among equals the component whose first voxel comes first."""
    lab = ref_label(vol, cls, connectivity, defect if defect != "off_by_one" else None)
    values, sizes = np.unique(lab[lab > 0], return_counts=True)
    if values.size == 0:
        return np.array([0, 0, 0, -1], np.int64)
    best = sizes.max()
    ties = values[sizes == best]
    chosen = ties.max() if defect == "tie_last" else ties.min()
    return np.array([sizes.sum(), values.size, best, chosen - 1], np.int64)


def ref_keep_largest(vol, cls=1, connectivity=6, defect=None):
    """uint8: `vol` with the voxels of class `cls` outside its largest component set to 0; every other value passes through"""
    vol = np.asarray(vol)
    lab = ref_label(vol, cls, connectivity, defect if defect != "off_by_one" else None)
    chosen = ref_stats(vol, cls, connectivity, defect)[3] + 1
    out = vol.astype(np.uint8)
    out[(vol == cls) & (lab != chosen)] = 0
    if defect == "zero_other_classes":
        out[vol != cls] = 0
    return out


def ref_counts(filtered, truth, cls=1):
    """int64 {|P and T|, |P|, |T|}"""
    p, t = np.asarray(filtered) == cls, np.asarray(truth) == cls
    return np.array([(p & t).sum(), p.sum(), t.sum()], np.int64)


# ------------------------------------------------------------------------------------------------------------- contents
def _grid(shape):
    return np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")


def empty(shape):
    return np.zeros(shape, np.uint8)


def full(shape):
    return np.ones(shape, np.uint8)


def checkerboard(shape):
    """under 6 every voxel is its own component, under 26 there is one"""
    z, y, x = _grid(shape)
    return ((z + y + x) % 2 == 0).astype(np.uint8)


def serpentine(shape):
    """one path, one voxel wide: full x lines on the even rows of the even slices, joined at alternating ends; the slices joined
    through the odd slices at alternating ends of the path.  It crosses every seam many times."""
    D, H, W = shape
    plane = np.zeros((H, W), np.uint8)
    plane[0::2] = 1
    for y in range(1, H, 2):
        if y + 1 < H:
            plane[y, W - 1 if (y // 2) % 2 == 0 else 0] = 1
    last = H - 1 if (H - 1) % 2 == 0 else H - 2
    end = (last, W - 1 if (last // 2) % 2 == 0 else 0)
    v = np.zeros(shape, np.uint8)
    v[0::2] = plane
    for z in range(1, D, 2):
        if z + 1 < D:
            at = end if (z // 2) % 2 == 0 else (0, 0)
            v[z, at[0], at[1]] = 1
    return v


def u_shape(shape):
    """two arms along x, in opposite corners of the (z, y) plane, that join only at x = W - 1"""
    D, H, W = shape
    v = np.zeros(shape, np.uint8)
    v[0, 0, :] = 1
    v[D - 1, H - 1, :] = 1
    v[0, :, W - 1] = 1
    v[:, H - 1, W - 1] = 1
    return v


def _box(v, at, size, value=1):
    v[tuple(slice(a, a + s) for a, s in zip(at, size))] = value


def two_blobs(shape, later_larger=False, flip=False):
    """two boxes of one size in opposite corners (the tie: the first one wins); later_larger: the second one voxel-layer larger"""
    size = [max(1, min(3, s // 3)) for s in shape]
    v = np.zeros(shape, np.uint8)
    _box(v, (0, 0, 0), size)
    big = [s + 1 if later_larger and shape[k] >= 3 * s + 1 else s for k, s in enumerate(size)]
    _box(v, [s - b for s, b in zip(shape, big)], big)
    return v[::-1, ::-1, ::-1].copy() if flip else v


def touching(shape, corner=False):
    """two boxes that share only an edge (corner=False) or only a corner: separate under 6, joined under 26"""
    size = [max(1, min(2, s // 2)) for s in shape]
    v = np.zeros(shape, np.uint8)
    _box(v, (0, 0, 0), size)
    at = [size[0] if corner and shape[0] > size[0] else 0, size[1] if shape[1] > size[1] else 0, size[2] if shape[2] > size[2] else 0]
    _box(v, at, size)
    return v


def noise(shape, density, seed=0):
    return (np.random.RandomState(1000 + seed + int(density * 100)).rand(*shape) < density).astype(np.uint8)


def three_classes(shape, seed=3):
    return np.random.RandomState(seed).choice(4, size=shape, p=[0.4, 0.25, 0.2, 0.15]).astype(np.uint8)


def contents(shape):
    """(name, uint8 volume) of every content of the table at one extent"""
    out = [("empty", empty(shape)), ("full", full(shape)), ("checkerboard", checkerboard(shape)), ("serpentine", serpentine(shape)),
           ("u", u_shape(shape)), ("equal blobs", two_blobs(shape)), ("equal blobs, flipped", two_blobs(shape, flip=True)),
           ("later blob larger", two_blobs(shape, later_larger=True)), ("edge", touching(shape)), ("corner", touching(shape, corner=True))]
    out += [(f"noise {d}", noise(shape, d)) for d in DENSITIES]
    return out
