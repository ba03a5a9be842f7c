"""Masks shared by tests/test_host_surface.py and tests/test_gpu_surface.py (numpy only)."""
import numpy as np

# the smallest shapes at which each kernel path of csrc/surface.hip can go wrong: no z neighbours; odd and below every tile; lines that
# straddle tile and wave boundaries; a long line on each axis; the axis limit on each axis
SMALL = [(1, 16, 16), (5, 7, 9), (9, 33, 20), (17, 40, 36)]
LONG = [(2, 3, 300), (2, 300, 3), (300, 3, 2)]
LIMIT = [(1024, 2, 1), (1, 1024, 2), (2, 1, 1024)]


def dilate(m, times=1):
    """6-neighbourhood dilation by shifted arrays, outside = background"""
    m = np.asarray(m, dtype=bool)
    for _ in range(times):
        p = np.pad(m, 1, constant_values=False)
        out = m.copy()
        for axis in range(3):
            for shift in (-1, 1):
                out |= np.roll(p, shift, axis=axis)[1:-1, 1:-1, 1:-1]
        m = out
    return m


def dilated_random(shape, seed, p=0.02, times=2):
    """a few random seeds grown into blobs (at least one voxel is set)"""
    rs = np.random.RandomState(seed)
    m = rs.rand(*shape) < p
    m.flat[rs.randint(m.size)] = True
    return dilate(m, times)


def random_pair(shape, seed=0):
    """(prediction, truth) uint8: two different dilated random masks"""
    a, b = dilated_random(shape, 1000 + seed + sum(shape)), dilated_random(shape, 2000 + seed + sum(shape), times=1)
    assert (a != b).any()
    return a.astype(np.uint8), b.astype(np.uint8)


def single_voxels(shape):
    """one voxel each, in opposite corners"""
    a, b = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    a[0, 0, 0] = 1
    b[-1, -1, -1] = 1
    return a, b


def two_blobs(shape):
    """the truth: a box in the low corner; the prediction: the same box and a single stray voxel in the far corner (HD95 < HD)"""
    D, H, W = shape
    b = np.zeros(shape, np.uint8)
    b[:max(1, D // 2), :max(1, H // 2), :max(1, W // 2)] = 1
    a = b.copy()
    a[-1, -1, -1] = 1
    return a, b


def three_valued(shape, seed=0):
    """masks of the values 0, 1, 2: class 2 differs between prediction and truth"""
    a1, b1 = random_pair(shape, seed)
    a2, b2 = random_pair(shape, seed + 7)
    a, b = a1.copy(), b1.copy()
    a[(a2 == 1) & (a1 == 0)] = 2
    b[(b2 == 1) & (b1 == 0)] = 2
    if not (a == 2).any():
        a.flat[0] = 2
    if not (b == 2).any():
        b.flat[-1] = 2
    return a, b
