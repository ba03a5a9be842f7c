"""Helpers of tests/test_gpu_augment.py that need no GPU: test slices, the fp64 recomputation of sampling coordinates
(the rounding bands a nearest-neighbour comparison has to exclude) and the host calibrations of its tolerances."""
import random

import numpy as np
import torch

from rpnet_amd.utils import volume_reader as VR

BAND = 1e-3          # half-width, in pixels, of the excluded band around a rounding boundary


def seed_all(s):
    random.seed(s), np.random.seed(s), torch.manual_seed(s)


def rng_state():
    n = np.random.get_state()
    return random.getstate(), (n[1].tobytes(), n[2], n[3], n[4]), torch.get_rng_state().numpy().tobytes()


def make_slice(seed, H, W):
    """a CT-like slice in [-1,1] with an exact -1 border (the HU pad) and a blob label"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    body = ((yy - H / 2) / (0.42 * H)) ** 2 + ((xx - W / 2) / (0.40 * W)) ** 2 < 1
    img = np.where(body, -0.5 + 0.3 * rs.rand(H, W), -1.0).astype(np.float32)
    cy, cx = H * rs.uniform(0.35, 0.65), W * rs.uniform(0.35, 0.65)
    lab = (((yy - cy) / (0.2 * H)) ** 2 + ((xx - cx) / (0.17 * W)) ** 2 < 1).astype(np.float32)
    img[lab > 0] += 0.4
    return img, lab


def affine_source(m, H, W):
    """fp64 source pixel coordinates (iy, ix) of random_affine's sampling for the fp32-rounded map m (what grid_sample
    un-normalises to: s + n/2 - 1/2)"""
    m = np.asarray(m, dtype=np.float32).astype(np.float64)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    bx, by = xx - W * 0.5 + 0.5, yy - H * 0.5 + 0.5
    return m[3] * bx + m[4] * by + m[5] + (H * 0.5 - 0.5), m[0] * bx + m[1] * by + m[2] + (W * 0.5 - 0.5)


def near_half(c, band=BAND):
    """coordinate within `band` of a rounding boundary k + 1/2"""
    return np.abs(c - np.floor(c) - 0.5) < band


def gather(src, iy, ix, fill=0.0):
    """src[iy, ix] for integer arrays, `fill` outside"""
    H, W = src.shape
    ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
    out = np.full(iy.shape, fill, dtype=src.dtype)
    out[ok] = src[iy[ok], ix[ok]]
    return out


def candidates(src, cy, cx, fill=0.0, band=BAND):
    """the values a nearest-neighbour sample at (cy, cx) may take: on an axis whose coordinate sits within `band` of a
    rounding boundary either of the two neighbouring pixels, on the other axis the rounded one only"""
    def axis(c):
        f, r = np.floor(c).astype(np.int64), np.rint(c).astype(np.int64)
        near = near_half(c, band)
        return np.where(near, f, r), np.where(near, f + 1, r)
    return [gather(src, iy, ix, fill) for iy in axis(cy) for ix in axis(cx)]


def make_slice_rng(seed, H, W):
    """an unstructured slice in [-1,1] with an exact -1 top band, and a random label"""
    rs = np.random.RandomState(seed)
    img = rs.rand(1, 1, H, W).astype(np.float32) * 2 - 1
    img[0, 0, : H // 5] = -1.0                               # exact zeros of the [0,1] image, as the HU pad gives
    lab = (rs.rand(1, H, W) > 0.6).astype(np.float32)
    return torch.from_numpy(img), torch.from_numpy(lab)


def intensity_formula(img, gamma, dtype):
    """the value map of gamma_transform (gamma not None) followed by random_transform's [0,1] round trip, in `dtype`"""
    x = img.astype(dtype)
    if gamma is not None:
        x = VR.gamma_apply(x, dtype(gamma))
    return ((x + 1) / 2) * 2 - 1


def elastic_coords(Minv, noise, alpha, sigma, H, W):
    from scipy.ndimage import gaussian_filter
    dx, dy = gaussian_filter(noise[0], sigma) * alpha, gaussian_filter(noise[1], sigma) * alpha
    xx, yy = np.meshgrid(np.arange(W), np.arange(H))
    src_x = Minv[0, 0] * xx + Minv[0, 1] * yy + Minv[0, 2]
    src_y = Minv[1, 0] * xx + Minv[1, 1] * yy + Minv[1, 2]
    return src_y, src_x, yy + dy, xx + dx


def elastic_image_fp32_coords(image, Minv, noise, alpha=1000, sigma=30, padding_value=-1.0):
    """elastic_apply's image path with its sampling coordinates rounded to fp32 (the tolerance calibration)"""
    from scipy.ndimage import map_coordinates
    D, H, W = image.shape
    sy, sx, wy, wx = [c.astype(np.float32) for c in elastic_coords(Minv, noise, alpha, sigma, H, W)]
    out = np.zeros_like(image)
    for z in range(D):
        aff = map_coordinates(image[z], (sy, sx), order=1, mode="constant", cval=padding_value)
        out[z] = map_coordinates(aff, (wy.reshape(-1, 1), wx.reshape(-1, 1)), order=1, mode="constant", cval=padding_value).reshape(H, W)
    return out


def elastic_mask_band(Minv, noise, alpha, sigma, H, W, band=BAND):
    """pixels whose mask value may legitimately differ: stage 2 reads within `band` of a rounding boundary or of the edge
    of the plane, or reads a stage-1 pixel that does"""
    sy, sx, wy, wx = elastic_coords(Minv, noise, alpha, sigma, H, W)
    b1 = near_half(sy, band) | near_half(sx, band)
    edge = (np.abs(wy) < band) | (np.abs(wy - (H - 1)) < band) | (np.abs(wx) < band) | (np.abs(wx - (W - 1)) < band)
    b2 = near_half(wy, band) | near_half(wx, band) | edge
    return b2 | gather(b1, np.floor(wy + 0.5).astype(np.int64), np.floor(wx + 0.5).astype(np.int64), False)


def host_query_slice(raw, mask, elastic, gamma, m, fp32_coords=False):
    """the host reader's path of one query slice [H,W] with given draws: elastic_apply (elastic = (Minv, noise) or None)
    -> gamma_apply (gamma or None) -> transform_apply(m).  fp32_coords: the elastic image through
    elastic_image_fp32_coords instead (the calibration of the composed path's image tolerance)."""
    img, msk = raw[None, None], mask[None, None]
    if elastic is not None:
        e_img, msk = VR.elastic_apply(img, msk, elastic[0], elastic[1])
        img = elastic_image_fp32_coords(raw[None], elastic[0], elastic[1])[None] if fp32_coords else e_img
    q = img[0]
    if gamma is not None:
        q = VR.gamma_apply(q, gamma)
    qi, ql = VR.transform_apply(torch.from_numpy(np.ascontiguousarray(q))[None], torch.from_numpy(np.ascontiguousarray(msk[0])), m)
    return qi[0, 0].numpy(), ql[0].numpy()


def composed_band(m, elastic, H, W, band=BAND):
    """pixels of an augmented query slice whose label may legitimately differ: the affine sampling's own rounding band, or
    a source pixel (the rounded one) that lies in the elastic transform's mask band"""
    cy, cx = affine_source(m, H, W)
    out = near_half(cy, band) | near_half(cx, band)
    if elastic is not None:
        eb = elastic_mask_band(elastic[0], elastic[1], 1000, 30, H, W, band)
        out = out | gather(eb, np.rint(cy).astype(np.int64), np.rint(cx).astype(np.int64), False)
    return out
