"""Train-time augmentation of episode slices on the device (csrc/augment.hip): what the train-mode reader
(rpnet_amd/utils/volume_reader.py) does per slice on the host — gamma_transform, random_transform,
random_label_transform, elastic_transform_all — as a fixed number of launches per item.

The random draws are separated from their application.  `draw_*` consume the `random` / `numpy.random` / `torch`
generators in exactly the order and number the host functions do (the reader convention), so a
seeded run here and a seeded run of the host reader pick the same parameters; the host functions themselves call these
draws.  The application (`augment_slices`, `label_transform`, `elastic_slices`) takes device tensors and has no CPU
fallback.
"""
import ctypes as C
import functools
import math

import numpy as np
import torch

from . import hip
from .hip import call, ptr

N_PARAMS = 8      # per slice: the 2x3 inverse map (row major), gamma, gamma flag


# ------------------------------------------------------------------------------------------------------------- draws
def _uniform(lo, hi):
    return float(torch.empty(1).uniform_(float(lo), float(hi)).item())


def draw_random_affine(H, W, degrees, translate=None, scale=None, shear=None):
    """The six numbers torchvision's RandomAffine puts into `theta` (the inverse map about the image centre, in
    pixels), as python floats.  Draw order: angle, tx, ty, scale, shear (torch generator); an argument that is None
    draws nothing."""
    deg = (-degrees, degrees) if np.isscalar(degrees) else degrees
    angle = _uniform(*deg)
    tx = ty = 0
    if translate is not None:
        tx = int(round(_uniform(-translate[0] * W, translate[0] * W)))
        ty = int(round(_uniform(-translate[1] * H, translate[1] * H)))
    s = _uniform(*scale) if scale is not None else 1.0
    shx = 0.0
    if shear is not None:
        sh = (-shear, shear) if np.isscalar(shear) else shear
        shx = _uniform(sh[0], sh[1])
    rot, sx = math.radians(angle), math.radians(shx)
    # forward map = T(translate) R(rot) Shear(sx) S(s) about the centre; rows of its inverse:
    a, b = math.cos(rot), -math.cos(rot) * math.tan(sx) - math.sin(rot)
    c, d = math.sin(rot), -math.sin(rot) * math.tan(sx) + math.cos(rot)
    m = [d / s, -b / s, 0.0, -c / s, a / s, 0.0]
    m[2] = m[0] * -tx + m[1] * -ty
    m[5] = m[3] * -tx + m[4] * -ty
    return m


TRANSFORM_ARGS = dict(degrees=5, translate=(0.2, 0.2), scale=(0.7, 1.5), shear=0)              # random_transform
LABEL_TRANSFORM_ARGS = dict(degrees=5, translate=(0.02, 0.02), scale=(0.5, 1.5), shear=5)       # random_label_transform


def draw_gamma(gamma_range):
    """gamma_transform's exponent: one np.random.rand() draw"""
    return np.random.rand() * (gamma_range[1] - gamma_range[0]) + gamma_range[0]


def three_point_affine(src, dst):
    """the 2x3 M with M [x, y, 1]^T = dst for three point pairs (cv2.getAffineTransform)"""
    A = np.concatenate([src, np.ones((3, 1))], axis=1).astype(np.float64)
    return np.linalg.solve(A, dst.astype(np.float64)).T


def draw_elastic(plane, alpha_affine=0.04, random_state=None):
    """elastic_transform_all's draws for a plane (H, W): the 2x3 fp64 inverse affine `Minv` (three corner points
    jittered by +-alpha_affine) and the two uniform noise planes [2,H,W] fp64 in [-1,1) (x displacement first), from
    `random_state` (None: an unseeded RandomState, as the reference)."""
    rs = random_state if random_state is not None else np.random.RandomState(None)
    centre, half = np.float32(plane) // 2, min(plane) // 3
    pts1 = np.float32([centre + half, [centre[0] + half, centre[1] - half], centre - half])
    pts2 = pts1 + rs.uniform(-alpha_affine, alpha_affine, size=pts1.shape).astype(np.float32)
    M = three_point_affine(pts1, pts2)
    Minv = np.linalg.inv(np.vstack([M, [0, 0, 1]]))[:2]
    noise_x = rs.rand(*plane) * 2 - 1
    noise_y = rs.rand(*plane) * 2 - 1
    return Minv, np.stack([noise_x, noise_y])


def gaussian_weights(sigma, truncate=4.0):
    """the 1-D kernel of scipy.ndimage.gaussian_filter(sigma): radius int(truncate * sigma + 0.5), normalised, fp64"""
    radius = int(truncate * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    return phi / phi.sum(), radius


@functools.lru_cache(maxsize=16)
def device_weights(sigma, device):
    w, radius = gaussian_weights(sigma)
    return torch.from_numpy(w).to(device), radius


def pack_params(affines, gammas=None):
    """[S,8] fp32 table of rpnet_augment_affine from S lists of six numbers and S gammas (None: the slice's power law
    is off) — a host tensor; one copy takes it to the device"""
    S = len(affines)
    t = torch.zeros((S, N_PARAMS), dtype=torch.float32)
    for i, m in enumerate(affines):
        t[i, :6] = torch.tensor(m, dtype=torch.float32)
        if gammas is not None and gammas[i] is not None:
            t[i, 6], t[i, 7] = float(gammas[i]), 1.0
    return t


def upload(t, device):
    """host tensor -> device through pinned memory, without a host synchronisation"""
    return t.pin_memory().to(device, non_blocking=True)


# ------------------------------------------------------------------------------------------------------- application
def _planes(x, what):
    if x.dim() != 3 or x.dtype != torch.float32:
        raise ValueError(f"{what}: expected a float32 [S,H,W] tensor, got {x.dtype} {tuple(x.shape)}")
    return x.contiguous()


def _table(params, S, device):
    if params.dtype != torch.float32 or tuple(params.shape) != (S, N_PARAMS):
        raise ValueError(f"params: expected float32 [{S},{N_PARAMS}] (pack_params), got {params.dtype} {tuple(params.shape)}")
    return params.contiguous() if params.is_cuda else upload(params, device)


def augment_slices(images, labels, params):
    """gamma_transform (where params[:, 7] is set) followed by random_transform, for S slices at once.  images [S,H,W]
    in [-1,1], labels [S,H,W], both float32 on the GPU; params [S,8] (pack_params; host or device).  Returns
    (images, labels) [S,H,W].  Two launches."""
    hip.require_gpu(images, labels)
    images, labels = _planes(images, "images"), _planes(labels, "labels")
    if images.shape != labels.shape:
        raise ValueError(f"images {tuple(images.shape)} and labels {tuple(labels.shape)} differ")
    S, H, W = images.shape
    params = _table(params, S, images.device)
    mm = torch.empty((S, 2), device=images.device, dtype=torch.float32)
    out_i, out_l = torch.empty_like(images), torch.empty_like(labels)
    call("rpnet_slice_minmax", ptr(images), ptr(mm), S, H, W)
    call("rpnet_augment_affine", ptr(images), ptr(labels), ptr(params), ptr(mm), ptr(out_i), ptr(out_l), S, H, W)
    return out_i, out_l


def label_transform(labels, params):
    """random_label_transform for S label slices [S,H,W] (float32, GPU): the sampling of augment_slices alone"""
    hip.require_gpu(labels)
    labels = _planes(labels, "labels")
    S, H, W = labels.shape
    params = _table(params, S, labels.device)
    out = torch.empty_like(labels)
    call("rpnet_augment_affine", None, ptr(labels), ptr(params), None, None, ptr(out), S, H, W)
    return out


def elastic_field(noise, alpha=1000, sigma=30):
    """[2,H,W] fp32 (dx, dy) = alpha * gaussian_filter(noise [2,H,W] fp64, sigma), on the device.  Two launches."""
    hip.require_gpu(noise)
    if noise.dim() != 3 or noise.shape[0] != 2 or noise.dtype != torch.float64:
        raise ValueError(f"noise: expected float64 [2,H,W], got {noise.dtype} {tuple(noise.shape)}")
    noise = noise.contiguous()
    _, H, W = noise.shape
    w, radius = device_weights(float(sigma), noise.device)       # uploaded once per (sigma, device)
    tmp = torch.empty_like(noise)
    field = torch.empty((2, H, W), device=noise.device, dtype=torch.float32)
    call("rpnet_elastic_field", ptr(noise), ptr(w), radius, float(alpha), ptr(tmp), ptr(field), H, W)
    return field


def elastic_slices(images, masks, Minv, noise, alpha=1000, sigma=30, padding_value=-1.0):
    """elastic_transform_all for the S slices it is given: images [S,H,W] (bilinear, `padding_value` outside) and masks
    [S,H,W] (nearest, 0 outside), float32 on the GPU, either may be None; Minv the 2x3 fp64 inverse affine (host: numpy
    or nested lists), noise [2,H,W] fp64 (host numpy or a device tensor; a device [2,H,W] float32 tensor is taken as the
    finished field of elastic_field).  All slices share the map and the field.  Four launches."""
    hip.require_gpu(images, masks)
    ref = images if images is not None else masks
    if ref is None:
        raise ValueError("elastic_slices: neither images nor masks")
    images = None if images is None else _planes(images, "images")
    masks = None if masks is None else _planes(masks, "masks")
    if images is not None and masks is not None and images.shape != masks.shape:
        raise ValueError(f"images {tuple(images.shape)} and masks {tuple(masks.shape)} differ")
    S, H, W = ref.shape
    if isinstance(noise, np.ndarray):
        noise = upload(torch.from_numpy(np.ascontiguousarray(noise, dtype=np.float64)), ref.device)
    field = noise if noise.dtype == torch.float32 else elastic_field(noise, alpha, sigma)
    hip.require_gpu(field)
    if tuple(field.shape) != (2, H, W):
        raise ValueError(f"field {tuple(field.shape)} does not match the slices [{S},{H},{W}]")
    m = (C.c_double * 6)(*np.asarray(Minv, dtype=np.float64).reshape(6).tolist())
    tmp_i = out_i = tmp_m = out_m = None
    if images is not None:
        tmp_i, out_i = torch.empty_like(images), torch.empty_like(images)
    if masks is not None:
        tmp_m, out_m = torch.empty_like(masks), torch.empty_like(masks)
    call("rpnet_elastic_apply", ptr(images), ptr(masks), m, ptr(field.contiguous()), ptr(tmp_i), ptr(tmp_m), ptr(out_i), ptr(out_m),
         S, H, W, float(padding_value))
    return out_i, out_m
