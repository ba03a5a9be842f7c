"""The deterministic preprocessing of FewshotVolumeReader.load_image_and_mask (rpnet_amd/utils/volume_reader.py) on the device
(csrc/volload.hip, include/rpnet_volload_abi.h): the payloads of the two NRRD files go up in their file dtype and order, and the annotated
z range, truncate, pad to 16, centre crop, symmetric pad, the 99.5th-percentile clip, the HU clip and the map to [-1, 1] run there.
tests/volload_cases.py restates every definition in numpy, and tests/test_host_volload.py pins that restatement to the host reader and to
numpy.percentile bit for bit.

Definitions (word for word those of include/rpnet_volload_abi.h).
Window: nz = min(D, num_slice); y1 = max(0, H // 2 - num_y // 2), y2 = min(H, H // 2 + num_y // 2), x likewise; padded extents: the
window's rounded up to a multiple of 16, padding at the far end.  Crop: rh = min(crop_h, pH) rows from pH // 2 - rh // 2, padded with
(crop_h - rh) // 2 rows before and the rest behind.  The image takes pad_value in every pad, the mask 0.
Percentile: numpy's method 'linear' as numpy >= 2 computes it for a float32 array, the virtual index in float32 (percentile_rank), the
two order statistics exact, the interpolation numpy's _lerp in float32; a NaN anywhere makes the percentile a NaN, which clips nothing.
Normalize: v > top -> top; v > maximum -> maximum; v < minimum -> minimum; ((v - minimum) / max(1, maximum - minimum)) * 2 - 1, every
operation one float32 rounding, minimum, maximum and the denominator rounded to float32 as numpy rounds a Python number beside a float32
array.
"""
import os

import numpy as np
import torch

from . import hip
from ._volume_checks import WorkspaceCache, one_device
from .utils import nrrd

SOURCE_KINDS = {torch.float32: 0, torch.int16: 1, torch.uint8: 2}       # RPNET_PREP_F32, RPNET_PREP_I16, RPNET_VOLLOAD_U8
IMAGE_KINDS = (torch.float32, torch.int16)
X_FASTEST, Z_FASTEST = 0, 1                         # RPNET_VOLLOAD_X_FASTEST, RPNET_VOLLOAD_Z_FASTEST
MAX_EXTENT = 1024                                   # RPNET_CC_MAX_DIM
MAX_VALUES = 1 << 30                                # RPNET_VOLLOAD_MAX_N
SELECT_BLOCKS = 1024                                # RPNET_VOLLOAD_SELECT_BLOCKS
SELECT_SWEEP = SELECT_BLOCKS * 256 * 4              # values one sweep of a counting pass covers
HOST_READER = "rpnet_amd.utils.volume_reader.FewshotVolumeReader.load_image_and_mask"
# one selection workspace per device (8256 bytes whatever n); a captured graph holds it by its address, and it is never regrown
_workspaces = WorkspaceCache(by_shape=False)


def load_geometry(cfg, file_shape):
    """the integers of the reader's truncate, pad to 16 and crop for a file of shape (D, H, W) under `cfg` (num_slice, num_y, num_x,
    crop_size): the window nz, y1, y2, x1, x2; the padded extents pD, pH, pW; the crop rh, rw (rows and columns kept), cy, cx (where they
    start in the padded volume), pt, pl (pad before them), ch, cw (the output's extents)"""
    D, H, W = (int(v) for v in file_shape)
    ns, ny, nx = int(cfg["num_slice"]), int(cfg["num_y"]), int(cfg["num_x"])
    ch, cw = (int(v) for v in cfg.get("crop_size", [256, 256]))
    if min(D, H, W) < 1 or max(D, H, W) > MAX_EXTENT or min(ch, cw) < 1 or max(ch, cw) > MAX_EXTENT:
        raise ValueError(f"load_geometry: file shape {(D, H, W)} and crop_size {(ch, cw)} must have every extent 1..{MAX_EXTENT} "
                         f"(the host reader is {HOST_READER})")
    if min(ns, ny, nx) < 1:
        raise ValueError(f"load_geometry: num_slice={ns} num_y={ny} num_x={nx} must each be at least 1 (the host reader is {HOST_READER})")
    g = {"D": D, "H": H, "W": W, "num_slice": ns, "num_y": ny, "num_x": nx, "ch": ch, "cw": cw}
    g["nz"] = min(D, ns)
    g["y1"], g["y2"] = max(0, H // 2 - ny // 2), min(H, H // 2 + ny // 2)
    g["x1"], g["x2"] = max(0, W // 2 - nx // 2), min(W, W // 2 + nx // 2)
    if g["y2"] <= g["y1"] or g["x2"] <= g["x1"]:
        raise ValueError(f"load_geometry: the window of num_y={ny} num_x={nx} in a {H} x {W} slice is empty (the host reader is {HOST_READER})")
    g["pD"], g["pH"], g["pW"] = (-(-n // 16) * 16 for n in (g["nz"], g["y2"] - g["y1"], g["x2"] - g["x1"]))
    g["rh"], g["rw"] = min(ch, g["pH"]), min(cw, g["pW"])
    g["cy"], g["cx"] = g["pH"] // 2 - g["rh"] // 2, g["pW"] // 2 - g["rw"] // 2
    g["pt"], g["pl"] = (ch - g["rh"]) // 2, (cw - g["rw"]) // 2
    return g


def _source(fn, vol, kinds, what):
    """(layout, (D, H, W)) of a source volume: a [D,H,W] tensor that is contiguous, or whose memory is the payload of a file with the
    sizes D H W (strides (1, D, D * H): `flat.view(W, H, D).permute(2, 1, 0)`)"""
    hip.require_gpu(vol)
    if not torch.is_tensor(vol) or vol.dtype not in kinds:
        names = ", ".join(str(k)[6:] for k in kinds)
        raise ValueError(f"{fn}: {what} is {getattr(vol, 'dtype', type(vol))}; {names} are accepted (the host reader is {HOST_READER})")
    if vol.dim() != 3 or not all(1 <= n <= MAX_EXTENT for n in vol.shape):
        raise ValueError(f"{fn}: {what} must be a [D,H,W] tensor with every axis 1..{MAX_EXTENT}, got {tuple(vol.shape)}")
    if vol.is_contiguous():
        return X_FASTEST, tuple(vol.shape)
    if vol.permute(2, 1, 0).is_contiguous():
        return Z_FASTEST, tuple(vol.shape)
    raise ValueError(f"{fn}: {what} must be contiguous, or the transposed view of a file's payload (strides (1, D, D * H))")


def _window_args(geom):
    return geom["D"], geom["H"], geom["W"], geom["num_slice"], geom["num_y"], geom["num_x"]


def annotated_range(mask, geom, out=None):
    """the annotated z range of `mask` (uint8, int16 or float32 [D,H,W], contiguous or in file order) inside the window of `geom`
    (load_geometry) -> int32 [4] on the device: first and last z with a non-zero voxel (a NaN counts), the number of non-zero voxels, 0;
    first = last = -1 where there is none.  Three launches, nothing read back."""
    fn = "annotated_range"
    layout, shape = _source(fn, mask, tuple(SOURCE_KINDS), "mask")
    if shape != (geom["D"], geom["H"], geom["W"]):
        raise ValueError(f"{fn}: mask {shape} is not the file shape {(geom['D'], geom['H'], geom['W'])} of the geometry")
    if out is None:
        out = torch.empty(4, device=mask.device, dtype=torch.int32)
    elif not torch.is_tensor(out) or out.dtype != torch.int32 or out.shape != (4,) or not out.is_contiguous():
        raise ValueError(f"{fn}: out must be a contiguous int32 [4] tensor")
    hip.require_gpu(out)
    one_device(fn, mask, out, what="the mask and the row")
    hip.call("rpnet_volload_range", hip.ptr(mask), SOURCE_KINDS[mask.dtype], layout, *_window_args(geom), hip.ptr(out))
    return out


def gather_volume(src, geom, lo, hi, pad_value=0.0, out=None):
    """float32 [hi - lo, ch, cw]: slices lo .. hi - 1 of `src` (uint8, int16 or float32 [D,H,W], contiguous or in file order) truncated, padded to 16,
    centre-cropped and padded to crop_size in one launch; every pad holds float32(pad_value)"""
    fn = "gather_volume"
    layout, shape = _source(fn, src, tuple(SOURCE_KINDS), "src")
    if shape != (geom["D"], geom["H"], geom["W"]):
        raise ValueError(f"{fn}: src {shape} is not the file shape {(geom['D'], geom['H'], geom['W'])} of the geometry")
    lo, hi = int(lo), int(hi)
    if not 0 <= lo < hi <= geom["nz"]:
        raise ValueError(f"{fn}: lo={lo} hi={hi} must satisfy 0 <= lo < hi <= {geom['nz']} (the host reader is {HOST_READER})")
    want = (hi - lo, geom["ch"], geom["cw"])
    if out is None:
        out = torch.empty(want, device=src.device, dtype=torch.float32)
    elif not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != want or not out.is_contiguous():
        raise ValueError(f"{fn}: out must be a contiguous float32 tensor of shape {want}")
    hip.require_gpu(out)
    one_device(fn, src, out, what="the volumes")
    hip.call("rpnet_volload_gather", hip.ptr(src), SOURCE_KINDS[src.dtype], layout, *_window_args(geom), lo, hi, geom["ch"], geom["cw"],
             float(pad_value), hip.ptr(out))
    return out


def _flat_f32(fn, x, what="x"):
    hip.require_gpu(x)
    if not torch.is_tensor(x) or x.dtype != torch.float32 or not x.is_contiguous() or not 1 <= x.numel() <= MAX_VALUES:
        raise ValueError(f"{fn}: {what} must be a contiguous float32 tensor of 1..{MAX_VALUES} values, got "
                         f"{getattr(x, 'dtype', type(x))} {tuple(getattr(x, 'shape', ()))}")
    return x.numel()


def order_statistics(x, ranks, out=None):
    """the values of the two `ranks` (k0 <= k1 <= n - 1) of the ascending order of the float32 tensor `x`, in which -0.0 == +0.0 and
    NaNs stand last (numpy's sort) -> int32 [4] on the device: the bits of the two float32 values, the number of NaNs, 0
    (`out[:2].view(torch.float32)` are the values).  Nine launches, nothing read back."""
    fn = "order_statistics"
    n = _flat_f32(fn, x)
    k0, k1 = (int(k) for k in ranks)
    if not 0 <= k0 <= k1 <= n - 1:
        raise ValueError(f"{fn}: ranks {(k0, k1)} of {n} values must satisfy 0 <= k0 <= k1 <= n - 1")
    if out is None:
        out = torch.empty(4, device=x.device, dtype=torch.int32)
    elif not torch.is_tensor(out) or out.dtype != torch.int32 or out.shape != (4,) or not out.is_contiguous():
        raise ValueError(f"{fn}: out must be a contiguous int32 [4] tensor")
    hip.require_gpu(out)
    one_device(fn, x, out, what="the values and the row")
    ws, nbytes = _workspaces.get("rpnet_volload_select_workspace_bytes", x.device, (n,))
    hip.call("rpnet_volload_select", hip.ptr(x), n, k0, k1, hip.ptr(out), hip.ptr(ws), nbytes)
    return out


def percentile_rank(n, q):
    """(k0, k1, g): the two ranks and the float32 weight with which numpy.percentile(x, q) (method 'linear', numpy >= 2) interpolates a
    float32 array of n values.  numpy forms the virtual index in the dtype of the array: q / 100, (n - 1) * q', the floor and the
    difference are all float32 operations, n - 1 rounded to float32.  Beyond the ends numpy takes the end value twice, and the weight
    is then immaterial: 0 here."""
    f = np.float32
    qq = f(q) / f(100)
    v = f(n - 1) * qq
    if not np.isfinite(v) or not 0.0 <= float(q) <= 100.0:
        raise ValueError(f"percentile_rank: q={q!r} must be within 0..100")
    if v >= n - 1:
        return n - 1, n - 1, f(0)
    if v < 0:
        return 0, 0, f(0)
    k = np.floor(v)
    return int(k), int(k) + 1, f(v - k)


def percentile_f32(x, q):
    """numpy.percentile(x, q) of a float32 tensor, on the device -> a float32 scalar tensor (a NaN where x holds one): the selection,
    then numpy's _lerp in float32 as torch spells it one rounding at a time.  Nothing is read back."""
    n = _flat_f32("percentile_f32", x)
    k0, k1, g = percentile_rank(n, q)
    st = order_statistics(x, (k0, k1))
    a, b = st[:2].view(torch.float32).unbind(0)
    d = b - a
    top = b - d * float(np.float32(1) - g) if g >= 0.5 else a + d * float(g)
    return torch.where(st[2] != 0, torch.full_like(top, float("nan")), top)


def window_normalize(x, minimum, maximum, top_percent=0.5, out=None):
    """the reader's `normalize` of a float32 tensor on the device: clip at the (100 - top_percent)th percentile of all of x, clip to
    [minimum, maximum], map to [-1, 1].  out: None (a new tensor), x itself (in place) or a tensor of the shape of x.  Ten launches
    (selection and map), nothing read back; the pair can be captured in a graph."""
    fn = "window_normalize"
    n = _flat_f32(fn, x)
    if out is None:
        out = torch.empty_like(x)
    elif not torch.is_tensor(out) or out.dtype != torch.float32 or out.shape != x.shape or not out.is_contiguous():
        raise ValueError(f"{fn}: out must be a contiguous float32 tensor of shape {tuple(x.shape)}")
    hip.require_gpu(out)
    one_device(fn, x, out, what="the volumes")
    mn, mx = np.float32(minimum), np.float32(maximum)
    den = np.float32(max(1, maximum - minimum))
    if not (np.isfinite(mn) and np.isfinite(mx) and mn <= mx):
        raise ValueError(f"{fn}: minimum {minimum!r} and maximum {maximum!r} must be finite and ordered")
    k0, k1, g = percentile_rank(n, 100.0 - top_percent)
    st = order_statistics(x, (k0, k1))
    hip.call("rpnet_volload_normalize", hip.ptr(x), hip.ptr(out), n, hip.ptr(st), float(g), float(mn), float(mx), float(den))
    return out


def read_payload(path):
    """(the payload of an NRRD file as a flat array in file order and native byte order, its sizes): no transposing copy is made"""
    data, _ = nrrd.read(path)
    return data.reshape(-1, order="F"), tuple(int(s) for s in data.shape)


def upload_payload(flat, shape, device):
    """the flat payload of a file with the sizes D H W on the device, as the [D,H,W] view whose strides are (1, D, D * H)"""
    D, H, W = shape
    return torch.from_numpy(flat).to(device).view(W, H, D).permute(2, 1, 0)


class DeviceVolumeLoader:
    """load(pid, roi) -> (image, mask), float32 [d, ch, cw] on `device`, bit for bit the pair of `reader.load_image_and_mask(pid, roi)`.
    The payloads go up in their file dtype (an int16 volume is half the bytes of the float32 one the host route uploads); one 16-byte
    readback per volume fetches the annotated z range, on which the output's shape depends; there is no other host synchronisation.
    What the kernels do not serve is refused, never handed to the host reader silently."""

    def __init__(self, reader, device):
        self.reader, self.device = reader, torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"DeviceVolumeLoader runs on MI355X only (there is no CPU fallback; the host reader is {HOST_READER})")
        self.last_read_seconds = None                 # the time the last load spent reading and decoding its two files

    def load(self, pid, roi):
        import time
        rd, cfg = self.reader, self.reader.cfg
        t0 = time.perf_counter()
        m_flat, m_shape = read_payload(os.path.join(rd.data_dir, f"{pid}_{roi}.nrrd"))
        v_flat, v_shape = read_payload(os.path.join(rd.data_dir, f"{pid}_clean.nrrd"))
        self.last_read_seconds = time.perf_counter() - t0
        return self.load_arrays(v_flat, m_flat, v_shape, m_shape, f"{pid} / {roi}")

    def load_arrays(self, v_flat, m_flat, v_shape, m_shape, what="volume"):
        """load() after the files have been read: the flat payloads and their sizes"""
        cfg = self.reader.cfg
        if len(v_shape) != 3 or tuple(m_shape) != tuple(v_shape):
            raise ValueError(f"DeviceVolumeLoader: {what}: image {tuple(v_shape)} and mask {tuple(m_shape)} must be one [D,H,W] shape "
                             f"(the host reader is {HOST_READER})")
        if v_flat.dtype not in (np.int16, np.float32):
            raise ValueError(f"DeviceVolumeLoader: {what}: the image is {v_flat.dtype}; int16 and float32 images are loaded on the device "
                             f"(the host reader is {HOST_READER})")
        if m_flat.dtype not in (np.uint8, np.int16, np.float32):
            raise ValueError(f"DeviceVolumeLoader: {what}: the mask is {m_flat.dtype}; uint8, int16 and float32 masks are loaded on the "
                             f"device (the host reader is {HOST_READER})")
        pad = cfg["pad_value"]
        try:
            held = bool(np.isfinite(pad)) and float(v_flat.dtype.type(pad)) == float(pad) == float(np.float32(pad))
        except (OverflowError, ValueError):
            held = False
        if not held:
            raise ValueError(f"DeviceVolumeLoader: {what}: pad_value {pad!r} is not held exactly by {v_flat.dtype} and float32 "
                             f"(the host reader is {HOST_READER})")
        geom = load_geometry(cfg, v_shape)
        mask = upload_payload(m_flat, m_shape, self.device)
        image = upload_payload(v_flat, v_shape, self.device)
        first, last, count, _ = annotated_range(mask, geom).tolist()          # the one readback: 16 bytes
        if count == 0:
            raise ValueError(f"DeviceVolumeLoader: {what}: the mask is empty inside the window, as zero-size array to reduction operation "
                             f"minimum in the host reader ({HOST_READER})")
        if first == last:
            raise ValueError(f"DeviceVolumeLoader: {what}: one annotated slice (z = {first}) gives an empty volume [lo:hi) "
                             f"(the host reader {HOST_READER} returns a volume of depth 0)")
        hu = cfg["HU_range"]
        out_mask = gather_volume(mask, geom, first, last, 0.0)
        out_image = gather_volume(image, geom, first, last, float(pad))
        window_normalize(out_image, hu[0], hu[1], out=out_image)
        return out_image, out_mask
