"""Body-mask preprocessing of a raw CT volume on the device (csrc/prep.hip, include/rpnet_prep_abi.h): what the reference's
utils/preprocess_abd_110.py does per axial slice through SimpleITK on the host, and what makes the `<pid>_clean.nrrd` and `<pid>_<roi>.nrrd`
files FewshotVolumeReader and train_rpnet.py --data_dir read (tools/preprocess_volumes.py is the driver).

The chain of `body_mask`, every z slice on its own: an Otsu threshold, a closing and an opening by a ball (morphology.closing / opening with
per_slice=True), the connected region of the centre pixel, hole filling (postprocess.fill_holes in slice mode).  `clean_volume` then sets
the voxels outside the mask to `fill` and finds the bounding box of the voxels above `fill`.

Definitions (word for word those of include/rpnet_prep_abi.h; tests/preprocess_cases.py restates them in numpy, bit for bit).  An image is
[D,H,W] float32 or int16.  fl(.) is one float64 rounding.

Fixed threshold: foreground is `(double)v > t`; NaN is background.
Otsu threshold, per slice: lo and hi are the smallest and largest finite value; non-finite voxels are background; no finite voxel or
hi == lo gives an empty slice and k* = -1; scale = fl(128 / fl(hi - lo)); b(v) = min(127, (int)fl(fl(v - lo) * scale)); with the counts
c_b, N their sum, w(k) = sum_{b<=k} c_b and m(k) = sum_{b<=k} b c_b in int64, val(k) = fl(fl(num * num) / fl(w(k) * (N - w(k)))) for
num = m(127) w(k) - m(k) N over k = 0..126 with 0 < w(k) < N; k* is the first k with the largest val; foreground is b(v) > k*; the
reported threshold is fl(lo + fl((k* + 1) * fl(fl(hi - lo) / 128))).  The rows of a slice: int64 {n_finite, k*, n_foreground, 0} and
float64 {lo, hi, threshold} (no finite voxel: lo = hi = 0; fixed mode: k* = -1 and the threshold is t).
Seeded component, per slice: the pixels of the class connected to the seed pixel under connectivity 4 or 8 keep the class, every other
pixel of the class becomes 0 (all of them when the seed pixel is not of the class), other values pass through.  The row of a slice:
int64 {seed_hit, voxels_before, voxels_kept, n_components}.
Mask and box: out = mask ? img : fill; the box is taken over `mask && (double)img > (double)fill`, as the reference takes it over
`processed_image > -1024`.  The row: int64 {zmin, zmax, ymin, ymax, xmin, xmax, n_kept, n_mask}, inclusive, six times -1 when nothing
is kept.

Not claimed: parity with SimpleITK.  OtsuThreshold bins and returns its threshold by ITK's own calculator (the mask is the same whenever
that picks the same bin); BinaryMorphologicalClosing / Opening rasterise their ball as an ellipsoid by ITK's own rule and handle the
border their own way (see morphology.py: the ball here is {dy^2 + dx^2 <= floor(r^2)}, and outside the slice counts as object in an erosion
unless erode_border=0).  Everything is integer work or separately rounded float64 with integer atomics: two runs give the same bits.
"""
import math

import numpy as np
import torch

from . import hip, morphology, postprocess
from ._volume_checks import WorkspaceCache, check_table, one_device

IMAGE_KINDS = {torch.float32: 0, torch.int16: 1}    # RPNET_PREP_F32, RPNET_PREP_I16
FIXED, OTSU = 0, 1                                  # RPNET_PREP_FIXED, RPNET_PREP_OTSU
THRESHOLD_ROW, THRESHOLD_FROW, SEED_ROW, BBOX_ROW = 4, 3, 4, 8     # RPNET_PREP_*_ROW
OVERRUN_OFFSET = 24                                 # RPNET_CC_OVERRUN_OFFSET
STAGES = ("threshold", "closing", "opening", "seed", "holes")
_thr_ws = WorkspaceCache(by_shape=False)
_seed_ws = WorkspaceCache(by_shape=True)            # seed_overrun() reads the word a call left in the buffer of its shape
_box_ws = WorkspaceCache(by_shape=False)


def _check_image(t, what, fn):
    if not torch.is_tensor(t) or t.dtype not in IMAGE_KINDS:
        raise ValueError(f"{fn}: {what} is {getattr(t, 'dtype', type(t))}; float32 and int16 images are accepted")
    if t.dim() != 3 or not t.is_contiguous():
        raise ValueError(f"{fn}: {what} must be a contiguous [D,H,W] tensor, got {tuple(t.shape)}")


def _check_mask(t, shape, what, fn):
    if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.dim() != 3 or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError(f"{fn}: {what} must be a contiguous uint8 [D,H,W] tensor" + (f" of shape {tuple(shape)}" if shape is not None else ""))


def threshold_mask(vol, threshold="otsu", out=None, rows=None, frows=None):
    """The 0/1 mask of every slice of `vol` (float32 or int16 [D,H,W]), one `rpnet_prep_threshold` call on the current stream ->
    (mask uint8 [D,H,W], rows int64 [D,4] {n_finite, k*, n_foreground, 0}, frows float64 [D,3] {lo, hi, threshold}).  threshold: "otsu"
    (per slice, the definition above) or a number t (foreground is v > t).  Launches only: nothing is copied or synchronised."""
    fn = "threshold_mask"
    hip.require_gpu(vol, out, rows, frows)
    _check_image(vol, "vol", fn)
    if isinstance(threshold, str):
        if threshold != "otsu":
            raise ValueError(f"{fn}: threshold must be 'otsu' or a number, got {threshold!r}")
        mode, t = OTSU, 0.0
    elif isinstance(threshold, (int, float, np.integer, np.floating)) and not isinstance(threshold, bool) and not math.isnan(float(threshold)):
        mode, t = FIXED, float(threshold)
    else:
        raise ValueError(f"{fn}: threshold must be 'otsu' or a number that is not NaN, got {threshold!r}")
    D, H, W = vol.shape
    if out is None:
        out = torch.empty(vol.shape, device=vol.device, dtype=torch.uint8)
    _check_mask(out, vol.shape, "out", fn)
    if rows is None:
        rows = torch.zeros((D, THRESHOLD_ROW), device=vol.device, dtype=torch.int64)
    if frows is None:
        frows = torch.zeros((D, THRESHOLD_FROW), device=vol.device, dtype=torch.float64)
    check_table(rows, D, THRESHOLD_ROW, torch.int64, "rows", fn)
    check_table(frows, D, THRESHOLD_FROW, torch.float64, "frows", fn)
    one_device(fn, vol, out, rows, frows)
    ws, nbytes = _thr_ws.get("rpnet_prep_threshold_workspace_bytes", vol.device, (D, H, W))
    hip.call("rpnet_prep_threshold", hip.ptr(vol), IMAGE_KINDS[vol.dtype], hip.ptr(out), D, H, W, mode, t, hip.ptr(rows), hip.ptr(frows), hip.ptr(ws),
             nbytes)
    return out, rows, frows


def check_seed(seed, H, W, fn="seeded_component"):
    """the `seed` option -> (y, x) inside the slice; None is the centre pixel (H // 2, W // 2)"""
    if seed is None:
        return H // 2, W // 2
    if (isinstance(seed, (tuple, list)) and len(seed) == 2 and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in seed)
            and 0 <= int(seed[0]) < H and 0 <= int(seed[1]) < W):
        return int(seed[0]), int(seed[1])
    raise ValueError(f"{fn}: seed must be None or (y, x) inside the {H} x {W} slice, got {seed!r}")


def seeded_component(mask, classes, seed=None, connectivity=4, out=None, stats=None):
    """Keep, in every z slice, only the pixels of each class in `classes` that are connected to the seed pixel, one
    `rpnet_prep_seeded_component` call per class on the current stream -> (out uint8 [D,H,W], stats int64 [len(classes), D, 4]
    {seed_hit, voxels_before, voxels_kept, n_components} per slice).  mask: uint8 [D,H,W]; out may be `mask` itself.  connectivity: 4
    or 8 within the slice; there is no link across z.  A slice whose seed pixel is not of the class loses the class.

    seed: (y, x), row then column; the default is the centre pixel (H // 2, W // 2).  The reference hands (H // 2, W // 2) to ITK's
    ConnectedThreshold, which reads a seed as an (x, y) index; on the square slices it is used with that is the same pixel, and on a
    slice that is not square this function takes (y, x) as written here.  Launches only: nothing is copied or synchronised."""
    fn = "seeded_component"
    hip.require_gpu(mask, out, stats)
    _check_mask(mask, None, "mask", fn)
    classes = [int(c) for c in classes]
    if not classes:
        raise ValueError(f"{fn}: no class to process")
    if connectivity not in (4, 8):
        raise ValueError(f"{fn}: connectivity must be 4 or 8 (every slice is its own image), got {connectivity!r}")
    D, H, W = mask.shape
    sy, sx = check_seed(seed, H, W, fn)
    if out is None:
        out = torch.empty(mask.shape, device=mask.device, dtype=torch.uint8)
    _check_mask(out, mask.shape, "out", fn)
    if stats is None:
        stats = torch.zeros((len(classes), D, SEED_ROW), device=mask.device, dtype=torch.int64)
    if not torch.is_tensor(stats) or stats.dtype != torch.int64 or tuple(stats.shape) != (len(classes), D, SEED_ROW) or not stats.is_contiguous():
        raise ValueError(f"{fn}: stats must be a contiguous int64 [{len(classes)}, {D}, {SEED_ROW}] tensor")
    one_device(fn, mask, out, stats)
    ws, _ = _seed_ws.get("rpnet_prep_seeded_component_workspace_bytes", mask.device, (D, H, W))
    src = mask
    for r, c in enumerate(classes):
        hip.call("rpnet_prep_seeded_component", hip.ptr(src), hip.ptr(out), c, D, H, W, sy, sx, int(connectivity), hip.ptr(stats[r]), hip.ptr(ws),
                 ws.numel())
        src = out
    return out, stats


def seed_overrun(device, shape):
    """the `overrun` word the last seeded_component call on a volume of this shape left in its workspace (0 unless a bounded loop of
    the labelling ran out of its bound); a device-to-host copy, for tests and diagnosis: the row says the same by n_components = -1"""
    ws, _ = _seed_ws.get("rpnet_prep_seeded_component_workspace_bytes", torch.device(device), shape)
    return int(ws[OVERRUN_OFFSET:OVERRUN_OFFSET + 4].view(torch.int32).item())


def mask_bbox(vol, mask, fill=-1024, out=None, rows=None, row=0):
    """out = mask ? vol : fill in the kind of `vol`, and the box of the voxels with mask and vol > fill, one `rpnet_prep_mask_bbox` call
    on the current stream -> (out, rows int64 [n, 8]; rows[row] = {zmin, zmax, ymin, ymax, xmin, xmax, n_kept, n_mask}).  out may be
    `vol` itself.  Launches only: nothing is copied or synchronised."""
    fn = "mask_bbox"
    hip.require_gpu(vol, mask, out, rows)
    _check_image(vol, "vol", fn)
    _check_mask(mask, vol.shape, "mask", fn)
    if out is None:
        out = torch.empty_like(vol)
    if out.dtype != vol.dtype or out.shape != vol.shape or not out.is_contiguous():
        raise ValueError(f"{fn}: out must be a contiguous {vol.dtype} tensor of shape {tuple(vol.shape)}")
    if rows is None:
        rows = torch.zeros((1, BBOX_ROW), device=vol.device, dtype=torch.int64)
    check_table(rows, None, BBOX_ROW, torch.int64, "rows", fn)
    one_device(fn, vol, mask, out, rows)
    D, H, W = vol.shape
    ws, nbytes = _box_ws.get("rpnet_prep_mask_bbox_workspace_bytes", vol.device, (D, H, W))
    hip.call("rpnet_prep_mask_bbox", hip.ptr(vol), IMAGE_KINDS[vol.dtype], hip.ptr(mask), hip.ptr(out), float(fill), D, H, W, hip.ptr(rows), int(row),
             rows.shape[0], hip.ptr(ws), nbytes)
    return out, rows


def body_mask(vol, radius=7, threshold="otsu", seed=None, connectivity=4, hole_connectivity=4, erode_border=1):
    """The body mask of a raw volume, every z slice on its own: threshold -> morphology.closing(per_slice=True) ->
    morphology.opening(per_slice=True) -> seeded_component -> postprocess.fill_holes('slice'), all on the current stream ->
    (mask uint8 [D,H,W] of 0 / 1, tables).  tables, all on the device: 'threshold' int64 [D,4] and 'threshold_f' float64 [D,3]
    (threshold_mask), 'closing' and 'opening' int64 [1,4] (morphology: before, after, added, removed over the volume), 'seed' int64 [D,4]
    (seeded_component), 'holes' int64 [1,4] (postprocess.fill_holes), and 'voxels' int64 [5]: the voxels of the mask after each stage of
    STAGES, summed from those rows.  radius: of the ball, as morphology takes it (7 is the reference's); seed: (y, x), None for the centre
    pixel (see seeded_component).

    Not claimed: ITK's rasterised ball and its border handling (BinaryMorphologicalClosing / Opening), nor the bin ITK's Otsu calculator
    picks; the definitions are those of this module and of morphology.py.  Launches only: nothing is copied or synchronised."""
    m, rows, frows = threshold_mask(vol, threshold)
    _, _, closing = morphology.closing(m, (1,), radius, per_slice=True, erode_border=erode_border, out=m)
    _, _, opening = morphology.opening(m, (1,), radius, per_slice=True, erode_border=erode_border, out=m)
    _, seeds = seeded_component(m, (1,), seed=seed, connectivity=connectivity, out=m)
    _, _, holes = postprocess.fill_holes(m, (1,), connectivity=hole_connectivity, per_slice=True, out=m)
    kept = seeds[0, :, 2].sum()
    voxels = torch.stack([rows[:, 2].sum(), closing[0, 1], opening[0, 1], kept, kept + holes[0, 2]])
    return m, {"threshold": rows, "threshold_f": frows, "closing": closing, "opening": opening, "seed": seeds[0], "holes": holes, "voxels": voxels}


def crop_box(bbox_row, reference_crop=True):
    """a host bbox row -> (y0, y1, x0, x1), the slice bounds of the crop: reference_crop cuts [ymin:ymax, xmin:xmax] as the reference does
    (the last row and column of the box are dropped), otherwise [ymin:ymax + 1, xmin:xmax + 1].  z is never cropped.  An empty box, or
    one the reference's crop leaves nothing of, raises."""
    r = [int(v) for v in bbox_row]
    if r[6] == 0 or r[0] < 0:
        raise ValueError("clean_volume: nothing is left above the fill value inside the mask (the box is empty)")
    extra = 0 if reference_crop else 1
    y0, y1, x0, x1 = r[2], r[3] + extra, r[4], r[5] + extra
    if y1 <= y0 or x1 <= x0:
        raise ValueError(f"clean_volume: the reference's half-open crop [{y0}:{y1}, {x0}:{x1}] is empty (reference_crop=False keeps the box)")
    return y0, y1, x0, x1


def clean_volume(vol, structures=None, fill=-1024, reference_crop=True, mask=None, **mask_options):
    """Mask a raw volume with its body mask and crop it to what is left -> a dict:
      'masked'      vol with the voxels outside the mask set to `fill`, [D,H,W] in the kind of `vol`;
      'mask'        the body mask (body_mask(vol, **mask_options) unless `mask` hands one in), 'tables' its tables (None with `mask`);
      'bbox'        the int64 [1,8] row of mask_bbox on the device;
      'box'         (y0, y1, x0, x1) of crop_box, on the host: the one small read, of the bbox row;
      'image'       masked[:, y0:y1, x0:x1], 'structures': {name: s[:, y0:y1, x0:x1]} of the tensors in `structures`, by slicing.
    reference_crop=True cuts [ymin:ymax, xmin:xmax] as the reference does, which drops the last row and column of the box; False
    includes them.  z is never cropped.  An empty box raises.  Nothing else crosses to the host."""
    tables = None
    if mask is None:
        mask, tables = body_mask(vol, **mask_options)
    elif mask_options:
        raise ValueError(f"clean_volume: {sorted(mask_options)} shape the body mask and a mask was handed in")
    structures = dict(structures or {})
    for name, s in structures.items():
        if not torch.is_tensor(s) or tuple(s.shape) != tuple(vol.shape):
            raise ValueError(f"clean_volume: structure {name!r} must be a tensor of shape {tuple(vol.shape)}")
    masked, bbox = mask_bbox(vol, mask, fill)
    y0, y1, x0, x1 = box = crop_box(bbox[0].cpu().numpy(), reference_crop)
    return {"masked": masked, "mask": mask, "tables": tables, "bbox": bbox, "box": box, "image": masked[:, y0:y1, x0:x1],
            "structures": {name: s[:, y0:y1, x0:x1] for name, s in structures.items()}}
