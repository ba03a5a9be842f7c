"""Raw volumes -> the preprocessed data set FewshotVolumeReader and train_rpnet.py --data_dir read, on the device
(rpnet_amd.preprocess): what the reference's utils/preprocess_abd_110.py does through SimpleITK on four host processes.

  python tools/preprocess_volumes.py --raw-dir RAW --save-dir OUT [--radius 7] [--threshold otsu|T] [--fill -1024] [--inclusive-crop]
                                     [--rois Liver Spleen ...] [--resample Z,Y,X [--resample-align corner|center]
                                     [--mask-interp linear|nearest] [--antialias]]

Reads RAW/<pid>/img.nrrd and RAW/<pid>/structures/<roi>.nrrd (axes x, y, z as the reference's files have them), swaps the axes to
[D, H, W] as the reference does, masks the volume with its body mask, crops image and structures to the box of what is left above the
fill value, and writes OUT/<pid>_clean.nrrd, OUT/<pid>_<roi>.nrrd (uint8) and OUT/<pid>_bbox.npy in the reference's form
[[z_start, y_start, x_start], [z_start + D, y_end, x_end]] (z_start is 0: z is never cropped; y_end, x_end are the bounds the crop
used, the reference's yy.max(), xx.max(), one more with --inclusive-crop).  The per-axis spacing of the input header is carried into
the output headers in the order of the swapped axes, so spacing="header" keeps working downstream.  One line per volume: the box and
the voxels of the mask after each stage.

--resample Z,Y,X takes the image and every structure to that spacing in millimetres (rpnet_amd.resample) before the body mask and the
crop, in the reference's order (its do_resample): the grid is resample.output_shape of the input's shape and header spacing, the image is
resampled trilinearly, a structure by --mask-interp: linear (the default, the reference's `resample(mask) > 0.5`; it takes the voxels of
value 1, which is what the reference's 0 / 1 structure files hold) or nearest.  The output headers then carry the spacing the new grid
really has (resample.out_spacing), so spacing="header" downstream reports millimetres on the new grid, and bbox.npy is formed from the
resampled shape.  The input header must carry a spacing.  Without --resample the files are byte for byte what they were.
--antialias (read with --resample, on the image only) smooths every axis of the image that shrinks before it is resampled
(rpnet_amd.smooth: a Gaussian of (n / m - 1) / 2 voxels on an axis that goes from n to m, border "nearest"), so that what lies above the
new grid's Nyquist limit does not fold into the image; the structures keep the indicator rule.  Without it the files are byte for byte
what --resample alone writes.

Not written: the reference's <pid>_raw.npy and the combined _masks file; z_starts is switched off in the reference and absent here;
DICOM input is not read."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from rpnet_amd import preprocess as PP
from rpnet_amd import resample as RS
from rpnet_amd.surface_spacing import spacing_from_header
from rpnet_amd.utils import nrrd


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--raw-dir", required=True, help="one directory per volume: <pid>/img.nrrd, <pid>/structures/<roi>.nrrd")
    ap.add_argument("--save-dir", required=True)
    ap.add_argument("--radius", type=float, default=7, help="radius of the closing / opening ball in pixels (the reference's 7)")
    ap.add_argument("--threshold", default="otsu", help="'otsu' (per slice) or a fixed value")
    ap.add_argument("--fill", type=float, default=-1024, help="the value outside the mask")
    ap.add_argument("--inclusive-crop", action="store_true", help="keep the last row and column of the box (the reference drops them)")
    ap.add_argument("--rois", nargs="*", default=None, help="structure names; default: every file under structures/")
    ap.add_argument("--resample", default=None, metavar="Z,Y,X", help="resample image and structures to this spacing in mm before the body mask")
    ap.add_argument("--resample-align", choices=("corner", "center"), default="corner", help="which points of the two grids coincide")
    ap.add_argument("--mask-interp", choices=("linear", "nearest"), default="linear", help="how a structure is resampled (linear: > 0.5)")
    ap.add_argument("--antialias", action="store_true", help="with --resample: smooth the axes of the image that shrink before resampling it")
    ap.add_argument("--device", default="cuda:0")
    return ap


def image_array(data):
    """the axes swapped to [D, H, W]; int16 stays int16, everything else becomes float32"""
    a = np.swapaxes(np.asarray(data), 0, -1)
    return np.ascontiguousarray(a if a.dtype == np.int16 else a.astype(np.float32))


def spacing_fields(header, resampled=None):
    """the header fields that carry the input's spacing in the order of the swapped axes, or None when the input has none; resampled:
    the (sz, sy, sx) of the new grid, written in its place"""
    if resampled is not None:
        sz, sy, sx = resampled
    else:
        try:
            s = spacing_from_header(header)             # of the file's axes x, y, z
        except ValueError:
            return None
        sz, sy, sx = s[2], s[1], s[0]
    return {"space": "left-posterior-superior", "space directions": f"({sz!r},0,0) (0,{sy!r},0) (0,0,{sx!r})"}


def parse_spacing(text):
    """'Z,Y,X' -> (sz, sy, sx) in millimetres"""
    try:
        s = tuple(float(v) for v in text.split(","))
    except ValueError:
        s = ()
    if len(s) != 3 or not all(np.isfinite(v) and v > 0 for v in s):
        raise SystemExit(f"--resample wants three positive numbers Z,Y,X in millimetres, got {text!r}")
    return s


def resample_all(pid, image, structures, header, new_spacing, align, mask_interp, antialias=False):
    """the image and every structure (device tensors) at `new_spacing` -> (image, structures, the spacing of the new grid); antialias:
    the image is smoothed on the axes that shrink first"""
    try:
        s = spacing_from_header(header)
    except ValueError as e:
        raise ValueError(f"{pid}: --resample needs the spacing of the input and img.nrrd carries none ({e})")
    spacing = (s[2], s[1], s[0])
    image, grid_spacing = RS.resample_to_spacing(image, spacing, new_spacing, align=align, **({"antialias": True} if antialias else {}))
    options = {"classes": (1,), "mode": "linear"} if mask_interp == "linear" else {"mode": "nearest"}
    structures = {roi: RS.resample_like(m, tuple(image.shape), align=align, **options) for roi, m in structures.items()}
    return image, structures, grid_spacing


def preprocess_one(pid, raw_dir, save_dir, device, radius=7, threshold="otsu", fill=-1024, inclusive_crop=False, rois=None, resample=None,
                   resample_align="corner", mask_interp="linear", antialias=False):
    data, header = nrrd.read(os.path.join(raw_dir, pid, "img.nrrd"))
    if data.ndim != 3:
        raise ValueError(f"{pid}: img.nrrd has {data.ndim} axes, a volume has 3")
    image = image_array(data)
    sdir = os.path.join(raw_dir, pid, "structures")
    if rois is None:
        rois = sorted(f[:-5] for f in os.listdir(sdir) if f.endswith(".nrrd")) if os.path.isdir(sdir) else []
    structures = {}
    for roi in rois:
        path = os.path.join(sdir, f"{roi}.nrrd")
        if not os.path.isfile(path):
            print(f"{pid} does not have {roi}")
            continue
        m = np.ascontiguousarray(np.swapaxes(nrrd.read(path)[0], 0, -1).astype(np.uint8))
        if m.shape != image.shape:
            raise ValueError(f"{pid}: structure {roi} is {m.shape}, the image {image.shape}")
        structures[roi] = torch.from_numpy(m).to(device)
    volume, grid_spacing = torch.from_numpy(image).to(device), None
    if resample is not None:
        volume, structures, grid_spacing = resample_all(pid, volume, structures, header, resample, resample_align, mask_interp, antialias)
    res = PP.clean_volume(volume, structures, fill=fill, reference_crop=not inclusive_crop, radius=radius, threshold=threshold)
    y0, y1, x0, x1 = res["box"]
    extra = spacing_fields(header, grid_spacing)
    os.makedirs(save_dir, exist_ok=True)
    clean = res["image"].cpu().numpy()
    nrrd.write(os.path.join(save_dir, f"{pid}_clean.nrrd"), clean, header=extra)
    for roi, m in res["structures"].items():
        nrrd.write(os.path.join(save_dir, f"{pid}_{roi}.nrrd"), m.cpu().numpy(), header=extra)
    bbox = np.array([[0, y0, x0], [volume.shape[0], y1, x1]])
    np.save(os.path.join(save_dir, f"{pid}_bbox.npy"), bbox)
    voxels = res["tables"]["voxels"].cpu().numpy().tolist()
    print(f"{pid} {tuple(clean.shape)} box y {y0}:{y1} x {x0}:{x1} kept " + " ".join(f"{n} {v}" for n, v in zip(PP.STAGES, voxels))
          + (" (no spacing in the input header)" if extra is None else ""))
    return {"pid": pid, "shape": tuple(clean.shape), "bbox": bbox, "voxels": voxels, "rois": sorted(res["structures"])}


def main(argv=None):
    a = build_parser().parse_args(argv)
    threshold = "otsu" if a.threshold == "otsu" else float(a.threshold)
    pids = sorted(p for p in os.listdir(a.raw_dir) if os.path.isfile(os.path.join(a.raw_dir, p, "img.nrrd")))
    if not pids:
        raise SystemExit(f"no <pid>/img.nrrd under {a.raw_dir}")
    resample = None if a.resample is None else parse_spacing(a.resample)
    if a.antialias and resample is None:
        raise SystemExit("--antialias is read with --resample: there is nothing to prefilter without it")
    return [preprocess_one(pid, a.raw_dir, a.save_dir, a.device, a.radius, threshold, a.fill, a.inclusive_crop, a.rois, resample, a.resample_align,
                           a.mask_interp, a.antialias) for pid in pids]


if __name__ == "__main__":
    main()
