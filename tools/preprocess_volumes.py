"""Raw volumes -> the preprocessed data set FewshotVolumeReader and train_rpnet.py --data_dir read, on the device
(rpnet_amd.preprocess): what the reference's utils/preprocess_abd_110.py does through SimpleITK on four host processes.

  python tools/preprocess_volumes.py --raw-dir RAW --save-dir OUT [--radius 7] [--threshold otsu|T] [--fill -1024] [--inclusive-crop]
                                     [--rois Liver Spleen ...]

Reads RAW/<pid>/img.nrrd and RAW/<pid>/structures/<roi>.nrrd (axes x, y, z as the reference's files have them), swaps the axes to
[D, H, W] as the reference does, masks the volume with its body mask, crops image and structures to the box of what is left above the
fill value, and writes OUT/<pid>_clean.nrrd, OUT/<pid>_<roi>.nrrd (uint8) and OUT/<pid>_bbox.npy in the reference's form
[[z_start, y_start, x_start], [z_start + D, y_end, x_end]] (z_start is 0: z is never cropped; y_end, x_end are the bounds the crop
used, the reference's yy.max(), xx.max(), one more with --inclusive-crop).  The per-axis spacing of the input header is carried into
the output headers in the order of the swapped axes, so spacing="header" keeps working downstream.  One line per volume: the box and
the voxels of the mask after each stage.

Not written: the reference's <pid>_raw.npy and the combined _masks file; resampling and z_starts are switched off in the reference and
absent here; DICOM input is not read."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from rpnet_amd import preprocess as PP
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
    ap.add_argument("--device", default="cuda:0")
    return ap


def image_array(data):
    """the axes swapped to [D, H, W]; int16 stays int16, everything else becomes float32"""
    a = np.swapaxes(np.asarray(data), 0, -1)
    return np.ascontiguousarray(a if a.dtype == np.int16 else a.astype(np.float32))


def spacing_fields(header):
    """the header fields that carry the input's spacing in the order of the swapped axes, or None when the input has none"""
    try:
        s = spacing_from_header(header)             # of the file's axes x, y, z
    except ValueError:
        return None
    sz, sy, sx = s[2], s[1], s[0]
    return {"space": "left-posterior-superior", "space directions": f"({sz!r},0,0) (0,{sy!r},0) (0,0,{sx!r})"}


def preprocess_one(pid, raw_dir, save_dir, device, radius=7, threshold="otsu", fill=-1024, inclusive_crop=False, rois=None):
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
    res = PP.clean_volume(torch.from_numpy(image).to(device), structures, fill=fill, reference_crop=not inclusive_crop, radius=radius,
                          threshold=threshold)
    y0, y1, x0, x1 = res["box"]
    extra = spacing_fields(header)
    os.makedirs(save_dir, exist_ok=True)
    clean = res["image"].cpu().numpy()
    nrrd.write(os.path.join(save_dir, f"{pid}_clean.nrrd"), clean, header=extra)
    for roi, m in res["structures"].items():
        nrrd.write(os.path.join(save_dir, f"{pid}_{roi}.nrrd"), m.cpu().numpy(), header=extra)
    bbox = np.array([[0, y0, x0], [image.shape[0], y1, x1]])
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
    return [preprocess_one(pid, a.raw_dir, a.save_dir, a.device, a.radius, threshold, a.fill, a.inclusive_crop, a.rois) for pid in pids]


if __name__ == "__main__":
    main()
