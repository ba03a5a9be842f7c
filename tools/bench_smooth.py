"""Timing of rpnet_amd.smooth on the MI355X: the lines for profiles/smooth.txt.

  python tools/bench_smooth.py [--reps 20] [--inner 20] [--skip-host] > profiles/smooth.txt

smooth_image (float32 and int16) on a 64 x 256 x 256 and a 64 x 512 x 512 volume at sigma 0.75 (the prefilter of the reference's 2.5-fold
shrink), 2 and 8 voxels on every axis, and resample_image 64 x 512 x 512 -> 80 x 205 x 205 with and without `antialias`.  A sample is
--inner calls between two events divided by --inner; the line gives the median of --reps samples with min and max, the bytes the three
passes of csrc/smooth.hip have to move (the volume read, two float64 intermediates written and read, the volume written: 40 B per float32
voxel, 36 per int16 voxel), that traffic per second, and it as a share of the 6.29 TB/s copy rate of the README; beside it the rate
against the 8 B (4 B) per voxel that no design can go below.  Beside them the host route, scipy.ndimage.gaussian_filter on the same box
and the same volume, one run, with the outputs compared first: within twice the bound tests/smooth_cases.py derives plus one float32
rounding.  The per-pass lines at the end of profiles/smooth.txt are not written here: they are the means of a kernel trace
(rocprofv3 --kernel-trace --stats, a run of its own) over 40 calls of smooth_image on the 64 x 512 x 512 volume."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from scipy import ndimage

from rpnet_amd import resample as RS
from rpnet_amd import smooth as SM
from tests import smooth_cases as SC
from tools.bench_resample import COPY_RATE, timed


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_smooth.py measures on the MI355X; there is no device here")
    dev = "cuda:0"
    for shape in ((64, 256, 256), (64, 512, 512)):
        n = int(np.prod(shape))
        img, i16 = SC.noise_image(shape, np.float32, seed=1), SC.noise_image(shape, np.int16, seed=1)
        vol, vol16 = torch.from_numpy(img).to(dev), torch.from_numpy(i16).to(dev)
        outf, out16 = torch.empty_like(vol), torch.empty_like(vol16)
        for sigma in (0.75, 2.0, 8.0):
            if not a.skip_host and sigma == 0.75:
                t0 = time.perf_counter()
                want = ndimage.gaussian_filter(img.astype(np.float64), sigma, mode="reflect")
                host = (time.perf_counter() - t0) * 1e3
                got = SM.smooth_image(vol, sigma).cpu().numpy().astype(np.float64)
                bound = 2.0 * SC.error_bound(img, (sigma,) * 3) + 2.0 ** -24 * np.abs(want)
                err = np.abs(got - want)
                assert np.all(err <= bound), f"the device differs from scipy.ndimage.gaussian_filter by {err.max():.3e}"
                print(f"{shape} sigma {sigma} host route scipy.ndimage.gaussian_filter, one run: {host:.1f} ms (max difference {err.max():.2e}, "
                      f"within the derived bound everywhere)")
            for name, v, o, size in (("float32", vol, outf, 4), ("int16", vol16, out16, 2)):
                t = timed(lambda: SM.smooth_image(v, sigma, out=o), a.reps, a.inner)
                moved, floor = n * (2 * size + 32), n * 2 * size
                rate = moved / (t[0] * 1e-3)
                print(f"{shape} smooth_image {name} sigma {sigma} (radius {SC.weights(sigma)[1]}): {t[0]:.4f} ms ({t[1]:.4f} .. {t[2]:.4f}), "
                      f"{moved / 1e6:.1f} MB moved by three passes, {rate / 1e12:.3f} TB/s = {100 * rate / COPY_RATE:.1f}% of the copy rate; "
                      f"the {floor / 1e6:.1f} MB floor at the copy rate is {floor / COPY_RATE * 1e3:.4f} ms")
    shape, grid = (64, 512, 512), (80, 205, 205)
    vol = torch.from_numpy(SC.noise_image(shape, np.float32, seed=1)).to(dev)
    out = torch.empty(grid, device=dev, dtype=torch.float32)
    for flag in (False, True):
        t = timed(lambda: RS.resample_image(vol, grid, out=out, antialias=flag), a.reps, a.inner)
        print(f"{shape} -> {grid} resample_image float32 linear antialias={flag} (sigma {SM.antialias_sigma(shape, grid)}): "
              f"{t[0]:.4f} ms ({t[1]:.4f} .. {t[2]:.4f})")


if __name__ == "__main__":
    main()
