"""Timing of rpnet_amd.resample on the MI355X: the lines for profiles/resample.txt.

  python tools/bench_resample.py [--reps 20] [--inner 20] [--skip-host] > profiles/resample.txt

resample_image (float32 and int16, trilinear and nearest) and resample_labels (three classes, linear and nearest) on a 64 x 256 x 256
and a 64 x 512 x 512 volume taken from a spacing of (2.5, 0.8, 0.8) mm to (2, 2, 2) mm.  A call moves a few megabytes, less than its
launches cost, so a sample is --inner calls between two events divided by --inner; the line gives the median of --reps samples with min
and max, the bytes the call has to move (the input read once, the output written once; a merging label call also reads the output) and
that traffic as a share of the 6.29 TB/s copy rate of the README.  Beside them the host route, scipy.ndimage.zoom on the same box and
the same volumes, one run each, with the outputs compared first: the image within the bound tests/test_host_resample.py derives plus one
float32 rounding, the label map equal away from indicator values within 1e-9 of 0.5."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from scipy import ndimage

from rpnet_amd import resample as RS
from tests import resample_cases as RC

COPY_RATE = 6.29e12         # bytes per second, README: the device-to-device copy rate


def timed(fn, reps, inner):
    """median, min, max in ms per call: `reps` samples of `inner` calls after two warm-up calls, each sample bracketed by events"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return float(np.median(ms)), min(ms), max(ms)


def zoom(v, grid, order):
    return ndimage.zoom(v, [m / n for n, m in zip(v.shape, grid)], order=order, mode="nearest", grid_mode=False)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample.py measures on the MI355X; there is no device here")
    dev = "cuda:0"
    spacing, target, classes = (2.5, 0.8, 0.8), (2.0, 2.0, 2.0), (1, 2, 5)

    def line(what, t, nbytes):
        rate = nbytes / (t[0] * 1e-3)
        print(f"{what}: {t[0]:.4f} ms ({t[1]:.4f} .. {t[2]:.4f}), {nbytes / 1e6:.2f} MB moved, {rate / 1e12:.3f} TB/s = "
              f"{100 * rate / COPY_RATE:.1f}% of the copy rate")

    for shape in ((64, 256, 256), (64, 512, 512)):
        grid = RS.output_shape(shape, spacing, target)
        n_in, n_out = int(np.prod(shape)), int(np.prod(grid))
        img = RC.noise_image(shape, np.float32, seed=1)
        i16 = RC.noise_image(shape, np.int16, seed=1)
        lab = RC.label_map(shape, seed=1)
        vol, vol16, mask = (torch.from_numpy(x).to(dev) for x in (img, i16, lab))
        outf, out16, out8 = (torch.empty(grid, device=dev, dtype=t) for t in (torch.float32, torch.int16, torch.uint8))
        stats = torch.zeros((len(classes), RS.STATS_ROW), device=dev, dtype=torch.int64)
        print(f"{shape} at {spacing} mm -> {grid} at {RS.out_spacing(shape, grid, spacing)} mm")
        if not a.skip_host:
            t0 = time.perf_counter()
            want = zoom(img.astype(np.float64), grid, 1)
            host_img = (time.perf_counter() - t0) * 1e3
            got = RS.resample_image(vol, grid).cpu().numpy()
            vmax, vrange = float(np.abs(img).max()), float(img.max()) - float(img.min())
            bound = 2.0 ** -52 * sum(shape) * vrange + 9 * 2.0 ** -53 * vmax + 2.0 ** -24 * vmax
            err = float(np.abs(got.astype(np.float64) - want).max())
            assert err <= bound, f"the device image differs from scipy.ndimage.zoom by {err:.3e}, bound {bound:.3e}"
            t0 = time.perf_counter()
            zs = [zoom((lab == c).astype(np.float64), grid, 1) for c in classes]
            host_lab = (time.perf_counter() - t0) * 1e3
            got_l = RS.resample_labels(mask, grid, classes, mode="linear")[0].cpu().numpy()
            for c, z in zip(classes, zs):
                clear = np.abs(z - 0.5) > 1e-9
                assert np.array_equal((got_l == c)[clear], (z > 0.5)[clear]), f"class {c} differs from zoom(indicator) > 0.5"
            t0 = time.perf_counter()
            zn = zoom(lab, grid, 0)
            host_near = (time.perf_counter() - t0) * 1e3
            got_n = RS.resample_labels(mask, grid)[0].cpu().numpy()
            ties = [RC.has_exact_tie(n, m, "corner") for n, m in zip(shape, grid)]
            assert any(ties) or np.array_equal(got_n, zn), "the nearest label map differs from zoom(order=0)"
            print(f"{shape} host route scipy.ndimage.zoom, one run each: image order 1 {host_img:.1f} ms (max difference {err:.2e}, bound {bound:.2e}); "
                  f"{len(classes)} indicators order 1 {host_lab:.1f} ms (equal away from 0.5); labels order 0 {host_near:.1f} ms "
                  f"({'not compared: a coordinate is an exact tie' if any(ties) else 'equal'})")
        line(f"{shape} resample_image float32 linear", timed(lambda: RS.resample_image(vol, grid, out=outf), a.reps, a.inner), 4 * (n_in + n_out))
        line(f"{shape} resample_image float32 nearest", timed(lambda: RS.resample_image(vol, grid, order=0, out=outf), a.reps, a.inner), 4 * (n_in + n_out))
        line(f"{shape} resample_image int16 linear", timed(lambda: RS.resample_image(vol16, grid, out=out16), a.reps, a.inner), 2 * (n_in + n_out))
        line(f"{shape} resample_image float32 linear center", timed(lambda: RS.resample_image(vol, grid, align="center", out=outf), a.reps, a.inner),
             4 * (n_in + n_out))
        line(f"{shape} resample_labels nearest, no statistics", timed(lambda: RS.resample_labels(mask, grid, out=out8), a.reps, a.inner), n_in + n_out)
        line(f"{shape} resample_labels linear, {len(classes)} classes with statistics",
             timed(lambda: RS.resample_labels(mask, grid, classes, mode="linear", out=out8, stats=stats), a.reps, a.inner),
             len(classes) * (2 * n_in + n_out) + (len(classes) - 1) * n_out)
        line(f"{shape} resample_labels linear, 1 class with statistics",
             timed(lambda: RS.resample_labels(mask, grid, (1,), mode="linear", out=out8, stats=stats[:1]), a.reps, a.inner), 2 * n_in + n_out)


if __name__ == "__main__":
    main()
