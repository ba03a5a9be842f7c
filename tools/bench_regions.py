#!/usr/bin/env python3
"""Time the region statistics on the device against the host route, and write profiles/regions.txt.

    python tools/bench_regions.py [--out profiles/regions.txt] [--reps 20]

Volumes: 64 x 256 x 256 uint8 labels with a float32 image, made from a seed: a smooth phantom (one object, the stand-in for a real final
mask, which needs a trained checkpoint the repository does not carry: wave-uniform almost everywhere), independent noise over 256 labels
(one tree per present label per chunk: the worst case), and a volume that is one label throughout.
Per volume one `region_stats` call (memset + 2 launches), the median of `reps` calls with min and max, every call timed by device events
after a warm-up of 3, all in one process.  Beside it one `rpnet_seg_tally` launch on a [64, 2, 256, 256] float32 source, the project's
yardstick for a single-pass tally.  The host route on the same box: `.cpu()` of labels and image plus scipy.ndimage sum_labels (count,
S1, S2), center_of_mass, find_objects, minimum, maximum and standard_deviation, timed by the host clock after its results have been
asserted equal to (counts, boxes, extrema) or within the summation bound of (sums) the device's.  One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from rpnet_amd import regions as R
from rpnet_amd.volume import seg_tally

SHAPE = (64, 256, 256)


def volumes(seed=7):
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[np.linspace(-1, 1, s) for s in SHAPE], indexing="ij")
    phantom = ((z * z + y * y + x * x) < 0.45).astype(np.uint8)
    noise = rng.integers(0, 256, size=SHAPE, dtype=np.uint8)
    image = (rng.standard_normal(SHAPE) * 300.0 + 40.0).astype(np.float32)
    return {"phantom mask, L=2": (phantom, 2), "noise over 256 labels, L=256": (noise, 256), "one label throughout, L=2": (np.ones(SHAPE, np.uint8), 2)}, image


def device_times(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "reps": reps}


def host_route(d_labels, d_image, L):
    """what a user does today: the volumes to the host, six scipy.ndimage calls over the foreground labels"""
    from scipy import ndimage
    labels, image = d_labels.cpu().numpy().astype(np.int32), d_image.cpu().numpy().astype(np.float64)
    index = np.arange(1, L)
    return {"n": ndimage.sum_labels(np.ones(SHAPE), labels, index), "s1": ndimage.sum_labels(image, labels, index),
            "com": ndimage.center_of_mass(np.ones(SHAPE), labels, index), "boxes": ndimage.find_objects(labels, max_label=L - 1),
            "min": ndimage.minimum(image, labels, index), "max": ndimage.maximum(image, labels, index),
            "std": ndimage.standard_deviation(image, labels, index), "abs": ndimage.sum_labels(np.abs(image), labels, index)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "regions.txt"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_regions needs the MI355X: there is nothing to time without it")
    dev = "cuda:0"
    n = SHAPE[0] * SHAPE[1] * SHAPE[2]
    cases, image = volumes()
    d_image = torch.from_numpy(image).to(dev)
    lines = []
    for name, (labels, L) in cases.items():
        d_labels = torch.from_numpy(labels).to(dev)
        ri = torch.zeros((1, L, R.IROW), dtype=torch.int64, device=dev)
        rf = torch.zeros((1, L, R.FROW), dtype=torch.float64, device=dev)
        t = device_times(lambda: R.region_stats(d_labels, d_image, n_labels=L, out=(ri, rf)), a.reps)
        lines.append(dict(metric="region_stats (memset + 2 launches)", volume=f"{name}, 64x256x256 uint8 + float32 image", voxels=n,
                          bytes_moved=5 * n, gbytes_per_s=5 * n / t["median_ms"] / 1e6, **t))
        # the host route, its results checked against the device's first
        host = host_route(d_labels, d_image, L)
        rows_i, rows_f = ri[0].cpu().numpy(), rf[0].cpu().numpy()
        figs = R.derive(rows_i, rows_f)
        for l in range(1, L):
            assert rows_i[l, 0] == int(host["n"][l - 1])
            if rows_i[l, 0]:
                box = host["boxes"][l - 1]
                assert [s.start for s in box] == list(rows_i[l, 1:4]) and [s.stop - 1 for s in box] == list(rows_i[l, 4:7])
                assert figs[l]["min"] == host["min"][l - 1] and figs[l]["max"] == host["max"][l - 1]
                assert abs(rows_f[l, 0] - host["s1"][l - 1]) <= rows_i[l, 0] * 2.0 ** -52 * host["abs"][l - 1]
                assert np.allclose(figs[l]["centroid"], host["com"][l - 1], rtol=1e-12, atol=0)
        hs = []
        for _ in range(3):
            t0 = time.perf_counter()
            host_route(d_labels, d_image, L)
            hs.append((time.perf_counter() - t0) * 1e3)
        lines.append(dict(metric="host route: .cpu() + scipy.ndimage sum_labels x3, center_of_mass, find_objects, minimum, maximum, "
                                 "standard_deviation", volume=name, median_ms=float(np.median(hs)), min_ms=min(hs), max_ms=max(hs), reps=3))
    # the yardstick: one rpnet_seg_tally launch
    N, K, H, W = SHAPE[0], 2, SHAPE[1], SHAPE[2]
    logits = torch.randn((N, K, H, W), device=dev, dtype=torch.float32)
    truth = torch.from_numpy(cases["phantom mask, L=2"][0]).to(dev).to(torch.int32)
    counts = torch.zeros((1, K - 1, 3), device=dev, dtype=torch.int64)
    mask = torch.empty((N, H, W), device=dev, dtype=torch.uint8)
    nv = torch.full((1,), N, device=dev, dtype=torch.int32)
    t = device_times(lambda: seg_tally([logits], [0], nv, truth, counts, mask, mask_src=0, K=K), a.reps)
    moved = logits.numel() * 4 + truth.numel() * 4 + mask.numel()
    lines.append(dict(metric="yardstick: one rpnet_seg_tally launch, one [64, 2, 256, 256] float32 source", bytes_moved=moved,
                      gbytes_per_s=moved / t["median_ms"] / 1e6, **t))
    lines.append({"not measured": ["real final masks (the repository carries no trained checkpoint: a phantom stands in)",
                                   "VolumeSegmenter at batch 8 graphed with and without regions=True",
                                   "LDS or atomic counters of the pass", "other label and image kinds than uint8 + float32"]})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for row in lines:
            fh.write(json.dumps(row) + "\n")
            print(json.dumps(row))


if __name__ == "__main__":
    main()
