#!/usr/bin/env python3
"""Time the per-component statistics on the device against the host route, and write profiles/component_stats.txt.

    python tools/bench_component_stats.py [--out profiles/component_stats.txt] [--reps 20]

Volumes: 64 x 256 x 256 uint8 masks made from a seed: a smooth phantom (one object, the stand-in for a real final mask), a full volume
(one id in every chunk) and independent noise at density 0.31 under both connectivities (tens of thousands of components, more ids per
chunk than the pass has slots).  Per volume, the median of `reps` calls with min and max, every call timed by device events after a
warm-up of 3, all in one process: `rank_components` alone, `tally_components` alone with and without a float32 image, the whole
`component_table` chain; beside them one `rpnet_cc_label` call and one `rpnet_region_stats` call on the same mask as yardsticks.  The host
route on the same box: `.cpu()` + scipy.ndimage.label + sum / find_objects / center_of_mass, timed by the host clock after its results
have been asserted equal to the device's.  Last, `VolumeSegmenter` at batch 8 graphed on a synthetic item with and without
components=True, each against its own spread.  One JSON line per measurement."""
import argparse
import json
import os
import random
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from rpnet_amd import component_stats as CS
from rpnet_amd import regions as R
from rpnet_amd.components import label_components

SHAPE = (64, 256, 256)
MAX_COMPONENTS = 65536


def volumes(seed=7):
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[np.linspace(-1, 1, s) for s in SHAPE], indexing="ij")
    phantom = ((z * z + y * y + x * x) < 0.45).astype(np.uint8)
    noise = (rng.random(SHAPE) < 0.31).astype(np.uint8)
    image = (rng.standard_normal(SHAPE) * 300.0 + 40.0).astype(np.float32)
    return [("phantom mask", phantom, 6), ("full volume", np.ones(SHAPE, np.uint8), 6), ("noise 0.31", noise, 6), ("noise 0.31", noise, 26)], image


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


def host_route(d_mask, connectivity):
    """what a user does today: the mask to the host, scipy.ndimage.label and three more calls over its components"""
    from scipy import ndimage
    mask = d_mask.cpu().numpy()
    t0 = time.perf_counter()
    lab, n = ndimage.label(mask, structure=ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3))
    t_label = (time.perf_counter() - t0) * 1e3
    index = np.arange(1, n + 1)
    ones = np.ones(SHAPE)
    return {"lab": lab, "n": n, "sizes": ndimage.sum(ones, lab, index), "boxes": ndimage.find_objects(lab),
            "com": ndimage.center_of_mass(ones, lab, index), "label_ms": t_label}


def segmenter_lines(reps):
    from rpnet_amd import dataset_eval as DE
    from rpnet_amd.utils import volume_reader as VR
    from rpnet_amd.volume import VolumeSegmenter
    from tests.test_gpu_dataset_eval import CASE, _build_net, _eval_cfg, config_for
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        data_dir, set_name, csv_dir = VR.write_synthetic_dataset(tmp, **CASE["data"])
        cfg = _eval_cfg(dict(config_for(CASE, csv_dir), use_registration_mask=False, do_deformable=False))
        src = DE.DeviceEvalSource(data_dir, set_name, cfg, "cuda:0")
        src.warm()
        net = _build_net(cfg, "f32")
        random.seed(3)
        item = src.item(0)
        args = (item["support_images"], item["support_labels"], item["query_images"], item["appr_query_labels"], item["query_labels"])
        for name, kw in (("VolumeSegmenter batch 8 graphed", {}), ("VolumeSegmenter batch 8 graphed, components=True", dict(components=True))):
            seg = VolumeSegmenter(net, batch=8, graphed=True, **kw)
            lines.append(dict(metric=name, volume=f"synthetic item {tuple(item['query_images'].shape)}", **device_times(lambda: seg(*args), reps)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "component_stats.txt"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_component_stats needs the MI355X: there is nothing to time without it")
    dev = "cuda:0"
    n = SHAPE[0] * SHAPE[1] * SHAPE[2]
    cases, image = volumes()
    d_image = torch.from_numpy(image).to(dev)
    rows = torch.zeros((1, MAX_COMPONENTS, CS.COMP_ROW), dtype=torch.int64, device=dev)
    labels, dense = (torch.zeros(SHAPE, dtype=torch.int32, device=dev) for _ in range(2))
    head = torch.zeros((CS.HEAD_WORDS,), dtype=torch.int64, device=dev)
    lines = []
    for name, mask, connectivity in cases:
        volume = f"{name}, connectivity {connectivity}, 64x256x256 uint8"
        d_mask = torch.from_numpy(mask).to(dev)
        chain = dict(cls=1, connectivity=connectivity, max_components=MAX_COMPONENTS, out=rows, head_out=head, labels=labels, dense=dense)
        CS.component_table(d_mask, image=d_image, other=d_mask, **chain)
        got_head, got_rows, got_dense = head.cpu().numpy(), rows[0].cpu().numpy(), dense.cpu().numpy()
        host = host_route(d_mask, connectivity)
        C = int(got_head[0])
        assert C == host["n"] and list(got_head[1:]) == [0, int((host["lab"] > MAX_COMPONENTS).sum()), 0] and np.array_equal(got_dense, host["lab"])
        M = min(C, MAX_COMPONENTS)
        assert np.array_equal(got_rows[:M, 0], host["sizes"][:M].astype(np.int64))
        for k in range(0, M, max(1, M // 500)):
            box = host["boxes"][k]
            assert [s.start for s in box] == list(got_rows[k, 1:4]) and [s.stop - 1 for s in box] == list(got_rows[k, 4:7])
            assert np.allclose(got_rows[k, 7:10] / got_rows[k, 0], host["com"][k], rtol=1e-12, atol=0)
        common = dict(volume=volume, voxels=n, components=C)
        lines.append(dict(metric="yardstick: one rpnet_cc_label call", **common,
                          **device_times(lambda: label_components(d_mask, cls=1, connectivity=connectivity, labels=labels), a.reps)))
        lines.append(dict(metric="rank_components (memset + 5 launches)", **common, **device_times(lambda: CS.rank_components(labels, out=dense), a.reps)))
        lines.append(dict(metric="tally_components, no image (2 memsets + 2 launches)", **common,
                          **device_times(lambda: CS.tally_components(dense, None, d_mask, 1, MAX_COMPONENTS, out=rows), a.reps)))
        lines.append(dict(metric="tally_components, float32 image (2 memsets + 2 launches)", **common,
                          **device_times(lambda: CS.tally_components(dense, d_image, d_mask, 1, MAX_COMPONENTS, out=rows), a.reps)))
        lines.append(dict(metric="component_table: label + rank + tally, float32 image", **common,
                          **device_times(lambda: CS.component_table(d_mask, image=d_image, other=d_mask, **chain), a.reps)))
        ri = torch.zeros((1, 2, R.IROW), dtype=torch.int64, device=dev)
        rf = torch.zeros((1, 2, R.FROW), dtype=torch.float64, device=dev)
        lines.append(dict(metric="yardstick: one rpnet_region_stats call on the mask, L=2, float32 image", **common,
                          **device_times(lambda: R.region_stats(d_mask, d_image, n_labels=2, out=(ri, rf)), a.reps)))
        hs, ls = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            ls.append(host_route(d_mask, connectivity)["label_ms"])
            hs.append((time.perf_counter() - t0) * 1e3)
        lines.append(dict(metric="host route: .cpu() + scipy.ndimage label, sum, find_objects, center_of_mass", **common, median_ms=float(np.median(hs)),
                          min_ms=min(hs), max_ms=max(hs), label_alone_median_ms=float(np.median(ls)), reps=3))
    lines += segmenter_lines(a.reps)
    lines.append({"not measured": ["real final masks (the repository carries no trained checkpoint: a phantom stands in)",
                                   "LDS or atomic counters of the pass", "int16 images and other kinds of the second volume"]})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for row in lines:
            fh.write(json.dumps(row) + "\n")
            print(json.dumps(row))


if __name__ == "__main__":
    main()
