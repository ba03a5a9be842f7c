#!/usr/bin/env python3
"""Time of the two clean-up calls of rpnet_amd.postprocess (one rpnet_ccpost_fill_holes, one rpnet_ccpost_remove_small) beside
rpnet_cc_keep_largest on the same volume in the same process, beside the host routes through scipy.ndimage, and beside the evaluation
of the volume itself.

    python tools/bench_postprocess.py [--slices 64] [--size 256] [--reps 20] [--host-reps 3] [--out profiles/postprocess_eval.txt]
        one call on a uint8 volume, device-synchronised wall time, median / min / max of --reps:
          final mask      the mask of a real VolumeSegmenter run on a synthetic volume
          noise 0.31      the worst case for merges
          full volume     one component that spans every tile (for fill_holes: an empty complement)
        fill_holes in 3D (background connectivity 6 and 26) and per slice (4 and 8), remove_small at connectivity 6 and 26 with
        min_voxels 64, keep_largest at connectivity 6 and 26;
        the host routes they replace: mask.cpu() + binary_fill_holes + upload, mask.cpu() + label + bincount + filter + upload (median of
        --host-reps), with a check that host and device give the same mask;
        the volume's evaluation call, VolumeSegmenter batch 8 graphed, with the chain off and on.
    The question the figures answer: fill_holes labels the complement, which is most of a real volume, so its cost is expected near the
    full-volume row of keep_largest rather than near the final-mask row.  The lines it prints are the ones kept in
    profiles/postprocess_eval.txt.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tools.bench_surface import DEV, build_net, row, timed

MIN_VOXELS = 64


def host_fill(mask_dev, structure, per_slice):
    from scipy import ndimage as ndi
    m = mask_dev.cpu().numpy()
    obj = m == 1
    filled = (np.stack([ndi.binary_fill_holes(obj[z], structure=structure) for z in range(obj.shape[0])]) if per_slice
              else ndi.binary_fill_holes(obj, structure=structure))
    return torch.from_numpy(np.where(filled & (m == 0), 1, m).astype(np.uint8)).to(mask_dev.device)


def host_small(mask_dev, structure, min_voxels):
    from scipy import ndimage as ndi
    m = mask_dev.cpu().numpy()
    lab, n = ndi.label(m == 1, structure=structure)
    small = np.bincount(lab.ravel(), minlength=n + 1) < min_voxels
    small[0] = False
    return torch.from_numpy(np.where(small[lab], 0, m).astype(np.uint8)).to(mask_dev.device)


def host_timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return res, (statistics.median(ts), min(ts), max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--yaml", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "yamls", "example.yml"))
    ap.add_argument("--slices", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_postprocess.py measures on the MI355X: no GPU found")
    from dataset.few_shot_reader import FewshotRegReader
    from rpnet_amd import components as CC
    from rpnet_amd import postprocess as PP
    from rpnet_amd.volume import VolumeSegmenter
    from utils.util import load_yaml
    cfg, _ = load_yaml(a.yaml)
    cfg["n_iter_refinement"] = cfg["n_test_iter_refinement"]
    item = FewshotRegReader(None, cfg["eval_set_name"], cfg, mode="eval", n_volumes=1, n_slices=a.slices, size=a.size)[0]
    net = build_net(cfg)
    args = (item["support_images"], item["support_labels"], item["query_images"], item["appr_query_labels"], item["query_labels"])
    chain = dict(keep_largest=6, fill_holes=True, min_component=MIN_VOXELS)
    segs = {"chain off": VolumeSegmenter(net, batch=8, graphed=True), "keep_largest alone": VolumeSegmenter(net, batch=8, graphed=True, keep_largest=6),
            "chain on (remove small, keep largest, fill holes)": VolumeSegmenter(net, batch=8, graphed=True, **chain)}
    mask = segs["chain off"](*args).mask.contiguous()
    D, H, W = mask.shape
    n = D * H * W
    gen = torch.Generator(device=DEV).manual_seed(1)
    volumes = (("final mask", mask), ("noise 0.31", (torch.rand((D, H, W), device=DEV, generator=gen) < 0.31).to(torch.uint8)),
               ("full volume", torch.ones((D, H, W), device=DEV, dtype=torch.uint8)))
    dst = torch.empty_like(mask)
    stats = torch.zeros((1, PP.STATS_ROW), device=DEV, dtype=torch.int64)
    out = [f"clean-up calls on a {D} x {H} x {W} uint8 volume ({n} voxels), ms, device-synchronised wall time, {a.reps} runs after 3 warm-up "
           f"runs: median (min .. max)"]
    for name, vol in volumes:
        for conn in (6, 26):
            out.append(row(f"keep_largest: {name}, connectivity {conn}", timed(lambda: CC.keep_largest(vol, connectivity=conn, out=dst, stats=stats),
                                                                                 a.reps)))
        for conn, per_slice in ((6, False), (26, False), (4, True), (8, True)):
            fn = lambda: PP.fill_holes(vol, (1,), connectivity=conn, per_slice=per_slice, out=dst, stats=stats)     # noqa: E731
            out.append(row(f"fill_holes: {name}, background connectivity {conn}{', per slice' if per_slice else ''}", timed(fn, a.reps)))
            out.append(f"    statistics row {stats[0].tolist()}, overrun word {PP.post_overrun(DEV, (D, H, W))}")
        for conn in (6, 26):
            fn = lambda: PP.remove_small(vol, (1,), MIN_VOXELS, connectivity=conn, out=dst, stats=stats)     # noqa: E731
            out.append(row(f"remove_small: {name}, connectivity {conn}, min_voxels {MIN_VOXELS}", timed(fn, a.reps)))
            out.append(f"    statistics row {stats[0].tolist()}, overrun word {PP.post_overrun(DEV, (D, H, W))}")
    try:
        from scipy import ndimage as ndi
    except ImportError:
        out.append("  host routes: scipy is not installed here, not measured")
    else:
        for name, vol in volumes:
            for conn, per_slice, rank in ((6, False, 1), (26, False, 3), (4, True, 1), (8, True, 2)):
                st = ndi.generate_binary_structure(2 if per_slice else 3, rank)
                host, t = host_timed(lambda: host_fill(vol, st, per_slice), a.host_reps)
                PP.fill_holes(vol, (1,), connectivity=conn, per_slice=per_slice, out=dst, stats=stats)
                out.append(row(f"host route (binary_fill_holes): {name}, {conn}{', per slice' if per_slice else ''}", t)
                           + f"   same mask as the device: {torch.equal(host, dst)}")
            for conn, rank in ((6, 1), (26, 3)):
                st = ndi.generate_binary_structure(3, rank)
                host, t = host_timed(lambda: host_small(vol, st, MIN_VOXELS), a.host_reps)
                PP.remove_small(vol, (1,), MIN_VOXELS, connectivity=conn, out=dst, stats=stats)
                out.append(row(f"host route (label + bincount): {name}, connectivity {conn}", t) + f"   same mask as the device: {torch.equal(host, dst)}")
    times = {name: timed(lambda: seg(*args), a.reps) for name, seg in segs.items()}
    for name, t in times.items():
        out.append(row(f"volume, VolumeSegmenter batch 8 graphed, {name}", t))
    off, on = times["chain off"], times["chain on (remove small, keep largest, fill holes)"]
    out.append(f"  the chain adds {on[0] - off[0]:.3f} ms to the volume's {off[0]:.3f} ms; the spread of that call is {off[1]:.3f} .. {off[2]:.3f} ms")
    text = "\n".join(out)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
