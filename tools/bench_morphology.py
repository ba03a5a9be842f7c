#!/usr/bin/env python3
"""Time of the four ball-morphology calls of rpnet_amd.morphology (erode, dilate, opening, closing) beside one surface tally of the same
volume in the same process, beside the host route through scipy.ndimage, and beside the evaluation of the volume itself.

    python tools/bench_morphology.py [--slices 64] [--size 256] [--reps 20] [--host-reps 3] [--out profiles/morphology_eval.txt]
        one call on a uint8 volume, device-synchronised wall time, median / min / max of --reps:
          final mask      the mask of a real VolumeSegmenter run on a synthetic volume
          noise 0.31      seeds everywhere: every scan ends at its first step
          full volume     no complement: the erosions scan to the cap
        the voxel ball at rho = 1, 9, 49 (49: the radius 7 of the reference's preprocessing), the millimetre ball at spacing
        (2.5, 0.8, 0.8) with r = 2 and 5 mm, in 3D and per slice;
        the yardstick: one surface tally (integer and millimetre) of two such volumes, which runs the same three passes uncapped on
        two volumes; the ratio is printed with the figures it comes from;
        the host route: mask.cpu() + scipy.ndimage.binary_closing / binary_opening with the same ball + upload (median of --host-reps),
        asserted equal to the device with erode_border=0 (scipy's border_value) before it is timed;
        the volume's evaluation call, VolumeSegmenter batch 8 graphed, with the chain off, with closing alone and with opening + closing.
    The lines it prints are the ones kept in profiles/morphology_eval.txt.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tools.bench_postprocess import host_timed
from tools.bench_surface import DEV, build_net, row, timed

MM = (2.5, 0.8, 0.8)
BALLS = ((("rho", 1), None), (("rho", 9), None), (("rho", 49), None), ((2.0, "mm"), MM), ((5.0, "mm"), MM))


def structure_of(radius, spacing, shape, per_slice):
    """the ball as a scipy structure, by the rule of rpnet_amd.morphology (restated here offset by offset)"""
    if radius[0] == "rho":
        w, lim = (np.float64(1.0),) * 3, np.float64(radius[1])
    else:
        w, lim = tuple(np.float64(s) * np.float64(s) for s in spacing), np.float64(radius[0]) * np.float64(radius[0])
    reach = []
    for a in range(3):
        o = 0
        while o < shape[a] and w[a] * np.float64((o + 1) * (o + 1)) <= lim:
            o += 1
        reach.append(0 if per_slice and a == 0 else o)
    dz, dy, dx = np.meshgrid(*(np.arange(-r, r + 1) for r in reach), indexing="ij")
    return (w[2] * (dx * dx).astype(np.float64) + w[1] * (dy * dy).astype(np.float64)) + w[0] * (dz * dz).astype(np.float64) <= lim


def host_route(mask_dev, op, structure):
    from scipy import ndimage as ndi
    m = mask_dev.cpu().numpy()
    res = (ndi.binary_closing if op == "closing" else ndi.binary_opening)(m == 1, structure=structure)
    return torch.from_numpy(np.where(res & (m == 0), 1, np.where((m == 1) & ~res, 0, m)).astype(np.uint8)).to(mask_dev.device)


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
        raise SystemExit("bench_morphology.py measures on the MI355X: no GPU found")
    from dataset.few_shot_reader import FewshotRegReader
    from rpnet_amd import morphology as MO
    from rpnet_amd import surface as SF
    from rpnet_amd import surface_spacing as SS
    from rpnet_amd.volume import VolumeSegmenter
    from utils.util import load_yaml
    cfg, _ = load_yaml(a.yaml)
    cfg["n_iter_refinement"] = cfg["n_test_iter_refinement"]
    item = FewshotRegReader(None, cfg["eval_set_name"], cfg, mode="eval", n_volumes=1, n_slices=a.slices, size=a.size)[0]
    net = build_net(cfg)
    args = (item["support_images"], item["support_labels"], item["query_images"], item["appr_query_labels"], item["query_labels"])
    segs = {"chain off": VolumeSegmenter(net, batch=8, graphed=True), "closing alone (radius 7)": VolumeSegmenter(net, batch=8, graphed=True, closing=7),
            "opening + closing (radius 7)": VolumeSegmenter(net, batch=8, graphed=True, opening=7, closing=7)}
    mask = segs["chain off"](*args).mask.contiguous()
    D, H, W = mask.shape
    gen = torch.Generator(device=DEV).manual_seed(1)
    volumes = (("final mask", mask), ("noise 0.31", (torch.rand((D, H, W), device=DEV, generator=gen) < 0.31).to(torch.uint8)),
               ("full volume", torch.ones((D, H, W), device=DEV, dtype=torch.uint8)))
    dst = torch.empty_like(mask)
    stats = torch.zeros((1, MO.STATS_ROW), device=DEV, dtype=torch.int64)
    fns = (("erode", MO.erode), ("dilate", MO.dilate), ("opening", MO.opening), ("closing", MO.closing))
    out = [f"ball morphology on a {D} x {H} x {W} uint8 volume ({D * H * W} voxels), ms, device-synchronised wall time, {a.reps} runs after 3 "
           f"warm-up runs: median (min .. max)"]
    labels = item["query_labels"].to(DEV).to(torch.int32).contiguous()
    it, ft = torch.zeros((1, SF.IROW), device=DEV, dtype=torch.int64), torch.zeros((1, SF.FROW), device=DEV, dtype=torch.float64)
    im, fm = torch.zeros((1, SS.IROW), device=DEV, dtype=torch.int64), torch.zeros((1, SS.FROW), device=DEV, dtype=torch.float64)
    tally = timed(lambda: SF.surface_tally(mask, labels, it, 0, ft, 0), a.reps)
    tally_mm = timed(lambda: SS.surface_tally_spacing(mask, labels, MM, im, 0, fm, 0), a.reps)
    out.append(row("yardstick: one surface tally of the final mask against the labels (two volumes), voxels", tally))
    out.append(row("yardstick: the same tally under spacing (2.5, 0.8, 0.8)", tally_mm))
    for name, vol in volumes:
        for radius, spacing in BALLS:
            for per_slice in (False, True):
                for fname, fn in fns:
                    t = timed(lambda: fn(vol, (1,), radius, spacing=spacing, per_slice=per_slice, out=dst, stats=stats), a.reps)
                    base = tally_mm if spacing else tally
                    out.append(row(f"{fname}: {name}, {radius}{', per slice' if per_slice else ''}", t)
                               + f"   {t[0] / base[0]:.2f} of the tally's {base[0]:.3f} ms; statistics row {stats[0].tolist()}")
    try:
        from scipy import ndimage  # noqa: F401
    except ImportError:
        out.append("  host route: scipy is not installed here, not measured")
    else:
        for name, vol in volumes:
            for radius, spacing in BALLS:
                st = structure_of(radius, spacing, (D, H, W), False)
                for fname, fn in fns[2:]:
                    fn(vol, (1,), radius, spacing=spacing, erode_border=0, out=dst, stats=stats)
                    same = torch.equal(host_route(vol, fname, st), dst)
                    assert same, f"host and device differ: {fname} {name} {radius}"
                    _, t = host_timed(lambda: host_route(vol, fname, st), a.host_reps)
                    out.append(row(f"host route (binary_{fname}): {name}, {radius}", t) + f"   same mask as the device: {same}")
    times = {name: timed(lambda: seg(*args), a.reps) for name, seg in segs.items()}
    for name, t in times.items():
        out.append(row(f"volume, VolumeSegmenter batch 8 graphed, {name}", t))
    off = times["chain off"]
    for name in list(times)[1:]:
        out.append(f"  {name} adds {times[name][0] - off[0]:.3f} ms to the volume's {off[0]:.3f} ms; the spread of that call is "
                   f"{off[1]:.3f} .. {off[2]:.3f} ms")
    text = "\n".join(out)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
