#!/usr/bin/env python3
"""Time of the surface-distance tally under a voxel spacing (rpnet_amd.surface_spacing.surface_tally_spacing: fp64 transform, radix
selection) beside the integer tally (rpnet_amd.surface.surface_tally) on the same volumes in the same process.

    python tools/bench_surface_spacing.py [--slices 64] [--size 256] [--reps 20] [--out FILE]
        one tally, device-synchronised wall time, median / min / max of --reps, for each of
          box against shifted box, final mask against labels (a real VolumeSegmenter run on a synthetic volume), empty prediction:
          the integer tally, the spacing tally at (1, 1, 1) and at (2.5, 0.8, 0.8) with a tolerance of 2 mm;
        the volume's evaluation call, VolumeSegmenter batch 8 graphed, with surface=True and with surface=True, spacing=(2.5, 0.8, 0.8).
    The lines it prints are the ones kept in profiles/surface_spacing.txt.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.bench_surface import DEV, build_net, row, timed

MM = (2.5, 0.8, 0.8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--yaml", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "yamls", "example.yml"))
    ap.add_argument("--slices", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_surface_spacing.py measures on the MI355X: no GPU found")
    from dataset.few_shot_reader import FewshotRegReader
    from rpnet_amd import surface as SF
    from rpnet_amd import surface_spacing as SS
    from rpnet_amd.volume import VolumeSegmenter
    from utils.util import load_yaml
    cfg, _ = load_yaml(a.yaml)
    cfg["n_iter_refinement"] = cfg["n_test_iter_refinement"]
    item = FewshotRegReader(None, cfg["eval_set_name"], cfg, mode="eval", n_volumes=1, n_slices=a.slices, size=a.size)[0]
    net = build_net(cfg)
    args = (item["support_images"], item["support_labels"], item["query_images"], item["appr_query_labels"], item["query_labels"])
    seg_i = VolumeSegmenter(net, batch=8, graphed=True, surface=True)
    seg_mm = VolumeSegmenter(net, batch=8, graphed=True, surface=True, spacing=MM, surface_tolerance=2.0)
    res = seg_i(*args)
    labels = item["query_labels"].to(DEV, torch.int32).contiguous()
    D, H, W = labels.shape
    box = torch.zeros((D, H, W), device=DEV, dtype=torch.uint8)
    box[D // 4:3 * D // 4, H // 4:3 * H // 4, W // 4:3 * W // 4] = 1
    moved = torch.roll(box, (2, 5, 3), (0, 1, 2))
    empty = torch.zeros_like(box)
    it = torch.zeros((1, SF.IROW), device=DEV, dtype=torch.int64)
    ft = torch.zeros((1, SF.FROW), device=DEV, dtype=torch.float64)
    its = torch.zeros((1, SS.IROW), device=DEV, dtype=torch.int64)
    fts = torch.zeros((1, SS.FROW), device=DEV, dtype=torch.float64)

    out = [f"surface tallies of a {D} x {H} x {W} volume, integer path beside the spacing path, ms, device-synchronised wall time, "
           f"{a.reps} runs after 3 warm-up runs"]
    for name, p, t in (("box against shifted box", moved, box), ("final mask against labels", res.mask.contiguous(), labels),
                       ("empty prediction against box", empty, box)):
        out.append(row("integer tally: " + name, timed(lambda: SF.surface_tally(p, t, it, 0, ft, 0), a.reps)))
        out.append(row("spacing (1, 1, 1): " + name, timed(lambda: SS.surface_tally_spacing(p, t, (1, 1, 1), its, 0, fts, 0), a.reps)))
        out.append(row(f"spacing {MM}, tau 2: " + name, timed(lambda: SS.surface_tally_spacing(p, t, MM, its, 0, fts, 0, tau=2.0), a.reps)))
        out.append(f"    figures in mm: {SS.figures_from_rows(its[0].cpu().numpy(), fts[0].cpu().numpy(), 2.0)}")
    t_i, t_mm = timed(lambda: seg_i(*args), a.reps), timed(lambda: seg_mm(*args), a.reps)
    out.append(row("volume, VolumeSegmenter batch 8 graphed, surface", t_i))
    out.append(row(f"volume, the same with spacing={MM}", t_mm))
    out.append(f"  the spacing adds {t_mm[0] - t_i[0]:.3f} ms to the {t_i[0]:.3f} ms of the volume call with the integer tallies")
    text = "\n".join(out)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
