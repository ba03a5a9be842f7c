#!/usr/bin/env python3
"""Time of the surface-distance tally (rpnet_amd.surface.surface_tally: HD95 / HD / ASSD rows of one prediction against one truth)
beside the host route through scipy.ndimage and beside the evaluation of the volume itself.

    python tools/bench_surface.py [--slices 64] [--size 256] [--reps 20] [--host-reps 3] [--out FILE]
        one tally, device-synchronised wall time, median / min / max of --reps:
          box against shifted box     a box-shaped organ and the same box moved by (2, 5, 3) voxels
          final mask against labels   the mask of a real VolumeSegmenter run on a synthetic volume against its labels
          affine baseline             that volume's appr_query_labels against its labels
          empty prediction            the worst case of the outward scans: no seed anywhere in one volume
        the host route for the same volume: M & ~binary_erosion(M) and distance_transform_edt of the truth, the final mask and the
        affine baseline, then percentile / mean (median of --host-reps; scipy is looked for and its absence reported);
        the volume's evaluation call, VolumeSegmenter batch 8 graphed, with surface=False and with surface=True.
    The lines it prints are the ones kept in profiles/surface_eval.txt.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

DEV = "cuda:0"


def build_net(cfg):
    from rpnet_amd.modules import RP_Net
    from rpnet_amd.utils.seeding import seed_module_
    net = RP_Net(cfg={"align": True, "backbone": "UNet"}, backbone_cfg=cfg).to(DEV)
    seed_module_(net)
    return net.eval()


def timed(fn, reps, warmup=3):
    """device-synchronised wall time of fn() in ms: (median, min, max)"""
    ts = []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def row(name, t):
    return f"  {name:44s} median {t[0]:9.3f}   min {t[1]:9.3f}   max {t[2]:9.3f}"


def host_route(truth, preds):
    """what a user runs today on the masks written by --save-pred"""
    from scipy import ndimage as ndi
    st = ndi.generate_binary_structure(3, 1)

    def border_and_edt(m):
        b = m & ~ndi.binary_erosion(m, st)
        return b, ndi.distance_transform_edt(~b)
    bt, et = border_and_edt(truth)
    out = []
    for p in preds:
        bp, ep = border_and_edt(p)
        if not bp.any() or not bt.any():
            out.append(None)
            continue
        d = np.hstack([et[bp], ep[bt]])
        out.append((float(np.percentile(d, 95)), float((et[bp].mean() + ep[bt].mean()) / 2)))
    return out


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
        raise SystemExit("bench_surface.py measures on the MI355X: no GPU found")
    from dataset.few_shot_reader import FewshotRegReader
    from rpnet_amd import surface as SF
    from rpnet_amd.volume import VolumeSegmenter
    from utils.util import load_yaml
    cfg, _ = load_yaml(a.yaml)
    cfg["n_iter_refinement"] = cfg["n_test_iter_refinement"]
    item = FewshotRegReader(None, cfg["eval_set_name"], cfg, mode="eval", n_volumes=1, n_slices=a.slices, size=a.size)[0]
    net = build_net(cfg)
    args = (item["support_images"], item["support_labels"], item["query_images"], item["appr_query_labels"], item["query_labels"])
    seg, seg_s = VolumeSegmenter(net, batch=8, graphed=True), VolumeSegmenter(net, batch=8, graphed=True, surface=True)
    res = seg_s(*args)
    labels = item["query_labels"].to(DEV, torch.int32).contiguous()
    appr = item["appr_query_labels"].to(DEV, torch.float32).contiguous()
    D, H, W = labels.shape
    box = torch.zeros((D, H, W), device=DEV, dtype=torch.uint8)
    box[D // 4:3 * D // 4, H // 4:3 * H // 4, W // 4:3 * W // 4] = 1
    moved = torch.roll(box, (2, 5, 3), (0, 1, 2))
    empty = torch.zeros_like(box)
    it = torch.zeros((1, SF.IROW), device=DEV, dtype=torch.int64)
    ft = torch.zeros((1, SF.FROW), device=DEV, dtype=torch.float64)

    out = [f"surface tally of a {D} x {H} x {W} volume (nbins {(D - 1) ** 2 + (H - 1) ** 2 + (W - 1) ** 2 + 1}), ms, device-synchronised wall "
           f"time, {a.reps} runs after 3 warm-up runs"]
    figures = {}
    for name, p, t in (("box against shifted box", moved, box), ("final mask against labels", res.mask.contiguous(), labels),
                       ("affine baseline against labels", appr, labels), ("empty prediction against box", empty, box)):
        out.append(row("tally: " + name, timed(lambda: SF.surface_tally(p, t, it, 0, ft, 0), a.reps)))
        figures[name] = SF.surface_from_rows(it[0].cpu().numpy(), ft[0].cpu().numpy())
    out += [f"  figures, {name}: {fig}" for name, fig in figures.items()]
    t_plain, t_surf = timed(lambda: seg(*args), a.reps), timed(lambda: seg_s(*args), a.reps)
    out.append(row("volume, VolumeSegmenter batch 8 graphed", t_plain))
    out.append(row("volume, the same with surface=True", t_surf))
    out.append(f"  the two tallies of a volume add {t_surf[0] - t_plain[0]:.3f} ms to its {t_plain[0]:.3f} ms "
               f"({'MORE' if t_surf[0] - t_plain[0] > t_plain[0] else 'less'} than the evaluation call itself)")
    try:
        import scipy  # noqa: F401
    except ImportError:
        out.append("  host route: scipy is not installed here, not measured")
    else:
        truth, preds = labels.cpu().numpy() == 1, [res.mask.cpu().numpy() == 1, appr.cpu().numpy() == 1]
        ts = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            host = host_route(truth, preds)
            ts.append((time.perf_counter() - t0) * 1e3)
        out.append(row("host route, scipy.ndimage, 3 borders + EDTs", (statistics.median(ts), min(ts), max(ts))))
        out.append(f"  host (hd95, assd) of final mask, affine: {host}; device: {res.surface}")
        out.append(f"  host route / device tallies: {statistics.median(ts) / max(t_surf[0] - t_plain[0], 1e-9):.0f} x")
    text = "\n".join(out)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
