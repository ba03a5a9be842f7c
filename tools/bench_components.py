#!/usr/bin/env python3
"""Time of the largest-component filter (rpnet_amd.components.keep_largest: one rpnet_cc_keep_largest call) beside the host route
through scipy.ndimage.label and beside the evaluation of the volume itself.

    python tools/bench_components.py [--slices 64] [--size 256] [--reps 20] [--host-reps 3] [--out FILE]
        one call on a uint8 volume, device-synchronised wall time, median / min / max of --reps, connectivity 6 and 26:
          final mask      the mask of a real VolumeSegmenter run on a synthetic volume
          noise 0.31      the worst case for merges
          full volume     one component that spans every tile
        each phase's launch of those calls (kernel times from torch.profiler, mean over --reps) and the bytes a phase moves at the
        least, set against the 6.29 TB/s copy rate;
        the host route it replaces: mask.cpu() + scipy.ndimage.label + bincount + filter + upload (median of --host-reps);
        the volume's evaluation call, VolumeSegmenter batch 8 graphed, with and without keep_largest, with and without surface.
    The lines it prints are the ones kept in profiles/components_eval.txt.
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

COPY_RATE = 6.29e12         # bytes / s, the copy rate of the README
PHASES = ("cc_local_kernel", "cc_merge_kernel", "cc_flatten_kernel", "cc_choose_kernel", "cc_stats_kernel", "cc_filter_kernel")


def phase_times(fn, reps):
    """{kernel name: mean time in us over reps} of the component kernels inside fn(), from torch.profiler; None where it is missing"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            for name in PHASES:
                if name in ev.key:
                    total = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
                    out[name] = out.get(name, 0.0) + total / reps
        return out or None
    except Exception as e:          # a torch build without the device profiler
        print(f"  (phase times: torch.profiler failed: {e})")
        return None


def phase_bytes(n):
    """the bytes each phase moves at the least for a uint8 volume of n voxels without a truth"""
    return {"cc_local_kernel": n + 4 * n, "cc_merge_kernel": 4 * n // 4, "cc_flatten_kernel": 4 * n, "cc_choose_kernel": 4 * n,
            "cc_stats_kernel": 64, "cc_filter_kernel": 4 * n + n + n}


def host_route(mask_dev, structure):
    from scipy import ndimage as ndi
    m = mask_dev.cpu().numpy()
    lab, n = ndi.label(m == 1, structure=structure)
    if n:
        best = 1 + int(np.argmax(np.bincount(lab.ravel())[1:]))
        m = np.where((m == 1) & (lab != best), 0, m).astype(np.uint8)
    return torch.from_numpy(m).to(mask_dev.device), n


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
        raise SystemExit("bench_components.py measures on the MI355X: no GPU found")
    from dataset.few_shot_reader import FewshotRegReader
    from rpnet_amd import components as CC
    from rpnet_amd.volume import VolumeSegmenter
    from utils.util import load_yaml
    cfg, _ = load_yaml(a.yaml)
    cfg["n_iter_refinement"] = cfg["n_test_iter_refinement"]
    item = FewshotRegReader(None, cfg["eval_set_name"], cfg, mode="eval", n_volumes=1, n_slices=a.slices, size=a.size)[0]
    net = build_net(cfg)
    args = (item["support_images"], item["support_labels"], item["query_images"], item["appr_query_labels"], item["query_labels"])
    segs = {(s, k): VolumeSegmenter(net, batch=8, graphed=True, surface=s, keep_largest=k) for s in (False, True) for k in (False, 6)}
    res = segs[(False, 6)](*args)
    mask = res.mask.contiguous()
    D, H, W = mask.shape
    n = D * H * W
    gen = torch.Generator(device=DEV).manual_seed(1)
    volumes = (("final mask", mask), ("noise 0.31", (torch.rand((D, H, W), device=DEV, generator=gen) < 0.31).to(torch.uint8)),
               ("full volume", torch.ones((D, H, W), device=DEV, dtype=torch.uint8)))
    dst = torch.empty_like(mask)
    stats = torch.zeros((1, CC.STATS_ROW), device=DEV, dtype=torch.int64)
    out = [f"largest-component filter of a {D} x {H} x {W} uint8 volume ({n} voxels), ms, device-synchronised wall time, {a.reps} runs "
           f"after 3 warm-up runs; phases: kernel time in us (torch.profiler) | least bytes moved | that many bytes at 6.29 TB/s in us"]
    pb = phase_bytes(n)
    for name, vol in volumes:
        for conn in (6, 26):
            fn = lambda: CC.keep_largest(vol, connectivity=conn, out=dst, stats=stats)     # noqa: E731
            out.append(row(f"keep_largest: {name}, connectivity {conn}", timed(fn, a.reps)))
            out.append(f"    statistics row {stats[0].tolist()}, overrun word {CC.overrun(DEV, (D, H, W))}")
            ph = phase_times(fn, a.reps)
            if ph:
                out += [f"    {k:20s} {ph.get(k, float('nan')):9.1f} us | {pb[k]:11d} B | {pb[k] / COPY_RATE * 1e6:7.2f} us" for k in PHASES]
                out.append(f"    {'kernels together':20s} {sum(ph.values()):9.1f} us")
    try:
        from scipy import ndimage as ndi
    except ImportError:
        out.append("  host route: scipy is not installed here, not measured")
    else:
        for name, vol in volumes:
            for conn, rank in ((6, 1), (26, 3)):
                st = ndi.generate_binary_structure(3, rank)
                ts = []
                for _ in range(a.host_reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    host, ncomp = host_route(vol, st)
                    torch.cuda.synchronize()
                    ts.append((time.perf_counter() - t0) * 1e3)
                CC.keep_largest(vol, connectivity=conn, out=dst, stats=stats)
                same = torch.equal(host, dst) and int(stats[0, 1]) == ncomp
                out.append(row(f"host route: {name}, connectivity {conn}", (statistics.median(ts), min(ts), max(ts)))
                           + f"   same mask and component count as the device: {same}")
    base = None
    for (s, k), seg in segs.items():
        t = timed(lambda: seg(*args), a.reps)
        base = t if (s, k) == (False, False) else base
        out.append(row(f"volume, VolumeSegmenter batch 8 graphed, surface={s}, keep_largest={k}", t))
    t6, ts6, ts0 = (timed(lambda: segs[key](*args), a.reps) for key in ((False, 6), (True, 6), (True, False)))
    out.append(f"  keep_largest adds {t6[0] - base[0]:.3f} ms to the volume's {base[0]:.3f} ms; with surface {ts6[0] - ts0[0]:.3f} ms to {ts0[0]:.3f} ms "
               "(the filter and one more surface tally)")
    text = "\n".join(out)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
