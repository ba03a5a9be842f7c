#!/usr/bin/env python3
"""Time label fusion on the device against the host route, and write profiles/fusion.txt.

    python tools/bench_fusion.py [--out profiles/fusion.txt] [--reps 20]

Masks: a 64 x 256 x 256 uint8 phantom (one smooth object) and R perturbed copies of it (R = 5 and R = 12; misses 2 .. 45 %, false marks
0.2 %), made from a seed.  Real final masks need a trained checkpoint, which the repository does not carry.
Per R: `fuse` under each method and the pattern pass alone (`pattern_histogram`), each the median of `reps` calls with min and max,
every call timed by device events after a warm-up of 3.  The host route on the same box: masks `.cpu()`, a numpy vote (or a per-voxel
EM in float64 with STAPLE's stopping rule), the result uploaded; timed by the host clock around work that ends in a synchronise, after
the masks have been asserted equal to the device's.  One JSON line per measurement.
`decision_and_pass2_ms` is the difference of two medians (fuse minus the pattern pass) and `em_ms` the difference between STAPLE and
the vote, whose passes 1 and 2 are the same launches: neither separates the decision launch from pass 2.  For that split run
`--trace-only --R 12 --method staple` under a kernel trace (rocprofv3 --kernel-trace --stats): 20 `fuse` calls and nothing else, so
that the three kernels' rows are that configuration's."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from rpnet_amd import fusion as F

SHAPE = (64, 256, 256)
LO, HI = 2.0 ** -20, 1.0 - 2.0 ** -20


def phantom(R, seed=7):
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[np.linspace(-1, 1, s) for s in SHAPE], indexing="ij")
    truth = ((z * z + y * y + x * x) < 0.45).astype(np.uint8)
    raters = []
    for r in range(R):
        miss = (0.02, 0.03, 0.45, 0.45, 0.45, 0.1, 0.2, 0.3, 0.05, 0.4, 0.15, 0.25)[r]
        u = rng.random(SHAPE)
        raters.append(np.where(truth > 0, u >= miss, u < 0.002).astype(np.uint8))
    return truth, raters


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


def host_vote(d_raters, k):
    stack = np.stack([t.cpu().numpy() for t in d_raters])
    mask = ((stack == 1).sum(0) >= k).astype(np.uint8)
    out = torch.from_numpy(mask).to(d_raters[0].device)
    torch.cuda.synchronize()
    return out


def host_em(d_raters, max_iter=100, tol=1e-9):
    """per-voxel STAPLE in float64 on the host, consensus voxels left out, then the upload"""
    D = np.stack([t.cpu().numpy().ravel() == 1 for t in d_raters])
    R = D.shape[0]
    votes = D.sum(0)
    use = (votes > 0) & (votes < R)
    Du = D[:, use]
    g = Du.sum() / (R * Du.shape[1])
    p, q = np.full(R, 0.99999), np.full(R, 0.99999)
    for it in range(max_iter):
        a, b = np.full(Du.shape[1], g), np.full(Du.shape[1], 1.0 - g)
        for r in range(R):
            a *= np.where(Du[r], p[r], 1.0 - p[r])
            b *= np.where(Du[r], 1.0 - q[r], q[r])
        w = a / (a + b)
        pn = np.clip(np.array([w[Du[r]].sum() for r in range(R)]) / w.sum(), LO, HI)
        qn = np.clip(np.array([(1.0 - w)[~Du[r]].sum() for r in range(R)]) / (1.0 - w).sum(), LO, HI)
        delta = max(np.abs(pn - p).max(), np.abs(qn - q).max())
        p, q = pn, qn
        if delta < tol:
            break
    mask = (votes == R).astype(np.uint8)
    mask[use] = w >= 0.5
    out = torch.from_numpy(mask.reshape(SHAPE)).to(d_raters[0].device)
    torch.cuda.synchronize()
    return out, it + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "fusion.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace-only", action="store_true", help="only --reps fuse calls of one configuration, for a kernel trace")
    ap.add_argument("--R", type=int, default=5)
    ap.add_argument("--method", default="staple", choices=("vote", "weighted", "staple"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fusion needs the MI355X: there is nothing to time without it")
    dev = "cuda:0"
    if a.trace_only:
        d = [torch.from_numpy(r).to(dev) for r in phantom(a.R)[1]]
        out = torch.empty(SHAPE, dtype=torch.uint8, device=dev)
        kw = {"weights": [1.0 + 0.1 * r for r in range(a.R)]} if a.method == "weighted" else {}
        for _ in range(a.reps):
            F.fuse(d, method=a.method, out=out, **kw)
        torch.cuda.synchronize()
        return
    n = SHAPE[0] * SHAPE[1] * SHAPE[2]
    lines = []
    for R in (5, 12):
        truth, raters = phantom(R)
        d = [torch.from_numpy(r).to(dev) for r in raters]
        d_truth = torch.from_numpy(truth).to(dev)
        out = torch.empty(SHAPE, dtype=torch.uint8, device=dev)
        base = {"masks": "phantom 64x256x256 uint8 with perturbed copies (no checkpoint-free run makes real final masks)", "R": R, "voxels": n}
        t_pat = device_times(lambda: F.pattern_histogram(d, 1), a.reps)
        lines.append(dict(base, metric="pattern pass alone (memset + 1 launch)", bytes_moved=n * (R + 2),
                          gbytes_per_s=n * (R + 2) / t_pat["median_ms"] / 1e6, **t_pat))
        vote_ms = None
        for method, kw in (("vote", {}), ("weighted", {"weights": [1.0 + 0.1 * r for r in range(R)]}), ("staple", {})):
            res = F.fuse(d, method=method, truth=d_truth, out=out, **kw)
            stats = res.stats.cpu().numpy()[0]
            c = res.counts.cpu().numpy()[0]
            t = device_times(lambda: F.fuse(d, method=method, out=out, **kw), a.reps)
            vote_ms = t["median_ms"] if method == "vote" else vote_ms
            extra = {}
            if method == "staple":
                extra = {"em_ms": t["median_ms"] - vote_ms, "em_us_per_iteration": 1e3 * (t["median_ms"] - vote_ms) / max(int(stats[4]), 1)}
            lines.append(dict(base, metric=f"fuse, method {method} (memset + 3 launches)", iterations=int(stats[4]), disputed_voxels=int(stats[3]),
                              dice=2.0 * c[0] / (c[1] + c[2]), decision_and_pass2_ms=t["median_ms"] - t_pat["median_ms"],
                              decision_vs_pass2="not separated here: see --trace-only", bytes_moved=n * (R + 2 + 2 + 1), **t, **extra))
        # the host route, masks asserted equal first
        dev_vote = F.fuse(d, method="vote").mask
        assert torch.equal(host_vote(d, R // 2 + 1), dev_vote)
        hs = []
        for _ in range(3):
            t0 = time.perf_counter()
            host_vote(d, R // 2 + 1)
            hs.append((time.perf_counter() - t0) * 1e3)
        lines.append(dict(base, metric="host route: .cpu() + numpy vote + upload", median_ms=float(np.median(hs)), min_ms=min(hs), max_ms=max(hs),
                          reps=3))
        dev_staple = F.fuse(d, method="staple").mask
        t0 = time.perf_counter()
        host_mask, its = host_em(d)
        ms = (time.perf_counter() - t0) * 1e3
        differing = int((host_mask != dev_staple).sum().item())
        assert differing == 0, f"host EM and device STAPLE differ on {differing} voxels"
        lines.append(dict(base, metric="host route: .cpu() + per-voxel EM (float64 numpy) + upload", median_ms=ms, reps=1, iterations=its))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for row in lines:
            fh.write(json.dumps(row) + "\n")
            print(json.dumps(row))


if __name__ == "__main__":
    main()
