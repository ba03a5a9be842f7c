#!/usr/bin/env python3
"""Wall time per evaluated volume: the driver's host loop (tools/eval_driver.py:evaluate — softmax, `.cpu()` and numpy Dice per
call) against rpnet_amd.volume.VolumeSegmenter (one tally launch per call, one transfer per volume).

    python tools/bench_volume.py [--slices 64] [--size 256] [--volumes 20] [--out FILE]
        variants, run alternately, one volume each per round; every timing ends in a device synchronise:
          host loop, batch 2, eager               the parent's evaluate()
          host loop, batch 2, GraphedEval         the same loop with only `net` swapped for GraphedEval(net)
          on device, batch 2, eager / graphed     evaluate_on_device()
          on device, batch 8, graphed
        prints median, minimum and maximum per variant.
    python tools/bench_volume.py --tally-only [--batch 8]
        the tally launch alone (T = 10 logit tensors + output + baseline) and, for scale, an existing streaming pass of the library
        of the same traffic (rpnet_bn_eval_relu: reads and writes fp32 once); for a `rocprofv3 --kernel-trace --stats` run of its own.
"""
import argparse
import contextlib
import io
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.eval_driver import evaluate, evaluate_on_device

DEV = "cuda:0"


class _One:
    def __init__(self, item):
        self.item = item

    def __len__(self):
        return 1

    def __getitem__(self, i):
        return self.item


class _Graphed:
    """GraphedEval behind the `net.eval()` call of evaluate()"""

    def __init__(self, net):
        from rpnet_amd.graph import GraphedEval
        self.g = GraphedEval(net)

    def eval(self):
        return self

    def __call__(self, *a, **kw):
        return self.g(*a, **kw)


def build_net(cfg):
    from rpnet_amd.modules import RP_Net
    from rpnet_amd.utils.seeding import seed_module_
    net = RP_Net(cfg={"align": True, "backbone": "UNet"}, backbone_cfg=cfg).to(DEV)
    seed_module_(net)
    return net.eval()


def volumes(a):
    from dataset.few_shot_reader import FewshotRegReader
    from utils.util import load_yaml
    cfg, _ = load_yaml(a.yaml)
    cfg["n_iter_refinement"] = cfg["n_test_iter_refinement"]
    ds = FewshotRegReader(None, cfg["eval_set_name"], cfg, mode="eval", n_volumes=1, n_slices=a.slices, size=a.size)
    item = _One(ds[0])
    # nets of the same seed: GraphedEval freezes the weight packs of the net it wraps (the eager variants keep the parent's behaviour),
    # and a net carries ONE GraphedEval (a second wrapper would clear the packs the first one's graphs point to)
    net, net_h, net_g = build_net(cfg), build_net(cfg), build_net(cfg)
    graphed = _Graphed(net_h)
    from rpnet_amd.volume import VolumeSegmenter
    # one VolumeSegmenter per variant, kept over the volumes as a user's loop keeps it (its captured graphs live with it)
    segs = {k: VolumeSegmenter(net_g if k[1] else net, batch=k[0], graphed=k[1]) for k in ((2, False), (2, True), (8, True))}
    variants = [
        ("host loop, batch 2, eager", lambda: evaluate(net, item, cfg, 1, 2)),
        ("host loop, batch 2, GraphedEval", lambda: evaluate(graphed, item, cfg, 1, 2)),
        ("on device, batch 2, eager", lambda: evaluate_on_device(net, item, cfg, 1, segmenter=segs[2, False])),
        ("on device, batch 2, graphed", lambda: evaluate_on_device(net_g, item, cfg, 1, segmenter=segs[2, True])),
        ("on device, batch 8, graphed", lambda: evaluate_on_device(net_g, item, cfg, 1, segmenter=segs[8, True])),
    ]
    times = {name: [] for name, _ in variants}
    lines = {}
    for rnd in range(a.warmup + a.volumes):
        for name, fn in variants:
            buf = io.StringIO()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(buf):
                fn()
            torch.cuda.synchronize()
            if rnd >= a.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
            lines[name] = buf.getvalue().splitlines()[0]
    out = [f"volume of {a.slices} slices of {a.size}x{a.size}, T = {cfg['n_iter_refinement']}, 1-way 1-shot; ms per volume, "
           f"{a.volumes} volumes per variant after {a.warmup} warm-up rounds, variants alternating, device-synchronised"]
    for name, _ in variants:
        t = times[name]
        out.append(f"  {name:34s} median {statistics.median(t):8.2f}   min {min(t):8.2f}   max {max(t):8.2f}")
    out.append("last printed line of every variant (the Dice values agree):")
    out += [f"  {name:34s} {lines[name]}" for name, _ in variants]
    return out


def tally_only(a):
    from rpnet_amd import hip
    from rpnet_amd.volume import seg_tally
    N, K, H, W, T = a.batch, 2, a.size, a.size, 10
    g = torch.Generator(device=DEV).manual_seed(0)
    logits = [torch.randn(N, K, H, W, device=DEV, generator=g) * 3 for _ in range(T + 1)]
    base = (torch.rand(N, H, W, device=DEV, generator=g) < 0.4).float()
    labels = (torch.rand(N, H, W, device=DEV, generator=g) < 0.4).int()
    counts = torch.zeros(T + 2, K - 1, 3, device=DEV, dtype=torch.int64)
    mask = torch.empty(N, H, W, device=DEV, dtype=torch.uint8)
    nv = torch.full((1,), N, device=DEV, dtype=torch.int32)
    srcs, kinds = logits + [base], [0] * (T + 1) + [1]
    bytes_tally = sum(t.numel() * 4 for t in srcs) + labels.numel() * 4 + mask.numel()
    # the yardstick: relu(y scale + shift) over as many bytes (half read, half written)
    C = 64
    P = bytes_tally // (2 * 4 * C)
    y, z = torch.randn(P, C, device=DEV, generator=g), torch.empty(P, C, device=DEV)
    sc, sh, mx = torch.ones(C, device=DEV), torch.zeros(C, device=DEV), torch.zeros(1, device=DEV)
    bytes_bn = 2 * P * C * 4

    def tally():
        seg_tally(srcs, kinds, nv, labels, counts, mask, mask_src=T, K=K)

    def bn():
        hip.call("rpnet_bn_eval_relu", hip.ptr(y), hip.ptr(sc), hip.ptr(sh), hip.ptr(z), hip.ptr(mx), P, C)
    out = []
    for name, fn, nbytes in (("seg_tally_kernel", tally, bytes_tally), ("bn_eval_relu_kernel", bn, bytes_bn)):
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / a.reps * 1e3
        out.append(f"  {name:22s} {nbytes / 1e6:7.2f} MB per launch, {us:7.2f} us per launch back to back (device events, {a.reps} launches): "
                   f"{nbytes / us / 1e6:6.2f} TB/s")
    return [f"tally launch alone: batch {N}, {H}x{W}, K = {K}, {T + 2} sources"] + out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--yaml", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "yamls", "example.yml"))
    ap.add_argument("--slices", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--volumes", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tally-only", action="store_true")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_volume.py measures on the MI355X: no GPU found")
    text = "\n".join(tally_only(a) if a.tally_only else volumes(a))
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
