#!/usr/bin/env python3
"""Wall time of a data-set evaluation from NRRD volumes: host-built items (tools/eval_driver.py:evaluate_on_device over
FewshotRegReader(mode="eval"): both volumes decoded and preprocessed per item, the pairing in Python loops, registration results
copied down and up again, one tally transfer and one blocking NCC per volume) against device-built items
(rpnet_amd.dataset_eval: DeviceEvalSource + evaluate_dataset), each with the affine registration alone and with the demons stage.

    python tools/bench_dataset_eval.py [--slices 64] [--size 256] [--volumes 4] [--rounds 5] [--warmup 1] [--out FILE]

A synthetic data set in the reference's on-disk layout is written to a temporary directory (write_synthetic_dataset; the annotated
z-range of a volume is about `--slices`).  Every timing is a host clock around work that ends in a device synchronise; the
variants alternate inside every round, on one machine, in one process.  Reported: per variant the whole data set (median, min,
max over the rounds) and the time per item to completion (each item evaluated on its own, median over items and rounds); the one-off
cost of DeviceEvalSource.warm(); and the registration stage alone on one item's slices, with and without the demons stage.
"""
import argparse
import contextlib
import io
import os
import random
import shutil
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import yaml

from tools.eval_driver import evaluate_on_device

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _From:
    """item j of a reader / source as a one-item data set"""

    def __init__(self, inner, j):
        self.inner, self.j = inner, j

    def __len__(self):
        return 1

    def __getitem__(self, i):
        return self.inner[self.j]

    def item(self, i):
        return self.inner.item(self.j)


def build_net(cfg):
    from rpnet_amd.modules import RP_Net
    from rpnet_amd.utils.seeding import seed_module_
    net = RP_Net(cfg={"align": True, "backbone": "UNet"}, backbone_cfg=cfg).to(DEV)
    seed_module_(net)
    return net.eval()


def timed(fn):
    buf = io.StringIO()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(buf):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, buf.getvalue().splitlines()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--yaml", default=os.path.join(ROOT, "yamls", "example.yml"))
    ap.add_argument("--slices", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--volumes", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dataset_eval.py measures on the MI355X: no GPU found")
    from rpnet_amd import registration as R
    from rpnet_amd.dataset_eval import DeviceEvalSource, evaluate_dataset
    from rpnet_amd.utils import volume_reader as VR
    from rpnet_amd.volume import VolumeSegmenter

    root = tempfile.mkdtemp(prefix="dataset_eval_")
    try:
        # the organ's z-radius is 0.25 .. 0.35 of the depth: an annotated range of about 0.6 D
        depth, plane = int(round(a.slices / 0.6)), a.size + 32
        data_dir, set_name, csv_dir = VR.write_synthetic_dataset(root, n_volumes=a.volumes, classes=("Liver",), shape=(depth, plane, plane), seed=5)
        base = yaml.load(open(a.yaml), Loader=yaml.FullLoader)
        base.update(class_csv_dir=csv_dir, eval_classes=["Liver"], train_classes=["Liver"], n_shot=1, n_way=1, pad_value=-1024,
                    HU_range=[-1024, 3072], use_registration_loss=True, use_registration_mask=False, num_slice=depth + 16, num_x=plane,
                    num_y=plane, crop_size=[a.size, a.size])
        base["n_iter_refinement"] = base["n_test_iter_refinement"]
        variants, warm_s, sources = [], {}, {}
        for deformable in (False, True):
            cfg = dict(base, do_deformable=deformable)
            tag = "demons" if deformable else "affine"
            host = VR.FewshotRegReader(data_dir, set_name, cfg, mode="eval")
            net_h, net_d = build_net(cfg), build_net(cfg)
            seg = VolumeSegmenter(net_h, batch=a.batch, graphed=True)
            t0 = time.perf_counter()
            src = DeviceEvalSource(data_dir, set_name, cfg, DEV)
            src.warm()
            torch.cuda.synchronize()
            warm_s[tag] = time.perf_counter() - t0
            sources[tag] = src
            variants.append((f"host items, {tag}", cfg,
                             lambda rd, cfg=cfg, net=net_h, seg=seg: evaluate_on_device(net, rd, cfg, batch_size=a.batch, segmenter=seg), host))
            variants.append((f"device items, {tag}", cfg,
                             lambda rd, cfg=cfg, net=net_d: evaluate_dataset(net, rd, cfg, batch=a.batch, graphed=True), src))
        n = len(sources["affine"])
        depths = [sources["affine"].volume(c, i)[0].shape[0] for c, i in sources["affine"].reader.indices]
        whole = {name: [] for name, *_ in variants}
        per_item = {name: [] for name, *_ in variants}
        last = {}
        for rnd in range(a.warmup + a.rounds):
            for name, cfg, fn, rd in variants:
                random.seed(rnd)
                ms, lines = timed(lambda: fn(rd))
                last[name] = lines[-1]
                if rnd >= a.warmup:
                    whole[name].append(ms)
            for j in range(n):
                for name, cfg, fn, rd in variants:
                    random.seed(100 * rnd + j)
                    ms, _ = timed(lambda: fn(_From(rd, j)))
                    if rnd >= a.warmup:
                        per_item[name].append(ms)
        # the registration stage alone on the first item's slices
        random.seed(0)
        sources["affine"].item(0)
        pre = sources["affine"].pre
        sup01, q01, lab = (pre["support_images"][:, 0] + 1) / 2, (pre["query_images"][:, 0] + 1) / 2, pre["support_labels"]
        reg = {}
        for deformable in (False, True):
            ts = []
            for r in range(a.warmup + a.rounds):
                ms, _ = timed(lambda: R.register_slices(sup01, q01, lab, do_deformable=deformable))
                if r >= a.warmup:
                    ts.append(ms)
            reg[deformable] = ts
        out = [f"data set of {n} volumes, annotated depths {depths}, slices of {a.size}x{a.size}, T = {base['n_iter_refinement']}, 1-way 1-shot, "
               f"batch {a.batch} through the captured graph; ms, {a.rounds} rounds after {a.warmup} warm-up, variants alternating, "
               "device-synchronised host clock"]
        for name, *_ in variants:
            w, p = whole[name], per_item[name]
            out.append(f"  {name:22s} whole data set: median {statistics.median(w):9.1f}   min {min(w):9.1f}   max {max(w):9.1f}   |   "
                       f"per item to completion: median {statistics.median(p):8.1f}   min {min(p):8.1f}   max {max(p):8.1f}")
        out.append(f"  DeviceEvalSource.warm() (all volumes decoded, preprocessed and uploaded, once): {warm_s['affine']:.2f} s / {warm_s['demons']:.2f} s")
        out.append(f"  registration stage alone, {sup01.shape[0]} slices: affine median {statistics.median(reg[False]):.1f} ms (min {min(reg[False]):.1f}, "
                   f"max {max(reg[False]):.1f}); with the demons stage median {statistics.median(reg[True]):.1f} ms (min {min(reg[True]):.1f}, "
                   f"max {max(reg[True]):.1f})")
        out.append("last printed line of every variant:")
        out += [f"  {name:22s} {last[name]}" for name, *_ in variants]
        text = "\n".join(out)
        print(text)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text + "\n")
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
