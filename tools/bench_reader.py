"""Train-mode episode production: the host reader against the device source, and what it does to the training step.

    python tools/bench_reader.py [--items 9] [--steps 30] [--out profiles/reader_train.txt]

On a data set written by volume_reader.write_synthetic_dataset at 256x256 (k = 12, the shipped do_deformable: False):
  (a) median wall time of a FewshotRegReader(mode="train") item on the host (registration on the GPU, as it stands),
  (b) median time of DeviceEpisodeSource.item, volumes cached, host clock around work that ends in a device synchronise
      (the HIP launches and the torch plumbing around them: index gathers, [0,1] maps, concatenation), and of batch(8),
  (c) train_rpnet.train ms/step at batch 8 on synthetic episodes and on the device source, same run.
"""
import argparse
import os
import random
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402

from rpnet_amd.episodes import DeviceEpisodeSource  # noqa: E402
from rpnet_amd.utils import volume_reader as VR  # noqa: E402
from train_rpnet import train  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--items", type=int, default=9)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reader_train.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_reader.py needs the MI355X (no CPU fallback)")
dev = torch.device("cuda:0")
cfg = yaml.load(open(os.path.join(ROOT, "yamls", "example.yml")), Loader=yaml.FullLoader)

with tempfile.TemporaryDirectory() as tmp:
    data_dir, set_name, csv_dir = VR.write_synthetic_dataset(tmp, n_volumes=3, classes=("Liver",), shape=(40, 272, 272), seed=5)
    cfg.update(class_csv_dir=csv_dir, train_classes=["Liver"], n_iter_refinement=cfg.get("n_iter_refinement", 4))
    for s in (random.seed, np.random.seed, torch.manual_seed):
        s(0)

    host = VR.FewshotRegReader(data_dir, set_name, cfg, mode="train")
    host[0]                                                       # code objects, base grids
    t_host = []
    for i in range(args.items):
        t0 = time.perf_counter()
        host[i % len(host)]
        t_host.append(time.perf_counter() - t0)

    src = DeviceEpisodeSource(data_dir, set_name, cfg, dev)
    src.warm()
    for i in range(len(src)):
        src.item(i)
    torch.cuda.synchronize()
    t_dev, t_enq = [], []
    for i in range(4 * args.items):
        t0 = time.perf_counter()
        src.item(i % len(src))
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t_dev.append(time.perf_counter() - t0)
        t_enq.append(t1 - t0)

    t_b8 = []
    for i in range(4 * args.items):
        t0 = time.perf_counter()
        src.batch(8)
        torch.cuda.synchronize()
        t_b8.append(time.perf_counter() - t0)

    def ms_per_step(source):
        train(cfg, 6, 8, 256, dev, log_every=0, source=source)            # warm-up of every shape
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        train(cfg, args.steps, 8, 256, dev, log_every=0, source=source)   # ends in a synchronise (its loss history)
        return (time.perf_counter() - t0) / args.steps * 1e3

    step = {"synthetic": [], "device source": []}
    for _ in range(2):                                                    # alternate the two
        step["synthetic"].append(ms_per_step(None))
        step["device source"].append(ms_per_step(src))

k = src.k
med = statistics.median
lines = [
    f"train-mode episode production, 256x256, k = {k} pairs per item, do_deformable: {cfg.get('do_deformable', True)}, MI355X",
    f"(a) host FewshotRegReader(mode='train') item: median {med(t_host) * 1e3:.1f} ms over {len(t_host)} items "
    f"(min {min(t_host) * 1e3:.1f}, max {max(t_host) * 1e3:.1f}) = {med(t_host) / k * 1e3:.2f} ms per pair",
    f"(b) DeviceEpisodeSource.item, volumes cached: median {med(t_dev) * 1e3:.2f} ms to completion over {len(t_dev)} items "
    f"(min {min(t_dev) * 1e3:.2f}, max {max(t_dev) * 1e3:.2f}), of which {med(t_enq) * 1e3:.2f} ms host enqueue "
    f"= {med(t_dev) / k * 1e3:.3f} ms per pair; host / device = {med(t_host) / med(t_dev):.0f} x",
    f"    batch(8) (items of {k} pairs, remainder carried over, so a call runs one item or none): mean {statistics.mean(t_b8) * 1e3:.2f} ms, "
    f"median {med(t_b8) * 1e3:.2f} ms, max {max(t_b8) * 1e3:.2f} ms over {len(t_b8)} calls",
    f"(c) train_rpnet.train, batch 8, {args.steps} steps, two alternating runs each: synthetic episodes "
    f"{' / '.join(f'{v:.1f}' for v in step['synthetic'])} ms/step; device source {' / '.join(f'{v:.1f}' for v in step['device source'])} ms/step",
    "    (a train() step is bench.py's forward + backward plus the gradient bucket's zeroing and all-reduce hook, the Adam update and the",
    "    episode itself; the synthetic episodes are generated on the host, which bounds that leg)",
]
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
