"""Timing of rpnet_amd.volume_load on the MI355X against the host route on the same box: the lines for profiles/volume_load.txt.

  python tools/bench_volume_load.py [--reps 20] > profiles/volume_load.txt

Per volume, 64 x 256 x 256 and 64 x 512 x 512, int16 and float32, files (raw encoding) in a temporary directory: the host route
(FewshotVolumeReader.load_image_and_mask, then the upload of the two float32 volumes) against DeviceVolumeLoader.load, wall clock to a
device synchronise, the time spent reading and decoding the files given separately for both; the select + clip pair alone (events around
window_normalize, in place, 9 + 1 launches), with the bytes of its byte account (four 4-byte read passes, one read, one write: 24 B per
voxel) per second and as a share of the 6.29 TB/s copy rate of the README; numpy.percentile alone on the same box.  Per item:
DeviceEpisodeSource.item with cache_volumes=False, with and without device_load.  Every figure is the median of --reps samples with min and
max, in one process.  The outputs of the two routes are compared for equality first."""
import argparse
import os
import random
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from rpnet_amd import volume_load as VL
from rpnet_amd.utils import nrrd
from rpnet_amd.utils import volume_reader as VR
from tests import volload_cases as VC
from tools.bench_resample import COPY_RATE, timed


def stats(samples):
    return f"{np.median(samples) * 1e3:.2f} ms ({min(samples) * 1e3:.2f} .. {max(samples) * 1e3:.2f})"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_volume_load.py measures on the MI355X; there is no device here")
    dev = torch.device("cuda:0")
    print(f"numpy {np.__version__}, torch {torch.__version__}, {a.reps} samples per figure: median (min .. max)")
    with tempfile.TemporaryDirectory() as tmp:
        for shape in ((64, 256, 256), (64, 512, 512)):
            cfg = VC.config((64, 512, 512), [256, 256])
            for dtype in (np.int16, np.float32):
                d = os.path.join(tmp, "%dx%dx%d_%s" % (shape + (np.dtype(dtype).name,)))
                os.makedirs(d)
                nrrd.write(os.path.join(d, "p_clean.nrrd"), VC.file_volume(shape, dtype, 1), encoding="raw")
                nrrd.write(os.path.join(d, "p_Liver.nrrd"), VC.file_mask(shape, np.uint8, 0, shape[0] - 1), encoding="raw")
                rd = object.__new__(VR.FewshotVolumeReader)
                rd.data_dir, rd.cfg = d, cfg
                loader = VL.DeviceVolumeLoader(rd, dev)
                want, got = rd.load_image_and_mask("p", "Liver"), loader.load("p", "Liver")
                assert np.array_equal(got[0].cpu().numpy().view(np.uint32), want["image"][0].view(np.uint32)), "the routes differ"
                assert np.array_equal(got[1].cpu().numpy(), want["mask"][0])
                host, host_read, device, device_read = [], [], [], []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    nrrd.read(os.path.join(d, "p_Liver.nrrd")), nrrd.read(os.path.join(d, "p_clean.nrrd"))
                    host_read.append(time.perf_counter() - t0)
                    t0 = time.perf_counter()
                    s = rd.load_image_and_mask("p", "Liver")
                    v = (torch.from_numpy(s["image"][0]).to(dev), torch.from_numpy(s["mask"][0]).to(dev))
                    torch.cuda.synchronize()
                    host.append(time.perf_counter() - t0)
                    t0 = time.perf_counter()
                    v = loader.load("p", "Liver")
                    torch.cuda.synchronize()
                    device.append(time.perf_counter() - t0)
                    device_read.append(loader.last_read_seconds)
                del v
                name = f"{shape} {np.dtype(dtype).name} -> {tuple(got[0].shape)}"
                print(f"{name} host route load_image_and_mask + upload: {stats(host)}, of which reading the two files {stats(host_read)}")
                print(f"{name} DeviceVolumeLoader.load: {stats(device)}, of which reading the two files {stats(device_read)}")
                x = got[0].clone()
                n = x.numel()
                t = timed(lambda: VL.window_normalize(x, *VC.HU, out=x), a.reps, 10)
                rate = 24 * n / (t[0] * 1e-3)
                print(f"{name} select + clip pair alone ({n} voxels, 10 launches): {t[0]:.4f} ms ({t[1]:.4f} .. {t[2]:.4f}), {24 * n / 1e6:.1f} MB "
                      f"by the byte account, {rate / 1e12:.3f} TB/s = {100 * rate / COPY_RATE:.1f}% of the copy rate")
                arr, pct = want["image"][0] * 1000, []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    np.percentile(arr, 99.5)
                    pct.append(time.perf_counter() - t0)
                print(f"{name} numpy.percentile alone on the host: {stats(pct)}")
        from rpnet_amd.episodes import DeviceEpisodeSource
        from tests.reader_cases import config_for
        case = {"data": dict(n_volumes=3, classes=("Liver",), shape=(64, 256, 256), seed=11),
                "cfg": dict(num_slice=64, num_x=256, num_y=256, crop_size=[256, 256], k=4)}
        data_dir, set_name, csv_dir = VR.write_synthetic_dataset(os.path.join(tmp, "items"), **case["data"])
        cfg = dict(config_for(case, csv_dir), do_elastic=False, do_deformable=False)
        for on in (False, True):
            src = DeviceEpisodeSource(data_dir, set_name, cfg, dev, cache_volumes=False, device_load=on)
            random.seed(1), np.random.seed(1), torch.manual_seed(1)
            src.item(0)
            torch.cuda.synchronize()
            samples = []
            for j in range(a.reps):
                t0 = time.perf_counter()
                src.item(j % len(src))
                torch.cuda.synchronize()
                samples.append(time.perf_counter() - t0)
            print(f"DeviceEpisodeSource.item, 64 x 256 x 256 int16 gzip volumes, cache_volumes=False, device_load={on}: {stats(samples)}")


if __name__ == "__main__":
    main()
