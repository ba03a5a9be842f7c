"""Timing of rpnet_amd.preprocess on the MI355X: the lines for profiles/preprocess.txt.

  python tools/bench_preprocess.py [--reps 20] [--skip-host] > profiles/preprocess.txt

body_mask and clean_volume on a 64 x 256 x 256 and a 64 x 512 x 512 float volume (a body on a table, tests/preprocess_cases.py), median
of --reps with min and max; each stage on its own; beside them the host route through scipy.ndimage on the same box and the same
volumes (threshold by the numpy restatement, binary closing / opening with the same ball, label, binary_fill_holes, slice by slice),
with the masks asserted equal first."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from scipy import ndimage

from rpnet_amd import morphology as MO
from rpnet_amd import postprocess as PO
from rpnet_amd import preprocess as PP
from tests import morphology_cases as MX
from tests import preprocess_cases as PC


def timed(fn, reps):
    """median, min, max in ms of `reps` calls after two warm-up calls, each bracketed by events"""
    for _ in range(2):
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
    return float(np.median(ms)), min(ms), max(ms)


def host_chain(img, radius):
    st2 = MX.structure_of(MX.voxel_ball(int(radius * radius), per_slice=True))[0]
    m = PC.ref_threshold(img)[0].astype(bool)
    out = np.zeros(m.shape, np.uint8)
    H, W = m.shape[1:]
    for z in range(m.shape[0]):
        s = ndimage.binary_erosion(ndimage.binary_dilation(m[z], structure=st2), structure=st2, border_value=1)
        s = ndimage.binary_dilation(ndimage.binary_erosion(s, structure=st2, border_value=1), structure=st2)
        lab, _ = ndimage.label(s)
        s = (lab == lab[H // 2, W // 2]) & (lab > 0)
        out[z] = ndimage.binary_fill_holes(s)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--radius", type=int, default=7)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    dev = "cuda:0"
    line = lambda what, t: print(f"{what}: {t[0]:.3f} ms ({t[1]:.3f} .. {t[2]:.3f})")  # noqa: E731
    for shape in ((64, 256, 256), (64, 512, 512)):
        img = PC.body_phantom(shape, np.float32)[0]
        vol = torch.from_numpy(img).to(dev)
        mask, _ = PP.body_mask(vol, radius=a.radius)
        if not a.skip_host:
            t0 = time.perf_counter()
            want = host_chain(img, a.radius)
            host_ms = (time.perf_counter() - t0) * 1e3
            assert np.array_equal(mask.cpu().numpy(), want), "the device mask differs from the scipy.ndimage chain"
            print(f"{shape} host route (numpy Otsu + scipy.ndimage, masks equal): {host_ms:.1f} ms, one run")
        line(f"{shape} body_mask radius {a.radius}", timed(lambda: PP.body_mask(vol, radius=a.radius), a.reps))
        line(f"{shape} clean_volume (with the read of the box row)", timed(lambda: PP.clean_volume(vol, radius=a.radius), a.reps))
        thr = PP.threshold_mask(vol)[0]
        line(f"{shape} threshold_mask otsu", timed(lambda: PP.threshold_mask(vol), a.reps))
        line(f"{shape} threshold_mask fixed", timed(lambda: PP.threshold_mask(vol, -500.0), a.reps))
        line(f"{shape} closing per slice", timed(lambda: MO.closing(thr, (1,), a.radius, per_slice=True), a.reps))
        line(f"{shape} opening per slice", timed(lambda: MO.opening(thr, (1,), a.radius, per_slice=True), a.reps))
        line(f"{shape} seeded_component", timed(lambda: PP.seeded_component(thr, (1,)), a.reps))
        line(f"{shape} fill_holes slice", timed(lambda: PO.fill_holes(mask, (1,), connectivity=4, per_slice=True), a.reps))
        line(f"{shape} mask_bbox", timed(lambda: PP.mask_bbox(vol, mask), a.reps))


if __name__ == "__main__":
    main()
