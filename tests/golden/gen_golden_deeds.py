#!/usr/bin/env python3
"""Golden vectors of the DEEDS registration stage from the REFERENCE itself.

Runs ONLY in the build container (needs /root/reference).  Imports net/registration.py of uci-cbcl/RP-Net with the absent third-party
modules stubbed, as tests/golden/gen_golden_registration.py does, and runs the reference's own AffineDEEDSRegistration on seeded
synthetic slices (rpnet_amd.utils.synth.make_episode), slice by slice on the CPU, composed like reference_deformable there: 50 Adam
steps (lr 0.01, MSE) of its affine stage, then DEEDSRegistration.train_registraion on the affine-warped source, then the module's
forward on the source and its label.  Writes tests/golden/registration_deeds.npz: seeds and dims, the reference's theta, its
affine-warped moving image (the input of the DEEDS stage), pred_xyz, sample_grid, the warped source (in [-1, 1]) and the thresholded
warped label.

    python tests/golden/gen_golden_deeds.py
"""
import importlib.machinery
import importlib.util
import os
import sys
import unittest.mock as mock

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))


def stub(name):
    m = mock.MagicMock()
    m.__spec__ = importlib.machinery.ModuleSpec(name, None)
    m.__name__ = name
    sys.modules[name] = m


for _m in ["cv2", "torchviz", "nrrd", "nibabel", "torchvision", "torchvision.transforms", "SimpleITK", "pydicom",
           "skimage", "skimage.measure", "utils", "utils.util"]:
    stub(_m)
import matplotlib  # noqa: E402

matplotlib.use("Agg")
spec = importlib.util.spec_from_file_location("refreg", "/root/reference/net/registration.py")
refreg = importlib.util.module_from_spec(spec)
sys.modules["refreg"] = refreg
spec.loader.exec_module(refreg)

import numpy as np  # noqa: E402
import torch  # noqa: E402

spec = importlib.util.spec_from_file_location("rp_synth", os.path.join(REPO, "rpnet_amd/utils/synth.py"))
synth = importlib.util.module_from_spec(spec)
sys.modules["rp_synth"] = synth
spec.loader.exec_module(synth)
torch.set_num_threads(8)


def reference_deeds(qry, supp, lab, grid_size, displacement_width, iters=50):
    src_all = (supp[:, 0].numpy() + 1) / 2.0
    dst_all = (qry[:, 0].numpy() + 1) / 2.0
    lab_all = lab.numpy()
    res = {k: [] for k in ("theta", "affined", "pred", "grid", "reg", "wsrc")}
    for s in range(len(dst_all)):
        src = torch.from_numpy(src_all[s])[None, None]
        dst = torch.from_numpy(dst_all[s])[None, None]
        src_label = torch.from_numpy(lab_all[s])[None, None]
        registration = refreg.AffineDEEDSRegistration(src_all[s].shape, use_GPU=False, stop_shear=False)
        registration.deeds = refreg.DEEDSRegistration(grid_size=grid_size, displacement_width=displacement_width)
        opt = torch.optim.Adam(registration.affine_reg.parameters(), lr=0.01)
        registration.affine_reg.train_registraion(src, dst, opt, loss_fn=refreg.MSE, iters=iters)
        with torch.no_grad():
            affined = registration.affine_reg(src).detach()
            # pred_xyz is a local of train_registraion, the result of its only torch.sum: kept as it passes
            sums, torch_sum = [], torch.sum

            def keeping_sum(*a, **kw):
                sums.append(torch_sum(*a, **kw))
                return sums[-1]
            with mock.patch.object(torch, "sum", keeping_sum):
                registration.deeds.train_registraion(affined, dst)
            assert len(sums) == 1 and tuple(sums[0].shape) == (grid_size ** 2, 2)
            res["theta"].append(registration.affine_reg.theta.data[0].clone())
            res["affined"].append(affined[0, 0].clone())
            res["pred"].append(sums[0].view(grid_size, grid_size, 2).clone())
            res["grid"].append(registration.deeds.sample_grid[0].clone())
            res["reg"].append((registration(src_label, None)[0, 0] > 0.1).float())
            res["wsrc"].append(registration(src, None)[0, 0] * 2 - 1)
    return {k: torch.stack(v) for k, v in res.items()}


CASES = [("g128", 91, 2, 64, 128, 15), ("g24", 92, 2, 48, 24, 7)]          # tag, seed, slices, size, grid_size, displacement_width
out = {}
for tag, seed, S, size, G, D in CASES:
    ep = synth.make_episode(seed, S, size)
    supp, lab, qry = [torch.from_numpy(a) for a in (ep["support_images"][0][0], ep["support_fg"][0][0], ep["query_images"])]
    ref = reference_deeds(qry, supp, lab, G, D)
    # the stored pred is the reference's: added to the base grid and upsampled by the nearest rule it gives the stored sample grid
    base = torch.nn.functional.affine_grid(torch.eye(2, 3).unsqueeze(0), (1, 1, G, G))
    again = torch.nn.functional.interpolate((base + ref["pred"]).permute(0, 3, 1, 2), size=(size, size), mode="nearest").permute(0, 2, 3, 1)
    err = (again - ref["grid"]).abs().max().item()
    print(f"{tag}: |pred| max {ref['pred'].abs().max().item():.3e}, sample grid from the stored pred: {err:.1e}, "
          f"label pixels {int(ref['reg'].sum())}")
    assert err == 0.0
    out.update({f"{tag}_dims": np.array([seed, S, size, G, D]), f"{tag}_theta": ref["theta"].numpy(), f"{tag}_affined": ref["affined"].numpy(),
                f"{tag}_pred_xyz": ref["pred"].numpy(), f"{tag}_sample_grid": ref["grid"].numpy(), f"{tag}_warped_src": ref["wsrc"].numpy(),
                f"{tag}_reg_pred": ref["reg"].numpy().astype(np.uint8)})
path = os.path.join(HERE, "registration_deeds.npz")
np.savez_compressed(path, **out)
print("wrote registration_deeds.npz", os.path.getsize(path) / 1e6, "MB")
