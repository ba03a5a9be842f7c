"""The DEEDS restatement of tests/deeds_cases.py held to the reference's own run (tests/golden/registration_deeds.npz), its nearest index
rule held to torch, and the comparison rule shown to notice seeded defects.  Runs without a GPU."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import deeds_cases as DC
from tests.reg_cases import worst

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "registration_deeds.npz")
FIXTURE_CASES = ["g128", "g24"]


def fixture(tag):
    z = np.load(GOLDEN)
    seed, S, size, G, D = [int(v) for v in z[tag + "_dims"]]
    return dict(S=S, size=size, G=G, D=D, **{k: torch.from_numpy(z[f"{tag}_{k}"]) for k in
                                            ("theta", "affined", "pred_xyz", "sample_grid", "warped_src", "reg_pred")}), seed


def fixture_inputs(tag):
    """(fx, moving = the reference's affine-warped source, fixed, source, label): the slices of make_episode(seed)"""
    from rpnet_amd.utils.synth import make_episode
    fx, seed = fixture(tag)
    ep = make_episode(seed, fx["S"], fx["size"])
    src = torch.from_numpy((ep["support_images"][0][0][:, 0] + 1) / 2.0).float()
    dst = torch.from_numpy((ep["query_images"][:, 0] + 1) / 2.0).float()
    lab = torch.from_numpy(ep["support_fg"][0][0]).float()
    return fx, fx["affined"], dst, src, lab


def affine_warped(x, theta):
    return F.grid_sample(x[:, None], F.affine_grid(theta, (x.shape[0], 1) + tuple(x.shape[1:]), align_corners=False), align_corners=False)[:, 0]


@pytest.mark.parametrize("tag", FIXTURE_CASES)
def test_float32_restatement_reproduces_the_reference(tag):
    """the float32 restatement against the reference's stored run: pred, sample grid and warped source within 3 e32 (e32 = float32
    against float64 of the restatement itself), the thresholded label equal; measured: every difference is 0.0"""
    fx, mov, fix, src, lab = fixture_inputs(tag)
    G, D, size = fx["G"], fx["D"], fx["size"]
    pred32, _ = DC.deeds_ref(mov, fix, G, D, 0.1, DC.DEF, DC.F32)
    pred64, _ = DC.deeds_ref(mov, fix, G, D, 0.1, DC.DEF, DC.F64)
    grid32 = DC.sampling_grid(pred32, size, size, "nearest", DC.F32)
    grid64 = DC.sampling_grid(pred32, size, size, "nearest", DC.F64)
    aw_src, aw_lab = affine_warped(src, fx["theta"]), affine_warped(lab, fx["theta"])
    assert torch.equal(aw_src, mov)
    wsrc32, _ = DC.warp_ref(aw_src, pred32, "nearest", scale=2.0, shift=-1.0, dtype=DC.F32)
    wsrc64, _ = DC.warp_ref(aw_src, pred32, "nearest", scale=2.0, shift=-1.0, dtype=DC.F64)
    lab32, _ = DC.warp_ref(aw_lab, pred32, "nearest", threshold=0.1, dtype=DC.F32)
    figures = {"pred": ((pred32 - fx["pred_xyz"]).abs().max().item(), 3 * (pred32.double() - pred64).abs().max().item()),
               "sample_grid": ((grid32 - fx["sample_grid"]).abs().max().item(), 3 * (grid32.double() - grid64).abs().max().item()),
               "warped_src": ((wsrc32 - fx["warped_src"]).abs().max().item(), 3 * (wsrc32.double() - wsrc64).abs().max().item())}
    print(tag, figures, "|pred| max", pred64.abs().max().item())
    for name, (err, tol) in figures.items():
        assert err <= tol, (name, err, tol)
    assert torch.equal(lab32, fx["reg_pred"].float())
    assert fx["reg_pred"].sum() > 100 and pred64.abs().max() > 1e-4


@pytest.mark.parametrize("n_in,n_out", [(128, 64), (24, 48), (9, 41), (9, 37), (18, 33), (18, 65), (1, 16), (5, 11), (128, 256), (7, 65),
                                        (15, 40), (512, 3), (3, 512), (31, 1000)])
def test_nearest_index_rule_is_torchs(n_in, n_out):
    idx = DC.nearest_index(n_in, n_out)
    for dtype in (torch.float32, torch.float64):
        image = torch.arange(n_in, dtype=dtype)
        rows = F.interpolate(image[None, None, :, None].expand(1, 1, n_in, 2).contiguous(), size=(n_out, 2), mode="nearest")[0, 0, :, 0]
        cols = F.interpolate(image[None, None, None, :].expand(1, 1, 2, n_in).contiguous(), size=(2, n_out), mode="nearest")[0, 0, 0]
        assert torch.equal(rows.long(), idx) and torch.equal(cols.long(), idx), (n_in, n_out, dtype)
    assert not torch.equal(DC.nearest_index(n_in, n_out, "nearest_off_by_one"), idx) or n_in == 1


@pytest.mark.parametrize("case", DC.CASES, ids=DC.case_id)
def test_every_case_passes_with_the_float32_restatement(case):
    recs = DC.check_case(DC.RefBackend(DC.F32), case)
    DC.hold(recs)
    mov, fix, pred64, cost64, _, _ = DC.reference(case)
    S, H, W, G, D, R, alpha, mode = case
    assert torch.isfinite(cost64).all() and tuple(pred64.shape) == (S, G, G, 2) and tuple(cost64.shape) == (S, G * G, D * D)
    if alpha[5] == 0 or D == 1:         # uniform weights: the mean of a symmetric set of shifts
        assert pred64.abs().max() < 1e-15
    elif G > 1:
        assert pred64.abs().max() > 1e-4


@pytest.mark.parametrize("shape", DC.WARP_SHAPES, ids=str)
def test_warp_cases_pass_with_the_float32_restatement(shape):
    DC.hold(DC.check_warps(DC.RefBackend(DC.F32), shape))


@pytest.mark.parametrize("defect", DC.DEFECTS)
def test_seeded_defects_fail_the_checks(defect):
    """every defect is caught by the rule on at least one case of the table it can show in, by a factor of 100 or more"""
    small = [c for c in DC.CASES if c[3] * c[3] * c[4] * c[4] <= 18 * 18 * 225]
    if defect == "drop_alpha3":
        small = [c for c in small if c[6][3] != 0]
    if defect == "nearest_off_by_one":
        small = [c for c in small if c[7] == "nearest" and c[3] > 1]
    if defect == "seam":
        small = [c for c in small if c[3] > DC.TILE + 2]
    ratios = [worst(DC.check_case(DC.RefBackend(DC.F32, defect), case)) for case in small]
    print(defect, ["%.1e" % r for r in ratios])
    assert max(ratios) > 100, (defect, ratios)


def test_recovery_case_has_its_margin():
    """the constructed case of tests/test_gpu_deeds.py on the float64 reference: at interior points the displacement that undoes the shift
    has the lowest cost by the margin the softmax needs, and pred is that shift"""
    mov, fix, R = DC.recovery_pair()
    G, D = DC.REC["G"], DC.REC["D"]
    pred, cost = DC.deeds_ref(mov, fix, G, D, R, DC.REC["alpha"], DC.F64)
    kx, ky = DC.REC["px"]
    best = (ky + D // 2) * D + (kx + D // 2)
    inner = torch.zeros(G, G, dtype=torch.bool)
    b = DC.REC["border"]
    inner[b:G - b, b:G - b] = True
    c = cost[0][inner.reshape(-1)]
    others = torch.cat([c[:, :best], c[:, best + 1:]], 1).min(1).values
    margin = (others - c[:, best]).min().item()
    step = DC.f32(R) * 2 / D
    want = torch.tensor([kx * step, ky * step], dtype=torch.float64)
    err = (pred[0][inner] - want).abs().max().item()
    print(f"margin {margin:.4f} (needed {DC.recovery_margin_needed():.4f}), pred error {err / step:.3f} steps")
    assert margin >= DC.recovery_margin_needed()
    assert err < 0.5 * step
