"""CPU self-check of tests/ref64.py: its float64 functions agree with the oracle's restatement of the same operator sequences
(oracle/rpnet_oracle.py, itself pinned to the reference's recorded values by test_oracle_golden.py) to 1e-12.  The two are
written independently; ref64 is not built from the oracle."""
import pytest
import torch

from tests import ref64 as R
from tests.helpers import rel_err, rnd


def nchw(f, h, w):
    return f.reshape(f.shape[0], h, w, f.shape[-1]).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("B,C,H,W,h,w,nmask", [(2, 8, 24, 20, 6, 5, 3), (1, 64, 32, 32, 8, 8, 2)])
def test_masked_pool_is_get_features_as_written(B, C, H, W, h, w, nmask):
    from oracle import rpnet_oracle as O
    f = rnd(1, B, h * w, C)
    masks = (torch.rand(nmask, B, H, W, generator=torch.Generator().manual_seed(2)) > 0.5).float()
    masks[-1] = 0                                   # an empty mask
    fts = nchw(f, h, w).double()
    ref = torch.stack([torch.cat([O.get_features_as_written(fts[[b]], masks[k, [b]].double()) for k in range(nmask)], 0)
                       for b in range(B)], 0)
    assert rel_err(R.masked_pool(f, masks, h, w), ref) < 1e-12
    # the adjoint weights: the oracle's explicit tap construction against autograd of the up-sampler
    am, msum = R.mask_adjoint(masks, h, w)
    ref_am = O.bilinear_adjoint(masks.double(), h, w).reshape(nmask, B, h * w).transpose(0, 1)
    assert rel_err(am, ref_am) < 1e-6               # the oracle builds its tap weights in float32
    assert torch.equal(msum, masks.double().sum((2, 3)).t())


@pytest.mark.parametrize("B,K,C,h,w", [(2, 2, 64, 8, 6), (1, 4, 8, 5, 7)])
def test_cosine_match_is_cal_dist(B, K, C, h, w):
    from oracle import rpnet_oracle as O
    f, p = rnd(3, B, h * w, C), rnd(4, B, K, C)
    fts = nchw(f, h, w).double()
    ref = torch.stack([torch.stack([O.cal_dist(fts[[b]], p[b, [k]].double()) for k in range(K)], 1)[0] for b in range(B)], 0)
    assert rel_err(R.cosine_match(f, p, 20.0).reshape(B, K, h, w), ref) < 1e-12


@pytest.mark.parametrize("B,K,H,W", [(3, 2, 24, 20), (2, 4, 7, 5)])
def test_dice_ce_is_the_oracles(B, K, H, W):
    from oracle import rpnet_oracle as O
    logits = rnd(5, B, K, H, W) * 2
    labels = torch.randint(0, K, (B, H, W), generator=torch.Generator().manual_seed(6))
    assert rel_err(R.dice_ce(logits, labels), O.dice_ce(logits.double(), labels)) < 1e-12
    lg = logits.double().requires_grad_(True)
    (g,) = torch.autograd.grad(O.dice_ce(lg, labels), lg)
    assert rel_err(R.dice_ce_bwd(logits, labels), g) < 1e-12


def test_per_sample_form_is_the_align_loss_term():
    """per_sample = 1 with ignore_index = 255 and a zero weight is alignLoss's sum of per-episode F.cross_entropy calls over the
    episodes that are not skipped, divided by the number of episodes (net/rp_net.py:343,349,414,421,438)"""
    import torch.nn.functional as F
    B, K, H, W = 3, 2, 12, 10
    logits = rnd(7, B, K, H, W).double()
    labels = torch.randint(0, K, (B, H, W), generator=torch.Generator().manual_seed(8))
    labels[:, ::3] = 255
    w = torch.tensor([1.0, 0.0, 1.0])
    want = (F.cross_entropy(logits[[0]], labels[[0]], ignore_index=255) + F.cross_entropy(logits[[2]], labels[[2]], ignore_index=255)) / B
    assert rel_err(R.dice_ce(logits, labels, with_dice=0, ignore_index=255, per_sample=1, sample_weight=w), want) < 1e-12


def test_float32_is_the_same_code():
    f, p = rnd(9, 2, 30, 16), rnd(10, 2, 3, 16)
    a, b = R.cosine_match(f, p), R.cosine_match(f, p, dtype=torch.float32)
    assert a.dtype == torch.float64 and b.dtype == torch.float32 and 0 < rel_err(b, a) < 1e-5


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("B,C,h,w,r", [(2, 8, 7, 9, 3), (1, 64, 3, 5, 5)])
def test_local_corr_is_the_oracles(B, C, h, w, r):
    from oracle import rpnet_oracle as O
    f1, f2, go = rnd(21, B, h, w, C), rnd(22, B, h, w, C), rnd(23, B, h, w, (2 * r + 1) ** 2 + 3)
    a, b = nchw(f1, h, w).double().requires_grad_(True), nchw(f2, h, w).double().requires_grad_(True)
    ref = O.local_correlation(a, b, r)
    kk = ref.shape[1]
    g1, g2 = torch.autograd.grad(ref, (a, b), go[..., :kk].permute(0, 3, 1, 2).double())
    out = R.local_corr(f1, f2, r, cstride=kk + 3)
    assert out.dtype == torch.float64 and out.shape == (B, h, w, kk + 3) and out[..., kk:].abs().max() == 0
    assert rel_err(out[..., :kk], nhwc(ref)) < 1e-12
    add = rnd(24, B, h, w, C)
    d1, d2 = R.local_corr_bwd(f1, f2, go, r, df1_add=add)         # the three channels of go beyond KK are ignored
    assert rel_err(d1, nhwc(g1) + add.double()) < 1e-12 and rel_err(d2, nhwc(g2)) < 1e-12
    assert torch.equal(R.local_corr_bwd(f1, f2, go, r)[1], d2)


def test_local_corr_is_the_recorded_correlation():
    """corr_r5_* of tests/golden/ops.npz: the reference's own Correlation() and its autograd in float32 (the inputs are those of
    tests/test_gpu_ops.py::test_local_correlation_golden)"""
    import os
    import numpy as np
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops.npz"))
    b, c, h, w, r = (int(v) for v in g["corr_r5_dims"])
    f1, f2, go = nhwc(rnd(11, b, c, h, w)), nhwc(rnd(12, b, c, h, w)), nhwc(rnd(13, b, 121, h, w))
    assert rel_err(R.local_corr(f1, f2, r), nhwc(torch.from_numpy(g["corr_r5_out"]))) < 1e-5
    d1, d2 = R.local_corr_bwd(f1, f2, go, r)
    assert rel_err(d1, nhwc(torch.from_numpy(g["corr_r5_g1"]))) < 1e-5 and rel_err(d2, nhwc(torch.from_numpy(g["corr_r5_g2"]))) < 1e-5


def test_local_corr_outside_the_image_is_exactly_zero():
    B, h, w, C, r = 2, 3, 5, 8, 5
    K = 2 * r + 1
    out = R.local_corr(rnd(25, B, h, w, C) + 3, rnd(26, B, h, w, C) + 3, r).reshape(B, h, w, K, K)      # [.., a, c]
    for y in range(h):
        for x in range(w):
            for a in range(K):
                for c in range(K):
                    inside = 0 <= y + c - r < h and 0 <= x + a - r < w
                    assert inside or (out[:, y, x, a, c] == 0.0).all()
                    assert not inside or (out[:, y, x, a, c] != 0.0).all()


@pytest.mark.parametrize("taps,dilation,upsample,mode,two", [(9, 1, 0, 0, False), (9, 1, 0, 1, True), (9, 1, 1, 2, False),
                                                             (9, 2, 0, 0, True), (1, 1, 0, 0, True), (9, 1, 1, 0, True)])
def test_conv_wgrad_is_autograd_of_conv2d(taps, dilation, upsample, mode, two):
    """the pin of R.conv_wgrad (shifted slices and einsum): autograd of F.conv2d in float64 on the same gathered input"""
    import torch.nn.functional as F
    N, H, W, C0, C1, Co = 2, 6, 10, 5, 3 if two else 0, 4
    h, w = H >> upsample, W >> upsample
    x0, x1 = rnd(901, N, h, w, C0), rnd(902, N, h, w, C1) if two else None
    dy, s = rnd(903, N, H, W, Co), torch.rand(N, h, w, generator=torch.Generator().manual_seed(904))
    got = R.conv_wgrad(x0, x1, dy, taps, dilation, upsample, s if mode else None, mode)
    x = (x0 if x1 is None else torch.cat([x0, x1], -1)).double()
    if mode:
        x = x * (s.double() if mode == 1 else 1 - s.double())[..., None]
    x = x.permute(0, 3, 1, 2)
    if upsample:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    k = 3 if taps == 9 else 1
    wt = torch.zeros(Co, C0 + C1, k, k, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, wt, padding=dilation if taps == 9 else 0, dilation=dilation if taps == 9 else 1)
    (want,) = torch.autograd.grad(y, wt, dy.double().permute(0, 3, 1, 2))
    assert got.shape == want.shape and rel_err(got, want) < 1e-14
    assert R.conv_wgrad(x0, x1, dy, taps, dilation, upsample, s if mode else None, mode, dtype=torch.float32).dtype == torch.float32


@pytest.mark.parametrize("groups", [1, 2])
def test_first_layer_references_are_autograd_of_conv_bn_relu(groups):
    """the pin of R.conv1, conv1_affine_relu, bn_bwd_sums, bn_dy and conv1_dgrad: autograd of nn.Conv2d(1, C, 3, padding=1) ->
    nn.BatchNorm2d (train mode, one batch per statistic group) -> nn.ReLU in float64"""
    import torch.nn.functional as F
    N, H, W, C, eps = 4, 5, 7, 6, 1e-5
    x, w, b = rnd(911, N, H, W).double(), rnd(912, C, 1, 3, 3).double(), rnd(913, C).double()
    gamma, beta, dz = 1 + 0.1 * rnd(914, C).double(), 0.1 * rnd(915, C).double(), rnd(916, N, H, W, C).double()
    xr, wr, gr, br = (t.clone().requires_grad_(True) for t in (x, w, gamma, beta))
    n = N // groups
    ys = [F.conv2d(xr[g * n:(g + 1) * n, None], wr, b, padding=1) for g in range(groups)]
    z = torch.cat([torch.relu(F.batch_norm(y, None, None, gr, br, True, 0.1, eps)) for y in ys]).permute(0, 2, 3, 1)
    dx, dw, dg, db = torch.autograd.grad(z, (xr, wr, gr, br), dz)
    y = R.conv1(x, w, b)
    assert rel_err(y, torch.cat(ys).permute(0, 2, 3, 1)) < 1e-12
    yg = y.reshape(groups, -1, C)
    mean, var = yg.mean(1), yg.var(1, unbiased=False)
    invstd = (var + eps).rsqrt()
    stats = torch.stack([gamma * invstd, beta - mean * gamma * invstd, mean, invstd])
    assert rel_err(R.conv1_affine_relu(y, stats[0], stats[1], groups), z) < 1e-12
    s1, s2 = R.bn_bwd_sums(dz, y, stats, groups)
    assert rel_err(s1.sum(0), db) < 1e-12 and rel_err(s2.sum(0), dg) < 1e-12
    dy = R.bn_dy(dz, y, stats, torch.stack([s1, s2], -1) / (n * H * W), groups)
    assert rel_err(R.conv1_dgrad(dy, w), dx) < 1e-12
    assert rel_err(R.conv_wgrad(x[..., None], None, dy), dw) < 1e-12
    # coef None: nothing subtracted (eval mode); float32 is the same code
    assert torch.equal(R.bn_dy(dz, y, stats, None, groups), R.bn_dy(dz, y, stats, torch.zeros(groups, C, 2), groups))
    assert R.conv1(x, w, b, dtype=torch.float32).dtype == torch.float32 and R.conv1_dgrad(dy, w, dtype=torch.float32).dtype == torch.float32
