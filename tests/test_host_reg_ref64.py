"""tests/reg_ref64.py and tests/reg_cases.py without a GPU: the float64 reference of the registration pre-step is pinned to
oracle/registration_oracle.py in float32, the linearised Adam step is what tests/test_gpu_registration_fp64.py takes it to be,
every committed case meets its kink and threshold conditions on the reference, the float32 yardstick passes the very comparison
functions the GPU tests use — and a copy of the reference with one seeded defect fails them by at least 10 x their bound."""
import math

import pytest
import torch

from tests import reg_cases as C
from tests import reg_ref64 as R

F32 = torch.float32
IDENT = torch.tensor([[1.0, 0, 0], [0, 1.0, 0]])


def test_reference_agrees_with_the_oracle_in_float32():
    """the same operators, the base grid formed by another expression: fp32 round-off on the warps, the displacement and the NCC
    (8 ulps of the largest value, and a sampling position that is off by 2 ulps of a coordinate of magnitude 1, n / 2 px each, on
    a slope of at most max|value| per px); one and two default-Adam steps of both stages within 4 ulps of a parameter of magnitude 1 / 8 ulps of the flow"""
    from oracle import registration_oracle as RO
    S, H, W = 2, 19, 23
    mov, fix = C.image_pair((S, H, W), 7)
    xs, ys = C.library_grid(W), C.library_grid(H)
    theta = torch.tensor([[0.9, 0.1, 0.05], [-0.08, 1.1, -0.02]]).repeat(S, 1, 1)
    grid_t = RO.compute_grid(H, W).permute(0, 2, 3, 1).contiguous()
    flow = 0.05 * (C.image_pair((S * 2, H, W), 8)[0].reshape(S, 2, H, W) - 0.5)
    tol = lambda x: (8 + max(H, W)) * C.ULP * x.abs().max().item()          # noqa: E731
    for s in range(S):
        m = mov[s][None, None]
        o = RO.affine_warp(m, theta[s][None])[0, 0]
        assert (R.affine_warp(mov, theta, xs, ys, dtype=F32)[s] - o).abs().max() <= tol(o)
        o = RO.identity_grid_warp(m)[0, 0]
        assert (R.identity_grid_warp(mov, dtype=F32)[s] - o).abs().max() <= tol(o)
        od = RO.diffeomorphic(flow[s][None], grid_t)
        assert (R.diffeomorphic(flow, F32)[s] - od[0]).abs().max() <= tol(od)
        o = RO.displacement_warp(m, od, grid_t)[0, 0]
        assert (R.displacement_warp(mov, od.expand(S, -1, -1, -1), dtype=F32)[s] - o).abs().max() <= tol(o)
        assert abs(R.ncc(mov, fix)[s].item() - RO.ncc(m, fix[s][None, None]).item()) <= 8 * C.ULP
    ref = C.RefBackend(F32)
    for iters in (1, 2):
        th, _ = ref.affine_register(mov, fix, xs, ys, iters, **C.DEFAULT_ADAM)
        fl, _, _ = ref.demons_register(mov, fix, C.gaussian_kernel_2d(2.0), iters, **C.DEFAULT_ADAM)
        for s in range(S):
            o = RO.affine_register(mov[s][None, None], fix[s][None, None], iters=iters)
            assert (th[s] - o[0]).abs().max() <= 4 * C.ULP, (iters, s)
            o = RO.demons_register(mov[s][None, None], fix[s][None, None], iters=iters)
            assert (fl[s] - o[0]).abs().max() <= tol(o), (iters, s)
    assert (C.gaussian_kernel_2d(2.0) - RO.gaussian_kernel_2d()).abs().max() <= 1e-9


def test_linearised_adam_step_returns_the_gradient():
    """beta = 0, lr = rho eps, eps = 2^20 in fp32 arithmetic: p - p' = rho g to a few ulps (4) of rho max|g|, also where g * g
    underflows in fp32 (|g| < 1e-23); |g| / eps stays below an ulp for the gradients of these cases (|g| < 0.3), beyond that the
    1 / (1 + |g| / eps) factor shows, which the float64 form keeps"""
    g = torch.tensor([0.3, -0.02, 1e-5, -1e-12, 1e-25, -3e-30, 0.0, -0.11], dtype=F32)
    rho = 2.0 ** -4
    p = torch.zeros_like(g)
    for it in (1, 2, 5):
        q = R.adam_step(p, g, {}, it, rho * C.EPS, 0.0, 0.0, C.EPS)
        assert q.dtype == F32 and (q + rho * g).abs().max() <= 4 * C.ULP * rho * 0.3
        small = g.abs() < 1e-20
        assert ((q + rho * g)[small].abs() <= 4 * C.ULP * rho * g[small].abs()).all()
    big = torch.tensor([7.5], dtype=F32)
    assert abs(R.adam_step(p[:1], big, {}, 1, rho * C.EPS, 0.0, 0.0, C.EPS).item() + rho * 7.5) > 20 * C.ULP * rho * 7.5
    q64 = R.adam_step(p.double(), g.double(), {}, 1, rho * C.EPS, 0.0, 0.0, C.EPS)
    assert torch.equal(q64, -rho * g.double() / (1 + g.double().abs() / C.EPS))
    # the general formula against torch.optim.Adam itself
    w = torch.nn.Parameter(torch.tensor([0.5, -1.5, 2.0], dtype=torch.float64))
    opt, state, mine = torch.optim.Adam([w], lr=0.01), {}, w.detach().clone()
    for it in (1, 2, 3):
        w.grad = torch.tensor([0.1 * it, -0.3, 1e-4], dtype=torch.float64)
        opt.step()
        mine = R.adam_step(mine, w.grad, state, it, 0.01, 0.9, 0.999, 1e-8)
        assert (mine - w.detach()).abs().max() < 1e-15


def test_xcorr2d_against_a_double_loop():
    g = torch.Generator().manual_seed(3)
    f = torch.rand(1, 2, 6, 7, generator=g, dtype=torch.float64)
    for K in (1, 3, 17):
        k = C.random_kernel(K, 1).double()
        r = K // 2
        want = torch.zeros_like(f)
        for y in range(6):
            for x in range(7):
                for u in range(K):
                    for v in range(K):
                        yy, xx = y + u - r, x + v - r
                        if 0 <= yy < 6 and 0 <= xx < 7:
                            want[0, :, y, x] += k[u, v] * f[0, :, yy, xx]
        assert (R.xcorr2d(f, k) - want).abs().max() < 1e-14
        assert K == 1 or (R.xcorr2d(f, k, defect="transposed_taps") - want).abs().max() > 1e-3


YARD = C.RefBackend(F32)


@pytest.mark.parametrize("shape", C.AFFINE_SHAPES)
def test_affine_cases_meet_their_conditions_and_the_yardstick_passes(shape, monkeypatch):
    """the float32 yardstick in the role of the device; the kink-free cases keep the search margin clear (asserted inside)"""
    monkeypatch.setattr(C, "NEAR_PX", C.SEARCH_PX)
    for grid in C.AFFINE_GRIDS + ["library"]:
        C.hold(C.check_affine(YARD, shape, grid), show=False)
    C.hold(C.check_affine(YARD, shape, "scaled", kind="raw"), show=False) if shape not in C.AFFINE_KINK_FREE else None
    C.hold(C.check_affine_default_adam(YARD, shape), show=False)


def test_degenerate_cases_on_the_yardstick():
    recs, loss = C.check_demons_degenerate(YARD)
    C.hold(recs, show=False)


def test_two_step_seeds_come_from_the_search():
    """the committed seeds are what find_two_step_seed returns (the two small shapes; the others are asserted inside the checks)"""
    for shape in ((1, 9, 11), (7, 16, 16)):
        assert C.find_two_step_seed(shape, C.TWO_STEP_CLEAR_FROM[shape]) == C.TWO_STEP_SEED.get(shape, 0)
    assert C.find_affine_nudge((2, 32, 32), "nonuniform") == C.AFFINE_NUDGE[((2, 32, 32), "nonuniform")]


def test_affine_allowance_is_zero_on_three_shapes():
    zero = 0
    for shape in C.AFFINE_SHAPES:
        tot = 0.0
        for grid in C.AFFINE_GRIDS:
            mov, fix = C.image_pair(shape, 100 + C.AFFINE_SEED.get((shape, grid), 0) + sum(shape))
            xs, ys = C.base_grids(grid, shape[1], shape[2], C.AFFINE_NUDGE.get((shape, grid), 0))
            rho = C.affine_rho(mov, fix, xs, ys)
            th1, _ = YARD.affine_register(mov, fix, xs, ys, 1, rho * C.EPS, 0.0, 0.0, C.EPS)
            assert 0.03 < (th1 - IDENT).abs().max() < 0.12          # the step moves theta by about 0.05 - 0.1
            tot += C.affine_allowance(mov, fix, IDENT.repeat(shape[0], 1, 1), xs, ys)[1] + C.affine_allowance(mov, fix, th1, xs, ys)[1]
        zero += tot == 0
        assert (tot == 0) == (shape in C.AFFINE_KINK_FREE), (shape, tot)
    assert zero >= 3


@pytest.mark.parametrize("shape", C.DEMONS_SHAPES)
def test_demons_cases_meet_their_conditions_and_the_yardstick_passes(shape, monkeypatch):
    monkeypatch.setattr(C, "NEAR_PX", C.SEARCH_PX)
    recs, flow1 = C.check_demons_first_step(YARD, shape)
    assert 0.015 <= flow1.abs().max() <= 0.06
    for K, sh in C.SMOOTH_CASES:
        if sh == shape:
            kern = C.random_kernel(K, sum(shape))
            assert (kern - kern.t()).abs().max() > 0.01 and (kern - kern.flip(0, 1)).abs().max() > 0.01
            r, fk = C.check_demons_first_step(YARD, shape, kernel=kern)
            recs += r + C.check_smoothing_of_own_result(fk, flow1, kern)
    if shape in C.DEMONS_TWO_STEP:
        recs += C.check_demons_second_step(YARD, shape)
    if shape == (1, 64, 64):
        recs += C.check_demons_first_step(YARD, shape, kind="synth")[0] + C.check_demons_first_step(YARD, shape, kind="raw")[0]
    C.hold(recs, show=False)
    assert any((C.random_kernel(K, 0) < 0).any() for K, _ in C.SMOOTH_CASES)


@pytest.mark.parametrize("shape", C.WARP_SHAPES)
def test_warp_cases_meet_their_threshold_margins(shape):
    C.hold(C.check_warps(YARD, shape), show=False)
    S, H, W = shape
    d = C.warp_displacement(shape)
    ix = (R.compute_grid(H, W)[0][0, 0] + d[0, 0, H - 1].double() + 1) * (W / 2) - 0.5
    assert (ix[:3] - torch.tensor([-1.0, W - 1.0, float(W)])).abs().max() < 1e-4 and ix[3] > 1e11


# which committed checks must catch which seeded defect
SENSITIVITY = {
    "wh_swap": [("affine", (3, 37, 52), "scaled"), ("affine", (1, 64, 96), "nonuniform"), ("first", (2, 24, 40)), ("second", (2, 24, 40))],
    "transposed_taps": [("smooth", 3, (2, 24, 40)), ("smooth", 9, (3, 33, 65)), ("smooth", 17, (1, 9, 11))],
    "no_position_grad": [("second", (2, 24, 40)), ("second", (1, 64, 64)), ("second", (7, 16, 16))],
    "no_abb_term": [("first", (1, 9, 11)), ("first", (2, 24, 40)), ("first", (1, 260, 256))],
    "border_inside": [("affine", (3, 37, 52), "outside"), ("affine", (1, 64, 96), "halfcolumn"), ("first", (7, 16, 16))],
}


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_a_seeded_defect_fails_the_committed_checks_tenfold(defect):
    """a copy of the reference (float32, like the device) with one defect through the shared comparison functions"""
    bad, ratios = C.RefBackend(F32, defect), []
    for what, *arg in SENSITIVITY[defect]:
        if what == "affine":
            recs = C.check_affine(bad, *arg)
        elif what == "first":
            recs = C.check_demons_first_step(bad, arg[0])[0]
        elif what == "second":
            recs = C.check_demons_second_step(bad, arg[0])
        else:
            K, shape = arg
            recs = C.check_demons_first_step(bad, shape, kernel=C.random_kernel(K, sum(shape)))[0]
        ratios.append(C.worst(recs))
    print(f"SENSITIVITY {defect}: " + ", ".join(f"{r:.3g}" for r in ratios))
    assert min(ratios) >= 10, (defect, ratios)
