"""The registration kernels (csrc/registration.hip, csrc/demons.hip) against the float64 reference of tests/reg_ref64.py, one
gradient at a time: the six entry points through the C ABI (rpnet_amd.hip.call), so that the optimiser's scalars, the base grid
and the smoothing kernel can be chosen.  With beta1 = beta2 = 0, eps = 2^20 and lr = rho eps, Adam's update is
p -= rho g / (1 + |g| / eps): iters=1 returns the gradient at the start, iters=2 the gradient at the point the first step
chose, `loss` the objective there.  Cases, bounds and comparison functions are those of tests/reg_cases.py (its docstring
derives every bound; tests/test_host_reg_ref64.py runs them on the float32 yardstick and on five seeded defects).  Every check
prints `REG64 name: value <= bound (ratio)`.

Measured on an MI355X (value / bound, the largest of each family): affine loss 0.29, dense flow relative L2 0.33 (first step,
1.9e-5 against 5.7e-5 at 260 x 256), 0.15 (second step, 5.6e-7 against 3.7e-6 at 2 x 24 x 40), warps 0.33 (2.5e-6 against
7.6e-6 at 3 x 37 x 52), no threshold flip; 27 tests ran in 4 s.  Not measured yet: the warps on the seven further shapes, the
1e12 translation, the all-zero moving image, the default-Adam check on every component, the library grid's second-step gradient,
and the second step at the seeds of 1 x 9 x 11 and 3 x 33 x 65; their bounds rest on the float32 yardstick alone."""
import pytest
import torch

from tests import reg_cases as C
from tests import reg_ref64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPE, ARG, WORKSPACE = -1, -2, -3          # enum rpnet_status of include/rpnet_abi.h


@pytest.fixture(scope="module")
def gpu():
    """the backend of the shared checks: the six entry points through the C ABI (the ledger reads the calls here)"""
    class HipBackend:
        """the entry points of the library; host tensors in, host tensors out"""

        def __init__(self):
            from rpnet_amd import hip
            self.hip = hip
            hip.load()

        def _dv(self, *ts):
            return [t.to(DEV, torch.float32).contiguous() for t in ts]

        def affine_register(self, mov, fix, xs, ys, iters, lr, beta1, beta2, eps):
            mov, fix, xs, ys = self._dv(mov, fix, xs, ys)
            S, H, W = mov.shape
            theta, loss = torch.full((S, 2, 3), 7.0, device=DEV), torch.full((S,), 7.0, device=DEV)
            p = self.hip.ptr
            self.hip.call("rpnet_affine_register", p(mov), p(fix), p(xs), p(ys), p(theta), p(loss), S, H, W, iters, lr, beta1, beta2, eps)
            return theta.cpu(), loss.cpu()

        def demons_register(self, mov, fix, kern, iters, lr, beta1, beta2, eps):
            mov, fix, kern = self._dv(mov, fix, kern)
            S, H, W = mov.shape
            flow, disp = torch.full((S, 2, H, W), 7.0, device=DEV), torch.full((S, 2, H, W), 7.0, device=DEV)
            loss = torch.full((S,), 7.0, device=DEV)
            wb = self.hip.query("rpnet_demons_workspace_bytes", S, H, W)
            ws = torch.empty(wb, device=DEV, dtype=torch.uint8)
            p = self.hip.ptr
            self.hip.call("rpnet_demons_register", p(mov), p(fix), p(kern), kern.shape[0], p(flow), p(disp), p(loss), S, H, W, iters,
                          lr, beta1, beta2, eps, p(ws), wb)
            return flow.cpu(), disp.cpu(), loss.cpu()

        def affine_warp(self, x, theta, xs, ys, threshold=-1.0, scale=1.0, shift=0.0):
            x, theta, xs, ys = self._dv(x, theta, xs, ys)
            out, p = torch.full_like(x, 7.0), self.hip.ptr
            self.hip.call("rpnet_affine_warp", p(x), p(theta), p(xs), p(ys), p(out), *x.shape, threshold, scale, shift)
            return out.cpu()

        def identity_grid_warp(self, x, threshold=-1.0, scale=1.0, shift=0.0):
            (x,) = self._dv(x)
            out, p = torch.full_like(x, 7.0), self.hip.ptr
            self.hip.call("rpnet_identity_grid_warp", p(x), p(out), *x.shape, threshold, scale, shift)
            return out.cpu()

        def displacement_warp(self, x, disp, threshold=-1.0, scale=1.0, shift=0.0):
            x, disp = self._dv(x, disp)
            out, p = torch.full_like(x, 7.0), self.hip.ptr
            self.hip.call("rpnet_displacement_warp", p(x), p(disp), p(out), *x.shape, threshold, scale, shift)
            return out.cpu()

    return HipBackend()


# ================================================================================================================= affine stage
@pytest.mark.parametrize("shape", C.AFFINE_SHAPES)
def test_affine_gradient_and_loss(gpu, shape):
    """rpnet_affine_register, iters=1 and iters=2 of the linearised step on every base grid: loss against the float64 MSE, theta
    against the float64 step (max(3 e32, 8 ulps of 1) + the kink allowance, zero on the three kink-free shapes); the library's
    grid puts every sample on a kink at the identity, so its gradient is compared at the second step only; one unblurred pair on
    the larger shapes"""
    recs = []
    for grid in C.AFFINE_GRIDS + ["library"]:
        recs += C.check_affine(gpu, shape, grid)
    if shape not in C.AFFINE_KINK_FREE:
        recs += C.check_affine(gpu, shape, "scaled", kind="raw")
    C.hold(recs)


@pytest.mark.parametrize("shape", C.AFFINE_SHAPES)
def test_affine_default_adam_first_step(gpu, shape):
    """the default path (rpnet_affine_register, lr 0.01, betas 0.9 / 0.999, eps 1e-8, the library's grid): every component of every
    slice is the identity +- lr, and the loss is the float64 MSE"""
    C.hold(C.check_affine_default_adam(gpu, shape))


# ================================================================================================================= demons stage
@pytest.mark.parametrize("shape", C.DEMONS_SHAPES)
def test_demons_first_step(gpu, shape):
    """rpnet_demons_register, iters=1: ksize=1 with the kernel [[1.0]] returns -rho g(0) elementwise, NCC(0) and the
    displacement of that flow; with random asymmetric kernels (3, 9 with negative taps, 17; 17 on the 9 x 11 image) the same
    correlated with the kernel as handed in — against float64, and against xcorr2d of the device's own ksize=1 result"""
    recs, flow1 = C.check_demons_first_step(gpu, shape)
    for K, sh in C.SMOOTH_CASES:
        if sh == shape:
            kern = C.random_kernel(K, sum(shape))
            r, fk = C.check_demons_first_step(gpu, shape, kernel=kern)
            recs += r + C.check_smoothing_of_own_result(fk, flow1, kern)
    if shape == (1, 64, 64):
        recs += C.check_demons_first_step(gpu, shape, kind="synth")[0] + C.check_demons_first_step(gpu, shape, kind="raw")[0]
    C.hold(recs)


@pytest.mark.parametrize("shape", C.DEMONS_TWO_STEP)
def test_demons_second_step(gpu, shape):
    """one call of two steps with the reference Gaussian: flow2 against xcorr2d(flow1 - rho g64(flow1), K) at the device's own
    flow1 (magnitude ~0.03): the position-gradient terms and the scatter at a non-trivial field; relative L2 and the 90th
    percentile are held to max(3 e32, 8 ulps) with no allowance for a kink"""
    C.hold(C.check_demons_second_step(gpu, shape))


def test_demons_degenerate_inputs(gpu):
    """rpnet_demons_register on an all-zero moving image (C = 0, D = sqrt(1e-10): loss, flow and displacement exactly zero), on a
    constant fixed image (residues of the yardstick's size), and iters=0 of both stages (the loss is left unwritten)"""
    recs, loss = C.check_demons_degenerate(gpu)
    C.hold(recs)
    assert (loss == 7.0).all()


# ================================================================================================================= warps
@pytest.mark.parametrize("shape", C.WARP_SHAPES)
def test_warps(gpu, shape):
    """rpnet_affine_warp (rotation, zoom out, zoom in, all outside, 1e12 outside: the output is the shift),
    rpnet_identity_grid_warp, rpnet_displacement_warp (samples at -1, W - 1, W and 1e12) plain, scaled and shifted, and
    thresholded (no flip outside 1e-5 of the threshold), on every shape of both stages"""
    C.hold(C.check_warps(gpu, shape))


# ================================================================================================================= refusals
def test_registration_refusals(gpu):
    """the RPNET_REQUIRE lines of the six entry points and of rpnet_demons_workspace_bytes: return codes and the error string"""
    hip = gpu.hip
    lib = hip.load()
    t = torch.zeros(4096, device=DEV)
    p, st = t.data_ptr(), hip.stream()
    ad = (0.01, 0.9, 0.999, 1e-8)
    wb = hip.query("rpnet_demons_workspace_bytes", 1, 8, 8)
    assert wb > 0 and hip.query("rpnet_demons_workspace_bytes", 0, 8, 8) == 0 and hip.query("rpnet_demons_workspace_bytes", 1, 0, 8) == 0
    ws = torch.zeros(wb, device=DEV, dtype=torch.uint8)
    w = ws.data_ptr()
    cases = [
        (lib.rpnet_affine_register, (p, None, p, p, p, p, 1, 8, 8, 1, *ad), ARG),
        (lib.rpnet_affine_register, (p, p, p, p, None, p, 1, 8, 8, 1, *ad), ARG),
        (lib.rpnet_affine_register, (p, p, p, p, p, p, 1, 1, 8, 1, *ad), SHAPE),
        (lib.rpnet_affine_register, (p, p, p, p, p, p, -1, 8, 8, 1, *ad), SHAPE),
        (lib.rpnet_affine_register, (p, p, p, p, p, p, 1, 8, 8, -1, *ad), SHAPE),
        (lib.rpnet_affine_warp, (p, p, p, None, p, 1, 8, 8, -1.0, 1.0, 0.0), ARG),
        (lib.rpnet_affine_warp, (p, p, p, p, p, 1, 8, 1, -1.0, 1.0, 0.0), SHAPE),
        (lib.rpnet_identity_grid_warp, (None, p, 1, 8, 8, -1.0, 1.0, 0.0), ARG),
        (lib.rpnet_identity_grid_warp, (p, p, 1, 1, 8, -1.0, 1.0, 0.0), SHAPE),
        (lib.rpnet_displacement_warp, (p, None, p, 1, 8, 8, -1.0, 1.0, 0.0), ARG),
        (lib.rpnet_displacement_warp, (p, p, p, 1, 1, 8, -1.0, 1.0, 0.0), SHAPE),
        (lib.rpnet_demons_register, (p, p, None, 1, p, p, p, 1, 8, 8, 1, *ad, w, wb), ARG),
        (lib.rpnet_demons_register, (p, p, p, 1, p, p, p, 1, 8, 8, 1, *ad, None, wb), ARG),
        (lib.rpnet_demons_register, (p, p, p, 1, p, p, p, 1, 1, 8, 1, *ad, w, wb), SHAPE),
        (lib.rpnet_demons_register, (p, p, p, 2, p, p, p, 1, 8, 8, 1, *ad, w, wb), SHAPE),
        (lib.rpnet_demons_register, (p, p, p, 19, p, p, p, 1, 8, 8, 1, *ad, w, wb), SHAPE),
        (lib.rpnet_demons_register, (p, p, p, 0, p, p, p, 1, 8, 8, 1, *ad, w, wb), SHAPE),
        (lib.rpnet_demons_register, (p, p, p, 1, p, p, p, 1, 8, 8, 1, *ad, w, wb - 1), WORKSPACE),
    ]
    for fn, args, want in cases:
        got = fn(*args, st)
        assert got == want, f"{fn.__name__}{args}: rc {got}, expected {want}"
        assert lib.rpnet_last_error_string().decode() != ""
    # S = 0 succeeds and writes nothing
    out = torch.full((64,), 7.0, device=DEV)
    o = out.data_ptr()
    assert lib.rpnet_affine_register(p, p, p, p, o, o, 0, 8, 8, 1, *ad, st) == 0
    assert lib.rpnet_affine_warp(p, p, p, p, o, 0, 8, 8, -1.0, 1.0, 0.0, st) == 0
    assert lib.rpnet_identity_grid_warp(p, o, 0, 8, 8, -1.0, 1.0, 0.0, st) == 0
    assert lib.rpnet_displacement_warp(p, p, o, 0, 8, 8, -1.0, 1.0, 0.0, st) == 0
    assert lib.rpnet_demons_register(p, p, p, 1, o, o, o, 0, 8, 8, 1, *ad, w, wb, st) == 0
    torch.cuda.synchronize()
    assert (out == 7.0).all() and t.abs().max() == 0 and ws.max() == 0
