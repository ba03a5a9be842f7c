"""Cases and comparison functions shared by tests/test_host_reg_ref64.py and tests/test_gpu_registration_fp64.py.

A *backend* runs the registration entry points (the HIP library on the GPU; RefBackend = tests/reg_ref64.py in float32, with or
without a seeded defect, on the host).  The check_* functions below drive a backend through the linearised Adam step
(beta1 = beta2 = 0, eps = 2^20, lr = rho eps: p -= rho g / (1 + |g| / eps)), evaluate the float64 reference and the float32
yardstick AT THE SAME POINTS as the backend, and return records (name, value, bound).  hold() asserts value <= bound.

Bounds (none is taken from the code under test):
  bound = max(3 e32, floor); e32 = the same metric of the float32 yardstick against float64; floor = 8 fp32 ulps (2^-23) of the
  quantity's largest reference magnitude (the final fp32 store, the subtraction of two read-backs).
  Dense gradient fields: relative L2 error and the 90th percentile of |x - ref| / max|ref|, every pixel counted; the maximum is
  held to the reference's largest kink jump.  A sample within NEAR_PX of a cell boundary in float64 can be evaluated on the other
  side of the bilinear kink by ANY fp32 evaluation; its derivative then differs by the second difference of the sampled field.
  One such pixel at the final warp moves the relative L2 error by 1e-3 .. 1e-2 on these shapes, far above fp32 round-off.  The
  dense bounds carry NO allowance for that.  Instead the second-step cases are chosen (find_two_step_seed) so that the float64
  reference keeps every sample of the stages listed in TWO_STEP_CLEAR_FROM clear of a boundary: all eleven stages where a seed
  allows it, the final warp (where a flip weighs most) on the two largest.  On an odd extent the centre line of the early compositions sits d_i px from a boundary by construction (d_0 =
  flow / 2^10) and cannot be cleared; a flip at composition i reaches the flow's gradient scaled by 2^(i-10), and the yardstick
  meets those flips as the device does.
  Affine sums: bound + the sum over near-boundary samples of |gl| |second difference| (n / 2) max(|xb|, |yb|, 1)."""
import math

import numpy as np
import torch

from tests import reg_ref64 as R

F32, F64 = torch.float32, torch.float64
ULP = 2.0 ** -23
EPS = 2.0 ** 20                 # the linearising epsilon
NEAR_PX = 1e-4                  # a float64 sample this close to a cell boundary may flip sides in fp32
THRESH_MARGIN = 1e-5
DEFAULT_ADAM = dict(lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8)

AFFINE_SHAPES = [(1, 5, 7), (3, 37, 52), (2, 32, 32), (5, 33, 31), (1, 64, 96)]
AFFINE_GRIDS = ["scaled", "nonuniform", "outside", "halfcolumn"]       # + "library": loss and default path only (all on kinks)
DEMONS_SHAPES = [(1, 9, 11), (2, 24, 40), (3, 33, 65), (1, 64, 64), (1, 260, 256), (7, 16, 16)]
DEMONS_TWO_STEP = [(1, 9, 11), (2, 24, 40), (3, 33, 65), (1, 64, 64), (7, 16, 16)]
# (ksize, shape): random, asymmetric, not normalised; 17 on the 9 x 11 image is a halo wider than the image
SMOOTH_CASES = [(3, (2, 24, 40)), (9, (3, 33, 65)), (17, (1, 9, 11)), (17, (3, 33, 65)), (9, (1, 64, 64))]


# ------------------------------------------------------------------------------------------------------------------ inputs
def gaussian_kernel_2d(sigma=2.0):
    """GaussianRegulariser's kernel (net/registration.py:14-49): 2 ceil(2 sigma) + 1 taps, outer product, renormalised"""
    n = int(2 * np.ceil(sigma * 2) + 1)
    x = np.linspace(-(n - 1) // 2, (n - 1) // 2, num=n)
    k = np.exp(-(x ** 2) / (2 * sigma ** 2))
    k = np.tensordot(k / k.sum(), k / k.sum(), 0)
    return torch.tensor(k / k.sum(), dtype=F32)


def random_kernel(K, seed):
    """asymmetric, not normalised; the 9-tap one has negative taps"""
    g = torch.Generator().manual_seed(900 + seed + K)
    k = torch.rand(K, K, generator=g) / K
    if K == 9:
        k = k - 0.3 / K
    return k.float()


def _blur(x, sigma):
    r = int(3 * sigma)
    k = torch.exp(-torch.arange(-r, r + 1, dtype=F64) ** 2 / (2 * sigma ** 2))
    k = k / k.sum()
    x = torch.nn.functional.pad(x.double()[:, None], (r, r, r, r), mode="replicate")
    x = torch.nn.functional.conv2d(x, k[None, None, :, None])
    return torch.nn.functional.conv2d(x, k[None, None, None, :])[:, 0]


def image_pair(shape, seed, kind="smooth"):
    """(moving, fixed) [S, H, W] fp32 in [0, 1]; fixed = a shifted and sheared copy of moving plus a little noise.
    kind: "smooth" (random field blurred with sigma 3 px), "raw" (unblurred), "synth" (rpnet_amd.utils.synth, square only)"""
    S, H, W = shape
    g = torch.Generator().manual_seed(seed)
    if kind == "synth":
        from rpnet_amd.utils.synth import make_episode
        ep = make_episode(seed, S, H)
        mov = torch.from_numpy((ep["support_images"][0][0][:, 0] + 1) / 2).float()
        fix = torch.from_numpy((ep["query_images"][:, 0] + 1) / 2).float()
        return mov.contiguous(), fix.contiguous()
    big = torch.rand(S, H + 8, W + 8, generator=g, dtype=F64)
    if kind == "smooth":
        big = _blur(big, 3.0)
        lo, hi = big.amin(dim=(1, 2), keepdim=True), big.amax(dim=(1, 2), keepdim=True)
        big = (big - lo) / (hi - lo)
    mov = big[:, 4:4 + H, 4:4 + W]
    # the copy: 1.5 px down, 1 px left, sheared by a pixel over the height
    yy, xx = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    px, py = xx + 4 + 1.0 + (yy / H - 0.5), yy + 4 - 1.5
    gx, gy = (2 * px + 1) / (W + 8) - 1, (2 * py + 1) / (H + 8) - 1
    fix = torch.nn.functional.grid_sample(big[:, None], torch.stack([gx, gy], -1)[None].expand(S, -1, -1, -1), align_corners=False)[:, 0]
    fix = (fix + 0.02 * torch.rand(S, H, W, generator=g, dtype=F64)).clamp(0, 1)
    return mov.float().contiguous(), fix.float().contiguous()


def library_grid(n):
    """the base grid of F.affine_grid(align_corners=False) as the library takes it"""
    return (torch.linspace(-1, 1, n) * (n - 1) / n).float()


def base_grids(kind, H, W, nudge=0):
    """(xs [W], ys [H]) fp32.  `nudge` moves a grid by multiples of 1e-3 of its offsets: the host test picks, per case, the
    smallest one at which the kink conditions hold (AFFINE_NUDGE)."""
    x, y, e = library_grid(W).double(), library_grid(H).double(), 1e-3 * nudge
    if kind == "library":
        xs, ys = x, y
    elif kind == "scaled":
        xs, ys = 0.93 * x + 0.021 + e, 1.04 * y - 0.033 - e
    elif kind == "nonuniform":
        xs, ys = x + 0.04 * torch.sin(3 * x + 0.4 + e), y + 0.05 * torch.sin(2 * y - 0.7 - e)
    elif kind == "outside":                      # a band of samples beyond the image on every side
        xs, ys = 1.3 * x + 0.013 + e, 1.3 * y - 0.017 - e
    elif kind == "halfcolumn":                   # column 0 sits at x0 = -1 (ix = -0.45): its right corner inside, its left outside
        xs, ys = x - (0.9 + e) / W, y + (0.41 + e) / H
    else:
        raise KeyError(kind)
    return xs.float().contiguous(), ys.float().contiguous()


# per (shape, grid): the nudge at which the iters=1 and iters=2 samples of the float64 reference keep clear of every cell boundary
# (chosen on the CPU by find_affine_nudge below; default 0)
AFFINE_NUDGE = {((2, 32, 32), "scaled"): 2, ((2, 32, 32), "nonuniform"): 3, ((5, 33, 31), "scaled"): 28,
                ((5, 33, 31), "nonuniform"): 11, ((5, 33, 31), "outside"): 10, ((5, 33, 31), "halfcolumn"): 25}
AFFINE_SEED = {((5, 33, 31), "nonuniform"): 1}
# the search keeps SEARCH_PX clear, the tests assert NEAR_PX: the device's theta1 / flow1 differ from the float32 reference's by rounding
SEARCH_PX = 1.5e-4
# cases too large for that carry the allowance instead; it must stay zero for these
AFFINE_KINK_FREE = [(1, 5, 7), (2, 32, 32), (5, 33, 31)]


# per shape: the first stage (0 .. 9 = compositions, 10 = the final warp) from which on no sample at flow1 lies within NEAR_PX
# of a cell boundary in the float64 reference, and the seed find_two_step_seed chose for that (default 0)
# (all eleven stages on 2 x 24 x 40 and 7 x 16 x 16; 1 x 64 x 64 and 3 x 33 x 65 have too many samples for more than the final warp,
# where a flip weighs most: no seed below 2500 / 600 clears an earlier stage as well)
TWO_STEP_SEED = {(1, 9, 11): 22, (3, 33, 65): 10, (1, 64, 64): 32}
TWO_STEP_CLEAR_FROM = {(1, 9, 11): 4, (2, 24, 40): 0, (3, 33, 65): 10, (1, 64, 64): 10, (7, 16, 16): 0}


def pow2_near(x):
    return 2.0 ** round(math.log2(float(x)))


# ------------------------------------------------------------------------------------------------------------------ backend
class RefBackend:
    """the entry points' semantics from tests/reg_ref64.py in `dtype`, optionally with one seeded defect"""

    def __init__(self, dtype=F32, defect=None):
        self.dtype, self.defect = dtype, defect

    def affine_register(self, mov, fix, xs, ys, iters, lr, beta1, beta2, eps):
        S = mov.shape[0]
        theta = torch.tensor([[1.0, 0, 0], [0, 1.0, 0]], dtype=self.dtype).repeat(S, 1, 1)
        state, loss = {}, torch.zeros(S, dtype=self.dtype)
        for it in range(1, iters + 1):
            loss, g = R.affine_loss_grad(mov, fix, theta, xs, ys, self.dtype, self.defect)
            theta = R.adam_step(theta, g, state, it, lr, beta1, beta2, eps)
        return theta, loss

    def demons_register(self, mov, fix, kern, iters, lr, beta1, beta2, eps):
        S, H, W = mov.shape
        flow = torch.zeros(S, 2, H, W, dtype=self.dtype)
        state, loss = {}, torch.zeros(S, dtype=self.dtype)
        for it in range(1, iters + 1):
            loss, g = R.ncc_loss_grad(mov, fix, flow, self.dtype, self.defect)
            flow = R.xcorr2d(R.adam_step(flow, g, state, it, lr, beta1, beta2, eps), kern, self.dtype, self.defect)
        return flow, R.diffeomorphic(flow, self.dtype), loss

    def affine_warp(self, x, theta, xs, ys, threshold=-1.0, scale=1.0, shift=0.0):
        return R.affine_warp(x, theta, xs, ys, threshold, scale, shift, self.dtype)

    def identity_grid_warp(self, x, threshold=-1.0, scale=1.0, shift=0.0):
        return R.identity_grid_warp(x, threshold, scale, shift, self.dtype)

    def displacement_warp(self, x, disp, threshold=-1.0, scale=1.0, shift=0.0):
        return R.displacement_warp(x, disp, threshold, scale, shift, self.dtype)


# ------------------------------------------------------------------------------------------------------------------ metrics
def bound(e32, magnitude):
    return max(3.0 * float(e32), 8 * ULP * float(magnitude))


def small_record(name, got, ref, yard, allowance=0.0):
    """largest absolute error of a small quantity (a loss, the six affine parameters)"""
    ref = ref.double()
    err, e32 = (got.double() - ref).abs().max().item(), (yard.double() - ref).abs().max().item()
    return (name, err, bound(e32, ref.abs().max()) + allowance)


def dense_records(name, got, ref, yard, jump):
    """relative L2, 90th percentile and maximum of a dense field; `jump` = the reference's largest kink jump (absolute)"""
    ref = ref.double()
    mag, nrm, n = ref.abs().max().item(), ref.norm().item(), ref.numel()

    def metrics(x):
        e = (x.double() - ref).abs().flatten()
        return e.norm().item() / nrm, torch.quantile(e, 0.9).item() / mag, e.max().item()

    (l2, p90, mx), (y_l2, y_p90, y_mx) = metrics(got), metrics(yard)
    floor_l2 = 8 * ULP * mag * math.sqrt(n) / nrm
    return [(name + " relL2", l2, max(3 * y_l2, floor_l2)),
            (name + " p90", p90, max(3 * y_p90, 8 * ULP)),
            (name + " max", mx, bound(y_mx, mag) + jump)]


def worst(records):
    """largest value / bound"""
    return max(v / b if b > 0 else (0.0 if v == 0 else math.inf) for _, v, b in records)


def hold(records, show=True):
    for name, v, b in records:
        if show:
            print(f"REG64 {name}: {v:.3e} <= {b:.3e} ({v / b if b > 0 else 0.0:.2f})")
    bad = [f"{name}: {v:.3e} > {b:.3e}" for name, v, b in records if not (math.isfinite(v) and v <= b)]
    assert not bad, "\n".join(bad)


def second_difference(x):
    """largest |second difference| of a field along x and along y (the jump of a bilinear derivative at a cell boundary)"""
    x = x.double()
    sx = (x[..., :, 2:] - 2 * x[..., :, 1:-1] + x[..., :, :-2]).abs().max().item() if x.shape[-1] > 2 else 0.0
    sy = (x[..., 2:, :] - 2 * x[..., 1:-1, :] + x[..., :-2, :]).abs().max().item() if x.shape[-2] > 2 else 0.0
    # at the image border the zero padding is the neighbour
    bx = max(x[..., :, 0].abs().max().item(), x[..., :, -1].abs().max().item())
    by = max(x[..., 0, :].abs().max().item(), x[..., -1, :].abs().max().item())
    return max(sx, bx), max(sy, by)


# ------------------------------------------------------------------------------------------------------------------ affine
def affine_allowance(mov, fix, theta, xs, ys):
    """(near-boundary sample count, allowance on d MSE / d theta) at theta, from the float64 reference alone"""
    S, H, W = mov.shape
    dx, dy = R.kink_report(H, W, theta=theta, xs=xs, ys=ys)["affine"]
    warped = R.affine_warp(mov, theta, xs, ys)
    gl = (2.0 / (H * W)) * (warped - fix.double()).abs()
    sdx, sdy = second_difference(mov)
    lever = max(xs.abs().max().item(), ys.abs().max().item(), 1.0)
    nx, ny = dx < NEAR_PX, dy < NEAR_PX
    allowance = (gl[nx].sum().item() * sdx * (W / 2) + gl[ny].sum().item() * sdy * (H / 2)) * lever
    return int(nx.sum() + ny.sum()), allowance


def affine_rho(mov, fix, xs, ys, target=0.08):
    _, g = R.affine_loss_grad(mov, fix, torch.tensor([[1.0, 0, 0], [0, 1.0, 0]]).repeat(mov.shape[0], 1, 1), xs, ys)
    return pow2_near(target / g.abs().max().item())


def _affine_step_records(tag, mov, fix, xs, ys, theta0, theta_got, loss_got, rho, compare_gradient=True, kink_free=False):
    """one linearised step from theta0 (fp32 values): the backend's theta and loss against float64, yardstick at the same point"""
    recs = []
    l64, g64 = R.affine_loss_grad(mov, fix, theta0, xs, ys)
    l32, g32 = R.affine_loss_grad(mov, fix, theta0, xs, ys, F32)
    recs.append(small_record(tag + " loss", loss_got, l64, l32))
    if compare_gradient:
        want = R.adam_step(theta0.double(), g64, {}, 1, rho * EPS, 0.0, 0.0, EPS)
        yard = R.adam_step(theta0.float(), g32, {}, 1, rho * EPS, 0.0, 0.0, EPS)
        near, allow = affine_allowance(mov, fix, theta0, xs, ys)
        if kink_free:
            assert near == 0, f"{tag}: {near} samples within {NEAR_PX} px of a cell boundary"
        recs.append(small_record(tag + " theta", theta_got, want, yard, rho * allow))
    return recs


def check_affine(backend, shape, grid, seed=None, kind="smooth"):
    """iters=1 and iters=2 of the linearised step on one (shape, base grid) -> records"""
    seed = AFFINE_SEED.get((shape, grid), 0) if seed is None else seed
    mov, fix = image_pair(shape, 100 + seed + sum(shape), kind)
    xs, ys = base_grids(grid, shape[1], shape[2], AFFINE_NUDGE.get((shape, grid), 0))
    tag = f"affine {shape} {grid}"
    ident = torch.tensor([[1.0, 0, 0], [0, 1.0, 0]]).repeat(shape[0], 1, 1)
    rho = affine_rho(mov, fix, xs, ys)
    args = (rho * EPS, 0.0, 0.0, EPS)
    th1, l1 = backend.affine_register(mov, fix, xs, ys, 1, *args)
    th2, l2 = backend.affine_register(mov, fix, xs, ys, 2, *args)
    lib = grid == "library"          # at the identity every sample of the library's grid sits on a kink: loss only; theta1 is generic
    free = shape in AFFINE_KINK_FREE and not lib
    recs = _affine_step_records(tag + " it1", mov, fix, xs, ys, ident, th1, l1, rho, not lib, free)
    # the backend's own theta1 is the evaluation point of step 2 (one launch's reduction order is fixed: the same bits)
    recs += _affine_step_records(tag + " it2", mov, fix, xs, ys, th1.float(), th2, l2, rho, True, free)
    return recs


def check_affine_default_adam(backend, shape):
    """the default path on the library's grid: Adam's first step is lr g / (|g| + 1e-8), so EVERY component of every slice is the
    identity +- lr: none moves further than lr (4 ulps of 1 for the store), none falls short of it by more than lr 1e-8 / |g|
    = 1e-4 for |g| >= 1e-6 (the components of these cases are >= 7e-5 in the reference, one-sided derivatives included)"""
    mov, fix = image_pair(shape, 100 + sum(shape))
    xs, ys = library_grid(shape[2]), library_grid(shape[1])
    ident = torch.tensor([[1.0, 0, 0], [0, 1.0, 0]]).repeat(shape[0], 1, 1)
    th, loss = backend.affine_register(mov, fix, xs, ys, 1, **DEFAULT_ADAM)
    step, lr = (th.double() - ident.double()).abs(), DEFAULT_ADAM["lr"]
    l64, _ = R.affine_loss_grad(mov, fix, ident, xs, ys)
    l32, _ = R.affine_loss_grad(mov, fix, ident, xs, ys, F32)
    tag = f"affine {shape} default"
    return [(tag + " step beyond lr", max(step.max().item() - lr, 0.0), 4 * ULP),
            (tag + " step short of lr", max(lr - step.min().item(), 0.0), 1e-4 + 4 * ULP),
            small_record(tag + " loss", loss, l64, l32)]


# ------------------------------------------------------------------------------------------------------------------ demons
def _gl(mov, fix, flow):
    """|d NCC / d warped| of the float64 reference, largest value"""
    w = R.displacement_warp(mov, R.diffeomorphic(flow)).requires_grad_(True)
    (g,) = torch.autograd.grad(R.ncc(w, fix.double()).sum(), w)
    return g.abs().max().item()


def demons_kinks(mov, fix, flow, g64):
    """from the float64 reference alone: (per stage 0 .. 10 the number of samples within NEAR_PX of a cell boundary, the largest
    single jump of the flow's gradient).  The jump of the final warp is |gl| |second difference of moving| n / 2, carried back
    through the chain (d_0 = flow / 2^10 and ten steps that at most double: gain <= 1); that of a composition is
    |g| |second difference of d_10| n / 2 at the most.  Samples at distance exactly 0 are the centre line of an odd extent at
    flow = 0, which fp32 hits exactly as well."""
    S, H, W = mov.shape
    rep = R.kink_report(H, W, flow=flow)
    n2 = max(H, W) / 2
    j_warp = _gl(mov, fix, flow) * max(second_difference(mov)) * n2
    j_comp = g64.abs().max().item() * max(second_difference(R.diffeomorphic(flow))) * n2
    near = [0] * (R.SCALING + 1)
    for stage, (dx, dy) in rep.items():
        i = R.SCALING if stage == "warp" else int(stage[7:])
        near[i] = int(((dx < NEAR_PX) & (dx > 0)).sum() + ((dy < NEAR_PX) & (dy > 0)).sum())
    return near, max(j_warp, j_comp)


def demons_rho(g64, target=0.03):
    return pow2_near(target / g64.abs().max().item())


def check_demons_first_step(backend, shape, seed=0, kind="smooth", kernel=None):
    """iters=1: flow1 = xcorr2d(-rho g(0) / (1 + |g| / eps), K), loss = NCC(0), disp = diffeomorphic(flow1) -> records"""
    mov, fix = image_pair(shape, 200 + seed + sum(shape), kind)
    S, H, W = shape
    kern = torch.ones(1, 1) if kernel is None else kernel
    zero = torch.zeros(S, 2, H, W)
    l64, g64 = R.ncc_loss_grad(mov, fix, zero)
    l32, g32 = R.ncc_loss_grad(mov, fix, zero, F32)
    rho = demons_rho(g64)
    flow, disp, loss = backend.demons_register(mov, fix, kern, 1, rho * EPS, 0.0, 0.0, EPS)
    want = R.xcorr2d(R.adam_step(zero.double(), g64, {}, 1, rho * EPS, 0.0, 0.0, EPS), kern)
    yard = R.xcorr2d(R.adam_step(zero, g32, {}, 1, rho * EPS, 0.0, 0.0, EPS), kern, F32)
    near, jump = demons_kinks(mov, fix, zero, g64)
    assert sum(near) == 0, f"{shape}: {near} samples within {NEAR_PX} px of a cell boundary at flow = 0"
    tag = f"demons {shape} {kind} K={kern.shape[0]} it1"
    k1 = kern.abs().sum().item()
    recs = dense_records(tag + " flow", flow, want, yard, rho * jump * k1)
    recs.append(small_record(tag + " ncc", loss, l64, l32))
    recs += dense_records(tag + " disp", disp, R.diffeomorphic(flow), R.diffeomorphic(flow, F32), 0.0)
    return recs, flow


def check_smoothing_of_own_result(flow_k, flow_1, kern):
    """the backend's smoothed first step against xcorr2d of its own unsmoothed one (ksize = 1, weight 1): the gradient cancels,
    what is left is the fp32 summation of K^2 terms in sequence: K^2 2^-24 sum |k| max|in| (Higham 2002, eq. 3.5)"""
    want = R.xcorr2d(flow_1, kern)
    K = kern.shape[0]
    tol = K * K * 2.0 ** -24 * kern.abs().sum().item() * flow_1.abs().max().item() + 8 * ULP * want.abs().max().item()
    return [(f"smooth K={K} {tuple(flow_1.shape)} own", (flow_k.double() - want).abs().max().item(), tol)]


def _two_step_inputs(shape, seed):
    mov, fix = image_pair(shape, 200 + seed + sum(shape), "smooth")
    kern = gaussian_kernel_2d(2.0)
    _, g0 = R.ncc_loss_grad(mov, fix, torch.zeros(shape[0], 2, *shape[1:]))
    return mov, fix, kern, demons_rho(R.xcorr2d(g0, kern))                   # flow1 has magnitude ~0.03


def find_two_step_seed(shape, first, seeds=range(400), px=SEARCH_PX):
    """the search behind TWO_STEP_SEED: the first seed at which the float64 reference, at the float32 yardstick's flow1, keeps
    every sample of the stages first .. 10 further than `px` from a cell boundary (None if there is none among `seeds`)"""
    for seed in seeds:
        mov, fix, kern, rho = _two_step_inputs(shape, seed)
        flow1 = RefBackend(F32).demons_register(mov, fix, kern, 1, rho * EPS, 0.0, 0.0, EPS)[0]
        rep = R.kink_report(shape[1], shape[2], flow=flow1.float())
        stages = [f"compose{i}" for i in range(first, R.SCALING)] + ["warp"]
        if all(((rep[st][0] < px) & (rep[st][0] > 0)).sum() + ((rep[st][1] < px) & (rep[st][1] > 0)).sum() == 0 for st in stages):
            return seed
    return None


def find_affine_nudge(shape, grid, seed=0, nudges=range(60), px=SEARCH_PX):
    """the search behind AFFINE_NUDGE / AFFINE_SEED: the smallest nudge of the base grid at which the float64 reference keeps every
    sample further than `px` from a cell boundary at the identity and at the float32 yardstick's theta1"""
    mov, fix = image_pair(shape, 100 + seed + sum(shape))
    ident = torch.tensor([[1.0, 0, 0], [0, 1.0, 0]]).repeat(shape[0], 1, 1)
    for nudge in nudges:
        xs, ys = base_grids(grid, shape[1], shape[2], nudge)
        rho = affine_rho(mov, fix, xs, ys)
        th1, _ = RefBackend(F32).affine_register(mov, fix, xs, ys, 1, rho * EPS, 0.0, 0.0, EPS)
        if all(min(d.min().item() for d in R.kink_report(shape[1], shape[2], theta=t, xs=xs, ys=ys)["affine"]) >= px for t in (ident, th1)):
            return nudge
    return None


def check_demons_second_step(backend, shape, seed=None):
    """one call of two steps with the reference Gaussian handed in: flow2 against xcorr2d(flow1 - rho g64(flow1), K), flow1 read
    back from the backend's own iters=1 call -> records"""
    seed = TWO_STEP_SEED.get(shape, 0) if seed is None else seed
    mov, fix, kern, rho = _two_step_inputs(shape, seed)
    S, H, W = shape
    args = (rho * EPS, 0.0, 0.0, EPS)
    flow1, _, _ = backend.demons_register(mov, fix, kern, 1, *args)
    flow2, disp2, loss2 = backend.demons_register(mov, fix, kern, 2, *args)
    flow1 = flow1.float()
    l64, g64 = R.ncc_loss_grad(mov, fix, flow1)
    l32, g32 = R.ncc_loss_grad(mov, fix, flow1, F32)
    want = R.xcorr2d(R.adam_step(flow1.double(), g64, {}, 2, *args), kern)
    yard = R.xcorr2d(R.adam_step(flow1, g32, {}, 2, *args), kern, F32)
    near, jump = demons_kinks(mov, fix, flow1, g64)
    first = TWO_STEP_CLEAR_FROM[shape]
    assert sum(near[first:]) == 0, f"{shape}: {near} samples per stage within {NEAR_PX} px of a cell boundary (find_two_step_seed)"
    tag = f"demons {shape} it2"
    recs = dense_records(tag + " flow", flow2, want, yard, rho * jump)
    recs.append(small_record(tag + " ncc", loss2, l64, l32))
    recs += dense_records(tag + " disp", disp2, R.diffeomorphic(flow2), R.diffeomorphic(flow2, F32), 0.0)
    return recs


def check_demons_degenerate(backend, shape=(2, 24, 40)):
    """an all-zero moving image: the warped image is constant, so b = 0, C = 0, D = sqrt(1e-10), NCC = -0 / D and every term of the
    gradient multiplies a sampled zero: loss, flow and displacement are exactly zero in any precision.  A constant fixed image:
    a is the rounding residue of 0.6 - mean(0.6), the NCC and its gradient are residues held to the yardstick's own size.
    iters = 0 leaves the flow and the displacement zero, the loss unwritten and theta the identity."""
    S, H, W = shape
    mov, fix = image_pair(shape, 11)
    one, zero = torch.ones(1, 1), torch.zeros(S, 2, H, W)
    rho = 2.0 ** 10
    flow, disp, loss = backend.demons_register(torch.zeros_like(mov), fix, one, 1, rho * EPS, 0.0, 0.0, EPS)
    l64, g64 = R.ncc_loss_grad(torch.zeros_like(mov), fix, zero)
    assert l64.abs().max() == 0 and g64.abs().max() == 0
    recs = [("demons zero moving flow", flow.abs().max().item(), 0.0), ("demons zero moving disp", disp.abs().max().item(), 0.0),
            ("demons zero moving ncc", loss.abs().max().item(), 0.0)]
    cf = torch.full_like(fix, 0.6)
    flow, disp, loss = backend.demons_register(mov, cf, one, 1, rho * EPS, 0.0, 0.0, EPS)
    l32, g32 = R.ncc_loss_grad(mov, cf, zero, F32)
    assert torch.isfinite(flow).all() and torch.isfinite(loss).all()
    recs += [("demons constant fixed flow", flow.abs().max().item(), max(3 * g32.abs().max().item(), 1e-6) * rho),
             ("demons constant fixed ncc", loss.abs().max().item(), max(3 * l32.abs().max().item(), 8 * ULP))]
    flow, disp, loss = backend.demons_register(mov, fix, gaussian_kernel_2d(2.0), 0, **DEFAULT_ADAM)
    th, _ = backend.affine_register(mov, fix, library_grid(W), library_grid(H), 0, **DEFAULT_ADAM)
    ident = torch.tensor([[1.0, 0, 0], [0, 1.0, 0]]).repeat(S, 1, 1)
    recs += [("iters=0 flow", flow.abs().max().item(), 0.0), ("iters=0 disp", disp.abs().max().item(), 0.0),
             ("iters=0 theta", (th.double() - ident.double()).abs().max().item(), 0.0)]
    return recs, loss


# ------------------------------------------------------------------------------------------------------------------ warps
WARP_SHAPES = AFFINE_SHAPES + DEMONS_SHAPES
WARP_THETAS = {
    "rotate": [[0.9, 0.25, 0.03], [-0.22, 0.95, -0.02]],
    "zoom_out": [[1.4, 0.0, 0.1], [0.05, 1.5, -0.1]],
    "zoom_in": [[0.55, 0.02, 0.07], [-0.03, 0.6, 0.11]],
    "all_outside": [[1.0, 0.0, 2.25], [0.0, 1.0, 0.0]],         # a shift of a whole image width and an eighth: the output is `shift`
    "far_outside": [[1.0, 0.0, 1e12], [0.0, 1.0, -1e12]],       # beyond the range of an int: sample_cell's clamp
}
POSTS = [dict(), dict(scale=2.0, shift=-1.0), dict(threshold=0.1)]


def warp_displacement(shape, seed=0):
    """a smooth field of a pixel or two, with columns that put samples at ix = -1, W - 1, W exactly and far outside (1e12)"""
    S, H, W = shape
    g = torch.Generator().manual_seed(300 + seed + sum(shape))
    d = (_blur(torch.rand(S * 2, H, W, generator=g, dtype=F64), 2.0).reshape(S, 2, H, W) - 0.5) * (8.0 / max(H, W))
    gx = R.compute_grid(H, W)[0][0, 0]                        # [W]
    for col, ix in ((0, -1.0), (1 % W, W - 1.0), (2 % W, float(W))):
        d[:, 0, :, col] = (ix + 0.5) * 2 / W - 1 - gx[col]
    d[:, 0, :, 3 % W] = 1e12
    d[:, 1, 0, :] = -1e12
    return d.float().contiguous()


def warp_records(name, got, ref64, ref32, post, value64=None):
    """a warped image against float64.  threshold mode: pixels whose un-thresholded reference lies within THRESH_MARGIN of the
    threshold are left out (at most 0.5 % of the case, asserted), no flip may remain among the rest"""
    if post.get("threshold", -1.0) < 0:
        return [small_record(name, got, ref64, ref32)]
    clear = (value64 - R._f32(post["threshold"])).abs() >= THRESH_MARGIN
    assert (~clear).double().mean().item() <= 0.005, f"{name}: {(~clear).sum()} pixels within {THRESH_MARGIN} of the threshold"
    return [(name + " flips", float((got.double() != ref64)[clear].sum()), 0.0)]


def check_warps(backend, shape, seed=0):
    mov, _ = image_pair(shape, 400 + seed + sum(shape), "smooth")
    S, H, W = shape
    xs, ys = library_grid(W), library_grid(H)
    recs = []
    disp = warp_displacement(shape, seed)
    for post in POSTS:
        ptag = "thr" if "threshold" in post else ("scaled" if post else "plain")
        for tname, th in WARP_THETAS.items():
            theta = torch.tensor(th).repeat(S, 1, 1)
            recs += warp_records(f"affine_warp {shape} {tname} {ptag}", backend.affine_warp(mov, theta, xs, ys, **post),
                                 R.affine_warp(mov, theta, xs, ys, **post), R.affine_warp(mov, theta, xs, ys, dtype=F32, **post), post,
                                 R.affine_warp(mov, theta, xs, ys))
        recs += warp_records(f"identity_grid_warp {shape} {ptag}", backend.identity_grid_warp(mov, **post),
                             R.identity_grid_warp(mov, **post), R.identity_grid_warp(mov, dtype=F32, **post), post, R.identity_grid_warp(mov))
        recs += warp_records(f"displacement_warp {shape} {ptag}", backend.displacement_warp(mov, disp, **post),
                             R.displacement_warp(mov, disp, **post), R.displacement_warp(mov, disp, dtype=F32, **post), post,
                             R.displacement_warp(mov, disp))
    for tname in ("all_outside", "far_outside"):
        out = backend.affine_warp(mov, torch.tensor(WARP_THETAS[tname]).repeat(S, 1, 1), xs, ys, shift=-1.0)
        recs.append((f"affine_warp {shape} {tname} is the shift", (out.double() + 1).abs().max().item(), 0.0))
    return recs
