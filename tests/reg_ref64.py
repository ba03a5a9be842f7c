"""Plain float64 reference of the registration pre-step (csrc/registration.hip, csrc/demons.hip): stock torch operators on the
CPU, restated from the reference's operator sequence (net/registration.py:147-212,225-261,316-357, dataset/few_shot_reader.py:
109-198), every gradient through autograd.  Test infrastructure only: nothing here imports the package under test or oracle/
(tests/test_host_reg_ref64.py compares this file with oracle/registration_oracle.py).

Layouts are the kernels' own: images [S, H, W], theta [S, 2, 3], flow / displacement [S, 2, H, W] (channel 0 = x), the base grid
xs [W], ys [H] and the smoothing kernel [K, K] are inputs.  Every function takes `dtype`: float64 is the reference, float32 the
yardstick — the same operators at the kernels' precision.  `defect` is for the sensitivity test alone (test_host_reg_ref64.py:
a copy of the reference with one seeded fault must fail the comparisons of tests/reg_cases.py); None everywhere else."""
import math

import torch
import torch.nn.functional as F

F64 = torch.float64
SCALING = 10            # Diffeomorphic(10), net/registration.py:240
NCC_EPS = 1e-10         # net/registration.py:159
DEFECTS = ("wh_swap", "transposed_taps", "no_position_grad", "no_abb_term", "border_inside")


def _c(t, dtype):
    return None if t is None else torch.as_tensor(t).detach().cpu().to(dtype)


def _f32(v):
    """a C float argument as the kernel receives it"""
    return float(torch.tensor(v, dtype=torch.float32))


def _gscale(x, s):
    """x in value, s * d/dx in gradient"""
    return x * s + (x * (1.0 - s)).detach()


def _sample(img, gx, gy, defect=None):
    """F.grid_sample at its defaults (bilinear, zero padding, align_corners=False): img [S, C, H, W], gx / gy [S, H, W]"""
    if defect == "border_inside":
        # the corner just outside the image takes the edge pixel's value instead of zero: one ring of replicated pixels, the
        # coordinates mapped so that every sample keeps its pixel position; beyond that ring the padding is zero as before
        H, W = img.shape[-2:]
        img = F.pad(img, (1, 1, 1, 1), mode="replicate")
        gx, gy = ((gx + 1) * W + 2) / (W + 2) - 1, ((gy + 1) * H + 2) / (H + 2) - 1
    return F.grid_sample(img, torch.stack([gx, gy], dim=-1), mode="bilinear", padding_mode="zeros", align_corners=False)


def post(v, threshold=-1.0, scale=1.0, shift=0.0):
    """[threshold](v) * scale + shift; a negative threshold means none (few_shot_reader.py:168,172,190,196)"""
    if threshold >= 0:
        v = (v > _f32(threshold)).to(v.dtype)
    return v * _f32(scale) + _f32(shift)


# ------------------------------------------------------------------------------------------------------------ affine stage
def affine_coords(theta, xs, ys):
    """F.affine_grid on a given base grid: gx = t0 x + t1 y + t2, gy = t3 x + t4 y + t5 -> ([S, H, W], [S, H, W])"""
    t = theta.reshape(-1, 6)
    x, y = xs[None, None, :], ys[None, :, None]
    c = [t[:, k, None, None] for k in range(6)]
    return c[0] * x + c[1] * y + c[2], c[3] * x + c[4] * y + c[5]


def affine_loss_grad(moving, fixed, theta, xs, ys, dtype=F64, defect=None):
    """per slice: MSE(grid_sample(moving, grid(theta)), fixed) [S] and d MSE / d theta [S, 2, 3]; the base grid as given"""
    mov, fix, xs, ys = _c(moving, dtype), _c(fixed, dtype), _c(xs, dtype), _c(ys, dtype)
    theta = _c(theta, dtype).requires_grad_(True)
    H, W = mov.shape[-2:]
    gx, gy = affine_coords(theta, xs, ys)
    if defect == "wh_swap":
        gy = _gscale(gy, W / H)
    warped = _sample(mov[:, None], gx, gy, defect)[:, 0]
    loss = ((fix - warped) ** 2).mean(dim=(1, 2))
    (g,) = torch.autograd.grad(loss.sum(), theta)
    return loss.detach(), g


def affine_warp(x, theta, xs, ys, threshold=-1.0, scale=1.0, shift=0.0, dtype=F64):
    gx, gy = affine_coords(_c(theta, dtype), _c(xs, dtype), _c(ys, dtype))
    return post(_sample(_c(x, dtype)[:, None], gx, gy)[:, 0], threshold, scale, shift)


# ------------------------------------------------------------------------------------------------------------ demons stage
def compute_grid(H, W, dtype=F64):
    """compute_grid() (net/registration.py:171-187): 2 (j / (n - 1) - 0.5) -> (gx [1, H, W], gy [1, H, W])"""
    gx = 2 * (torch.arange(W, dtype=dtype) / (W - 1) - 0.5)
    gy = 2 * (torch.arange(H, dtype=dtype) / (H - 1) - 0.5)
    return gx[None, None, :].expand(1, H, W), gy[None, :, None].expand(1, H, W)


def identity_grid_warp(x, threshold=-1.0, scale=1.0, shift=0.0, dtype=F64):
    x = _c(x, dtype)
    gx, gy = compute_grid(*x.shape[-2:], dtype=dtype)
    S = x.shape[0]
    return post(_sample(x[:, None], gx.expand(S, -1, -1), gy.expand(S, -1, -1))[:, 0], threshold, scale, shift)


def _diffeo(flow, defect=None, keep=None):
    gx, gy = compute_grid(*flow.shape[-2:], dtype=flow.dtype)
    d = flow / (2 ** SCALING)
    for _ in range(SCALING):
        if keep is not None:
            keep.append(d.detach())
        at = d.detach() if defect == "no_position_grad" else d
        d = d + _sample(d, gx + at[:, 0], gy + at[:, 1], defect)
    return d


def diffeomorphic(flow, dtype=F64):
    """scaling and squaring: d_0 = flow / 2^10, d_{i+1} = d_i + grid_sample(d_i, grid + d_i), ten times"""
    return _diffeo(_c(flow, dtype))


def displacement_warp(x, disp, threshold=-1.0, scale=1.0, shift=0.0, dtype=F64):
    x, d = _c(x, dtype), _c(disp, dtype)
    gx, gy = compute_grid(*x.shape[-2:], dtype=dtype)
    return post(_sample(x[:, None], gx + d[:, 0], gy + d[:, 1])[:, 0], threshold, scale, shift)


def ncc(moving, fixed, defect=None):
    """-sum(a b) / sqrt(sum a^2 sum b^2 + 1e-10), a / b the centred fixed / moving image, per slice [S]"""
    a = fixed - fixed.mean(dim=(1, 2), keepdim=True)
    b = moving - moving.mean(dim=(1, 2), keepdim=True)
    bb = (b * b).sum(dim=(1, 2))
    if defect == "no_abb_term":
        bb = bb.detach()
    return -(a * b).sum(dim=(1, 2)) / torch.sqrt((a * a).sum(dim=(1, 2)) * bb + NCC_EPS)


def ncc_loss_grad(moving, fixed, flow, dtype=F64, defect=None):
    """NCC(grid_sample(moving, grid + diffeomorphic(flow)), fixed) [S] and its gradient by the flow [S, 2, H, W]"""
    mov, fix = _c(moving, dtype), _c(fixed, dtype)
    flow = _c(flow, dtype).requires_grad_(True)
    H, W = mov.shape[-2:]
    gx, gy = compute_grid(H, W, dtype)
    d = _diffeo(flow, defect)
    py = gy + d[:, 1]
    if defect == "wh_swap":
        py = _gscale(py, W / H)
    loss = ncc(_sample(mov[:, None], gx + d[:, 0], py, defect)[:, 0], fix, defect)
    (g,) = torch.autograd.grad(loss.sum(), flow)
    return loss.detach(), g


def xcorr2d(field, kernel, dtype=F64, defect=None):
    """conv2d with zero padding, per channel, no flip: out[y, x] = sum_uv k[u, v] in[y + u - r, x + v - r]; field [S, 2, H, W]"""
    f, k = _c(field, dtype), _c(kernel, dtype)
    if defect == "transposed_taps":
        k = k.t()
    S, C, H, W = f.shape
    return F.conv2d(f.reshape(S * C, 1, H, W), k[None, None], padding=k.shape[0] // 2).reshape(S, C, H, W)


# ------------------------------------------------------------------------------------------------------------ optimiser
def adam_step(p, g, state, it, lr, beta1, beta2, eps):
    """torch.optim.Adam's single-tensor update, step `it` (from 1), in the dtype of p: exp_avg.lerp_(g, 1 - b1);
    exp_avg_sq.mul_(b2).addcmul_(g, g, 1 - b2); denom = exp_avg_sq.sqrt() / sqrt(1 - b2^t) + eps;
    p.addcdiv_(exp_avg, denom, value=-lr / (1 - b1^t)).  `state` is {"m", "v"} (created as zeros when empty) and is updated.
    With beta1 = beta2 = 0 this is p - lr g / (|g| + eps) = p - (lr / eps) g / (1 + |g| / eps): linear in g for a large eps."""
    g = g.to(p.dtype)
    if not state:
        state["m"], state["v"] = torch.zeros_like(p), torch.zeros_like(p)
    m = state["m"] + (1.0 - beta1) * (g - state["m"])
    v = state["v"] * beta2 + (1.0 - beta2) * g * g
    state["m"], state["v"] = m, v
    step, bc2s = lr / (1.0 - beta1 ** it), math.sqrt(1.0 - beta2 ** it)
    return p - step * (m / (v.sqrt() / bc2s + eps))


# ------------------------------------------------------------------------------------------------------------ kinks
def _to_boundary(g, n):
    """pixel position of the normalised coordinate g on an axis of n pixels -> distance to the nearest cell boundary, px"""
    ix = (g + 1) * (n / 2) - 0.5
    fr = ix - torch.floor(ix)
    return torch.minimum(fr, 1 - fr)


def kink_report(H, W, theta=None, xs=None, ys=None, flow=None):
    """From float64 alone: for each sample of each bilinear stage the distance (px) of its position from the nearest cell
    boundary, where the interpolant's derivative jumps.  -> {stage: (dx [S, H, W], dy [S, H, W])}; stages: "affine" (given
    theta, xs, ys), "compose0" .. "compose9" and "warp" (given flow)."""
    out = {}
    if theta is not None:
        gx, gy = affine_coords(_c(theta, F64), _c(xs, F64), _c(ys, F64))
        out["affine"] = (_to_boundary(gx, W), _to_boundary(gy, H))
    if flow is not None:
        keep = []
        d = _diffeo(_c(flow, F64), keep=keep)
        gx, gy = compute_grid(H, W, F64)
        for i, di in enumerate(keep + [d]):
            out["warp" if i == SCALING else f"compose{i}"] = (_to_boundary(gx + di[:, 0], W), _to_boundary(gy + di[:, 1], H))
    return out
