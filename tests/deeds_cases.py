"""Cases, reference and comparison rule shared by tests/test_host_deeds.py and tests/test_gpu_deeds.py.

The reference is a torch restatement of DEEDSRegistration (net/registration.py:360-381,412-471; include/rpnet_deeds_abi.h), batched over
slices and parametrised by dtype: float64 is the reference, float32 the yardstick (it reproduces the reference's own float32 run on the
fixture, tests/test_host_deeds.py).  A *backend* runs the two entry points: the HIP library on the GPU, or RefBackend here on the host,
in float32, with or without a seeded defect.

Comparison rule (that of tests/reg_cases.py; nothing in a bound comes from the code under test):
    |backend - ref64| <= max(3 e32, 8 * 2^-23 * max|ref64|), the maximum over all elements, every element counted;
    e32 = the float32 restatement against float64 on the same inputs.
Thresholded outputs: a pixel whose float64 value lies within 1e-5 of the threshold is exempt, at most 0.1 % of a case's pixels may be
(asserted on the reference before the backend is looked at), no other pixel may differ."""
import math

import torch
import torch.nn.functional as F

from tests.reg_cases import THRESH_MARGIN, ULP, hold, image_pair, library_grid, small_record  # noqa: F401

F32, F64 = torch.float32, torch.float64
TILE = 8                        # grid points along a side of a block's tile for D <= 15 (csrc/deeds.hip deeds_plan)
MAX_EXEMPT = 0.001

DEF = (1, .1, 1, 0, .1, 10)                 # DEEDSRegistration.alpha: alpha3 = 0, the one-launch path
GEN = (1, .1, 1, .5, .1, 10)                # alpha3 != 0: both paths
ODD = (.7, .05, 1.3, .6, .2, 25)            # no value that is 0 or 1

# (S, H, W, G, D, R, alpha, mode)
CASES = [
    (1, 41, 37, 1, 15, 0.1, DEF, "nearest"),                    # one grid point
    (3, 41, 37, 2, 7, 0.1, GEN, "bilinear"),
    (1, 33, 65, TILE - 1, 15, 0.1, DEF, "bilinear"),
    (7, 16, 16, TILE, 5, 0.1, GEN, "nearest"),                  # one whole tile, G < H
    (1, 41, 37, TILE + 1, 15, 0.1, GEN, "nearest"),             # a second tile of one point
    (3, 33, 65, 2 * TILE + 2, 15, 0.1, DEF, "nearest"),         # three tiles a side, the last ragged
    (1, 33, 65, 2 * TILE + 2, 3, 0.25, ODD, "bilinear"),
    (1, 24, 40, TILE + 1, 1, 0.1, DEF, "nearest"),              # one displacement: pred = 0
    (1, 24, 40, 5, 31, 0.2, GEN, "bilinear"),                   # the widest plane: a tile of one point
    (1, 24, 40, 15, 17, 0.1, DEF, "nearest"),                   # D above 15: a tile of 7
    (1, 64, 64, 128, 15, 0.1, DEF, "nearest"),                  # the defaults, G > H
    (3, 41, 37, 2 * TILE + 2, 7, 1.5, DEF, "bilinear"),         # most samples outside the image
    (2, 41, 37, TILE + 1, 7, 1.5, ODD, "nearest"),
    (1, 33, 65, TILE + 1, 5, 0.1, (1, .1, 1, 0, .1, 0), "nearest"),     # alpha5 = 0: pred is the mean shift
    (1, 33, 65, TILE + 1, 5, 0.1, (1, .1, 1, .3, .1, 0), "bilinear"),
]
DEFECTS = ["max_for_min", "zero_pad", "one_average", "swap_xy", "softmax_sign", "drop_alpha3", "nearest_off_by_one", "seam"]


def case_id(case):
    S, H, W, G, D, R, alpha, mode = case
    return f"S{S}-{H}x{W}-G{G}-D{D}-R{R}-a3_{alpha[3]}-a5_{alpha[5]}-{mode}"


def case_inputs(case):
    S, H, W, G, D = case[:5]
    return image_pair((S, H, W), 700 + G + D + S, "smooth")


def f32(v):
    return float(torch.tensor(v, dtype=F32))


# --------------------------------------------------------------------------------------------------------------- restatement
def _sample(img, gx, gy, dtype):
    """F.grid_sample (bilinear, zeros, align_corners=False) of img [S,H,W] at (gx, gy) [S,...] -> [S,...]"""
    grid = torch.stack([gx, gy], -1).reshape(img.shape[0], 1, -1, 2)
    return F.grid_sample(img[:, None].to(dtype), grid.to(dtype), mode="bilinear", padding_mode="zeros", align_corners=False).reshape(gx.shape)


def _minconv(c, defect=None):
    """avg1(avg1(-max1(-pad1(c)))) over the last two axes of c [S, G*G, D, D]"""
    p = F.pad(c, (3, 3, 3, 3), mode="constant", value=0.0) if defect == "zero_pad" else F.pad(c, (3, 3, 3, 3), mode="replicate")
    m = F.max_pool2d(p, 3, stride=1) if defect == "max_for_min" else -F.max_pool2d(-p, 3, stride=1)
    a = F.avg_pool2d(m, 3, stride=1)
    return a[..., 1:-1, 1:-1] if defect == "one_average" else F.avg_pool2d(a, 3, stride=1)


def _meanfield(c, G, D, defect=None):
    """avg1(avg1(pad2(.))) over the grid plane of c [S, G*G, D, D] -> the same shape"""
    S = c.shape[0]
    cp = c.permute(0, 2, 3, 1).reshape(S, D * D, G, G)
    out = F.avg_pool2d(F.avg_pool2d(F.pad(cp, (2, 2, 2, 2), mode="replicate"), 3, stride=1), 3, stride=1)
    if defect == "seam":
        # a block that lacks the outermost halo column to its right: the last column of every tile takes x + 1 for x + 2
        w = torch.tensor([1.0, 2.0, 3.0, 2.0, 1.0], dtype=c.dtype) / 9
        idx = torch.arange(G)
        rows = torch.stack([(idx + k - 2).clamp(0, G - 1) for k in range(5)])                   # [5, G]
        cols = rows.clone()
        last = (idx % TILE == TILE - 1) & (idx + 2 <= G - 1)
        cols[4, last] = (idx + 1)[last]
        out = sum(w[a] * w[b] * cp[:, :, rows[a]][:, :, :, cols[b]] for a in range(5) for b in range(5))
    return out.permute(0, 2, 3, 1).reshape(S, G * G, D, D)


def deeds_ref(moving, fixed, G, D, R, alpha, dtype=F64, defect=None):
    """moving, fixed [S,H,W] fp32 -> (pred [S,G,G,2], cost [S,G*G,D*D]) in `dtype`; R and alpha are taken as float32 values"""
    S = moving.shape[0]
    a0, a1, a2, a3, a4, a5 = [f32(a) for a in alpha]
    gb, sb = library_grid(G).to(dtype), library_grid(D).to(dtype) * f32(R)
    gx, gy = gb[None, :].expand(G, G).reshape(-1), gb[:, None].expand(G, G).reshape(-1)                 # [G*G]
    sx, sy = sb[None, :].expand(D, D).reshape(-1), sb[:, None].expand(D, D).reshape(-1)                 # [D*D]
    if defect == "swap_xy":
        sx, sy = sy, sx
    mx, my = (gx[:, None] + sx[None, :]).expand(S, -1, -1), (gy[:, None] + sy[None, :]).expand(S, -1, -1)
    mov = _sample(moving, mx, my, dtype)                                                                # [S, G*G, D*D]
    fix = _sample(fixed, gx.expand(S, -1), gy.expand(S, -1), dtype)[:, :, None]
    dc = (a1 + a0 * (fix - mov) ** 2).reshape(S, G * G, D, D)
    first = _meanfield(_minconv(dc, defect), G, D, defect)
    cost = a4 + a2 * dc + (0.0 if defect == "drop_alpha3" else a3) * first
    cost = _meanfield(_minconv(cost, defect), G, D, defect).reshape(S, G * G, D * D)
    soft = F.softmax((a5 if defect == "softmax_sign" else -a5) * cost, 2)
    pred = torch.stack([(soft * sx).sum(2), (soft * sy).sum(2)], -1)
    return pred.reshape(S, G, G, 2), cost


def nearest_index(n_in, n_out, defect=None):
    """torch's legacy `nearest` rule: source index = min(floor(i * (float) n_in / n_out), n_in - 1), in float32"""
    scale = torch.tensor(n_in, dtype=F32) / torch.tensor(n_out, dtype=F32)
    idx = torch.floor(torch.arange(n_out, dtype=F32) * scale).long()
    if defect == "nearest_off_by_one":
        idx = idx + 1
    return idx.clamp(max=n_in - 1)


def sampling_grid(pred, H, W, mode, dtype=F64, defect=None):
    """(grid + pred) [S,G,G,2] brought to [S,H,W,2] as F.upsample(mode) does"""
    S, G = pred.shape[:2]
    gb = library_grid(G).to(dtype)
    grid = torch.stack([gb[None, :].expand(G, G), gb[:, None].expand(G, G)], -1)[None] + pred.to(dtype)
    if mode == "nearest":
        return grid[:, nearest_index(G, H, defect)][:, :, nearest_index(G, W, defect)]
    return F.interpolate(grid.permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)


def warp_ref(x, pred, mode, threshold=-1.0, scale=1.0, shift=0.0, dtype=F64, defect=None):
    """-> (out [S,H,W], the un-thresholded sample), both in `dtype`"""
    S, H, W = x.shape
    g = sampling_grid(pred, H, W, mode, dtype, defect)
    v = _sample(x, g[..., 0], g[..., 1], dtype)
    out = (v > f32(threshold)).to(dtype) if threshold >= 0 else v
    return out * f32(scale) + f32(shift), v


class RefBackend:
    """the entry points' semantics from the restatement in `dtype`, optionally with one seeded defect"""

    def __init__(self, dtype=F32, defect=None):
        self.dtype, self.defect = dtype, defect

    def register(self, moving, fixed, G, D, R, alpha):
        return deeds_ref(moving, fixed, G, D, R, alpha, self.dtype, self.defect)

    def warp(self, x, pred, mode, threshold=-1.0, scale=1.0, shift=0.0):
        return warp_ref(x, pred, mode, threshold, scale, shift, self.dtype, self.defect)[0]


# ------------------------------------------------------------------------------------------------------------------ checks
_REFERENCE = {}


def reference(case):
    """(moving, fixed, pred64, cost64, pred32, cost32) of a case, computed once and shared; read-only"""
    key = case_id(case)
    if key not in _REFERENCE:
        S, H, W, G, D, R, alpha, mode = case
        mov, fix = case_inputs(case)
        _REFERENCE[key] = (mov, fix) + deeds_ref(mov, fix, G, D, R, alpha, F64) + deeds_ref(mov, fix, G, D, R, alpha, F32)
    return _REFERENCE[key]


def label_of(x):
    """a 0 / 1 label image whose warped edges cross the 0.1 threshold"""
    return (x > x.mean()).float()


POSTS = [dict(), dict(scale=2.0, shift=-1.0), dict(threshold=0.1)]


def warp_records(name, got, x, pred, mode, post):
    """a warped image against the float64 restatement on the same pred (fp32 values)"""
    ref64, value64 = warp_ref(x, pred, mode, dtype=F64, **post)
    ref32, _ = warp_ref(x, pred, mode, dtype=F32, **post)
    if post.get("threshold", -1.0) < 0:
        return [small_record(name, got, ref64, ref32)]
    clear = (value64 - f32(post["threshold"])).abs() >= THRESH_MARGIN
    exempt = (~clear).double().mean().item()
    assert exempt <= MAX_EXEMPT, f"{name}: {(~clear).sum()} pixels within {THRESH_MARGIN} of the threshold"
    return [(name + " flips", float((got.double() != ref64)[clear].sum()), 0.0)]


def check_case(backend, case):
    """pred and cost of a case against float64, then the case's image and label warped by the reference's pred in the case's mode"""
    S, H, W, G, D, R, alpha, mode = case
    mov, fix, pred64, cost64, pred32, cost32 = reference(case)
    pred, cost = backend.register(mov, fix, G, D, R, alpha)
    tag = case_id(case)
    recs = [small_record(tag + " cost", cost, cost64, cost32), small_record(tag + " pred", pred, pred64, pred32)]
    given = pred64.float()
    recs += warp_records(tag + " warp", backend.warp(mov, given, mode, scale=2.0, shift=-1.0), mov, given, mode, POSTS[1])
    recs += warp_records(tag + " label", backend.warp(label_of(mov), given, mode, threshold=0.1), label_of(mov), given, mode, POSTS[2])
    return recs


WARP_SHAPES = [(1, 41, 37, 9), (3, 33, 65, 18), (2, 64, 64, 128), (2, 48, 48, 24), (1, 16, 16, 1), (1, 9, 11, 5)]      # S, H, W, G


def random_pred(S, G, seed, amplitude=0.08):
    g = torch.Generator().manual_seed(800 + seed + G)
    p = (torch.rand(S, G, G, 2, generator=g) - 0.5) * 2 * amplitude
    p[:, 0, :, 0] = 2.5         # a row of samples beyond the image
    return p.float().contiguous()


def check_warps(backend, shape, seed=0):
    S, H, W, G = shape
    x, _ = image_pair((S, H, W), 600 + seed + H + W, "smooth")
    pred = random_pred(S, G, seed)
    recs = []
    for mode in ("nearest", "bilinear"):
        for k, post in enumerate(POSTS):
            img = label_of(x) if "threshold" in post else x
            recs += warp_records(f"deeds_warp {shape} {mode} post{k}", backend.warp(img, pred, mode, **post), img, pred, mode, post)
    return recs


# ---------------------------------------------------------------------------------------------------------------- recovery
REC = dict(H=64, W=64, G=16, D=7, steps=1, px=(2, -1), border=4, alpha=(400.0, .1, 1, 0, .1, 200.0))     # px: the shift in steps, (x, y)


def recovery_pair():
    """a smooth image without a period (four waves of 9 to 19 pixels in four directions), and the same image moved by a whole number
    of displacement steps: with R = steps * D / W a step of the displacement plane is `steps` pixels, so moving(p + shift) == fixed(p)
    wherever both are inside.  The waves turn within the 5 x 5 grid points of the mean field, so that the valleys the minimum
    convolution leaves along each point's edge direction add up to a bowl around the shift."""
    H, W, st, (kx, ky) = REC["H"], REC["W"], REC["steps"], REC["px"]

    def f(x, y):
        return (0.5 + 0.11 * torch.sin(2 * math.pi * (0.9 * x + 0.45 * y) / 11.3 + 0.3) + 0.1 * torch.sin(2 * math.pi * (-0.5 * x + 0.85 * y) / 8.7 + 1.1)
                + 0.09 * torch.sin(2 * math.pi * (0.2 * x - 0.97 * y) / 14.9 + 2.0) + 0.08 * torch.sin(2 * math.pi * (0.7 * x - 0.7 * y) / 19.1 + 0.7))
    yy, xx = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    fixed = f(xx, yy)
    moving = f(xx - kx * st, yy - ky * st)
    R = REC["steps"] * REC["D"] / W
    return moving.float()[None].contiguous(), fixed.float()[None].contiguous(), R


def recovery_margin_needed():
    """softmax weights of the other D^2 - 1 displacements, each at most (D - 1) sqrt 2 steps away, must sum to less than half a step:
    (D^2 - 1) exp(-alpha5 m) (D - 1) sqrt 2 < 1 / 2"""
    D, a5 = REC["D"], REC["alpha"][5]
    return math.log(2 * (D * D - 1) * (D - 1) * math.sqrt(2)) / a5
