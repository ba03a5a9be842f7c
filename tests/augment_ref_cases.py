"""Cases, restatements and comparison functions shared by tests/test_host_augment_ref64.py and tests/test_gpu_augment_fp64.py: the
train-time augmentation of csrc/augment.hip (rpnet_slice_minmax, rpnet_augment_affine, rpnet_elastic_field, rpnet_elastic_apply) against
plain numpy restatements of the four entry points AS include/rpnet_abi.h WORDS THEM.  Nothing here comes from rpnet_amd.augment but the
draw helpers (draw_random_affine, draw_elastic, gaussian_weights and the two argument sets).

The contract at an exact tie is the header's pixel-space rule, not torch's normalised grid: the coordinate of the affine stage is
fma(m0, bx, fma(m1, by, m2)) + (W/2 - 1/2) in fp32, rounded half to even, inside iff 0 <= r <= n-1.  affine_sample of
rpnet_amd/utils/volume_reader.py normalises by 0.5 * W in fp32 and un-normalises again, which returns the same number on planes whose
extents are powers of two (16x16, 32x32, 32x64; tests/test_host_augment_ref64.py holds the two equal on every pixel there) and a
neighbouring fp32 number elsewhere (37x19, 64x48: up to hundreds of pixels of a tie case land on the other side).

A *backend* runs the four entry points on numpy arrays and returns a dict of numpy arrays: the HIP library (the GPU test: every output and
intermediate NaN-filled between GUARD sentinel elements, "guards" = sentinel elements that changed, "repeat" = elements whose bits differ
in a second call) or SimBackend, a float32 / float64 restatement in the kernels' own operation order, with or without a seeded defect.
The check_* functions drive a backend through one row and return records; hold() prints and asserts.  Neither test restates a bound.

Bounds, none of them measured on the code under test:
  slice_minmax    exact (by value: the sign of a zero minimum is not defined by fminf; NaN inputs are not defined by the header and
                  are left out).
  augment_affine  labels, and images of slices whose power law is off: bit for bit on every pixel for the EXACT maps (six dyadic numbers:
                  the fp32 and the fp64 coordinate are the same number, asserted on the CPU); for maps drawn by draw_random_affine,
                  equal outside the 1e-3 pixel band of tests/augment_cases.py, one of the candidates inside it, band <= 1 % of a slice.
                  Power law on: the device pow may differ from numpy's by a few fp64 units, which can flip the one fp32 rounding of v
                  (2^-24 on [0,1]); the round trip keeps that and v * 2 - 1 doubles it: |got - ref| <= 2^-22.
  elastic_field   the fp64 sums may differ by contraction only: |got - ref32| <= one fp32 ulp of |ref32|, ref32 the fp64 reference
                  rounded once; radius 0 with weight 1: bit for bit (float)(alpha * noise).  The fp64 intermediate of the axis-0 pass:
                  |tmp - ref| <= (2 radius + 1) 2^-52 max |noise| sum |w| (one rounding per multiply-add on either side).
  elastic_apply   mask equal on every pixel; image within one fp32 ulp of |ref32| per pixel, stage 2 referred to the backend's OWN
                  stage-1 result (an ulp of stage 1 is charged once); crafted cases with dyadic coordinates and pixel values: bit for bit."""
import math

import numpy as np
import torch

from rpnet_amd.augment import LABEL_TRANSFORM_ARGS, TRANSFORM_ARGS, draw_elastic, draw_random_affine, gaussian_weights
from tests import augment_cases as AC
from tests.corr_cases import ARG, SHAPE, Rec, hold  # noqa: F401

F32, F64 = np.float32, np.float64
GUARD = 64
IMAGE_BOUND = 2.0 ** -22
BAND_CAP = 0.01
TIE_SHARE = 0.5
BLOCK = 256                     # pixels per block of the four gather kernels
MINMAX_STRIDE = 1024            # threads of slice_minmax_kernel

# ------------------------------------------------------------------------------------------------------------------ tables
PLANES = [(1, 1), (1, 7), (5, 1), (3, 5),      # smallest, single row, single column
          (17, 15), (16, 16), (257, 1),        # HW = 255, 256, 257
          (33, 31), (32, 32), (41, 25),        # HW = 1023, 1024, 1025
          (37, 19), (32, 64), (64, 48)]        # an odd plane, a power of two (the host cross-check), the existing small size
ODD_PLANES = [(17, 15), (37, 19), (33, 31), (41, 25)]
POW2_PLANES = [(16, 16), (32, 32), (32, 64)]
PRODUCTION = (12, 256, 256)
S_VALUES = (1, 2, 3, 7)

# the inverse map about the centre, m00 m01 m02 m10 m11 m12: multiples of 1/4 of magnitude <= 2, and one far translation
EXACT_MAPS = {"id": (1, 0, 0, 0, 1, 0), "half_shift": (1, 0, .5, 0, 1, -.5), "flipx_q": (-1, 0, .25, 0, 1, 0), "rot90": (0, -1, 0, 1, 0, 0),
              "zoom2": (.5, 0, 0, 0, .5, 0), "shrink": (2, 0, 1.5, 0, 2, -2.5), "shear": (1, .5, 0, .25, 1, .5), "far": (1, 0, 1000, 0, 1, 0)}
MAP_NAMES = list(EXACT_MAPS)
# (S, index of the first slice's map; slice s takes map first + s): every map, every S and a table index that matters, on every plane
EXACT_FORMS = [(7, 0), (1, 7), (2, 3), (3, 5)]
PAIRS = ("both", "img", "lab")
EXACT_ROWS = [(p, S, first, PAIRS[(i + j) % 3]) for i, p in enumerate(PLANES) for j, (S, first) in enumerate(EXACT_FORMS)]
# the (map, plane) pairs that are there for their ties: at least TIE_SHARE of the pixels exactly on k + 1/2 (the host test asserts it)
TIE_CASES = ([("half_shift", p) for p in PLANES]
             + [("zoom2", p) for p in [(1, 7), (3, 5)] + ODD_PLANES]
             + [("shrink", p) for p in [(1, 1), (1, 7), (5, 1), (3, 5), (257, 1)] + ODD_PLANES]
             + [("shear", p) for p in [(5, 1), (3, 5), (257, 1)] + ODD_PLANES])      # the even planes have their ties from half_shift alone
BIG_S = (65535, 1, 3)           # blockIdx.y at its limit: 196 605 pixels

# (plane, S, seed, argument set): maps drawn by draw_random_affine; the seeds are those for which the fp64 coordinates alone keep the
# excluded band within BAND_CAP of every slice (tests/test_host_augment_ref64.py asserts it: change the seed, never the cap)
RANDOM_ROWS = [(p, S, seed, args) for p, S, seed in [((17, 15), 3, 4), ((37, 19), 7, 2), ((33, 31), 2, 3), ((41, 25), 3, 3)]
               for args in ("transform", "label")]
RANDOM_ARGS = {"transform": TRANSFORM_ARGS, "label": LABEL_TRANSFORM_ARGS}

IMAGE_CASES = ["gammas", "flag_zero", "flag_other", "min_is_minus_one", "near_minimum", "constant", "extremes_last", "all_fill"]
IMAGE_ROWS = [(c, p, PAIRS[(i + j) % 3] if c == "gammas" else "both") for i, c in enumerate(IMAGE_CASES)
              for j, p in enumerate([(37, 19), (41, 25), (3, 5)])]

MINMAX_KINDS = ["random", "extremes_last", "constant", "signed_zeros", "extremes_first"]
MINMAX_ROWS = [(p, S_VALUES[(i + j) % 4], k) for i, p in enumerate(PLANES) for j, k in enumerate(MINMAX_KINDS)]

# (plane, weights, noise, alpha); weights: ("one",) radius 0 weight 1, ("r1",) radius 1, ("gauss", sigma)
FIELD_ROWS = ([(p, ("one",), n, a) for p in [(1, 1), (3, 5), (17, 15), (41, 25)] for n, a in (("random", 1000.0), ("random", 1.0))]
              + [(p, ("r1",), n, 1.0) for p in [(1, 7), (5, 1), (37, 19), (16, 16)] for n in ("random", "impulses")]
              + [(p, ("gauss", 30), n, a) for p in [(3, 5), (1, 7), (37, 19)] for n, a in (("random", 1000.0), ("impulses", 1.0))]
              + [((41, 25), ("gauss", 2), n, a) for n, a in (("random", 1.0), ("random", 1000.0), ("impulses", 1000.0))]
              + [((257, 1), ("gauss", 2), "random", 1000.0), ((33, 31), ("gauss", 2), "impulses", 1.0)])

MINV = {"identity": (1, 0, 0, 0, 1, 0), "shift": (1, 0, 2, 0, 1, -1), "half": (1, 0, .5, 0, 1, .5), "partly_outside": (1, 0, -2.5, 0, 1, 1.25),
        "swap": (0, 1, 0, 1, 0, 0)}
FIELDS = ["zero", "plus_half", "minus_half", "ramp_top", "ramp_bottom", "dx_dy_differ"]
TRIPLES = ("both", "img", "mask")
# crafted: (plane, S, Minv name, field name, padding_value, triples): dyadic coordinates and pixel values, bit for bit
ELASTIC_CRAFTED = ([((17, 15), 1 + 2 * (i % 2), m, f, (-1.0, 0.25)[(i + j) % 2], "both")
                    for i, m in enumerate(["identity", "shift", "half", "partly_outside"]) for j, f in enumerate(FIELDS)]
                   + [(p, 3, "half", f, 0.25, t) for p, f, t in [((1, 1), "zero", "both"), ((1, 7), "plus_half", "img"), ((5, 1), "minus_half", "mask"),
                                                                 ((3, 5), "ramp_top", "both"), ((41, 25), "ramp_bottom", "both"),
                                                                 ((33, 31), "dx_dy_differ", "both"), ((16, 16), "dx_dy_differ", "img"),
                                                                 ((257, 1), "plus_half", "both"), ((37, 19), "ramp_top", "mask")]]
                   + [((37, 19), 1, "swap", "dx_dy_differ", -1.0, "both")])
# random: (plane, S, seed, padding_value, triples): Minv from draw_elastic, an fp32 field of magnitude up to 8
ELASTIC_RANDOM = [((17, 15), 1, 0, -1.0, "both"), ((37, 19), 3, 1, 0.25, "both"), ((41, 25), 3, 2, -1.0, "img"), ((33, 31), 1, 3, 0.25, "mask"),
                  ((64, 48), 3, 4, -1.0, "both"), ((3, 5), 3, 5, 0.25, "both"), ((32, 32), 1, 6, -1.0, "both")]


# ----------------------------------------------------------------------------------------------------------------- records
class ARec(Rec):
    def line(self):
        return f"PARITY augment {self.family} {self.what} err={self.err:.3e} bound={self.bound:.3e}"


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def exact(family, what, got, want):
    """elements whose fp32 bits differ (a NaN left in an output differs from every reference)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (family, what, got.shape, want.shape)
    return ARec(family, what, int((bits(got) != bits(want)).sum()), 0.0, 0.0, exact=True)


def by_value(family, what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (family, what, got.shape, want.shape)
    return ARec(family, what, int((~(got == want)).sum()), 0.0, 0.0, exact=True)


def count(family, what, n):
    return ARec(family, what, int(n), 0.0, 0.0, exact=True)


def within(family, what, err, bound):
    return ARec(family, what, err if math.isfinite(err) else math.inf, bound, bound)


def ulps(got, ref64):
    """largest |got - ref32| in fp32 ulps of |ref32|, ref32 the reference rounded once; inf for a value that is not finite"""
    got, ref32 = np.asarray(got, dtype=F32), np.asarray(ref64).astype(F32)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return math.inf
    return float((np.abs(got.astype(F64) - ref32.astype(F64)) / np.spacing(np.abs(ref32)).astype(F64)).max())


def common(fam, tag, res):
    return [count(fam, f"guard elements touched {tag}", res["guards"]), count(fam, f"elements that change in a second call {tag}", res["repeat"])]


def tag_of(plane, S):
    return f"{S}x{plane[0]}x{plane[1]}"


# ------------------------------------------------------------------------------------- the header's rules, restated in numpy
def ref_minmax(x):
    S = x.shape[0]
    flat = x.reshape(S, -1)
    return np.stack([flat.min(axis=1), flat.max(axis=1)], axis=1).astype(F32)


def fma32(a, b, c):
    """fmaf on fp32 arrays: the product of two fp32 numbers is exact in fp64"""
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def affine_coords32(params, H, W, centre_w_both=False):
    """(fy, fx) [S, H, W] fp32: fma(m0, bx, fma(m1, by, m2)) + (W/2 - 1/2), bx = x - W/2 + 1/2"""
    q = np.asarray(params, dtype=F32)[:, :, None, None]
    half = F32(0.5)
    x, y = np.arange(W, dtype=F32)[None, None, :], np.arange(H, dtype=F32)[None, :, None]
    Hc = W if centre_w_both else H
    bx, by = (x - half * F32(W)) + half, (y - half * F32(Hc)) + half
    bx, by = np.broadcast_to(bx, (1, H, W)), np.broadcast_to(by, (1, H, W))
    fx = fma32(q[:, 0], bx, fma32(q[:, 1], by, q[:, 2])) + (half * F32(W) - half)
    fy = fma32(q[:, 3], bx, fma32(q[:, 4], by, q[:, 5])) + (half * F32(Hc) - half)
    return fy.astype(F32), fx.astype(F32)


def affine_coords64(params, H, W):
    """the same coordinates in fp64 from the fp32 table: what the EXACT maps must equal"""
    return np.stack([np.stack(AC.affine_source(q[:6], H, W)) for q in np.asarray(params, dtype=F32)]).transpose(1, 0, 2, 3)


def power_law(u, lo, hi, gamma, pow_fn=np.power, eps=1e-5, round_trip=True):
    """the law in fp64 rounded once to fp32, then the host's fp32 round trip between its two functions"""
    u, lo, hi, gamma = (np.asarray(a, dtype=F32).astype(F64) for a in (u, lo, hi, gamma))
    span = hi - lo + 1e-5
    v = (span * pow_fn(((u - lo) + eps) / span, gamma) + lo).astype(F32)
    return ((v * F32(2) - F32(1)) + F32(1)) / F32(2) if round_trip else v


def ref_affine(img, lab, params, mm, H, W, defect=None, pow_fn=np.power):
    """-> (img_out, lab_out), None for an absent pair; `defect` and `pow_fn` are SimBackend's"""
    params = np.asarray(params, dtype=F32)
    S = params.shape[0]
    q = np.broadcast_to(params[:1], params.shape) if defect == "params_slice0" else params
    fy, fx = affine_coords32(q, H, W, defect == "centre_w_both")
    rnd = (lambda c: np.floor(c + F32(0.5))) if defect == "affine_half_up" else np.rint
    ry, rx = rnd(fy), rnd(fx)
    if defect == "inside_lt":
        inside = (rx >= 0) & (rx < W - 1) & (ry >= 0) & (ry < H - 1)
    else:
        inside = (rx >= 0) & (rx <= W - 1) & (ry >= 0) & (ry <= H - 1)
    iy, ix = np.where(inside, ry, 0).astype(np.int64), np.where(inside, rx, 0).astype(np.int64)
    s = np.arange(S)[:, None, None]
    lab_out = img_out = None
    if lab is not None:
        lab_out = np.where(inside, lab[s, iy, ix], F32(0)).astype(F32)
    if img is not None and S:
        m = np.broadcast_to(mm[:1], mm.shape) if defect == "mm_slice0" else mm
        lo_u = ((m[:, 0].astype(F32) + F32(1)) / F32(2))[:, None, None]
        hi_u = ((m[:, 1].astype(F32) + F32(1)) / F32(2))[:, None, None]
        g = ((q[:, 7] == 1) if defect == "flag_eq_1" else (q[:, 7] != 0))[:, None, None]
        gamma = np.where(g, q[:, 6][:, None, None], F32(1))
        kw = dict(pow_fn=pow_fn, eps=0.0 if defect == "law_without_1e5" else 1e-5, round_trip=defect != "no_round_trip")
        lo = lo_u if defect == "lo_without_law" else np.where(g, power_law(lo_u, lo_u, hi_u, gamma, **kw), lo_u)
        v = (img[s, iy, ix].astype(F32) + F32(1)) / F32(2)
        v = np.where(g, power_law(v, lo_u, hi_u, gamma, **kw), v)
        v = np.where(inside, v, F32(0))
        v = np.where(v == 0, lo, v).astype(F32)
        img_out = v * F32(2) - F32(1)
    if defect == "last_block_unwritten" and (H * W) % BLOCK:
        for o in (img_out, lab_out):
            if o is not None:
                o.reshape(S, -1)[:, (H * W) // BLOCK * BLOCK:] = np.nan
    return img_out, lab_out


def reflect(i, n, defect=None):
    """index of the reflect extension (d c b a | a b c d | d c b a), period 2n"""
    if defect == "reflect_period_n":
        return i % n
    if defect == "reflect_mirror":
        if n == 1:
            return i * 0
        i = i % (2 * n - 2)
        return np.where(i < n, i, 2 * n - 2 - i)
    i = i % (2 * n)
    return np.where(i < n, i, 2 * n - 1 - i)


def blur_axis(a, w, radius, axis, defect=None, acc_type=F64):
    """sum_t w[t] a[.. reflect(i + t - r) ..] along `axis` of [2, H, W], ascending t"""
    n = a.shape[axis]
    acc = np.zeros(a.shape, dtype=acc_type)
    for t in range(-radius, radius + 1):
        acc = acc + acc_type(w[t + radius]) * np.take(a, reflect(np.arange(n) + t, n, defect), axis=axis).astype(acc_type)
    return acc.astype(F64)


def ref_field(noise, w, radius, alpha, defect=None, acc_type=F64):
    """-> (tmp [2, H, W] fp64, field [2, H, W] fp32): axis 0 (y) then axis 1 (x), times alpha, rounded once"""
    tmp = blur_axis(noise, w, radius, 1, defect, acc_type)
    out = blur_axis(tmp, w, radius, 1 if defect == "blur_same_axis" else 2, defect, acc_type)
    return tmp, (out * F64(alpha)).astype(F32)


def bilinear_const(p, cy, cx, cval, blend=False, wide=F64):
    """p [S, H, W] at fp64 (cy, cx) [H, W]: scipy's mode constant, a coordinate outside [0, n-1] gives cval without blending -> fp64.
    blend (a defect): the constant is blended in up to one pixel outside, as grid_sample's zero padding does"""
    S, H, W = p.shape
    fy, fx = np.floor(cy), np.floor(cx)
    wy, wx = (cy - fy).astype(wide), (cx - fx).astype(wide)
    y0, x0 = fy.astype(np.int64), fx.astype(np.int64)

    def tap(iy, ix):
        ok = (iy >= 0) & (iy <= H - 1) & (ix >= 0) & (ix <= W - 1)
        v = p[:, np.clip(iy, 0, H - 1), np.clip(ix, 0, W - 1)].astype(wide)
        return np.where(ok, v, wide(cval)) if blend else v
    if blend:
        inside = (cy > -1) & (cy < H) & (cx > -1) & (cx < W)
        y1, x1 = y0 + 1, x0 + 1
    else:
        inside = (cy >= 0) & (cy <= H - 1) & (cx >= 0) & (cx <= W - 1)
        y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)          # a tap past the edge has weight zero
    top = (1 - wx) * tap(y0, x0) + wx * tap(y0, x1)
    bot = (1 - wx) * tap(y1, x0) + wx * tap(y1, x1)
    return np.where(inside, ((1 - wy) * top + wy * bot).astype(F64), F64(F32(cval)))


def nearest_const(p, iy, ix, inside):
    H, W = p.shape[1:]
    ok = inside & (iy >= 0) & (iy <= H - 1) & (ix >= 0) & (ix <= W - 1)
    return np.where(ok, p[:, np.clip(iy, 0, H - 1).astype(np.int64), np.clip(ix, 0, W - 1).astype(np.int64)], F32(0)).astype(F32)


def elastic_coords(minv, field, H, W):
    """((sy, sx) of stage 1, (cy, cx) of stage 2), fp64, in numpy's (the host's) unfused order"""
    m = np.asarray(minv, dtype=F64).reshape(6)
    xx, yy = np.meshgrid(np.arange(W, dtype=F64), np.arange(H, dtype=F64))
    sx, sy = (m[0] * xx + m[1] * yy) + m[2], (m[3] * xx + m[4] * yy) + m[5]
    return (sy, sx), (yy + field[1].astype(F64), xx + field[0].astype(F64))


def ref_stage1(img, mask, minv, H, W, cval, defect=None, wide=F64):
    (sy, sx), _ = elastic_coords(minv, np.zeros((2, H, W), F32), H, W)
    i = None if img is None else bilinear_const(img, sy, sx, cval, defect == "blend_with_constant", wide)
    rnd = (lambda c: np.floor(c + 0.5)) if defect == "stage1_floor_half" else np.rint
    k = None if mask is None else nearest_const(mask, rnd(sy), rnd(sx), np.ones((H, W), bool))
    return i, k


def ref_stage2(img_tmp, mask_tmp, field, H, W, cval, defect=None, wide=F64):
    if defect == "field_swapped":
        field = field[::-1]
    _, (cy, cx) = elastic_coords((1, 0, 0, 0, 1, 0), field, H, W)
    i = None if img_tmp is None else bilinear_const(img_tmp, cy, cx, cval, defect == "blend_with_constant", wide)
    rnd = np.rint if defect == "stage2_rint" else (lambda c: np.floor(c + 0.5))
    inside = (cy >= 0) & (cy <= H - 1) & (cx >= 0) & (cx <= W - 1)
    k = None if mask_tmp is None else nearest_const(mask_tmp, rnd(cy), rnd(cx), inside)
    return i, k


# ------------------------------------------------------------------------------------------------------------------ inputs
def rs_for(*key):
    """a generator that depends on the case alone, not on the order the cases run in"""
    return np.random.RandomState(sum((i + 1) * 7919 * (int(k) + 1) for i, k in enumerate(key)) % (2 ** 31))


def coded_labels(S, H, W):
    """every pixel of every slice its own fp32 number: a gather from the wrong place shows"""
    return (1 + np.arange(S * H * W, dtype=np.int64)).astype(F32).reshape(S, H, W)


def random_image(rs, S, H, W):
    """[-1, 1) on a 2^-12 grid with some exact -1 (the zeros of the [0,1] image)"""
    img = (rs.randint(-4096, 4096, size=(S, H, W)) / 4096.0).astype(F32)
    img[rs.rand(S, H, W) < 0.1] = -1.0
    return img


def table(maps, gammas=None, flags=None):
    t = np.zeros((len(maps), 8), dtype=F32)
    t[:, :6] = np.asarray(maps, dtype=F32)
    if gammas is not None:
        t[:, 6] = gammas
        t[:, 7] = 1.0 if flags is None else flags
    return t


def pick(pairs, img, lab):
    return (img if pairs in ("both", "img") else None), (lab if pairs in ("both", "lab", "mask") else None)


def exact_inputs(plane, S, first):
    H, W = plane
    names = [MAP_NAMES[(first + s) % len(MAP_NAMES)] for s in range(S)]
    rs = rs_for(H, W, S, first)
    return random_image(rs, S, H, W), coded_labels(S, H, W), table([EXACT_MAPS[n] for n in names]), names


def tie_share(name, plane):
    """share of the pixels of `plane` whose fp32 coordinate is exactly k + 1/2 on either axis, under the exact map `name`"""
    fy, fx = affine_coords32(table([EXACT_MAPS[name]]), *plane)
    return float(((fy - np.floor(fy) == 0.5) | (fx - np.floor(fx) == 0.5)).mean())


def random_maps(plane, S, seed, args):
    H, W = plane
    state = torch.get_rng_state()
    torch.manual_seed(1000 * seed + 7)
    maps = [draw_random_affine(H, W, **RANDOM_ARGS[args]) for _ in range(S)]
    torch.set_rng_state(state)
    return maps


def band_of(m, H, W):
    cy, cx = AC.affine_source(m, H, W)
    return cy, cx, AC.near_half(cy) | AC.near_half(cx)


def image_inputs(case, plane):
    """-> (img [S, H, W], params [S, 8]); the maps rotate through shear / id / half_shift / zoom2 so that fill pixels occur"""
    H, W = plane
    rs = rs_for(H, W, IMAGE_CASES.index(case), 99)
    maps = lambda n: [EXACT_MAPS[("shear", "id", "half_shift", "zoom2", "shrink")[i % 5]] for i in range(n)]   # noqa: E731
    if case == "gammas":
        img = (rs.rand(3, H, W) * 1.6 - 0.9).astype(F32)
        return img, table(maps(3), [0.5, 1.0, 1.5])
    if case == "flag_zero":                               # the exponent of a slice whose flag is off is not read
        return random_image(rs, 3, H, W), table(maps(3), [0.5, 1.5, 0.5], [0.0, -0.0, 1.0])
    if case == "flag_other":
        return random_image(rs, 3, H, W), table(maps(3), [0.5, 1.5, 0.75], [2.0, -1.0, 1e-30])
    if case == "min_is_minus_one":                        # an exact zero of the [0,1] image takes lo, law on and off
        return random_image(rs, 3, H, W), table(maps(3), [0.5, 1.5, 1.0], [1.0, 1.0, 0.0])
    if case == "near_minimum":                            # -1 + 2^-24: 3e-8 above the minimum; under gamma 2 the round trip makes it zero
        img = random_image(rs, 3, H, W)
        img[:, 0, :] = -1.0
        img.reshape(3, -1)[:, 1::2] = np.nextafter(F32(-1), F32(0))
        return img, table([EXACT_MAPS["id"], EXACT_MAPS["half_shift"], EXACT_MAPS["id"]], [1.5, 2.0, 2.0])
    if case == "constant":                                # span = 1e-5
        img = np.stack([np.full((H, W), v, dtype=F32) for v in (0.3, -1.0, 0.0)])
        return img, table(maps(3), [0.5, 1.5, 1.0], [1.0, 1.0, 0.0])
    if case == "extremes_last":                           # minimum at the last element, maximum just before it
        img = (rs.rand(2, H, W) * 0.5 - 0.25).astype(F32)
        img.reshape(2, -1)[:, -1] = -0.875
        if H * W > 1:
            img.reshape(2, -1)[:, -2] = 0.9375
        return img, table(maps(2), [0.5, 1.5])
    if case == "all_fill":                                # every pixel outside: the fill takes lo
        return random_image(rs, 2, H, W), table([EXACT_MAPS["far"]] * 2, [0.5, 1.0], [1.0, 0.0])
    raise KeyError(case)


def minmax_inputs(plane, S, kind):
    H, W = plane
    rs = rs_for(H, W, S, MINMAX_KINDS.index(kind))
    x = (rs.rand(S, H, W) * 2 - 1).astype(F32)
    flat = x.reshape(S, -1)
    if kind == "extremes_last":
        flat[:, -1] = -3.0 - np.arange(S)
        if H * W > 1:
            flat[:, -2] = 5.0 + np.arange(S)
    elif kind == "extremes_first":
        flat[:, 0] = 7.0 + np.arange(S)
        if H * W > 1:
            flat[:, 1] = -9.0 - np.arange(S)
    elif kind == "constant":
        flat[:] = (0.25 * np.arange(S) - 0.5)[:, None]
    elif kind == "signed_zeros":
        flat[:] = np.where(rs.rand(S, H * W) < 0.5, F32(0.0), F32(-0.0))
    return x


def field_weights(spec):
    if spec[0] == "one":
        return np.ones(1), 0
    if spec[0] == "r1":
        return np.array([0.25, 0.5, 0.25]), 1
    return gaussian_weights(spec[1])


def field_noise(plane, kind):
    """random planes in [-1, 1), or unit impulses at a corner / the centre: the response is the reflect-folded outer product of the weights"""
    H, W = plane
    if kind == "random":
        return [rs_for(H, W, 5).rand(2, H, W) * 2 - 1]
    out = []
    spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)]
    for a, b in zip(spots[0::2] + spots[1::2], spots[1::2] + spots[0::2]):
        n = np.zeros((2, H, W))
        n[0][a], n[1][b] = 1.0, -1.0
        out.append(n)
    return out[:3]                                        # every corner and the centre appear in plane 0 or plane 1


def crafted_field(name, plane):
    """[2, H, W] fp32 = (dx, dy), dyadic"""
    H, W = plane
    f = np.zeros((2, H, W), dtype=F32)
    x, y = np.meshgrid(np.arange(W, dtype=F32), np.arange(H, dtype=F32))
    e = F32(2.0 ** -20)
    if name == "plus_half":
        f[:] = 0.5
    elif name == "minus_half":
        f[:] = -0.5
    elif name == "ramp_top":                              # even columns land exactly on W-1, odd ones 2^-20 past it; rows likewise
        f[0] = (W - 1) - x + np.where(x % 2 == 1, e, 0)
        f[1] = np.where(y % 3 == 2, (H - 1) - y + np.where(x % 2 == 0, e, 0), 0)
    elif name == "ramp_bottom":                           # exactly 0, and -2^-20
        f[0] = -x - np.where(x % 2 == 1, e, 0)
        f[1] = np.where(y % 3 == 1, -y - np.where(x % 2 == 0, e, 0), 0)
    elif name == "dx_dy_differ":
        f[0], f[1] = 1.5, -0.25 * (x % 4)
    return f


def elastic_inputs(plane, S, seed, dyadic):
    H, W = plane
    rs = rs_for(H, W, S, seed, 17)
    if dyadic:                                            # multiples of 1/64 in [-1, 1): every bilinear blend at quarter weights is exact
        img = (rs.randint(-64, 64, size=(S, H, W)) / 64.0).astype(F32)
    else:
        img = (rs.rand(S, H, W) * 2 - 1).astype(F32)
    mask = (rs.rand(S, H, W) < 0.5).astype(F32)
    if S >= 3:
        mask[1] = 0                                       # one slice of three (or more) with an empty mask
    return img, mask


# ------------------------------------------------------------------------------------------------------------------ checks
def check_minmax(be, plane, S, kind):
    """rpnet_slice_minmax, by value"""
    x = minmax_inputs(plane, S, kind)
    res = be.minmax(x)
    tag = f"{kind} {tag_of(plane, S)}"
    return [by_value("minmax", tag, res["mm"], ref_minmax(x))] + common("minmax", tag, res)


def check_big_s(be):
    """S = 65535 on a 1 x 3 plane: rpnet_slice_minmax and rpnet_augment_affine with blockIdx.y at its limit"""
    S, H, W = BIG_S
    rs = rs_for(S, H, W)
    img, lab = random_image(rs, S, H, W), coded_labels(S, H, W)
    names = [MAP_NAMES[s % len(MAP_NAMES)] for s in range(S)]
    params = table([EXACT_MAPS[n] for n in names], 0.5 + (np.arange(S) % 5) * 0.25, (np.arange(S) % 3 == 0).astype(F32))
    mm = ref_minmax(img)
    r1 = be.minmax(img)
    recs = [by_value("minmax", f"{S}x{H}x{W}", r1["mm"], mm)] + common("minmax", f"{S}x{H}x{W}", r1)
    res = be.affine(img, lab, params, mm)
    want_i, want_l = ref_affine(img, lab, params, mm, H, W)
    off = params[:, 7] == 0
    recs += [exact("affine", f"labels {S}x{H}x{W}", res["lab_out"], want_l), exact("affine", f"images, law off {S}x{H}x{W}", res["img_out"][off], want_i[off])]
    recs += law_records(f"{S}x{H}x{W}", res["img_out"][~off], want_i[~off])
    return recs + common("affine", f"{S}x{H}x{W}", res)


def law_records(tag, got, want):
    err = float(np.abs(got.astype(F64) - want.astype(F64)).max(initial=0.0)) if np.isfinite(got).all() else math.inf
    return [within("law", f"images, law on {tag}", err, IMAGE_BOUND)]


def check_affine_exact(be, plane, S, first, pairs):
    """rpnet_augment_affine with exact maps and the power law off: labels and images bit for bit on every pixel, ties included"""
    H, W = plane
    img, lab, params, names = exact_inputs(plane, S, first)
    mm = ref_minmax(img)
    img_in, lab_in = pick(pairs, img, lab)
    res = be.affine(img_in, lab_in, params, mm if img_in is not None else None)
    want_i, want_l = ref_affine(img_in, lab_in, params, mm, H, W)
    tag = f"{'+'.join(names)} {pairs} {tag_of(plane, S)}"
    recs = common("affine", tag, res)
    if lab_in is not None:
        recs.append(exact("affine", f"labels {tag}", res["lab_out"], want_l))
    if img_in is not None:
        recs.append(exact("affine", f"images {tag}", res["img_out"], want_i))
    return recs


def check_affine_random(be, plane, S, seed, args):
    """rpnet_augment_affine with drawn maps: the band helpers of tests/augment_cases.py, at most BAND_CAP of a slice excluded"""
    H, W = plane
    maps = random_maps(plane, S, seed, args)
    rs = rs_for(H, W, S, seed)
    img, lab = random_image(rs, S, H, W), coded_labels(S, H, W)
    mm = ref_minmax(img)
    res = be.affine(img, lab, table(maps), mm)
    tag = f"{args} seed {seed} {tag_of(plane, S)}"
    recs = common("affine", tag, res)
    for s, m in enumerate(maps):
        cy, cx, band = band_of(m, H, W)
        recs.append(within("affine_band", f"excluded share slice {s} {tag}", float(band.mean()), BAND_CAP))
        u = (img[s] + F32(1)) / F32(2)                    # the [0,1] image the sampling stage is given: zeros outside, zeros take lo
        lo = u.min()
        post = lambda v: (np.where(v == 0, lo, v) * F32(2) - F32(1)).astype(F32)   # noqa: E731
        for what, got, src, fn in (("labels", res["lab_out"][s], lab[s], lambda v: v), ("images", res["img_out"][s], u, post)):
            want = fn(AC.gather(src, np.rint(cy).astype(np.int64), np.rint(cx).astype(np.int64)))
            cands = np.stack([fn(c) for c in AC.candidates(src, cy, cx)])
            bad = (bits(got) != bits(want)) & ~band
            bad_in = band & ~(bits(cands) == bits(got)[None]).any(axis=0)
            recs.append(count("affine", f"{what} outside the band, or no candidate inside it, slice {s} {tag}", bad.sum() + bad_in.sum()))
    return recs


def check_image(be, case, plane, pairs):
    """rpnet_augment_affine's image path: slices with the law off bit for bit, with it on within IMAGE_BOUND"""
    H, W = plane
    img, params = image_inputs(case, plane)
    S = img.shape[0]
    lab = coded_labels(S, H, W)
    mm = ref_minmax(img)
    img_in, lab_in = pick(pairs, img, lab)
    res = be.affine(img_in, lab_in, params, mm if img_in is not None else None)
    want_i, want_l = ref_affine(img_in, lab_in, params, mm, H, W)
    tag = f"{case} {pairs} {tag_of(plane, S)}"
    recs = common("affine", tag, res)
    if lab_in is not None:
        recs.append(exact("affine", f"labels {tag}", res["lab_out"], want_l))
    if img_in is not None:
        off = params[:, 7] == 0
        recs.append(exact("affine", f"images, law off {tag}", res["img_out"][off], want_i[off]))
        recs += law_records(tag, res["img_out"][~off], want_i[~off])
    return recs


def check_field(be, plane, wspec, noise_kind, alpha):
    """rpnet_elastic_field with the caller's own weights: one fp32 ulp; radius 0 with weight 1 bit for bit"""
    w, radius = field_weights(wspec)
    recs = []
    for i, noise in enumerate(field_noise(plane, noise_kind)):
        res = be.field(noise, w, radius, alpha)
        tag = f"{'_'.join(str(v) for v in wspec)} {noise_kind}{i} alpha {alpha:g} {plane[0]}x{plane[1]}"
        want_tmp, want = ref_field(noise, w, radius, alpha)
        recs += common("field", tag, res)
        recs.append(count("field", f"tmp elements not finite {tag}", (~np.isfinite(res["tmp"])).sum()))
        # the axis-0 pass on its own: n = 2 radius + 1 multiply-adds, each rounded to 2^-53 of a partial sum that the normalised weights
        # keep within max |noise|, on either side of the comparison
        tmp_err = float(np.abs(res["tmp"] - want_tmp).max()) if np.isfinite(res["tmp"]).all() else math.inf
        recs.append(within("field_tmp", f"axis-0 pass {tag}", tmp_err, (2 * radius + 1) * 2.0 ** -52 * float(np.abs(noise).max()) * float(np.abs(w).sum())))
        if radius == 0:
            recs.append(exact("field", f"(float)(alpha * noise) {tag}", res["field"], (F64(alpha) * noise).astype(F32)))
        recs.append(within("field", f"ulps {tag}", ulps(res["field"], want.astype(F64)), 1.0))
    return recs


def _elastic_records(be, tag, img, mask, minv, field, pad, triples, crafted):
    S, H, W = (img if img is not None else mask).shape
    img_in, mask_in = pick(triples, img, mask)
    res = be.elastic(img_in, mask_in, minv, field, pad)
    recs = common("elastic", tag, res)
    w1_i, w1_m = ref_stage1(img_in, mask_in, minv, H, W, pad)
    if mask_in is not None:
        _, w2_m = ref_stage2(None, w1_m, field, H, W, pad)
        recs += [exact("elastic", f"mask stage 1 {tag}", res["mask_tmp"], w1_m), exact("elastic", f"mask {tag}", res["mask_out"], w2_m)]
    if img_in is not None:
        ok = np.isfinite(res["img_tmp"]).all()
        own = res["img_tmp"] if ok else w1_i.astype(F32)            # stage 2 from the backend's own stage 1: its ulp is charged once
        w2_own, _ = ref_stage2(own, None, field, H, W, pad)
        if crafted:
            w2_i, _ = ref_stage2(w1_i.astype(F32), None, field, H, W, pad)
            recs += [exact("elastic", f"image stage 1 {tag}", res["img_tmp"], w1_i.astype(F32)), exact("elastic", f"image {tag}", res["img_out"], w2_i.astype(F32))]
        else:
            recs += [within("bilinear", f"image stage 1 ulps {tag}", ulps(res["img_tmp"], w1_i), 1.0),
                     within("bilinear", f"image ulps {tag}", ulps(res["img_out"], w2_own), 1.0)]
    return recs


def check_elastic_crafted(be, plane, S, mname, fname, pad, triples):
    """rpnet_elastic_apply on dyadic coordinates and pixel values: image and mask bit for bit, both stages"""
    img, mask = elastic_inputs(plane, S, FIELDS.index(fname), True)
    tag = f"{mname} {fname} pad {pad:g} {triples} {tag_of(plane, S)}"
    return _elastic_records(be, tag, img, mask, MINV[mname], crafted_field(fname, plane), pad, triples, True)


def elastic_random_inputs(plane, S, seed):
    minv, _ = draw_elastic(plane, 0.04, np.random.RandomState(seed))
    field = (rs_for(plane[0], plane[1], seed, 3).rand(2, *plane) * 16 - 8).astype(F32)
    return minv.reshape(6), field


def check_elastic_random(be, plane, S, seed, pad, triples):
    """rpnet_elastic_apply with Minv of draw_elastic and a random fp32 field of magnitude up to 8: mask equal, image within one ulp"""
    img, mask = elastic_inputs(plane, S, seed, False)
    minv, field = elastic_random_inputs(plane, S, seed)
    return _elastic_records(be, f"random seed {seed} pad {pad:g} {triples} {tag_of(plane, S)}", img, mask, minv, field, pad, triples, False)


def check_production(be, entry):
    """the production size, 12 slices of 256 x 256, once per entry point"""
    S, H, W = PRODUCTION
    rs = rs_for(S, H, W)
    if entry == "minmax":
        x = random_image(rs, S, H, W)
        res = be.minmax(x)
        return [by_value("minmax", "production", res["mm"], ref_minmax(x))] + common("minmax", "production", res)
    if entry == "affine":
        img, lab = random_image(rs, S, H, W), coded_labels(S, H, W)
        params = table([EXACT_MAPS[MAP_NAMES[s % 8]] for s in range(S)], 0.5 + 0.125 * np.arange(S), (np.arange(S) % 2).astype(F32))
        mm = ref_minmax(img)
        res = be.affine(img, lab, params, mm)
        want_i, want_l = ref_affine(img, lab, params, mm, H, W)
        off = params[:, 7] == 0
        return (common("affine", "production", res) + [exact("affine", "labels production", res["lab_out"], want_l),
                                                       exact("affine", "images, law off production", res["img_out"][off], want_i[off])]
                + law_records("production", res["img_out"][~off], want_i[~off]))
    if entry == "field":
        return check_field(be, (H, W), ("gauss", 30), "random", 1000.0)
    return check_elastic_random(be, (H, W), S, 9, -1.0, "both")


# --------------------------------------------------------------------------------------------------------------- refusals
def refusals(buf, dbuf):
    """[(label, entry point, args without the stream, expected rpnet_status, words of the message)]: every call is refused on the host,
    before any launch.  buf(n) -> a valid buffer of n floats, dbuf(n) of n doubles; Minv is the tuple MINV6 (a host array).
    -> (rows, the buffers that must come back unchanged)"""
    n = 1 << 12
    x, mm, params, img, lab, io, lo = buf(n), buf(n), buf(n), buf(n), buf(n), buf(n), buf(n)
    noise, w, tmp, field = dbuf(n), dbuf(n), dbuf(n), buf(n)
    msk, it, mt, mo = buf(n), buf(n), buf(n), buf(n)
    S, H, W = 2, 4, 4
    minv = MINV6

    def sm(x=x, mm=mm, S=S, H=H, W=W):
        return ("rpnet_slice_minmax", (x, mm, S, H, W))

    def af(img=img, lab=lab, params=params, mm=mm, io=io, lo=lo, S=S, H=H, W=W):
        return ("rpnet_augment_affine", (img, lab, params, mm, io, lo, S, H, W))

    def ef(noise=noise, w=w, radius=1, tmp=tmp, field=field, H=H, W=W):
        return ("rpnet_elastic_field", (noise, w, radius, 1.0, tmp, field, H, W))

    def ea(img=img, msk=msk, minv=minv, field=field, it=it, mt=mt, io=io, mo=mo, S=S, H=H, W=W):
        return ("rpnet_elastic_apply", (img, msk, minv, field, it, mt, io, mo, S, H, W, -1.0))

    plane, many, big = "S=", "at most 65535", "32-bit index"
    pair, both3 = "come together", "come together"
    rows = []
    for fn in (sm, af, ea):
        rows += [("H = 0", fn(H=0), SHAPE, plane), ("W = 0", fn(W=0), SHAPE, plane), ("H = -1", fn(H=-1), SHAPE, plane), ("S = -1", fn(S=-1), SHAPE, plane),
                 ("S = 65536", fn(S=65536), SHAPE, many), ("S H W = 2^31", fn(S=32768, H=256, W=256), SHAPE, big),
                 ("S H W = 2^31 with S = 1", fn(S=1, H=65536, W=32768), SHAPE, big)]
    rows += [("H = 0", ef(H=0), SHAPE, plane), ("W = -1", ef(W=-1), SHAPE, plane), ("2 H W = 2^31", ef(H=32768, W=32768), SHAPE, big),
             ("null x", sm(x=None), ARG, "null pointer"), ("null mm", sm(mm=None), ARG, "null pointer"),
             ("null params", af(params=None), ARG, "null parameter table"),
             ("img without img_out", af(io=None), ARG, pair), ("img_out without img", af(img=None), ARG, pair),
             ("lab without lab_out", af(lo=None), ARG, pair), ("lab_out without lab", af(lab=None), ARG, pair),
             ("neither pair", af(img=None, io=None, lab=None, lo=None), ARG, "at least one pair"),
             ("images without mm", af(mm=None), ARG, "need the min/max table"),
             ("images in place", af(io=img), ARG, "cannot run in place"), ("labels in place", af(lo=lab), ARG, "cannot run in place"),
             ("labels in place, labels alone", af(img=None, io=None, mm=None, lo=lab), ARG, "cannot run in place"),
             ("null noise", ef(noise=None), ARG, "null pointer"), ("null weights", ef(w=None), ARG, "null pointer"),
             ("null tmp", ef(tmp=None), ARG, "null pointer"), ("null field", ef(field=None), ARG, "null pointer"),
             ("radius -1", ef(radius=-1), ARG, "radius -1"), ("radius 2^20", ef(radius=1 << 20), ARG, "radius 1048576"),
             ("tmp aliases noise", ef(tmp=noise), ARG, "must not alias"),
             ("null minv", ea(minv=None), ARG, "null Minv or field"), ("null field", ea(field=None), ARG, "null Minv or field"),
             ("img without img_tmp", ea(it=None), ARG, "image, its intermediate"), ("img without img_out", ea(io=None), ARG, "image, its intermediate"),
             ("img_tmp and img_out without img", ea(img=None), ARG, "image, its intermediate"),
             ("img_tmp alone", ea(img=None, io=None), ARG, "image, its intermediate"), ("img_out alone", ea(img=None, it=None), ARG, "image, its intermediate"),
             ("img alone", ea(it=None, io=None), ARG, "image, its intermediate"),
             ("mask without mask_tmp", ea(mt=None), ARG, "mask, its intermediate"), ("mask without mask_out", ea(mo=None), ARG, "mask, its intermediate"),
             ("mask_tmp and mask_out without mask", ea(msk=None), ARG, "mask, its intermediate"),
             ("mask_tmp alone", ea(msk=None, mo=None), ARG, "mask, its intermediate"), ("mask_out alone", ea(msk=None, mt=None), ARG, "mask, its intermediate"),
             ("mask alone", ea(mt=None, mo=None), ARG, "mask, its intermediate"),
             ("neither triple", ea(img=None, it=None, io=None, msk=None, mt=None, mo=None), ARG, "neither images nor masks"),
             ("img == img_tmp", ea(it=img), ARG, "cannot run in place"), ("img_tmp == img_out", ea(io=it), ARG, "cannot run in place"),
             ("mask == mask_tmp", ea(mt=msk), ARG, "cannot run in place"), ("mask_tmp == mask_out", ea(mo=mt), ARG, "cannot run in place")]
    outputs = [mm, io, lo, tmp, field, it, mt, mo]
    return [(label, entry, args, code, words) for label, (entry, args), code, words in rows], outputs


MINV6 = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


# ------------------------------------------------------------------------------------- the numpy stand-in for the library
DEFECTS = ["affine_half_up", "last_block_unwritten", "params_slice0", "mm_slice0", "minmax_first_1024", "lo_without_law", "law_without_1e5",
           "inside_lt", "centre_w_both", "flag_eq_1", "reflect_period_n", "reflect_mirror", "blur_same_axis", "field_swapped",
           "blend_with_constant", "stage2_rint", "stage1_floor_half", "stage2_reads_input", "pad_fixed"]


# A change that NO row can see, because no output depends on it: leaving out the fp32 round trip ((v * 2 - 1) + 1) / 2 of the power law.
# r = fl(2v - 1) lies on the 2^-24 grid of [-1, -1/2] or is exact (Sterbenz, 2v in [1/2, 2]), so fl(r + 1) is exact and fl(2 RT(v) - 1) =
# fl(fl(r + 1) - 1) = r = fl(2v - 1): the last line of the kernel undoes it bit for bit.  What is left is the zero test: RT(v) == 0 iff
# fl(2v - 1) == -1, and then `lo` (the law at the slice minimum, <= v, through the same round trip) is zero as well, so the pixel is -1
# with the round trip and without it.  The argument needs v in [0, 1] and lo <= v, that is a slice in [-1, 1] (lo_u >= 0) and mm the
# slice's own minimum and maximum, as the header asks.  tests/test_host_augment_ref64.py holds both on the fp32 numbers of [0, 1] it draws.
UNOBSERVABLE = ["no_round_trip"]


def exp_log_pow(x, y):
    """a pow that is not numpy's: a few fp64 units away, as another library's may be"""
    return np.exp(y * np.log(x))


class SimBackend:
    """the four entry points in the kernels' own operation order.  Where the device may legitimately differ from the restatement so
    does this: pow through exp and log, the fp64 sums of the blur and the bilinear blend carried in extended precision and rounded
    once (what contracting every multiply-add would do at most).  `defect`: one of DEFECTS"""
    WIDE = np.longdouble

    def __init__(self, defect=None):
        assert defect is None or defect in DEFECTS + UNOBSERVABLE, defect
        self.defect = defect

    def minmax(self, x):
        y = x.reshape(x.shape[0], -1)[:, :MINMAX_STRIDE] if self.defect == "minmax_first_1024" else x
        return {"mm": ref_minmax(y), "guards": 0, "repeat": 0}

    def affine(self, img, lab, params, mm):
        S, H, W = (img if img is not None else lab).shape
        i, l = ref_affine(img, lab, params, mm, H, W, self.defect, exp_log_pow)
        return {"img_out": i, "lab_out": l, "guards": 0, "repeat": 0}

    def field(self, noise, w, radius, alpha):
        tmp, field = ref_field(noise, w, radius, alpha, self.defect, self.WIDE)
        return {"tmp": tmp, "field": field, "guards": 0, "repeat": 0}

    def elastic(self, img, mask, minv, field, pad):
        S, H, W = (img if img is not None else mask).shape
        d = self.defect
        cval = -1.0 if d == "pad_fixed" else pad
        i1, m1 = ref_stage1(img, mask, minv, H, W, cval, d, self.WIDE)
        i1 = None if i1 is None else i1.astype(F32)
        src_i, src_m = (img, mask) if d == "stage2_reads_input" else (i1, m1)
        i2, m2 = ref_stage2(src_i, src_m, field, H, W, cval, d, self.WIDE)
        return {"img_tmp": i1, "mask_tmp": m1, "img_out": None if i2 is None else i2.astype(F32), "mask_out": m2, "guards": 0, "repeat": 0}
