"""Cases and comparison functions shared by tests/test_host_corr_ref64.py and tests/test_gpu_corr_fp64.py: the local-window
correlation (csrc/corr.hip on the VALU, csrc/corr_split.hip on the matrix pipe) against tests/ref64.py at every dispatch edge.

A *backend* runs the five entry points on CPU tensors and returns CPU tensors: the HIP library (the GPU test), or SimBackend, a
float32 torch restatement with or without a seeded defect (the host test).  The check_* functions drive a backend through one
case and return records; hold() prints them and asserts.  Neither test restates a bound.

Bound (the yardstick of tests/test_gpu_small_ops.py, FACTOR and FLOOR are its numbers; tests/test_host_corr_ref64.py asserts
they still are): rel_err(got, r64) <= 8 * yard + 4 * 2^-24, yard = rel_err(r32, r64), r32 = the same ref64 function at float32.

Plane arithmetics: the reference is evaluated on the values the planes REPRESENT (plane_values: s * (p0 + p1), or the sum of
three bf16 planes, in float64), so operand rounding is not charged to the kernel.  The one rounding the kernels do themselves is
the on-the-fly split of the window gradient in the split backward; it gets the explicit term of split_term().

Exact checks (pad channels, window entries outside the image, all-zero operands, written fp16 planes, out_absmax) count
mismatching elements and allow none.  The dynamic-range case takes its error per 8 x 8 tile, relative to that tile's own
reference maximum (per_tile)."""
import math

import torch
import torch.nn.functional as F

from tests import ref64 as R
from tests.helpers import rel_err, rnd

F32, F64 = torch.float32, torch.float64
FACTOR, FLOOR = 8.0, 4 * 2.0 ** -24
SHAPE, ARG, WORKSPACE = -1, -2, -3          # enum rpnet_status of include/rpnet_abi.h
TILE = 8                                    # pixel tile edge of every correlation kernel

# unit round-offs of the plane formats (csrc/split_bf16.h): fp16 has 11 significand bits, bf16 has 8, round to nearest even
U_F16, U_BF16 = 2.0 ** -11, 2.0 ** -8


def split_unit_roundoff(planes):
    """|x - (sum of the planes of x)| <= u * max|x| over the tile whose maximum set the scale.
    planes = 1: x = fp16(x) (1 + d), |d| <= 2^-11.
    planes = 2: h = fp16(x), l = fp16(x - h): |x - h| <= 2^-11 |x| and |(x - h) - l| <= 2^-11 |x - h| <= 2^-22 |x| while the
                residual is a normal fp16 number; below that its spacing is 2^-24, i.e. an absolute 2^-25 on values that the
                block-local power-of-two scale has brought to a tile maximum in (2^14, 2^15]: 2^-25 / 2^14 of that maximum.
    planes = 3: three bf16 planes, 2^-8 each: (2^-8)^3 = 2^-24 (an fp32 value is in fact the exact sum of its three planes)."""
    return {1: U_F16, 2: U_F16 ** 2 + 2.0 ** -25 / 2.0 ** 14, 3: U_BF16 ** 3}[planes]


def corr_stride(r):
    """the Function's own stride (rpnet_amd.functional.corr_stride; the GPU test asserts the two agree)"""
    kk = (2 * r + 1) ** 2
    return 128 if kk <= 128 else (kk + 63) // 64 * 64


# ------------------------------------------------------------------------------------------------------------------ tables
# B, h, w, C
FP32_SHAPES = [(1, 1, 1, 64),        # one pixel: a window that is all outside but its centre; FastDiv(1) twice in the transpose
               (1, 1, 9, 64),        # h = 1, two tiles across, the second one pixel wide
               (2, 9, 1, 64),        # w = 1, two tiles down
               (1, 3, 5, 64),        # every extent below radius 5: one ragged tile, windows mostly outside
               (2, 8, 8, 64),        # exactly one full tile
               (3, 9, 17, 64),       # ragged in both axes, 2 x 3 tiles
               (1, 16, 20, 128)]     # two 64-channel stages (four 32-channel ones at radius 6 / 7)
# (r, shape, cstride): every radius at cstride = KK (the zero-fill loop runs zero times) and at the Function's stride
FP32_CASES = [(r, s, cs) for r in range(1, 8) for s in FP32_SHAPES for cs in sorted({(2 * r + 1) ** 2, corr_stride(r), 256 if r == 7 else 0} - {0})]
# forward only: C % 32 that is no multiple of 64
FP32_FWD_ONLY = [(r, (3, 9, 17, C), corr_stride(r)) for r in range(1, 8) for C in (32, 96)]

SPLIT_SHAPES = [(1, 1, 1), (1, 3, 5), (2, 8, 8), (3, 9, 17), (1, 16, 24), (5, 8, 16)]      # the last: 10 blocks, remainder 2 in xcd_swizzle
SPLIT_FWD_CASES = [(p, s, C, cs) for p in (3, 2, 1) for s in SPLIT_SHAPES for C in (32, 96, 128, 256) for cs in (121, 128, 160)]
SPLIT_BWD_CASES = [(p, s, C, cs) for p in (3, 2, 1) for s in SPLIT_SHAPES for C in ((128, 256) if p == 3 else (128, 256, 384))
                   for cs in (121, 128)]
# The one check that missed 8 yardsticks on the MI355X: split forward, three planes, 1 x 1 x 1 x 256 at cstride 121, measured
# 78.3 (err 1.438e-06, yard 1.837e-08).  A 1 x 1 image has ONE non-zero output, a single dot product, so err and yard are one
# draw each instead of a maximum over thousands.  This draw cancels: the value is 1.51 / 16 against sum |f1 f2| = 33.3 / 16, a
# condition number of 22.  torch adds the 256 products pairwise and happened to land 0.3 ulp from the float64 value; the kernel
# adds them in ONE fp32 accumulator as a chain of 96 matrix-pipe steps (16 channel groups of 16, each as the six plane products
# lh hl mm mh hm hh, smallest first), and its error is 1.09 unit round-offs OF sum |f1 f2| — a chain of 96 additions may take 96.
# Every other ratio above 8 (five, all of them 1 x 1 x 1 draws as well) is inside the bound through its floor.  This one check
# gets twice its measured ratio.
MEASURED_FACTORS = {(3, (1, 1, 1), 256, 121): 157.0}       # (planes, (B, h, w), C, cstride) of SPLIT_FWD_CASES
DYNAMIC_CASES = [(3, 128), (2, 256), (1, 256)]            # planes, C at 2 x 16 x 16
# per 8 x 8 tile of the 2 x 16 x 16 gradient: a power of two, "one" (a single non-zero element) or "zero"
DYNAMIC_TILES = [-40, 20, -13, "one", "zero", 7, -27, 13]
CROSS_PATH = (5, (3, 9, 17, 128))


def case_seed(*key):
    return 1 + sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % 100003


# ------------------------------------------------------------------------------------------------------------------ planes
def pow2_scale(bound):
    """the smallest power of two >= bound, times 2^-15 (csrc/split_bf16.h): |x / s| <= 2^15"""
    if not bound > 0:
        return 2.0 ** -100
    if math.isinf(float(bound)):              # frexp(inf) has no exponent; the clamp is 2^100 (tests/operand_cases.py pins both ends)
        return 2.0 ** 100
    m, e = math.frexp(float(bound))           # bound = m 2^e, 0.5 <= m < 1
    e = e - 1 if m == 0.5 else e
    return 2.0 ** max(-100, min(100, e - 15))


def split_planes(x, planes, scale=None):
    """fp32 x -> int16 [planes, ...]: three bf16 planes of x, or two / one fp16 planes of x / scale (round to nearest even)"""
    x = x.float()
    if planes == 3:
        h = x.bfloat16()
        r1 = x - h.float()
        m = r1.bfloat16()
        return torch.stack([h, m, (r1 - m.float()).bfloat16()]).view(torch.int16)
    xs = x / scale
    h = xs.half()
    return torch.stack([h, (xs - h.float()).half()][:planes]).view(torch.int16)


def plane_values(bits, scale=None, dtype=F64):
    """what the planes represent: s * (p0 + p1) for fp16 planes, p0 + p1 + p2 for bf16 planes"""
    if bits.shape[0] == 3:
        return bits.view(torch.bfloat16).to(dtype).sum(0)
    return bits.view(torch.float16).to(dtype).sum(0) * scale


def make_operands(seed, shape, planes):
    """(f1, f2) fp32 [B, h, w, C] of different magnitude (so that the two tensor scales differ); for planes: (bits1, bits2, s1, s2)"""
    f1, f2 = rnd(seed, *shape), 3.0 * rnd(seed + 1, *shape)
    if not planes:
        return f1, f2
    s1, s2 = (None, None) if planes == 3 else (pow2_scale(f1.abs().max()), pow2_scale(f2.abs().max()))
    return split_planes(f1, planes, s1), split_planes(f2, planes, s2), s1, s2


def dynamic_dcorr(seed, cstride):
    """[2, 16, 16, cstride]: standard normal times a power of two per 8 x 8 tile (DYNAMIC_TILES)"""
    g = rnd(seed, 2, 16, 16, cstride)
    for i, e in enumerate(DYNAMIC_TILES):
        b, ty, tx = i // 4, (i // 2) % 2, i % 2
        t = g[b, ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8]
        if e == "zero":
            t.zero_()
        elif e == "one":
            keep = float(t[3, 5, 17])
            t.zero_()
            t[3, 5, 17] = keep
        else:
            t.mul_(2.0 ** e)
    return g


# ---------------------------------------------------------------------------------------------------------------- geometry
def inside_mask(h, w, r, cstride):
    """[h, w, cstride] bool: window channel o = a K + c of pixel (y, x) has its source pixel (y + c - r, x + a - r) in the image"""
    K = 2 * r + 1
    y, x = torch.arange(h)[:, None, None, None], torch.arange(w)[None, :, None, None]
    a, c = torch.arange(K)[None, None, :, None], torch.arange(K)[None, None, None, :]
    m = ((y + c - r >= 0) & (y + c - r < h) & (x + a - r >= 0) & (x + a - r < w)).reshape(h, w, K * K)
    return F.pad(m, (0, cstride - K * K))


def transpose_window(dcorr, r):
    """dcT[b, q, o] = dcorr[b, q - off(o), o] (0 outside): the window gradient seen from the f2 pixel; channels < KK only"""
    B, h, w, _ = dcorr.shape
    K = 2 * r + 1
    dp = F.pad(dcorr[..., :K * K], (0, 0, r, r, r, r))
    return torch.stack([dp[:, 2 * r - c:2 * r - c + h, 2 * r - a:2 * r - a + w, a * K + c] for a in range(K) for c in range(K)], -1)


def tile_max(t):
    """[B, h, w, C] -> [B, th, tw]: max |t| over each 8 x 8 tile and all channels"""
    return F.max_pool2d(t.abs().amax(-1)[:, None], TILE, ceil_mode=True)[:, 0]


def to_pixels(tm, h, w):
    return tm.repeat_interleave(TILE, 1).repeat_interleave(TILE, 2)[:, :h, :w]


def split_term(g, fo, r, planes):
    """the rounding of the split backward's on-the-fly split of the window gradient, an absolute allowance per output element
    [B, h, w, C] in float64: u * max_tile |g| * sum over the window of |fo[q, ch]| / sqrt(C).  g: the gradient as the pass sees
    it (dcorr for d f1, its transpose for d f2), fo: the other operand's values."""
    B, h, w, C = fo.shape
    K = 2 * r + 1
    box = F.avg_pool2d(fo.double().abs().permute(0, 3, 1, 2), K, 1, r, count_include_pad=True, divisor_override=1).permute(0, 2, 3, 1)
    gmax = to_pixels(tile_max(g.double()[..., :K * K]), h, w)
    return split_unit_roundoff(planes) * gmax[..., None] * box / math.sqrt(C)


# ----------------------------------------------------------------------------------------------------------------- records
class Rec:
    def __init__(self, family, what, err, yard, bound, exact=False):
        self.family, self.what, self.err, self.yard, self.bound, self.exact = family, what, float(err), float(yard), float(bound), exact

    @property
    def ok(self):
        return self.err == 0 if self.exact else self.err <= self.bound

    @property
    def ratio(self):
        return self.err / self.yard if self.yard > 0 else 0.0

    @property
    def multiple(self):
        """of the bound (an exact check that fails counts its mismatches)"""
        return self.err if self.exact else self.err / self.bound

    def line(self):
        return f"PARITY corr {self.family} {self.what} err={self.err:.3e} yard={self.yard:.3e} ratio={self.ratio:.2f}"


def measure(family, what, got, r64, r32, extra=None, factor=FACTOR):
    """the yardstick bound of the module docstring; `extra`: an absolute per-element allowance taken off the difference first"""
    d = (got.double() - r64).abs()
    if extra is not None:
        d = (d - extra).clamp_min(0)
    err = (d.max() / (r64.abs().max() + 1e-12)).item() if torch.isfinite(got).all() else math.inf
    yard = rel_err(r32, r64)
    return Rec(family, what, err, yard, factor * yard + FLOOR)


def per_tile(family, what, got, r64, r32, extra=None, factor=FACTOR):
    """as measure(), but per 8 x 8 tile and relative to that tile's own reference maximum: the record of the worst tile.  A tile
    whose reference is all zero must be exactly zero."""
    d = (got.double() - r64).abs()
    if extra is not None:
        d = (d - extra).clamp_min(0)
    if not torch.isfinite(got).all():
        return Rec(family, what, math.inf, 0.0, FLOOR)
    ref, worst = tile_max(r64), None
    err, yard = tile_max(d) / ref, tile_max(r32.double() - r64) / ref
    for idx in torch.cartesian_prod(*[torch.arange(n) for n in ref.shape]).tolist():
        b, ty, tx = idx
        name = f"{what}[tile {b},{ty},{tx}]"
        if ref[b, ty, tx] == 0:
            bad = int((got[b, ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8] != 0).sum())
            rec = Rec(family, name, bad, 0.0, 0.0, exact=True)
            if bad:
                return rec
            continue
        rec = Rec(family, name, err[b, ty, tx], yard[b, ty, tx], factor * float(yard[b, ty, tx]) + FLOOR)
        if worst is None or rec.multiple > worst.multiple:
            worst = rec
    return worst


def exact(family, what, got, want):
    """mismatching elements (NaN never matches)"""
    got, want = torch.as_tensor(got), torch.as_tensor(want)
    return Rec(family, what, int((got != want.to(got.dtype).expand_as(got)).sum()), 0.0, 0.0, exact=True)


def hold(recs, verbose=True):
    for r in recs:
        if verbose and (not r.exact or not r.ok):
            print(r.line())
    bad = [r for r in recs if not r.ok]
    assert not bad, "; ".join(f"{r.family} {r.what}: " + (f"{int(r.err)} elements differ" if r.exact else
                                                           f"rel err {r.err:.3e} > bound {r.bound:.3e} (yard {r.yard:.3e})") for r in bad[:6])


def worst(recs):
    return max(recs, key=lambda r: r.multiple if not r.exact else (math.inf if r.err else 0.0))


# ------------------------------------------------------------------------------------------------------------------ checks
def check_fp32(be, r, shape, cstride, backward=True):
    """rpnet_local_corr_fwd / _bwd at one radius, shape and stride"""
    B, h, w, C = shape
    KK = (2 * r + 1) ** 2
    seed = case_seed(r, B, h, w, C, cstride)
    fam = f"fp32_r{r}"
    tag = f"{B}x{h}x{w}x{C}/s{cstride}"
    f1, f2 = make_operands(seed, shape, 0)
    recs = []
    corr = be.fwd32(f1, f2, r, cstride)
    r64, r32 = R.local_corr(f1, f2, r, cstride), R.local_corr(f1, f2, r, cstride, dtype=F32)
    recs.append(measure(fam, f"corr {tag}", corr, r64, r32))
    inside = inside_mask(h, w, r, cstride).expand(B, -1, -1, -1)
    recs.append(exact(fam, f"corr outside the image and pad channels {tag}", corr[~inside], 0.0))
    recs.append(exact(fam, f"corr of a zero f1 {tag}", be.fwd32(torch.zeros_like(f1), f2, r, cstride), 0.0))
    recs.append(exact(fam, f"corr of a zero f2 {tag}", be.fwd32(f1, torch.zeros_like(f2), r, cstride), 0.0))
    if not backward:
        return recs
    dcorr, add = rnd(seed + 2, B, h, w, cstride), rnd(seed + 3, *shape)        # the pad channels of dcorr hold values: they are ignored
    for a in (add, None):
        df1, df2 = be.bwd32(f1, f2, dcorr, r, cstride, a)
        (g1, g2), (q1, q2) = R.local_corr_bwd(f1, f2, dcorr, r, a), R.local_corr_bwd(f1, f2, dcorr, r, a, dtype=F32)
        how = "add" if a is not None else "noadd"
        recs += [measure(fam, f"df1({how}) {tag}", df1, g1, q1), measure(fam, f"df2({how}) {tag}", df2, g2, q2)]
        zero = torch.zeros_like(dcorr)
        zero[..., KK:] = dcorr[..., KK:]
        z1, z2 = be.bwd32(f1, f2, zero, r, cstride, a)
        recs += [exact(fam, f"df1({how}) of a zero dcorr {tag}", z1, a if a is not None else 0.0),
                 exact(fam, f"df2({how}) of a zero dcorr {tag}", z2, 0.0)]
    return recs


def check_split_fwd(be, planes, bhw, C, cstride):
    """rpnet_local_corr_split_fwd: with and without out_absmax and corr_planes (the three launches give the same fp32 tensor)"""
    B, h, w = bhw
    shape = (B, h, w, C)
    seed = case_seed(planes, B, h, w, C, cstride)
    fam, tag = f"split_fwd_p{planes}", f"{B}x{h}x{w}x{C}/s{cstride}"
    p1, p2, s1, s2 = make_operands(seed, shape, planes)
    v1, v2 = plane_values(p1, s1), plane_values(p2, s2)
    r64, r32 = R.local_corr(v1, v2, 5, cstride), R.local_corr(v1, v2, 5, cstride, dtype=F32)
    cscale = pow2_scale(4.0 * float(r64.abs().max())) if planes <= 2 else None        # a "predicted" scale: four times the maximum
    corr, amax, cpl = be.split_fwd(p1, p2, s1, s2, planes, shape, cstride, True, cscale)
    recs = [measure(fam, f"corr {tag}", corr, r64, r32, factor=MEASURED_FACTORS.get((planes, bhw, C, cstride), FACTOR))]
    inside = inside_mask(h, w, 5, cstride).expand(B, -1, -1, -1)
    recs.append(exact(fam, f"corr outside the image and pad channels {tag}", corr[~inside], 0.0))
    recs.append(exact(fam, f"out_absmax {tag}", amax, corr.abs().max()))
    if planes <= 2:
        recs.append(exact(fam, f"written planes {tag}", cpl, be.split_f16(corr, cscale, planes)))
        recs.append(exact(fam, f"written planes, pad channels {tag}", cpl[..., 121:], 0))
        c2, a2, _ = be.split_fwd(p1, p2, s1, s2, planes, shape, cstride, True, None)
        recs += [exact(fam, f"corr without planes {tag}", c2, corr), exact(fam, f"out_absmax without planes {tag}", a2, amax)]
    c3, _, _ = be.split_fwd(p1, p2, s1, s2, planes, shape, cstride, False, None)
    recs.append(exact(fam, f"corr without out_absmax {tag}", c3, corr))
    z = torch.zeros_like(p1)
    recs.append(exact(fam, f"corr of a zero f1 {tag}", be.split_fwd(z, p2, s1, s2, planes, shape, cstride, False, None)[0], 0.0))
    recs.append(exact(fam, f"corr of a zero f2 {tag}", be.split_fwd(p1, z, s1, s2, planes, shape, cstride, False, None)[0], 0.0))
    return recs


def _split_bwd_records(fam, tag, got, v1, v2, dcorr, planes, add, how, judge):
    df1, df2 = got
    (g1, g2), (q1, q2) = R.local_corr_bwd(v1, v2, dcorr, 5, add), R.local_corr_bwd(v1, v2, dcorr, 5, add, dtype=F32)
    x1 = split_term(dcorr, v2, 5, planes)
    x2 = split_term(transpose_window(dcorr.double(), 5), v1, 5, planes)
    return [judge(fam, f"df1({how}) {tag}", df1, g1, q1, extra=x1), judge(fam, f"df2({how}) {tag}", df2, g2, q2, extra=x2)]


def check_split_bwd(be, planes, bhw, C, cstride):
    """rpnet_local_corr_split_bwd with df1_add given and null"""
    B, h, w = bhw
    shape = (B, h, w, C)
    seed = case_seed(planes, B, h, w, C, cstride, 1)
    fam, tag = f"split_bwd_p{planes}", f"{B}x{h}x{w}x{C}/s{cstride}"
    p1, p2, s1, s2 = make_operands(seed, shape, planes)
    v1, v2 = plane_values(p1, s1), plane_values(p2, s2)
    dcorr, add = rnd(seed + 2, B, h, w, cstride), rnd(seed + 3, *shape)
    recs = []
    for a in (add, None):
        how = "add" if a is not None else "noadd"
        got = be.split_bwd(p1, p2, s1, s2, dcorr, planes, shape, cstride, a)
        recs += _split_bwd_records(fam, tag, got, v1, v2, dcorr, planes, a, how, measure)
        zero = torch.zeros_like(dcorr)
        zero[..., 121:] = dcorr[..., 121:]
        z1, z2 = be.split_bwd(p1, p2, s1, s2, zero, planes, shape, cstride, a)       # every tile hits the e < -100 clamp of pow2_scale
        recs += [exact(fam, f"df1({how}) of a zero dcorr {tag}", z1, a if a is not None else 0.0),
                 exact(fam, f"df2({how}) of a zero dcorr {tag}", z2, 0.0)]
    return recs


def check_dynamic_range(be, planes, C, cstride=128):
    """tiles of very different magnitude, an all-zero tile and a tile with one non-zero element: the error per tile"""
    shape = (2, 16, 16, C)
    seed = case_seed(planes, C, 77)
    fam, tag = f"split_bwd_p{planes}", f"dynamic 2x16x16x{C}/s{cstride}"
    p1, p2, s1, s2 = make_operands(seed, shape, planes)
    v1, v2 = plane_values(p1, s1), plane_values(p2, s2)
    dcorr = dynamic_dcorr(seed + 2, cstride)
    got = be.split_bwd(p1, p2, s1, s2, dcorr, planes, shape, cstride, None)
    return _split_bwd_records(fam, tag, got, v1, v2, dcorr, planes, None, "noadd", per_tile)


def cross_path_inputs():
    r, shape = CROSS_PATH
    seed = case_seed(r, *shape, 5)
    f1, f2 = make_operands(seed, shape, 0)
    return f1, f2, rnd(seed + 2, *shape[:3], 128), rnd(seed + 3, *shape)


def cross_path_records(what, corr, df1, df2, planes):
    """one path's (corr, df1 with the alias gradient summed, df2) against the float64 reference of the SAME fp32 inputs (three
    bf16 planes represent them exactly); planes: what the backward splits the window gradient into, 0 = not at all"""
    f1, f2, dcorr, add = cross_path_inputs()
    (g1, g2), (q1, q2) = R.local_corr_bwd(f1, f2, dcorr, 5, add), R.local_corr_bwd(f1, f2, dcorr, 5, add, dtype=F32)
    x1 = split_term(dcorr, f2, 5, planes) if planes else None
    x2 = split_term(transpose_window(dcorr.double(), 5), f1, 5, planes) if planes else None
    return [measure("cross", f"corr {what}", corr, R.local_corr(f1, f2, 5, 128), R.local_corr(f1, f2, 5, 128, dtype=F32)),
            measure("cross", f"df1 {what}", df1, g1, q1, extra=x1), measure("cross", f"df2 {what}", df2, g2, q2, extra=x2)]


def check_cross_path(be):
    f1, f2, dcorr, add = cross_path_inputs()
    shape = tuple(f1.shape)
    recs = cross_path_records("fp32", be.fwd32(f1, f2, 5, 128), *be.bwd32(f1, f2, dcorr, 5, 128, add), 0)
    p1, p2 = split_planes(f1, 3), split_planes(f2, 3)
    corr = be.split_fwd(p1, p2, None, None, 3, shape, 128, False, None)[0]
    return recs + cross_path_records("planes3", corr, *be.split_bwd(p1, p2, None, None, dcorr, 3, shape, 128, add), 3)


# --------------------------------------------------------------------------------------------------------------- refusals
def refusals(buf):
    """[(label, entry point, args without the stream, expected rpnet_status)]: every call is refused on the host.  buf(n) -> a
    valid buffer of n floats: every pointer is valid (unless the case is about null) and large enough for what the call claims."""
    B, h, w = 1, 8, 8
    px = B * h * w
    f1, f2, corr, dc, d1, d2, add, ws = (buf(px * 320) for _ in range(8))
    s1, s2, mx, cs, cpl = buf(4), buf(4), buf(4), buf(4), buf(px * 320)
    wsb = lambda cstride: px * cstride * 4          # noqa: E731  rpnet_local_corr_bwd_workspace_bytes

    def fwd(f1=f1, f2=f2, corr=corr, C=64, r=5, cstride=128):
        return ("rpnet_local_corr_fwd", (f1, f2, corr, B, h, w, C, r, cstride))

    def bwd(f1=f1, f2=f2, dc=dc, d1=d1, d2=d2, C=64, r=5, cstride=128, ws=ws, wb=None):
        return ("rpnet_local_corr_bwd", (f1, f2, dc, d1, d2, B, h, w, C, r, cstride, add, ws, wsb(cstride) if wb is None else wb))

    def sfwd(f1=f1, f2=f2, corr=corr, C=128, r=5, cstride=128, planes=3, s1=None, s2=None, cpl=None, cs=None):
        return ("rpnet_local_corr_split_fwd", (f1, f2, corr, B, h, w, C, r, cstride, planes, s1, s2, mx, cpl, cs))

    def sbwd(f1=f1, f2=f2, dc=dc, d1=d1, d2=d2, C=128, r=5, cstride=128, planes=3, s1=None, s2=None, ws=ws, wb=None):
        return ("rpnet_local_corr_split_bwd", (f1, f2, dc, d1, d2, B, h, w, C, r, cstride, planes, s1, s2, add, ws,
                                               wsb(cstride) if wb is None else wb))

    rows = [("radius 0", fwd(r=0), SHAPE), ("radius 8", fwd(r=8, cstride=256), SHAPE), ("C = 48", fwd(C=48), SHAPE),
            ("cstride < KK", fwd(cstride=120), SHAPE), ("cstride > 256", fwd(r=7, cstride=257), SHAPE),
            ("null f1", fwd(f1=None), ARG), ("null f2", fwd(f2=None), ARG), ("null corr", fwd(corr=None), ARG),
            ("radius 0", bwd(r=0), SHAPE), ("radius 8", bwd(r=8, cstride=300), SHAPE), ("C = 48", bwd(C=48), SHAPE),
            ("C = 96", bwd(C=96), SHAPE), ("cstride < KK", bwd(cstride=120), SHAPE),
            ("short workspace", bwd(wb=wsb(128) - 1), WORKSPACE), ("null f1", bwd(f1=None), ARG), ("null f2", bwd(f2=None), ARG),
            ("null dcorr", bwd(dc=None), ARG), ("null df1", bwd(d1=None), ARG), ("null df2", bwd(d2=None), ARG),
            ("null workspace", bwd(ws=None), ARG),
            ("radius 4", sfwd(r=4), SHAPE), ("C = 48", sfwd(C=48), SHAPE), ("cstride < KK", sfwd(cstride=120), SHAPE),
            ("cstride > 160", sfwd(cstride=161), SHAPE), ("planes 0", sfwd(planes=0), SHAPE), ("planes 4", sfwd(planes=4), SHAPE),
            ("fp16 planes without scales", sfwd(planes=2), SHAPE), ("one plane without scale2", sfwd(planes=1, s1=s1), SHAPE),
            ("corr_planes with three planes", sfwd(cpl=cpl, cs=cs), ARG),
            ("corr_planes without their scale", sfwd(planes=2, s1=s1, s2=s2, cpl=cpl), ARG),
            ("null f1", sfwd(f1=None), ARG), ("null f2", sfwd(f2=None), ARG), ("null corr", sfwd(corr=None), ARG),
            ("radius 4", sbwd(r=4), SHAPE), ("C = 64", sbwd(C=64), SHAPE), ("cstride < KK", sbwd(cstride=120), SHAPE),
            ("fp16 planes without scales", sbwd(planes=2), SHAPE), ("one plane without scale1", sbwd(planes=1, s2=s2), SHAPE),
            ("planes 4", sbwd(planes=4), SHAPE), ("short workspace", sbwd(wb=wsb(128) - 1), WORKSPACE),
            ("null f1", sbwd(f1=None), ARG), ("null dcorr", sbwd(dc=None), ARG), ("null df2", sbwd(d2=None), ARG),
            ("null workspace", sbwd(ws=None), ARG)]
    return [(label, entry, args, code) for label, (entry, args), code in rows], (corr, d1, d2, ws, cpl, mx)


# ----------------------------------------------------------------------------------------- the float32 stand-in for the library
DEFECTS = ["swap_ac", "right_border", "no_inv_sqrt_c", "unmirrored", "no_df1_add", "lowest_plane", "neighbour_scale"]


class SimBackend:
    """A float32 torch restatement of the five entry points, NOT the pairwise yardstick: the forward sums the channels in
    sequence, 32 at a time, the backward adds the window offsets in sequence; the split backward scales every 8 x 8 tile of the
    window gradient by its own power of two and rounds it to the plane format, as the kernel does.  `defect`: one of DEFECTS."""

    def __init__(self, defect=None):
        assert defect is None or defect in DEFECTS
        self.defect = defect

    # ---- arithmetic
    def _corr(self, f1, f2, r, cstride):
        B, h, w, C = f1.shape
        K = 2 * r + 1
        isc = 1.0 if self.defect == "no_inv_sqrt_c" else torch.tensor(1.0 / math.sqrt(C), dtype=F32)
        f2q = F.pad(f2, (0, 0, r + 1, r + 1, r, r))
        out = torch.zeros(B, h, w, cstride)
        if not f1.any() or not f2.any():            # sums of products with 0 (the operands are finite): 0, without the loops
            return out
        for a in range(K):
            for c in range(K):
                acc = torch.zeros(B, h, w)
                for c0 in range(0, C, 32):
                    win = f2q[:, c:c + h, a + 1:a + 1 + w, c0:c0 + 32]
                    if self.defect == "right_border":           # the last column reads its window one pixel to the left
                        win = torch.cat([win[:, :, :-1], f2q[:, c:c + h, a + w - 1:a + w, c0:c0 + 32]], 2)
                    acc = acc + (f1[..., c0:c0 + 32] * win).sum(-1)
                out[..., c * K + a if self.defect == "swap_ac" else a * K + c] = acc * isc
        return out

    def _pass(self, g, fo, r, sign):
        """df[p, ch] = sum_o g[p, o] fo[p + sign off(o), ch]"""
        B, h, w, C = fo.shape
        K = 2 * r + 1
        fop = F.pad(fo, (0, 0, r, r, r, r))
        acc = torch.zeros(B, h, w, C)
        if not g[..., :K * K].any():
            return acc
        for a in range(K):
            for c in range(K):
                dy, dx = r + sign * (c - r), r + sign * (a - r)
                acc = acc + g[..., a * K + c, None] * fop[:, dy:dy + h, dx:dx + w]
        return acc

    def _bwd(self, f1, f2, dcorr, r, add, planes=0):
        C = f1.shape[-1]
        isc = torch.tensor(1.0 / math.sqrt(C), dtype=F32)
        g, gt = dcorr, transpose_window(dcorr, r)
        if planes:
            g, gt = self._split_gradient(g * isc, planes), self._split_gradient(gt * isc, planes)
            isc = 1.0
        df1 = self._pass(g, f2, r, 1) * isc
        df2 = self._pass(gt, f1, r, 1 if self.defect == "unmirrored" else -1) * isc
        if add is not None and self.defect != "no_df1_add":
            df1 = df1 + add
        return df1, df2

    def _split_gradient(self, g, planes):
        """what the sum of the planes of the scaled window gradient represents, tile by tile"""
        if planes == 3:
            return g
        B, h, w, _ = g.shape
        tm = tile_max(g)
        sg = torch.tensor([[[pow2_scale(float(v)) for v in row] for row in img] for img in tm], dtype=F32)
        if self.defect == "neighbour_scale" and sg.shape[2] > 1:
            sg[0, 0, 0] = sg[0, 0, 1]
        sg = to_pixels(sg, h, w)[..., None]
        v = g / sg
        hi = v.half().float()
        return (hi if planes == 1 else hi + (v - hi).half().float()) * sg

    def _values(self, bits, scale):
        if self.defect == "lowest_plane" and bits.shape[0] == 3:
            bits = bits[:2]
            return bits.view(torch.bfloat16).float().sum(0)
        return plane_values(bits, scale, dtype=F32)

    # ---- the entry points
    def fwd32(self, f1, f2, r, cstride):
        return self._corr(f1, f2, r, cstride)

    def bwd32(self, f1, f2, dcorr, r, cstride, add):
        return self._bwd(f1, f2, dcorr, r, add)

    def split_f16(self, x, scale, planes):
        return split_planes(x, planes, scale)

    def split_fwd(self, p1, p2, s1, s2, planes, shape, cstride, want_absmax, cscale):
        corr = self._corr(self._values(p1, s1), self._values(p2, s2), 5, cstride)
        return corr, (corr.abs().max().reshape(1) if want_absmax else None), (None if cscale is None else split_planes(corr, planes, cscale))

    def split_bwd(self, p1, p2, s1, s2, dcorr, planes, shape, cstride, add):
        return self._bwd(self._values(p1, s1), self._values(p2, s2), dcorr, 5, add, planes)
