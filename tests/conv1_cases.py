"""Cases and comparison functions shared by tests/test_host_conv1_ref64.py and tests/test_gpu_conv1_fp64.py: the first-layer (Cin = 1)
kernels of csrc/conv_first.hip (rpnet_conv1_fwd, rpnet_conv1_bn_relu, rpnet_conv1_bn_bwd_partial, rpnet_conv1_wgrad_bn,
rpnet_conv1_dgrad_bn, with rpnet_bn_relu and rpnet_bn_bwd(given_partial) beside them) against the float64 references of
tests/ref64.py (conv1, conv1_affine_relu, bn_bwd_sums, bn_dy, conv1_dgrad, conv_wgrad) at every branch of their dispatch.  The layout
is that of tests/wgrad_cases.py; the definitions of tests/corr_cases.py (FACTOR, FLOOR, Rec, exact, hold, case_seed, pow2_scale,
split_planes, plane_values, split_unit_roundoff) are used, not restated.

A *backend* runs one entry point on CPU tensors and returns CPU tensors: the HIP library (the GPU test) or SimBackend, a float32
torch restatement with or without a seeded defect (the host test).

Bound of an arithmetic result: rel_err(got, r64) <= FACTOR * yard + FLOOR, yard = rel_err(r32, r64), r32 the same ref64 functions at
float32.  y and z are judged over the tensor and per output channel, dW per tap, dx per image (per_slice: relative to the slice's own
reference maximum; a slice whose reference is all zero must be exactly zero).

The ReLU switch m = [y scale + shift > 0] is discrete: the reference evaluates it in float64 on the fp32 bits of y that the kernels
use (rpnet_conv1_fwd at the same shape, or the y handed in).  An element is undecided when |y scale + shift| <= 4 * 2^-24 (|y scale| +
|shift|): a fused and an unfused fp32 evaluation of y scale + shift differ from the exact value by at most 2 * 2^-24 of that sum, so a
decided element has one sign in all three.  Every row's seed leaves NO element undecided; the checks assert that on the backend's own
y before they compare anything (assert_decided) and never drop an element.

The fp64 partial rows (stats_partial of rpnet_conv1_fwd, partial of rpnet_conv1_bn_bwd_partial) are sums in double of fp32 terms: the
sum over a group's rows is held to the float64 sum of the same terms within n 2^-52 sum |term| (n terms; each of the n - 1 double
additions rounds by at most 2^-53 of a partial sum), per group, so that a row holding another group's pixels shows.  The second
moment sum dz m xhat has xhat = (y - mean) invstd formed in fp32 (a subtraction, a product, and the fp32 value of the product with dz m
is exact in double): 3 * 2^-24 sum |dz m xhat| more.

Exact checks (impulses, bit-identical pairs, second identical call, out_absmax, plane round-off, guard words) count mismatching
elements and allow none."""
import math

import torch
import torch.nn.functional as F

from tests import corr_cases as CC
from tests import ref64 as R
from tests.corr_cases import ARG, FACTOR, FLOOR, SHAPE, WORKSPACE, case_seed, plane_values, pow2_scale, split_planes, split_unit_roundoff  # noqa: F401
from tests.helpers import rnd

F32, F64 = torch.float32, torch.float64
GUARD = 64                      # words behind a workspace / a partial array that must come back as they went in
NAN = float("nan")
U32 = 2.0 ** -24                # unit round-off of fp32
UNDECIDED = 4 * U32             # the ReLU switch (module docstring)
STATS_PIXELS, STATS_CAP = 512, 2048          # rpnet_conv1_stats_blocks: pixels per partial row, rows per group at most
WGRAD_BLOCKS = 1024             # kConv1WgradBlocks
FWD_BLOCKS, BN_RELU_BLOCKS = 16384, 8192      # grid caps of the plain forward and of rpnet_conv1_bn_relu
# A check that needs more than the plain bound: (row id, what) -> factor, twice its measured ratio, the reason beside it
# (profiles/conv1_parity.txt holds the measurement).  Empty: no check needs one.
MEASURED_FACTORS = {}

# every kernel (template instantiation) of csrc/conv_first.hip; the two <false, *> weight-gradient forms belong to rpnet_conv1_wgrad
# and are the rows of tests/wgrad_cases.py CONV1
KERNELS = (["conv1_fwd_kernel", "conv1_fwd4_kernel", "conv1_bn_bwd_partial_kernel", "conv1_bn_bwd_partial4_kernel", "conv1_wgrad_final"]
           + [f"conv1_bn_relu{s}_kernel<{p}>" for s in ("", "4") for p in (1, 2, 3)]
           + [f"conv1_wgrad_partial{s}<true,{rc}>" for s in ("", "4") for rc in ("false", "true")]
           + [f"conv1_dgrad_bn_kernel<{rc}>" for rc in ("false", "true")])
KERNELS_OF_WGRAD_CASES = ["conv1_wgrad_partial<false,false>", "conv1_wgrad_partial4<false,false>"]


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------------- rows
class Row:
    """one table row.  entry: fwd | bn_relu | bwd_partial | wgrad_bn | dgrad_bn; y: "given" | "null" (the two gradients: y handed in, or
    made again from the image); kernel: what the launch is meant to reach (route() restates the launcher's conditions); seed: operands
    for which no element of the ReLU switch is undecided."""

    def __init__(self, entry, nhwg, cout, kernel, y="null", seed=1):
        self.entry, (self.N, self.H, self.W, self.groups), self.cout, self.kernel, self.y, self.seed = entry, nhwg, cout, kernel, y, seed

    M = property(lambda s: s.N * s.H * s.W)
    Mg = property(lambda s: s.M // s.groups)

    @property
    def id(self):
        return (f"{self.entry}-{self.N}x{self.H}x{self.W}-c{self.cout}" + (f"-g{self.groups}" if self.groups > 1 else "")
                + (f"-y{self.y}" if self.entry in ("wgrad_bn", "dgrad_bn") else ""))


def strips_ok(N, H, W, groups):
    """conv1_strips_ok: the four-pixel strip kernels"""
    return W % 4 == 0 and groups >= 1 and N % groups == 0 and N * H * W < 2 ** 31


def stats_blocks(N, H, W, groups):
    """rpnet_conv1_stats_blocks = rpnet_conv1_bn_bwd_rows: partial rows per group"""
    if groups < 1 or N % groups:
        return 0
    return min(_cdiv((N // groups) * H * W, STATS_PIXELS), STATS_CAP)


def route(r):
    """the kernel the launchers of csrc/conv_first.hip pick for a row; a forward row's launches (plain, epilogue, out_absmax, fused
    statistics with y written and with y == NULL) are all this one kernel"""
    return _named(r.entry, strips_ok(r.N, r.H, r.W, r.groups), r.y)


def kernels_named(rows):
    out = set()
    for r in rows:
        if r.entry == "bn_relu":
            out |= {r.kernel.replace("<1,2,3>", f"<{p}>") for p in (1, 2, 3)}
        else:
            out.add(r.kernel)
        if r.entry == "wgrad_bn":
            out.add("conv1_wgrad_final")
    return out


def blocks(r):
    """(threads per pixel, pixels or strips per block, blocks of the launch) as the launchers compute them: what the comments of
    the tables state"""
    q = r.cout // (8 if r.entry == "bn_relu" else 4)
    ppb = 256 // q
    s = strips_ok(r.N, r.H, r.W, r.groups)
    if r.entry == "fwd":
        nb = _cdiv(r.M, ppb)
        return q, ppb, min(_cdiv(nb, 4) if s else nb, FWD_BLOCKS)
    if r.entry == "bn_relu":
        nb = max(1, min(_cdiv(r.M, ppb * 4), BN_RELU_BLOCKS))
        return q, ppb, _cdiv(nb, 4) if s else nb
    if r.entry == "bwd_partial":
        return q, ppb, stats_blocks(r.N, r.H, r.W, r.groups)
    if r.entry == "wgrad_bn":
        return q, ppb, max(1, min(_cdiv(r.Mg, ppb), WGRAD_BLOCKS // r.groups))
    return 32, 256, _cdiv(r.W, 16) * _cdiv(r.H, 16) * r.N


# N, H, W, groups.  Strips (W % 4 == 0):
STRIP_SHAPES = [(1, 1, 4, 1),            # one strip: row[-1] and row[4] both off, every row above and below outside
                (1, 2, 8, 1),            # two strips per row: one edge load on in each
                (2, 16, 24, 1),          # 768 pixels: two partial rows of 96 strips each
                (2, 16, 24, 2),          # a statistic group = one image
                (3, 5, 12, 1),           # 45 strips: no multiple of any block's strips
                (4, 8, 8, 1), (4, 8, 8, 2), (4, 8, 8, 4)]
# per pixel (W % 4 != 0):
PIXEL_SHAPES = [(1, 1, 1, 1),            # one pixel: only the centre tap inside
                (1, 1, 3, 1), (1, 3, 1, 1),          # one row, one column
                (2, 7, 5, 1), (2, 7, 5, 2),          # 35 pixels per image: a group boundary inside a block's pixel range
                (3, 37, 21, 1),          # 2331 pixels: five partial rows, the last 463 pixels long
                (3, 37, 21, 3),          # 777 pixels per group: two rows of 389 and 388, group boundaries at no multiple of 256
                (1, 25, 41, 1),          # 1025 pixels: three rows of 342, 342 and 341
                (4, 9, 6, 1), (4, 9, 6, 2), (4, 9, 6, 4)]
SHAPES = STRIP_SHAPES + PIXEL_SHAPES
# the shapes that every channel count other than the model's runs at: strips and pixels with two groups, and the five-row image
COUT_SHAPES = [(4, 8, 8, 2), (2, 7, 5, 2), (3, 37, 21, 1)]


def _named(entry, strips, y):
    """the table's kernel column, from the list a shape stands in (route() is held against it)"""
    s, rc = "4" if strips else "", "true" if y == "null" else "false"
    return {"fwd": f"conv1_fwd{s}_kernel", "bn_relu": f"conv1_bn_relu{s}_kernel<1,2,3>", "bwd_partial": f"conv1_bn_bwd_partial{s}_kernel",
            "wgrad_bn": f"conv1_wgrad_partial{s}<true,{rc}>", "dgrad_bn": f"conv1_dgrad_bn_kernel<{rc}>"}[entry]


def _table(entry, model_cout, other_couts, y="null"):
    return ([Row(entry, s, model_cout, _named(entry, s in STRIP_SHAPES, y), y=y) for s in SHAPES]
            + [Row(entry, s, c, _named(entry, s in STRIP_SHAPES, y), y=y) for c in other_couts for s in COUT_SHAPES])


# rpnet_conv1_fwd, cout 4 .. 1024: 1 .. 256 threads per pixel, 256 .. 1 pixels (strips) per block
FWD = _table("fwd", 64, (4, 16, 256, 1024))
# rpnet_conv1_bn_relu, cout 8 .. 1024 (eight channels per thread): planes 3, 2, 1, z given and NULL in every row
BN_RELU = _table("bn_relu", 64, (8, 1024))
# rpnet_conv1_bn_bwd_partial, then rpnet_bn_bwd on its rows
BWD_PARTIAL = _table("bwd_partial", 64, (4, 16, 256, 1024))
# rpnet_conv1_wgrad_bn, cout 4 .. 256
WGRAD_BN = _table("wgrad_bn", 64, (4, 256), y="given") + _table("wgrad_bn", 64, (4, 256), y="null")
# rpnet_conv1_dgrad_bn, multiples of 32 up to 256; 96 and 160 are channel chunks that rpnet_conv1_fwd cannot make (256 % (cout / 4) != 0):
# their y is the float64 reference's, rounded
DGRAD_BN = _table("dgrad_bn", 32, (96, 160, 256), y="given") + _table("dgrad_bn", 32, (64, 128, 256), y="null")
TABLES = {"fwd": FWD, "bn_relu": BN_RELU, "bwd_partial": BWD_PARTIAL, "wgrad_bn": WGRAD_BN, "dgrad_bn": DGRAD_BN}
# seeds other than 1: the rows whose first operands leave an element of the ReLU switch undecided (tests/test_host_conv1_ref64.py
# shows that none is left)
SEEDS = {"bwd_partial-3x37x21-c256": 2, "wgrad_bn-3x37x21-c256-ygiven": 2, "wgrad_bn-3x37x21-c256-ynull": 2, "dgrad_bn-3x37x21-c256-ygiven": 2,
         "dgrad_bn-3x37x21-c256-ynull": 2, "dgrad_bn-4x8x8-c128-g2-ynull": 3}
for _t in TABLES.values():
    for _r in _t:
        _r.seed = SEEDS.get(_r.id, 1)
ALL_ROWS = [r for t in TABLES.values() for r in t]

# the block caps, one row each (the only rows above 100 K pixels)
CAP_STATS = Row("fwd", (1, 1024, 1028, 1), 4, "conv1_fwd4_kernel")                  # 1052672 pixels / 512 = 2056 rows -> 2048
CAP_WGRAD = Row("wgrad_bn", (1, 512, 516, 1), 4, "conv1_wgrad_partial4<true,true>")  # 264192 pixels / 256 per block = 1032 blocks -> 1024
CAP_WRAP = Row("fwd", (1, 127, 131, 1), 1024, "conv1_fwd_kernel")                  # 16637 blocks of one pixel -> 16384: 253 pixels on the second lap
CAPS = [CAP_STATS, CAP_WGRAD, CAP_WRAP]


# ---------------------------------------------------------------------------------------------------------------- operands
class Ops:
    pass


def make_stats(y64, gamma, beta, groups):
    """stats [4][groups][C] fp32 = scale, shift, mean, invstd: the batch statistics of y per group (eps 1e-5); a group of fewer than 32
    pixels has no meaningful variance (one pixel: 0, invstd = 316 and y scale + shift all cancellation), it gets mean = a quarter of a
    normal draw and invstd in 0.5 .. 2.5 instead"""
    C = y64.shape[-1]
    yg = y64.reshape(groups, -1, C)
    if yg.shape[1] >= 32:
        mean, invstd = yg.mean(1), (yg.var(1, unbiased=False) + 1e-5).rsqrt()
    else:
        mean, invstd = 0.25 * rnd(77, groups, C).double(), 0.5 + rnd(78, groups, C).double().abs().clamp_max(2.0)
    scale = gamma.double() * invstd
    return torch.stack([scale, beta.double() - mean * scale, mean, invstd]).float().contiguous()


def operands(r, key=0):
    seed = case_seed(r.N, r.H, r.W, r.cout, r.groups, r.seed, key)
    o = Ops()
    o.x, o.w, o.bias = rnd(seed, r.N, r.H, r.W), rnd(seed + 1, r.cout, 1, 3, 3) / 3.0, 0.1 * rnd(seed + 2, r.cout)
    o.gamma, o.beta = 1.0 + 0.1 * rnd(seed + 3, r.cout), 0.1 * rnd(seed + 4, r.cout)
    o.dz = 0.5 * rnd(seed + 5, r.N, r.H, r.W, r.cout)
    o.y64 = R.conv1(o.x, o.w, o.bias)
    o.stats = make_stats(o.y64, o.gamma, o.beta, r.groups)
    return o


def fwd_accepts(cout):
    return cout % 4 == 0 and cout <= 1024 and 256 % (cout // 4) == 0


def kernel_y(be, r, o):
    """the fp32 bits of y that the kernels use: rpnet_conv1_fwd at the same shape (a cout it refuses: the reference's, rounded)"""
    if not fwd_accepts(r.cout):
        return o.y64.float()
    return be.fwd(r, o.x, o.w, o.bias).y


def undecided(y32, stats, groups, margin=UNDECIDED):
    st = stats.double().reshape(4, groups, -1)
    ys = y32.double() * R._per_image(st[0], y32.shape[0])
    sh = R._per_image(st[1], y32.shape[0])
    return int(((ys + sh).abs() <= margin * (ys.abs() + sh.abs())).sum())


def assert_decided(r, y32, stats):
    n = undecided(y32, stats, r.groups)
    assert n == 0, f"{r.id} seed {r.seed}: {n} elements of the ReLU switch are undecided on the y of this backend"


def coef_of(r, o, y32):
    """coef [groups][C][2] fp32 = the reduction's sums over the group's pixel count, as rpnet_bn_bwd leaves them"""
    s1, s2 = R.bn_bwd_sums(o.dz, y32, o.stats, r.groups)
    return (torch.stack([s1, s2], -1) / r.Mg).float().contiguous()


# ----------------------------------------------------------------------------------------------------------------- records
class Rec(CC.Rec):
    def line(self):
        return (f"PARITY conv1 {self.family} {self.what} err={self.err:.3e} yard={self.yard:.3e} ratio={self.ratio:.2f} "
                f"of_bound={self.multiple:.3f}")


def _factor(r, what):
    return MEASURED_FACTORS.get((r.id, what), FACTOR)


def whole(r, what, got, r64, r32):
    rec = CC.measure(r.id, what + " whole", got, r64, r32, factor=_factor(r, what + " whole"))
    rec.__class__ = Rec
    return rec


def per_slice(r, what, got, r64, r32, dim, name):
    """the bound per slice along `dim` (output channel, tap, image), relative to the slice's own reference maximum: the record of the
    worst slice.  A slice whose reference is all zero must be exactly zero."""
    tag = f"{what} per {name}"
    if not torch.isfinite(got).all():
        return Rec(r.id, tag, math.inf, 0.0, FLOOR)
    fl = lambda t: t.double().movedim(dim, 0).reshape(t.shape[dim], -1)         # noqa: E731
    g, a, b = fl(got), fl(r64), fl(r32)
    ref, err, yard = a.abs().amax(1), (g - a).abs().amax(1), (b - a).abs().amax(1)
    zero = ref == 0
    bad = int((g[zero] != 0).sum())
    if bad:
        return Rec(r.id, f"{tag}[a zero {name}]", bad, 0.0, 0.0, exact=True)
    if bool(zero.all()):
        return Rec(r.id, tag, 0.0, 0.0, FLOOR)
    ref = ref.masked_fill(zero, 1.0)
    e, y = (err / ref).masked_fill(zero, 0.0), (yard / ref).masked_fill(zero, 0.0)
    bound = _factor(r, tag) * y + FLOOR
    i = int((e / bound).argmax())
    return Rec(r.id, f"{tag}[{name} {i}]", e[i], y[i], bound[i])


def within(r, what, got, want, allow):
    """|got - want| <= allow element by element (float64; allow == 0: equal): the largest multiple of its allowance, bound 1"""
    got, want = got.double(), want.double()
    if not torch.isfinite(got).all():
        return Rec(r.id, what, math.inf, 0.0, 1.0)
    d = (got - want).abs()
    bad = int(((allow == 0) & (d != 0)).sum())
    if bad:
        return Rec(r.id, what + " [no allowance]", bad, 0.0, 0.0, exact=True)
    return Rec(r.id, what, float((d / allow.clamp_min(1e-300)).max()), 0.0, 1.0)


def exact(r, what, got, want):
    rec = CC.exact(r.id, what, got, want)
    rec.__class__ = Rec
    return rec


def bits_equal(r, what, got, want):
    """bit for bit (NaN equals the same NaN)"""
    v = lambda t: t.contiguous().view(torch.int64 if t.dtype == F64 else torch.int32 if t.dtype == F32 else t.dtype)         # noqa: E731
    if got.shape != want.shape:
        return Rec(r.id, what + " (shape)", 1, 0.0, 0.0, exact=True)
    return exact(r, what, v(got), v(want))


hold = CC.hold


def judge_nhwc(r, what, got, r64, r32):
    return [whole(r, what, got, r64, r32), per_slice(r, what, got, r64, r32, -1, "channel")]


# ------------------------------------------------------------------------------------------------------------------ checks
def _sums_records(r, what, part, want, terms_abs, extra=None):
    """part [groups, rows, C]: the sum over a group's rows against want [groups, C] within n 2^-52 sum |term| (+ extra)"""
    allow = r.Mg * 2.0 ** -52 * terms_abs
    if extra is not None:
        allow = allow + extra
    return within(r, what, part.sum(1), want, allow)


def check_fwd(be, r, caps_only=False):
    """rpnet_conv1_fwd: plain with and without bias, the eval-mode epilogue, out_absmax, the fused statistics with y written and
    with y == NULL"""
    o = operands(r)
    r64, r32 = o.y64, R.conv1(o.x, o.w, o.bias, dtype=F32)
    plain = be.fwd(r, o.x, o.w, o.bias)
    recs = judge_nhwc(r, "y", plain.y, r64, r32) + [bits_equal(r, "y, second identical call", be.fwd(r, o.x, o.w, o.bias).y, plain.y)]
    if r is CAP_WRAP:
        return recs
    G, C = r.groups, r.cout
    if not caps_only:
        recs += judge_nhwc(r, "y without bias", be.fwd(r, o.x, o.w, None).y, R.conv1(o.x, o.w, None), R.conv1(o.x, o.w, None, dtype=F32))
        sc, sh = o.stats[0, 0], o.stats[1, 0]
        ep = be.fwd(r, o.x, o.w, o.bias, ep=(sc, sh), absmax=0.0)
        recs += judge_nhwc(r, "epilogue z", ep.y, R.conv1_affine_relu(r64, sc, sh), R.conv1_affine_relu(r32, sc, sh, dtype=F32))
        recs.append(exact(r, "out_absmax of the epilogue form", ep.absmax, ep.y.abs().max()))
        am = be.fwd(r, o.x, o.w, o.bias, absmax=0.0)
        top = float(plain.y.abs().max())
        recs += [bits_equal(r, "y with out_absmax", am.y, plain.y), exact(r, "out_absmax", am.absmax, top),
                 exact(r, "a larger out_absmax is left alone", be.fwd(r, o.x, o.w, o.bias, absmax=2.0 * top).absmax, 2.0 * top)]
    both, only = be.fwd(r, o.x, o.w, o.bias, stats=True), be.fwd(r, o.x, o.w, o.bias, stats=True, write_y=False)
    recs += [bits_equal(r, "y beside the fused statistics", both.y, plain.y), bits_equal(r, "statistics rows with y == NULL", only.part, both.part),
             bits_equal(r, "statistics rows, second identical call", be.fwd(r, o.x, o.w, o.bias, stats=True, write_y=False).part, only.part)]
    assert only.part.shape == (G, stats_blocks(r.N, r.H, r.W, G), C, 2), (r.id, only.part.shape)
    yg = plain.y.double().reshape(G, -1, C)
    recs += [_sums_records(r, "sum y over a group's rows", only.part[..., 0], yg.sum(1), yg.abs().sum(1)),
             _sums_records(r, "sum y^2 over a group's rows", only.part[..., 1], (yg * yg).sum(1), (yg * yg).sum(1))]
    return recs


def check_bn_relu(be, r):
    """rpnet_conv1_bn_relu on planes 3, 2, 1 with z given and NULL against rpnet_bn_relu on the y of rpnet_conv1_fwd (bit for bit),
    ref64.conv1_affine_relu (the bound) and the values the planes represent (split_unit_roundoff)"""
    o = operands(r)
    y32 = kernel_y(be, r, o)
    sc, sh = o.stats[0], o.stats[1]
    r64 = R.conv1_affine_relu(o.y64, sc, sh, r.groups)
    r32 = R.conv1_affine_relu(R.conv1(o.x, o.w, o.bias, dtype=F32), sc, sh, r.groups, dtype=F32)
    recs = []
    for planes in (3, 2, 1):
        for want_z in (True, False):
            a = be.conv1_bn_relu(r, o.x, o.w, o.bias, sc, sh, planes, want_z, o.gamma, o.beta)
            b = be.bn_relu(r, y32, sc, sh, planes, want_z, o.gamma, o.beta)
            tag = f"planes {planes}" + ("" if want_z else ", z NULL")
            recs.append(bits_equal(r, f"{tag}: the planes of rpnet_bn_relu", a.planes, b.planes))
            if planes <= 2:
                recs.append(bits_equal(r, f"{tag}: split_scale of rpnet_bn_relu", a.scale, b.scale))
            if not want_z:
                recs.append(bits_equal(r, f"{tag}: z stays as found", a.z, torch.full_like(a.z, NAN)))
                continue
            recs.append(bits_equal(r, f"{tag}: z of rpnet_bn_relu", a.z, b.z))
            s = float(a.scale) if planes <= 2 else None
            top = s * 2.0 ** 15 if planes <= 2 else float(a.z.abs().max())
            d = (plane_values(a.planes, s) - a.z.double()).abs()
            recs.append(exact(r, f"{tag}: the planes represent z within split_unit_roundoff", d > split_unit_roundoff(planes) * top, False))
            if planes == 3:
                recs += judge_nhwc(r, "z", a.z, r64, r32)
                again = be.conv1_bn_relu(r, o.x, o.w, o.bias, sc, sh, planes, want_z, o.gamma, o.beta)
                recs += [bits_equal(r, "z, second identical call", again.z, a.z), bits_equal(r, "planes, second identical call", again.planes, a.planes)]
    return recs


def check_bwd_partial(be, r):
    """rpnet_conv1_bn_bwd_partial, then rpnet_bn_bwd(y = NULL, dy = dy_split = NULL, given_partial, given_rows)"""
    o = operands(r)
    y32 = kernel_y(be, r, o)
    assert_decided(r, y32, o.stats)
    G, C = r.groups, r.cout
    part = be.bwd_partial(r, o.x, o.w, o.bias, o.dz, o.stats)
    assert part.shape == (G, stats_blocks(r.N, r.H, r.W, G), C, 2), (r.id, part.shape)
    recs = [bits_equal(r, "partial rows, second identical call", be.bwd_partial(r, o.x, o.w, o.bias, o.dz, o.stats), part)]
    s1, s2 = R.bn_bwd_sums(o.dz, y32, o.stats, G)
    dm, xhat, _ = R._bn_terms(o.dz, y32, o.stats, G, F64)
    a1, a2 = dm.abs().reshape(G, -1, C).sum(1), (dm * xhat).abs().reshape(G, -1, C).sum(1)
    recs += [_sums_records(r, "sum dz m over a group's rows", part[..., 0], s1, a1),
             _sums_records(r, "sum dz m xhat over a group's rows", part[..., 1], s2, a2, extra=3 * U32 * a2)]
    t1, t2 = R.bn_bwd_sums(o.dz, y32, o.stats, G, dtype=F32)
    fin = be.bn_bwd_given(r, o.dz, o.stats, part)
    cf64, cf32 = torch.stack([s1, s2], -1) / r.Mg, torch.stack([t1, t2], -1) / r.Mg
    recs += [whole(r, "dgamma", fin.dgamma, s2.sum(0), t2.sum(0)), whole(r, "dbeta", fin.dbeta, s1.sum(0), t1.sum(0)),
             whole(r, "coef c1", fin.coef[..., 0], cf64[..., 0], cf32[..., 0]), whole(r, "coef c2", fin.coef[..., 1], cf64[..., 1], cf32[..., 1])]
    return recs


def _dy_refs(r, o, y32, coef):
    return R.bn_dy(o.dz, y32, o.stats, coef, r.groups), R.bn_dy(o.dz, y32, o.stats, coef, r.groups, dtype=F32)


def check_wgrad_bn(be, r):
    """rpnet_conv1_wgrad_bn against ref64.conv_wgrad of ref64.bn_dy, per tap; y == NULL bit for bit the y-given form"""
    o = operands(r)
    y32 = kernel_y(be, r, o)
    assert_decided(r, y32, o.stats)
    coef = coef_of(r, o, y32)
    d64, d32 = _dy_refs(r, o, y32, coef)
    r64, r32 = R.conv_wgrad(o.x[..., None], None, d64), R.conv_wgrad(o.x[..., None], None, d32, dtype=F32)
    null = r.y == "null"
    got = be.wgrad_bn(r, o.x, o.dz, None if null else y32, o.stats, coef, o.w, o.bias)
    again = be.wgrad_bn(r, o.x, o.dz, None if null else y32, o.stats, coef, o.w, o.bias)
    flat = lambda t: t.reshape(r.cout, 9)         # noqa: E731
    recs = [per_slice(r, "dW", flat(got), flat(r64), flat(r32), 1, "tap"), whole(r, "dW", got, r64, r32),
            bits_equal(r, "dW, second identical call", again, got)]
    if null:
        recs.append(bits_equal(r, "dW with y == NULL is dW with y given", got, be.wgrad_bn(r, o.x, o.dz, y32, o.stats, coef, o.w, o.bias)))
    return recs


def check_dgrad_bn(be, r):
    """rpnet_conv1_dgrad_bn against ref64.conv1_dgrad of ref64.bn_dy, per image; y == NULL bit for bit the y-given form (where
    rpnet_conv1_fwd makes that y); coef == NULL: the eval form"""
    o = operands(r)
    y32 = kernel_y(be, r, o)
    assert_decided(r, y32, o.stats)
    coef = coef_of(r, o, y32)
    null = r.y == "null"
    recs = []
    for cf, tag in ((coef, "dx"), (None, "dx, coef NULL")):
        d64, d32 = _dy_refs(r, o, y32, cf)
        r64, r32 = R.conv1_dgrad(d64, o.w), R.conv1_dgrad(d32, o.w, dtype=F32)
        got = be.dgrad_bn(r, o.dz, None if null else y32, o.stats, cf, o.w, o.bias, o.x)
        recs += [per_slice(r, tag, got, r64, r32, 0, "image"), whole(r, tag, got, r64, r32)]
        if cf is not None:
            recs.append(bits_equal(r, "dx, second identical call", be.dgrad_bn(r, o.dz, None if null else y32, o.stats, cf, o.w, o.bias, o.x), got))
            if null:
                recs.append(bits_equal(r, "dx with y == NULL is dx with y given", got, be.dgrad_bn(r, o.dz, y32, o.stats, cf, o.w, o.bias, None)))
    return recs


CHECKS = {"fwd": check_fwd, "bn_relu": check_bn_relu, "bwd_partial": check_bwd_partial, "wgrad_bn": check_wgrad_bn, "dgrad_bn": check_dgrad_bn}


def check_row(be, r):
    assert route(r) == r.kernel, f"{r.id}: the launcher takes {route(r)}, the table says {r.kernel}"
    return CHECKS[r.entry](be, r)


def check_cap(be, r):
    assert route(r) == r.kernel, f"{r.id}: the launcher takes {route(r)}, the table says {r.kernel}"
    if r.entry == "fwd":
        return check_fwd(be, r, caps_only=True)
    return check_wgrad_bn(be, r)


# ---------------------------------------------------------------------------------------------------------------- impulses
# (N, H, W): W = 4: one strip per row, row[-1] and row[4] both off; W = 8: both on (one each in the two strips of a row); W = 5: per pixel
IMPULSE_SHAPES = [(2, 3, 4), (2, 3, 8), (2, 3, 5)]
IMPULSE_COUT = 8
DGRAD_IMPULSE_SHAPE, DGRAD_IMPULSE_COUT = (2, 17, 33), 32


def impulse_filter(cout):
    """nine distinct powers of two per channel (2^-4 .. 2^4 by tap, times 2^(c % 3))"""
    w = 2.0 ** (torch.arange(9.0) - 4).reshape(1, 1, 3, 3) * 2.0 ** (torch.arange(cout) % 3).reshape(cout, 1, 1, 1).float()
    return w.contiguous()


def impulse_positions(N, H, W):
    """an interior pixel, the four corners, the last pixel of a row and the first of the next, the last pixel of an image and the
    first of the next"""
    pos = [(0, H // 2, W // 2), (0, 0, 0), (0, 0, W - 1), (0, H - 1, 0), (0, H - 1, W - 1), (0, 1, 0), (N - 1, 0, 0), (N - 1, H - 1, W - 1),
           (N - 1, 1, W - 1)]
    return list(dict.fromkeys(pos))


def check_impulses(be, nhw):
    """one power of two in x, a filter of nine distinct powers of two, zero bias: every y is one product of powers of two or zero"""
    N, H, W = nhw
    r = Row("fwd", (N, H, W, 1), IMPULSE_COUT, "")
    w, recs = impulse_filter(r.cout), []
    for i, (n, y, x) in enumerate(impulse_positions(N, H, W)):
        img = torch.zeros(N, H, W)
        img[n, y, x] = 2.0 ** (i % 5 - 2)
        want = R.conv1(img, w, None)
        assert int((want != 0).sum()) == r.cout * len([1 for dy in (-1, 0, 1) for dx in (-1, 0, 1) if 0 <= y + dy < H and 0 <= x + dx < W])
        recs.append(exact(r, f"impulse at image {n} pixel {y},{x}", be.fwd(r, img, w, torch.zeros(r.cout)).y.double(), want))
    return recs


def check_dgrad_impulses(be):
    """one power of two in dz at the corners of a 16 x 16 tile of a 17 x 33 image (and at the image's own), scale 1, shift 1 on y = 0
    (the switch is on), coef NULL: dx is one product of powers of two per tap, or zero; y given and y == NULL"""
    N, H, W = DGRAD_IMPULSE_SHAPE
    r, C = Row("dgrad_bn", (N, H, W, 1), DGRAD_IMPULSE_COUT, ""), DGRAD_IMPULSE_COUT
    w = impulse_filter(C)
    stats = torch.stack([torch.ones(1, C), torch.ones(1, C), torch.zeros(1, C), torch.ones(1, C)])
    zero_y, zero_x, recs = torch.zeros(N, H, W, C), torch.zeros(N, H, W), []
    pos = [(0, 15, 15), (0, 16, 16), (0, 15, 16), (0, 16, 15), (1, 0, 0), (1, 16, 32), (0, 15, 31), (1, 15, 32), (0, 16, 31), (0, 0, 32), (1, 16, 0)]
    for i, (n, y, x) in enumerate(pos):
        dz = torch.zeros(N, H, W, C)
        dz[n, y, x, (i * 5) % C] = 2.0 ** (i % 5 - 2)
        want = R.conv1_dgrad(R.bn_dy(dz, zero_y, stats, None, 1), w)
        assert bool((want != 0).any())
        recs += [exact(r, f"dz impulse at image {n} pixel {y},{x}, y given", be.dgrad_bn(r, dz, zero_y, stats, None, w, None, None).double(), want),
                 exact(r, f"dz impulse at image {n} pixel {y},{x}, y == NULL", be.dgrad_bn(r, dz, None, stats, None, w, None, zero_x).double(), want)]
    return recs


# --------------------------------------------------------------------------------------------------------------- refusals
# (label, entry point, changes to a call that would run, status, head of rpnet_last_error_string): every RPNET_REQUIRE of
# csrc/conv_first.hip, refused on the host before any launch.  The call that would run: N = 4, H = 4, W = 8, cout = 64, groups = 2,
# planes = 3, every pointer set (rpnet_conv1_fwd: no epilogue, y and stats_partial both set).  Changes: N, cout, groups, planes;
# null = names of pointers handed in as NULL; ep = 1: ep_scale / ep_shift set; ws_short = 1: one byte less than the query.
_WG = "conv1_wgrad:"          # rpnet_conv1_wgrad_bn's launch is rpnet_conv1_wgrad's: its refusals carry that head
REFUSALS = [
    ("null x", "rpnet_conv1_fwd", dict(null="x"), ARG, "conv1_fwd:"), ("null w", "rpnet_conv1_fwd", dict(null="w"), ARG, "conv1_fwd:"),
    ("y and stats_partial both NULL", "rpnet_conv1_fwd", dict(null="y,stats_partial"), ARG, "conv1_fwd:"),
    ("cout = 6", "rpnet_conv1_fwd", dict(cout=6), SHAPE, "conv1_fwd:"), ("cout = 12", "rpnet_conv1_fwd", dict(cout=12), SHAPE, "conv1_fwd:"),
    ("cout = 2048", "rpnet_conv1_fwd", dict(cout=2048), SHAPE, "conv1_fwd:"),
    ("N % groups != 0 under stats_partial", "rpnet_conv1_fwd", dict(groups=3), ARG, "conv1_fwd:"),
    ("ep_scale together with stats_partial", "rpnet_conv1_fwd", dict(ep=1), ARG, "conv1_fwd:"),
    ("null x", "rpnet_conv1_wgrad_bn", dict(null="x"), ARG, _WG), ("null dz", "rpnet_conv1_wgrad_bn", dict(null="dz"), ARG, _WG),
    ("null dw", "rpnet_conv1_wgrad_bn", dict(null="dw"), ARG, _WG), ("null workspace", "rpnet_conv1_wgrad_bn", dict(null="workspace"), ARG, _WG),
    ("y and w both NULL", "rpnet_conv1_wgrad_bn", dict(null="y,w"), ARG, "conv1_wgrad_bn:"),
    ("null stats", "rpnet_conv1_wgrad_bn", dict(null="stats"), ARG, "conv1_wgrad_bn:"), ("null coef", "rpnet_conv1_wgrad_bn", dict(null="coef"), ARG, "conv1_wgrad_bn:"),
    ("groups = 1025", "rpnet_conv1_wgrad_bn", dict(groups=1025, N=1025), SHAPE, "conv1_wgrad_bn:"),
    ("cout = 6", "rpnet_conv1_wgrad_bn", dict(cout=6), SHAPE, _WG), ("cout = 12", "rpnet_conv1_wgrad_bn", dict(cout=12), SHAPE, _WG),
    ("cout = 2048", "rpnet_conv1_wgrad_bn", dict(cout=2048), SHAPE, _WG), ("cout = 512", "rpnet_conv1_wgrad_bn", dict(cout=512), SHAPE, _WG),
    ("N % groups != 0", "rpnet_conv1_wgrad_bn", dict(groups=3), SHAPE, _WG), ("groups = 0", "rpnet_conv1_wgrad_bn", dict(groups=0), SHAPE, _WG),
    ("short workspace", "rpnet_conv1_wgrad_bn", dict(ws_short=1), WORKSPACE, _WG),
    ("null x", "rpnet_conv1_bn_relu", dict(null="x"), ARG, "conv1_bn_relu:"), ("null scale", "rpnet_conv1_bn_relu", dict(null="scale"), ARG, "conv1_bn_relu:"),
    ("null z_split", "rpnet_conv1_bn_relu", dict(null="z_split"), ARG, "conv1_bn_relu:"),
    ("cout = 6", "rpnet_conv1_bn_relu", dict(cout=6), SHAPE, "conv1_bn_relu:"), ("cout = 12", "rpnet_conv1_bn_relu", dict(cout=12), SHAPE, "conv1_bn_relu:"),
    ("cout = 2048", "rpnet_conv1_bn_relu", dict(cout=2048), SHAPE, "conv1_bn_relu:"), ("cout = 4", "rpnet_conv1_bn_relu", dict(cout=4), SHAPE, "conv1_bn_relu:"),
    ("N % groups != 0", "rpnet_conv1_bn_relu", dict(groups=3), SHAPE, "conv1_bn_relu:"),
    ("planes = 0", "rpnet_conv1_bn_relu", dict(planes=0), ARG, "conv1_bn_relu:"), ("planes = 4", "rpnet_conv1_bn_relu", dict(planes=4), ARG, "conv1_bn_relu:"),
    ("planes = 2 without gamma", "rpnet_conv1_bn_relu", dict(planes=2, null="gamma"), ARG, "conv1_bn_relu:"),
    ("planes = 1 without split_scale", "rpnet_conv1_bn_relu", dict(planes=1, null="split_scale"), ARG, "conv1_bn_relu:"),
    ("null dz", "rpnet_conv1_bn_bwd_partial", dict(null="dz"), ARG, "conv1_bn_bwd_partial:"), ("null partial", "rpnet_conv1_bn_bwd_partial", dict(null="partial"), ARG, "conv1_bn_bwd_partial:"),
    ("cout = 6", "rpnet_conv1_bn_bwd_partial", dict(cout=6), SHAPE, "conv1_bn_bwd_partial:"), ("cout = 12", "rpnet_conv1_bn_bwd_partial", dict(cout=12), SHAPE, "conv1_bn_bwd_partial:"),
    ("cout = 2048", "rpnet_conv1_bn_bwd_partial", dict(cout=2048), SHAPE, "conv1_bn_bwd_partial:"),
    ("N % groups != 0", "rpnet_conv1_bn_bwd_partial", dict(groups=3), SHAPE, "conv1_bn_bwd_partial:"),
    ("null dz", "rpnet_conv1_dgrad_bn", dict(null="dz"), ARG, "conv1_dgrad_bn:"), ("null w", "rpnet_conv1_dgrad_bn", dict(null="w"), ARG, "conv1_dgrad_bn:"),
    ("y and x both NULL", "rpnet_conv1_dgrad_bn", dict(null="y,x"), ARG, "conv1_dgrad_bn:"),
    ("cout = 16", "rpnet_conv1_dgrad_bn", dict(cout=16), SHAPE, "conv1_dgrad_bn:"), ("cout = 12", "rpnet_conv1_dgrad_bn", dict(cout=12), SHAPE, "conv1_dgrad_bn:"),
    ("cout = 2048", "rpnet_conv1_dgrad_bn", dict(cout=2048), SHAPE, "conv1_dgrad_bn:"),
    ("N % groups != 0", "rpnet_conv1_dgrad_bn", dict(groups=3), SHAPE, "conv1_dgrad_bn:"), ("H = 0", "rpnet_conv1_dgrad_bn", dict(H=0), SHAPE, "conv1_dgrad_bn:"),
    ("N = 65536", "rpnet_conv1_dgrad_bn", dict(N=65536, groups=1), SHAPE, "conv1_dgrad_bn:"),
    ("2^31 pixels", "rpnet_conv1_dgrad_bn", dict(N=32768, H=256, W=256), SHAPE, "conv1_dgrad_bn:"),
]
REFUSAL_BASE = dict(N=4, H=4, W=8, cout=64, groups=2, planes=3)
# the conditions of the RPNET_REQUIRE lines of csrc/conv_first.hip, as the head of each line's message and its status: the host test
# counts the lines in the source and holds the table against them
REQUIRE_LINES = 20


# ----------------------------------------------------------------------------------------- the float32 stand-in for the library
DEFECTS = ["strip_right_edge", "row_minus1_at_0", "no_bias_again", "group_from_block", "mask_from_y", "swap_c1c2", "xhat_no_invstd",
           "stale_row", "drop_low_plane", "absmax_overwrite", "dgrad_taps_transposed"]


class Out:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class SimBackend:
    """A float32 torch restatement of the entry points on the CPU.  y is the kernels' chain: the bias, then nine fused multiply-adds
    in row-major tap order (a product of two fp32 values is exact in double; the sum is rounded to double, then to fp32: a fused
    multiply-add but for double roundings).  Sums are taken in double where the kernels use double; the partial rows are contiguous
    pixel ranges of a group.  `defect`: one of DEFECTS."""

    def __init__(self, defect=None):
        assert defect is None or defect in DEFECTS
        self.defect = defect

    # -- y
    def _window(self, r, x):
        """x [N, H, W] -> zero-padded [N, H + 2, W + 2] (double)"""
        xp = F.pad(x, (1, 1, 1, 1))
        N, H, W = x.shape
        if self.defect in ("strip_right_edge", "row_minus1_at_0") and strips_ok(r.N, r.H, r.W, r.groups):
            flat = torch.cat([torch.zeros(1), x.reshape(-1), torch.zeros(1)])
            rows = torch.arange(N * H).reshape(N, H)
            if self.defect == "strip_right_edge":        # row[4] of a row's last strip: the first pixel of the next row
                xp[:, 1:H + 1, W + 1] = flat[1 + rows * W + W]
            else:                                        # row[-1] of a row's first strip: the last pixel of the row before
                xp[:, 1:H + 1, 0] = flat[rows * W]
        return xp.double()

    def _y(self, r, x, w, bias, again=False):
        N, H, W = x.shape
        xp = self._window(r, x)
        b = torch.zeros(r.cout) if bias is None or (again and self.defect == "no_bias_again") else bias.float()
        acc = b.expand(N, H, W, r.cout).contiguous()
        wd = w.double()
        for ky in range(3):
            for kx in range(3):
                acc = (xp[:, ky:ky + H, kx:kx + W, None] * wd[:, 0, ky, kx] + acc.double()).float()
        return acc

    @staticmethod
    def _pi(v, N):
        return R._per_image(v, N)

    def _rows(self, r, terms):
        """terms [N, H, W, C, 2] double -> [groups, rows, C, 2]: contiguous pixel ranges"""
        G, nblk, C = r.groups, stats_blocks(r.N, r.H, r.W, r.groups), r.cout
        t = terms.reshape(G, -1, C, 2)
        chunk = _cdiv(t.shape[1], nblk)
        out = torch.full((G, nblk, C, 2), NAN, dtype=F64)
        for b in range(nblk):
            out[:, b] = t[:, b * chunk:(b + 1) * chunk].sum(1)
        if self.defect == "stale_row":
            out[G - 1, nblk - 1] = NAN
        return out

    def fwd(self, r, x, w, bias, ep=None, absmax=None, stats=False, write_y=True):
        y = self._y(r, x, w, bias)
        if ep is not None:
            y = torch.relu(y * ep[0].float() + ep[1].float())
        out = Out(y=y if write_y else None, absmax=None, part=None)
        if absmax is not None:
            top = float(y.abs().max())
            out.absmax = torch.tensor(top if self.defect == "absmax_overwrite" else max(absmax, top), dtype=F32)
        if stats:
            yd = y.double()
            out.part = self._rows(r, torch.stack([yd, yd * yd], -1))
        return out

    def _group_of_pixel(self, r, defect_ok):
        p = torch.arange(r.M)
        g = (p // 256) % r.groups if defect_ok and self.defect == "group_from_block" else p // r.Mg
        return g.reshape(r.N, r.H, r.W)

    def _affine_relu(self, r, y, scale, shift, own):
        g = self._group_of_pixel(r, own)
        return torch.relu(y * scale.float()[g] + shift.float()[g])

    def _split(self, r, z, planes, want_z, gamma, beta, own):
        s = None
        if planes <= 2:
            sqrt_n = (torch.tensor(float(r.Mg), dtype=F32).sqrt() * torch.tensor(1.0001, dtype=F32))
            s = pow2_scale(float((gamma.float().abs() * sqrt_n + beta.float().abs()).max()))
        bits = split_planes(z if s is None else z * torch.tensor(1.0 / s, dtype=F32), planes, 1.0 if s is not None else None)
        if own and self.defect == "drop_low_plane":
            bits[planes - 1] = 0
        return Out(z=z if want_z else torch.full_like(z, NAN), planes=bits, scale=None if s is None else torch.tensor(s, dtype=F32))

    def conv1_bn_relu(self, r, x, w, bias, scale, shift, planes, want_z, gamma, beta):
        z = self._affine_relu(r, self._y(r, x, w, bias, again=True), scale, shift, True)
        return self._split(r, z, planes, want_z, gamma, beta, True)

    def bn_relu(self, r, y, scale, shift, planes, want_z, gamma, beta):
        return self._split(r, self._affine_relu(r, y, scale, shift, False), planes, want_z, gamma, beta, False)

    def _dm_xhat(self, r, dz, y, stats):
        st = stats.float().reshape(4, r.groups, -1)
        sc, sh, mu, inv = (self._pi(st[i], r.N) for i in range(4))
        m = (y > 0) if self.defect == "mask_from_y" else (y * sc + sh > 0)
        xhat = (y - mu) if self.defect == "xhat_no_invstd" else (y - mu) * inv
        return dz * m.float(), xhat, sc

    def bwd_partial(self, r, x, w, bias, dz, stats):
        dm, xhat, _ = self._dm_xhat(r, dz, self._y(r, x, w, bias, again=True), stats)
        return self._rows(r, torch.stack([dm.double(), dm.double() * xhat.double()], -1))

    def bn_bwd_given(self, r, dz, stats, part):
        s = part.sum(1)                                             # [G, C, 2] double
        return Out(dgamma=s[..., 1].sum(0).float(), dbeta=s[..., 0].sum(0).float(), coef=(s / r.Mg).float())

    def _dy(self, r, dz, y, stats, coef):
        dm, xhat, sc = self._dm_xhat(r, dz, y, stats)
        if coef is None:
            coef = torch.zeros(r.groups, r.cout, 2)
        c1, c2 = self._pi(coef[..., 0].float(), r.N), self._pi(coef[..., 1].float(), r.N)
        if self.defect == "swap_c1c2":
            c1, c2 = c2, c1
        return sc * (dm - c1 - xhat * c2)

    def wgrad_bn(self, r, x, dz, y, stats, coef, w, bias):
        dy = self._dy(r, dz, self._y(r, x, w, bias, again=True) if y is None else y, stats, coef)
        return R.conv_wgrad(x[..., None], None, dy, dtype=F32)

    def dgrad_bn(self, r, dz, y, stats, coef, w, bias, x):
        dy = self._dy(r, dz, self._y(r, x, w, bias, again=True) if y is None else y, stats, coef)
        wt = w.float().transpose(2, 3) if self.defect == "dgrad_taps_transposed" else w.float()
        return R.conv1_dgrad(dy, wt, dtype=F32)
