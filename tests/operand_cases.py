"""Cases, references and comparison functions shared by tests/test_host_operands.py and tests/test_gpu_operands.py: the operand
splitters and weight packers behind every convolution and correlation on the 16-bit matrix pipe (rpnet_split_bf16, rpnet_split_f16,
rpnet_pow2_scale, rpnet_predict_scales, rpnet_pack_conv_weight_split, rpnet_pack_conv_weights_split, rpnet_pack_conv_weight,
rpnet_upconv_collapse_weights), held BIT FOR BIT to references written from include/rpnet_abi.h.

The plane reference is tests/corr_cases.py's split_planes / plane_values / pow2_scale, the very functions with which the correlation,
weight-gradient and first-layer suites make their operands on the host: equality with them here is what entitles those suites to
judge the kernels "on the values the planes represent".  The pack reference builds the layouts of the header with reshape / permute /
scatter; the collapse reference sums, in float64, the taps that each output phase reads from each of its 2 x 2 source pixels.

A *backend* runs the entry points on CPU tensors and returns CPU tensors: the HIP library (the GPU test) or SimBackend, a restatement
of the kernels' INDEX arithmetic (grid-stride loops, tile walks, guards, reductions) in integer numpy / torch, with or without a seeded
defect (the host test).  The check_* functions drive a backend through one row and return records; hold() asserts.

There is no tolerance on a written bit.  Beside the bit equality the checks assert the DERIVED reconstruction bounds that the consumers'
error models rest on (corr_cases.split_unit_roundoff), with v = fp32(x f) / s in float64:
  two fp16 planes  |v - (h + l)| <= max(2^-22 |v|, 2^-25)      one plane  <= max(2^-11 |v|, 2^-25)
  (v - h is exact in fp32; fp16 rounds to 2^-11 relative in its normal range and its spacing below 2^-14 is 2^-24)
  three bf16 planes  h + m + l == x exactly for |x| >= 2^-100; below, where a device may flush subnormals, |x - sum| <= 2^-126.
The collapsed weights are at most four fp32 additions: |device - float64| <= 3 * 2^-24 * sum |addends|, exact on small integers."""
import collections
import math
from fractions import Fraction

import numpy as np
import torch
import torch.nn.functional as F

from tests.corr_cases import ARG, SHAPE, Rec, case_seed, hold, plane_values, pow2_scale, split_planes, split_unit_roundoff  # noqa: F401
from tests.helpers import rnd

F32, F64, I16, I32 = torch.float32, torch.float64, torch.int16, torch.int32
NAN = float("nan")
NAN16 = {3: 0x7FC0, 2: 0x7E00, 1: 0x7E00}      # a quiet NaN of the plane format: what every plane output is prefilled with
GUARD = 64                                      # 4-byte words behind (and, for an offset pointer, in front of) every output
GRID_CAP, BLOCK = 16384, 256                    # the split kernels: at most 16384 blocks of 256 threads, 8 elements per thread and pass
FLUSH_EDGE = 2.0 ** -100                        # below: fp32 / bf16 subnormal territory of a three-plane residual


def ulp_step(v, k):
    """the fp32 number k units in the last place from v"""
    return float((torch.tensor([v], dtype=F32).view(I32) + k).view(F32)[0])


# ------------------------------------------------------------------------------------------------------------------ records
TALLY = collections.OrderedDict()               # family -> [elements compared bit for bit, worst reconstruction error / its bound]


class ORec(Rec):
    def line(self):
        return f"PARITY operands {self.family} {self.what} err/bound={self.err:.3e}"


def bits(t):
    """the integer view in which equality is bit equality (NaN patterns and the sign of zero included)"""
    t = torch.as_tensor(t)
    return t.view(I32) if t.dtype == F32 else t


def exact(family, what, got, want):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, (family, what, tuple(got.shape), tuple(want.shape))
    TALLY.setdefault(family, [0, 0.0])[0] += got.numel()
    bad = got != want
    n = int(bad.sum())
    if n:        # the first mismatches by flat index, as integers: what a reader of the failure needs
        at = torch.nonzero(bad.reshape(-1))[:4, 0]
        show = (lambda v: repr(float(v))) if got.is_floating_point() else (lambda v: f"{int(v):#x}")
        what += " [" + ", ".join(f"at {int(i)}: got {show(got.reshape(-1)[i])} want {show(want.reshape(-1)[i])}" for i in at) + "]"
    return Rec(family, what, n, 0.0, 0.0, exact=True)


def within(family, what, err, bound):
    """max(err / bound) <= 1 over the elements, both float64 tensors; an element with bound 0 must have err 0"""
    frac = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0).to(F64))
    worst = float(frac.max()) if frac.numel() else 0.0
    worst = math.inf if math.isnan(worst) else worst
    t = TALLY.setdefault(family, [0, 0.0])
    t[1] = max(t[1], worst)
    return ORec(family, what, worst, 0.0, 1.0)


def twice(be, call):
    """(result, result of a second identical call); a backend that is a pure function of its arguments (SimBackend) runs once"""
    got = call()
    return got, (got if getattr(be, "pure", False) else call())


def tally_lines():
    return [f"OPERANDS {fam} elements={n} worst_reconstruction_of_bound={w:.3f}" for fam, (n, w) in TALLY.items()]


# ------------------------------------------------------------------------------------------------------------------ pow2 scale
def pow2_exponent_from_header(bits32):
    """include/rpnet_abi.h, in integers: s = 2^(ceil(log2 bound) - 15) clamped to 2^-100 .. 2^100; zero, negative, NaN -> 2^-100"""
    sign, e, m = bits32 >> 31, (bits32 >> 23) & 255, bits32 & 0x7FFFFF
    if e == 255:
        return 100 if (m == 0 and not sign) else -100            # +inf / NaN, -inf
    if sign or (e == 0 and m == 0):
        return -100
    b = Fraction(m + (1 << 23 if e else 0)) * Fraction(2) ** ((e if e else 1) - 150)
    k = (b.numerator.bit_length() - 1) - (b.denominator.bit_length() - 1)        # floor(log2 b): b is a dyadic rational
    while Fraction(2) ** k < b:
        k += 1
    while Fraction(2) ** (k - 1) >= b:
        k -= 1
    return max(-100, min(100, k - 15))


POW2_K = (-20, 0, 15, 16)
POW2_BOUNDS = ([0.0, -1.0, NAN, math.inf, 2.0 ** -149, 65504.0, 3.7]
               + [ulp_step(2.0 ** k, d) for k in (-85, 115) + POW2_K for d in (-1, 0, 1)])


def ref_pow2(bound):
    """fp32 scalar tensor of corr_cases.pow2_scale"""
    return torch.tensor(pow2_scale(float(bound)), dtype=F32)


def check_pow2(be, bound):
    b = torch.tensor([bound], dtype=F32)
    got, again = be.pow2_scale(b), be.pow2_scale(b)
    return [exact("pow2_scale", f"{bound!r}", got, ref_pow2(b[0]).reshape(1)), exact("pow2_scale", f"{bound!r} second call", again, got)]


# n, safety, check
PREDICT_ROWS = [(n, s, c) for n in (0, 1, 255, 256, 257) for s in (1.0, 4.0) for c in (0, 1)]
VIOL_SEED = 5


def predict_inputs(n, safety):
    """measured / bound pairs that walk below, equal, one ulp above, far above, 0, +inf, NaN, the clamps and exact powers of two"""
    bound = torch.tensor([2.0 ** ((i % 9) - 3) for i in range(n)], dtype=F32)
    m = bound.clone()
    how = ["below", "equal", "ulp_above", "far", "zero", "inf", "nan", "pow2", "tiny"]
    for i in range(n):
        h = how[i % len(how)] if n > 1 else "ulp_above"
        m[i] = {"below": 0.37 * float(bound[i]), "equal": float(bound[i]), "ulp_above": ulp_step(float(bound[i]), 1), "far": 1e30,
                "zero": 0.0, "inf": math.inf, "nan": NAN, "pow2": 0.25 * float(bound[i]), "tiny": 1e-38}[h]
    return m, bound


def ref_predict(m, bound, n, safety, check, viol):
    p = m * torch.tensor(safety, dtype=F32)                     # the product is rounded in fp32 first
    scale = torch.stack([ref_pow2(v) for v in p]) if n else torch.zeros(0)
    count = int(sum(1 for i in range(n) if not float(m[i]) <= float(bound[i]))) if check else 0
    return scale * 32768.0, scale, viol + count


def check_predict(be, n, safety, check):
    fam, tag = "predict_scales", f"n={n} safety={safety:g} check={check}"
    m, bound = predict_inputs(n, safety)
    got = be.predict_scales(m, bound, n, safety, check, VIOL_SEED if check else None)
    again = be.predict_scales(m, bound, n, safety, check, VIOL_SEED if check else None)
    wb, ws, wv = ref_predict(m, bound, n, safety, check, VIOL_SEED)
    recs = [exact(fam, tag + " bound", got[0], wb), exact(fam, tag + " scale", got[1], ws),
            exact(fam, tag + " bound == scale * 2^15", got[0].double(), got[1].double() * 32768.0)]
    if check:
        recs.append(exact(fam, tag + " violations", torch.tensor([got[2]]), torch.tensor([wv])))
        if n >= 9:
            assert wv - VIOL_SEED == sum(1 for i in range(n) if i % 9 in (2, 3, 5, 6))      # ulp above, far, +inf, NaN: the table holds them
    recs += [exact(fam, tag + f" second call {k}", a, g) for k, (a, g) in enumerate(zip(again[:2], got[:2]))]
    return recs


# ------------------------------------------------------------------------------------------------------------------ split rows
SplitRow = collections.namedtuple("SplitRow", "id kernel rows C mode planes data bound a_is_bound sb s_out offset")

# values of v = x / s (fp16 rows) that an fp16 rounding can get wrong
F16_SPECIALS = [0.0, -0.0, 32768.0, -32768.0,
                1024.5, 1025.5, -1024.5, -1025.5,                 # ties of the first plane, even / odd neighbour below: truncation and
                2049.0 * 2.0 ** -6, 2051.0 * 2.0 ** -6,           # round-half-away each fail on one parity
                1025.0 - 4093 * 2.0 ** -13, 1025.0 - 4095 * 2.0 ** -13, -(1025.0 - 4093 * 2.0 ** -13),      # ties of the SECOND plane
                1.0 + 2.0 ** -20, 1.0 + 2.0 ** -23, 2.0 ** -10 + 2.0 ** -22, 2.0 ** -10 + 3 * 2.0 ** -26,    # residual an fp16 subnormal
                -(2.0 ** -12) - 2.0 ** -35, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -26, 2.0 ** -26, 65504.0 / 2]
# fp32 values an x itself may hold, whatever the scale
F32_SPECIALS = [2.0 ** -149, -(2.0 ** -130), 1.5 * 2.0 ** -127, 2.0 ** -126]
BF16_SPECIALS = [0.0, -0.0, 128.5, 129.5, -128.5, -129.5, 257.0 * 2.0 ** -9, 259.0 * 2.0 ** -9,          # ties of the first plane
                 1.0 + 2.0 ** -9 + 2.0 ** -17, 1.0 + 3 * 2.0 ** -9 + 3 * 2.0 ** -17,                       # ties of the second
                 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24, 3.0e38, -3.0e38, 2.0 ** 100, FLUSH_EDGE, ulp_step(FLUSH_EDGE, 1),
                 ulp_step(FLUSH_EDGE, -1), 2.0 ** -101, 1.2345e-36, 2.0 ** -120 * 1.001] + F32_SPECIALS

SPLIT_SHAPES = [(1, 8),          # one thread
                (1, 72),         # C / 8 = 9: the FastDiv that is no power of two, one row
                (7, 72),         # the same over rows: a wrong divisor reads another row's mask
                (3, 8),          # C / 8 = 1
                (33, 40),        # 165 items: the last block partly idle
                (256, 8),        # exactly one block of items (the launcher adds a second, idle one)
                (257, 8)]        # one item into the second block
# 524 320 items of 8 elements (4.2 M elements, 17 MB): 2049 blocks, a row index beyond 2^19.  At C = 8 this stays below the grid cap:
# the cap counts blocks of 256 ITEMS, so the grid-stride loop first runs twice at 16384 * 256 + 1 items (CAP row below).
LARGE = (16385 * 32, 8)
CAP = (GRID_CAP * BLOCK + 257, 8)           # second pass of the grid-stride loop in blocks 0 and 1, the row index crosses the cap
BOUNDS = [3.7] + [ulp_step(2.0 ** k, d) for k in POW2_K for d in (-1, 0, 1)]          # 1.0 is 2^0


def _split_rows():
    rows = []

    def add(kernel, shape, mode, planes, data="mix", bound=3.7, a_is_bound=0, sb="none", s_out=1, offset=0):
        rid = f"{kernel}-{shape[0]}x{shape[1]}-m{mode}-p{planes}-{data}" + (f"-bound{bound!r}" if a_is_bound else f"-sb_{sb}" if kernel == "f16" else "")
        rows.append(SplitRow(rid + ("-nosout" if kernel == "f16" and not s_out else "") + ("-offset" if offset else ""), kernel, shape[0], shape[1],
                             mode, planes, data, bound, a_is_bound, sb, s_out, offset))

    k = 0
    for shape in SPLIT_SHAPES:
        for mode in (0, 1, 2):
            add("bf16", shape, mode, 3)                                                     # split_bf16_kernel<3>
            for planes in (2, 1):                                                           # split_f16_kernel<2> / <1>
                add("f16", shape, mode, planes, sb=("none", "lo", "hi")[k % 3], s_out=(k // 3) % 2)
                k += 1
    for planes in (2, 1):
        for b in BOUNDS:                                                                    # a_is_bound: pow2_scale(*s_a) in the kernel
            add("f16", (7, 72), 0 if planes == 2 else 2, planes, bound=b, a_is_bound=1)
    for kernel, planes in (("bf16", 3), ("f16", 2), ("f16", 1)):
        add(kernel, (41, 16), 0, planes, data="decades", bound=2.0 ** 3)                    # 2^-40 .. 2^0 of the bound, one binade per row
        add(kernel, (0, 8), 1, planes)                                                      # rows = 0: OK, nothing written
        add(kernel, (33, 40), 2, planes, offset=1)                                          # pointers 16 bytes into a larger allocation
        add(kernel, LARGE, 1, planes, data="large")
        if planes != 2:                                                                     # one loop source per kernel: <2> shares <1>'s
            add(kernel, CAP, 2, planes, data="large")
    return rows


SPLIT_ROWS = _split_rows()
MASK_CYCLE = [1.0, 0.0, 2.0 ** -30, 0.25, 0.7, 1.0 - 2.0 ** -24]


def scatter_specials(x, vals):
    flat, n = x.view(-1), x.numel()
    vals = torch.tensor(vals, dtype=F64)
    if n >= len(vals):
        flat[torch.arange(len(vals)) * (n // len(vals))] = vals.to(F32)
    else:
        flat[:] = vals[:n].to(F32)


def split_inputs(r):
    """(x [rows, C], mask [rows] or None, s_a, s_b): fp32 tensors, the scales as [1]; |x| <= bound and |x / s| <= 2^15 by construction"""
    seed = case_seed(r.rows % 9973, r.C, r.mode, r.planes)
    n = r.rows * r.C
    s = pow2_scale(r.bound)
    if r.data == "large":            # a short seeded draw repeated: the reference stays one vector pass
        base = rnd(seed, 8191)
        x = base.repeat(n // 8191 + 1)[:n].reshape(r.rows, r.C).contiguous()
    else:
        x = rnd(seed, r.rows, r.C)
    if r.kernel == "f16":
        x = (x * torch.tensor(r.bound / 4, dtype=F32)).clamp(-r.bound, r.bound)
        if r.data == "decades":
            x = x * (2.0 ** -torch.arange(r.rows, dtype=F32))[:, None]
        if n:
            sp = [v * s for v in F16_SPECIALS if abs(v * s) <= r.bound] + [r.bound, -r.bound] + F32_SPECIALS
            scatter_specials(x, sp)
    else:
        x = x * 3.0
        if r.data == "decades":
            x = x * (2.0 ** -(3.0 * torch.arange(r.rows, dtype=F32)))[:, None]
        if n:
            scatter_specials(x, BF16_SPECIALS)
    mask = None
    if r.mode:
        mask = torch.tensor(MASK_CYCLE, dtype=F32).repeat(r.rows // len(MASK_CYCLE) + 1)[:r.rows].clone()
        if r.rows > 6:
            mask[6::7] = torch.from_numpy(np.random.RandomState(seed).uniform(0, 1, len(mask[6::7])).astype(np.float32))
    if r.a_is_bound:
        return x, mask, torch.tensor([r.bound], dtype=F32), None
    s_a = torch.tensor([s], dtype=F32)
    return x, mask, s_a, {"none": None, "lo": s_a / 4, "hi": s_a * 4}[r.sb]


def masked(x, mask, mode):
    """fp32(x * f), f = mask or fp32(1 - mask), formed in float32"""
    if not mode:
        return x
    f = mask if mode == 1 else torch.tensor(1.0, dtype=F32) - mask
    return x * f[:, None]


def ref_scale(r, s_a, s_b):
    if r.a_is_bound:
        return ref_pow2(s_a[0])
    return s_a[0] if s_b is None else torch.maximum(s_a[0], s_b[0])


def check_split(be, r):
    fam = f"split_{r.kernel}"
    x, mask, s_a, s_b = split_inputs(r)
    v = masked(x, mask, r.mode)
    recs = []
    if r.kernel == "bf16":
        got, again = twice(be, lambda: be.split_bf16(x, mask, r.mode, r.offset))
        want = split_planes(v, 3)
        big = (v.abs() >= FLUSH_EDGE) | (v == 0)
        zero16 = torch.zeros((), dtype=I16)
        recs.append(exact(fam, r.id + " planes", torch.where(big, got, zero16), torch.where(big, want, zero16)))
        total = plane_values(got)
        recs.append(exact(fam, r.id + " h + m + l == x", torch.where(big, total, 0.0), torch.where(big, v.double(), 0.0)))
        if not bool(big.all()):
            same = int((got[:, ~big] == want[:, ~big]).all(0).sum())
            print(f"OPERANDS split_bf16 {r.id}: {int((~big).sum())} elements below 2^-100, {same} of them bit for bit the CPU planes")
            err = (v.double() - total)[~big].abs()
            recs.append(within(fam, r.id + " below 2^-100", torch.nan_to_num(err, nan=math.inf), torch.full_like(err, 2.0 ** -126)))
    else:
        (got, s_got), (again, s_again) = twice(be, lambda: be.split_f16(x, mask, r.mode, s_a, s_b, r.planes, r.a_is_bound, r.s_out, r.offset))
        s = ref_scale(r, s_a, s_b)
        want = split_planes(v, r.planes, s)
        recs.append(exact(fam, r.id + " planes", got, want))
        if r.s_out:        # rows = 0 writes nothing, *s_out included: it comes back as prefilled
            s_want = s.reshape(1) if r.rows else torch.full((1,), NAN)
            recs += [exact(fam, r.id + " s_out", s_got.reshape(1), s_want), exact(fam, r.id + " s_out second call", s_again.reshape(1), s_got.reshape(1))]
        else:
            assert s_got is None
        h = got.view(torch.float16).double()
        recs.append(exact(fam, r.id + " planes finite, |h| <= 2^15", torch.isfinite(h) & (h.abs() <= 32768.0), torch.ones_like(h, dtype=torch.bool)))
        v64 = v.double() / float(s)
        u = 2.0 ** -22 if r.planes == 2 else 2.0 ** -11
        assert u <= split_unit_roundoff(r.planes)             # the consumers' model is no tighter than what is asserted here
        recs.append(within(fam, r.id + " reconstruction", (v64 - h.sum(0)).abs(), torch.maximum(u * v64.abs(), torch.full_like(v64, 2.0 ** -25))))
        if r.a_is_bound and r.mode == 0 and math.log2(r.bound).is_integer():
            assert int((h[0].abs() == 32768.0).sum()) >= 2, r.id       # the elements at the bound sit at exactly 2^15
    recs.append(exact(fam, r.id + " second call", again, got))
    return recs


# ------------------------------------------------------------------------------------------------------------------ pack rows
Item = collections.namedtuple("Item", "id cout cin taps off0 split off1 cin_pad")


def item(cout, cin, taps, off0=0, split=None, off1=None, cin_pad=None):
    split = cin if split is None else split
    off1 = off0 + split if off1 is None else off1
    cin_pad = (max(off0 + split, off1 + cin - split) + 31) // 32 * 32 if cin_pad is None else cin_pad
    return Item(f"{cout}x{cin}x{taps}-o{off0}s{split}o{off1}p{cin_pad}", cout, cin, taps, off0, split, off1, cin_pad)


PLAIN_ITEMS = [item(32, 32, 9),                     # one tile, nothing padded
               item(64, 64, 9),                     # 2 x 2 tiles
               item(32, 8, 9),                      # one group of 8 rows: g * 8 < ncin cuts three of four groups
               item(32, 40, 1),                     # cin no multiple of 32: last tile of 8 rows, cin_pad 64, one tap
               item(128, 32, 4),                    # the collapsed up_conv layer
               item(32, 96, 9),                     # three cin tiles
               item(32, 64, 9, 0, 32, 64, 128)]     # two ranges: padding between and behind them
GATHER_ITEMS = [item(64, 377, 1, 0, 121, 128, 384),  # the model's 1x1 layer over cat([corr(121 -> 128), fm1(256)])
                item(32, 13, 9, 0, 5, 32, 64),       # ranges of 5 and 8 rows, all else padding
                item(32, 16, 9, 3, 8, 16, 32)]       # cin_off0 = 3 alone sends an otherwise plain layer to the gathering walk
PACK_ITEMS = PLAIN_ITEMS + GATHER_ITEMS
F32_ITEMS = ([i._replace(taps=t, id=i.id + f"-t{t}") for i in PACK_ITEMS for t in (9, 1) if i.taps != 4 or t == 9]
             + [item(32, 6, 9, 0, 6, 6, 8), item(32, 10, 1, 1, 3, 5, 12)])        # cin_pad % 4 == 0 only
SENTINEL = 0x3C00                                    # 1.0 in fp16: a padding row the plain form must leave as found


def needs_gather(it):
    return bool(it.cin % 8 or it.off0 % 8 or it.split % 8 or it.off1 % 8)


def row_of(it):
    c = torch.arange(it.cin)
    return torch.where(c < it.split, it.off0 + c, it.off1 + (c - it.split))


def weights(it, kind="draw"):
    """[cout, cin, taps] fp32: rows over five decades, an all-zero output and input channel, channel maxima at exact powers of two"""
    if kind.startswith("impulse"):
        co, ci, tap = {"impulse_first": (0, 0, 0), "impulse_last": (it.cout - 1, it.cin - 1, it.taps - 1),
                       "impulse_mixed": (it.cout - 1, 0, it.taps - 1), "impulse_split": (0, min(it.split, it.cin - 1), 0)}[kind]
        w = torch.zeros(it.cout, it.cin, it.taps)
        w[co, ci, tap] = 1.5
        return w
    w = rnd(case_seed(it.cout, it.cin, it.taps, it.off0), it.cout, it.cin, it.taps)
    w = w * (10.0 ** -(torch.arange(it.cout) % 5).float())[:, None, None]
    if kind == "integers":
        return (w * 1e3).round().clamp(-8, 8) * 2.0 ** -6
    w[0] = w[0].clamp(-0.5, 0.5)
    w[0, 0, 0] = -0.5                                   # the maximum of output channel 0 is exactly 2^-1
    if it.cin > 2:
        w[:, 2] = 0                                     # an all-zero input channel
        w[:, 1] = w[:, 1].clamp(-2.0, 2.0)
        w[it.cout // 2, 1, it.taps - 1] = 2.0           # the maximum of input channel 1 is exactly 2^1
    w[1] = 0                                            # an all-zero output channel
    return w


def lay_wp(P, g):
    """[planes, cout, cin_pad, taps] -> [planes][taps][cin_pad / g][cout][g]"""
    pl, cout, cp, taps = P.shape
    return P.permute(0, 3, 2, 1).reshape(pl, taps, cp // g, g, cout).permute(0, 1, 2, 4, 3).contiguous()


def lay_wd(P, g):
    """[planes, cout, cin_pad, taps] -> [planes][taps flipped][cout / g][cin_pad][g]"""
    pl, cout, cp, taps = P.shape
    return P.flip(3).permute(0, 3, 1, 2).reshape(pl, taps, cout // g, g, cp).permute(0, 1, 2, 4, 3).contiguous()


def gathered(it, w):
    G = torch.zeros(it.cout, it.cin_pad, it.taps, dtype=w.dtype)
    G[:, row_of(it)] = w
    return G


def real_rows(it):
    m = torch.zeros(1, it.cout, it.cin_pad, it.taps, dtype=torch.bool)
    m[:, :, row_of(it)] = True
    return m


def ref_pack_split(it, w, planes):
    """(wp, wd int16, row_scale_wp [cout], row_scale_wd [cin_pad] with its padding at the preset 1) as the header states them"""
    G = gathered(it, w)
    if planes == 3:
        P = split_planes(G, 3)
        return lay_wp(P, 32), lay_wd(P, 32), None, None
    t = torch.stack([ref_pow2(w[co].abs().max()) for co in range(it.cout)])
    u = torch.ones(it.cin_pad)
    u[row_of(it)] = torch.stack([ref_pow2(w[:, c].abs().max()) for c in range(it.cin)])
    return lay_wp(split_planes(G, planes, t[:, None, None]), 32), lay_wd(split_planes(G, planes, u[None, :, None]), 32), t, u


PackCall = collections.namedtuple("PackCall", "it w wp0 wd0 t0 u0")


def pack_call(it, w, planes, want_wd, pad_fill=0):
    """the call with its outputs prefilled: a NaN pattern wherever the kernel must write; the padding rows of the plain form at
    `pad_fill` (the header: zero) and the padding entries of row_scale_wd at 1, for the kernel to leave as found"""
    written = real_rows(it).expand(planes, -1, -1, -1) if not needs_gather(it) else torch.ones(planes, it.cout, it.cin_pad, it.taps, dtype=torch.bool)
    nan16, fill = torch.tensor(NAN16[planes], dtype=I16), torch.tensor(pad_fill, dtype=I16)
    wp0 = torch.where(lay_wp(written, 32), nan16, fill)
    wd0 = torch.where(lay_wd(written, 32), nan16, fill) if want_wd else None
    t0 = u0 = None
    if planes <= 2:
        t0, u0 = torch.full((it.cout,), NAN), torch.ones(it.cin_pad)
        u0[row_of(it)] = NAN
    return PackCall(it, w, wp0, wd0, t0, u0)


def want_pack(call, planes):
    it = call.it
    wp, wd, t, u = ref_pack_split(it, call.w, planes)
    if not needs_gather(it):           # what the plain form leaves as found
        keep = real_rows(it).expand(planes, -1, -1, -1)
        wp = torch.where(lay_wp(keep, 32), wp, call.wp0)
        wd = torch.where(lay_wd(keep, 32), wd, call.wd0) if call.wd0 is not None else None
    return wp, (wd if call.wd0 is not None else None), t, u


def pack_records(fam, tag, got, call, planes):
    wp, wd, t, u = want_pack(call, planes)
    recs = [exact(fam, tag + " wp", got.wp, wp)]
    if call.wd0 is not None:
        recs.append(exact(fam, tag + " wd", got.wd, wd))
    else:
        assert got.wd is None
    if planes <= 2:
        recs += [exact(fam, tag + " row_scale_wp", got.t, t), exact(fam, tag + " row_scale_wd", got.u, u)]
        for name, pk, sc in (("wp", got.wp, t[None, None, None, :, None]), ("wd", got.wd, u[None, None, None, :, None])):
            if pk is None:
                continue
            h = pk.view(torch.float16).double()
            recs.append(exact(fam, tag + f" {name} finite, |h| <= 2^15", torch.isfinite(h) & (h.abs() <= 32768.0), torch.ones_like(h, dtype=torch.bool)))
            v = (lay_wp if name == "wp" else lay_wd)(gathered(call.it, call.w.double())[None], 32)[0] / sc[0].double()
            uu = 2.0 ** -22 if planes == 2 else 2.0 ** -11
            keep = (lay_wp if name == "wp" else lay_wd)(real_rows(call.it), 32)[0] | needs_gather(call.it)
            err = torch.where(keep, (v - h.sum(0)).abs(), torch.zeros_like(v))
            recs.append(within(fam, tag + f" {name} reconstruction", err, torch.maximum(uu * v.abs(), torch.full_like(v, 2.0 ** -25))))
    else:
        for name, pk, lay in (("wp", got.wp, lay_wp), ("wd", got.wd, lay_wd)):
            if pk is not None:
                keep = lay(real_rows(call.it), 32)[0] | needs_gather(call.it)
                total = torch.where(keep, plane_values(pk), torch.zeros((), dtype=F64))
                recs.append(exact(fam, tag + f" {name} h + m + l == w", total, lay(gathered(call.it, call.w.double())[None], 32)[0]))
    return recs


def same_out(fam, tag, a, b):
    return [exact(fam, f"{tag} {n}", x, y) for n, x, y in zip(("wp", "wd", "row_scale_wp", "row_scale_wd"), a, b) if x is not None]


PACK_ROWS = [(it, planes) for it in PACK_ITEMS for planes in (3, 2, 1)]


def check_pack(be, it, planes):
    """one layer through rpnet_pack_conv_weight_split, wd given and NULL; a padded plain layer once more with its padding at SENTINEL"""
    fam, recs, w = f"pack_split<{planes}>", [], weights(it)
    fills = [0] + ([SENTINEL] if not needs_gather(it) and it.cin_pad != it.cin else [])
    for want_wd in (1, 0):
        for fill in fills:
            tag = f"{it.id} wd={want_wd} pad={fill:#x}"
            call = pack_call(it, w, planes, want_wd, fill)
            got, again = twice(be, lambda: be.pack_split([call], planes, single=True)[0])
            recs += pack_records(fam, tag, got, call, planes) + same_out(fam, tag + " second call", again, got)
    return recs


IMPULSE_ROWS = [(it, planes, kind) for it in (PLAIN_ITEMS[6], GATHER_ITEMS[1], PLAIN_ITEMS[3]) for planes in (3, 2)
                for kind in ("impulse_first", "impulse_last", "impulse_mixed", "impulse_split")]


def check_impulse(be, it, planes, kind):
    """one non-zero weight lands at exactly one position of wp and one of wd, the tap flipped: the index written out from the header"""
    fam, w = f"pack_split<{planes}>", weights(it, kind)
    call = pack_call(it, w, planes, 1)
    got = be.pack_split([call], planes, single=True)[0]
    recs = pack_records(fam, f"{it.id} {kind}", got, call, planes)
    co, ci, tap = [int(v[0]) for v in torch.nonzero(w, as_tuple=True)]
    row = int(row_of(it)[ci])
    at_wp = ((tap * (it.cin_pad // 32) + row // 32) * it.cout + co) * 32 + row % 32
    at_wd = (((it.taps - 1 - tap) * (it.cout // 32) + co // 32) * it.cin_pad + row) * 32 + co % 32
    val = torch.tensor([1.5 if planes == 3 else 1.5 / pow2_scale(1.5)])
    code = int((val.bfloat16() if planes == 3 else val.half()).view(I16)[0])
    for name, pk, at in (("wp", got.wp, at_wp), ("wd", got.wd, at_wd)):
        flat = pk.reshape(planes, -1)
        recs.append(exact(fam, f"{it.id} {kind} {name} position", torch.tensor([torch.nonzero(flat).tolist() == [[0, at]]]), torch.tensor([True])))
        recs.append(exact(fam, f"{it.id} {kind} {name} value", flat[0, at].reshape(1), torch.tensor([code], dtype=I16)))
    return recs


def _multi(order):
    sized = sorted(PACK_ITEMS, key=lambda i: i.cout * i.cin_pad * i.taps)
    cyc = [sized[i % len(sized)] for i in range(24)]
    return {"one": [PLAIN_ITEMS[3]], "gather+plain": [GATHER_ITEMS[1], PLAIN_ITEMS[0]], "plain+gather": [PLAIN_ITEMS[1], GATHER_ITEMS[2]],
            "24 smallest first": sorted(cyc, key=lambda i: i.cout * i.cin_pad * i.taps),
            "24 smallest last": sorted(cyc, key=lambda i: -i.cout * i.cin_pad * i.taps)}[order]


MULTI_ROWS = [(o, p) for o in ("one", "gather+plain", "plain+gather", "24 smallest first", "24 smallest last") for p in (3, 2, 1)]


def check_multi(be, order, planes):
    """rpnet_pack_conv_weights_split: every item equal to the reference and, bit for bit, to its single-layer call; blocks beyond an
    item's own extent leave its neighbours alone (every buffer is exactly as long as its layout, guard words behind)"""
    fam, items = f"pack_split<{planes}>", _multi(order)
    calls = [pack_call(it, weights(it) * (1 + k % 3), planes, want_wd=(k % 4 != 3)) for k, it in enumerate(items)]
    got, again = twice(be, lambda: be.pack_split(calls, planes, single=False))
    recs = []
    for k, (call, g, a) in enumerate(zip(calls, got, again)):
        tag = f"{order}[{k}] {call.it.id}"
        recs += pack_records(fam, tag, g, call, planes) + same_out(fam, tag + " second call", a, g)
        recs += same_out(fam, tag + " single-layer call", be.pack_split([call], planes, single=True)[0], g)
    return recs


def ref_pack_f32(it, w):
    G = gathered(it, w)[None]
    return lay_wp(G, 4)[0], lay_wd(G, 4)[0]


def check_pack_f32(be, it):
    """rpnet_pack_conv_weight: exact copies, the padding rows (preset to zero) left as found"""
    fam, recs, w = "pack_f32", [], weights(it)
    written = real_rows(it)
    wp_ref, wd_ref = ref_pack_f32(it, w)
    for want_wd in (1, 0):
        wp0 = torch.where(lay_wp(written, 4)[0], torch.tensor(NAN), torch.tensor(0.0))
        wd0 = torch.where(lay_wd(written, 4)[0], torch.tensor(NAN), torch.tensor(0.0)) if want_wd else None
        got, again = twice(be, lambda: be.pack_f32(it, w, wp0, wd0))
        tag = f"{it.id} wd={want_wd}"
        recs += [exact(fam, tag + " wp", got[0], wp_ref), exact(fam, tag + " wp second call", again[0], got[0])]
        if want_wd:
            recs += [exact(fam, tag + " wd", got[1], wd_ref), exact(fam, tag + " wd second call", again[1], got[1])]
        else:
            assert got[1] is None
    return recs


# ------------------------------------------------------------------------------------------------------------------ collapse
COLLAPSE_SHAPES = [(1, 1), (3, 5), (32, 32), (64, 7)]


def phase_sets():
    """A[p, r, k] = 1 where output phase p (Y & 1) reads tap k from the r-th of its two source rows: output row Y = 2 y + p reads the
    up-sampled rows Y - 1 + k, i.e. the source rows y + floor((p - 1 + k) / 2); the two source rows of a phase are numbered from its
    lowest one"""
    A = torch.zeros(2, 2, 3, dtype=F64)
    for p in range(2):
        d = [(p - 1 + k) // 2 for k in range(3)]
        for k in range(3):
            A[p, d[k] - min(d), k] = 1
    return A


def ref_collapse(w):
    """w [cout, cin, 3, 3] -> (float64 sums [4 cout, cin, 2, 2], float64 sums of |addends|)"""
    A = phase_sets()
    cout, cin = w.shape[:2]
    f = lambda t: torch.einsum("prk,qcl,oikl->pqoirc", A, A, t.double()).reshape(4 * cout, cin, 2, 2)       # noqa: E731
    return f(w), f(w.abs())


def four_phase_conv(x, wc, cout):
    """the layer from its collapsed weights: phase (py, px) of the output is a 2 x 2 convolution of the SOURCE image whose window
    starts one pixel up / left for an even phase.  Interior only: [N, cout, 2 (H - 2), 2 (W - 2)] = output rows 2 .. 2 H - 3"""
    N, _, H, W = x.shape
    y = torch.zeros(N, cout, 2 * H, 2 * W, dtype=x.dtype)
    for py in range(2):
        for px in range(2):
            o = F.conv2d(x, wc[(py * 2 + px) * cout:(py * 2 + px + 1) * cout])           # [N, cout, H - 1, W - 1], window at (y, x)
            ys, xs = (1 if py == 0 else 0), (1 if px == 0 else 0)                          # an even phase reads from y - 1
            y[:, :, 2 * ys + py:2 * (H - 1 + ys):2, 2 * xs + px:2 * (W - 1 + xs):2] = o
    return y[:, :, 2:-2, 2:-2]


def check_collapse(be, cout, cin):
    fam, recs = "collapse", []
    for k in range(9):                                      # one tap set: the 4 x 4 outputs are the 0 / 1 pattern of the phase sets
        w = torch.zeros(cout, cin, 9)
        w[:, :, k] = 1
        got = be.collapse(w.reshape(cout, cin, 3, 3))
        recs.append(exact(fam, f"{cout}x{cin} impulse tap {k}", got, ref_collapse(w.reshape(cout, cin, 3, 3))[0].float()))
    w = rnd(case_seed(cout, cin, 7), cout, cin, 3, 3)
    got, again = be.collapse(w), be.collapse(w)
    ref, mag = ref_collapse(w)
    recs += [within(fam, f"{cout}x{cin} draw", (got.double() - ref).abs(), 3 * 2.0 ** -24 * mag), exact(fam, f"{cout}x{cin} second call", again, got)]
    wi = weights(item(max(cout, 32) // 32 * 32, cin, 9), "integers")[:cout].reshape(cout, cin, 3, 3)
    recs.append(exact(fam, f"{cout}x{cin} integers", be.collapse(wi), ref_collapse(wi)[0].float()))
    return recs


def check_collapse_then_pack(be, planes):
    """rpnet_upconv_collapse_weights, then rpnet_pack_conv_weight_split(taps = 4) on the result, against the reference pack of the
    reference collapse (weights on which the four-term sums are exact)"""
    cout, cin = 32, 32
    w = weights(item(cout, cin, 9), "integers").reshape(cout, cin, 3, 3)
    wc = be.collapse(w)
    it = item(4 * cout, cin, 4)
    call = pack_call(it, wc.reshape(4 * cout, cin, 4), planes, 1)
    got = be.pack_split([call], planes, single=True)[0]
    want = call._replace(w=ref_collapse(w)[0].float().reshape(4 * cout, cin, 4))
    return pack_records(f"pack_split<{planes}>", f"collapsed {it.id}", got, want, planes)


# ------------------------------------------------------------------------------------------------------------------ refusals
# (label, entry, arguments, status, head of rpnet_last_error_string).  "P": the one device buffer, None: NULL; the pack entry takes
# (list of item dicts or None, n, planes).  Every row is refused by a RPNET_REQUIRE on the host: none launches.
_BF = ["P", "P", 1, "P", 4, 8, 3]                        # x, scale, mode, out, rows, C, planes
_F16 = ["P", "P", 1, "P", None, "P", "P", 4, 8, 2, 0]    # x, mask, mode, s_a, s_b, s_out, out, rows, C, planes, a_is_bound
_PR = ["P", "P", "P", 4, 1.0, 1, "P"]                    # measured, bound, scale, n, safety, check, violations
_IT = dict(w="P", wp="P", wd="P", row_scale_wp="P", row_scale_wd="P", cout=32, cin=32, taps=9, cin_off0=0, cin_split=32, cin_off1=32, cin_pad=32)
_PS = ["P", "P", "P", 32, 32, 9, 0, 32, 32, 32, 2, "P", "P"]     # rpnet_pack_conv_weight_split
_PF = ["P", "P", "P", 32, 32, 9, 0, 32, 32, 32]                  # rpnet_pack_conv_weight


def _ch(base, **at):
    out = list(base)
    for k, v in at.items():
        out[int(k[1:])] = v
    return out


def _items(planes=2, n=1, **ch):
    return [[dict(_IT, **ch)], n, planes]


_RANGES = [("cin 0", dict(cin=0, cin_split=0), "cin "), ("cin_split < 0", dict(cin_split=-8), "cin "), ("cin_split > cin", dict(cin_split=40), "cin "),
           ("cin_off0 < 0", dict(cin_off0=-8, cin_pad=64), "cin "), ("cin_off1 < 0", dict(cin_split=16, cin_off1=-8, cin_pad=64), "cin "),
           ("first range exceeds cin_pad", dict(cin_off0=8), "channel ranges exceed"),
           ("second range exceeds cin_pad", dict(cin_split=16, cin_off1=32, cin_pad=32), "channel ranges exceed"),
           ("ranges overlap", dict(cin_split=16, cin_off1=8, cin_pad=64), "channel ranges overlap"),
           ("second range in front overlaps", dict(cin_split=16, cin_off0=8, cin_off1=0, cin_pad=64), "channel ranges overlap")]
_PS_AT = dict(cout=3, cin=4, taps=5, cin_off0=6, cin_split=7, cin_off1=8, cin_pad=9)
_PF_AT = _PS_AT

REFUSALS = (
    [(f"null {n}", "rpnet_split_bf16", _ch(_BF, **{f"a{i}": None}), ARG, "split_bf16: null pointer") for i, n in ((0, "x"), (1, "scale"), (3, "out"))]
    + [(f"{n}", "rpnet_split_bf16", _ch(_BF, **{f"a{i}": v}), SHAPE, "split_bf16: C=") for n, i, v in
       (("C 0", 5, 0), ("C 12", 5, 12), ("C -8", 5, -8), ("planes 2", 6, 2), ("mode 3", 2, 3), ("mode -1", 2, -1))]
    + [("2^32 items", "rpnet_split_bf16", _ch(_BF, a4=1 << 32), SHAPE, "split: ")]
    + [(f"null {n}", "rpnet_split_f16", _ch(_F16, **{f"a{i}": None}), ARG, "split_f16: null pointer") for i, n in ((0, "x"), (1, "mask"), (3, "s_a"), (6, "out"))]
    + [(f"{n}", "rpnet_split_f16", _ch(_F16, **{f"a{i}": v}), SHAPE, "split_f16: C=") for n, i, v in
       (("C 0", 8, 0), ("C 12", 8, 12), ("planes 3", 9, 3), ("planes 0", 9, 0), ("mode 3", 2, 3), ("mode -1", 2, -1))]
    + [("s_b with a_is_bound", "rpnet_split_f16", _ch(_F16, a4="P", a10=1), ARG, "split_f16: s_b must be NULL"),
       ("2^32 items", "rpnet_split_f16", _ch(_F16, a7=1 << 32), SHAPE, "split: ")]
    + [(f"null {n}", "rpnet_predict_scales", _ch(_PR, **{f"a{i}": None}), ARG, "predict_scales: null pointer")
       for i, n in ((0, "measured"), (1, "bound"), (2, "scale"), (6, "violations with check"))]
    + [(n, "rpnet_predict_scales", _ch(_PR, **{f"a{i}": v}), ARG, "predict_scales: n ") for n, i, v in (("n -1", 3, -1), ("safety 0.5", 4, 0.5), ("safety NaN", 4, NAN))]
    + [(f"null {n}", "rpnet_pow2_scale", _ch(["P", "P"], **{f"a{i}": None}), ARG, "pow2_scale: null pointer") for i, n in ((0, "bound"), (1, "s_out"))]
    + [("items NULL", "rpnet_pack_conv_weights_split", [None, 1, 2], ARG, "pack_conv_weights_split: "),
       ("0 items", "rpnet_pack_conv_weights_split", _items(n=0), ARG, "pack_conv_weights_split: 0 items"),
       ("25 items", "rpnet_pack_conv_weights_split", _items(n=25), ARG, "pack_conv_weights_split: 25 items"),
       ("planes 0", "rpnet_pack_conv_weights_split", _items(planes=0), SHAPE, "pack_conv_weights_split: planes"),
       ("planes 4", "rpnet_pack_conv_weights_split", _items(planes=4), SHAPE, "pack_conv_weights_split: planes"),
       ("null w", "rpnet_pack_conv_weights_split", _items(w=None), ARG, "pack_conv_weights_split: null pointer"),
       ("null wp", "rpnet_pack_conv_weights_split", _items(wp=None), ARG, "pack_conv_weights_split: null pointer"),
       ("no row_scale_wp", "rpnet_pack_conv_weights_split", _items(row_scale_wp=None), ARG, "pack_conv_weights_split: fp16 planes"),
       ("no row_scale_wd, one plane", "rpnet_pack_conv_weights_split", _items(planes=1, row_scale_wd=None), ARG, "pack_conv_weights_split: fp16 planes")]
    + [(n, "rpnet_pack_conv_weights_split", _items(**ch), SHAPE, "pack_conv_weights_split: cout ") for n, ch in
       (("cout 48", dict(cout=48)), ("cout 0", dict(cout=0)), ("cout -32", dict(cout=-32)), ("cin_pad 40", dict(cin_pad=40)), ("taps 3", dict(taps=3)))]
    + [(n, "rpnet_pack_conv_weights_split", _items(planes=p, **ch), SHAPE, "pack_conv_weights_split: " + head) for n, ch, head in _RANGES for p in (2, 3)]
    + [(n, "rpnet_pack_conv_weight_split", _ch(_PS, **{f"a{_PS_AT[k]}": v for k, v in ch.items()}), SHAPE, "pack_conv_weights_split: " + head)
       for n, ch, head in _RANGES]
    + [("null wp", "rpnet_pack_conv_weight_split", _ch(_PS, a1=None), ARG, "pack_conv_weights_split: null pointer"),
       ("no row scales", "rpnet_pack_conv_weight_split", _ch(_PS, a11=None), ARG, "pack_conv_weights_split: fp16 planes"),
       ("planes 0", "rpnet_pack_conv_weight_split", _ch(_PS, a10=0), SHAPE, "pack_conv_weights_split: planes")]
    + [(f"null {n}", "rpnet_pack_conv_weight", _ch(_PF, **{f"a{i}": None}), ARG, "pack_conv_weight: null pointer") for i, n in ((0, "w"), (1, "wp"))]
    + [(n, "rpnet_pack_conv_weight", _ch(_PF, **{f"a{i}": v}), SHAPE, "pack_conv_weight: cout ") for n, i, v in
       (("cout 48", 3, 48), ("cout 0", 3, 0), ("cin_pad 30", 9, 30), ("taps 4", 5, 4))]
    + [(n, "rpnet_pack_conv_weight", _ch(_PF, **{f"a{_PF_AT[k]}": v for k, v in ch.items()}), SHAPE, "pack_conv_weight: " + head) for n, ch, head in _RANGES]
    + [(n, "rpnet_upconv_collapse_weights", a, ARG, "upconv_collapse_weights: bad argument") for n, a in
       (("null w", [None, "P", 1, 1]), ("null wc", ["P", None, 1, 1]), ("Cout 0", ["P", "P", 0, 1]), ("Cin -1", ["P", "P", 1, -1]))])


# ------------------------------------------------------------------------------------------------------------------ the host backend
DEFECTS = ["truncate", "second_plane_of_v", "mask_row_by_C", "mode2_uses_f", "min_of_scales", "pow2_binade_high", "bound_as_scale",
           "taps_unflipped", "row_bits_exchanged", "gather_padding_left", "wd_scale_wrong_axis", "odd_phase_even_taps"]
Packed = collections.namedtuple("Packed", "wp wd t u")


def _toward_zero(rounded, v):
    """the 16-bit codes of `rounded` stepped back to the neighbour nearer zero wherever rounding went away from it"""
    code = rounded.view(I16).clone()
    code[rounded.float().abs() > v.abs()] -= 1          # sign-magnitude: one code less is one step toward zero
    return code


class SimBackend:
    """The kernels' index arithmetic on the CPU: which thread reads which element and writes which word.  The element arithmetic
    (one fp32 product, one rounding to a 16-bit format) is torch's; nothing here shares a line with the references above."""

    pure = True

    def __init__(self, defect=None):
        assert defect is None or defect in DEFECTS
        self.defect = defect

    # csrc/split_bf16.h
    def _pow2_bits(self, b):
        u = int(np.float32(max(b, 0.0) if b == b else 0.0).view(np.uint32))
        e = int((u >> 23) & 255) - 127 + (1 if (u & 0x7FFFFF) or (self.defect == "pow2_binade_high" and (u >> 23) & 255) else 0)
        e = min(100, max(-100, e - 15))
        return torch.tensor(np.uint32((e + 127) << 23).view(np.float32), dtype=F32)

    def _split8(self, v, NP):
        trunc = self.defect == "truncate"
        if NP <= 2:
            h = v.half()
            hb = _toward_zero(h, v) if trunc else h.view(I16)
            if NP == 1:
                return [hb]
            r = v if self.defect == "second_plane_of_v" else v - hb.view(torch.float16).float()
            low = r.half()
            return [hb, _toward_zero(low, r) if trunc else low.view(I16)]
        out = []
        for _ in range(3):
            h = v.bfloat16()
            hb = _toward_zero(h, v) if trunc else h.view(I16)
            out.append(hb)
            v = v - hb.view(torch.bfloat16).float()
        return out

    def _split(self, x, mask, mode, inv, NP):
        rows, C = x.shape
        n8, c8 = rows * (C // 8), C // 8
        out = torch.full((NP, rows * C // 8 if rows else 0, 8), NAN16[NP], dtype=I16)
        if rows == 0:
            return out.reshape(NP, rows, C)
        grid = min(n8 // BLOCK + 1, GRID_CAP)
        x8, first, k = x.reshape(-1, 8), torch.arange(grid * BLOCK), 0           # first: blockIdx.x * 256 + threadIdx.x
        while k * grid * BLOCK < n8:
            i = first + k * grid * BLOCK
            i = i[i < n8]
            v = x8[i]
            if mode:
                f = mask[i // (C if self.defect == "mask_row_by_C" else c8)]
                if mode == 2 and self.defect != "mode2_uses_f":
                    f = torch.tensor(1.0, dtype=F32) - f
                v = v * f[:, None]
            if inv is not None:
                v = v * inv
            for p, code in enumerate(self._split8(v, NP)):
                out[p, i] = code
            k += 1
        return out.reshape(NP, rows, C)

    def split_bf16(self, x, mask, mode, offset):
        return self._split(x, mask, mode, None, 3)

    def split_f16(self, x, mask, mode, s_a, s_b, planes, a_is_bound, s_out, offset):
        if a_is_bound and self.defect != "bound_as_scale":
            sc = self._pow2_bits(float(s_a[0]))
        else:
            sb = s_b[0] if s_b is not None and not a_is_bound else torch.tensor(0.0)
            sc = torch.minimum(s_a[0], sb) if (self.defect == "min_of_scales" and s_b is not None) else torch.maximum(s_a[0], sb)
        inv = torch.tensor(1.0, dtype=F32) / sc
        if x.shape[0] == 0:            # the launcher returns before any launch
            sc = torch.tensor(NAN)
        return self._split(x, mask, mode, inv, planes), (sc.clone() if s_out else None)

    def pow2_scale(self, b):
        return self._pow2_bits(float(b[0])).reshape(1)

    def predict_scales(self, m, bound, n, safety, check, viol):
        bound, scale, count = bound.clone(), torch.full((n,), NAN), 0
        for blk in range((n + BLOCK - 1) // BLOCK):
            for t in range(BLOCK):
                i = blk * BLOCK + t
                if i >= n:
                    continue
                if check and not float(m[i]) <= float(bound[i]):
                    count += 1
                s = self._pow2_bits(float(m[i] * torch.tensor(safety, dtype=F32)))
                scale[i], bound[i] = s, s * 32768.0
        return bound, scale, (viol + count if check else None)

    # csrc/conv_split.hip: weight_row_scale_block, pack_weight_split_block
    def _row_scales(self, q, w, t, u):
        wf = w.reshape(-1)
        for b in range(q.cout + q.cin):
            if b < q.cout:
                e = torch.arange(q.cin * q.taps)
                t[b] = self._pow2_bits(float(wf[b * q.cin * q.taps + e].abs().max()))
            else:
                cin = b - q.cout
                e = torch.arange(q.cout * q.taps)
                if self.defect == "wd_scale_wrong_axis":
                    e = torch.arange(q.cin * q.taps)
                    m = wf[min(cin, q.cout - 1) * q.cin * q.taps + e].abs().max()
                else:
                    m = wf[((e // q.taps) * q.cin + cin) * q.taps + e % q.taps].abs().max()
                u[q.off0 + cin if cin < q.split else q.off1 + (cin - q.split)] = self._pow2_bits(float(m))

    def _pack_block(self, NP, gather, bx, by, q, w, wp, wd, t_row, u_row):
        taps, Cin_g, Cout, cin_w = q.taps, q.cin_pad, q.cout, q.cin
        wf, tile = w.reshape(-1), torch.full((9, 32, 33), NAN)
        ci0, co0 = bx * 32, by * 32
        ncin = 32 if gather else min(32, cin_w - ci0)
        src_of = None
        if gather:
            e = torch.arange(32 * 32 * taps)
            col = e // (32 * taps)
            r = e - col * (32 * taps)
            c = r // taps
            tap = r - c * taps
            R = ci0 + c
            src = torch.full_like(R, -1)
            in0 = (R >= q.off0) & (R < q.off0 + q.split)
            in1 = ~in0 & (R >= q.off1) & (R < q.off1 + (cin_w - q.split))
            src[in0], src[in1] = (R - q.off0)[in0], (q.split + (R - q.off1))[in1]
            tile[tap, c, col] = torch.where(src >= 0, wf[((co0 + col) * cin_w + src.clamp_min(0)) * taps + tap], torch.tensor(0.0))
            src_of = {int(cc): int(ss) for cc, ss in zip(c.tolist(), src.tolist())}
        else:
            nel = ncin * taps
            e = torch.arange(32 * nel)
            col = e // nel
            r = e - col * nel
            c = r // taps
            tile[r - c * taps, c, col] = wf[((co0 + col) * cin_w + ci0) * taps + r]
        plane = taps * Cin_g * Cout
        rowmap = lambda cin: cin if gather else torch.where(cin < q.split, q.off0 + cin, q.off1 + (cin - q.split))      # noqa: E731
        e = torch.arange(taps * 32 * 4)
        g, cl, tap = e & 3, (e >> 2) & 31, e >> 7
        on = g * 8 < ncin
        g, cl, tap = g[on], cl[on], tap[on]
        row = rowmap(ci0 + g * 8)
        v = torch.stack([tile[tap, g * 8 + k, cl] for k in range(8)], 1)
        if NP <= 2:
            v = v * (torch.tensor(1.0) / t_row[co0 + cl])[:, None]
        hi, lo = (row >> 5, row & 31) if self.defect != "row_bits_exchanged" else (row & 31, row >> 5)
        dst = ((tap * (Cin_g >> 5) + hi) * Cout + co0 + cl) * 32 + lo
        for p, code in enumerate(self._split8(v, NP)):
            for k in range(8):
                wp[(p * plane + dst + k) % wp.numel()] = code[:, k]
        if wd is None:
            return
        e = torch.arange(taps * 32 * 4)
        g, c, tap = e & 3, (e >> 2) & 31, e >> 7
        on = c < ncin
        if gather and self.defect == "gather_padding_left":
            on = on & torch.tensor([src_of[int(cc)] >= 0 for cc in c.tolist()])
        g, c, tap = g[on], c[on], tap[on]
        row = rowmap(ci0 + c)
        v = torch.stack([tile[tap, c, g * 8 + k] for k in range(8)], 1)
        if NP <= 2:
            v = v * (torch.tensor(1.0) / u_row[row])[:, None]
        tf = tap if self.defect == "taps_unflipped" else taps - 1 - tap
        dst = ((tf * (Cout >> 5) + (co0 >> 5)) * Cin_g + row) * 32 + g * 8
        for p, code in enumerate(self._split8(v, NP)):
            for k in range(8):
                wd[p * plane + dst + k] = code[:, k]

    def pack_split(self, calls, planes, single):
        outs = [Packed(c.wp0.clone().reshape(-1), None if c.wd0 is None else c.wd0.clone().reshape(-1),
                       None if c.t0 is None else c.t0.clone(), None if c.u0 is None else c.u0.clone()) for c in calls]
        its = [c.it for c in calls]
        tiles = lambda q: (q.cin_pad // 32 if needs_gather(q) else (q.cin + 31) // 32)       # noqa: E731
        max_rows, max_tiles = max(q.cout + q.cin for q in its), max(tiles(q) * (q.cout // 32) for q in its)
        for y, (c, o) in enumerate(zip(calls, outs)):                   # blockIdx.y = layer
            q = c.it
            if planes <= 2:
                assert max_rows >= q.cout + q.cin                       # blocks beyond an item's rows return at once
                self._row_scales(q, c.w, o.t, o.u)
            tx = tiles(q)
            for bxy in range(max_tiles):
                if bxy >= tx * (q.cout // 32):
                    continue
                self._pack_block(planes, needs_gather(q), bxy % tx, bxy // tx, q, c.w, o.wp, o.wd, o.t, o.u)
        return [Packed(o.wp.reshape(c.wp0.shape), None if o.wd is None else o.wd.reshape(c.wd0.shape), o.t, o.u) for c, o in zip(calls, outs)]

    # csrc/conv_wgrad.hip: pack_weight_kernel
    def pack_f32(self, q, w, wp0, wd0):
        wp, wd, wf = wp0.clone().reshape(-1), None if wd0 is None else wd0.clone().reshape(-1), w.reshape(-1)
        taps, Cin_g, Cout = q.taps, q.cin_pad, q.cout
        for bx in range((q.cin + 31) // 32):
            for by in range(Cout // 32):
                ci0, co0 = bx * 32, by * 32
                ncin = min(32, q.cin - ci0)
                nel, tile = ncin * taps, torch.full((9, 32, 33), NAN)
                e = torch.arange(32 * nel)
                col = e // nel
                r = e - col * nel
                c = r // taps
                tile[r - c * taps, c, col] = wf[((co0 + col) * q.cin + ci0) * taps + r]
                e = torch.arange(taps * 32 * 32)
                cl, c, tap = e & 31, (e >> 5) & 31, e >> 10
                on = c < ncin
                cl, c, tap = cl[on], c[on], tap[on]
                cin = ci0 + c
                row = torch.where(cin < q.split, q.off0 + cin, q.off1 + (cin - q.split))
                wp[((tap * (Cin_g >> 2) + (row >> 2)) * Cout + co0 + cl) * 4 + (row & 3)] = tile[tap, c, cl]
                if wd is not None:
                    k4, c, cq, tap = e & 3, (e >> 2) & 31, (e >> 7) & 7, e >> 10
                    on = c < ncin
                    k4, c, cq, tap = k4[on], c[on], cq[on], tap[on]
                    cin = ci0 + c
                    row = torch.where(cin < q.split, q.off0 + cin, q.off1 + (cin - q.split))
                    cout = co0 + cq * 4 + k4
                    wd[(((taps - 1 - tap) * (Cout >> 2) + (cout >> 2)) * Cin_g + row) * 4 + k4] = tile[tap, c, cq * 4 + k4]
        return wp.reshape(wp0.shape), None if wd is None else wd.reshape(wd0.shape)

    # csrc/conv_up4_dma.hip: upconv_collapse_kernel
    def collapse(self, w):
        Cout, Cin = w.shape[:2]
        i = torch.arange(4 * Cout * Cin)
        ci, co, ph = i % Cin, (i // Cin) % Cout, i // (Cin * Cout)
        k = w.reshape(-1)[((co * Cin + ci) * 9)[:, None] + torch.arange(9)]
        py, px = ph >> 1, ph & 1
        if self.defect == "odd_phase_even_taps":
            py, px = torch.zeros_like(py), torch.zeros_like(px)
        o = torch.zeros(len(i), 4)
        for r in range(2):
            for c in range(2):
                ya = torch.zeros_like(py) if r == 0 else torch.where(py > 0, 2, 1)
                yb = torch.where(py > 0, 1, 0) if r == 0 else torch.full_like(py, 2)
                xa = torch.zeros_like(px) if c == 0 else torch.where(px > 0, 2, 1)
                xb = torch.where(px > 0, 1, 0) if c == 0 else torch.full_like(px, 2)
                s = torch.zeros(len(i))
                for ky in range(3):
                    for kx in range(3):
                        on = (ky >= ya) & (ky <= yb) & (kx >= xa) & (kx <= xb)
                        s = torch.where(on, s + k[:, ky * 3 + kx], s)
                o[:, r * 2 + c] = s
        return o.reshape(4 * Cout, Cin, 2, 2)
