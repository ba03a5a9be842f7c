"""Cases and comparison functions shared by tests/test_host_conv_ref64.py and tests/test_gpu_conv_fp64.py: the convolution forward
and input gradient (rpnet_conv_fwd: csrc/conv_igemm.hip on fp32 operands, csrc/conv_split.hip / conv_split_dma.hip on operand planes,
all through csrc/conv_epilogue.h; rpnet_conv_up4: csrc/conv_up4_dma.hip) against tests/ref64.py conv_fwd / conv_dgrad at every branch
of the dispatch.  The layout is that of tests/wgrad_cases.py; the definitions of tests/corr_cases.py (split_planes, plane_values,
pow2_scale, case_seed, FACTOR, FLOOR, Rec, measure, exact, hold, split_unit_roundoff) are used, not restated.  The weight packs are
made on the host with the layouts of tests/operand_cases.py (lay_wp, lay_wd, ref_pow2), which tests/test_gpu_operands.py holds to
the device packers bit for bit: what the planes of a pack represent is therefore known exactly.

A *backend* runs ONE launch described by a Case and its operands (Launch) on CPU tensors: the HIP library (the GPU test) or
SimBackend, a float32 torch restatement on the values the planes hold, with the kernels' dropped products, with or without a
seeded defect (the host test).

Bound: rel_err(got, r64) <= FACTOR * yard + FLOOR, yard = rel_err(r32, r64), r32 the same reference in float32; taken per block
of 32 consecutive pixels x 64 output channels relative to that block's own reference maximum (per_block), and over the whole
tensor.  Plane operands: the reference is evaluated on the values the planes represent; the products the kernels leave out on
purpose get dropped_term(), the reasoning of tests/wgrad_cases.py with the weight in the place of dy:
  two fp16 planes   x = s (h + l), |l| <= u (|x| + 2^-13 s)(1 + u), u = split_unit_roundoff(1), the same for a weight row on its
                    row scale: the sequence is l.h, h.l, h.h, l.l is dropped: <= u^2 (1 + u)^2 sum (|x| + 2^-13 sx)(|w| + 2^-13 t);
  three bf16 planes dropped are m.l, l.m and l.l: <= (2 v^3 + v^4)(1 + v)^2 sum |x||w|, v = 2^-8, v^3 = split_unit_roundoff(3);
  one plane         drops nothing.
The allowance is formed on the accumulator and follows it through the epilogue: times |ep_scale| and |out_scale factor| (the ReLU
does not stretch it), summed over the 2 x 2 pixels of rpnet_upsample2_bwd.  The collapsed up-conv rows take their reference
(ref64.upconv_collapsed / upconv_collapsed_dgrad) on the values the FOUR-tap pack of the collapsed weights represents, the nine-tap
form of the same layer on the same source planes takes its own (ref64.conv_fwd / conv_dgrad on what the nine-tap pack represents):
the two packs round the weights at different places, so each form is held to the float64 result of its own operands, with the
same bound and its own dropped_term().
Every record keeps the error BEFORE the allowance is taken off as `raw`, so that a run's lines show the margin where err is 0.
Exact checks (guard words, no NaN left, out_absmax, y_split planes, statistics, repeats, skipped tiles, impulses) count mismatching
elements and allow none.  No check carries a measured factor.

Every instantiation of conv_igemm_kernel has rows.  <1, 2> is never chosen at 64 or 128 output channels (at one column tile its
ceil(M / 64) tiles never fill the 1024 slots better than the 2 ceil(M / 128) tiles of <2, 1>), but at 384 it is from M = 21761:
341 x 3 = 1023 tiles fill 1024 slots 0.999, against 513 / 768 for <2, 2> and 1026 / 2048 for <2, 1>; the output is 32 MiB.
<1, 1> is reached from M = 7873 at 64 output channels (124 tiles of 64 rows fill 1536 slots 0.0807, 62 tiles of 128 rows fill 1024
slots 0.0605), and already at 3 x 16 x 48 with 128 output channels (noted beside the table).  test_host_conv_ref64.py searches
every M within the 64 MiB limit for these statements."""
import math

import torch
import torch.nn.functional as F

from tests import corr_cases as CC
from tests import operand_cases as OC
from tests import ref64 as R
from tests.corr_cases import ARG, FACTOR, FLOOR, SHAPE, U_BF16, WORKSPACE, case_seed, plane_values, pow2_scale, split_planes, split_unit_roundoff  # noqa: F401
from tests.helpers import rnd

F32, F64 = torch.float32, torch.float64
GUARD = 64                      # words behind every output and workspace that must come back as they went in
NAN = float("nan")


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------------- cases
class Case:
    """one launch.  fam: fp32 | planes | up4.  N, H, W: the launch's d->N, H, W (the OUTPUT's size; rpnet_conv_up4 mode 2: the size
    of dy, the output is half of it).  C0 | C1: the sources, Co0 | Co1: the destinations.  dgrad: the launch reads dy and the `wd`
    pack (up_bwd: rpnet_upsample2_bwd behind it).  up4: the mode of rpnet_conv_up4.  ep: epilogue features, blank-separated:
    bias aff relu os1 os2 acc stats amax ys3 ys2 ys1 skip<mode><halo><a|t>.  sx1 "own": source x1 on its own tensor scale, 2^5 times
    x0's.  splitk: the launch is lent the split-K workspace.  kernel: what the row is meant to reach (route())."""

    def __init__(self, fam, nhw, C0, Co0, kernel, C1=0, Co1=0, taps=9, dil=1, ups=0, mode=0, planes=0, tune=0, groups=1, ep="",
                 sx1=None, dgrad=0, up_bwd=0, up4=0, splitk=0):
        self.fam, (self.N, self.H, self.W), self.C0, self.C1, self.Co0, self.Co1, self.kernel = fam, nhw, C0, C1, Co0, Co1, kernel
        self.taps, self.dil, self.ups, self.mode, self.planes, self.tune, self.groups = taps, dil, ups, mode, planes, tune, groups
        self.ep, self.sx1, self.dgrad, self.up_bwd, self.up4, self.splitk = ep, sx1, dgrad, up_bwd, up4, splitk

    M = property(lambda s: s.N * s.H * s.W)
    Cin = property(lambda s: s.C0 + s.C1)
    Cout = property(lambda s: s.Co0 + s.Co1)
    feats = property(lambda s: set(s.ep.split()))
    entry = property(lambda s: "rpnet_conv_up4" if s.fam == "up4" else "rpnet_conv_fwd")
    src_hw = property(lambda s: (s.H >> 1, s.W >> 1) if (s.ups or s.up4 == 1) else (s.H, s.W))
    out_hw = property(lambda s: (s.H >> 1, s.W >> 1) if (s.up_bwd or s.up4 == 2) else (s.H, s.W))
    ys_planes = property(lambda s: next((int(f[2]) for f in s.feats if f[:2] == "ys"), 0))
    os_mode = property(lambda s: 1 if "os1" in s.feats else 2 if "os2" in s.feats else 0)
    skip = property(lambda s: next((f for f in s.feats if f.startswith("skip")), None))

    def has(self, f):
        return f in self.feats

    def but(self, **kw):
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.__dict__.update(kw)
        return c

    @property
    def id(self):
        return (f"{self.fam}-{self.N}x{self.H}x{self.W}-{self.C0}" + (f"+{self.C1}" if self.C1 else "") + f"to{self.Co0}"
                + (f"+{self.Co1}" if self.Co1 else "") + (f"-p{self.planes}" if self.planes else "") + (f"-v{self.tune - 1}" if self.tune else "")
                + (f"-d{self.dil}" if self.dil > 1 else "") + ("-1x1" if self.taps == 1 else "") + ("-up" if self.ups else "")
                + (f"-is{self.mode}" if self.mode else "") + (f"-g{self.groups}" if self.groups > 1 else "") + ("-sx1" if self.sx1 else "")
                + ("-dgrad" if self.dgrad else "") + ("-upbwd" if self.up_bwd else "") + (f"-mode{self.up4}" if self.up4 else "")
                + ("-splitk" if self.splitk else "") + ("-" + "+".join(sorted(self.feats)) if self.ep else ""))


# ------------------------------------------------------------------------------------------- the launchers' conditions, restated
def n128(c):
    return c.Cout % 128 == 0 and (c.Co1 == 0 or c.Co0 % 128 == 0)


def choose_tile(M, Cout, wide):
    """choose_tile (csrc/conv_igemm.hip): index into (<2,2>, <2,1>, <1,2>, <1,1>), the best fill of the block slots by 0.02"""
    best, best_fill = -1, -1.0
    for i, (wm, wn, slots) in enumerate(((2, 2, 768), (2, 1, 1024), (1, 2, 1024), (1, 1, 1536))):
        if wn == 2 and not wide:
            continue
        tiles = _cdiv(M, 64 * wm) * (Cout // (64 * wn))
        fill = tiles / (_cdiv(tiles, slots) * slots)
        if fill > best_fill + 0.02:
            best, best_fill = i, fill
    return best


IGEMM = ("igemm<2,2>", "igemm<2,1>", "igemm<1,2>", "igemm<1,1>")
# variant -> (rows of the block tile, columns): kSplitVariants (csrc/conv_split.hip), those still instantiated
VARIANT_TILE = {0: (128, 128), 1: (128, 64), 2: (64, 128), 3: (64, 64), 7: (256, 128), 8: (128, 128), 9: (128, 64), 11: (256, 128),
                12: (256, 64), 13: (256, 128), 14: (128, 64)}
PATCH_VARIANTS = (7, 8, 9, 11, 12, 13, 14)
DMA_VARIANTS = (11, 12, 13, 14)


def halo_tw(c):
    if c.taps != 9 or c.dil > 1:
        return 0
    return 32 if c.W % 32 == 0 and c.H % 8 == 0 else 16 if c.W % 16 == 0 and c.H % 16 == 0 else 0


def halo4_tw(c):
    if c.taps != 9 or c.dil > 1:
        return 0
    return 32 if c.W % 32 == 0 and c.H % 4 == 0 else 16 if c.W % 16 == 0 and c.H % 8 == 0 else 0


def halo_bn(c):
    return 128 if n128(c) else 64


def dma_addressable(c):
    hs, ws = c.src_hw
    msrc, np_, lim = c.N * hs * ws, max(c.planes, 1), 1 << 31
    return np_ * msrc * c.C0 * 2 < lim and np_ * msrc * c.C1 * 2 < lim and np_ * 9 * c.Cin * c.Cout * 2 < lim


def choose_tile_split(c):
    """choose_tile_split (csrc/conv_split.hip): the tile variant of a launch on operand planes"""
    M, Cout, addr, hbn = c.M, c.Cout, dma_addressable(c), halo_bn(c)
    if c.tune > 0:
        v = (c.tune & 0xff) - 1
        if v in (12, 14) and c.planes == 2 and halo_tw(c) and addr:
            return v
        if v == 13 and c.planes == 1 and halo_tw(c) and hbn == 128 and c.Cin % 64 == 0 and c.C0 % 64 == 0 and addr:
            return v
        if ((v == 7 or (v == 11 and c.planes == 2 and addr)) and halo_tw(c) and hbn == 128) or (v in (8, 9) and halo4_tw(c)):
            return v
        if 0 <= v < 4 and (VARIANT_TILE[v][1] == 64 or n128(c)):
            return v
    old = bool(c.tune & 0x10000)
    if c.planes == 1 and not old and addr and hbn == 128 and halo_tw(c) and c.Cin % 64 == 0 and c.C0 % 64 == 0 and (M // 256) * (Cout // 128) >= 192:
        return 13
    dma = c.planes == 2 and not old and addr
    if hbn == 128 and halo_tw(c) and (M // 256) * (Cout // 128) >= (192 if dma else 224):
        return 11 if dma else 7
    if dma and halo_tw(c) and c.Cin >= 128 and (M // 256) * (Cout // 64) >= 128:
        return 12
    if halo4_tw(c):
        if hbn == 128 and (M // 128) * (Cout // hbn) >= 1024:
            return 8
        if (M // 128) * (Cout // 64) >= 64:
            return 9
    best, best_fill = -1, -1.0
    for v, slots in ((0, 768), (1, 1024), (2, 1024), (3, 1536)):
        bm, bn = VARIANT_TILE[v]
        if bn == 128 and not n128(c):
            continue
        tiles = _cdiv(M, bm) * (Cout // bn)
        fill = tiles / (_cdiv(tiles, slots) * slots)
        if fill > best_fill + 0.02:
            best, best_fill = v, fill
    return best


def splitk_parts(c):
    """conv_splitk_parts (csrc/conv_split_dma.hip) behind splitk_parts_for (csrc/conv_split.hip)"""
    if not halo_tw(c) or not dma_addressable(c):
        return 1
    if c.planes != 2 or c.tune or c.taps != 9 or c.dil > 1 or c.Cin < 128 or c.M % 256:
        return 1
    if c.has("stats") or c.has("acc") or c.os_mode or c.Co1 or c.sx1 or c.groups > 1:
        return 1
    tiles, kchunks = (c.M // 256) * (c.Cout // 64), c.Cin >> 5
    if tiles > 128 or (tiles > 64 and kchunks < 32):
        return 1
    parts = 1
    while parts < 8 and tiles * parts * 2 <= 256 and kchunks % (parts * 2) == 0 and kchunks // (parts * 2) >= 2:
        parts *= 2
    return parts


def splitk_bytes(c):
    """what rpnet_conv_splitk_workspace_bytes must answer"""
    p = splitk_parts(c) if c.planes and c.taps == 9 else 1
    return p * c.M * c.Cout * 4 if p > 1 else 0


def up4_plan(c, mode):
    """up4_plan (csrc/conv_up4_dma.hip): (tw, wn), wn = 0: the shapes do not fit"""
    if c.planes not in (1, 2) or c.H % 2 or c.W % 2 or c.C1 or c.Co1:
        return 0, 0
    Hl, Wl, one = c.H // 2, c.W // 2, c.planes == 1
    tw = 32 if Wl % 32 == 0 and Hl % 8 == 0 else 16 if Wl % 16 == 0 and Hl % 16 == 0 else 0
    if not tw or c.C0 % (64 if one else 32) or c.Co0 % (128 if one else 64):
        return 0, 0
    if mode == 1:
        return tw, 2 if c.Co0 % 128 == 0 else 1
    if one:
        return tw, 2
    return tw, 2 if c.Co0 % 128 == 0 and (c.N * Hl * Wl // 256) * (c.Co0 // 128) >= 192 else 1


def variant(c):
    return choose_tile_split(c) if c.fam == "planes" else -1


def route(c):
    """the kernel the launchers pick for a case; every table row is asserted against it"""
    if c.fam == "up4":
        tw, wn = up4_plan(c, c.up4)
        return f"up4<mode {c.up4},tw {tw},wn {wn}" + (",K64>" if c.planes == 1 else ">") if wn else "refused"
    if c.fam == "fp32":
        return IGEMM[choose_tile(c.M, c.Cout, n128(c))] + ("+in_scale" if c.mode else "")
    if c.splitk and splitk_parts(c) > 1:
        return f"splitk x{splitk_parts(c)}"
    return f"v{choose_tile_split(c)}"


def tile_rows(c):
    """rows of the block tile (LinearRows: consecutive pixels; the patch kernels: a patch of one image)"""
    if c.fam == "up4":
        return 256
    if c.fam == "fp32":
        return 128 if choose_tile(c.M, c.Cout, n128(c)) < 2 else 64
    return VARIANT_TILE[choose_tile_split(c)][0]


def stats_blocks(c):
    """rpnet_conv_stats_blocks / rpnet_conv_up4_stats_blocks: partial rows per statistic group, 0: refused"""
    if c.N % c.groups:
        return 0
    per = (c.N // c.groups) * c.H * c.W
    return per // tile_rows(c) if per % tile_rows(c) == 0 else 0


def patch_rows(c):
    return c.fam == "up4" or (c.fam == "planes" and (choose_tile_split(c) in PATCH_VARIANTS or (c.splitk and splitk_parts(c) > 1)))


def epilogue_instance(c):
    """(AFF, ROWOPS) of conv_epilogue_store as conv_epilogue resolves them"""
    return (c.has("aff") or c.has("relu"), bool(c.os_mode or c.has("acc") or c.has("amax") or c.ys_planes))


def patch_shape(c):
    """(rows, columns) of the image patch a block of a patch kernel owns"""
    if c.fam == "up4":
        tw = up4_plan(c, c.up4)[0]
        return 256 // tw, tw
    v = choose_tile_split(c)
    if c.splitk and splitk_parts(c) > 1:
        v = 12
    tw = halo4_tw(c) if v in (8, 9) else halo_tw(c)
    return VARIANT_TILE[v][0] // tw, tw


# ------------------------------------------------------------------------------------------------------------------ tables
def _f(nhw, C0, Co0, kernel, **kw):
    return Case("fp32", nhw, C0, Co0, kernel, **kw)


def _p(planes, v, nhw, C0, Co0, **kw):
    """plane operands; v: the forced variant (None: the default policy; then `kernel` names what it gives)"""
    kernel = kw.pop("kernel", None)
    return Case("planes", nhw, C0, Co0, kernel or f"v{v}", planes=planes, tune=0 if v is None else v + 1, **kw)


# 1. fp32 operands: conv_igemm_kernel<WM, WN, INSCALE>, LinearRows.  Every shape carries every form of the gather, at 64 and at 128
# output channels.  M = 35: one partial tile, rows past the tensor.  2 x 5 x 7 (2 x 6 x 10) in two statistic groups: the one 128-row
# tile straddles them, the affine is looked up per row.  1 x 1 x 1: every tap but the centre is outside.  Up-sampling needs even
# sizes: 6 x 10 stands for 5 x 7 and 2 x 2 for 1 x 1.
FP32_SHAPES = [(1, 5, 7), (2, 5, 7), (3, 16, 48), (1, 1, 1), (1, 2, 2)]
FP32_FORMS = [dict(), dict(taps=1), dict(dil=2), dict(mode=1), dict(mode=2), dict(C1=32), dict(ups=1)]
_EVEN = {(1, 5, 7): (1, 6, 10), (2, 5, 7): (2, 6, 10), (1, 1, 1): (1, 2, 2)}


def _fx(s, cout, **kw):
    """an fp32 row named by the rule of the table: 128-row tiles at these sizes, except 3 x 16 x 48 at 128 output channels, where 72
    tiles of 64 x 64 fill 1536 slots 0.047 and 18 of 128 x 128 fill 768 slots 0.023: <1,1>"""
    if kw.get("ups"):
        s = _EVEN.get(s, s)
    if s[0] == 2:
        kw.update(groups=2, ep="aff")
    m = s[0] * s[1] * s[2]
    k = "igemm<1,1>" if (cout == 128 and m == 2304) else "igemm<2,2>" if cout == 128 else "igemm<2,1>"
    return _f(s, 32, cout, k + ("+in_scale" if kw.get("mode") else ""), **kw)


def _unique(rows):
    return list({c.id: c for c in rows}.values())


FP32 = _unique([_fx(s, co, **f) for s in FP32_SHAPES for f in FP32_FORMS for co in (64, 128)]) + [
    _f((1, 5, 7), 64, 128, "igemm<2,2>"), _f((3, 16, 48), 64, 64, "igemm<2,1>"),                        # two channel chunks
    _f((1, 16, 48), 32, 128, "igemm<2,2>"), _f((1, 16, 48), 32, 128, "igemm<2,2>", dil=2), _f((1, 16, 48), 32, 128, "igemm<2,2>+in_scale", mode=2),
    _f((1, 16, 48), 32, 128, "igemm<2,2>", C1=32, taps=1), _f((1, 16, 48), 32, 128, "igemm<2,2>", ups=1),     # six tiles of <2,2>
    _f((1, 1, 1), 32, 64, "igemm<2,1>", C1=32, taps=1), _f((1, 5, 7), 32, 64, "igemm<2,1>", C1=32, dil=2),
    _f((2, 8, 8), 32, 64, "igemm<2,1>+in_scale", ups=1, mode=1),                   # in_scale is indexed by the SOURCE pixel
    _f((2, 5, 7), 32, 64, "igemm<2,1>", groups=2, ep="bias aff relu"),
    # 64 output channels: the smallest M (but one) at which the fill rule takes 64-row tiles (module docstring): 124 tiles, the last two rows long
    _f((1, 127, 62), 32, 64, "igemm<1,1>"), _f((1, 127, 62), 32, 64, "igemm<1,1>+in_scale", mode=1, ep="bias"),
    # 384 output channels: 341 x 3 tiles of 64 x 128 (module docstring); 311 x 70 = 21770 pixels: the last tile ten rows long
    _f((1, 341, 64), 32, 384, "igemm<1,2>"), _f((1, 311, 70), 32, 384, "igemm<1,2>+in_scale", mode=2, ep="bias")]
assert 127 * 62 == 7874 and -(-311 * 70 // 64) == 341

# 2. plain split kernels, variants 0 - 3: conv_igemm_split_kernel<2, WM, WN, NP>, LinearRows
ODD = [(1, 5, 7), (3, 16, 48), (1, 1, 1), (1, 2, 2)]
PLAIN = ([_p(p, v, s, 32, 128 if v in (0, 2) else 64) for p in (3, 2, 1) for v in range(4) for s in ((1, 5, 7), (3, 16, 48))] + [
    _p(p, 1, s, 64, 64) for p in (3, 2, 1) for s in ((1, 1, 1), (1, 2, 2))] + [
    _p(p, 1, (1, 5, 7), 32, 64, dil=2) for p in (3, 2, 1)] + [_p(2, 0, (3, 16, 48), 32, 128, dil=2)] + [
    _p(p, 3, (1, 5, 7), 32, 64, C1=32, taps=1, sx1="own") for p in (2, 1)] + [
    _p(2, 0, (3, 16, 48), 64, 128, C1=32, taps=1, sx1="own"), _p(3, 1, (3, 16, 48), 32, 64, C1=32, taps=1),
    _p(2, 1, (1, 6, 10), 32, 64, ups=1), _p(3, 0, (1, 5, 7), 32, 128, C1=32),
    _p(2, None, (1, 5, 7), 32, 64, kernel="v1"), _p(3, None, (1, 5, 7), 32, 128, kernel="v0")])      # the default policy at a small grid

# 3. patch kernels, PatchRows
PATCH = [
    # one patch per image: all four borders in one block
    _p(3, 7, (1, 8, 32), 32, 128), _p(2, 7, (1, 16, 16), 32, 128), _p(1, 7, (1, 8, 32), 32, 128),
    _p(2, 8, (1, 4, 32), 32, 128), _p(3, 8, (1, 8, 16), 32, 128), _p(2, 9, (1, 4, 32), 32, 64), _p(1, 9, (1, 8, 16), 32, 64),
    _p(2, 11, (1, 8, 32), 32, 128), _p(2, 11, (1, 16, 16), 32, 128),
    _p(2, 12, (1, 8, 32), 32, 64), _p(2, 12, (1, 16, 16), 32, 64), _p(2, 14, (1, 8, 32), 32, 64), _p(2, 14, (1, 16, 16), 32, 64),
    _p(1, 13, (1, 8, 32), 64, 128), _p(1, 13, (1, 16, 16), 64, 128),
    # 2 x 2 patches per image (each seam read from a neighbour) and two images (a top halo is the previous image's last row)
    _p(2, 7, (2, 16, 64), 32, 128), _p(2, 11, (2, 16, 64), 32, 128), _p(2, 11, (2, 32, 32), 32, 128), _p(2, 12, (2, 16, 64), 32, 64),
    _p(2, 14, (2, 32, 32), 32, 64), _p(1, 13, (2, 16, 64), 64, 128), _p(3, 9, (2, 8, 64), 32, 64), _p(2, 8, (2, 16, 32), 32, 128),
    # two sources with the seam inside a K chunk of 128 channels, up-sampling, two destinations, two channel chunks
    _p(2, 11, (2, 8, 32), 32, 128, C1=96), _p(2, 12, (2, 8, 32), 64, 64, C1=64), _p(1, 13, (2, 8, 32), 64, 128, C1=64),
    _p(2, 7, (2, 8, 32), 32, 128, C1=96),
    _p(2, 11, (2, 16, 64), 32, 128, ups=1), _p(2, 14, (2, 16, 64), 32, 64, ups=1), _p(1, 13, (2, 16, 64), 64, 128, ups=1),
    _p(3, 7, (2, 16, 64), 32, 128, ups=1), _p(2, 9, (2, 8, 64), 32, 64, ups=1),
    _p(2, 11, (2, 8, 32), 64, 128, Co1=128), _p(2, 12, (2, 8, 32), 64, 64, Co1=64), _p(3, 9, (2, 8, 32), 64, 64, Co1=64),
    _p(2, 11, (2, 8, 32), 64, 128), _p(2, 12, (2, 8, 32), 64, 64), _p(1, 13, (2, 8, 32), 128, 128)]

# 4. split K: the smallest shape for which rpnet_conv_splitk_workspace_bytes is non-zero: one tile, four chunks -> two parts
SPLITK = [_p(2, None, (1, 8, 32), 128, 64, splitk=1, kernel="splitk x2", ep="bias aff relu amax"),
          _p(2, None, (1, 8, 32), 96, 64, C1=32, splitk=1, kernel="splitk x2"),        # the second part straddles the two sources
          _p(2, None, (2, 16, 16), 256, 64, splitk=1, kernel="splitk x4", ep="bias ys2")]

# 5. the epilogue matrix: each feature alone, then all compatible ones together
_LIN, _PAT, _PAT7 = _p(2, 0, (2, 5, 7), 32, 128), _p(2, 11, (2, 8, 32), 32, 128), _p(3, 7, (2, 8, 32), 32, 128)
EP_FEATURES = ["bias", "aff", "aff relu", "os1", "os2", "acc", "stats", "amax", "ys3", "ys2", "ys1", "bias aff relu os2 acc amax ys2"]
EPILOGUE = ([b.but(ep=e, groups=g) for b in (_LIN, _PAT) for e in EP_FEATURES for g in ((1, 2) if "aff" in e else (1,))
             if not (b is _LIN and e == "stats")] + [
    # statistics need whole tiles per group: M = 70 is refused (REFUSALS), 128 rows per group are one tile
    _p(2, 0, (2, 8, 8), 32, 128, ep="stats bias"), _p(2, 0, (4, 8, 8), 32, 128, ep="stats bias", groups=2),
    _PAT.but(ep="stats bias aff relu", groups=2), _PAT.but(Co1=128, ep="bias os1 acc"), _LIN.but(Co1=128, ep="bias os1 acc"),
    _PAT7.but(ep="bias aff relu os1 acc amax ys3", groups=2), _PAT7.but(ep="stats"), _f((2, 5, 7), 32, 128, "igemm<2,2>", ep="os1 acc amax ys3"),
    _f((4, 8, 8), 32, 64, "igemm<2,1>", ep="stats bias", groups=2), _f((2, 5, 7), 32, 64, "igemm<2,1>", ep="ys1 bias", Co1=0)])
# skip_mask on the DMA kernels.  a: the mask zeroes one whole tile and its halo, t: the tile but not its halo
SKIP = [_p(2, v, (2, 16, 64), 32, co, ep=f"bias skip{m}{h}{k}" + (f" os{m}" if h == 0 else ""))
        for v, co in ((11, 128), (12, 64)) for m in (1, 2) for h in (0, 1) for k in "at"] + [
    _p(1, 13, (2, 16, 64), 64, 128, ep="bias skip11a"), _p(2, 14, (2, 16, 64), 32, 64, ep="bias skip20a os2")]

# 6. the input gradient: the same kernels on the `wd` pack with dy as the source
DGRAD = [_f((1, 5, 7), 64, 64, "igemm<2,1>", dgrad=1), _f((3, 16, 48), 128, 64, "igemm<2,1>", Co1=64, dgrad=1),
         _p(3, 0, (1, 5, 7), 64, 128, dgrad=1), _p(2, 1, (3, 16, 48), 64, 64, Co1=64, dgrad=1), _p(1, 3, (1, 5, 7), 64, 64, dgrad=1),
         _p(2, 11, (2, 8, 32), 64, 128, Co1=128, dgrad=1), _p(2, 12, (2, 16, 16), 64, 64, Co1=64, dgrad=1), _p(1, 13, (2, 8, 32), 64, 128, dgrad=1),
         _p(2, 3, (1, 5, 7), 64, 64, taps=1, dgrad=1),
         _p(2, 11, (2, 16, 64), 64, 128, dgrad=1, up_bwd=1), _p(1, 13, (2, 16, 64), 64, 128, dgrad=1, up_bwd=1), _f((1, 6, 10), 64, 64, "igemm<2,1>", dgrad=1, up_bwd=1)]
# the CRE's two masked branches: out_scale_mode 1, then mode 2 accumulated into the same tensor
CRE_PAIRS = [_p(2, 11, (2, 8, 32), 64, 128, dgrad=1), _p(2, 0, (2, 5, 7), 64, 128, dgrad=1), _f((2, 5, 7), 64, 64, "igemm<2,1>", dgrad=1)]


def _u(planes, mode, nhw, C0, Co0, **kw):
    c = Case("up4", nhw, C0, Co0, "", planes=planes, up4=mode, dgrad=int(mode == 2), **kw)
    c.kernel = route(c)
    return c


# 7. the collapsed up-conv.  N, H, W: the HIGH resolution.  Mode 2 reads dy [N, H, W, C0] and writes dx [N, H/2, W/2, Co0]
UP4 = ([_u(2, 1, s, 32, co, ep=e) for s in ((1, 32, 32), (1, 16, 64)) for co, e in ((64, "bias stats amax"), (128, "bias"))] + [
    _u(1, 1, s, 64, 128, ep="bias stats amax") for s in ((1, 32, 32), (1, 16, 64))] + [_u(2, 1, (2, 32, 32), 32, 64, ep="bias stats", groups=2)] + [
    _u(2, 2, s, c0, co) for s in ((1, 32, 32), (1, 16, 64)) for c0, co in ((32, 64), (64, 128))] + [_u(2, 2, (2, 16, 64), 64, 64, ep="amax")] + [
    _u(1, 2, s, 64, 128) for s in ((1, 32, 32), (1, 16, 64))])
# rpnet_conv_up4_supported must answer 0 on each condition of up4_plan
UP4_UNSUPPORTED = [("odd height", _u(2, 1, (1, 31, 32), 32, 64)), ("odd width", _u(2, 1, (1, 32, 31), 32, 64)),
                   ("a second source", _u(2, 1, (1, 32, 32), 32, 64, C1=32)), ("a second destination", _u(2, 1, (1, 32, 32), 32, 64, Co1=64)),
                   ("C0 = 48", _u(2, 1, (1, 32, 32), 48, 64)), ("Co0 = 96", _u(2, 1, (1, 32, 32), 32, 96)),
                   ("one plane, C0 = 32", _u(1, 1, (1, 32, 32), 32, 128)), ("one plane, Co0 = 64", _u(1, 1, (1, 32, 32), 64, 64)),
                   ("three planes", _u(3, 1, (1, 32, 32), 32, 64)), ("low resolution 8 x 8", _u(2, 1, (1, 16, 16), 32, 64)),
                   ("mode 2, odd height", _u(2, 2, (1, 31, 32), 32, 64))]

# 8. source channels of magnitude 2^-20 .. 2^0 under one tensor scale, judged per output channel
DYNAMIC = [_p(2, 1, (3, 16, 48), 64, 64), _p(1, 1, (3, 16, 48), 64, 64), _p(2, 11, (2, 8, 32), 64, 128), _p(1, 13, (2, 8, 32), 64, 128)]

TABLES = {"fp32": FP32, "plain": PLAIN, "patch": PATCH, "splitk": SPLITK, "epilogue": EPILOGUE, "skip": SKIP, "dgrad": DGRAD, "up4": UP4}
ALL_ROWS = [c for t in TABLES.values() for c in t]


# ---------------------------------------------------------------------------------------------------------------- operands
class Launch:
    """what one launch reads.  x0, x1: fp32 tensors or int16 planes [planes, N, h, w, C]; v0, v1: the float64 values they represent;
    sx, sx1: tensor scales of fp16 planes (sx1 None: joint).  w: the pack; col: its scales per GEMM column (acc_scale_col);
    wl: the LAYER's weight [cout, cin, k, k] as the pack represents it (float64); wg: the planes of the GEMM's weight
    [planes][Cout, Cin, k, k] (float32, unscaled; the input gradient: transposed and flipped).  bias, ep_scale, ep_shift
    [groups, Cout], in_scale [N, h, w], out_scale [N, H, W], prev: the destinations' pre-fill under accumulate, amax0: the preset of
    out_absmax, ys_scale, mask: skip_mask."""
    x1 = v1 = sx = sx1 = col = w9 = bias = ep_scale = ep_shift = in_scale = out_scale = prev = ys_scale = mask = None
    amax0 = 0.0


def _pack(c, wl3):
    """wl3 [cout, cin, taps] fp32 of the layer -> (pack, col, wl float64 [cout, cin, k, k], wg)"""
    k = 3 if wl3.shape[2] == 9 else 2 if wl3.shape[2] == 4 else 1
    cout, cin, taps = wl3.shape
    lay = OC.lay_wd if c.dgrad else OC.lay_wp
    if not c.planes:
        wl = wl3.double().reshape(cout, cin, k, k)
        return lay(wl3[None], 4)[0].contiguous(), None, wl, [wl3.reshape(cout, cin, k, k)]
    col = sc = None
    if c.planes <= 2:
        col = torch.stack([OC.ref_pow2(wl3[:, i].abs().max()) for i in range(cin)] if c.dgrad else [OC.ref_pow2(r.abs().max()) for r in wl3])
        sc = col[None, :, None] if c.dgrad else col[:, None, None]
    P = split_planes(wl3, c.planes, sc)
    fl = P.view(torch.bfloat16 if c.planes == 3 else torch.float16).float()
    wl = (fl.double().sum(0) * (1.0 if sc is None else sc.double())).reshape(cout, cin, k, k)
    return lay(P, 32), col, wl, [f.reshape(cout, cin, k, k) for f in fl]


def _gemm_weight(c, w4):
    """[cout, cin, k, k] of the layer -> the GEMM's [Cout, Cin, k, k]"""
    return w4.transpose(0, 1).flip(2, 3) if c.dgrad else w4


def _planes_of(c, x, scale):
    return split_planes(x, c.planes, scale if c.planes <= 2 else None)


def make_launch(c, x0, x1, wl3, **kw):
    L = Launch()
    L.__dict__.update(kw)
    if c.fam == "up4":
        # the collapse in fp32 as rpnet_upconv_collapse_weights forms it (operand_cases.SimBackend, held to the device bit for bit by
        # tests/test_gpu_operands.py), then the ordinary four-tap pack.  wl: what THAT pack represents [4 cout, cin, 2, 2]; wg: its
        # planes times their power-of-two scales (exact), as the layer's own [4 cout, cin, 2, 2] in both modes
        L.w9 = wl3
        wc = OC.SimBackend().collapse(wl3.reshape(wl3.shape[0], wl3.shape[1], 3, 3))
        L.w, L.col, L.wl, wg = _pack(c, wc.reshape(wc.shape[0], wc.shape[1], 4))
        sc = L.col[None, :, None, None] if c.dgrad else L.col[:, None, None, None]
        L.wg = [g * sc for g in wg]
    else:
        L.w, L.col, L.wl, wg = _pack(c, wl3)
        L.wg = [_gemm_weight(c, g) for g in wg]
    if not c.planes:
        L.x0, L.x1, L.v0, L.v1 = x0, x1, x0.double(), None if x1 is None else x1.double()
        return L
    if c.planes <= 2:
        own = c.sx1 == "own"
        L.sx = pow2_scale(x0.abs().max() if own or x1 is None else max(x0.abs().max(), x1.abs().max()))
        L.sx1 = pow2_scale(x1.abs().max()) if own else None
    L.x0 = _planes_of(c, x0, L.sx)
    L.v0 = plane_values(L.x0, L.sx)
    if x1 is not None:
        L.x1 = _planes_of(c, x1, L.sx1 or L.sx)
        L.v1 = plane_values(L.x1, L.sx1 or L.sx)
    return L


def _seed(c, key):
    return case_seed(c.N, c.H, c.W, c.C0, c.C1, c.Co0, c.Co1, c.taps, c.dil, c.ups, c.planes, c.dgrad, key)


def layer_weight(c, seed):
    """[cout, cin, taps] of the LAYER: the forward reads C0 + C1 input channels, the input gradient C0 OUTPUT channels"""
    cout, cin = (c.Cin, c.Cout) if c.dgrad else (c.Cout, c.Cin)
    taps = 9 if c.fam == "up4" else c.taps
    return rnd(seed, cout, cin, taps) * (1.0 / math.sqrt(taps * cin)) * (2.0 ** (torch.arange(cout) % 4).float())[:, None, None]


def skip_mask(c):
    """[N, H, W] in [0, 1] whose factor (mode 1: mask, 2: 1 - mask) is zero on tile 1 of image 0 (`t`), or on that tile and its
    one-pixel halo (`a`), and positive elsewhere"""
    mode, kind = int(c.skip[4]), c.skip[6]
    th, tw = patch_shape(c)
    f = 0.25 + 0.5 * torch.rand(c.N, c.H, c.W, generator=torch.Generator().manual_seed(7))
    y0, x0 = 0, tw                                  # tile 1: the second patch of the first patch row
    h = 1 if kind == "a" else 0
    f[0, max(y0 - h, 0):y0 + th + h, max(x0 - h, 0):x0 + tw + h] = 0.0
    return f if mode == 1 else 1.0 - f


def skip_flags(c, mask):
    """what mask_tile_flags_kernel must leave in skip_ws: 0 = the tile is skipped"""
    mode, halo = int(c.skip[4]), int(c.skip[5])
    th, tw = patch_shape(c)
    f = (mask if mode == 1 else 1.0 - mask) != 0
    fp = F.pad(f, (halo, halo, halo, halo))
    out = []
    for n in range(c.N):
        for ty in range(c.H // th):
            for tx in range(c.W // tw):
                out.append(int(fp[n, ty * th:ty * th + th + 2 * halo, tx * tw:tx * tw + tw + 2 * halo].any()))
    return torch.tensor(out, dtype=torch.uint8)


def random_launch(c, key=0, x0=None):
    seed = _seed(c, key)
    g = torch.Generator().manual_seed(seed)
    hs, ws = c.src_hw
    H, W = c.H, c.W
    x0 = rnd(seed, c.N, hs, ws, c.C0) if x0 is None else x0
    x1 = 3.0 * rnd(seed + 1, c.N, hs, ws, c.C1) if c.C1 else None
    if c.sx1 == "own":       # the second source's scale exactly 2^5 times the first's
        x1 = x1 * (32.0 * x0.abs().max() / x1.abs().max())
    kw = {}
    if c.has("bias"):
        kw["bias"] = 0.5 * rnd(seed + 2, c.Cout)
    if c.mode:
        kw["in_scale"] = torch.rand(c.N, hs, ws, generator=g)
    if c.has("aff"):
        kw["ep_scale"], kw["ep_shift"] = 1.0 + 0.5 * rnd(seed + 3, c.groups, c.Cout), 0.3 * rnd(seed + 4, c.groups, c.Cout)
    if c.os_mode:
        kw["out_scale"] = torch.rand(c.N, H, W, generator=g)
    if c.skip:
        kw["mask"] = skip_mask(c)
        if c.skip[5] == "1":          # the factor multiplies the INPUT: the planes hold x * f(mask)
            m = kw["mask"] if c.skip[4] == "1" else 1.0 - kw["mask"]
            x0 = x0 * m[..., None]
        else:
            kw["out_scale"] = kw["mask"]
    if c.has("acc"):
        kw["prev"] = [rnd(seed + 5 + i, c.N, H, W, co) for i, co in enumerate((c.Co0, c.Co1)) if co]
    if c.has("amax"):
        kw["amax0"] = 0.0
    L = make_launch(c, x0, x1, layer_weight(c, seed + 9), **kw)
    assert c.sx1 != "own" or L.sx1 == 32.0 * L.sx
    return L


def _dests(c, y):
    return [y[..., :c.Co0].contiguous(), y[..., c.Co0:].contiguous()] if c.Co1 else [y]


def reference(c, L, dtype=F64):
    """([the destinations], acc + bias) of the launch (and of rpnet_upsample2_bwd behind it) on the represented values"""
    prev = None if L.prev is None else torch.cat(L.prev, -1)
    if c.fam == "up4":
        if c.up4 == 2:
            return [R.upconv_collapsed_dgrad(L.v0, L.wl, dtype=dtype)], None
        y = R.upconv_collapsed(L.v0, L.wl, L.bias, dtype=dtype)
        return [y], y
    if c.dgrad:
        ys = R.conv_dgrad(L.v0, L.wl, 9 if c.fam == "up4" else c.taps, c.dil, (c.Co0, c.Co1), L.out_scale, c.os_mode, prev,
                          int(bool(c.up_bwd or c.up4)), dtype=dtype)
        return ys, None
    y, pre = R.conv_fwd(L.v0, L.v1, L.wl, L.bias, 9 if c.fam == "up4" else c.taps, c.dil, int(bool(c.ups or c.up4)), L.in_scale, c.mode,
                        L.ep_scale, L.ep_shift, int(c.has("relu")), c.groups, L.out_scale, c.os_mode, prev, dtype=dtype)
    return _dests(c, y), pre


def dropped_term(c, L):
    """the absolute allowance per output element for the products the plane kernels leave out (module docstring), float64, as a
    list per destination; None: nothing is dropped"""
    if c.planes not in (2, 3):
        return None
    if c.fam == "up4":           # (two fp16 planes; the scale of a weight is that of its GEMM column: row of wc forward, cin backward)
        u = split_unit_roundoff(1)
        wa = L.wl.abs() + (L.col[None, :, None, None] if c.dgrad else L.col[:, None, None, None]).double() * 2.0 ** -13
        a0 = L.v0.abs() + L.sx * 2.0 ** -13
        return [u * u * (1 + u) ** 2 * (R.upconv_collapsed_dgrad(a0, wa) if c.up4 == 2 else R.upconv_collapsed(a0, wa))]
    wg = _gemm_weight(c, L.wl).abs()
    if c.planes == 2:
        u = split_unit_roundoff(1)
        k = u * u * (1 + u) ** 2
        fl = lambda v, s: None if v is None else v.abs() + s * 2.0 ** -13         # noqa: E731
        a0, a1, wg = fl(L.v0, L.sx), fl(L.v1, L.sx1 or L.sx), wg + L.col.double()[:, None, None, None] * 2.0 ** -13
    else:
        k = split_unit_roundoff(3) * (2 + U_BF16) * (1 + U_BF16) ** 2
        a0, a1 = L.v0.abs(), None if L.v1 is None else L.v1.abs()
    e, _ = R.conv_fwd(a0, a1, wg, None, c.taps, c.dil, c.ups)
    e = e * k
    if L.ep_scale is not None:
        e = e * R._per_image(L.ep_scale.double().abs(), c.N)
    if c.os_mode:
        e = e * (L.out_scale if c.os_mode == 1 else 1 - L.out_scale).double().abs()[..., None]
    if c.up_bwd:
        e = R.upsample2_bwd(e)
    return _dests(c, e)


# ----------------------------------------------------------------------------------------------------------------- records
class Rec(CC.Rec):
    raw = None           # the error before the allowance for the dropped products is taken off (None: the check has no allowance)

    def line(self):
        return (f"PARITY conv {self.family} {self.what} err={self.err:.3e} yard={self.yard:.3e} ratio={self.ratio:.2f} "
                f"of_bound={self.multiple:.3f}" + ("" if self.raw is None else f" raw={self.raw:.3e}"))


def _mine(r, raw=None):
    r.__class__ = Rec
    r.raw = raw
    return r


def exact(c, what, got, want):
    return _mine(CC.exact(c.id, what, got, want))


def bits_equal(c, what, got, want):
    """bit for bit (NaN equals the same NaN)"""
    v = torch.int16 if got.dtype in (torch.int16, torch.float16, torch.bfloat16) else torch.int64 if got.dtype == F64 else torch.int32
    return _mine(CC.exact(c.id, what, got.contiguous().view(v), want.contiguous().view(v)))


def whole(c, what, got, r64, r32, extra=None):
    raw = None if extra is None or not torch.isfinite(got).all() else float((got.double() - r64).abs().max() / (r64.abs().max() + 1e-12))
    return _mine(CC.measure(c.id, what + " whole", got, r64, r32, extra=extra), raw)


def close(c, what, got, want, tol):
    """rel_err(got, want) <= tol"""
    err = float((got.double() - want.double()).abs().max() / (want.double().abs().max() + 1e-300)) if torch.isfinite(got).all() else math.inf
    return Rec(c.id, what, err, 0.0, tol)


def per_block(c, what, got, r64, r32, extra=None, group="block"):
    """the bound per block of 32 consecutive pixels x 64 channels of an output [..., C] (group = "channel": per output channel over
    all pixels), relative to the block's own reference maximum: the record of the worst block.  A block whose reference is all
    zero must be exactly zero."""
    C = r64.shape[-1]
    if not torch.isfinite(got).all():
        return Rec(c.id, f"{what} per {group}", math.inf, 0.0, FLOOR)
    g, d = got.reshape(-1, C), (got.double() - r64).abs().reshape(-1, C)
    d_raw = d
    if extra is not None:
        d = (d - extra.reshape(-1, C)).clamp_min(0)
    y, r = (r32.double() - r64).abs().reshape(-1, C), r64.abs().reshape(-1, C)
    M = d.shape[0]
    pr, pc = (M, 1) if group == "channel" else (32, 64)
    pad = (-M) % pr

    def blocks(t):
        return F.pad(t, (0, 0, 0, pad)).reshape((M + pad) // pr, pr, C // pc, pc).amax((1, 3))

    ref, err, yard, nz = blocks(r), blocks(d), blocks(y), blocks((g != 0).double())
    dead = ref == 0
    if bool((dead & (nz > 0)).any()):
        i = torch.nonzero(dead & (nz > 0))[0].tolist()
        return Rec(c.id, f"{what} per {group}[{i}]: values where the reference is all zero", float((dead & (nz > 0)).sum()), 0.0, 0.0, exact=True)
    ref = torch.where(dead, torch.ones_like(ref), ref)
    e, yd = err / ref, yard / ref
    mult = torch.where(dead, torch.zeros_like(e), e / (FACTOR * yd + FLOOR))
    i = int(mult.argmax())
    bi, bj = i // mult.shape[1], i % mult.shape[1]
    rec = Rec(c.id, f"{what} per {group}[{bi},{bj}]", e[bi, bj], yd[bi, bj], FACTOR * float(yd[bi, bj]) + FLOOR)
    if extra is not None:           # of the block whose raw error is the largest multiple of its own bound
        rec.raw = float((torch.where(dead, torch.zeros_like(e), blocks(d_raw) / ref)).max())
    return rec


hold = CC.hold


# ------------------------------------------------------------------------------------------------------------------ checks
class Out:
    """ys: the destinations [N, H', W', Co] (behind rpnet_upsample2_bwd where the row has one); stats [groups, Cout, 2] float64,
    summed over the partial rows; amax [1]; ysplit int16 [planes, M, Cout]; flags: skip_ws; guard_ok: every guard word behind
    every output and workspace came back; ws_clean: the split-K workspace still holds its fill (the run that must not use it)"""

    def __init__(self, ys, stats=None, amax=None, ysplit=None, flags=None, guard_ok=True, ws_clean=None):
        self.ys, self.stats, self.amax, self.ysplit, self.flags, self.guard_ok, self.ws_clean = ys, stats, amax, ysplit, flags, guard_ok, ws_clean


def _run(be, c, L, **kw):
    out = be.run(c, L, **kw)
    assert out.guard_ok, f"{c.id}: the launch wrote behind an output or a workspace"
    return out


def _bound_records(c, what, ys, r64, r32, x, group="block"):
    recs = []
    for i, y in enumerate(ys):
        tag = f"{what} y{i}"
        recs.append(per_block(c, tag, y, r64[i], r32[i], None if x is None else x[i], group))
        if group == "block":
            recs.append(whole(c, tag, y, r64[i], r32[i], None if x is None else x[i]))
    return recs


def feature_records(c, L, out, own_pre=None):
    """the exact checks of the epilogue features on the launch's OWN output"""
    recs = []
    full = torch.cat(out.ys, -1)
    if c.has("amax"):
        recs.append(bits_equal(c, "out_absmax", out.amax.reshape(1), torch.maximum(full.abs().max(), torch.tensor(float(L.amax0))).reshape(1)))
    if c.ys_planes:
        want = split_planes(full.reshape(-1, c.Cout), c.ys_planes, L.ys_scale)
        recs.append(bits_equal(c, f"y_split, {c.ys_planes} planes", out.ysplit, want))
    if c.has("stats"):
        pre = full if own_pre is None else own_pre
        yg = pre.double().reshape(c.groups, -1, c.Cout)
        recs += [close(c, "stats_partial, sums", out.stats[..., 0], yg.sum(1), 1e-9), close(c, "stats_partial, sums of squares", out.stats[..., 1], (yg * yg).sum(1), 1e-9)]
    if c.skip:
        recs.append(exact(c, "skip_ws flags", out.flags, skip_flags(c, L.mask)))
    return recs


def plain_output(c):
    """the row without what stands between acc + bias and the output"""
    return c.but(ep=" ".join(f for f in c.feats if f in ("bias", "stats")))


def prepare(c, L, r64=None):
    """fields that depend on the reference: a y_split_scale four times the output's maximum ("predicted")"""
    if c.ys_planes in (1, 2) and L.ys_scale is None:
        r64 = reference(c, L)[0] if r64 is None else r64
        L.ys_scale = pow2_scale(4.0 * max(float(y.abs().max()) for y in r64))
    return L


def check_bound(be, c):
    """random operands: the bound per block and over the tensor, the exact checks of the row's features; a second identical
    launch is bit-identical"""
    L = random_launch(c)
    (r64, _), (r32, _), x = reference(c, L), reference(c, L, F32), dropped_term(c, L)
    prepare(c, L, r64)
    out = _run(be, c, L)
    recs = _bound_records(c, "y", out.ys, r64, r32, x)
    own_pre = None
    if c.has("stats") and plain_output(c).ep != c.ep:           # acc + bias of the SAME accumulators: the launch without the rest
        own_pre = torch.cat(_run(be, plain_output(c), random_launch(plain_output(c))).ys, -1)
    recs += feature_records(c, L, out, own_pre)
    again = _run(be, c, L)
    recs += [bits_equal(c, f"second identical launch y{i}", a, b) for i, (a, b) in enumerate(zip(again.ys, out.ys))]
    if c.has("amax"):           # a larger preset stays
        big = float(torch.cat(out.ys, -1).abs().max()) * 4.0
        L.amax0 = big
        recs.append(bits_equal(c, "out_absmax under a larger preset", _run(be, c, L).amax.reshape(1), torch.tensor([big])))
        L.amax0 = 0.0
    return recs


def check_skip(be, c):
    """the launch with the tile skip armed against the same launch without it: equal in every value (==: a skipped tile writes +0
    where the computed one may hold -0), and both inside the bound"""
    L = random_launch(c)
    (r64, _), (r32, _), x = reference(c, L), reference(c, L, F32), dropped_term(c, L)
    armed, plain = _run(be, c, L), _run(be, c, L, arm_skip=False)
    want = skip_flags(c, L.mask)
    assert int((want == 0).sum()) == (1 if c.skip[5] == "0" or c.skip[6] == "a" else 0), "the mask does not do what the row says"
    return (_bound_records(c, "y", armed.ys, r64, r32, x) + feature_records(c, L, armed)
            + [exact(c, "skipped == computed", armed.ys[0], plain.ys[0])])


def impulse_positions(c):
    """source pixels (n, y, x) at SOURCE resolution: the corners, an edge centre, both sides of every patch seam, the last row of
    image 0 and the first of image 1"""
    hs, ws = c.src_hw
    pos = [(0, 0, 0), (0, 0, ws // 2), (0, hs - 1, ws - 1), (0, hs // 2, 0)]
    if patch_rows(c) and c.fam != "up4":
        th, tw = patch_shape(c)
        th, tw = th >> c.ups, tw >> c.ups
        if tw < ws:
            pos += [(0, min(1, hs - 1), tw - 1), (0, min(1, hs - 1), tw)]
        if th < hs:
            pos += [(0, th - 1, ws // 2), (0, th, ws // 2)]
    if c.N > 1:
        pos += [(0, hs - 1, ws // 3), (1, 0, ws // 3), (c.N - 1, hs - 1, 0)]
    return list(dict.fromkeys(pos))


def check_impulses(be, c):
    """one non-zero pixel per position, each in a channel of its own, a weight of 2^(tap - 4) with a sign per channel pair: every
    output value is a short sum of products of powers of two, exact in fp32 and in every plane arithmetic"""
    hs, ws = c.src_hw
    xs = torch.zeros(c.N, hs, ws, c.Cin)
    for j, (n, y, x) in enumerate(impulse_positions(c)):
        xs[n, y, x, (j * 37) % c.Cin] = 2.0 ** (j % 4 - 2)
    cout, cin = (c.Cin, c.Cout) if c.dgrad else (c.Cout, c.Cin)
    sign = 1.0 - 2.0 * ((torch.arange(cout)[:, None] + torch.arange(cin)[None, :]) % 2).float()
    wl3 = sign[..., None] * (2.0 ** (torch.arange(c.taps).float() - 4))[None, None, :]
    L = make_launch(c, xs[..., :c.C0].contiguous(), xs[..., c.C0:].contiguous() if c.C1 else None, wl3,
                    in_scale=torch.ones(c.N, hs, ws) if c.mode == 1 else torch.zeros(c.N, hs, ws) if c.mode == 2 else None)
    want, _ = reference(c, L)
    assert all(bool((w.float().double() == w).all()) for w in want) and bool((want[0] != 0).any())
    out = _run(be, c, L)
    return [exact(c, f"impulses y{i}", y.double(), w) for i, (y, w) in enumerate(zip(out.ys, want))]


def check_splitk(be, c):
    """with exactly the workspace rpnet_conv_splitk_workspace_bytes asks for: inside the bound of float64 and of the one-block-per-
    tile launch; one byte less: one block per tile, bit for bit, the workspace untouched"""
    L = random_launch(c)
    (r64, _), (r32, _), x = reference(c, L), reference(c, L, F32), dropped_term(c, L)
    prepare(c, L, r64)
    one = _run(be, c.but(splitk=0), L)
    sk = _run(be, c, L)
    short = _run(be, c, L, ws_short=True)
    again = _run(be, c, L)
    assert short.ws_clean is True, f"{c.id}: a workspace one byte short was written"
    assert sk.ws_clean is False, f"{c.id}: the exact workspace still holds its fill: the launch did not split K"
    recs = _bound_records(c, "split K y", sk.ys, r64, r32, x) + _bound_records(c, "one block per tile y", one.ys, r64, r32, x)
    recs += feature_records(c, L, sk)
    # (the two launches drop the same products: no allowance; the yard is the float32 reference's distance from float64)
    recs.append(per_block(c, "split K against one block per tile", sk.ys[0], one.ys[0].double(), one.ys[0].double() + (r32[0].double() - r64[0])))
    recs += [bits_equal(c, "a workspace one byte short: one block per tile", short.ys[0], one.ys[0]), bits_equal(c, "second identical launch", again.ys[0], sk.ys[0])]
    return recs


def check_cre_pair(be, c):
    """out_scale_mode 1 into a NaN-filled tensor, then out_scale_mode 2 with accumulate into the same one: dx = g1 s + g2 (1 - s)"""
    a, b = c.but(ep="os1"), c.but(ep="os2 acc")
    La = random_launch(a)
    Lb = random_launch(b, key=1)
    Lb.out_scale = La.out_scale
    first = _run(be, a, La)
    Lb.prev = first.ys
    second = _run(be, b, Lb)
    r64a, r32a = reference(a, La)[0], reference(a, La, F32)[0]
    Lr = Launch()
    Lr.__dict__.update(Lb.__dict__)
    Lr.prev = r64a
    r64 = reference(b, Lr)[0]
    Lr.prev = r32a
    r32 = reference(b, Lr, F32)[0]
    xa, xb = dropped_term(a, La), dropped_term(b, Lb)
    x = None if xa is None else [p + q for p, q in zip(xa, xb)]
    return _bound_records(a, "first branch dx", first.ys, r64a, r32a, xa) + _bound_records(b, "both branches dx", second.ys, r64, r32, x)


def nine_tap_form(c):
    """the same layer through rpnet_conv_fwd: with d->upsample (mode 1), with rpnet_upsample2_bwd behind it (mode 2)"""
    n = Case("planes", (c.N, c.H, c.W), c.C0, c.Co0, "", planes=c.planes, ups=int(c.up4 == 1), dgrad=c.dgrad, up_bwd=int(c.up4 == 2),
             ep=" ".join(f for f in c.feats if f == "bias"))
    n.kernel = route(n)
    return n


def check_up4(be, c):
    """rpnet_conv_up4 against float64 on what its four-tap pack represents, and the nine-tap form of the same layer on the same source
    planes against float64 on what the nine-tap pack represents, inside the same bound (module docstring)"""
    L = random_launch(c)
    (r64, _), (r32, _), x = reference(c, L), reference(c, L, F32), dropped_term(c, L)
    out = _run(be, c, L)
    recs = _bound_records(c, "y", out.ys, r64, r32, x) + feature_records(c, L, out)
    again = _run(be, c, L)
    recs.append(bits_equal(c, "second identical launch", again.ys[0], out.ys[0]))
    n = nine_tap_form(c)
    Ln = make_launch(n, L.v0.float(), None, L.w9, bias=L.bias)
    Ln.x0, Ln.v0, Ln.sx = L.x0, L.v0, L.sx           # the very same planes
    (n64, _), (n32, _) = reference(n, Ln), reference(n, Ln, F32)
    return recs + _bound_records(n, "nine-tap form y", _run(be, n, Ln).ys, n64, n32, dropped_term(n, Ln))


def check_dynamic_range(be, c):
    """source channel j of magnitude 2^-(20 j / (C - 1)) under ONE tensor scale, the weight of output channel o reading channel
    band o % 4 only, judged per output channel against the ORIGINAL fp32 source (the split of the source is what is under
    test).  Two fp16 planes keep a value v of a tensor of maximum m to u^2 (1 + u) |v| while its residual is a normal fp16 number, one
    plane to u |v| while v / s is; below that the spacing is 2^-24 on values the scale s <= 2^-14 m has brought below 2^15: an
    absolute 2^-25 s <= 2^-39 m.  Per element of the output: sum |w| (U |x| + 2^-39 m), U = u^2 (1 + u) or u, beside the dropped l.l
    product of two planes."""
    seed = _seed(c, 55)
    e = torch.round(torch.arange(c.C0) * (20.0 / (c.C0 - 1)))
    x = rnd(seed, c.N, c.H, c.W, c.C0) * 2.0 ** -e
    wl3 = layer_weight(c, seed + 9)
    band = (torch.arange(c.C0) * 4 // c.C0)[None, :] == (torch.arange(c.Cout) % 4)[:, None]
    wl3 = wl3 * band[..., None] * 2.0 ** (5.0 * (torch.arange(c.Cout) % 4).float())[:, None, None]
    L = make_launch(c, x, None, wl3)
    full = Launch()
    full.__dict__.update(L.__dict__)
    full.v0 = x.double()
    (r64, _), (r32, _) = reference(c, full), reference(c, full, F32)
    m = float(x.abs().max())
    wabs, u = _gemm_weight(c, L.wl).abs(), CC.U_F16
    floor = R.conv_fwd((u if c.planes == 1 else u * u * (1 + u)) * full.v0.abs() + 2.0 ** -39 * m, None, wabs)[0]
    xd = dropped_term(c, L)
    x_all = floor if xd is None else floor + xd[0]
    return _bound_records(c, "dynamic y", _run(be, c, L).ys, r64, r32, [x_all], group="channel")


def checks_of(c):
    fns = [check_skip if c.skip else check_splitk if c.splitk else check_up4 if c.fam == "up4" else check_bound]
    if not c.ep and not c.splitk and c.fam != "up4":
        fns.append(check_impulses)
    return fns


def check_row(be, c):
    assert route(c) == c.kernel, f"{c.id}: the launcher takes {route(c)}, the table says {c.kernel}"
    return [r for fn in checks_of(c) for r in fn(be, c)]


# --------------------------------------------------------------------------------------------------------------- refusals
# (label, base case, changes to the call, status, words of the message): every RPNET_REQUIRE line of the two entry points and each
# half of its condition, refused on the host before any launch; the words pin a row to ITS line.  Changes: a Case field;
# null=<pointer>; set=<descriptor fields> (a pointer field gets a valid buffer); huge=(N, H, W) (the pointers stay small buffers:
# nothing is read); no_scales=1; up4=<the mode argument of rpnet_conv_up4>.
_BF, _BS, _BU = _f((2, 8, 8), 32, 64, ""), _p(2, 1, (2, 8, 8), 32, 64), _u(2, 1, (1, 32, 32), 32, 64)
_NULL, _TAPS, _CIN, _COUT = "null pointer", "taps must be 9 or 1", "multiple of 32 per source", "multiple of 64 per destination"
_STAT, _YS, _FIT, _PLAIN = "statistic groups do not split into whole tiles", "y_split needs a single destination", "do not fit", "plain epilogue only"
REFUSALS = [
    ("null x0", _BF, dict(null="x0"), ARG, _NULL), ("null w", _BF, dict(null="w"), ARG, _NULL), ("null y0", _BF, dict(null="y0"), ARG, _NULL),
    ("taps = 4", _BF, dict(taps=4), ARG, _TAPS), ("C0 = 48", _BF, dict(C0=48), SHAPE, _CIN), ("C0 + C1 = 32 + 16", _BF, dict(C1=16), SHAPE, _CIN),
    ("a second source without its pointer", _BF, dict(C1=32, null="x1"), SHAPE, _CIN), ("Cout = 96", _BF, dict(Co0=96), SHAPE, _COUT),
    ("Co0 = 32 of two destinations", _BF, dict(Co0=32, Co1=96), SHAPE, _COUT),
    ("a second destination without its pointer", _BF, dict(Co1=64, null="y1"), SHAPE, _COUT),
    ("statistic groups that do not split into whole tiles", _BF, dict(N=3, groups=1, set=dict(stats_partial=1)), SHAPE, _STAT),
    ("statistics with N % groups != 0", _BF, dict(N=3, groups=2, set=dict(stats_partial=1)), SHAPE, _STAT),
    ("odd height with upsample", _BF, dict(H=7, ups=1), SHAPE, "odd size with upsample"), ("odd width with upsample", _BF, dict(W=7, ups=1), SHAPE, "odd size with upsample"),
    ("y_split with two destinations", _BF, dict(Co1=64, set=dict(y_split=1, split_out_planes=3)), ARG, _YS),
    ("y_split with four planes", _BF, dict(set=dict(y_split=1, split_out_planes=4)), ARG, _YS),
    ("y_split with no planes", _BF, dict(set=dict(y_split=1, split_out_planes=0)), ARG, _YS),
    ("fp16 y_split, two planes, without its scale", _BF, dict(set=dict(y_split=1, split_out_planes=2)), ARG, "need y_split_scale"),
    ("fp16 y_split, one plane, without its scale", _BF, dict(set=dict(y_split=1, split_out_planes=1)), ARG, "need y_split_scale"),
    ("y_enc", _BF, dict(set=dict(y_enc=1)), ARG, "y_enc / y_enc_stride are reserved"), ("y_enc_stride", _BF, dict(set=dict(y_enc_stride=4)), ARG, "y_enc / y_enc_stride are reserved"),
    ("bnb_y", _BF, dict(set=dict(bnb_y=1)), ARG, "bnb_* fields are reserved"), ("bnb_stats", _BF, dict(set=dict(bnb_stats=1)), ARG, "bnb_* fields are reserved"),
    ("bnb_partial", _BF, dict(set=dict(bnb_partial=1)), ARG, "bnb_* fields are reserved"), ("bnb_pmax", _BF, dict(set=dict(bnb_pmax=1)), ARG, "bnb_* fields are reserved"),
    ("2^31 pixels", _BF, dict(huge=(65536, 256, 128)), SHAPE, "too many pixels"), ("a source of 2 GiB", _BF, dict(huge=(256, 256, 256)), SHAPE, "2 GiB buffer-descriptor range"),
    ("a second source of 2 GiB", _BF, dict(C1=64, huge=(128, 256, 256)), SHAPE, "2 GiB buffer-descriptor range"),
    ("a weight pack of 2 GiB", _BF, dict(C0=8192, Co0=8192), SHAPE, "2 GiB buffer-descriptor range"),
    ("four planes", _BS, dict(planes=4), ARG, "1 to 3 planes and no in_scale"), ("planes with in_scale", _BS, dict(mode=1), ARG, "1 to 3 planes and no in_scale"),
    ("fp16 planes without scales", _BS, dict(no_scales=1), ARG, "acc_scale_col and acc_scale_x are required"),
    ("one fp16 plane without scales", _BS, dict(planes=1, no_scales=1), ARG, "acc_scale_col and acc_scale_x are required"),
    ("fp16 planes without acc_scale_x", _BS, dict(null="acc_scale_x"), ARG, "acc_scale_col and acc_scale_x are required"),
    ("null x0", _BU, dict(null="x0"), ARG, _NULL + " / mode"), ("null w", _BU, dict(null="w"), ARG, _NULL + " / mode"), ("null y0", _BU, dict(null="y0"), ARG, _NULL + " / mode"),
    ("mode 0", _BU, dict(up4=0), ARG, _NULL + " / mode"), ("mode 3", _BU, dict(up4=3), ARG, _NULL + " / mode"),
    ("odd height", _BU, dict(H=31), SHAPE, _FIT), ("odd width", _BU, dict(W=63), SHAPE, _FIT), ("three planes", _BU, dict(planes=3), SHAPE, _FIT),
    ("C1 set", _BU, dict(C1=32, null="x1"), SHAPE, _FIT), ("x1 set", _BU, dict(set=dict(x1=1)), SHAPE, _FIT),
    ("Co1 set", _BU, dict(Co1=64, null="y1"), SHAPE, _FIT), ("y1 set", _BU, dict(set=dict(y1=1)), SHAPE, _FIT),
    ("C0 = 48", _BU, dict(C0=48), SHAPE, _FIT), ("Co0 = 96", _BU, dict(Co0=96), SHAPE, _FIT), ("low resolution 8 x 8", _BU, dict(H=16, W=16), SHAPE, _FIT),
    ("fp16 planes without scales", _BU, dict(no_scales=1), ARG, "need acc_scale_col and acc_scale_x"),
    ("fp16 planes without acc_scale_x", _BU, dict(null="acc_scale_x"), ARG, "need acc_scale_col and acc_scale_x"),
    ("statistics in mode 2", _BU, dict(up4=2, set=dict(stats_partial=1)), ARG, "statistics belong to the forward launch"),
    ("statistics with N % groups != 0", _BU, dict(groups=2, set=dict(stats_partial=1)), SHAPE, _STAT),
    ("out_scale", _BU, dict(set=dict(out_scale=1, out_scale_mode=1)), ARG, _PLAIN), ("y_split", _BU, dict(set=dict(y_split=1, split_out_planes=2)), ARG, _PLAIN),
    ("splitk_ws", _BU, dict(set=dict(splitk_ws=1, splitk_ws_bytes=1 << 20)), ARG, _PLAIN), ("bnb_y", _BU, dict(set=dict(bnb_y=1)), ARG, _PLAIN),
    ("tile_skip", _BU, dict(set=dict(tile_skip=1)), ARG, _PLAIN), ("y_enc", _BU, dict(set=dict(y_enc=1)), ARG, _PLAIN),
]
REFUSAL_POINTERS = ("stats_partial", "y_split", "y_enc", "bnb_y", "bnb_stats", "bnb_partial", "bnb_pmax", "out_scale", "splitk_ws", "tile_skip", "x1", "y1")
REFUSAL_PREFIX = {"rpnet_conv_fwd": "conv_fwd:", "rpnet_conv_up4": "conv_up4:"}


# ----------------------------------------------------------------------------------------- the float32 stand-in for the library
DEFECTS = ["seam_column", "previous_image_top", "bias_after_affine", "one_minus_s", "no_accumulate", "group_of_first_row", "second_dest_offset",
           "drop_cross", "up_round", "no_dilation", "ignore_sx1", "amax_before_out_scale", "stats_without_bias", "ysplit_before_rowops",
           "splitk_part_missing"]


class SimBackend:
    """A float32 torch restatement of one launch on the planes themselves: the gather (up-sampling, dilation, zero border) as nine
    shifted slices, the plane products formed one by one as the kernels form them (the dropped ones dropped), one matrix product
    per tap, the split-K parts summed in sequence, then the epilogue of csrc/conv_epilogue.h in its order.  `defect`: one of
    DEFECTS."""

    def __init__(self, defect=None):
        assert defect is None or defect in DEFECTS
        self.defect = defect

    def _taps(self, c, x):
        """x [N, hs, ws, C] fp32 -> [taps][M, C]"""
        N, H, W = c.N, c.H, c.W
        d = 1 if self.defect == "no_dilation" else max(c.dil, 1)
        if c.ups or c.up4 == 1:
            iy, ix = torch.arange(H) >> 1, torch.arange(W) >> 1
            if self.defect == "up_round":
                ix = ((torch.arange(W) + 1) >> 1).clamp_max((W >> 1) - 1)
            x = x[:, iy][:, :, ix]
        if c.taps == 1 and c.fam != "up4":
            return [x.reshape(c.M, -1)]
        xp = F.pad(x, (0, 0, d, d, d, d))
        tw = patch_shape(c)[1] if patch_rows(c) and c.fam != "up4" else 0
        out = []
        for kh in range(3):
            for kw in range(3):
                a = xp[:, kh * d:kh * d + H, kw * d:kw * d + W].clone()
                if self.defect == "seam_column" and kw == 2 and tw and tw < W:           # the halo column right of a seam: one further
                    cols = torch.arange(tw - 1, W - 1, tw)
                    a[:, :, cols] = xp[:, kh * d:kh * d + H][:, :, (cols + 2 + d).clamp_max(W + 2 * d - 1)]
                if self.defect == "previous_image_top" and kh == 0 and N > 1:
                    a[1:, 0] = xp[:-1, d + H - 1, kw * d:kw * d + W]
                out.append(a.reshape(c.M, -1))
        return out

    def _prods(self, planes):
        """(source plane, weight plane) in the kernels' order, smallest first (split_bf16.h prod_a / prod_b)"""
        prods = {3: [(2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)], 2: [(1, 0), (0, 1), (0, 0)], 1: [(0, 0)], 0: [(0, 0)]}[planes]
        if self.defect == "drop_cross":
            prods = {3: prods[1:], 2: [(1, 0), (0, 0)]}.get(planes, prods)
        return prods

    def _up4_acc(self, c, L):
        """the collapsed up-conv [rows, Cout] in units of sx: the four-phase form on the pack's planes, product by product"""
        xs = [L.x0[p].view(torch.float16).float() for p in range(c.planes)]
        fn = R.upconv_collapsed_dgrad if c.up4 == 2 else R.upconv_collapsed
        acc = 0.0
        for (pa, pb) in self._prods(c.planes):
            acc = acc + fn(xs[pa], L.wg[pb], dtype=F32)
        return acc.reshape(-1, c.Cout)

    def _acc(self, c, L, lo, hi):
        """the accumulator [M, Cout] over the gathered channels lo .. hi, in units of sx * col"""
        prods = self._prods(c.planes)
        if c.planes:
            f = torch.bfloat16 if c.planes == 3 else torch.float16
            xs = [torch.cat([L.x0[p].view(f).float()] + ([L.x1[p].view(f).float()] if c.C1 else []), -1) for p in range(c.planes)]
        else:
            x = L.x0 if L.x1 is None else torch.cat([L.x0, L.x1], -1)
            if c.mode:
                s = L.in_scale.float()
                x = x * (s if c.mode == 1 else 1.0 - s)[..., None]
            xs = [x]
        if L.sx1 is not None and self.defect != "ignore_sx1":           # the accumulator in units of source 0
            xs = [torch.cat([x[..., :c.C0], x[..., c.C0:] * (float(L.sx1) / float(L.sx))], -1) for x in xs]
        A = [self._taps(c, x) for x in xs]
        acc = torch.zeros(c.M, c.Cout)
        nt = len(A[0])
        for t in range(nt):
            kh, kw = (t // 3, t % 3) if nt == 9 else (0, 0)
            for (pa, pb) in prods:
                acc = acc + A[pa][t][:, lo:hi] @ L.wg[pb][:, lo:hi, kh, kw].T
        return acc

    @staticmethod
    def _sum2x2(c, t):
        t = t.reshape(c.N, c.H // 2, 2, c.W // 2, 2, c.Cout)
        return (t[:, :, 0, :, 0] + t[:, :, 0, :, 1]) + (t[:, :, 1, :, 0] + t[:, :, 1, :, 1])

    def run(self, c, L, arm_skip=True, ws_short=False):
        parts = splitk_parts(c) if (c.splitk and not ws_short) else 1
        step = c.Cin // parts
        acc = torch.zeros(c.M, c.Cout)
        for p in range(parts):
            if self.defect == "splitk_part_missing" and parts > 1 and p == parts - 1:
                continue
            if c.fam != "up4":
                acc = acc + self._acc(c, L, p * step, (p + 1) * step)
        if c.fam == "up4":           # (mode 2: the low-resolution gradient itself; L.wg carries the pack's scales)
            acc = self._up4_acc(c, L)
        asv = torch.ones(c.Cout) if L.col is None else torch.full((c.Cout,), float(L.sx)) if c.fam == "up4" else L.col * float(L.sx)
        rows = acc.shape[0]
        bias = torch.zeros(c.Cout) if L.bias is None else L.bias
        scaled = acc * asv
        pre = scaled + bias
        stats = None
        if c.has("stats"):
            s = (scaled if self.defect == "stats_without_bias" else pre).double().reshape(c.groups, -1, c.Cout)
            stats = torch.stack([s.sum(1), (s * s).sum(1)], -1)
        v = pre
        if c.has("aff"):
            row = torch.arange(rows)
            if self.defect == "group_of_first_row" and not patch_rows(c):
                row = row // tile_rows(c) * tile_rows(c)
            g = row // ((c.N // c.groups) * c.H * c.W)
            v = (scaled * L.ep_scale[g] + L.ep_shift[g] + bias) if self.defect == "bias_after_affine" else pre * L.ep_scale[g] + L.ep_shift[g]
        if c.has("relu"):
            v = torch.relu(v)
        before = v
        if c.os_mode:
            s = L.out_scale.float().reshape(-1, 1)
            v = v * (s if (c.os_mode == 1) != (self.defect == "one_minus_s") else 1.0 - s)
        amax_src = before if self.defect == "amax_before_out_scale" else None
        if c.has("acc") and self.defect != "no_accumulate":
            v = v + torch.cat(L.prev, -1).reshape(rows, c.Cout)
        amax = None
        if c.has("amax"):
            amax = torch.maximum((v if amax_src is None else amax_src).abs().max(), torch.tensor(float(L.amax0))).reshape(1)
        ysplit = None
        if c.ys_planes:
            ysplit = split_planes(before if self.defect == "ysplit_before_rowops" else v, c.ys_planes, L.ys_scale)
        full = v.reshape(c.N, -1, c.W >> int(c.up4 == 2), c.Cout)
        if c.up_bwd:
            full = self._sum2x2(c, full)
        ys = _dests(c, full)
        if self.defect == "second_dest_offset" and c.Co1:
            ys[1] = full[..., :c.Co1].contiguous()
        flags = skip_flags(c, L.mask) if c.skip and arm_skip else None
        return Out(ys, stats, amax, ysplit, flags, True, (ws_short or parts == 1) if c.splitk else None)
