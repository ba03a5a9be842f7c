"""Cases and comparison functions shared by tests/test_host_wgrad_ref64.py and tests/test_gpu_wgrad_fp64.py: the convolution weight
gradient (rpnet_conv_wgrad: csrc/conv_wgrad.hip on fp32 operands, csrc/conv_wgrad_split.hip / conv_wgrad_split_dma.hip /
conv_wgrad_ring.hip on operand planes; rpnet_conv_wgrad_up4: csrc/conv_wgrad_up4.hip; rpnet_conv1_wgrad: csrc/conv_first.hip)
against tests/ref64.py conv_wgrad at every branch of the dispatch.  The layout is that of tests/corr_cases.py, whose definitions
(split_planes, plane_values, pow2_scale, case_seed, FACTOR, FLOOR, Rec, measure, exact, hold) are used, not restated.

A *backend* runs ONE launch described by a Case and its operands on CPU tensors: the HIP library (the GPU test) or SimBackend, a
float32 torch restatement with the same split-K plan, workspace and reduce, with or without a seeded defect (the host test).

Bound: rel_err(got, r64) <= FACTOR * yard + FLOOR, yard = rel_err(r32, r64), taken per (tap, 64 input x 64 output channel) block
of dW relative to that block's own reference maximum (per_block), and over the whole tensor as well.  Plane operands: the
reference is evaluated on the values the planes represent; the products the kernels leave out on purpose get dropped_term():
  two fp16 planes   x = h + l, |l| <= u (|x| + 2^-13) (1 + u), u = split_unit_roundoff(1): the sequence is l.h, h.l, h.h
                    (split_bf16.h prod_a / prod_b), l.l is dropped: <= u^2 (1 + u)^2 sum (|x| + 2^-13)(|dy| + 2^-13) in units of
                    the two scales (2^-13: an fp16 residual below 2^-14 is subnormal, spacing 2^-24 = u 2^-13);
  three bf16 planes x = h + m + l, |m| <= v |x| (1 + v), |l| <= v^2 |x| (1 + v), v = 2^-8: the six products are
                    l.h, h.l, m.m, m.h, h.m, h.h; dropped are m.l, l.m and l.l, the three smallest of the nine:
                    <= (2 v^3 + v^4)(1 + v)^2 sum |x||dy|, v^3 = split_unit_roundoff(3);
  one plane         drops nothing.
Exact checks (impulses, zero operands, bit-identical repeats, two-phase against one call, guard words) count mismatching
elements and allow none.  No check carries a measured factor."""
import math

import torch
import torch.nn.functional as F

from tests import corr_cases as CC
from tests import ref64 as R
from tests.corr_cases import ARG, FACTOR, FLOOR, SHAPE, U_BF16, WORKSPACE, case_seed, plane_values, pow2_scale, split_planes, split_unit_roundoff  # noqa: F401
from tests.helpers import rnd

F32, F64 = torch.float32, torch.float64
GUARD = 64                      # words behind the workspace that must come back as they went in
MAX1 = 128                      # kWgrad1MaxSplits (csrc/common.h)
CONV1_BLOCKS = 1024             # kConv1WgradBlocks (csrc/conv_first.hip)


# ------------------------------------------------------------------------------------------------------------------- plans
def _cdiv(a, b):
    return -(-a // b)


def _pow2(v):
    return v >= 1 and v & (v - 1) == 0


def plan9(M, Cin, Cout, target):
    """wgrad9_plan (csrc/conv_wgrad.hip): (ksplit, 32-pixel steps per split)"""
    tiles, steps = (Cin // 64) * (Cout // 64), _cdiv(M, 32)
    ks = 1 if tiles >= target else _cdiv(target, tiles)
    ks = min(ks, max(1, steps // 8))
    if ks >= 8:
        ks = ks // 8 * 8
    sps = _cdiv(steps, ks)
    k2 = _cdiv(steps, sps)
    return ((k2 + 7) // 8 * 8 if ks >= 8 else k2), sps


def plan_tap(M, Cin, Cout, taps):
    """wgrad_plan: (bm, bn, ksplit, steps per split) of the one-tap-per-block fp32 kernel"""
    bm, bn = (128 if Cin % 128 == 0 and taps > 1 else 64), (128 if Cout % 128 == 0 else 64)
    tiles, steps = max(1, (Cin // bm) * (Cout // bn) * taps), _cdiv(M, 32)
    ks = max(1, min(_cdiv(768, tiles), max(1, steps // 8)))
    if taps == 1:
        ks = min(ks, MAX1)
    sps = _cdiv(steps, ks)
    if taps == 9:
        sps += sps & 1
    return bm, bn, _cdiv(steps, sps), sps


def plan1_split(M, Cin, Cout):
    """wgrad1_split_plan (csrc/conv_wgrad_split.hip)"""
    tiles, steps = (Cin // 64) * (Cout // 64), _cdiv(M, 32)
    ks = min(max(1, min(_cdiv(512, tiles), max(1, steps // 8))), MAX1)
    sps = _cdiv(steps, ks)
    return _cdiv(steps, sps), sps


def plan_up4(Ml, Cin, Cout, pxs):
    """up4_wgrad_plan (csrc/conv_wgrad_up4.hip): steps of pxs low-resolution pixels"""
    tiles, steps = (Cin // 64) * (Cout // 64) * 4, _cdiv(Ml, pxs)
    ks = 1 if tiles >= 256 else _cdiv(256, tiles)
    ks = min(ks, max(1, steps // 8))
    if ks >= 8:
        ks = ks // 8 * 8
    sps = _cdiv(steps, ks)
    k2 = _cdiv(steps, sps)
    return ((k2 + 7) // 8 * 8 if ks >= 8 else k2), sps


# ------------------------------------------------------------------------------------------------------------------- cases
class Case:
    """one launch shape.  fam: fp32_9 | fp32_tap | planes9 | planes1 | up4 | conv1.  N, H, W: the OUTPUT's (dy's) size; C0 | C1 the
    gathered sources; map = (cin_w, off0, split, off1) (None: every gathered channel); sx1: "own" = source x1 on its own tensor
    scale, 2^5 times x0's.  kernel: the launch the row is meant to reach (route() restates the launcher's conditions)."""

    def __init__(self, fam, nhw, C0, cout, kernel, C1=0, taps=9, dil=1, ups=0, mode=0, planes=0, tune=0, map=None, sx1=None,
                 checks="zap"):
        self.fam, (self.N, self.H, self.W), self.C0, self.C1, self.cout, self.kernel = fam, nhw, C0, C1, cout, kernel
        self.taps, self.dil, self.ups, self.mode, self.planes, self.tune, self.sx1 = taps, dil, ups, mode, planes, tune, sx1
        self.map = map if map is not None else (C0 + C1, 0, C0 + C1, C0 + C1)
        self.checks = checks            # z: zeros, a: accumulate, p: impulses (two-phase wherever the entry point has it)

    M = property(lambda s: s.N * s.H * s.W)
    Cin = property(lambda s: s.C0 + s.C1)
    entry = property(lambda s: {"up4": "rpnet_conv_wgrad_up4", "conv1": "rpnet_conv1_wgrad"}.get(s.fam, "rpnet_conv_wgrad"))
    two_phase = property(lambda s: s.fam in ("planes9", "planes1", "up4"))

    def but(self, **kw):
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.__dict__.update(kw)
        return c

    def rows(self):
        """gathered row of every dW input channel"""
        cin_w, off0, split, off1 = self.map
        return torch.tensor([off0 + i if i < split else off1 + i - split for i in range(cin_w)])

    @property
    def id(self):
        m = "" if self.map[0] == self.Cin else f"-map{self.map[0]}"
        return (f"{self.fam}-{self.N}x{self.H}x{self.W}-{self.C0}" + (f"+{self.C1}" if self.C1 else "") + f"to{self.cout}" + m
                + (f"-p{self.planes}" if self.planes else "") + (f"-t{self.tune}" if self.tune else "") + (f"-d{self.dil}" if self.dil > 1 else "")
                + ("-1x1" if self.taps == 1 else "") + ("-up" if self.ups else "") + (f"-is{self.mode}" if self.mode else "")
                + (f"-sx1{self.sx1}" if self.sx1 else ""))


def route(c):
    """the kernel the launchers pick for a case: the conditions of rpnet_conv_wgrad (csrc/conv_wgrad.hip), conv_wgrad9_split_dma,
    conv_wgrad9_dma_one_plane_ok and conv_wgrad9_ring_ok, restated once; every table row is asserted against it"""
    if c.fam == "conv1":
        return "conv1_wgrad"
    if c.fam == "up4":
        return "up4<K64>" if c.planes == 1 else "up4"
    p2 = _pow2(c.W) and _pow2(c.H)
    if c.taps == 9 and c.dil <= 1:
        if not c.planes:
            return f"wgrad9<P2={int(p2)},IS={int(c.mode != 0)}>"
        _, sps = plan9(c.M, c.Cin, c.cout, 256)
        tv = c.tune & 255
        k64 = c.planes == 1 and not c.ups and c.W >= 64 and p2 and c.M % 64 == 0 and sps % 2 == 0
        dma = (c.planes == 2 or k64) and tv not in (4, 8)
        ring_ok = p2 and not c.ups and ((c.planes == 2 and c.W >= 32) or k64)
        if dma and tv != 16 and ring_ok:
            return "ring<K64>" if c.planes == 1 else "ring<shallow>" if tv == 17 else "ring"
        if dma:
            if c.planes == 1:
                return "dma<K64>"
            dp2 = _pow2(c.W) and c.W >= 8 and _pow2(c.H)
            return "dma<P2,fast>" if dp2 and c.W >= 32 and not c.ups else "dma<P2>" if dp2 else "dma<>"
        return f"staged<{c.planes},P2={int(p2)},{'4' if c.tune == 4 else '12'} waves>"
    if c.planes and c.taps == 1:
        return f"wgrad1_split<{c.planes}>"
    bm, bn, _, _ = plan_tap(c.M, c.Cin, c.cout, c.taps)
    return f"wgrad<{bm // 64},{bn // 64}>"


def workspace_bytes(c):
    """what the *_workspace_bytes query of the case's entry point must answer (the GPU test asserts the two agree)"""
    if c.fam == "conv1":
        return CONV1_BLOCKS * c.cout * 9 * 4
    if c.fam == "up4":
        Ml = c.N * (c.H // 2) * (c.W // 2)
        return 4 * max(plan_up4(Ml, c.C0, c.cout, 32)[0], plan_up4(Ml, c.C0, c.cout, 64)[0]) * 4 * c.C0 * c.cout * 4
    need = plan_tap(c.M, c.Cin, c.cout, c.taps)[2] * c.taps * c.Cin * c.cout * 4
    if c.taps == 9:
        need = max(need, plan9(c.M, c.Cin, c.cout, 512)[0] * 9 * c.Cin * c.cout * 4)
    return need


def launch_plan(c):
    """(chunks the GEMM writes and the reduce reads, pixels per chunk) of the launch itself"""
    if c.fam == "conv1":
        return 1, c.M
    if c.fam == "up4":
        px = 64 if c.planes == 1 else 32
        ks, sps = plan_up4(c.N * (c.H // 2) * (c.W // 2), c.C0, c.cout, px)
        return ks, sps * px
    if c.taps == 9 and c.dil <= 1:
        ks, sps = plan9(c.M, c.Cin, c.cout, 256 if c.planes else 512)
        return ks, sps * 32
    if c.planes:
        ks, sps = plan1_split(c.M, c.Cin, c.cout)
        return ks, sps * 32
    _, _, ks, sps = plan_tap(c.M, c.Cin, c.cout, c.taps)
    return ks, sps * 32


def _f9(nhw, C0, cout, kernel, **kw):
    return Case("fp32_9", nhw, C0, cout, kernel, **kw)


# fp32 operands, dense 3 x 3: conv_wgrad9_kernel<P2, IS>.  Plans: wgrad9_plan(M, Cin, Cout, 512).
FP32_9 = [
    _f9((1, 16, 16), 64, 64, "wgrad9<P2=1,IS=0>"),                 # power-of-two image; 8 steps: ks = min(512, 8 / 8) = 1
    _f9((2, 8, 32), 64, 128, "wgrad9<P2=1,IS=1>", mode=1),         # x * s in the gather; two column tiles
    _f9((2, 8, 32), 128, 64, "wgrad9<P2=1,IS=1>", mode=2),         # x * (1 - s); two row tiles
    _f9((3, 16, 48), 64, 64, "wgrad9<P2=0,IS=0>"),                 # divisions; 72 steps: ks = min(512, 9) = 9 -> 8, sps = 9, 8 chunks
    _f9((3, 16, 48), 64, 64, "wgrad9<P2=0,IS=1>", mode=1),
    _f9((1, 5, 7), 64, 64, "wgrad9<P2=0,IS=1>", mode=2),           # M = 35: two steps, the second three pixels long
    _f9((1, 5, 7), 64, 64, "wgrad9<P2=0,IS=0>"),
    _f9((2, 16, 16), 64, 64, "wgrad9<P2=1,IS=0>", C1=64),          # two sources: the row tile picks its source
    _f9((2, 16, 16), 64, 64, "wgrad9<P2=1,IS=0>", ups=1),          # the gather through the nearest x2 up-sampling, shifts
    _f9((1, 6, 10), 64, 64, "wgrad9<P2=0,IS=0>", ups=1),           # ... and divisions (source 3 x 5)
    _f9((2, 8, 8), 64, 64, "wgrad9<P2=1,IS=1>", ups=1, mode=1),    # in_scale is indexed by the SOURCE pixel
    _f9((1, 1, 1), 64, 64, "wgrad9<P2=1,IS=0>"),                   # one pixel: only the centre tap is non-zero
    _f9((1, 1, 64), 64, 64, "wgrad9<P2=1,IS=0>"),                  # H = 1: the ky = -1 / +1 strips are all outside
    _f9((2, 2, 32), 64, 64, "wgrad9<P2=1,IS=0>"),
    # gathered 64 + 64, the first source holding 40 channels and 24 pad channels WITH values: dW has 40 + 64 input channels
    _f9((2, 8, 16), 64, 64, "wgrad9<P2=1,IS=0>", C1=64, map=(104, 0, 40, 64)),
]


def _ft(nhw, C0, cout, kernel, **kw):
    return Case("fp32_tap", nhw, C0, cout, kernel, **kw)


# fp32 operands, 1 x 1 and dilation 2: conv_wgrad_kernel<WM, WN>, one tap per block.  Plans: wgrad_plan.
FP32_TAP = [
    _ft((2, 16, 16), 64, 64, "wgrad<1,1>", dil=2),                 # 9 tiles: ks = min(86, 16 / 8) = 2, sps = 8
    _ft((2, 16, 16), 64, 128, "wgrad<1,2>", dil=2),
    _ft((2, 16, 16), 128, 64, "wgrad<2,1>", dil=2),                # the 128-row tile: taps > 1 only
    _ft((3, 9, 17), 128, 128, "wgrad<2,2>", dil=2),                # ragged M = 459: 15 steps, ks = 1, sps = 15 -> 16 (even)
    _ft((1, 5, 7), 64, 64, "wgrad<1,1>", dil=2, mode=1),           # every extent within two dilated taps of a border; in_scale
    _ft((1, 3, 3), 64, 64, "wgrad<1,1>", dil=2),                   # only the centre pixel sees a neighbour two pixels away
    _ft((3, 9, 17), 64, 64, "wgrad<1,1>", taps=1),                 # 1 x 1, ragged M
    _ft((2, 16, 16), 64, 128, "wgrad<1,2>", taps=1),
    _ft((2, 16, 16), 128, 64, "wgrad<1,1>", taps=1),               # 1 x 1 keeps the 64-row tile: two row tiles
    _ft((2, 16, 16), 128, 128, "wgrad<1,2>", taps=1, C1=0),
    _ft((2, 8, 16), 64, 64, "wgrad<1,1>", taps=1, C1=64, mode=2),  # two sources and x * (1 - s)
    # M = 40960: 1280 steps, ks = min(768, 1280 / 8 = 160) = 160 -> kWgrad1MaxSplits = 128, sps = 10, 128 chunks
    _ft((2, 128, 160), 64, 64, "wgrad<1,1>", taps=1, checks=""),
]


def _p9(planes, tune, nhw, C0, cout, kernel, **kw):
    return Case("planes9", nhw, C0, cout, kernel, planes=planes, tune=tune, **kw)


# plane operands, dense 3 x 3.  Plans: wgrad9_plan(M, Cin, Cout, 256).
PLANES9 = [
    # the register-staged kernel (conv_wgrad9_split_kernel<NP, POW2, KYW>)
    _p9(3, 0, (2, 16, 16), 64, 64, "staged<3,P2=1,12 waves>"),     # three planes: always
    _p9(3, 4, (2, 16, 16), 64, 64, "staged<3,P2=1,4 waves>"),
    _p9(3, 0, (3, 16, 48), 64, 128, "staged<3,P2=0,12 waves>"),    # 72 steps: ks = min(128, 9) = 9 -> 8, sps = 9
    _p9(3, 0, (1, 5, 7), 64, 64, "staged<3,P2=0,12 waves>"),       # M = 35, no multiple of 32
    _p9(3, 0, (2, 16, 16), 64, 64, "staged<3,P2=1,12 waves>", C1=64),
    _p9(2, 8, (2, 8, 32), 64, 64, "staged<2,P2=1,12 waves>"),
    _p9(2, 4, (2, 8, 32), 64, 64, "staged<2,P2=1,4 waves>"),
    _p9(1, 0, (2, 32, 32), 64, 64, "staged<1,P2=1,12 waves>"),     # one plane, W = 32 < 64: conv_wgrad9_dma_one_plane_ok is false
    _p9(1, 0, (1, 16, 48), 64, 64, "staged<1,P2=0,12 waves>"),     # W = 48
    _p9(1, 0, (1, 5, 7), 64, 64, "staged<1,P2=0,12 waves>"),       # M % 64 != 0
    _p9(1, 8, (1, 16, 64), 64, 64, "staged<1,P2=1,12 waves>"),     # tune 8 keeps one plane off the DMA kernels where they fit
    # the LDS-DMA kernel (conv_wgrad9_dma_kernel<NPL, P2, FAST>)
    _p9(2, 0, (4, 4, 4), 64, 64, "dma<>"),                         # W = 4: a DMA piece of 8 pixels spans image rows
    _p9(2, 0, (1, 16, 48), 64, 64, "dma<>"),                       # W = 48
    _p9(2, 0, (2, 8, 8), 64, 64, "dma<P2>"),
    _p9(2, 0, (2, 16, 16), 64, 64, "dma<P2>"),
    _p9(2, 0, (2, 16, 16), 64, 64, "dma<P2>", C1=64),
    _p9(2, 0, (2, 32, 32), 64, 64, "dma<P2>", ups=1),              # up-sampling keeps W = 32 off the fast form and off the ring
    _p9(2, 16, (2, 32, 32), 64, 64, "dma<P2,fast>"),
    _p9(1, 16, (1, 16, 64), 64, 64, "dma<K64>"),                   # one plane in 64-pixel steps (32 steps: ks = 4, sps = 8, even)
    # the ring kernel (conv_wgrad9_ring_kernel)
    _p9(2, 0, (2, 32, 32), 64, 64, "ring"),                        # also bit for bit tune 16 (RING_EQUALS_ROW_MAJOR)
    _p9(2, 0, (1, 16, 64), 64, 64, "ring"),                        # W = 64: two K-steps per image row
    _p9(2, 0, (1, 8, 128), 64, 64, "ring"),                        # W = 128
    _p9(2, 0, (4, 1, 32), 64, 64, "ring"),                         # H = 1: columns one pixel high
    _p9(2, 0, (2, 2, 64), 64, 64, "ring"),                         # H = 2
    _p9(2, 0, (3, 8, 32), 64, 128, "ring"),                        # eight-row columns, odd image count: 24 steps, ks = 3, sps = 8
    _p9(2, 17, (2, 32, 32), 64, 64, "ring<shallow>"),
    _p9(1, 0, (2, 16, 64), 64, 64, "ring<K64>"),                   # 64 steps: ks = 8, sps = 8 (even)
    _p9(1, 0, (1, 16, 128), 64, 64, "ring<K64>"),
    # plan edges
    # M = 4800: 150 steps, 3 tiles: ks = min(86, 150 / 8 = 18) = 18 -> 16, sps = 10, 15 chunks hold work, rounded up to 16:
    # the reduce reads a sixteenth chunk that the GEMM must have zeroed
    _p9(2, 0, (5, 24, 40), 64, 192, "dma<>"),
    _p9(3, 0, (5, 24, 40), 64, 192, "staged<3,P2=0,12 waves>"),
    # M = 8192: 256 steps, ks = min(256, 32) = 32, sps = 8 = 256 pixels: every split starts and ends inside an image column
    _p9(2, 0, (2, 64, 64), 64, 64, "ring"),
    # 64 tiles, 8 steps: ks = 1; 16 x 16 = 256 reduce tiles: reduce_grid runs all taps per block
    _p9(2, 0, (2, 8, 16), 512, 512, "dma<P2>", checks="z"),
    _p9(2, 0, (3, 9, 17), 64, 64, "dma<>"),                        # M = 459, no multiple of 32
]
RING_EQUALS_ROW_MAJOR = (_p9(2, 0, (2, 32, 32), 64, 64, "ring"), _p9(2, 16, (2, 32, 32), 64, 64, "dma<P2,fast>"))


def _p1(planes, nhw, C0, cout, **kw):
    return Case("planes1", nhw, C0, cout, f"wgrad1_split<{planes}>", planes=planes, taps=1, **kw)


# plane operands, 1 x 1: conv_wgrad1_split_kernel<NP>.  Plans: wgrad1_split_plan.
PLANES1 = [_p1(p, (3, 9, 17), 64, 64) for p in (3, 2, 1)] + [                     # 15 steps: ks = 1
    _p1(p, (2, 16, 16), 64, 128, C1=64) for p in (3, 2, 1)] + [                   # two sources, one joint scale
    # the CRE layer: cat([corr, fm1]) gathered as 128 + C, the correlation's channels 121 .. 127 are padding WITH values; fm1 on
    # its own tensor scale, 2^5 times the correlation's
    _p1(2, (2, 16, 16), 128, 64, C1=64, map=(185, 0, 121, 128), sx1="own"),
    _p1(2, (2, 16, 16), 128, 64, C1=128, map=(249, 0, 121, 128), sx1="own"),
    _p1(1, (2, 16, 16), 128, 64, C1=64, map=(185, 0, 121, 128), sx1="own"),
    _p1(1, (2, 16, 16), 128, 64, C1=128, map=(249, 0, 121, 128), sx1="own"),
    _p1(3, (2, 16, 16), 128, 64, C1=64, map=(185, 0, 121, 128)),
    _p1(2, (2, 16, 16), 128, 64, C1=64, map=(185, 0, 121, 128)),                 # acc_scale_x1 = NULL: one joint scale
    # M = 40960: 1280 steps, ks = min(512, 160) = 160 -> kWgrad1MaxSplits = 128, sps = 10
    _p1(2, (2, 128, 160), 64, 64, checks="")]


def _u4(planes, nhw, C0, cout, **kw):
    return Case("up4", nhw, C0, cout, "up4<K64>" if planes == 1 else "up4", planes=planes, ups=1, **kw)


# the collapsed up_conv: conv_wgrad_up4_kernel<ONE>; N, H, W the HIGH-resolution size
UP4 = [_u4(2, (1, 16, 16), 64, 64),         # 64 low-resolution pixels: two steps
       _u4(2, (1, 2, 64), 64, 64),          # Hl = 1; 32 low-resolution pixels: two planes only
       _u4(2, (2, 32, 32), 64, 64),
       _u4(2, (3, 16, 32), 128, 192),       # 384 low-resolution pixels, 24 tiles x 4 phases
       _u4(1, (1, 16, 16), 64, 64),         # one plane: one 64-pixel step
       _u4(1, (2, 32, 32), 64, 64),
       _u4(1, (3, 16, 32), 128, 192)]


def nine_tap_form(c):
    """the same layer through rpnet_conv_wgrad with d->upsample"""
    return c.but(fam="planes9", tune=0, kernel=route(c.but(fam="planes9", tune=0)))


# rpnet_conv_wgrad_up4_supported must answer 0; `runs`: the nine-tap route takes the operands and is held to the bound
UP4_UNSUPPORTED = [("Wl = 4", _u4(2, (2, 8, 8), 64, 64), True),
                   ("odd H", _u4(2, (1, 7, 16), 64, 64), False),               # (no up-sampled source has an odd height: not run)
                   ("C0 = 96", _u4(2, (1, 16, 16), 96, 64), False),            # refused by rpnet_conv_wgrad too: REFUSALS
                   ("three planes", _u4(3, (2, 16, 16), 64, 64), True),
                   ("x1 set", _u4(2, (2, 16, 16), 64, 64, C1=64), True),
                   ("8 low-resolution pixels", _u4(2, (1, 2, 16), 64, 64), True),
                   ("32 low-resolution pixels on one plane", _u4(1, (1, 8, 16), 64, 64), True)]

# the first layer, Cin = 1 (cout = 96: 256 % (96 / 4) != 0, refused: REFUSALS)
CONV1 = [Case("conv1", nhw, 1, cout, "conv1_wgrad", checks="zp") for nhw in ((1, 1, 1), (1, 5, 7), (2, 16, 16), (3, 9, 17)) for cout in (32, 64)]

# dy channel magnitudes 2^-20 .. 2^0 under one tensor scale
DYNAMIC = [_p9(2, 0, (2, 32, 32), 64, 64, "ring"), _p9(2, 8, (2, 8, 32), 64, 64, "staged<2,P2=1,12 waves>"),
           _p9(2, 0, (2, 16, 16), 64, 64, "dma<P2>"), _p9(3, 0, (2, 16, 16), 64, 64, "staged<3,P2=1,12 waves>"),
           _p1(2, (2, 16, 16), 64, 64), _p1(3, (2, 16, 16), 64, 64), _u4(2, (2, 32, 32), 64, 64)]

TABLES = {"fp32_9": FP32_9, "fp32_tap": FP32_TAP, "planes9": PLANES9, "planes1": PLANES1, "up4": UP4, "conv1": CONV1}
ALL_ROWS = [c for t in TABLES.values() for c in t]


# ---------------------------------------------------------------------------------------------------------------- operands
class Ops:
    """x0, x1, dy: what the launch reads (fp32 tensors, or int16 planes [planes, N, h, w, C]); v0, v1, vdy: the float64 values they
    represent; sx, sx1, sdy: tensor scales of fp16 planes (sx1 None: joint)"""
    x1 = v1 = in_scale = sx = sx1 = sdy = None


def make_ops(c, x0, x1, dy, in_scale=None):
    o = Ops()
    o.in_scale = in_scale
    if not c.planes:
        o.x0, o.x1, o.dy = x0, x1, dy
        o.v0, o.v1, o.vdy = x0.double(), None if x1 is None else x1.double(), dy.double()
        return o
    if c.planes <= 2:
        own = c.sx1 == "own"
        o.sx = pow2_scale(x0.abs().max() if own or x1 is None else max(x0.abs().max(), x1.abs().max()))
        o.sx1 = pow2_scale(x1.abs().max()) if own else None
        o.sdy = pow2_scale(dy.abs().max())
    o.x0, o.dy = split_planes(x0, c.planes, o.sx), split_planes(dy, c.planes, o.sdy)
    o.v0, o.vdy = plane_values(o.x0, o.sx), plane_values(o.dy, o.sdy)
    if x1 is not None:
        o.x1 = split_planes(x1, c.planes, o.sx1 or o.sx)
        o.v1 = plane_values(o.x1, o.sx1 or o.sx)
    return o


def random_ops(c, key=0, dy=None):
    seed = case_seed(c.N, c.H, c.W, c.C0, c.C1, c.cout, c.taps, c.dil, c.ups, c.planes, key)
    h, w = c.H >> c.ups, c.W >> c.ups
    x0 = rnd(seed, c.N, h, w, c.C0)
    x1 = 3.0 * rnd(seed + 1, c.N, h, w, c.C1) if c.C1 else None
    if c.sx1 == "own":       # the second source's scale exactly 2^5 times the first's
        x1 = x1 * (32.0 * x0.abs().max() / x1.abs().max())
    dy = 0.5 * rnd(seed + 2, c.N, c.H, c.W, c.cout) if dy is None else dy
    s = torch.rand(c.N, h, w, generator=torch.Generator().manual_seed(seed + 3)) if c.mode else None
    o = make_ops(c, x0, x1, dy, s)
    assert c.sx1 != "own" or o.sx1 == 32.0 * o.sx
    return o


def reference(c, o, dtype=F64, absolute=False):
    """dW [cout][cin_w][kh][kw] of the represented values; absolute (plane operands: no in_scale): sum |x||dy|, with the subnormal
    floor of dropped_term() on two fp16 planes"""
    if absolute:
        assert not c.mode
        fl = lambda v, s: None if v is None else v.abs() + (s * 2.0 ** -13 if c.planes == 2 else 0.0)         # noqa: E731
        dw = R.conv_wgrad(fl(o.v0, o.sx), fl(o.v1, o.sx1 or o.sx), fl(o.vdy, o.sdy), c.taps, c.dil, c.ups, dtype=dtype)
    else:
        dw = R.conv_wgrad(o.v0, o.v1, o.vdy, c.taps, c.dil, c.ups, o.in_scale, c.mode, dtype=dtype)
    return dw[:, c.rows()].contiguous()


def dropped_term(c, o):
    """the absolute allowance per element of dW for the products the plane kernels leave out (module docstring), float64"""
    if c.planes == 2:
        u = split_unit_roundoff(1)
        return u * u * (1 + u) ** 2 * reference(c, o, absolute=True)
    if c.planes == 3:
        return split_unit_roundoff(3) * (2 + U_BF16) * (1 + U_BF16) ** 2 * reference(c, o, absolute=True)
    return None


# ----------------------------------------------------------------------------------------------------------------- records
class Rec(CC.Rec):
    def line(self):
        return (f"PARITY wgrad {self.family} {self.what} err={self.err:.3e} yard={self.yard:.3e} ratio={self.ratio:.2f} "
                f"of_bound={self.multiple:.3f}")


def _mine(r):
    r.__class__ = Rec
    return r


def exact(c, what, got, want):
    return _mine(CC.exact(c.id, what, got, want))


def bits_equal(c, what, got, want):
    """bit for bit (NaN equals the same NaN)"""
    return _mine(CC.exact(c.id, what, got.contiguous().view(torch.int32), want.contiguous().view(torch.int32)))


def whole(c, what, got, r64, r32, extra=None):
    return _mine(CC.measure(c.id, what + " whole", got, r64, r32, extra=extra))


def per_block(c, what, got, r64, r32, extra=None, group="block"):
    """the bound per (tap, 64 x 64 channel block) of dW [cout][cin][kh][kw] (group = "row": per output channel), relative to the
    block's own reference maximum: the record of the worst block.  A block whose reference is all zero must be exactly zero."""
    if not torch.isfinite(got).all():
        return Rec(c.id, f"{what} per {group}", math.inf, 0.0, FLOOR)
    d = (got.double() - r64).abs()
    if extra is not None:
        d = (d - extra).clamp_min(0)
    y = (r32.double() - r64).abs()
    worst = None
    Co, Ci = r64.shape[:2]
    blocks = ([(slice(o, o + 1), slice(0, Ci), f"row {o}") for o in range(Co)] if group == "row" else
              [(slice(o, o + 64), slice(i, i + 64), f"block co{o} ci{i}") for o in range(0, Co, 64) for i in range(0, Ci, 64)])
    for so, si, name in blocks:
        ref, err, yard = r64[so, si].abs().amax((0, 1)), d[so, si].amax((0, 1)), y[so, si].amax((0, 1))
        if group == "row":
            ref, err, yard = ref.amax().reshape(1, 1), err.amax().reshape(1, 1), yard.amax().reshape(1, 1)
        for kh in range(ref.shape[0]):
            for kw in range(ref.shape[1]):
                tag = f"{what} per {group}[{name} tap {kh},{kw}]"
                if ref[kh, kw] == 0:
                    g = got[so, si] if group == "row" else got[so, si, kh, kw]
                    bad = int((g != 0).sum())
                    if bad:
                        return Rec(c.id, tag, bad, 0.0, 0.0, exact=True)
                    continue
                yd = float(yard[kh, kw] / ref[kh, kw])
                rec = Rec(c.id, tag, err[kh, kw] / ref[kh, kw], yd, FACTOR * yd + FLOOR)
                if worst is None or rec.multiple > worst.multiple:
                    worst = rec
    return worst if worst is not None else Rec(c.id, f"{what} per {group}", 0.0, 0.0, FLOOR)


hold = CC.hold


# ------------------------------------------------------------------------------------------------------------------ checks
NAN = float("nan")


def dw_shape(c):
    k = 3 if c.taps == 9 else 1
    return (c.cout, c.map[0], k, k)


def prefill(c, key=9):
    return rnd(case_seed(c.cout, c.map[0], key), *dw_shape(c))


def _run(be, c, o, **kw):
    out = be.run(c, o, **kw)
    assert out.guard_ok, f"{c.id}: the launch wrote behind rpnet_*_workspace_bytes"
    return out


def check_bound(be, c):
    """random operands: the bound per block and over the tensor; a second identical call is bit-identical"""
    o = random_ops(c)
    r64, r32, x = reference(c, o), reference(c, o, F32), dropped_term(c, o)
    got = _run(be, c, o).dw
    again = _run(be, c, o).dw
    return [per_block(c, "dW", got, r64, r32, x), whole(c, "dW", got, r64, r32, x), bits_equal(c, "second identical call", again, got)]


def check_zeros(be, c):
    o = random_ops(c)
    z = make_ops(c, *_given(c, o, dy=torch.zeros(c.N, c.H, c.W, c.cout)))
    pre = prefill(c)
    recs = [exact(c, "dW of a zero dy", _run(be, c, z).dw, 0.0)]
    if c.fam != "conv1":          # (rpnet_conv1_wgrad has no accumulate)
        recs.append(bits_equal(c, "accumulate of a zero dy returns the pre-fill", _run(be, c, z, dw_init=pre, accumulate=1).dw, pre))
    return recs


def _given(c, o, dy):
    """the operands of o with another dy (the sources as their represented values: splitting them again is exact)"""
    f = lambda v: None if v is None else v.float()         # noqa: E731
    return f(o.v0), f(o.v1), dy, o.in_scale


def check_accumulate(be, c):
    o = random_ops(c, key=1)
    r64, r32, x, pre = reference(c, o), reference(c, o, F32), dropped_term(c, o), prefill(c)
    acc, over = _run(be, c, o, dw_init=pre, accumulate=1).dw, _run(be, c, o, dw_init=pre, accumulate=0).dw
    return [per_block(c, "dW accumulate=1", acc, r64 + pre.double(), r32 + pre, x), whole(c, "dW accumulate=1", acc, r64 + pre.double(), r32 + pre, x),
            per_block(c, "dW accumulate=0 over a pre-fill", over, r64, r32, x)]


def check_two_phase(be, c):
    """GEMM only (dw NULL), then reduce only (dy NULL): bit for bit the one-call dW; the GEMM-only call leaves dw alone"""
    o = random_ops(c, key=2)
    one = _run(be, c, o).dw
    g = _run(be, c, o, phase="gemm")
    r = _run(be, c, o, phase="reduce", ws=g.ws)
    return [bits_equal(c, "dw after the GEMM-only call", g.dw, torch.full(dw_shape(c), NAN)), bits_equal(c, "two-phase dW", r.dw, one)]


def impulse_groups(c):
    """[(x positions, dy positions)] per launch: x = 2^a at ONE pixel of input channel j, dy = 2^b at one pixel of output channel
    9 j + k: the pixel from which tap k of dy reaches x's.  Positions: an interior pixel and the four image corners (with
    up-sampling: the four phases of one source pixel, the first and the last pixel), all nine relative offsets each; then the
    leakage pairs: x in the last column and dy in the first column of the next row, x in the last row of image n and dy in the
    first row of image n + 1.  Every dW element is one product of powers of two or zero: exact in every plane arithmetic."""
    H, W, d = c.H, c.W, max(c.dil, 1)
    iy, ix = min(H - 1, (H // 2) | 1 if c.ups else H // 2), min(W - 1, (W // 2) | 1 if c.ups else W // 2)
    if c.ups:
        pos = [(iy - 1, ix - 1), (iy - 1, ix), (iy, ix - 1), (iy, ix), (0, 0), (H - 1, W - 1)]
    else:
        pos = [(iy, ix), (0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    pos = list(dict.fromkeys(pos))
    n0 = c.N - 1
    items = []           # (image, y, x) of the x impulse (output resolution), [(image, y, x) of dy impulses]
    for (y, x) in pos:
        items.append(((n0, y, x), [(n0, y - (k // 3 - 1) * d, x - (k % 3 - 1) * d) if c.taps == 9 else (n0, y, x) for k in range(c.taps)]))
    if c.taps == 9:
        if H > 1:           # ... and the other way round: x in the first column, dy in the last column of the row above
            items += [((n0, 0, W - 1), [(n0, 1, 0)]), ((n0, 1, 0), [(n0, 0, W - 1)])]
        if c.N > 1:
            items += [((0, H - 1, W // 2), [(1, 0, W // 2)]), ((1, 0, W // 2), [(0, H - 1, W // 2)])]
    per = c.Cin if c.fam != "conv1" else 1
    return [items[i:i + per] for i in range(0, len(items), per)]


def check_impulses(be, c):
    recs = []
    for gi, items in enumerate(impulse_groups(c)):
        h, w = c.H >> c.ups, c.W >> c.ups
        xs = torch.zeros(c.N, h, w, c.Cin)
        dy = torch.zeros(c.N, c.H, c.W, c.cout)
        co = 0
        for j, ((n, y, x), dys) in enumerate(items):
            xs[n, y >> c.ups, x >> c.ups, (j * 37) % c.Cin] = 2.0 ** (j % 4 - 2)
            for (m, yy, xx) in dys:
                if 0 <= yy < c.H and 0 <= xx < c.W:
                    dy[m, yy, xx, co % c.cout] = 2.0 ** (co % 5 - 3)
                co += 1
        assert co <= c.cout
        o = make_ops(c, xs[..., :c.C0].contiguous(), xs[..., c.C0:].contiguous() if c.C1 else None, dy,
                     torch.ones(c.N, h, w) if c.mode == 1 else torch.zeros(c.N, h, w) if c.mode == 2 else None)
        want = reference(c, o)
        assert bool((want.float().double() == want).all()) and (gi > 0 or bool((want != 0).any()))     # (a leakage pair alone: all zero)
        recs.append(exact(c, f"impulses {gi}", _run(be, c, o).dw.double(), want))
    return recs


def dynamic_dy(c, seed):
    """[N, H, W, cout]: standard normal times 2^-(20 j / (cout - 1)) rounded to a power of two, channel j"""
    e = torch.round(torch.arange(c.cout) * (20.0 / (c.cout - 1)))
    return rnd(seed, c.N, c.H, c.W, c.cout) * 2.0 ** -e, e


def check_dynamic_range(be, c):
    """dy rows from 2^0 down to 2^-20 under ONE tensor scale, judged per output channel against the ORIGINAL fp32 dy (the split of
    dy is what is under test).  Three bf16 planes represent an fp32 value exactly: every row meets the plain bound.  Two fp16
    planes: a value v of a tensor whose maximum m sets the scale is kept to u^2 |v| while its residual is a normal fp16 number and
    to 2^-25 2^-14 m below that, together <= split_unit_roundoff(2) m; rows within 2^-13 of the largest have every residual that
    matters normal and meet the plain bound (the dropped l.l product is allowed for as everywhere); smaller rows get
    split_unit_roundoff(2) * max |dy| * sum |x| per element."""
    seed = case_seed(c.N, c.H, c.W, c.cout, c.planes, 55)
    dy, e = dynamic_dy(c, seed)
    o = random_ops(c, key=3, dy=dy)
    full = Ops()
    full.__dict__.update(o.__dict__)
    full.vdy = dy.double()
    r64, r32, x = reference(c, full), reference(c, full, F32), dropped_term(c, o)
    got = _run(be, c, o).dw
    if c.planes == 3:
        return [per_block(c, "dynamic dW", got, r64, r32, x, group="row")]
    ones = Ops()
    ones.__dict__.update(o.__dict__)
    ones.vdy, ones.sdy = torch.full_like(full.vdy, float(dy.abs().max())), 0.0
    floor = split_unit_roundoff(2) * reference(c.but(planes=0), ones, absolute=True)
    big = e <= 13
    recs = [per_block(c, "dynamic dW, rows within 2^-13", got[big], r64[big], r32[big], x[big], group="row")]
    if (~big).any():
        recs.append(per_block(c, "dynamic dW, smaller rows", got[~big], r64[~big], r32[~big], (x + floor)[~big], group="row"))
    return recs


def checks_of(c):
    """every check of a table row, in the order the lines are recorded"""
    fns = [check_bound]
    if "z" in c.checks:
        fns.append(check_zeros)
    if "a" in c.checks:
        fns.append(check_accumulate)
    if c.two_phase:
        fns.append(check_two_phase)
    if "p" in c.checks:
        fns.append(check_impulses)
    return fns


def check_row(be, c):
    assert route(c) == c.kernel, f"{c.id}: the launcher takes {route(c)}, the table says {c.kernel}"
    return [r for fn in checks_of(c) for r in fn(be, c)]


def check_ring_equals_row_major(be):
    ring, row = RING_EQUALS_ROW_MAJOR
    assert route(ring) == "ring" and route(row) == "dma<P2,fast>"
    o = random_ops(ring)
    return [bits_equal(ring, "ring == tune 16", _run(be, ring, o).dw, _run(be, row, o).dw)]


def check_up4_against_nine_tap(be, c):
    """the collapsed form and rpnet_conv_wgrad with d->upsample on the same operands, both held to the same reference"""
    n = nine_tap_form(c)
    o = random_ops(c)
    r64, r32, x = reference(c, o), reference(c, o, F32), dropped_term(c, o)
    got = _run(be, n, o).dw
    return [per_block(n, "dW nine-tap form", got, r64, r32, x), whole(n, "dW nine-tap form", got, r64, r32, x)]


# --------------------------------------------------------------------------------------------------------------- refusals
# (label, base case, changes to the call, status): every RPNET_REQUIRE line of the three entry points, refused on the host before
# any launch.  Changes: a Case field; or null=<pointer name>; ws_short=1; huge=(N, H, W) (the pointers stay small buffers: nothing
# is read); no_scales=1; phase.  The lines that fire BEHIND the GEMM launch (fp16 planes without scales) are reached reduce-only.
_B9, _B1, _BT = _f9((1, 16, 16), 64, 64, ""), _p1(2, (2, 16, 16), 64, 64), _ft((2, 16, 16), 64, 64, "", dil=2)
_S9, _BU, _BC = _p9(2, 0, (2, 16, 16), 64, 64, ""), _u4(2, (1, 16, 16), 64, 64), Case("conv1", (2, 16, 16), 1, 64, "")
REFUSALS = [
    ("null x0", _B9, dict(null="x0"), ARG), ("null workspace", _B9, dict(null="ws"), ARG), ("null dy and dw", _S9, dict(null="dy,dw"), ARG),
    ("two-phase on fp32 operands", _B9, dict(phase="gemm"), ARG), ("two-phase on fp32 operands (reduce)", _B9, dict(phase="reduce"), ARG),
    ("taps = 4", _B9, dict(taps=4), ARG), ("planes with dilation 2", _S9, dict(dil=2), ARG),
    ("Cin = 96", _B9, dict(C0=96), SHAPE), ("Cout = 96", _B9, dict(cout=96), SHAPE),
    ("Cin = 96, the shape rpnet_conv_wgrad_up4_supported turns away", nine_tap_form(_u4(2, (1, 16, 16), 96, 64)), {}, SHAPE),
    ("2^31 pixels", _B9, dict(huge=(65536, 256, 128)), SHAPE), ("an operand of 2 GiB", _B9, dict(huge=(128, 256, 256)), SHAPE),
    ("source split 32 + 32", _B9, dict(C0=32, C1=32), SHAPE), ("short workspace, nine taps", _B9, dict(ws_short=1), WORKSPACE),
    ("four planes", _S9, dict(planes=4), ARG), ("planes with in_scale", _S9, dict(mode=1), ARG),
    ("fp16 planes without scales, nine taps", _S9, dict(no_scales=1, phase="reduce"), ARG),
    ("four planes, 1 x 1", _B1, dict(planes=4), ARG), ("planes with in_scale, 1 x 1", _B1, dict(mode=2), ARG),
    ("planes with upsampling, 1 x 1", _B1, dict(ups=1), ARG), ("source split 32 + 32, 1 x 1", _B1, dict(C0=32, C1=32), SHAPE),
    ("second source without its pointer, 1 x 1", _B1, dict(C1=64, null="x1"), SHAPE),
    ("short workspace, 1 x 1", _B1, dict(ws_short=1), WORKSPACE),
    ("fp16 planes without scales, 1 x 1", _B1, dict(no_scales=1, phase="reduce"), ARG),
    ("source split 64 + 64 under the 128-row tile", _BT, dict(C1=64), SHAPE), ("short workspace, one tap per block", _BT, dict(ws_short=1), WORKSPACE),
    ("null x0", _BU, dict(null="x0"), ARG), ("null workspace", _BU, dict(null="ws"), ARG), ("null dy and dw", _BU, dict(null="dy,dw"), ARG),
    ("Wl = 4", _u4(2, (2, 8, 8), 64, 64), {}, SHAPE), ("three planes", _BU, dict(planes=3), SHAPE), ("x1 set", _BU, dict(C1=64), SHAPE),
    ("short workspace", _BU, dict(ws_short=1), WORKSPACE), ("fp16 planes without scales", _BU, dict(no_scales=1, phase="reduce"), ARG),
    ("null x", _BC, dict(null="x0"), ARG), ("null dy", _BC, dict(null="dy"), ARG), ("null dw", _BC, dict(null="dw"), ARG),
    ("null workspace", _BC, dict(null="ws"), ARG), ("cout = 96", _BC, dict(cout=96), SHAPE), ("cout = 260", _BC, dict(cout=260), SHAPE),
    ("short workspace", _BC, dict(ws_short=1), WORKSPACE),
    # (conv1_wgrad's N % groups line cannot fail through rpnet_conv1_wgrad: it passes groups = 1)
]


# ----------------------------------------------------------------------------------------- the float32 stand-in for the library
DEFECTS = ["drop_cross", "last_col", "row_wrap", "image_wrap", "swap_khkw", "pad_rows", "ignore_sx1", "overwrite", "surplus", "up_phase"]


class Out:
    def __init__(self, dw, ws, guard_ok=True):
        self.dw, self.ws, self.guard_ok = dw, ws, guard_ok


class SimBackend:
    """A float32 torch restatement of the three entry points with the library's split-K plan: the GEMM writes partial
    [chunks][taps][Cin][Cout] into a NaN-filled workspace (zeros into the surplus chunks), the plane products are formed one by
    one as the kernels form them (the dropped ones dropped), the reduce adds the chunks in sequence, applies the scales, maps the
    gathered rows onto dW's input channels and accumulates.  `defect`: one of DEFECTS."""

    def __init__(self, defect=None):
        assert defect is None or defect in DEFECTS
        self.defect = defect

    def _taps(self, c, x, s):
        """x [N, h, w, C] fp32 -> [taps][M, C]: the gathered, shifted operand of every tap"""
        N, H, W, d = c.N, c.H, c.W, max(c.dil, 1)
        if s is not None:
            x = x * (s if c.mode == 1 else 1.0 - s)[..., None]
        if c.ups:
            iy, ix = torch.arange(H) >> 1, torch.arange(W) >> 1
            if self.defect == "up_phase":
                ix = ((torch.arange(W) + 1) >> 1).clamp_max((W >> 1) - 1)
            x = x[:, iy][:, :, ix]
        if c.taps == 1:
            return [x.reshape(c.M, -1)]
        xp = F.pad(x, (0, 0, d, d, d, d))
        flat = torch.cat([x.reshape(c.M, -1), torch.zeros(W + 1, x.shape[-1])])
        out = [None] * 9
        for kh in range(3):
            for kw in range(3):
                a = xp[:, kh * d:kh * d + H, kw * d:kw * d + W].clone()
                if self.defect == "last_col" and kw == 2 and W > d:
                    a[:, :, W - 1 - d] = 0
                a = a.reshape(c.M, -1)
                p = torch.arange(c.M)
                if self.defect == "row_wrap" and kw == 2 and kh == 1:
                    m = p % W == W - 1
                    a[m] = flat[p[m] + 1]
                if self.defect == "image_wrap" and kh == 2 and kw == 1:
                    m = (p // W) % H == H - 1
                    a[m] = flat[p[m] + W]
                out[kw * 3 + kh if self.defect == "swap_khkw" else kh * 3 + kw] = a
        return out

    def _gemm(self, c, o, ws):
        ks, px = launch_plan(c)
        if c.fam == "up4":
            px *= 4
        s = None if o.in_scale is None else o.in_scale.float()
        if c.planes:
            f = torch.bfloat16 if c.planes == 3 else torch.float16
            xs = [torch.cat([o.x0[p].view(f).float()] + ([o.x1[p].view(f).float()] if c.C1 else []), -1) for p in range(c.planes)]
            ds = [o.dy[p].view(f).float().reshape(c.M, -1) for p in range(c.planes)]
            prods = {3: [(2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)], 2: [(1, 0), (0, 1), (0, 0)], 1: [(0, 0)]}[c.planes]
            if self.defect == "drop_cross" and c.planes == 2:
                prods = [(1, 0), (0, 0)]
        else:
            xs = [o.x0 if o.x1 is None else torch.cat([o.x0, o.x1], -1)]
            ds, prods = [o.dy.reshape(c.M, -1)], [(0, 0)]
        A = [self._taps(c, x, s) for x in xs]
        for z in range(ks):
            lo, hi = z * px, min((z + 1) * px, c.M)
            if lo >= hi:
                if self.defect != "surplus":
                    ws[z] = 0
                continue
            for t in range(c.taps):
                acc = torch.zeros(c.Cin, c.cout)
                for (pa, pb) in prods:
                    acc = acc + A[pa][t][lo:hi].T @ ds[pb][lo:hi]
                ws[z, t] = acc
        return ws

    def _reduce(self, c, o, ws, dw, accumulate):
        total = torch.zeros_like(ws[0])
        for z in range(ws.shape[0]):
            total = total + ws[z]
        if c.planes in (1, 2):
            sc = torch.full((c.Cin, 1), float(o.sx))
            if o.sx1 is not None and self.defect != "ignore_sx1":
                sc[c.C0:] = float(o.sx1)
            total = total * (sc * float(o.sdy))
        rows = c.rows()
        res = total[:, rows]                                        # [taps, cin_w, cout]
        cin_w, off0, split, off1 = c.map
        if self.defect == "pad_rows" and off1 > off0 + split:
            res[:, split - 1] += total[:, off0 + split:off1].sum(1)
        res = res.permute(2, 1, 0).reshape(dw.shape)
        return dw + res if accumulate and self.defect != "overwrite" else res

    def run(self, c, o, dw_init=None, accumulate=0, phase="both", ws=None):
        dw = torch.full(dw_shape(c), NAN) if dw_init is None else dw_init.clone()
        if ws is None:
            ws = torch.full((launch_plan(c)[0], c.taps, c.Cin, c.cout), NAN)
        if phase != "reduce":
            ws = self._gemm(c, o, ws)
        if phase != "gemm":
            dw = self._reduce(c, o, ws, dw, accumulate)
        return Out(dw, ws)
