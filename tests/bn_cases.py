"""Cases and comparison functions shared by tests/test_host_bn_ref64.py and tests/test_gpu_bn_fp64.py: the BatchNorm kernels of
csrc/bn.hip (rpnet_bn_stats, rpnet_bn_stats_from_partial, rpnet_bn_eval_affine, rpnet_bn_relu, rpnet_bn_bwd, rpnet_bn_eval_relu,
rpnet_bn_eval_bwd) against the float64 references of tests/ref64.py (bn_stats, bn_relu, bn_relu_pool, bn_bwd, bn_eval_*) at every
branch of their dispatch.  The layout is that of tests/wgrad_cases.py; the definitions of tests/corr_cases.py (split_planes,
plane_values, pow2_scale, split_unit_roundoff, case_seed, FACTOR, FLOOR, Rec, measure, exact, hold) are used, not restated.

A *backend* runs ONE entry point described by a Case on CPU tensors: the HIP library (the GPU test) or SimBackend, a float32 torch
restatement with the library's partial / finalize split, with or without a seeded defect (the host test).

Element-wise outputs (z, dy): rel_err(got, r64) <= FACTOR * yard + FLOOR, yard = rel_err(r32, r64), per (group, channel) against
that channel's own reference maximum and over the whole tensor; a channel whose reference is all zero must be exactly zero.

Activation mask.  Where |y scale + shift| of the float64 reference is <= 2^-23 (|y scale| + |shift|), the rounding of that
expression in fp32, a kernel may land on the other side of the ReLU; in a pooled window, where the two largest affine values differ
by no more than that (and are not equal: an exact tie is settled by position) the gradient may go to either pixel.  Those elements
(whole windows in the pooled form) are excluded, by this criterion computed from the reference alone, at most EXCLUDED_CAP of a
case's elements; the sums they feed get |dz|, respectively |dz xhat|, per excluded element as an allowance.

Reductions the header promises in fp64 (mean, invstd, scale, shift, running buffers, dgamma, dbeta, coef): NOT the yardstick (on the
offset row, mean = 2^10 standard deviations, an fp32 reference is useless).  The bound is the arithmetic the code states.  U = 2^-23
is one unit in the last place of an fp32 result, i.e. two units of 2^-24; round to nearest commits half of it, which is the room the
host test demands of a correct stand-in (of_bound < 0.5).  E = (R + 2048) 2^-53 bounds a sum of R + nblk + 256 + 8 fp64 additions
relative to sum |terms| (bn_stats_partial / bn_bwd_partial, rows_reduce, the 256 lanes of the finalize, block_sum256).
  bn_stats_finalize, per (group, channel), m = s / R, var = q / R - m m in fp64:
    dvar = 4 E (mean(y^2) + m^2)                      the fp64 cancellation, k = dvar / (2 (var + eps)) its share of invstd
    mean   = (float) m                                 1 op:  U |m| + E mean|y|
    invstd = (float)(1 / sqrt(var + eps))              1 op:  (U + k) invstd
    scale  = gamma * invstd                            2 ops: (2 U + k) |scale|
    shift  = beta - (float) m * scale                  (float) m, scale (2), the product, the difference:
                                                       (4 U + k) |m scale| + U |shift| + E mean|y| |scale|
    running = (1.f - momentum) * r + momentum * x      per group, x = (float) m or (float) unbiased var; 1.f - momentum, the two
                                                       products, (float) x and the sum; the error so far shrinks by 1 - momentum:
                                                       a' = (1 - mom) a + U (2 |(1 - mom) r| + 2 |mom x| + |r'|) + mom dx,
                                                       dx = E mean|y| (mean) or dvar R / (R - 1) (variance)
  bn_bwd_finalize, per channel, s1 = sum dz m, s2 = sum dz m xhat with xhat = (y - mean) * invstd formed in fp32 (2 ops):
    coef1 = (float)(s1 / R)                            U |coef1| + E sum|dz m| / R
    coef2 = (float)(s2 / R)                            U |coef2| + (2 U + E) sum|dz m xhat| / R
    dbeta = (float) sum_g s1, dgamma = (float) sum_g s2   the same with R = 1, summed over the groups
  each plus the activation-mask allowance.  Cancellation is part of the definition of dbeta and dgamma, hence sum |terms|.

Split outputs are compared as the values they represent (plane_values): three bf16 planes bit for bit with the fp32 output where
both are written, else within split_unit_roundoff(3); two and one fp16 plane within split_unit_roundoff(planes) times the range of
the tensor scale (s 2^15), the published scale s = pow2_scale of the header's rigorous bound evaluated in float64 (the library
evaluates it in fp32 with 1.0001 of slack on sqrt(n), respectively on the bound: s may be the float64 value with or without that
slack), and max |value / s| <= 2^15.  Pooled planes: bit for bit the split of the pooled fp32 output on the same scale.

Exact checks count mismatching elements and allow none.  No check carries a measured factor."""
import math
import types

import numpy as np
import torch
import torch.nn.functional as F

from tests import corr_cases as CC
from tests import ref64 as R
from tests.corr_cases import ARG, FACTOR, FLOOR, SHAPE, WORKSPACE, case_seed, plane_values, pow2_scale, split_planes, split_unit_roundoff  # noqa: F401
from tests.helpers import rnd

F32, F64 = torch.float32, torch.float64
GUARD = 64                                  # words behind the workspace that must come back as they went in
NAN = float("nan")
U = 2.0 ** -23                              # one unit in the last place of an fp32 result (module docstring)
MOM, EPS = float(np.float32(0.1)), float(np.float32(1e-5))       # the values the launch receives as fp32
EXCLUDED_CAP = 1e-3
POISON = 1.0e6                              # rows behind the given partial sums: no launch may read them
SLACK = 1.0001                              # on sqrt(n) (rpnet_bn_relu) and on the bound (bn_bwd_finalize)


# ---------------------------------------------------------------------------------------------------------------- geometry
def max_blocks(C):
    """bn_max_blocks (csrc/bn.hip)"""
    return min(max(131072 // C, 256), 1024)


def geom(Rg, C):
    """bn_geom: (C4, rows_it, nblk, rows_blk)"""
    C4 = C // 4
    rows_it = 256 // C4
    nblk = min(max(-(-Rg // (rows_it * 4)), 1), max_blocks(C))
    return C4, rows_it, nblk, -(-Rg // nblk)


def workspace_bytes(c):
    """what rpnet_bn_workspace_bytes must answer (the GPU test asserts the two agree)"""
    rows = c.G * max_blocks(c.C)
    return rows * c.C * 2 * 8 + c.G * c.C * 2 * 4 + rows * c.C * 4 + c.C * 4


def coef_offset(c):
    """rpnet_bn_bwd_coef_offset"""
    return c.G * max_blocks(c.C) * c.C * 2 * 8


# ------------------------------------------------------------------------------------------------------------------- cases
class Case:
    """one launch.  op: stats | from_partial | relu | bwd | eval_affine | eval_relu | eval_bwd.  N, H, W, C of the pre-BatchNorm
    tensor, G statistic groups.  planes: 0 (no split output) .. 3; fp32: the fp32 output is asked for; pool: the MaxPool2d(2, 2)
    form; given: rows of caller-made partial sums (0: the launch reduces itself); nblk: partial rows of from_partial; red: the
    reduction-only call; want_scale: the fp32-only forward publishes the tensor scale.  data: letters o (offset: mean = 2^10
    standard deviations), e (edges: channel 0 constant, channel 2 negative throughout), t (tied window maxima), d (dz channels
    2^0 .. 2^-20), x (one element of dz 2^12 times the rest).  kernel: what route() must answer."""

    def __init__(self, op, nhw, C, G, kernel, planes=0, fp32=True, pool=False, given=0, nblk=0, red=False, want_scale=False,
                 data="", no_y=False):
        self.op, (self.N, self.H, self.W), self.C, self.G, self.kernel = op, nhw, C, G, kernel
        self.planes, self.fp32, self.pool, self.given, self.nblk, self.red = planes, fp32, pool, given, nblk, red
        self.want_scale, self.data, self.no_y = want_scale, data, no_y

    HW = property(lambda s: s.H * s.W)
    R = property(lambda s: s.N // s.G * s.H * s.W)            # rows per group
    f16 = property(lambda s: s.planes in (1, 2))

    @property
    def id(self):
        return (f"{self.op}-{self.N}x{self.H}x{self.W}x{self.C}-g{self.G}" + (f"-p{self.planes}" if self.planes else "")
                + ("" if self.fp32 or self.op not in ("relu", "bwd", "eval_bwd") else "-nofp32") + ("-pool" if self.pool else "")
                + (f"-given{self.given}" if self.given else "") + (f"-nblk{self.nblk}" if self.nblk else "") + ("-red" if self.red else "")
                + ("-scale" if self.want_scale else "") + ("-noy" if self.no_y else "") + (f"-{self.data}" if self.data else ""))


def route(c):
    """the launches an entry point makes for a case, in order: the conditions of rpnet_bn_stats, _stats_from_partial, _eval_affine,
    _relu, _bwd, _eval_relu and _eval_bwd (csrc/bn.hip) under the default dispatch (one-wave LDS window, guarded pooled passes),
    restated once; every table row is asserted against it"""
    p = c.planes
    if c.op == "stats":
        return "bn_stats_partial<64> bn_stats_finalize"
    if c.op == "from_partial":
        return "bn_stats_finalize"
    if c.op == "eval_affine":
        return "bn_eval_affine_kernel"
    if c.op == "eval_relu":
        return "bn_eval_relu_kernel"
    if c.op == "relu":
        if c.pool:
            assert p and c.C % 8 == 0
            return f"bn_relu_pool_split_kernel<{p},drain>" + ("" if c.fp32 else "[zp=NULL]")
        if p:
            assert c.C % 8 == 0
            return f"bn_relu_split_kernel<{p}>" + ("" if c.fp32 else "[z=NULL]")
        return "bn_relu_kernel" + ("[s_out]" if c.want_scale else "")
    pm = "[pmax]" if c.f16 else ""
    if c.op == "bwd" and c.pool:
        assert p and not c.given and not c.red
        return f"bn_bwd_partial_pool<64>{pm} bn_bwd_finalize{pm} bn_bwd_apply_pool_split<{p},drain>" + ("" if c.fp32 else "[dy=NULL]")
    if c.op == "bwd":
        red = f"bn_bwd_finalize[given]{pm}" if c.given else f"bn_bwd_partial<64>{pm} bn_bwd_finalize{pm}"
    else:
        assert c.op == "eval_bwd"
        red = f"bn_bwd_partial<64>{pm} bn_eval_bwd_finalize{pm}"
    if c.red:
        assert not p
        return red
    if p:
        return f"{red} bn_bwd_apply_split<{p}>" + ("" if c.fp32 else "[dy=NULL]")
    return f"{red} bn_bwd_apply"


# rows_it = 256 / C4 rows per block iteration, a block iteration covers 4 rows_it rows:
#   C = 4: 256 / 1024    8: 128 / 512    24: 42 / 168    64: 16 / 64    72: 14 / 56 (252 of 256 threads hold rows)
#   192: 5 / 20 (240 threads)    512: 2 / 8 (the owners, row 0, span two waves)    1024: 1 / 4 (every thread owns its sums)
SHAPES = {
    "one": ((1, 1, 1), 4, 1),            # R = 1: variance 0, the R > 1 branch of the unbiased variance
    "c4": ((2, 3, 5), 4, 1),             # R = 30 < rows_it = 256: most threads hold no row
    "c4g3": ((3, 1, 1), 4, 3),           # three groups of one row each
    "c8g3": ((6, 5, 5), 8, 3),           # three groups of two images; R = 50 < rows_it = 128; 400 elements per group: the boundary
                                         # falls inside the first 256-thread block of every element-wise pass
    "c24": ((1, 5, 7), 24, 1),           # R = 35 < rows_it = 42
    "c24g2": ((4, 9, 13), 24, 2),        # R = 234 = 168 + 66: two blocks, the second ragged; 5616 elements per group, no multiple
                                         # of 256 x 8: the group boundary falls inside a block
    "c24big": ((2, 25, 43), 24, 1),      # R = 2150 = 12 x 168 + 134: thirteen blocks
    "c72": ((2, 7, 9), 72, 1),           # C4 = 18: 256 threads are no whole number of rows; R = 126 = 2 x 56 + 14
    "c72g3": ((3, 5, 7), 72, 3),         # R = 35 < 56, three groups of one image
    "c192g2": ((2, 9, 11), 192, 2),      # R = 99 = 4 x 20 + 19
    "c512g2": ((4, 3, 3), 512, 2),       # R = 18 = 2 x 8 + 2, two images per group
    "c1024": ((1, 3, 3), 1024, 1),       # one row per pass; R = 9 = 2 x 4 + 1
    "c1024g2": ((2, 3, 3), 1024, 2),
    "clamp": ((1, 2, 32801), 64, 1),     # R = 65602 > 1024 x 16 x 4: bn_geom clamps to bn_max_blocks = 1024 and the blocks loop
    # pooled: H, W, Ho, Wo and the images per group are no powers of two
    "pool": ((6, 6, 10), 24, 2),         # three images per group, 3 x 5 pooled pixels
    "pool72": ((3, 10, 6), 72, 1),       # C / 8 = 9, 5 x 3 pooled pixels
    "pool2x2": ((3, 2, 2), 8, 3),        # H = W = 2: one window per image, one image per group
    "pool512": ((2, 6, 2), 512, 2),      # Wo = 1
}


def _row(op, shape, kernel, **kw):
    nhw, C, G = SHAPES[shape]
    return Case(op, nhw, C, G, kernel, **kw)


# Every row carries the launches it is meant to reach as a LITERAL string (the host test asserts route(c) == c.kernel row by row)
# and says beside it which edge it hits; the shape's own edge stands in SHAPES.
def _st(shape, data=""):
    return _row("stats", shape, "bn_stats_partial<64> bn_stats_finalize", data=data)


STATS = [
    _st("one"),                          # R = 1: var = 0, invstd = 1 / sqrt(eps), the unbiased variance keeps var
    _st("c4"),                           # fewer rows than rows_it: one block, threads without a row add zeros
    _st("c4g3"),                         # three running updates from three one-row groups
    _st("c8g3", "o"),                    # offset data: fp64 accumulation; three groups of two images
    _st("c24", "e"),                     # R below rows_it; a constant channel and one negative throughout
    _st("c24g2", "e"),                   # two blocks per group, the second ragged; the running update per group
    _st("c24big", "o"),                  # offset data over thirteen blocks: q / R - m m cancels 20 bits
    _st("c72"),                          # 252 of 256 threads hold rows: the one-wave window walks C4 = 18 columns
    _st("c72g3", "o"),                   # offset data, three groups, rows_reduce with a ragged last window
    _st("c192g2"),                       # rows_it = 5, 240 threads
    _st("c512g2", "e"),                  # the owners span two waves: two LDS windows hold owner rows
    _st("c1024"),                        # rows_it = 1: rows_reduce adds nothing, every thread writes its own sums
    _st("c1024g2", "o"),                 # the same per group, offset data
    _st("clamp"),                        # nblk clamped to 1024, rows_blk = 65: blocks loop over five iterations
]


def _fp(shape, nblk, data=""):
    return _row("from_partial", shape, "bn_stats_finalize", nblk=nblk, data=data)


# rpnet_bn_stats_from_partial on partial sums formed on the host in float64; nblk is never what bn_geom would have chosen
FROM_PARTIAL = [
    _fp("c24g2", 1),                     # one partial row per group (bn_geom: 2): 255 lanes read nothing
    _fp("c24g2", 257, "e"),              # one more than the finalize's 256 lanes: lane 0 reads two rows; most rows are empty
    _fp("c72g3", 5, "o"),                # five rows where bn_geom has one; offset data, three groups: the group stride is nblk
    _fp("c1024", 257),                   # 257 rows at the widest channel count
    _fp("c4", 3),                        # three rows at C = 4
]


def _re(shape, kernel, planes=0, fp32=True, data="", want_scale=False, pool=False):
    return _row("relu", shape, kernel, planes=planes, fp32=fp32, data=data, want_scale=want_scale, pool=pool)


RELU = [
    # fp32 output only: bn_relu_kernel, FastDiv by C / 4 and by the group's float4 count
    _re("one", "bn_relu_kernel"),                                        # one float4: FastDiv(1) twice
    _re("c4", "bn_relu_kernel"),                                         # C4 = 1
    _re("c8g3", "bn_relu_kernel"),                                       # three groups, the boundaries inside block 0
    _re("c24g2", "bn_relu_kernel", data="e"),                            # group boundary inside a block; an all-zero channel
    _re("c24big", "bn_relu_kernel", data="o"),                           # offset data: y scale + shift cancels ten bits
    _re("c72", "bn_relu_kernel"),                                        # C4 = 18, no power of two
    _re("c192g2", "bn_relu_kernel[s_out]", want_scale=True),             # block 0 also publishes the tensor scale
    _re("c512g2", "bn_relu_kernel"),                                     # two images per group
    _re("c1024g2", "bn_relu_kernel"),                                    # C4 = 256: one row per block
    # three bf16 planes
    _re("c24g2", "bn_relu_split_kernel<3>", 3, data="e"),                # planes and fp32 z: bit for bit
    _re("c72", "bn_relu_split_kernel<3>", 3),                            # C / 8 = 9
    _re("c8g3", "bn_relu_split_kernel<3>[z=NULL]", 3, fp32=False),       # planes only; C / 8 = 1, three groups
    # two fp16 planes on the scale of the rigorous bound
    _re("c24g2", "bn_relu_split_kernel<2>", 2, data="e"),                # |beta| of the negative channel sets the scale
    _re("c192g2", "bn_relu_split_kernel<2>", 2),                         # every block forms the scale from 192 channels
    _re("c72g3", "bn_relu_split_kernel<2>[z=NULL]", 2, fp32=False),      # planes only, three groups
    _re("c24big", "bn_relu_split_kernel<2>", 2, data="o"),               # offset data
    # one fp16 plane
    _re("c24g2", "bn_relu_split_kernel<1>", 1),                          # group boundary inside a block
    _re("c512g2", "bn_relu_split_kernel<1>[z=NULL]", 1, fp32=False),     # the channel loop of the scale runs twice per thread
    _re("c8g3", "bn_relu_split_kernel<1>", 1),                           # C / 8 = 1
]
RELU_POOL = [
    _re("pool", "bn_relu_pool_split_kernel<3,drain>", 3, data="t", pool=True),               # tied windows; FastDiv by 3, 5, 3
    _re("pool", "bn_relu_pool_split_kernel<2,drain>", 2, data="t", pool=True),               # the same on two fp16 planes
    _re("pool", "bn_relu_pool_split_kernel<1,drain>", 1, pool=True),                         # one plane
    _re("pool72", "bn_relu_pool_split_kernel<2,drain>", 2, data="t", pool=True),             # C / 8 = 9, one group of three
    _re("pool72", "bn_relu_pool_split_kernel<3,drain>[zp=NULL]", 3, fp32=False, pool=True),  # planes only
    _re("pool2x2", "bn_relu_pool_split_kernel<2,drain>", 2, pool=True),                      # H = W = 2: Ho = Wo = 1
    _re("pool2x2", "bn_relu_pool_split_kernel<1,drain>[zp=NULL]", 1, fp32=False, data="t", pool=True),      # ... tied, planes only
    _re("pool512", "bn_relu_pool_split_kernel<2,drain>", 2, pool=True),                      # Wo = 1, 64 threads per pooled pixel
]


def _bw(shape, kernel, planes=0, fp32=True, data="", op="bwd", **kw):
    return _row(op, shape, kernel, planes=planes, fp32=fp32, data=data, **kw)


_RED, _REDM = "bn_bwd_partial<64> bn_bwd_finalize", "bn_bwd_partial<64>[pmax] bn_bwd_finalize[pmax]"      # (the reduction's two launches)
# One offset row (c8g3, data "o"): the passes are GIVEN the statistics in fp32, and a mean rounded at 2^10 standard deviations is
# 2^-14 of one off the batch mean, so autograd of the batch statistics and the closed form the kernels evaluate differ by that
# much whatever the kernel does.  That row is held to the closed form at the given statistics (ref64.bn_bwd_sums / bn_dy): it
# covers xhat = (y - mean) invstd under ten bits of cancellation.  It is small enough that no element of it lies inside the
# activation-mask zone (asserted on the host): a flipped element uses its whole allowance.
BWD = [
    # fp32 dy: bn_bwd_apply
    _bw("one", _RED + " bn_bwd_apply"),                                  # R = 1: dy cancels exactly, coef = dz
    _bw("c4", _RED + " bn_bwd_apply"),                                   # fewer rows than rows_it
    _bw("c4g3", _RED + " bn_bwd_apply"),                                 # dgamma / dbeta summed over three groups
    _bw("c8g3", _RED + " bn_bwd_apply"),                                 # group boundaries inside block 0 of the apply pass
    _bw("c8g3", _RED + " bn_bwd_apply", data="o"),                       # offset data against the closed form (above)
    _bw("c24", _RED + " bn_bwd_apply"),                                  # R below rows_it at C4 = 6
    _bw("c24g2", _RED + " bn_bwd_apply", data="e"),                      # zero-gradient channel, constant channel; two ragged blocks
    _bw("c24big", _RED + " bn_bwd_apply"),                               # thirteen blocks dealt cyclically, the two-group pass and its tail
    _bw("c72", _RED + " bn_bwd_apply"),                                  # C4 = 18 through the one-wave window with maxima off
    _bw("c72g3", _RED + " bn_bwd_apply"),                                # one block per group, three groups
    _bw("c192g2", _RED + " bn_bwd_apply"),                               # rows_it = 5
    _bw("c512g2", _RED + " bn_bwd_apply", data="e"),                     # owners in two waves
    _bw("c1024", _RED + " bn_bwd_apply"),                                # rows_it = 1
    _bw("c1024g2", _RED + " bn_bwd_apply"),                              # ... two groups
    # three bf16 planes: no maxima, no scale
    _bw("c24g2", _RED + " bn_bwd_apply_split<3>", 3, data="e"),          # planes and fp32 dy bit for bit
    _bw("c72", _RED + " bn_bwd_apply_split<3>[dy=NULL]", 3, fp32=False),     # planes only
    _bw("c8g3", _RED + " bn_bwd_apply_split<3>", 3),                     # C / 8 = 1, three groups
    # two fp16 planes: per-block maxima, the bound, the scale
    _bw("c24g2", _REDM + " bn_bwd_apply_split<2>", 2, data="e"),         # the zero channel's bound is 0
    _bw("c72g3", _REDM + " bn_bwd_apply_split<2>[dy=NULL]", 2, fp32=False),  # planes only; maxima through the one-wave window
    _bw("c192g2", _REDM + " bn_bwd_apply_split<2>", 2, data="d"),        # dz channels 2^0 .. 2^-20 under one tensor scale
    _bw("c24big", _REDM + " bn_bwd_apply_split<2>", 2, data="x"),        # one element 2^12 times the rest: |value / s| <= 2^15
    # one fp16 plane
    _bw("c24g2", _REDM + " bn_bwd_apply_split<1>", 1),                   # group boundary inside a block
    _bw("c512g2", _REDM + " bn_bwd_apply_split<1>[dy=NULL]", 1, fp32=False, data="d"),    # dynamic range on one plane, planes only
    _bw("c8g3", _REDM + " bn_bwd_apply_split<1>", 1, data="x"),          # the outlier on one plane
    # the reduction alone: coef stays at rpnet_bn_bwd_coef_offset
    _bw("c24g2", _RED, data="e", red=True),                              # two groups: coef [2][24][2]
    _bw("c72", _RED, red=True),                                          # C4 = 18
    _bw("clamp", _RED, red=True),                                        # 1024 blocks, each looping over five row groups
]
_REDP, _REDPM = "bn_bwd_partial_pool<64> bn_bwd_finalize", "bn_bwd_partial_pool<64>[pmax] bn_bwd_finalize[pmax]"
BWD_POOL = [
    _bw("pool", _REDP + " bn_bwd_apply_pool_split<3,drain>", 3, data="t", pool=True),             # tied maxima: the first in scan order
    _bw("pool", _REDPM + " bn_bwd_apply_pool_split<2,drain>", 2, data="t", pool=True),            # the same on fp16 planes
    _bw("pool", _REDPM + " bn_bwd_apply_pool_split<1,drain>", 1, data="e", pool=True),            # windows that are negative throughout
    _bw("pool72", _REDPM + " bn_bwd_apply_pool_split<2,drain>", 2, data="t", pool=True),          # C / 8 = 9, Rp = 45 pooled rows
    _bw("pool72", _REDP + " bn_bwd_apply_pool_split<3,drain>[dy=NULL]", 3, fp32=False, pool=True),    # planes only
    _bw("pool2x2", _REDPM + " bn_bwd_apply_pool_split<2,drain>", 2, data="t", pool=True),         # one window per image and group
    _bw("pool2x2", _REDPM + " bn_bwd_apply_pool_split<1,drain>", 1, pool=True),                   # ... untied, one plane
    _bw("pool512", _REDPM + " bn_bwd_apply_pool_split<2,drain>[dy=NULL]", 2, fp32=False, data="d", pool=True),   # Wo = 1, dynamic range
]
# rpnet_bn_bwd on caller-made sums (given_partial / given_pmax / given_rows)
GIVEN = [
    _bw("c24g2", "bn_bwd_finalize[given] bn_bwd_apply", given=1),                                # one row per group
    _bw("c24g2", "bn_bwd_finalize[given] bn_bwd_apply", data="e", given=257),                    # lane 0 reads two rows
    _bw("c72g3", "bn_bwd_finalize[given]", given=257, red=True, no_y=True),                      # y = NULL, no dy: three groups of 257
    _bw("c24g2", "bn_bwd_finalize[given]", given=1, red=True, no_y=True),                        # y = NULL with one row
    _bw("c24g2", "bn_bwd_finalize[given][pmax] bn_bwd_apply_split<1>", 1, data="d", given=257),  # given_pmax on one plane, dynamic range
    _bw("c24g2", "bn_bwd_finalize[given][pmax] bn_bwd_apply_split<2>", 2, data="x", given=1),    # given_pmax carries the outlier
    _bw("c192g2", "bn_bwd_finalize[given][pmax] bn_bwd_apply_split<2>", 2, given=257),           # 257 rows of 192 maxima
]

EVAL_AFFINE = [Case("eval_affine", (1, 1, 1), C, 1, "bn_eval_affine_kernel") for C in (
    4,                                   # four of 128 threads
    72,
    128,                                 # exactly one block
    132,                                 # two blocks, the second ragged
    1024)]
EVAL_RELU = [
    _row("eval_relu", "one", "bn_eval_relu_kernel"),                     # one float4
    _row("eval_relu", "c24", "bn_eval_relu_kernel"),                     # C4 = 6
    _row("eval_relu", "c72", "bn_eval_relu_kernel"),                     # C4 = 18; several blocks race for the absmax
    _row("eval_relu", "c24big", "bn_eval_relu_kernel", data="o"),        # offset data
    _row("eval_relu", "c1024", "bn_eval_relu_kernel"),                   # C4 = 256
]
_ERED, _EREDM = "bn_bwd_partial<64> bn_eval_bwd_finalize", "bn_bwd_partial<64>[pmax] bn_eval_bwd_finalize[pmax]"
EVAL_BWD = [
    _bw("c4", _ERED + " bn_bwd_apply", op="eval_bwd"),                                   # C4 = 1
    _bw("c24g2", _ERED + " bn_bwd_apply", data="e", op="eval_bwd"),                      # two groups of statistics; zero channel
    _bw("c72", _ERED + " bn_bwd_apply", op="eval_bwd"),                                  # C4 = 18
    _bw("c1024", _ERED + " bn_bwd_apply", op="eval_bwd"),                                # rows_it = 1
    _bw("c24g2", _ERED + " bn_bwd_apply_split<3>", 3, op="eval_bwd"),                    # the train-mode apply on zero coefficients
    _bw("c72g3", _EREDM + " bn_bwd_apply_split<2>[dy=NULL]", 2, fp32=False, data="d", op="eval_bwd"),    # bound = |scale| max |dz m|
    _bw("c24g2", _EREDM + " bn_bwd_apply_split<2>", 2, data="x", op="eval_bwd"),         # the outlier sets the scale
    _bw("c8g3", _EREDM + " bn_bwd_apply_split<1>", 1, op="eval_bwd"),                    # one plane, three groups
    _bw("c24g2", _ERED, red=True, op="eval_bwd"),                                        # reduction only: zeros at the coef offset
]

TABLES = {"stats": STATS, "from_partial": FROM_PARTIAL, "relu": RELU, "relu_pool": RELU_POOL, "bwd": BWD, "bwd_pool": BWD_POOL,
          "given": GIVEN, "eval_affine": EVAL_AFFINE, "eval_relu": EVAL_RELU, "eval_bwd": EVAL_BWD}
ALL_ROWS = [c for t in TABLES.values() for c in t]

# every hipLaunchKernelGGL of the default dispatch -> the words of route() that reach it
KERNELS = ["bn_stats_partial<64>", "bn_stats_finalize", "bn_eval_affine_kernel", "bn_relu_kernel", "bn_relu_kernel[s_out]",
           "bn_relu_split_kernel<1>", "bn_relu_split_kernel<2>", "bn_relu_split_kernel<3>", "bn_relu_pool_split_kernel<1,drain>",
           "bn_relu_pool_split_kernel<2,drain>", "bn_relu_pool_split_kernel<3,drain>", "bn_bwd_partial<64>", "bn_bwd_partial<64>[pmax]",
           "bn_bwd_finalize", "bn_bwd_finalize[pmax]", "bn_bwd_finalize[given]", "bn_bwd_finalize[given][pmax]", "bn_bwd_apply",
           "bn_bwd_apply_split<1>", "bn_bwd_apply_split<2>", "bn_bwd_apply_split<3>", "bn_bwd_partial_pool<64>",
           "bn_bwd_partial_pool<64>[pmax]", "bn_bwd_apply_pool_split<1,drain>", "bn_bwd_apply_pool_split<2,drain>",
           "bn_bwd_apply_pool_split<3,drain>", "bn_eval_relu_kernel", "bn_eval_bwd_finalize", "bn_eval_bwd_finalize[pmax]"]


# -------------------------------------------------------------------------------------------------------------------- data
def _seed(c):
    return case_seed(c.N, c.H, c.W, c.C, c.G, sum(map(ord, c.data)))


def make_data(c):
    """-> namespace(y, gamma, beta, dz): fp32 CPU tensors; gamma[1] < 0 in every case"""
    k, C = _seed(c), c.C
    y = rnd(k, c.N, c.H, c.W, C) * 1.3 + 0.2
    gamma, beta = rnd(k + 1, C) * 0.25 + 1.0, rnd(k + 2, C) * 0.3
    gamma[1] = -gamma[1].abs()
    if "o" in c.data:                       # per-channel mean 2^10 times the standard deviation
        sd = 0.5 + rnd(k + 3, C).abs()
        y = rnd(k, c.N, c.H, c.W, C) * sd + 1024.0 * sd
    if "t" in c.data:                       # small integers: equal values inside most windows; one window tied in all four
        y = torch.from_numpy(np.random.RandomState(k + 5).randint(0, 3, tuple(y.shape)).astype(np.float32))
        y[0, :2, :2, :] = 1.0
    if "e" in c.data:
        y[..., 0] = 1.5                     # variance 0: invstd = 1 / sqrt(eps)
        beta[2] = -(gamma[2].abs() * 8.0 + 1.0)           # |xhat| < 8 on these draws: y scale + shift < 0 throughout
    dz = rnd(k + 4, c.N, c.H // 2, c.W // 2, C) if c.pool else rnd(k + 4, c.N, c.H, c.W, C)
    if "d" in c.data:
        dz = dz * torch.exp2(-20.0 * torch.arange(C) / (C - 1)).float()
    if "x" in c.data:
        dz[0, 0, 0, 3] *= 2.0 ** 12
    return types.SimpleNamespace(y=y.contiguous(), gamma=gamma, beta=beta, dz=dz.contiguous())


def stats_of(c, d):
    """the statistics a forward hands the other passes: fp32 [4][G][C] (scale, shift, mean, invstd), rounded from float64"""
    return torch.stack(R.bn_stats(d.y, d.gamma, d.beta, None, None, MOM, EPS, c.G)[:4]).float()


def _pi(v, N):
    return R._per_image(v, N)


# ----------------------------------------------------------------------------------------------------------------- records
class Rec(CC.Rec):
    def line(self):
        return (f"PARITY bn {self.family} {self.what} err={self.err:.3e} yard={self.yard:.3e} ratio={self.ratio:.2f} "
                f"of_bound={self.multiple:.3f}")


def _mine(r):
    r.__class__ = Rec
    return r


def exact(c, what, got, want):
    return _mine(CC.exact(c.id, what, got, want))


def bits_equal(c, what, got, want):
    """bit for bit (NaN equals the same NaN)"""
    v = lambda t: t.contiguous().view(torch.int32 if t.dtype == F32 else t.dtype)         # noqa: E731
    return _mine(CC.exact(c.id, what, v(got), v(want)))


def truth(c, what, ok):
    return Rec(c.id, what, 0 if ok else 1, 0.0, 0.0, exact=True)


def whole(c, what, got, r64, r32, extra=None):
    return _mine(CC.measure(c.id, what + " whole", got, r64, r32, extra=extra))


def per_channel(c, what, got, r64, r32, extra=None, skip=None, zero_below=0.0):
    """the yardstick bound per (group, channel) of an [N, h, w, C] tensor against that channel's own reference maximum: the record
    of the worst channel.  A channel whose reference is all zero must be exactly zero.  skip: elements left out; zero_below: the
    float64 reference's own round-off, below which a channel of it counts as zero (a gradient that cancels exactly, R = 1)"""
    if not torch.isfinite(got).all():
        return Rec(c.id, what + " per channel", math.inf, 0.0, FLOOR)
    C = r64.shape[-1]
    d = (got.double() - r64).abs()
    if extra is not None:
        d = (d - extra).clamp_min(0)
    y = (r32.double() - r64).abs()
    g0 = got.clone()
    if skip is not None:
        d, y, g0 = d.masked_fill(skip, 0), y.masked_fill(skip, 0), g0.masked_fill(skip, 0)
    G = c.G if r64.dim() == 4 else 1
    ref, err, yard = (t.reshape(G, -1, C).amax(1) for t in (r64.abs(), d, y))
    ref = torch.where(ref <= zero_below, torch.zeros_like(ref), ref)
    nz = (g0 != 0).reshape(G, -1, C).sum(1)
    bad = int(nz[ref == 0].sum())
    if bad:
        return Rec(c.id, what + " of an all-zero channel", bad, 0.0, 0.0, exact=True)
    worst = Rec(c.id, what + " per channel", 0.0, 0.0, FLOOR)
    for g, ch in (ref > 0).nonzero().tolist():
        yd = float(yard[g, ch] / ref[g, ch])
        rec = Rec(c.id, f"{what} per channel[g{g} c{ch}]", err[g, ch] / ref[g, ch], yd, FACTOR * yd + FLOOR)
        if rec.multiple > worst.multiple:
            worst = rec
    return worst


def derived(c, what, got, ref, allow):
    """|got - ref| <= allow element by element (float64 tensors): the record of the element that uses most of its allowance,
    err and bound relative to the reference's maximum"""
    got, ref, allow = got.double().reshape(-1), ref.double().reshape(-1), allow.double().reshape(-1)
    if not torch.isfinite(got).all():
        return Rec(c.id, what, math.inf, 0.0, FLOOR)
    d = (got - ref).abs()
    scale = float(ref.abs().max()) or 1.0
    use = torch.where(allow > 0, d / allow.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, math.inf), torch.zeros_like(d)))
    i = int(use.argmax())
    if math.isinf(float(use[i])):
        return Rec(c.id, what + " (no allowance)", math.inf, 0.0, 0.0)
    return Rec(c.id, what, float(d[i]) / scale, 0.0, max(float(allow[i]) / scale, 1e-300))


hold = CC.hold


# -------------------------------------------------------------------------------------------------------- the statistics
def stats_bounds(c, d, rm0, rv0):
    """the references and allowances of the module docstring -> {name: (ref, allow)} (float64)"""
    Rg = c.R
    sc, sh, mu, inv, _, _ = R.bn_stats(d.y, d.gamma, d.beta, None, None, MOM, EPS, c.G)
    yg = d.y.double().reshape(c.G, -1, c.C)
    E = (Rg + 2048) * 2.0 ** -53
    may, var = yg.abs().mean(1), yg.var(1, unbiased=False)
    dvar = 4 * E * ((yg * yg).mean(1) + mu * mu)
    k = dvar / (2 * (var + EPS))
    out = {"mean": (mu, U * mu.abs() + E * may), "invstd": (inv, (U + k) * inv), "scale": (sc, (2 * U + k) * sc.abs()),
           "shift": (sh, (4 * U + k) * (mu * sc).abs() + U * sh.abs() + E * may * sc.abs())}
    rm, rv = rm0.double(), rv0.double()
    am, av = torch.zeros_like(rm), torch.zeros_like(rv)
    for g in range(c.G):
        unb = var[g] * Rg / (Rg - 1) if Rg > 1 else var[g]
        rm1, rv1 = (1 - MOM) * rm + MOM * mu[g], (1 - MOM) * rv + MOM * unb
        am = (1 - MOM) * am + U * (2 * ((1 - MOM) * rm).abs() + 2 * (MOM * mu[g]).abs() + rm1.abs()) + MOM * E * may[g]
        av = (1 - MOM) * av + U * (2 * ((1 - MOM) * rv).abs() + 2 * (MOM * unb).abs() + rv1.abs()) + MOM * dvar[g] * (Rg / (Rg - 1) if Rg > 1 else 1)
        rm, rv = rm1, rv1
    out["running_mean"], out["running_var"] = (rm, am), (rv, av)
    return out


def host_partials(terms, nblk, pad=2):
    """[G, R, C, 2] float64 terms -> [G * nblk + pad, C, 2] partial sums over nblk uneven row ranges per group (some empty when
    nblk > R), formed in float64, and `pad` POISON rows behind them that no launch may read"""
    G, Rg, C, _ = terms.shape
    cuts = [round(i * Rg / nblk) for i in range(nblk + 1)]
    p = torch.stack([terms[:, a:b].sum(1) for a, b in zip(cuts, cuts[1:])], 1).reshape(G * nblk, C, 2)
    return torch.cat([p, torch.full((pad, C, 2), POISON, dtype=F64)]).contiguous()


def check_stats(be, c):
    d = make_data(c)
    k = _seed(c)
    rm0, rv0, nbt0 = rnd(k + 6, c.C) * 0.1, 1.0 + 0.1 * rnd(k + 7, c.C).abs(), 7
    partial = None
    if c.op == "from_partial":
        yg = d.y.double().reshape(c.G, -1, c.C)
        partial = host_partials(torch.stack([yg, yg * yg], -1), c.nblk)
    o = be.stats(c, d, rm0, rv0, nbt0, partial)
    names = ["mean", "invstd", "scale", "shift", "running_mean", "running_var"]
    recs = [derived(c, n, getattr(o, n), *stats_bounds(c, d, rm0, rv0)[n]) for n in names]
    recs.append(exact(c, "num_batches_tracked rises by groups", torch.tensor(o.nbt), torch.tensor(nbt0 + c.G)))
    recs.append(truth(c, "nothing written behind rpnet_bn_workspace_bytes", o.guard_ok))
    again = be.stats(c, d, rm0, rv0, nbt0, partial)
    bare = be.stats(c, d, None, None, None, partial)                # NULL running buffers and a NULL counter are accepted
    for n in names[:4]:
        recs.append(bits_equal(c, f"{n} of a second identical call", getattr(again, n), getattr(o, n)))
        recs.append(bits_equal(c, f"{n} without running buffers", getattr(bare, n), getattr(o, n)))
    return recs


# ------------------------------------------------------------------------------------------------------------ the forward
def act_scale_ok(c, s, bound64):
    """s is pow2_scale of the float64 bound, with or without the library's 1.0001 of slack"""
    return float(s) in (pow2_scale(bound64), pow2_scale(bound64 * SLACK * (1 + 2.0 ** -20)))


def plane_records(c, what, bits, s, out32, r64, r32, bound64, pooled_bits=False, extra=0.0, skip=None):
    """the split output `bits` [planes, ...] (int16) on scale s against the fp32 output of the same launch (None: not written) and
    the references (extra, skip: the activation-mask allowance and the excluded elements of a backward)"""
    p = c.planes
    recs = []
    off = (lambda t: t) if skip is None else (lambda t: t.masked_fill(skip, 0))
    if p == 3:
        vals = plane_values(bits)
        if out32 is not None:
            recs.append(exact(c, f"{what}: three planes sum to the fp32 output", vals.float(), out32))
        else:
            recs.append(whole(c, f"{what} planes", off(vals), off(r64), off(r32), extra=split_unit_roundoff(3) * r64.abs().max() + extra))
        return recs
    recs.append(truth(c, f"{what}: the published scale is pow2_scale of the rigorous bound", act_scale_ok(c, s, bound64)))
    vals = plane_values(bits, float(s))
    rng = float(s) * 2.0 ** 15
    recs.append(truth(c, f"{what}: max |value / s| <= 2^15", bool(torch.isfinite(vals).all()) and float(vals.abs().max()) <= rng
                      and float(r64.abs().max()) <= rng))
    if out32 is not None:
        if pooled_bits:
            recs.append(exact(c, f"{what}: planes are the split of the fp32 output on the same scale", bits, split_planes(out32, p, float(s))))
        recs.append(derived(c, f"{what}: planes against the fp32 output", vals, out32.double(),
                            torch.full_like(vals, split_unit_roundoff(p) * rng)))
    else:
        recs.append(whole(c, f"{what} planes", off(vals), off(r64), off(r32), extra=split_unit_roundoff(p) * rng + extra))
    return recs


def check_relu(be, c):
    d = make_data(c)
    st = stats_of(c, d)
    ref = R.bn_relu_pool if c.pool else R.bn_relu
    r64, r32 = ref(d.y, st[0], st[1], c.G), ref(d.y, st[0], st[1], c.G, F32)
    o = be.relu(c, d, st)
    recs = []
    if c.fp32:
        recs += [per_channel(c, "z", o.z, r64, r32), whole(c, "z", o.z, r64, r32)]
    b64 = float(R.bn_act_bound(d.gamma, d.beta, c.R))
    if c.planes:
        recs += plane_records(c, "z", o.bits, o.s, o.z if c.fp32 else None, r64, r32, b64, pooled_bits=c.pool)
    if c.want_scale:
        recs.append(truth(c, "the published scale is pow2_scale of the rigorous bound", act_scale_ok(c, o.s, b64)))
    again = be.relu(c, d, st)
    if c.fp32:
        recs.append(bits_equal(c, "z of a second identical call", again.z, o.z))
    if c.planes:
        recs.append(exact(c, "planes of a second identical call", again.bits, o.bits))
    return recs


# ----------------------------------------------------------------------------------------------------------- the backward
def _windows(t):
    """[N, H, W, C] -> [N, H/2, W/2, C, 4] in row, column scan order"""
    N, H, W, C = t.shape
    return t.reshape(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(N, H // 2, W // 2, C, 4)


def _pixels(w):
    """the inverse of _windows for a per-window value [N, Ho, Wo, C]: repeated over its four pixels"""
    return w.repeat_interleave(2, 1).repeat_interleave(2, 2)


def excluded(c, d, st):
    """bool [N, H, W, C]: the elements whose ReLU / window decision is inside the fp32 rounding of y scale + shift (module docstring)"""
    y = d.y.double()
    sc, sh = _pi(st[0].double(), c.N), _pi(st[1].double(), c.N)
    a, tol = y * sc + sh, U * ((y * sc).abs() + sh.abs())
    if not c.pool:
        return a.abs() <= tol
    top = _windows(a).topk(2, -1).values
    tw = _windows(tol).amax(-1)
    gap = top[..., 0] - top[..., 1]
    return _pixels((top[..., 0].abs() <= tw) | ((gap > 0) & (gap <= tw)))


def bwd_reference(c, d, st, eval_=False):
    """-> namespace of float64 references, the fp32 yardstick of dy, and the allowances of the module docstring"""
    Rg, G, C, N = c.R, c.G, c.C, c.N
    if eval_:
        dy, dg, db = R.bn_eval_bwd(d.dz, d.y, st, G)
        dy32 = R.bn_eval_bwd(d.dz, d.y, st, G, F32)[0]
        coef = torch.zeros(G, C, 2, dtype=F64)
    elif "o" in c.data:                 # the closed form at the GIVEN statistics (see the comment above BWD)
        assert not c.pool
        (s1, s2), (t1_, t2_) = R.bn_bwd_sums(d.dz, d.y, st, G), R.bn_bwd_sums(d.dz, d.y, st, G, F32)
        coef, coef32 = torch.stack([s1, s2], -1) / Rg, torch.stack([t1_, t2_], -1) / Rg
        dy, dy32 = R.bn_dy(d.dz, d.y, st, coef, G), R.bn_dy(d.dz, d.y, st, coef32, G, F32)
        dg, db = s2.sum(0), s1.sum(0)
    else:
        dy, dg, db, coef = R.bn_bwd(d.dz, d.y, st, G, c.pool)
        dy32 = R.bn_bwd(d.dz, d.y, st, G, c.pool, F32)[0]
    # dz as the full-resolution tensor the sums run over: the pooled gradient on its window's first maximum
    dzf = R.maxpool2_bwd(R.bn_relu(d.y, st[0], st[1], G), d.dz) if c.pool else d.dz.double()
    dm, xh, sc = R._bn_terms(dzf, d.y, st, G, F64)
    ex = excluded(c, d, st)
    dze = (_pixels(d.dz.double().abs()) if c.pool else d.dz.double().abs()) * ex
    per = 4.0 if c.pool else 1.0                                    # a pooled window counts once, not once per pixel
    xw = _pixels(_windows(xh.abs()).amax(-1)) if c.pool else xh.abs()
    grp = lambda t: t.reshape(G, -1, C).sum(1)                      # noqa: E731
    a1, a2 = grp(dze) / per, grp(dze * xw) / per
    t1, t2 = grp(dm.abs()), grp((dm * xh).abs())
    E = (Rg + 2048) * 2.0 ** -53
    al_c1, al_c2 = E * t1 + a1, (2 * U + E) * t2 + a2               # of s1 and s2, before the (float) of the result
    mx = dm.abs().reshape(G, -1, C).amax(1)
    st64 = st.double()
    if eval_:
        bnd = (st64[0].abs() * mx).amax(0)
        extra = sc.abs() * dze
    else:
        s1, s2 = coef[..., 0] * Rg, coef[..., 1] * Rg
        bnd = (st64[0].abs() * (mx + s1.abs() / Rg + s2.abs() / math.sqrt(Rg))).amax(0)
        extra = sc.abs() * (dze + _pi(a1, N) / Rg + xh.abs() * _pi(a2, N) / Rg)
    return types.SimpleNamespace(
        dy=dy, dy32=dy32, dgamma=dg, dbeta=db, coef=coef, ex=ex, extra=extra, bound64=float(bnd.max()),
        noise=2.0 ** -40 * float(st64[0].abs().max() * d.dz.abs().max()),
        al_dbeta=U * db.abs() + al_c1.sum(0), al_dgamma=U * dg.abs() + al_c2.sum(0),
        al_coef=torch.stack([U * coef[..., 0].abs() + al_c1 / Rg, U * coef[..., 1].abs() + al_c2 / Rg], -1),
        terms=torch.stack([dm, dm * xh], -1).reshape(G, -1, C, 2), dmabs=dm.abs().reshape(G, -1, C))


def given_sums(c, ref):
    """caller-made sums of c.given rows per group, formed in float64 (+ POISON rows behind), and their maxima for fp16 planes"""
    partial = host_partials(ref.terms, c.given)
    cuts = [round(i * c.R / c.given) for i in range(c.given + 1)]
    pm = torch.stack([ref.dmabs[:, a:b].amax(1) if b > a else torch.zeros(c.G, c.C, dtype=F64) for a, b in zip(cuts, cuts[1:])], 1)
    pmax = torch.cat([pm.reshape(c.G * c.given, c.C), torch.full((2, c.C), POISON, dtype=F64)]).float().contiguous()
    return partial, (pmax if c.f16 else None)


def check_bwd(be, c):
    eval_ = c.op == "eval_bwd"
    d = make_data(c)
    st = stats_of(c, d)
    ref = bwd_reference(c, d, st, eval_)
    given = given_sums(c, ref) if c.given else None
    k = _seed(c)
    pre_g, pre_b = rnd(k + 8, c.C), rnd(k + 9, c.C)
    run = lambda dd, acc, pg=None, pb=None: be.bwd(c, dd, st, pg, pb, acc, given)        # noqa: E731
    o = run(d, 0)
    recs = [truth(c, "nothing written behind rpnet_bn_workspace_bytes", o.guard_ok),
            truth(c, "excluded share <= EXCLUDED_CAP", float(ref.ex.double().mean()) <= EXCLUDED_CAP),
            derived(c, "dgamma", o.dgamma, ref.dgamma, ref.al_dgamma), derived(c, "dbeta", o.dbeta, ref.dbeta, ref.al_dbeta)]
    if eval_:
        recs.append(exact(c, "coef at rpnet_bn_bwd_coef_offset is zero", o.coef, 0.0))
    else:
        recs.append(derived(c, "coef at rpnet_bn_bwd_coef_offset", o.coef, ref.coef, ref.al_coef))
    if c.fp32 and not c.red:
        recs += [per_channel(c, "dy", o.dy, ref.dy, ref.dy32, ref.extra, skip=ref.ex, zero_below=ref.noise), whole(c, "dy", o.dy.masked_fill(ref.ex, 0),
                 ref.dy.masked_fill(ref.ex, 0), ref.dy32.masked_fill(ref.ex, 0), ref.extra)]
    if c.planes:
        if c.fp32:
            recs += plane_records(c, "dy", o.bits, o.s, o.dy, ref.dy, ref.dy32, ref.bound64, pooled_bits=c.pool)
        else:
            recs += plane_records(c, "dy", o.bits, o.s, None, ref.dy, ref.dy32, ref.bound64, extra=ref.extra, skip=ref.ex)
    # accumulate: onto a pre-fill = pre-fill + the accumulate = 0 result, rounded once; a zero dz returns the pre-fill
    acc = run(d, 1, pre_g, pre_b)
    over = run(d, 0, pre_g, pre_b)
    recs += [bits_equal(c, "dgamma accumulate=0 over a pre-fill", over.dgamma, o.dgamma), bits_equal(c, "dbeta accumulate=0 over a pre-fill", over.dbeta, o.dbeta),
             bits_equal(c, "dgamma accumulate=1", acc.dgamma, pre_g + o.dgamma), bits_equal(c, "dbeta accumulate=1", acc.dbeta, pre_b + o.dbeta)]
    if not c.given:
        zero = types.SimpleNamespace(y=d.y, gamma=d.gamma, beta=d.beta, dz=torch.zeros_like(d.dz))
        z = run(zero, 1, pre_g, pre_b)
        recs += [bits_equal(c, "dgamma accumulate=1 of a zero dz", z.dgamma, pre_g), bits_equal(c, "dbeta accumulate=1 of a zero dz", z.dbeta, pre_b)]
        if c.fp32 and not c.red:
            recs.append(exact(c, "dy of a zero dz", z.dy, 0.0))
    if c.fp32 and not c.red:
        recs.append(bits_equal(c, "dy of a second identical call", over.dy, o.dy))
    if c.planes:
        recs.append(exact(c, "planes of a second identical call", over.bits, o.bits))
    return recs


# ----------------------------------------------------------------------------------------------------------------- eval mode
def check_eval_affine(be, c):
    k = case_seed(c.C, 77)
    gamma, beta, rm, rv = rnd(k, c.C) * 0.25 + 1.0, rnd(k + 1, c.C) * 0.3, rnd(k + 2, c.C), 0.5 + rnd(k + 3, c.C).abs()
    rv[0] = 0.0                                         # scale = gamma / sqrt(eps)
    sc, sh = be.eval_affine(c, gamma, beta, rm, rv)
    r_sc, r_sh = R.bn_eval_affine(gamma, beta, rm, rv, EPS)
    # scale = gamma / sqrtf(rv + eps): the sum, the root, the quotient; shift = beta - rm * scale: the product and the difference
    return [derived(c, "scale", sc, r_sc, 3 * U * r_sc.abs()), derived(c, "shift", sh, r_sh, 4 * U * (rm.double() * r_sc).abs() + U * r_sh.abs())]


def check_eval_relu(be, c):
    d = make_data(c)
    st = stats_of(c, d)[:, 0]                           # one affine pair per channel
    y2 = d.y.reshape(-1, c.C)
    (r64, m64), (r32, _) = R.bn_eval_relu(y2, st[0], st[1]), R.bn_eval_relu(y2, st[0], st[1], F32)
    o = be.eval_relu(c, y2, st[0], st[1], 0.0)
    hi = be.eval_relu(c, y2, st[0], st[1], 1.0e6)       # a running maximum above every z stays
    return [per_channel(c, "z", o.z, r64, r32), whole(c, "z", o.z, r64, r32), exact(c, "absmax is the maximum of the z written", o.absmax, o.z.max().clamp_min(0)),
            derived(c, "absmax", o.absmax, m64, FACTOR * (r32.double() - r64).abs().max() + FLOOR * m64.abs()),
            exact(c, "a larger running absmax stays", hi.absmax, torch.tensor(1.0e6)), bits_equal(c, "z of a second call", hi.z, o.z)]


CHECKS = {"stats": check_stats, "from_partial": check_stats, "relu": check_relu, "bwd": check_bwd, "eval_affine": check_eval_affine,
          "eval_relu": check_eval_relu, "eval_bwd": check_bwd}


def check_row(be, c):
    return CHECKS[c.op](be, c)


# ------------------------------------------------------------------------------------------------------------------ refusals
# (label, entry point, changes to the good call, status).  The good call: N = 4, HW = 16, C = 8, groups = 2, planes = 0.
# Keys: N, HW, C, G, planes, pool_w, null (buffers passed as NULL), ws_short, y_dec, split (a dy_split / z_split buffer is passed),
# given (given_partial passed), rows (given_rows), nblk.  Sizes only, on small buffers: every refusal happens before any launch.
HUGE = dict(N=1 << 15, HW=1 << 15, C=32)                # 2^35 elements: total4 = 2^33, the pooled total8 = 2^30 ... (see POOL_HUGE)
POOL_HUGE = dict(N=1 << 16, HW=1 << 16, C=64, pool_w=256)           # pooled total8 = 2^32 / 4 ... N HW / 4 C / 8 = 2^33
REFUSALS = [
    ("null y", "rpnet_bn_stats", dict(null="y"), ARG), ("null workspace", "rpnet_bn_stats", dict(null="ws"), ARG),
    ("C % 4", "rpnet_bn_stats", dict(C=6), SHAPE), ("C > 1024", "rpnet_bn_stats", dict(C=1028), SHAPE),
    ("N % groups", "rpnet_bn_stats", dict(N=3), SHAPE), ("groups = 0", "rpnet_bn_stats", dict(G=0), SHAPE),
    ("N = 0", "rpnet_bn_stats", dict(N=0), SHAPE), ("HW = 0", "rpnet_bn_stats", dict(HW=0), SHAPE), ("C = 0", "rpnet_bn_stats", dict(C=0), SHAPE),
    ("workspace short", "rpnet_bn_stats", dict(ws_short=1), WORKSPACE),
    ("null partial", "rpnet_bn_stats_from_partial", dict(null="partial"), ARG), ("nblk = 0", "rpnet_bn_stats_from_partial", dict(nblk=0), ARG),
    ("N % groups", "rpnet_bn_stats_from_partial", dict(N=3), SHAPE), ("HW = 0", "rpnet_bn_stats_from_partial", dict(HW=0), SHAPE),
    ("null gamma", "rpnet_bn_eval_affine", dict(null="gamma"), ARG), ("C = 0", "rpnet_bn_eval_affine", dict(C=0), SHAPE),
    ("null y", "rpnet_bn_relu", dict(null="y"), ARG), ("no output", "rpnet_bn_relu", dict(null="z"), ARG),
    ("y_dec", "rpnet_bn_relu", dict(y_dec=1), ARG), ("N = 0", "rpnet_bn_relu", dict(N=0), SHAPE), ("HW = 0", "rpnet_bn_relu", dict(HW=0), SHAPE),
    ("pooled without planes", "rpnet_bn_relu", dict(pool_w=4), ARG), ("pooled C % 8", "rpnet_bn_relu", dict(pool_w=4, split=1, planes=3, C=12), ARG),
    ("pooled odd height", "rpnet_bn_relu", dict(pool_w=4, split=1, planes=3, HW=12), SHAPE),
    ("pooled fp16 planes without gamma", "rpnet_bn_relu", dict(pool_w=4, split=1, planes=2, null="gamma"), ARG),
    ("pooled index limit", "rpnet_bn_relu", dict(split=1, planes=3, **POOL_HUGE), SHAPE),
    ("index limit", "rpnet_bn_relu", dict(**HUGE), SHAPE),
    ("planes = 4", "rpnet_bn_relu", dict(split=1, planes=4), SHAPE), ("split C % 8", "rpnet_bn_relu", dict(split=1, planes=3, C=12), SHAPE),
    ("fp16 planes without the scale", "rpnet_bn_relu", dict(split=1, planes=2, null="s"), ARG),
    ("scale without gamma", "rpnet_bn_relu", dict(null="gamma"), ARG),
    ("y_dec", "rpnet_bn_bwd", dict(y_dec=1), ARG), ("null dz", "rpnet_bn_bwd", dict(null="dz"), ARG),
    ("null y with a dy", "rpnet_bn_bwd", dict(null="y", given=1, rows=1), ARG), ("null y without sums", "rpnet_bn_bwd", dict(null="y,dy"), ARG),
    ("planes = 0", "rpnet_bn_bwd", dict(split=1, planes=0), SHAPE), ("split C % 8", "rpnet_bn_bwd", dict(split=1, planes=3, C=12), SHAPE),
    ("N = 0", "rpnet_bn_bwd", dict(N=0), SHAPE), ("HW = 0", "rpnet_bn_bwd", dict(HW=0), SHAPE), ("workspace short", "rpnet_bn_bwd", dict(ws_short=1), WORKSPACE),
    ("fp16 planes without the scale", "rpnet_bn_bwd", dict(split=1, planes=2, null="s"), ARG),
    ("pooled without planes", "rpnet_bn_bwd", dict(pool_w=4), ARG), ("pooled with given sums", "rpnet_bn_bwd", dict(pool_w=4, split=1, planes=3, given=1, rows=1), ARG),
    ("pooled odd width", "rpnet_bn_bwd", dict(pool_w=3, split=1, planes=3, HW=12), SHAPE),
    ("pooled index limit", "rpnet_bn_bwd", dict(split=1, planes=3, **POOL_HUGE), SHAPE),
    ("given_rows = 0", "rpnet_bn_bwd", dict(given=1, rows=0), ARG), ("fp16 planes without given_pmax", "rpnet_bn_bwd", dict(given=1, rows=1, split=1, planes=2, null="pmax"), ARG),
    ("index limit", "rpnet_bn_bwd", dict(**HUGE), SHAPE),
    ("null y", "rpnet_bn_eval_relu", dict(null="y"), ARG), ("C % 4", "rpnet_bn_eval_relu", dict(C=6), SHAPE), ("C = 0", "rpnet_bn_eval_relu", dict(C=0), SHAPE),
    ("index limit", "rpnet_bn_eval_relu", dict(**HUGE), SHAPE),
    ("null y", "rpnet_bn_eval_bwd", dict(null="y"), ARG), ("planes = 4", "rpnet_bn_eval_bwd", dict(split=1, planes=4), SHAPE),
    ("N % groups", "rpnet_bn_eval_bwd", dict(N=3), SHAPE), ("HW = 0", "rpnet_bn_eval_bwd", dict(HW=0), SHAPE),
    ("workspace short", "rpnet_bn_eval_bwd", dict(ws_short=1), WORKSPACE), ("index limit", "rpnet_bn_eval_bwd", dict(**HUGE), SHAPE),
    ("fp16 planes without the scale", "rpnet_bn_eval_bwd", dict(split=1, planes=1, null="s"), ARG),
]


# -------------------------------------------------------------------------------------------------- the float32 stand-in
DEFECTS = ["fp32_stats", "biased_running", "one_running_update", "group_from_image", "drop_last_rows", "surplus_partial", "mask_from_mean",
           "ignore_accumulate", "eval_coef_stale", "pool_last_max", "scale_from_max", "ignore_given_rows"]


def _f(v):
    return torch.tensor(v, dtype=F32)


class SimBackend:
    """the entry points in float32 torch operators with the library's split: per-block partial sums and a finalize in float64 over
    fp32 terms, every other operation in fp32.  defect: one of DEFECTS (None: a correct implementation)"""

    def __init__(self, defect=None):
        assert defect is None or defect in DEFECTS
        self.defect = defect

    # partial [G, nblk, C, K] of [G, R, C, K] terms over the block ranges of bn_geom, then the finalize's sum over the blocks
    def _reduce(self, terms, C):
        G, Rg = terms.shape[:2]
        _, rows_it, nblk, rows_blk = geom(Rg, C)
        if self.defect == "drop_last_rows" and Rg > 4 * rows_it:
            terms = terms[:, :Rg - Rg % (4 * rows_it)]
        if self.defect == "fp32_stats":
            return terms.float().sum(1).double()
        part = torch.stack([terms[:, b * rows_blk:(b + 1) * rows_blk].double().sum(1) for b in range(nblk)], 1)
        return self._finalize(part.reshape(G * nblk, *terms.shape[2:]), G, nblk)

    def _finalize(self, partial, G, nblk):
        """rows g nblk + b, b < nblk, of the flat partial buffer (a read behind its end lands on the last row)"""
        n, last = nblk + (self.defect == "surplus_partial"), partial.shape[0] - 1
        rows = [partial[min(g * nblk + b, last)] for g in range(G) for b in range(n)]
        return torch.stack(rows).reshape(G, n, *partial.shape[1:]).sum(1)

    def stats(self, c, d, rm0, rv0, nbt0, partial=None):
        G, C, Rg = c.G, c.C, c.R
        if partial is None:
            yg = d.y.reshape(G, -1, C)
            sq = self._reduce(torch.stack([yg.double(), yg.double() * yg.double()], -1) if self.defect != "fp32_stats"
                              else torch.stack([yg, yg * yg], -1), C)
        else:
            sq = self._finalize(partial, G, c.nblk)
        m = sq[..., 0] / Rg
        var = (sq[..., 1] / Rg - m * m).clamp_min(0)
        istd = (1.0 / (var + EPS).sqrt()).float()
        sc = d.gamma[None] * istd
        mf = m.float()
        sh = d.beta[None] - mf * sc
        rm, rv = (None if rm0 is None else rm0.clone()), (None if rv0 is None else rv0.clone())
        mom = _f(MOM)
        groups = [G - 1] if self.defect == "one_running_update" else range(G)
        for g in groups:
            unb = (var[g] if self.defect == "biased_running" or Rg <= 1 else var[g] * Rg / (Rg - 1)).float()
            if rm is not None:
                rm = (1 - mom) * rm + mom * mf[g]
            if rv is not None:
                rv = (1 - mom) * rv + mom * unb
        return types.SimpleNamespace(scale=sc, shift=sh, mean=mf, invstd=istd, running_mean=rm, running_var=rv,
                                     nbt=None if nbt0 is None else nbt0 + G, guard_ok=True)

    def _group(self, c):
        n = torch.arange(c.N)
        return n % c.G if self.defect == "group_from_image" else n // (c.N // c.G)

    def _affine(self, c, y, st):
        g = self._group(c)
        return y * st[0][g][:, None, None] + st[1][g][:, None, None]

    def _act_scale(self, c, d, z):
        if self.defect == "scale_from_max":
            return pow2_scale(float(z.abs().max()))
        sqrt_n = _f(math.sqrt(c.R)) * _f(SLACK)
        return pow2_scale(float((d.gamma.abs() * sqrt_n + d.beta.abs()).max()))

    def relu(self, c, d, st):
        z = torch.relu(self._affine(c, d.y, st))
        if c.pool:
            z = R._nhwc(F.max_pool2d(z.permute(0, 3, 1, 2), 2, 2))
        s = self._act_scale(c, d, z) if (c.f16 or c.want_scale) else None
        bits = split_planes(z, c.planes, s) if c.planes else None
        return types.SimpleNamespace(z=z if c.fp32 else None, bits=bits, s=s)

    def bwd(self, c, d, st, pre_g, pre_b, accumulate, given=None):
        G, C, Rg, N = c.G, c.C, c.R, c.N
        eval_ = c.op == "eval_bwd"
        g = self._group(c)
        e = lambda i: st[i][g][:, None, None]                       # noqa: E731
        dm = xh = None
        if not c.no_y:
            a = self._affine(c, d.y, st)
            xh = (d.y - e(2)) * e(3)
            if c.pool:
                w = _windows(a)
                q = (3 - w.flip(-1).argmax(-1)) if self.defect == "pool_last_max" else w.argmax(-1)
                best = w.gather(-1, q[..., None])[..., 0]
                hit = F.one_hot(q, 4).bool() & (best > 0)[..., None]
                dmw = torch.where(hit, d.dz[..., None], torch.zeros(()))
                Ho, Wo = c.H // 2, c.W // 2
                dm = dmw.reshape(N, Ho, Wo, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(N, c.H, c.W, C)
            else:
                mask = (d.y > e(2)) if self.defect == "mask_from_mean" else (a > 0)
                dm = torch.where(mask, d.dz, torch.zeros(()))
        if given is not None:
            rows = geom(Rg, C)[2] if self.defect == "ignore_given_rows" else c.given
            s = self._finalize(given[0], G, rows)
            mx = None if given[1] is None else torch.stack([given[1][min(gg * rows + b, given[1].shape[0] - 1)] for gg in range(G) for b in range(rows)]).reshape(G, rows, C).amax(1)
        else:
            s = self._reduce(torch.stack([dm.double(), dm.double() * xh.double()], -1).reshape(G, -1, C, 2), C)
            mx = dm.abs().reshape(G, -1, C).amax(1)
        s1, s2 = s[..., 0], s[..., 1]
        train_coef = torch.stack([(s1 / Rg).float(), (s2 / Rg).float()], -1)
        coef = train_coef if (not eval_ or self.defect == "eval_coef_stale") else torch.zeros(G, C, 2)
        dg, db = s2.sum(0).float(), s1.sum(0).float()
        if accumulate and self.defect != "ignore_accumulate":
            dg, db = pre_g + dg, pre_b + db
        out = types.SimpleNamespace(dy=None, bits=None, s=None, dgamma=dg, dbeta=db, coef=coef, guard_ok=True)
        if c.red:
            return out
        use = torch.zeros(G, C, 2) if eval_ else train_coef
        dy = e(0) * (dm - use[..., 0][g][:, None, None] - xh * use[..., 1][g][:, None, None])
        if c.f16:
            if self.defect == "scale_from_max":
                out.s = pow2_scale(float(dy.abs().max()))
            else:
                bnd = (st[0].abs() * (mx.float() if eval_ else mx.float() + (s1.abs() / Rg).float() + (s2.abs() / math.sqrt(Rg)).float())).amax(0) * _f(SLACK)
                out.s = pow2_scale(float(bnd.max()))
        if c.planes:
            out.bits = split_planes(dy, c.planes, out.s)
        out.dy = dy if c.fp32 else None
        return out

    def eval_affine(self, c, gamma, beta, rm, rv):
        sc = gamma / (rv + _f(EPS)).sqrt()
        return sc, beta - rm * sc

    def eval_relu(self, c, y2, scale, shift, absmax0):
        z = torch.relu(y2 * scale + shift)
        return types.SimpleNamespace(z=z, absmax=torch.maximum(z.max().clamp_min(0), _f(absmax0)))
