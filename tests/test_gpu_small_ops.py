"""GPU parity of the small kernels around the convolutions — matcher, loss, pooling, the separate entry points behind the
fused refinement glue — at the edges of their dispatch: every kernel through the C ABI directly (rpnet_amd.hip.call, not the
autograd Functions, so that the flags the Functions never set are exercised too) against the plain float64 references of
tests/ref64.py.

Tolerances are measured, not chosen.  Selection operations (max-pool, arg-max, labels, hard masks) are compared with
torch.equal on inputs built away from their decision boundaries.  Arithmetic results are held to a yardstick: the same ref64
function evaluated in float32 on the CPU gives yard = rel_err(r32, r64), and the kernel must meet
rel_err(hip, r64) <= 8 * yard + 4 * 2^-24 (the floor: four fp32 unit round-offs of the largest reference value, for outputs
whose yardstick comes out as exactly 0; the factor: summation order — these kernels add up to 64 terms in sequence where torch
adds pairwise).  Every check prints `PARITY family what err yard ratio`; profiles/small_ops_parity.txt keeps each family's
largest ratio."""
import numpy as np
import pytest
import torch

from tests import ref64 as R
from tests.helpers import rel_err, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 4 * 2.0 ** -24
SHAPE, ARG, WORKSPACE = -1, -2, -3          # enum rpnet_status of include/rpnet_abi.h


@pytest.fixture(scope="module")
def hip():
    from rpnet_amd import hip
    hip.load()
    return hip


_ALIVE = []


@pytest.fixture(autouse=True)
def _device_copies_live_until_the_test_ends():
    yield
    _ALIVE.clear()


def dv(t):
    """device copy, referenced until the test ends: a temporary whose pointer went into a call must not be freed (and its
    memory handed to the next temporary of the same argument list) before the launch"""
    _ALIVE.append(t.to(DEV).contiguous())
    return _ALIVE[-1]


def zeros(*shape, dtype=torch.float32):
    return torch.zeros(shape, device=DEV, dtype=dtype)


def ws_for(nbytes):
    return torch.empty(max(int(nbytes), 16), device=DEV, dtype=torch.uint8)


def hold(family, what, got, r64, r32, factor=8.0):
    """the yardstick bound of the module docstring"""
    yard, err = rel_err(r32, r64), rel_err(got, r64)
    print(f"PARITY {family} {what} err={err:.3e} yard={yard:.3e} ratio={err / yard if yard > 0 else 0.0:.2f}")
    assert torch.isfinite(torch.as_tensor(got)).all(), f"{family} {what}: not finite"
    assert err <= factor * yard + FLOOR, f"{family} {what}: rel err {err:.3e} > {factor} x {yard:.3e} + {FLOOR:.1e}"


def both(fn, *args, **kw):
    return fn(*args, **kw), fn(*args, dtype=torch.float32, **kw)


def rc_of(hip, name, *args):
    """return code of an entry point that is expected to refuse on the host, before any launch"""
    return getattr(hip.load(), name)(*[hip.ptr(a) if torch.is_tensor(a) else a for a in args], hip.stream())


# ============================================================================ cosine match
COSINE_ROWS = [
    # B, K, C, hw, accumulate_df, zero rows
    (1, 1, 4, 1, 0, False),        # L = 1 instantiation, one pixel, one prototype: a single live thread
    (3, 2, 8, 35, 1, False),       # L = 2; hw below one block of pixels; df accumulated onto a prefill
    (1, 3, 16, 63, 0, False),      # L = 4; hw one short of the 64 pixels per block
    (4, 4, 32, 64, 1, False),      # L = 8; K = 4 fills every prototype register; hw exactly one 64-pixel chunk
    (1, 2, 64, 4096, 0, False),    # L = 16; nblk = 64 partial rows in the backward
    (3, 4, 128, 35, 0, False),     # L = 32; 8 pixels per block, grid-stride in the backward's single block
    (1, 4, 256, 1, 0, False),      # L = 64: a whole wave per pixel, hw = 1
    (1, 2, 256, 6000, 1, False),   # past 1024 blocks x 4 pixels: the forward's grid-stride loop wraps
    (4, 2, 64, 16384, 0, False),   # the 512^2 shape: nblk = 256
    (70, 3, 8, 2304, 0, False),    # B = 70: 2048 / B < 32, the floor of 32 blocks in cos_blocks
    (1, 2, 4, 4096, 0, False),     # dproto through cosine_dproto_final at C = 4: 64 parts share the partial rows
    (1, 3, 256, 4096, 1, False),   # dproto through cosine_dproto_final at C = 256: one part
    (3, 1, 64, 63, 1, False),      # K = 1 with accumulate
    (2, 2, 64, 35, 0, True),       # a zero feature vector and a zero prototype
    (2, 3, 16, 64, 1, True),       # the same with K = 3, L = 4 and accumulate
]


@pytest.mark.parametrize("B,K,C,hw,acc,zero", COSINE_ROWS)
def test_cosine_match(hip, B, K, C, hw, acc, zero):
    seed = 1000 + 7 * C + hw % 97 + K
    f, p, dpred = rnd(seed, B, hw, C), rnd(seed + 1, B, K, C), rnd(seed + 2, B, K, hw)
    if zero:
        f[0, 0] = 0             # zero feature vector
        p[1, 0] = 0             # zero prototype
    scaler = 20.0
    fd, pd = dv(f), dv(p)
    pred = zeros(B, K, hw)
    hip.call("rpnet_cosine_match_fwd", hip.ptr(fd), hip.ptr(pd), hip.ptr(pred), B, K, hw, C, scaler)
    r64, r32 = both(R.cosine_match, f, p, scaler)
    hold("cosine", "pred", pred, r64, r32)
    pre = rnd(seed + 3, B, hw, C)
    df = dv(pre) if acc else torch.full((B, hw, C), float("nan"), device=DEV)
    dproto = torch.full((B, K, C), float("nan"), device=DEV)
    wb = hip.query("rpnet_cosine_match_bwd_workspace_bytes", B, K, hw, C)
    ws = ws_for(wb)
    hip.call("rpnet_cosine_match_bwd", hip.ptr(fd), hip.ptr(pd), hip.ptr(dv(dpred)), hip.ptr(df), hip.ptr(dproto), B, K, hw, C,
             scaler, acc, hip.ptr(ws), wb)
    (g64, q64), (g32, q32) = both(R.cosine_match_bwd, f, p, dpred, scaler)
    df, dproto = df.cpu(), dproto.cpu()
    if zero:
        assert pred[0, :, 0].abs().max() == 0 and pred[1, 0].abs().max() == 0          # forward exactly 0 there
        assert torch.isfinite(df).all() and torch.isfinite(dproto).all()
        # the reference's gradient of a zero vector is 1/eps-scaled: those two rows, and nothing else, stay out
        for t in (df, g64, g32):
            t[0, 0] = 0
        for t in (dproto, q64, q32):
            t[1, 0] = 0
        if acc:
            pre[0, 0] = 0
    if acc:
        g64, g32 = g64 + pre.double(), g32 + pre
    hold("cosine", "df", df, g64, g32)
    # C = 4 (L = 1): a block has 256 one-lane pixel groups and thread 0 adds their 256 partial rows IN SEQUENCE in LDS (the loop over
    # gidx in cosine_match_bwd_kernel); a sequential fp32 sum of n terms drifts like sqrt(n) round-offs where torch's pairwise sum
    # stays near sqrt(log n): 16 against ~3 here, every other C adds at most 128 rows.  Measured 10.5 yardsticks on the MI355X at
    # (B, K, C, hw) = (1, 2, 4, 4096); this one check gets twice that
    hold("cosine", "dproto", dproto, q64, q32, factor=21.0 if C == 4 else 8.0)


# ========================================================================== masked pooling
def make_masks(seed, kinds, B, H, W):
    g = torch.Generator().manual_seed(seed)
    out = []
    for kind in kinds:
        if kind == "binary":
            out.append((torch.rand(B, H, W, generator=g) > 0.5).float())
        elif kind == "soft":
            out.append(torch.rand(B, H, W, generator=g))
        elif kind == "empty":
            out.append(torch.zeros(B, H, W))
        else:
            out.append(torch.ones(B, H, W))
    return torch.stack(out, 0)          # [nmask, B, H, W]


POOL_ROWS = [
    # B, C, (H, W), (h, w), mask kinds, accumulate
    (1, 4, (5, 7), (5, 7), ("binary",), 0),                           # ratio 1; H W % 4 != 0: the scalar path of mask_sum_kernel; hw = 35 < 64 chunks
    (2, 8, (10, 26), (5, 13), ("soft", "binary"), 1),                 # ratio 2; hw = 65: chunks of 2 pixels, the last 31 chunks empty
    (1, 64, (32, 32), (8, 8), ("binary", "empty", "ones"), 0),        # ratio 4; hw = 64: one pixel per chunk; empty and all-ones masks
    (2, 256, (64, 64), (8, 8), ("soft", "ones", "binary", "empty"), 1),   # ratio 8; nmask = 4; C = 256: 4 pixel rows per block
    (1, 1024, (12, 16), (6, 4), ("binary", "soft"), 0),               # anisotropic (/2, /4); C = 1024: one row per block, no LDS partner
    (3, 4, (20, 28), (5, 7), ("soft", "empty", "binary", "ones"), 1),  # C = 4: 256 pixel rows per block, most idle at hw = 35
    (2, 8, (7, 9), (7, 9), ("soft", "binary", "ones"), 0),            # ratio 1, nmask = 3, odd H W = 63: scalar mask sums
    (1, 64, (48, 40), (6, 5), ("ones",), 1),                          # ratio 8 on a non-square map, hw = 30, nmask = 1
    (4, 256, (16, 16), (8, 8), ("binary", "soft"), 0),                # ratio 2 at C = 256
    (1, 8, (13, 5), (13, 5), ("empty", "soft"), 0),                   # hw = 65 the other way round, ratio 1, H W = 65 scalar path
    (2, 1024, (8, 8), (2, 2), ("binary", "ones", "soft", "soft"), 1),  # hw = 4, nmask = 4 at C = 1024
    (2, 64, (64, 64), (16, 16), ("binary", "soft", "empty"), 1),      # hw = 256: 4 pixels per chunk, accumulate
    (1, 4, (8, 8), (1, 1), ("soft", "binary"), 0),                    # a single low-resolution pixel: every tap clamps
    (3, 64, (24, 20), (6, 5), ("binary", "binary", "binary", "soft"), 0),  # the golden vector's geometry at nmask = 4, B = 3
    (8, 64, (256, 256), (64, 64), ("binary", "soft"), 0),             # the production shape: B = 8, 256^2 -> 64^2, C = 64
]


@pytest.mark.parametrize("B,C,HW,hw_,kinds,acc", POOL_ROWS)
def test_masked_pool(hip, B, C, HW, hw_, kinds, acc):
    (H, W), (h, w), nmask = HW, hw_, len(kinds)
    seed = 2000 + C + H * 3 + w
    masks = make_masks(seed, kinds, B, H, W)
    f, dproto = rnd(seed + 1, B, h * w, C), rnd(seed + 2, B, nmask, C)
    md, fd = dv(masks), dv(f)
    am, msum = torch.full((B, nmask, h * w), float("nan"), device=DEV), torch.full((B, nmask), float("nan"), device=DEV)
    hip.call("rpnet_mask_adjoint", hip.ptr(md), hip.ptr(am), hip.ptr(msum), B, nmask, H, W, h, w)
    (am64, ms64), (am32, ms32) = both(R.mask_adjoint, masks, h, w)
    hold("masked_pool", "am", am, am64, am32)
    hold("masked_pool", "msum", msum, ms64, ms32)
    proto = torch.full((B, nmask, C), float("nan"), device=DEV)
    wb = hip.query("rpnet_masked_pool_workspace_bytes", B, nmask, h * w, C)
    ws = ws_for(wb)
    hip.call("rpnet_masked_pool_fwd", hip.ptr(fd), hip.ptr(am), hip.ptr(msum), hip.ptr(proto), B, nmask, h * w, C, hip.ptr(ws), wb)
    r64, r32 = both(R.masked_pool, f, masks, h, w)           # the as-written form: the adjoint formulation itself is under test
    hold("masked_pool", "proto", proto, r64, r32)
    for k, kind in enumerate(kinds):
        if kind == "empty":
            assert proto[:, k].abs().max() == 0 and am[:, k].abs().max() == 0 and msum[:, k].abs().max() == 0
        if kind == "ones":
            assert torch.equal(msum[:, k].cpu(), torch.full((B,), float(H * W)))
    pre = rnd(seed + 3, B, h * w, C)
    df = dv(pre) if acc else torch.full((B, h * w, C), float("nan"), device=DEV)
    hip.call("rpnet_masked_pool_bwd", hip.ptr(dv(dproto)), hip.ptr(am), hip.ptr(msum), hip.ptr(df), B, nmask, h * w, C, acc)
    g64, g32 = both(R.masked_pool_bwd, f, masks, h, w, dproto)
    if acc:
        g64, g32 = g64 + pre.double(), g32 + pre
    hold("masked_pool", "df", df, g64, g32)


# ================================================================================= bilinear
BILINEAR_ROWS = [
    # planes, (h, w), (H, W)
    (1, (4, 4), (4, 4)),          # ratio 1: every second weight is exactly 0
    (24, (8, 6), (16, 12)),       # ratio 2, 24 planes
    (1, (8, 8), (32, 32)),        # ratio 4, one plane (the model's logits)
    (24, (4, 4), (32, 32)),       # ratio 8
    (3, (5, 7), (10, 28)),        # anisotropic (x2, x4); planes h w = 105 is no multiple of 64: `live` beside the 4-lane shuffle
    (1, (1, 1), (4, 4)),          # h = w = 1: both taps clamp onto the one source pixel
    (2, (1, 6), (2, 12)),         # h = 1 alone
    (24, (6, 1), (12, 4)),        # w = 1 alone
    (1, (16, 16), (128, 128)),    # ratio 8 with a window of 26 rows in the backward
    (24, (3, 5), (24, 10)),       # anisotropic the other way (x8, x2), planes h w = 360
    (1, (64, 64), (256, 256)),    # the production shape of one plane
    (5, (7, 3), (7, 3)),          # ratio 1 on odd extents
    (2, (2, 2), (16, 16)),        # ratio 8 where every source pixel is a border pixel
    (24, (16, 12), (64, 48)),     # ratio 4, 24 planes
    (1, (1, 1), (1, 1)),          # a single pixel in, a single pixel out
]


@pytest.mark.parametrize("planes,lo,hi", BILINEAR_ROWS)
def test_bilinear(hip, planes, lo, hi):
    (h, w), (H, W) = lo, hi
    x, dout = rnd(3000 + planes + h * 5 + W, planes, h, w), rnd(3001 + planes + h * 5 + W, planes, H, W)
    out = torch.full((planes, H, W), float("nan"), device=DEV)
    hip.call("rpnet_bilinear_up_fwd", hip.ptr(dv(x)), hip.ptr(out), planes, h, w, H, W)
    hold("bilinear", "up", out, *both(R.bilinear_up, x, H, W))
    din = torch.full((planes, h, w), float("nan"), device=DEV)
    hip.call("rpnet_bilinear_up_bwd", hip.ptr(dv(dout)), hip.ptr(din), planes, h, w, H, W)
    hold("bilinear", "adjoint", din, *both(R.bilinear_up_bwd, dout, h, w))


def test_bilinear_forward_takes_a_ratio_that_is_no_integer(hip):
    """5 -> 12: the forward launcher accepts it (only the adjoint asks for whole ratios), so it has to be F.interpolate(size=...)"""
    planes, h, w, H, W = 3, 5, 5, 12, 12
    x = rnd(3100, planes, h, w)
    out = torch.full((planes, H, W), float("nan"), device=DEV)
    hip.call("rpnet_bilinear_up_fwd", hip.ptr(dv(x)), hip.ptr(out), planes, h, w, H, W)
    hold("bilinear", "up_5_to_12", out, *both(R.bilinear_up, x, H, W))


# ============================================================== softmax / threshold / pool
SOFTMAX_ROWS = [
    # B, K, H, W, scale
    (2, 2, 16, 24, 1),      # scale 1: the pool is the identity
    (2, 3, 16, 24, 1),      # K = 3 at scale 1
    (1, 4, 8, 12, 1),       # K = 4 at scale 1
    (2, 2, 16, 24, 2),      # scale 2, generic kernel
    (1, 3, 4, 6, 2),        # W % 4 != 0 at scale 2
    (3, 4, 8, 10, 2),       # K = 4, W % 4 != 0 at scale 2
    (2, 2, 16, 24, 4),      # scale 4, K = 2: the 16-byte-load kernel
    (3, 3, 32, 16, 4),      # scale 4, K = 3: the 16-byte-load kernel
    (2, 4, 16, 24, 4),      # scale 4, K = 4: no vector instantiation, generic kernel
    (1, 2, 32, 48, 8),      # scale 8
    (2, 3, 16, 16, 8),      # K = 3 at scale 8
    (1, 4, 24, 8, 8),       # K = 4 at scale 8: one output column
    (2, 2, 256, 256, 4),    # the production shape of the fed-back mask
    (5, 3, 12, 20, 4),      # scale 4, B h w = 75: a partly filled block
    (1, 2, 4, 4, 4),        # one output pixel
]


def decided_logits(seed, B, K, H, W):
    """Logits whose class-1 probability is away from 0.5 everywhere: l1 = logsumexp(others) + m, |m| >= 0.01 — the boundary of
    softmax[1] > 0.5 itself (at K = 2 that is `class 1 against the largest other class`), four orders above fp32 round-off, so
    fp32 and fp64 cannot disagree.  Rows 0 - 1 of image 0 at K = 2 are exact ties (equal logits): the comparison is strict, so 0."""
    lg = (rnd(seed, B, K, H, W) * 3).double()
    m = rnd(seed + 1, B, H, W).double()
    m = torch.where(m >= 0, m + 0.01, m - 0.01)
    others = torch.cat([lg[:, :1], lg[:, 2:]], 1)
    lg[:, 1] = torch.logsumexp(others, 1) + m
    lg = lg.float()
    if K == 2:
        lg[0, 1, :2] = lg[0, 0, :2]
    return lg


def run_stp(hip, lg_dev, B, K, H, W, scale, soft):
    out = torch.full((B, H // scale, W // scale), float("nan"), device=DEV)
    hip.call("rpnet_softmax_thresh_pool", hip.ptr(lg_dev), hip.ptr(out), B, K, H, W, scale, soft)
    return out


def misaligned(t):
    """the same values behind a pointer that is offset by one float from a 16-byte boundary"""
    buf = torch.empty(t.numel() + 4, device=DEV, dtype=torch.float32)
    off = 1 + (-(buf.data_ptr() // 4)) % 4          # element offset with (ptr / 4) % 4 == 1
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    _ALIVE.append(v)
    return v


@pytest.mark.parametrize("B,K,H,W,scale", SOFTMAX_ROWS)
def test_softmax_thresh_pool(hip, B, K, H, W, scale):
    seed = 4000 + 11 * K + scale + W
    # hard masks: exact, no pixel left out
    lg = decided_logits(seed, B, K, H, W)
    h64, h32 = both(R.softmax_thresh_pool, lg, scale, False)
    assert torch.equal(h64.float(), h32)                          # the inputs are decided in both precisions
    if K == 2 and scale <= 2:
        assert h64[0, :2 // scale].abs().max() == 0              # the tie rows count nothing
    lgd = dv(lg)
    assert lgd.data_ptr() % 16 == 0
    hard = run_stp(hip, lgd, B, K, H, W, scale, 0)
    assert torch.equal(hard.cpu().double() * scale ** 2, h64 * scale ** 2)
    hard_off = run_stp(hip, misaligned(lgd), B, K, H, W, scale, 0)       # generic kernel whatever the shape
    assert torch.equal(hard_off, hard)
    # soft masks
    lgs = rnd(seed + 2, B, K, H, W) * 2
    soft = run_stp(hip, dv(lgs), B, K, H, W, scale, 1)
    hold("softmax", "soft_mask", soft, *both(R.softmax_thresh_pool, lgs, scale, True))
    assert torch.equal(run_stp(hip, misaligned(dv(lgs)), B, K, H, W, scale, 1), soft)
    # logits of +-80: nothing overflows
    big = torch.where(rnd(seed + 3, B, K, H, W) > 0, 80.0, -80.0)
    sb = run_stp(hip, dv(big), B, K, H, W, scale, 1)
    assert torch.isfinite(sb).all()
    hold("softmax", "soft_mask_pm80", sb, *both(R.softmax_thresh_pool, big, scale, True))
    # backward of the soft mask
    dmask = rnd(seed + 4, B, H // scale, W // scale)
    dl = torch.full((B, K, H, W), float("nan"), device=DEV)
    hip.call("rpnet_softmax_pool_bwd", hip.ptr(dv(lgs)), hip.ptr(dv(dmask)), hip.ptr(dl), B, K, H, W, scale)
    hold("softmax", "dlogits", dl, *both(R.softmax_pool_bwd, lgs, dmask, scale))
    hip.call("rpnet_softmax_pool_bwd", hip.ptr(dv(big)), hip.ptr(dv(dmask)), hip.ptr(dl), B, K, H, W, scale)
    assert torch.isfinite(dl).all()
    hold("softmax", "dlogits_pm80", dl, *both(R.softmax_pool_bwd, big, dmask, scale))
    # avg_pool2d of a given mask
    mk = torch.rand(B, H, W, generator=torch.Generator().manual_seed(seed))
    mo = torch.full((B, H // scale, W // scale), float("nan"), device=DEV)
    hip.call("rpnet_mask_avgpool", hip.ptr(dv(mk)), hip.ptr(mo), B, H, W, scale)
    hold("softmax", "mask_avgpool", mo, *both(R.mask_avgpool, mk, scale))


def test_softmax_tie_block_counts_nothing(hip):
    """equal logits at K = 2: softmax[1] is exactly 0.5, the reference's comparison is strict -> 0, at every scale"""
    for scale in (1, 2, 4, 8):
        lg = torch.zeros(1, 2, 8, 8)
        lg[:, :, :, 4:] = rnd(4100, 1, 1, 8, 4)          # both classes get the same values
        ref = R.softmax_thresh_pool(lg, scale, False)
        assert ref.abs().max() == 0
        assert run_stp(hip, dv(lg), 1, 2, 8, 8, scale, 0).abs().max() == 0


# ===================================================================================== loss
LOSS_ROWS = [
    # B, K, H, W, with_dice, ignore_index, per_sample, sample_weight, accumulate, gscale, absent class
    (1, 2, 7, 5, 1, -1, 0, None, 0, 1.0, None),          # the smallest: 35 pixels, 63 of the 64 partial blocks idle
    (3, 3, 24, 20, 1, -1, 0, None, 1, 0.37, None),       # K = 3, accumulate, gscale != 1
    (8, 4, 24, 20, 1, -1, 0, None, 0, 2.5, 2),           # K = 4, B = 8, class 2 absent from the labels
    (3, 2, 24, 20, 0, 255, 1, "zero", 0, 1.7, None),     # the align-loss form: CE only, a quarter ignored, per sample, one weight 0
    (3, 2, 7, 5, 0, 255, 1, "ones", 1, 0.5, None),       # the same with all-ones weights and accumulate
    (8, 2, 24, 20, 0, 255, 1, None, 0, 1.0, None),       # per sample without a weight tensor, B = 8
    (3, 3, 24, 20, 0, 255, 0, None, 0, 1.0, None),       # ignore_index with the batch-wide mean
    (3, 4, 7, 5, 0, -1, 1, None, 1, 3.0, 0),             # per sample, nothing ignored, class 0 absent
    (3, 2, 24, 20, 1, -1, 1, "zero", 0, 1.0, None),      # Dice on top of the per-sample cross-entropy
    (1, 3, 24, 20, 0, -1, 0, None, 0, 1.0, 1),           # with_dice = 0 alone, class 1 absent
    (8, 3, 7, 5, 1, -1, 0, None, 1, 0.25, None),         # B = 8 on the small image
    (1, 4, 7, 5, 1, -1, 0, None, 0, 1.0, 3),             # K = 4, B = 1, the last class absent
    (1, 2, 512, 512, 1, -1, 0, None, 0, 1.0, None),      # 512 x 512 wraps the 64 x 256 grid of the partial sums
    (3, 2, 512, 512, 0, 255, 1, "zero", 1, 0.8, None),   # the align-loss form at 512 x 512 with accumulate
    (8, 4, 512, 512, 1, -1, 0, None, 0, 1.3, None),      # the largest: dice at 8 x 4 x 512^2
]


@pytest.mark.parametrize("B,K,H,W,with_dice,ign,per_sample,sw,acc,gscale,absent", LOSS_ROWS)
def test_dice_ce(hip, B, K, H, W, with_dice, ign, per_sample, sw, acc, gscale, absent):
    seed = 5000 + B * 13 + K * 5 + H
    rs = np.random.RandomState(seed)
    logits = rnd(seed, B, K, H, W) * 2
    classes = [k for k in range(K) if k != absent]
    labels = torch.from_numpy(np.asarray(classes)[rs.randint(0, len(classes), (B, H, W))]).long()
    if ign >= 0:
        labels[torch.from_numpy(rs.rand(B, H, W) < 0.25)] = ign              # about a quarter of the pixels ignored
    weight = None if sw is None else torch.ones(B)
    if sw == "zero":
        weight[1] = 0.0
    kw = dict(with_dice=with_dice, ignore_index=ign, per_sample=per_sample, sample_weight=weight)
    ld, lb = dv(logits), dv(labels)
    wd = None if weight is None else dv(weight)
    loss, stats = torch.full((1,), float("nan"), device=DEV), zeros((B + 1) * (2 * K + 2))
    wb = hip.query("rpnet_loss_workspace_bytes", B, K, H, W)
    ws = ws_for(wb)
    hip.call("rpnet_dice_ce_fwd", hip.ptr(ld), hip.ptr(lb), hip.ptr(loss), hip.ptr(stats), B, K, H, W, with_dice, ign, per_sample,
             hip.ptr(wd), hip.ptr(ws), wb)
    hold("loss", "loss", loss[0], *both(R.dice_ce, logits, labels, **kw))
    pre = rnd(seed + 1, B, K, H, W)
    dl = dv(pre) if acc else torch.full((B, K, H, W), float("nan"), device=DEV)
    gs = torch.full((1,), gscale, device=DEV)
    hip.call("rpnet_dice_ce_bwd", hip.ptr(ld), hip.ptr(lb), hip.ptr(stats), hip.ptr(gs), hip.ptr(dl), B, K, H, W, with_dice, ign,
             per_sample, hip.ptr(wd), acc)
    g64, g32 = both(R.dice_ce_bwd, logits, labels, gscale=float(np.float32(gscale)), **kw)
    if acc:
        g64, g32 = g64 + pre.double(), g32 + pre
    hold("loss", "dlogits", dl, g64, g32)


# ============================================================================= align pieces
ARGMAX_ROWS = [
    # B, K, hw, keep given, a class that wins nowhere
    (1, 1, 1, True, None),        # K = 1: every pixel is class 0
    (2, 2, 255, True, None),      # one pixel short of the 256 threads
    (3, 3, 256, False, None),     # exactly one pass; keep NULL
    (2, 4, 257, True, 2),         # one pixel into the second pass; class 2 wins nowhere: keep 0
    (4, 2, 4096, True, 1),        # 16 passes; the foreground wins nowhere (the skipped way of alignLoss)
    (1, 4, 4096, False, None),    # K = 4, keep NULL
    (5, 3, 1, True, 0),           # hw = 1, the background wins nowhere
    (1, 2, 257, False, None),     # K = 2 at 257
    (3, 1, 255, False, None),     # K = 1 without keep
    (2, 4, 256, True, 3),         # the last class wins nowhere
    (1, 3, 4096, True, None),     # K = 3 at 4096
    (8, 2, 255, True, None),      # B = 8
    (2, 3, 257, True, 1),         # K = 3, class 1 wins nowhere
    (1, 4, 1, True, None),        # K = 4 on one pixel: three classes count 0
    (6, 2, 256, True, None),      # B = 6 at one pass
]


def test_argmax_reference_breaks_ties_towards_the_first_index():
    x = torch.tensor([[[1.0, 0.0, 2.0, 5.0], [1.0, 3.0, 2.0, 5.0], [0.0, 3.0, 2.0, 5.0]]], dtype=torch.float64)
    assert x.argmax(1).tolist() == [[0, 1, 0, 0]]
    assert x.float().argmax(1).tolist() == [[0, 1, 0, 0]]


@pytest.mark.parametrize("B,K,hw,with_keep,loser", ARGMAX_ROWS)
def test_argmax_masks(hip, B, K, hw, with_keep, loser):
    test_argmax_reference_breaks_ties_towards_the_first_index()
    seed = 6000 + K * 17 + hw % 101 + B
    pred = torch.from_numpy(np.random.RandomState(seed).randint(-3, 4, (B, K, hw)).astype(np.float32))   # small integers: planted ties
    if hw >= 4 and K >= 2:
        pred[:, :, :3] = 1.0                    # every class equal on the first pixels
    if loser is not None:
        pred[:, loser] = -10.0
    masks, counts = torch.full((B, K, hw), float("nan"), device=DEV), torch.full((B, K), float("nan"), device=DEV)
    keep = torch.full((K, B), float("nan"), device=DEV) if with_keep else None
    hip.call("rpnet_argmax_masks", hip.ptr(dv(pred)), hip.ptr(masks), hip.ptr(counts), hip.ptr(keep), B, K, hw)
    m64, c64, k64 = R.argmax_masks(pred)
    assert torch.equal(masks.cpu().double(), m64) and torch.equal(counts.cpu().double(), c64)
    if with_keep:
        assert torch.equal(keep.cpu().double(), k64)
        if loser is not None and K > 1:
            assert keep[loser].abs().max() == 0
    if loser is not None and K > 1:
        assert counts[:, loser].abs().max() == 0


@pytest.mark.parametrize("n", [1, 255, 4096 * 256 + 3])      # 4096 x 256 + 3 wraps the grid of 4096 blocks
def test_align_labels(hip, n):
    rs = np.random.RandomState(6100 + n % 7)
    vals = np.asarray([0.0, 0.5, 1.0], dtype=np.float32)
    fore, back = torch.from_numpy(vals[rs.randint(0, 3, n)]), torch.from_numpy(vals[rs.randint(0, 3, n)])
    if n >= 255:
        assert ((fore == 1) & (back == 1)).any() and ((fore == 0.5) & (back == 0.5)).any()      # both-ones: the background wins
    lab = torch.full((n,), -7, device=DEV, dtype=torch.int64)
    hip.call("rpnet_align_labels", hip.ptr(dv(fore)), hip.ptr(dv(back)), hip.ptr(lab), n)
    assert torch.equal(lab.cpu(), R.align_labels(fore, back))


# ================================================================================== pooling
def tied(seed, *shape):
    """small integers: equal values inside most windows, in every position"""
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 3, shape).astype(np.float32))


def test_maxpool_reference_routes_to_the_first_maximum():
    z = torch.ones(1, 4, 4, 4)
    g = R.maxpool2_bwd(z, torch.ones(1, 2, 2, 4))
    assert g[0, ::2, ::2].min() == 1 and g.sum() == 16
    g3 = R.maxpool3_bwd(torch.ones(1, 3, 3, 4), torch.ones(1, 3, 3, 4), 1)
    assert g3[0, 0, 0, 0] == 4 and g3[0, 2, 2, 0] == 0


MAXPOOL2_ROWS = [
    # N, H, W, C, skip
    (1, 2, 2, 4, False),      # H = W = 2, C = 4: every FastDiv divisor is 1
    (3, 2, 2, 12, True),      # the same with C / 4 = 3 and a skip tensor
    (2, 6, 10, 12, False),    # odd Ho = 3 and Wo = 5, C / 4 = 3 is no power of two
    (1, 6, 4, 64, True),      # odd Ho, C = 64, skip
    (2, 16, 16, 64, False),   # the plain case
    (1, 14, 2, 4, True),      # Wo = 1, odd Ho = 7
    (2, 2, 18, 4, False),     # Ho = 1, odd Wo = 9
    (1, 256, 256, 64, True),  # the first encoder level's shape: 1024 blocks
    (5, 10, 6, 12, True),     # N = 5, odd Ho = 5 and Wo = 3
    (1, 4, 4, 4, False),      # four windows
    (2, 6, 6, 64, False),     # odd Ho = Wo = 3 at C = 64
    (7, 2, 2, 4, True),       # seven images of one window
    (1, 2, 2, 64, True),      # one window, C = 64
    (3, 12, 20, 12, False),   # Wo = 10, Ho = 6
    (1, 30, 26, 4, True),     # odd Ho = 15, Wo = 13
]


@pytest.mark.parametrize("N,H,W,C,with_skip", MAXPOOL2_ROWS)
def test_maxpool2_and_upsample2(hip, N, H, W, C, with_skip):
    test_maxpool_reference_routes_to_the_first_maximum()
    seed = 7000 + H * 3 + W + C
    z = tied(seed, N, H, W, C)
    z[0, :2, :2, :] = 1.0                                       # one window tied in all four positions, every channel
    dpool, skip = rnd(seed + 1, N, H // 2, W // 2, C), (rnd(seed + 2, N, H, W, C) if with_skip else None)
    zd = dv(z)
    out = torch.full((N, H // 2, W // 2, C), float("nan"), device=DEV)
    hip.call("rpnet_maxpool2_fwd", hip.ptr(zd), hip.ptr(out), N, H, W, C)
    assert torch.equal(out.cpu().double(), R.maxpool2(z))
    dz = torch.full((N, H, W, C), float("nan"), device=DEV)
    hip.call("rpnet_maxpool2_bwd", hip.ptr(zd), hip.ptr(dv(dpool)), hip.ptr(None if skip is None else dv(skip)), hip.ptr(dz), N, H, W, C)
    if skip is None:
        assert torch.equal(dz.cpu().double(), R.maxpool2_bwd(z, dpool))          # a routed copy: exact
    else:
        r64, r32 = both(R.maxpool2_bwd, z, dpool, skip)
        assert torch.equal(dz.cpu(), r32)                                          # one fp32 addition per element: the same bits
        hold("pooling", "maxpool2_bwd_skip", dz, r64, r32)
    dyu = rnd(seed + 3, N, H, W, C)
    dx = torch.full((N, H // 2, W // 2, C), float("nan"), device=DEV)
    hip.call("rpnet_upsample2_bwd", hip.ptr(dv(dyu)), hip.ptr(dx), N, H, W, C)
    hold("pooling", "upsample2_bwd", dx, *both(R.upsample2_bwd, dyu))


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("N,H,W,C", [(2, 1, 1, 4), (1, 1, 7, 8), (3, 5, 1, 4), (2, 7, 9, 12), (1, 8, 6, 64), (1, 3, 3, 4), (2, 13, 5, 8)])
def test_maxpool3(hip, stride, N, H, W, C):
    """H = 1, W = 1 and odd extents at both strides; ties everywhere (small integers), all exact"""
    seed = 7100 + H * 5 + W + C
    z = tied(seed, N, H, W, C)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    dpool = rnd(seed + 1, N, Ho, Wo, C)
    out = torch.full((N, Ho, Wo, C), float("nan"), device=DEV)
    hip.call("rpnet_maxpool3_fwd", hip.ptr(dv(z)), hip.ptr(out), N, H, W, C, stride)
    assert torch.equal(out.cpu().double(), R.maxpool3(z, stride))
    dz = torch.full((N, H, W, C), float("nan"), device=DEV)
    hip.call("rpnet_maxpool3_bwd", hip.ptr(dv(z)), hip.ptr(dv(dpool)), hip.ptr(dz), N, H, W, C, stride)
    hold("pooling", "maxpool3_bwd", dz, *both(R.maxpool3_bwd, z, dpool, stride))      # up to 9 (stride 1) gradients add up


BIAS_ROWS = [
    # P, C, z given
    (1, 4, False),         # one row, one thread column, z NULL
    (3, 24, True),         # C / 4 = 6: rows_it = 42, threads 252 - 255 idle
    (100000, 64, True),    # 6250 row groups wrap the 512 blocks
    (3, 400, True),        # C / 4 = 100: rows_it = 2, 56 idle threads
    (1, 1024, False),      # C / 4 = 256: one row per pass, nothing to add in LDS
    (100000, 24, False),   # the wrap with idle threads and z NULL
    (3, 4, True),          # rows_it = 256 and three rows
    (1, 64, True),         # P = 1 with z
    (100000, 4, True),     # 391 blocks of 256 rows
    (3, 1024, True),       # three passes of the one row group
    (1, 400, False),       # P = 1 at C = 400
    (3, 64, False),        # z NULL at C = 64
    (1, 24, True),         # P = 1 at C = 24
    (100000, 400, True),   # the widest wrap: 50000 row pairs over 512 blocks
    (3, 24, False),        # z NULL at C = 24
]


@pytest.mark.parametrize("P,C,with_z", BIAS_ROWS)
def test_bias_relu_bwd(hip, P, C, with_z):
    seed = 7200 + C + P % 11
    dz = rnd(seed, P, C)
    z = None
    if with_z:
        z = rnd(seed + 1, P, C)
        z[torch.from_numpy(np.random.RandomState(seed).rand(P, C) < 0.3)] = 0.0      # z == 0 passes gradient 0
        z[0, 0] = 0.0
    dy, db = torch.full((P, C), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
    wb = hip.query("rpnet_bias_relu_bwd_workspace_bytes", C)
    ws = ws_for(wb)
    hip.call("rpnet_bias_relu_bwd", hip.ptr(dv(dz)), hip.ptr(None if z is None else dv(z)), hip.ptr(dy), hip.ptr(db), P, C, hip.ptr(ws), wb)
    (y64, b64), (y32, b32) = both(R.bias_relu_bwd, dz, z)
    assert torch.equal(dy.cpu().double(), y64)                                  # a selection: exact
    if with_z:
        assert dy[0, 0] == 0
    hold("pooling", "bias_grad", db, b64, b32)


# ======================================================================= soft-mask gradient
ROWDOT_ROWS = [
    # P, C, mode, accumulate_dscale
    (1, 4, 1, 0),          # one pixel, one live lane
    (5, 64, 2, 1),         # 16 live lanes, mode 2 onto a prefill
    (40000, 64, 1, 0),     # P = 40000 wraps 8192 blocks x 4 waves
    (5, 256, 1, 1),        # 64 lanes x float4: the whole wave, one pass
    (5, 260, 2, 0),        # C / 4 = 65: lane 0 wraps the channel loop
    (5, 1028, 1, 1),       # C / 4 = 257: four passes, then lane 0 alone
    (40000, 4, 2, 1),      # the wrap in mode 2 with accumulate
    (1, 1028, 2, 0),       # P = 1 at the widest row
    (1, 256, 2, 1),        # P = 1, mode 2, accumulate
    (5, 4, 1, 0),          # P = 5: the second block has one wave of work
    (40000, 260, 1, 1),    # both wraps at once
    (1, 64, 1, 1),         # P = 1 at C = 64
    (5, 64, 1, 0),         # mode 1 at C = 64
    (1, 260, 1, 0),        # P = 1 at C = 260
    (5, 1028, 2, 0),       # mode 2 at C = 1028
]


@pytest.mark.parametrize("P,C,mode,acc", ROWDOT_ROWS)
def test_rowdot_scale(hip, P, C, mode, acc):
    seed = 8000 + C + mode + P % 13
    g, x = rnd(seed, P, C), rnd(seed + 1, P, C)
    s = torch.rand(P, generator=torch.Generator().manual_seed(seed))
    pre = rnd(seed + 2, P)
    dx = torch.full((P, C), float("nan"), device=DEV)
    ds = dv(pre) if acc else torch.full((P,), float("nan"), device=DEV)
    hip.call("rpnet_rowdot_scale", hip.ptr(dv(g)), hip.ptr(dv(x)), hip.ptr(dv(s)), hip.ptr(dx), hip.ptr(ds), P, C, mode, acc)
    (x64, s64), (x32, s32) = both(R.rowdot_scale, g, x, s, mode)
    if acc:
        s64, s32 = s64 + pre.double(), s32 + pre
    hold("rowdot", "dx", dx, x64, x32)
    hold("rowdot", "dscale", ds, s64, s32)


# ====================================================== the fp16 tensor scale of BatchNorm + ReLU
@pytest.mark.parametrize("N,HW,C,groups", [(2, 64, 64, 1), (4, 1024, 256, 2), (1, 9, 7, 1), (6, 4096, 300, 2)])
def test_bn_act_scale(hip, N, HW, C, groups):
    """rpnet_bn_act_scale: s = a power of two with bound <= s 2^15 < 2 bound (1.0001 of slack on sqrt(n)),
    bound = max_c |gamma_c| sqrt(n) + |beta_c|, n = the values per channel of one statistic group"""
    gamma, beta = rnd(8100 + C, C) * 1.5, rnd(8101 + C, C)
    s = torch.full((1,), float("nan"), device=DEV)
    hip.call("rpnet_bn_act_scale", hip.ptr(dv(gamma)), hip.ptr(dv(beta)), hip.ptr(s), N, HW, C, groups)
    bound = R.bn_act_bound(gamma, beta, (N // groups) * HW).item()
    top = s.item() * 2.0 ** 15
    assert np.frexp(s.item())[0] == 0.5                                  # a power of two
    assert bound <= top < 2.0 * bound * 1.0002


@pytest.mark.parametrize("bound", [1.0, 3.7, 2.0 ** -20, 65504.0, 1.0e6, 0.75])
def test_pow2_scale(hip, bound):
    """rpnet_pow2_scale: the power-of-two tensor scale that maps a bound to <= 2^15 and wastes less than one bit"""
    b, s = torch.full((1,), bound, device=DEV), torch.full((1,), float("nan"), device=DEV)
    hip.call("rpnet_pow2_scale", hip.ptr(b), hip.ptr(s))
    top = s.item() * 2.0 ** 15
    assert np.frexp(s.item())[0] == 0.5
    assert float(np.float32(bound)) <= top < 2.0 * float(np.float32(bound)) * 1.0002


# ================================================================================= refusals
def test_refusals(hip):
    """one call per shape rule a launcher states: the documented rpnet_status comes back from the host, nothing is launched"""
    t = zeros(4096)
    lab = zeros(64, dtype=torch.int64)
    big = 1 << 20
    cases = [
        # cosine match: C = 4 * 2^n <= 256, 1 <= K <= 4, workspace
        ("rpnet_cosine_match_fwd", (t, t, t, 1, 2, 4, 12, 20.0), SHAPE),
        ("rpnet_cosine_match_fwd", (t, t, t, 1, 2, 4, 6, 20.0), SHAPE),
        ("rpnet_cosine_match_fwd", (t, t, t, 1, 2, 1, 512, 20.0), SHAPE),
        ("rpnet_cosine_match_fwd", (t, t, t, 1, 5, 4, 64, 20.0), SHAPE),
        ("rpnet_cosine_match_fwd", (t, t, t, 1, 0, 4, 64, 20.0), SHAPE),
        ("rpnet_cosine_match_fwd", (t, None, t, 1, 2, 4, 64, 20.0), ARG),
        ("rpnet_cosine_match_bwd", (t, t, t, t, t, 1, 2, 4, 12, 20.0, 0, t, big), SHAPE),
        ("rpnet_cosine_match_bwd", (t, t, t, t, t, 1, 5, 4, 64, 20.0, 0, t, big), SHAPE),
        ("rpnet_cosine_match_bwd", (t, t, t, t, t, 1, 2, 4, 64, 20.0, 0, t, 2 * 64 * 4 - 1), WORKSPACE),
        ("rpnet_cosine_match_bwd", (t, t, t, t, t, 1, 2, 4, 64, 20.0, 0, None, big), ARG),
        # masked pooling: C / 4 a power of two <= 256, 1 <= nmask <= 4, whole ratios, workspace
        ("rpnet_masked_pool_fwd", (t, t, t, t, 1, 2, 4, 24, t, big), SHAPE),
        ("rpnet_masked_pool_fwd", (t, t, t, t, 1, 2, 4, 2048, t, big), SHAPE),
        ("rpnet_masked_pool_fwd", (t, t, t, t, 1, 5, 4, 64, t, big), SHAPE),
        ("rpnet_masked_pool_fwd", (t, t, t, t, 1, 0, 4, 64, t, big), SHAPE),
        ("rpnet_masked_pool_fwd", (t, t, t, t, 1, 2, 4, 64, t, 64 * 2 * 64 * 4 - 1), WORKSPACE),
        ("rpnet_masked_pool_fwd", (t, t, t, t, 1, 2, 4, 64, None, big), ARG),
        ("rpnet_masked_pool_bwd", (t, t, t, t, 1, 2, 4, 6, 0), SHAPE),
        ("rpnet_mask_adjoint", (t, t, t, 1, 1, 12, 12, 5, 4), SHAPE),
        ("rpnet_mask_adjoint", (t, t, t, 1, 1, 12, 12, 4, 5), SHAPE),
        # bilinear: the adjoint needs whole ratios
        ("rpnet_bilinear_up_bwd", (t, t, 1, 5, 5, 12, 12), SHAPE),
        ("rpnet_bilinear_up_bwd", (t, None, 1, 4, 4, 8, 8), ARG),
        ("rpnet_bilinear_up_fwd", (None, t, 1, 4, 4, 8, 8), ARG),
        # softmax / threshold / pool: K >= 2, H and W multiples of the scale
        ("rpnet_softmax_thresh_pool", (t, t, 1, 1, 8, 8, 4, 0), SHAPE),
        ("rpnet_softmax_thresh_pool", (t, t, 1, 2, 6, 8, 4, 0), SHAPE),
        ("rpnet_softmax_thresh_pool", (t, t, 1, 2, 8, 6, 4, 1), SHAPE),
        ("rpnet_softmax_pool_bwd", (t, t, t, 1, 1, 8, 8, 4), SHAPE),
        ("rpnet_softmax_pool_bwd", (t, t, t, 1, 2, 8, 6, 4), SHAPE),
        ("rpnet_mask_avgpool", (t, t, 1, 8, 8, 0), SHAPE),
        ("rpnet_mask_avgpool", (t, t, 1, 8, 6, 4), SHAPE),
        # loss: 2 <= K <= 4, workspace
        ("rpnet_dice_ce_fwd", (t, lab, t, t, 1, 5, 4, 4, 1, -1, 0, None, t, big), SHAPE),
        ("rpnet_dice_ce_fwd", (t, lab, t, t, 1, 1, 4, 4, 1, -1, 0, None, t, big), SHAPE),
        ("rpnet_dice_ce_fwd", (t, lab, t, t, 1, 2, 4, 4, 1, -1, 0, None, t, 64 * 6 * 8 - 1), WORKSPACE),
        ("rpnet_dice_ce_fwd", (t, None, t, t, 1, 2, 4, 4, 1, -1, 0, None, t, big), ARG),
        ("rpnet_dice_ce_bwd", (t, lab, t, t, t, 1, 5, 4, 4, 1, -1, 0, None, 0), SHAPE),
        ("rpnet_dice_ce_bwd", (t, lab, None, t, t, 1, 2, 4, 4, 1, -1, 0, None, 0), ARG),
        # align pieces: 1 <= K <= 4
        ("rpnet_argmax_masks", (t, t, t, None, 1, 5, 16), SHAPE),
        ("rpnet_argmax_masks", (t, t, t, None, 1, 0, 16), SHAPE),
        ("rpnet_align_labels", (t, None, lab, 16), ARG),
        # pooling: even extents, C % 4, stride 1 or 2, C / 4 <= 256, workspace
        ("rpnet_maxpool2_fwd", (t, t, 1, 3, 4, 4), SHAPE),
        ("rpnet_maxpool2_fwd", (t, t, 1, 4, 4, 6), SHAPE),
        ("rpnet_maxpool2_bwd", (t, t, None, t, 1, 4, 5, 4), SHAPE),
        ("rpnet_upsample2_bwd", (t, t, 1, 4, 4, 2), SHAPE),
        ("rpnet_maxpool3_fwd", (t, t, 1, 4, 4, 4, 3), SHAPE),
        ("rpnet_maxpool3_bwd", (t, t, t, 1, 4, 4, 6, 1), SHAPE),
        ("rpnet_bias_relu_bwd", (t, t, t, t, 4, 6, t, big), SHAPE),
        ("rpnet_bias_relu_bwd", (t, t, t, t, 1, 1028, t, big), SHAPE),
        ("rpnet_bias_relu_bwd", (t, t, t, t, 4, 64, t, 512 * 64 * 8 - 1), WORKSPACE),
        # soft-mask gradient: C % 4, mode 1 or 2
        ("rpnet_rowdot_scale", (t, t, t, t, t, 4, 6, 1, 0), SHAPE),
        ("rpnet_rowdot_scale", (t, t, t, t, t, 4, 8, 3, 0), SHAPE),
        ("rpnet_rowdot_scale", (t, t, t, t, None, 4, 8, 1, 0), ARG),
        ("rpnet_bn_act_scale", (t, t, t, 2, 16, 0, 1), ARG),
    ]
    for name, args, want in cases:
        got = rc_of(hip, name, *args)
        assert got == want, f"{name}{tuple(a if not torch.is_tensor(a) else 'T' for a in args)}: rc {got}, expected {want}"
        assert hip.load().rpnet_last_error_string().decode() != ""
    torch.cuda.synchronize()
    assert t.abs().max() == 0               # nothing ran
