"""Cases, references and comparison functions shared by tests/test_host_glue_ref64.py and tests/test_gpu_glue_fp64.py: the launches
that training runs per refinement iteration and per step — the fused refinement glue (csrc/refine.hip: rpnet_refine_glue_fwd / _bwd /
_bwd_workspace_bytes / _supported) and the multi-tensor loss and objective (csrc/loss.hip: rpnet_dice_ce_multi_fwd / _bwd,
rpnet_objective_fwd / _bwd) — against the float64 references of tests/ref64.py (refine_glue, refine_glue_bwd, dice_ce, dice_ce_bwd,
dice_ce_stats, objective).

A *backend* runs the eight entry points on CPU tensors and returns CPU tensors: the HIP library (the GPU test: every output NaN-filled
inside a larger buffer with GUARD sentinel elements on both sides, "guards" = the number of sentinel elements that changed) or
SimBackend, a float32 torch restatement in the kernels' summation order, with or without a seeded defect (the host test).  The
check_* functions drive a backend through one case and return records; hold() prints them and asserts.  Neither test restates a bound.

Bound (FACTOR and FLOOR are tests/test_gpu_small_ops.py's numbers, tests/test_host_glue_ref64.py asserts they still are):
rel_err(got, r64) <= 8 * yard + 4 * 2^-24, yard = rel_err(r32, r64), r32 = the same ref64 function at float32.  A value that is not
finite has an infinite error: a NaN left in an owned output fails its check.

Hard masks: 16 * mask_next must be integral; per 4 x 4 cell |16 got - 16 ref64| may not exceed the number of UNDECIDED up-sampled
pixels of the cell, those whose float64 margin |l1 - logsumexp(others)| is at most 16 * (FACTOR * yard_logits + FLOOR) * max |logits64|
(the reference alone decides which); at most UNDECIDED_SHARE of a case's cells may hold one.  Operand planes: bit for bit the planes
of fp32(x * f), f = the kernel's OWN mask_next or fp32(1 - mask_next), by tests/operand_cases.py's reference (masked, split_planes):
a mask error is charged once.  Zero vectors: pred exactly 0, gradients finite, the feature-gradient row of the zero vector (and the
prototype-gradient row of a zero prototype) out of the comparison, as in test_cosine_match."""
import math

import torch
import torch.nn.functional as F

from tests import operand_cases as OC
from tests import ref64 as R
from tests.corr_cases import ARG, FACTOR, FLOOR, SHAPE, WORKSPACE, Rec, case_seed, hold, plane_values, pow2_scale, split_planes  # noqa: F401
from tests.helpers import rel_err, rnd

F32, F64, I16 = torch.float32, torch.float64, torch.int16
FEAT = 64                       # channels of the matched features: the one F the glue takes
SCALER = 20.0
GUARD = 64                      # sentinel elements in front of and behind every output of the HIP backend
UNDECIDED_SHARE = 0.02
ZERO_PIXEL = (0, 3, 4)          # (b, y, x) of the planted zero feature vector: an interior pixel of every shape's first tile
EPS = 1e-8                      # kCosEps

# ------------------------------------------------------------------------------------------------------------------ tables
# (B, K, h, w): all extents multiples of 8 and at least 8, the smallest the kernel takes
GLUE_SHAPES = [(1, 2, 8, 8),        # one tile: every halo pixel clamps
               (1, 4, 8, 8),        # K = 4 fills lg[3], pred_s[3], dps[3]
               (2, 3, 8, 16),       # one tile down, two across
               (2, 3, 16, 8),       # two down, one across
               (3, 2, 16, 24),      # 2 x 3 tiles
               (1, 4, 24, 16),      # 3 x 2 tiles: tile 2 has a real halo above and below, K = 4
               (5, 2, 8, 8)]        # B above 3
# every shape x {BatchNorm given, NULL} x {no mask, hard, soft}, without planes: stages A and B do not know about stage C
GLUE_FWD_CASES = [(s, bn, m, 0, 0) for s in GLUE_SHAPES for bn in (True, False) for m in (None, "hard", "soft")]
# Stage C sees the mask, B / h / w (its row index) and (planes, Cx) only, never K or the BatchNorm form, so the cross of every
# shape with every (planes, Cx) pair is pruned to: all twelve pairs at 2 x 3 x 16 x 8 (two tiles and two episodes: every term of the
# row index is non-zero; BatchNorm NULL on every third, hard and soft masks alternating), the three plane counts at K = 4 on six
# tiles, B = 5 at the two extreme Cx (256 pixel slots for 64 pixels, one pixel per pass), and planes at one tile down / two across.
GLUE_PLANE_CASES = ([((2, 3, 16, 8), i % 3 != 0, ("hard", "soft")[i % 2], p, C)
                     for i, (p, C) in enumerate((p, C) for p in (1, 2, 3) for C in (8, 64, 256, 2048))]
                    + [((1, 4, 24, 16), True, "hard", p, 64) for p in (1, 2, 3)]
                    + [((5, 2, 8, 8), False, "soft", 2, 8), ((5, 2, 8, 8), True, "hard", 3, 2048), ((2, 3, 8, 16), False, "hard", 1, 256)])
GLUE_BWD_CASES = [(s, kind) for s in GLUE_SHAPES for kind in ("random", "ring", "impulse")]
ZERO_PATCH_SHAPES = [(2, 3, 8, 16), (1, 4, 24, 16), (5, 2, 8, 8)]       # more than one patch per launch: one of them all zero
# (shape, kind) -> factor of the one backward check that may take more than FACTOR yardsticks (none measured above it so far)
MEASURED_FACTORS = {}

# (n, B, K, H, W, absent class, the first tensor listed again as the last)
LOSS_ROWS = [(1, 1, 2, 5, 7, None, False),           # n = 1, H W = 35: 63 of the 64 partial blocks idle
             (2, 3, 3, 129, 127, None, False),       # H W = 16383: one short of the forward's 64 x 256 grid stride
             (2, 1, 4, 113, 145, None, False),       # H W = 16385: one pixel into the second pass, K = 4
             (2, 1, 2, 257, 256, None, False),       # 257 blocks of 256 pixels: past the backward's 256-block cap
             (16, 8, 2, 5, 7, None, False),          # n = 16 fills the pointer set, B = 8
             (3, 3, 4, 24, 20, 2, True),             # class 2 absent; the same pointer in slots 0 and 2
             (3, 8, 3, 24, 20, None, False)]         # B = 8, K = 3, the weights (2, 1, 1) as they stand
WEIGHTS = {"211": (2.0, 1.0, 1.0), "frac": (0.5, 0.0, 1.25), "ones": (1.0, 1.0, 1.0)}
# the objective's forms: (weights, gscale, extra given, dextra given)
OBJECTIVE_FORMS = [("211", None, True, True), ("frac", 0.37, False, True), ("ones", 0.37, True, False), ("frac", None, False, False),
                   ("211", 0.37, True, True), ("ones", None, False, True)]
EXTRA, EXTRA_SCALE = 1.2345, 0.37


def weights_for(kind, n):
    return [WEIGHTS[kind][i % 3] for i in range(n)]


# ----------------------------------------------------------------------------------------------------------------- records
class GRec(Rec):
    def line(self):
        return f"PARITY glue {self.family} {self.what} err={self.err:.3e} yard={self.yard:.3e} ratio={self.ratio:.2f}"


def measure(family, what, got, r64, r32, factor=FACTOR):
    got, r64 = torch.as_tensor(got), torch.as_tensor(r64)
    assert got.shape == r64.shape, (family, what, tuple(got.shape), tuple(r64.shape))
    err = rel_err(got, r64) if torch.isfinite(got).all() else math.inf
    yard = rel_err(r32, r64)
    return GRec(family, what, err, yard, factor * yard + FLOOR)


def exact(family, what, got, want):
    """mismatching elements; fp32 is compared as bits (the sign of zero and NaN patterns included), as tests/operand_cases.py does"""
    got, want = OC.bits(torch.as_tensor(got)), OC.bits(torch.as_tensor(want))
    assert got.shape == want.shape, (family, what, tuple(got.shape), tuple(want.shape))
    return GRec(family, what, int((got != want).sum()), 0.0, 0.0, exact=True)


def count(family, what, n):
    """an exact record of a count that must be 0"""
    return GRec(family, what, int(n), 0.0, 0.0, exact=True)


def guards(family, what, touched):
    return count(family, f"guard elements touched {what}", touched)


# ------------------------------------------------------------------------------------------------------------------ inputs
def glue_inputs(shape, bn, zero_patch=False):
    """(y [B, h, w, 64], scale, shift [64] or None, proto [B, K, 64]).  One pixel's y is driven below zero in all 64 channels (zero
    after ReLU); without BatchNorm the zero feature vector and a zero prototype (class 0 of the last episode) are planted directly.
    zero_patch: the whole first 8 x 8 patch of the last episode is zero after ReLU."""
    B, K, h, w = shape
    seed = case_seed(B, K, h, w, int(bn), int(zero_patch))
    y = rnd(seed, B, h, w, FEAT) * 2
    proto = rnd(seed + 1, B, K, FEAT)
    scale = shift = None
    b, py, px = ZERO_PIXEL
    if bn:
        scale = 0.75 + 0.5 * torch.rand(FEAT, generator=torch.Generator().manual_seed(seed + 2))
        shift = rnd(seed + 3, FEAT) * 0.3
        y[b, py, px] = -9.0
        if zero_patch:
            y[B - 1, :8, :8] = -9.0
    else:
        y[b, py, px] = 0.0
        proto[B - 1, 0] = 0.0
        if zero_patch:
            y[B - 1, :8, :8] = 0.0
    return y, scale, shift, proto


def bwd_inputs(shape, kind):
    """(dlogits [B, K, 4h, 4w], f [B, h, w, 64] = features after BatchNorm + ReLU with the zero pixel, proto)"""
    B, K, h, w = shape
    y, scale, shift, proto = glue_inputs(shape, True)
    f = R.bn_relu(y, scale, shift, dtype=F32)
    g = rnd(case_seed(B, K, h, w, 9), B, K, 4 * h, 4 * w)
    if kind == "ring":              # the outermost ring of the image only: every window that reads it clamps
        inner = torch.zeros_like(g)
        inner[..., 1:-1, 1:-1] = 1
        g = g * (1 - inner)
    elif kind == "impulse":         # the far corner of the first patch: the corner of the image, or the meeting point of four patches
        v = g[B - 1, K - 1, 31, 31].clone()
        g = torch.zeros_like(g)
        g[B - 1, K - 1, 31, 31] = v
    return g, f, proto


# ----------------------------------------------------------------------------------------------------------- glue, forward
def undecided_cells(logits64, yard_logits):
    """[B, h, w]: the number of up-sampled pixels per 4 x 4 cell whose float64 margin is within the logits' bound of the boundary"""
    tol = 16 * (FACTOR * yard_logits + FLOOR) * float(logits64.abs().max())
    und = (R.hard_mask_margin(logits64) <= tol).double()
    return F.avg_pool2d(und[:, None], 4, divisor_override=1)[:, 0]


def undecided_share(shape, bn):
    """the share of a case's cells that hold an undecided pixel, from the two references alone"""
    y, scale, shift, proto = glue_inputs(shape, bn)
    lg64 = R.refine_glue(y, scale, shift, proto, SCALER)[2]
    lg32 = R.refine_glue(y, scale, shift, proto, SCALER, dtype=F32)[2]
    return float((undecided_cells(lg64, rel_err(lg32, lg64)) > 0).double().mean())


def hard_mask_records(fam, tag, got, mask64, logits64, yard_logits):
    und = undecided_cells(logits64, yard_logits)
    g16 = got.double() * 16
    if not torch.isfinite(g16).all():
        return [count(fam, f"hard mask not finite {tag}", int((~torch.isfinite(g16)).sum()))]
    return [count(fam, f"16 * hard mask not integral {tag}", int((g16 != g16.round()).sum())),
            count(fam, f"hard mask cells beyond their undecided pixels {tag}", int(((g16 - 16 * mask64).abs() > und).sum())),
            GRec(fam, f"share of cells with an undecided pixel {tag}", float((und > 0).double().mean()), 0.0, UNDECIDED_SHARE)]


def plane_records(fam, tag, out, x, xs, planes):
    """xk / xq against the exact reference of tests/operand_cases.py, fed the kernel's own mask_next"""
    B, h, w, C = x.shape
    m = out["mask_next"].reshape(-1)
    if not torch.isfinite(m).all():
        return [count(fam, f"planes of a mask that is not finite {tag}", 1)]
    recs = []
    for name, mode in (("xk", 1), ("xq", 2)):
        v = OC.masked(x.reshape(-1, C), m, mode)
        want = split_planes(v, planes, xs).reshape(planes, B, h, w, C)
        recs.append(exact(fam, f"{name} planes {tag}", out[name], want))
        if planes == 3:         # three bf16 planes sum exactly to fp32(x * f)
            recs.append(exact(fam, f"{name} h + m + l == fl32(x f) {tag}", plane_values(out[name]), v.double().reshape(B, h, w, C)))
    return recs


def check_glue_fwd(be, shape, bn, mask, planes=0, C=0):
    """rpnet_refine_glue_fwd at one shape and form; mask: None, "hard" or "soft"; planes 0: x NULL"""
    B, K, h, w = shape
    fam = "fwd" + ("_bn" if bn else "") + (f"_{mask}" if mask else "") + (f"_p{planes}" if planes else "")
    tag = f"{B}x{K}x{h}x{w}" + (f" Cx={C}" if planes else "")
    y, scale, shift, proto = glue_inputs(shape, bn)
    x = rnd(case_seed(B, h, w, C, planes, 5), B, h, w, C) if planes else None
    xs = pow2_scale(x.abs().max()) if planes in (1, 2) else None
    out = be.glue_fwd(y, scale, shift, proto, SCALER, mask is not None, mask == "soft", x, xs, planes)
    r64 = R.refine_glue(y, scale, shift, proto, SCALER, mask == "soft")
    r32 = R.refine_glue(y, scale, shift, proto, SCALER, mask == "soft", dtype=F32)
    recs = [guards(fam, tag, out["guards"])]
    if bn:
        recs.append(measure(fam, f"z {tag}", out["z"], r64[0], r32[0]))
    else:
        assert out["z"] is None
    recs += [measure(fam, f"pred {tag}", out["pred"], r64[1], r32[1]), measure(fam, f"logits {tag}", out["logits"], r64[2], r32[2])]
    b, py, px = ZERO_PIXEL
    recs.append(exact(fam, f"pred of the zero feature vector {tag}", out["pred"][b, :, py, px], torch.zeros(K)))
    if not bn:
        recs.append(exact(fam, f"pred of the zero prototype {tag}", out["pred"][B - 1, 0], torch.zeros(h, w)))
    if mask == "soft":
        recs.append(measure(fam, f"soft mask {tag}", out["mask_next"], r64[3], r32[3]))
    elif mask == "hard":
        recs += hard_mask_records(fam, tag, out["mask_next"], r64[3], r64[2], rel_err(r32[2], r64[2]))
    else:
        assert out["mask_next"] is None
    if planes:
        recs += plane_records(fam, tag, out, x, xs, planes)
    return recs


def check_glue_tie(be, planes=3, C=64):
    """two equal prototypes at K = 2: both logits have the same bits everywhere, softmax[1] is exactly 0.5 and the comparison is
    strict, so the hard mask is 0 in every precision; xk is all zero and xq is x"""
    shape = (1, 2, 8, 8)
    fam, tag = "fwd_tie", "1x2x8x8"
    y, scale, shift, proto = glue_inputs(shape, True)
    proto[0, 1] = proto[0, 0]
    x = rnd(77, 1, 8, 8, C)
    out = be.glue_fwd(y, scale, shift, proto, SCALER, True, False, x, None, planes)
    assert R.refine_glue(y, scale, shift, proto, SCALER)[3].abs().max() == 0
    return [guards(fam, tag, out["guards"]), exact(fam, f"logits of equal prototypes {tag}", out["logits"][:, 0], out["logits"][:, 1]),
            exact(fam, f"hard mask of a tie {tag}", out["mask_next"], torch.zeros(1, 8, 8))] + plane_records(fam, tag, out, x, None, planes)


# ---------------------------------------------------------------------------------------------------------- glue, backward
def _bwd_records(fam, tag, got, dl, f, proto, zero_rows, factor):
    df, dproto, touched = got
    (g64, q64), (g32, q32) = R.refine_glue_bwd(dl, f, proto, SCALER), R.refine_glue_bwd(dl, f, proto, SCALER, dtype=F32)
    recs = [guards(fam, tag, touched),
            count(fam, f"gradients not finite {tag}", int((~torch.isfinite(df)).sum() + (~torch.isfinite(dproto)).sum()))]
    df = df.clone()
    for t in (df, g64, g32):            # the reference's gradient of a zero vector is 1 / eps-scaled: those rows stay out
        t[zero_rows] = 0
    return recs + [measure(fam, f"df {tag}", df, g64, g32), measure(fam, f"dproto {tag}", dproto, q64, q32, factor=factor)]


def check_glue_bwd(be, shape, kind):
    """rpnet_refine_glue_bwd (workspace of rpnet_refine_glue_bwd_workspace_bytes) at one shape and one kind of dlogits"""
    B, K, h, w = shape
    dl, f, proto = bwd_inputs(shape, kind)
    zero = torch.zeros(B, h, w, dtype=torch.bool)
    zero[ZERO_PIXEL] = True
    return _bwd_records(f"bwd_{kind}", f"{B}x{K}x{h}x{w}", be.glue_bwd(dl, f, proto, SCALER), dl, f, proto, zero,
                        MEASURED_FACTORS.get((shape, kind), FACTOR))


def check_glue_zero_patch(be, shape):
    """a whole 8 x 8 patch that is zero after ReLU: pred exactly 0 on it (all 16 lane groups of the block), finite gradients, the
    prototype partial of that patch exactly the zero it adds"""
    B, K, h, w = shape
    fam, tag = "zero_patch", f"{B}x{K}x{h}x{w}"
    y, scale, shift, proto = glue_inputs(shape, True, zero_patch=True)
    out = be.glue_fwd(y, scale, shift, proto, SCALER, False, False, None, None, 0)
    r64, r32 = R.refine_glue(y, scale, shift, proto, SCALER), R.refine_glue(y, scale, shift, proto, SCALER, dtype=F32)
    recs = [guards(fam, tag, out["guards"]), exact(fam, f"z of the zero patch {tag}", out["z"][B - 1, :8, :8], torch.zeros(8, 8, FEAT)),
            exact(fam, f"pred of the zero patch {tag}", out["pred"][B - 1, :, :8, :8], torch.zeros(K, 8, 8)),
            measure(fam, f"logits {tag}", out["logits"], r64[2], r32[2])]
    f = r32[0]
    dl = rnd(case_seed(B, K, h, w, 11), B, K, 4 * h, 4 * w)
    zero = (f == 0).all(-1)
    return recs + _bwd_records(fam, tag, be.glue_bwd(dl, f, proto, SCALER), dl, f, proto, zero, FACTOR)


# ------------------------------------------------------------------------------------------------------------------- loss
def loss_inputs(row):
    """(distinct logit tensors, the list as it is passed (a tensor listed twice IS the same object), labels)"""
    n, B, K, H, W, absent, dup = row
    seed = case_seed(n, B, K, H, W)
    g = torch.Generator().manual_seed(seed)
    classes = torch.tensor([k for k in range(K) if k != absent])
    labels = classes[torch.randint(0, len(classes), (B, H, W), generator=g)]
    distinct = [rnd(seed + 1 + i, B, K, H, W) * 2 for i in range(n - 1 if dup else n)]
    return distinct, (distinct + [distinct[0]] if dup else distinct), labels


class LossRefs:
    """the float64 and float32 references of one row, computed once per distinct tensor"""

    def __init__(self, row):
        self.row = row
        self.distinct, self.listed, self.labels = loss_inputs(row)
        self.slot = [next(i for i, d in enumerate(self.distinct) if d is t) for t in self.listed]
        per = lambda fn, dt: [fn(t, self.labels, dtype=dt) for t in self.distinct]            # noqa: E731
        self.loss = {dt: per(R.dice_ce, dt) for dt in (F64, F32)}
        self.grad = {dt: per(R.dice_ce_bwd, dt) for dt in (F64, F32)}
        self.stats = {dt: per(R.dice_ce_stats, dt) for dt in (F64, F32)}

    def listed_of(self, what, dt):
        return [getattr(self, what)[dt][s] for s in self.slot]


def _loss_records(fam, tag, be, kind, refs, weights, gscale, extra, want_dextra):
    n, B, K, H, W, absent, dup = refs.row
    es = EXTRA_SCALE if kind == "objective" else 0.0
    ex = torch.tensor([EXTRA]) if extra else None
    loss, stats, touched = be.loss_fwd(kind, refs.listed, weights, refs.labels, ex, es)
    recs = [guards(fam, f"forward {tag}", touched)]
    s64, s32 = torch.stack(refs.listed_of("stats", F64)), torch.stack(refs.listed_of("stats", F32))
    recs.append(measure(fam, f"stats {tag}", stats[..., :-1], s64[..., :-1], s32[..., :-1]))
    recs.append(exact(fam, f"stats count {tag}", stats[..., -1], s64[..., -1].float()))
    if absent is not None:
        recs.append(exact(fam, f"inter of the absent class {tag}", stats[..., absent], torch.zeros(n, B + 1)))
    l64, l32 = torch.stack(refs.listed_of("loss", F64)), torch.stack(refs.listed_of("loss", F32))
    recs.append(measure(fam, f"loss[z] {tag}", loss[:n], l64, l32))
    wts = weights if kind == "objective" else [1.0] * n
    tot = lambda ls, dt: (torch.tensor(wts, dtype=dt) * ls).sum() + (torch.tensor(es * EXTRA if extra else 0.0, dtype=dt))     # noqa: E731
    recs.append(measure(fam, f"total {tag}", loss[n], tot(l64, F64), tot(l32, F32)))
    grads, dextra, touched = be.loss_bwd(kind, refs.listed, weights, refs.labels, stats, gscale, want_dextra, es)
    recs.append(guards(fam, f"backward {tag}", touched))
    g0 = float(torch.tensor(1.0 if gscale is None else gscale, dtype=F32))
    g64 = torch.stack([g0 * wz * g for wz, g in zip(wts, refs.listed_of("grad", F64))])
    g32 = torch.stack([torch.tensor(g0 * wz, dtype=F32) * g for wz, g in zip(wts, refs.listed_of("grad", F32))])
    recs.append(measure(fam, f"dlogits {tag}", torch.stack(grads), g64, g32))
    for z, wz in enumerate(wts):
        if wz == 0:
            recs.append(count(fam, f"gradient of a tensor of weight 0, slot {z} {tag}", int((grads[z] != 0).sum())))
    if want_dextra:
        recs.append(exact(fam, f"dextra {tag}", dextra, (torch.tensor([g0], dtype=F32) * torch.tensor([es], dtype=F32))))
    else:
        assert dextra is None
    return recs


def check_loss_row(be, row):
    """one row through rpnet_dice_ce_multi_fwd / _bwd (gscale given and NULL) and through every form of rpnet_objective_fwd / _bwd"""
    n, B, K, H, W, absent, dup = row
    refs = LossRefs(row)
    tag = f"n={n} {B}x{K}x{H}x{W}" + (f" absent={absent}" if absent is not None else "") + (" dup" if dup else "")
    recs = []
    for gscale in (None, 0.37):
        recs += _loss_records("multi", f"{tag} gscale={gscale}", be, "multi", refs, [1.0] * n, gscale, False, False)
    for wk, gscale, extra, dextra in OBJECTIVE_FORMS:
        recs += _loss_records("objective", f"{tag} w={wk} gscale={gscale} extra={int(extra)} dextra={int(dextra)}", be, "objective", refs,
                              weights_for(wk, n), gscale, extra, dextra)
    return recs


# --------------------------------------------------------------------------------------------------------------- refusals
class Ptrs(list):
    """a host array of device pointers (const float* const*): tensors or None"""


class Floats(list):
    """a host array of floats (const float* weights)"""


# rpnet_refine_glue_supported(K, h, w, F, C, planes) -> the answer; every refusal row below that is about a shape is in here too
SUPPORTED = [((2, 8, 8, 64, 0, 0), 1), ((4, 24, 16, 64, 2048, 3), 1), ((2, 8, 8, 64, 8, 1), 1), ((3, 16, 8, 64, 256, 2), 1),
             ((2, 8, 8, 32, 0, 0), 0), ((1, 8, 8, 64, 0, 0), 0), ((5, 8, 8, 64, 0, 0), 0), ((2, 12, 8, 64, 0, 0), 0),
             ((2, 8, 4, 64, 0, 0), 0), ((2, 0, 8, 64, 0, 0), 0), ((2, 8, 8, 64, 64, 4), 0), ((2, 8, 8, 64, 12, 2), 0),
             ((2, 8, 8, 64, 24, 2), 0), ((2, 8, 8, 64, 4096, 2), 0), ((2, 8, 8, 64, 4096, 0), 1), ((2, 8, 8, 64, 64, -1), 0)]


def refusals(buf, ibuf):
    """[(label, entry point, args without the stream, expected rpnet_status)]: every call is refused on the host.  buf(n) -> a valid
    buffer of n floats, ibuf(n) of n int64: every pointer is valid (unless the row is about null) and large enough for what the call
    claims.  -> (rows, the float buffers that must come back unchanged)"""
    B, K, h, w = 1, 2, 8, 8
    big = 1 << 16
    y, sc, sh, proto, z, pred, lg, mk, x, xs, xk, xq = (buf(big) for _ in range(12))
    dl, f, df, dpr, ws = (buf(big) for _ in range(5))
    glue_ws = B * K * FEAT * 4                          # one patch: rpnet_refine_glue_bwd_workspace_bytes(1, 2, 8, 8, 64)

    def gf(y=y, sc=None, sh=None, proto=proto, z=None, pred=pred, lg=lg, mk=None, x=None, xs=None, xk=None, xq=None, planes=0, K=K, h=h,
           w=w, Fc=FEAT, C=0):
        return ("rpnet_refine_glue_fwd", (y, sc, sh, proto, SCALER, z, pred, lg, mk, 0, x, xs, xk, xq, planes, B, K, h, w, Fc, C))

    def gp(planes=2, C=64, **kw):                       # the form with operand planes, everything it needs given
        return gf(mk=mk, x=x, xs=xs, xk=xk, xq=xq, planes=planes, C=C, **kw)

    def gb(dl=dl, f=f, proto=proto, df=df, dpr=dpr, K=K, h=h, w=w, Fc=FEAT, ws=ws, wb=glue_ws):
        return ("rpnet_refine_glue_bwd", (dl, f, proto, SCALER, df, dpr, B, K, h, w, Fc, ws, wb))

    lab, loss, stats, gs, ex, dex, lws = ibuf(big), buf(64), buf(big), buf(4), buf(4), buf(4), buf(big)
    t = [buf(big) for _ in range(2)]
    d = [buf(big) for _ in range(2)]
    H = W = 4
    loss_ws = lambda n, K=2: n * B * 64 * (2 * K + 2) * 8                                                    # noqa: E731

    def mf(lgs=Ptrs(t), n=2, lab=lab, K=2, wb=None):
        return ("rpnet_dice_ce_multi_fwd", (lgs, n, lab, loss, stats, B, K, H, W, lws, loss_ws(n, K) if wb is None else wb))

    def of(lgs=Ptrs(t), wts=Floats([1.0, 2.0]), n=2, K=2, wb=None):
        return ("rpnet_objective_fwd", (lgs, wts, n, lab, ex, 0.5, loss, stats, B, K, H, W, lws, loss_ws(n, K) if wb is None else wb))

    def mb(lgs=Ptrs(t), dls=Ptrs(d), n=2, K=2, stats=stats):
        return ("rpnet_dice_ce_multi_bwd", (lgs, dls, n, lab, stats, gs, B, K, H, W))

    def ob(lgs=Ptrs(t), dls=Ptrs(d), wts=Floats([1.0, 2.0]), n=2, K=2):
        return ("rpnet_objective_bwd", (lgs, dls, wts, n, lab, stats, gs, dex, 0.5, B, K, H, W))

    many, zeros17 = Ptrs([t[0]] * 17), Floats([1.0] * 17)
    rows = [("F = 32", gf(Fc=32), SHAPE), ("K = 1", gf(K=1), SHAPE), ("K = 5", gf(K=5), SHAPE), ("h = 12", gf(h=12), SHAPE),
            ("w = 4", gf(w=4), SHAPE), ("h = 0", gf(h=0), SHAPE), ("planes 4", gp(planes=4), SHAPE), ("C = 12", gp(C=12), SHAPE),
            ("C = 24", gp(C=24), SHAPE), ("C = 4096", gp(C=4096), SHAPE),
            ("x without mask_next", gf(x=x, xs=xs, xk=xk, xq=xq, planes=2, C=64), ARG),
            ("bn_scale without shift", gf(sc=sc, z=z), ARG), ("bn_scale without z", gf(sc=sc, sh=sh), ARG),
            ("planes 2 without x_scale", gf(mk=mk, x=x, xk=xk, xq=xq, planes=2, C=64), ARG),
            ("planes without xk", gf(mk=mk, x=x, xs=xs, xq=xq, planes=2, C=64), ARG),
            ("planes without xq", gf(mk=mk, x=x, xs=xs, xk=xk, planes=2, C=64), ARG),
            ("null y", gf(y=None), ARG), ("null proto", gf(proto=None), ARG), ("null pred", gf(pred=None), ARG), ("null logits", gf(lg=None), ARG),
            ("F = 32", gb(Fc=32), SHAPE), ("K = 1", gb(K=1), SHAPE), ("K = 5", gb(K=5), SHAPE), ("h = 12", gb(h=12), SHAPE),
            ("w = 4", gb(w=4), SHAPE), ("h = 0", gb(h=0, wb=big), SHAPE), ("workspace one byte short", gb(wb=glue_ws - 1), WORKSPACE),
            ("null dlogits", gb(dl=None), ARG), ("null f", gb(f=None), ARG), ("null proto", gb(proto=None), ARG), ("null df", gb(df=None), ARG),
            ("null dproto", gb(dpr=None), ARG), ("null workspace", gb(ws=None), ARG),
            ("n = 0", mf(n=0), ARG), ("n = 17", mf(lgs=many, n=17), ARG), ("K = 1", mf(K=1), SHAPE), ("K = 5", mf(K=5), SHAPE),
            ("NULL in the pointer array", mf(lgs=Ptrs([t[0], None])), ARG), ("null pointer array", mf(lgs=None), ARG),
            ("null labels", mf(lab=None), ARG), ("workspace one byte short", mf(wb=loss_ws(2) - 1), WORKSPACE),
            ("n = 0", of(n=0), ARG), ("n = 17", of(lgs=many, wts=zeros17, n=17), ARG), ("K = 1", of(K=1), SHAPE), ("K = 5", of(K=5), SHAPE),
            ("NULL in the pointer array", of(lgs=Ptrs([None, t[1]])), ARG), ("NULL weights", of(wts=None), ARG),
            ("workspace one byte short", of(wb=loss_ws(2) - 1), WORKSPACE),
            ("n = 0", mb(n=0), ARG), ("n = 17", mb(lgs=many, dls=many, n=17), ARG), ("K = 1", mb(K=1), SHAPE), ("K = 5", mb(K=5), SHAPE),
            ("NULL in the logit array", mb(lgs=Ptrs([t[0], None])), ARG), ("NULL in the gradient array", mb(dls=Ptrs([None, d[1]])), ARG),
            ("null stats", mb(stats=None), ARG),
            ("n = 0", ob(n=0), ARG), ("n = 17", ob(lgs=many, dls=many, wts=zeros17, n=17), ARG), ("K = 1", ob(K=1), SHAPE),
            ("K = 5", ob(K=5), SHAPE), ("NULL in the gradient array", ob(dls=Ptrs([d[0], None])), ARG), ("NULL weights", ob(wts=None), ARG)]
    outputs = [z, pred, lg, mk, xk, xq, df, dpr, ws, loss, stats, dex, lws] + d
    return [(label, entry, args, code) for label, (entry, args), code in rows], outputs


def workspace_bytes(B, K, h, w):
    """rpnet_refine_glue_bwd_workspace_bytes, from the header: one [K][64] float row per 8 x 8 patch and episode"""
    return B * (h // 8) * (w // 8) * K * FEAT * 4


# ------------------------------------------------------------------------------------------- the float32 stand-in for the library
DEFECTS = ["halo_clamp", "taps_hw_swapped", "k4_class2_twice", "threshold_ge", "mask_15_taps", "xq_from_mask", "last_patch_dropped",
           "window_row_short", "total_ignores_weight", "grad_ignores_weight", "stats_stride_B", "skip_pixel_16384"]


def _gsum16(t):
    """group_sum<16>: lane l adds lane l ^ 8, then l ^ 4, l ^ 2, l ^ 1 (what lane 0 ends up with)"""
    for o in (8, 4, 2, 1):
        t = t[..., :o] + t[..., o:2 * o]
    return t[..., 0]


def _dot(a, b):
    """[..., 64] x [..., 64]: each of 16 lanes adds its four products in sequence, then the xor-shuffle sum over the lanes"""
    pr = a * b
    pr = pr.reshape(pr.shape[:-1] + (16, 4))
    return _gsum16(((pr[..., 0] + pr[..., 1]) + pr[..., 2]) + pr[..., 3])


def _taps(n_out, in_size, rscale):
    """bl_taps for every destination index, in float32"""
    src = (torch.tensor(rscale, dtype=F32) * (torch.arange(n_out, dtype=F32) + 0.5) - 0.5).clamp_min(0)
    i0 = src.to(torch.int64).clamp_max(in_size - 1)
    i1 = (i0 + 1).clamp_max(in_size - 1)
    w1 = src - i0.float()
    return i0, i1, 1 - w1, w1


def _weights(n_out, n_in):
    """[n_in, n_out]: bl_weight(d, s)"""
    i0, i1, w0, w1 = _taps(n_out, n_in, n_in / n_out)
    s = torch.arange(n_in)[:, None]
    return (s == i0[None]).float() * w0[None] + (s == i1[None]).float() * w1[None]


def _split(v, planes):
    """split8<NP>: 16-bit planes of v, each the round-to-nearest-even of what the planes before it left"""
    out = []
    for _ in range(planes):
        p = v.bfloat16() if planes == 3 else v.half()
        out.append(p.view(I16))
        v = v - p.float()
    return torch.stack(out)


class SimBackend:
    """A float32 torch restatement of the eight entry points, NOT the pairwise yardstick: dot products over 64 channels as 16 lanes
    of four sequential products and an xor-shuffle sum, the softmax denominator and the 16 taps of the mask average in sequence, the
    adjoint of the up-sampling in the kernel's row / column / lane order, the prototype gradient as four pixels per lane group, the
    sequential sum of 16 groups and the patch partials in cosine_dproto_final's order; the loss sums in float64 of float32 terms, as
    the kernels form them.  `defect`: one of DEFECTS."""

    def __init__(self, defect=None):
        assert defect is None or defect in DEFECTS
        self.defect = defect

    # ---- glue, forward
    def glue_fwd(self, y, scale, shift, proto, scaler, want_mask, soft, x, xs, planes):
        B, h, w, _ = y.shape
        K, H, W = proto.shape[1], 4 * h, 4 * w
        v = torch.relu(y * scale + shift) if scale is not None else y
        pn = torch.sqrt(_dot(proto, proto)).clamp_min(EPS)                                       # [B, K]
        nf = torch.sqrt(_dot(v, v)).clamp_min(EPS)                                               # [B, h, w]
        d = _dot(v[:, None], proto[:, :, None, None])                                            # [B, K, h, w]
        pred = torch.tensor(scaler, dtype=F32) * d / (nf[:, None] * pn[:, :, None, None])
        lds = pred.clone()                                                                       # pred_s: what stage B reads
        if self.defect == "k4_class2_twice" and K == 4:
            lds[:, 3] = lds[:, 2]
        if self.defect == "halo_clamp":                                                          # rows clamp at h - 2
            lds[:, :, h - 1] = lds[:, :, h - 2]
        swap = self.defect == "taps_hw_swapped"
        y0, y1, wy0, wy1 = _taps(H, w if swap else h, 0.25)
        x0, x1, wx0, wx1 = _taps(W, h if swap else w, 0.25)
        y0, y1, x0, x1 = y0.clamp_max(h - 1), y1.clamp_max(h - 1), x0.clamp_max(w - 1), x1.clamp_max(w - 1)   # beyond: the clamped halo
        r0, r1 = lds[:, :, y0], lds[:, :, y1]                                                    # [B, K, H, w]
        logits = (wy0[:, None] * (wx0 * r0[..., x0] + wx1 * r0[..., x1]) + wy1[:, None] * (wx0 * r1[..., x0] + wx1 * r1[..., x1]))
        out = {"z": v if scale is not None else None, "pred": pred, "logits": logits, "mask_next": None, "xk": None, "xq": None, "guards": 0}
        if not want_mask:
            return out
        mx = logits.amax(1)
        e = torch.exp(logits - mx[:, None])
        den = torch.zeros_like(mx)
        for k in range(K):
            den = den + e[:, k]
        p1 = e[:, 1] / den
        if not soft:
            p1 = ((p1 >= 0.5) if self.defect == "threshold_ge" else (p1 > 0.5)).float()
        cell = p1.reshape(B, h, 4, w, 4).permute(0, 1, 3, 2, 4).reshape(B, h, w, 16)
        acc = torch.zeros(B, h, w)
        for i in range(15 if self.defect == "mask_15_taps" else 16):
            acc = acc + cell[..., i]
        m = acc / 16.0
        out["mask_next"] = m
        if x is None:
            return out
        f1 = m[..., None]
        f2 = torch.tensor(1.0, dtype=F32) - f1
        vk, vq = x * f1, x * (f1 if self.defect == "xq_from_mask" else f2)
        if planes <= 2:
            inv = torch.tensor(1.0, dtype=F32) / torch.tensor(xs, dtype=F32)
            vk, vq = vk * inv, vq * inv
        out["xk"], out["xq"] = _split(vk, planes), _split(vq, planes)
        return out

    # ---- glue, backward
    def _dps(self, dl, h, w):
        """the adjoint of the up-sampling [B, K, h, w]: a lane takes every fourth row of the window, adds a row's columns in sequence"""
        B, K, H, W = dl.shape
        Wy, Wx = _weights(H, h), _weights(W, w)
        ys, xs = torch.arange(h), torch.arange(w)
        Y0, Y1 = (4 * ys - 5).clamp_min(0), (4 * ys + (4 if self.defect == "window_row_short" else 9)).clamp_max(H - 1)
        X0, X1 = (4 * xs - 5).clamp_min(0), (4 * xs + 9).clamp_max(W - 1)
        row = torch.zeros(B, K, H, w)
        for c in range(15):
            X = X0 + c
            ok, Xc = X <= X1, X.clamp_max(W - 1)
            row = torch.where(ok, row + dl[..., Xc] * Wx[xs, Xc], row)
        parts = []
        for part in range(4):
            acc = torch.zeros(B, K, h, w)
            for r in range(4):
                Y = Y0 + part + 4 * r
                Yc = Y.clamp_max(H - 1)
                wy = torch.where(Y <= Y1, Wy[ys, Yc], torch.zeros(h))
                acc = torch.where((wy != 0)[:, None], acc + wy[:, None] * row[:, :, Yc], acc)
            parts.append(acc)
        return (parts[0] + parts[1]) + (parts[2] + parts[3])

    def glue_bwd(self, dl, f, proto, scaler):
        B, h, w, _ = f.shape
        K = proto.shape[1]
        dps = self._dps(dl, h, w)
        one, sc = torch.tensor(1.0, dtype=F32), torch.tensor(scaler, dtype=F32)
        pn_raw = torch.sqrt(_dot(proto, proto))                                                  # [B, K]
        pn_c = pn_raw.clamp_min(EPS)
        pnrm = proto * (one / pn_c)[..., None]
        nf = torch.sqrt(_dot(f, f))                                                              # [B, h, w]
        nfc = nf.clamp_min(EPS)
        inv = (one / nfc)[..., None]
        fn = f * inv
        g = torch.zeros_like(f)
        add, sub = [], []
        for k in range(K):
            go = sc * dps[:, k]                                                                  # [B, h, w]
            pk, pnk = proto[:, k, None, None], pnrm[:, k, None, None]                            # [B, 1, 1, 64]
            fp = _dot(f, pnk)
            g = g + go[..., None] * (pnk * inv)
            g = torch.where((nf > EPS)[..., None], g - (go * fp / (nfc * nfc * nf))[..., None] * f, g)
            fnp = _dot(fn, pk)
            pc, pr = pn_c[:, k, None, None], pn_raw[:, k, None, None]
            add.append(go[..., None] * (fn * (one / pc)[..., None]))
            sub.append(torch.where((pr > EPS)[..., None], (go * fnp / (pc * pc * pr))[..., None] * pk, torch.zeros_like(f)))
        # per patch: lane group pl = pix % 16 takes pixels pl, pl + 16, pl + 32, pl + 48; then the 16 groups in sequence
        th, tw = h // 8, w // 8
        patches = lambda t: (torch.stack(t, 1).reshape(B, K, th, 8, tw, 8, FEAT).permute(0, 2, 4, 1, 3, 5, 6)          # noqa: E731
                             .reshape(B, th * tw, K, 4, 16, FEAT))
        a, s = patches(add), patches(sub)
        dp = torch.zeros(B, th * tw, K, 16, FEAT)
        for step in range(4):
            dp = (dp + a[:, :, :, step]) - s[:, :, :, step]
        dpart = dp[:, :, :, 0]
        for grp in range(1, 16):
            dpart = dpart + dp[:, :, :, grp]
        nblk = th * tw - (1 if self.defect == "last_patch_dropped" else 0)
        red = []
        for part in range(4):                       # cosine_dproto_final at C = 64: four parts, each with four running sums
            s4, j = [torch.zeros(B, K, FEAT) for _ in range(4)], part
            while j + 12 < nblk:
                for q in range(4):
                    s4[q] = s4[q] + dpart[:, j + 4 * q]
                j += 16
            while j < nblk:
                s4[0] = s4[0] + dpart[:, j]
                j += 4
            red.append((s4[0] + s4[1]) + (s4[2] + s4[3]))
        dproto = red[0]
        for q in range(1, 4):
            dproto = dproto + red[q]
        return g, dproto, 0

    # ---- loss
    def _softmax(self, lg):
        K = lg.shape[1]
        mx = lg.amax(1)
        e = torch.exp(lg - mx[:, None])
        den = torch.zeros_like(mx)
        for k in range(K):
            den = den + e[:, k]
        return e / den[:, None], mx, den

    def loss_fwd(self, kind, logits, weights, labels, extra, extra_scale):
        n = len(logits)
        B, K, H, W = logits[0].shape
        S = 2 * K + 2
        flat = torch.full((n * (B + 1) * S,), float("nan"))
        loss = torch.full((n + 1,), float("nan"))
        oh = torch.eye(K)[labels].permute(0, 3, 1, 2)
        keep = torch.ones(H * W, dtype=F64)
        if self.defect == "skip_pixel_16384" and H * W > 16384:
            keep[16384] = 0
        total = 0.0
        for z, lg in enumerate(logits):
            p, mx, den = self._softmax(lg)
            ce = (mx + torch.log(den)) - lg.gather(1, labels[:, None])[:, 0]
            sums = torch.cat([((p * oh).double().reshape(B, K, -1) * keep).sum(-1), ((p + oh).double().reshape(B, K, -1) * keep).sum(-1),
                              (ce.double().reshape(B, -1) * keep).sum(-1, keepdim=True), keep.sum().expand(B, 1)], 1)      # [B, S]
            tot = sums.sum(0)
            stride = B * S if self.defect == "stats_stride_B" else (B + 1) * S
            flat[z * stride:z * stride + (B + 1) * S] = torch.cat([sums, tot[None]]).float().reshape(-1)
            l64 = tot[2 * K] / tot[2 * K + 1] + 1.0 - (2.0 * tot[:K] / (tot[K:2 * K] + 1e-7)).sum() / K
            loss[z] = l64.float()
            wz = 1.0 if (kind == "multi" or self.defect == "total_ignores_weight") else float(torch.tensor(weights[z], dtype=F32))
            total = total + wz * float(loss[z])
        tt = torch.tensor(total, dtype=F64).float()
        if extra is not None and kind == "objective":
            tt = tt + torch.tensor(extra_scale, dtype=F32) * extra[0]
        loss[n] = tt
        return loss, flat.reshape(n, B + 1, S), 0

    def loss_bwd(self, kind, logits, weights, labels, stats, gscale, want_dextra, extra_scale):
        B, K, H, W = logits[0].shape
        g0 = torch.tensor(1.0 if gscale is None else gscale, dtype=F32)
        oh = torch.eye(K)[labels].permute(0, 3, 1, 2)
        grads = []
        for z, lg in enumerate(logits):
            wz = 1.0 if (kind == "multi" or self.defect == "grad_ignores_weight") else weights[z]
            gs = g0 * torch.tensor(wz, dtype=F32)
            st = stats[z]
            ce_coef = 1.0 / st[B, 2 * K + 1]
            I, Cc = st[B, :K], st[B, K:2 * K] + torch.tensor(1e-7, dtype=F32)
            a_off = (torch.tensor(2.0 / K, dtype=F32)) * I / (Cc * Cc)
            a_on = a_off - torch.tensor(2.0 / K, dtype=F32) / Cc
            p, _, _ = self._softmax(lg)
            a = torch.where(oh > 0, a_on[None, :, None, None], a_off[None, :, None, None])
            ap = torch.zeros(B, H, W)
            for k in range(K):
                ap = ap + a[:, k] * p[:, k]
            g = p * (a - ap[:, None]) + ce_coef * (p - oh)
            grads.append(g * gs)
        dextra = (g0 * torch.tensor(extra_scale, dtype=F32)).reshape(1) if want_dextra else None
        return grads, dextra, 0
