"""CPU self-check of tests/glue_cases.py: (1) the bound has room for a correct float32 implementation — SimBackend, a torch
restatement that sums in the kernels' order, passes every arithmetic case of the tables; (2) the checks see what they are there to
see — each seeded defect of glue_cases.DEFECTS fails them, by the printed multiple of the bound; (3) every hard-mask case keeps its
undecided cells within the cap, from the references alone; (4) the ref64 compositions are the reference's operator sequence
(F.interpolate, softmax, avg_pool2d, autograd) in float64.  A defect the checks cannot see means the checks are changed, not the list."""
import inspect

import pytest
import torch
import torch.nn.functional as F

from tests import glue_cases as GC
from tests import ref64 as R
from tests.helpers import rel_err, rnd

SIM = GC.SimBackend()
F64 = torch.float64


@pytest.fixture(autouse=True, scope="module")
def _one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def run(family, rows, check):
    recs = []
    for row in rows:
        recs += check(*row)
    GC.hold(recs, verbose=False)
    arith = [r for r in recs if not r.exact]
    top = max(arith, key=lambda r: r.ratio)
    print(f"{family}: {len(rows)} cases, {len(recs)} checks, largest ratio {top.ratio:.2f} ({top.family} {top.what}), "
          f"largest multiple of the bound {max(r.multiple for r in arith):.2f}")
    return recs


def test_the_bound_is_the_small_ops_convention():
    from tests import test_gpu_small_ops as S
    assert GC.FLOOR == S.FLOOR and GC.FACTOR == inspect.signature(S.hold).parameters["factor"].default
    assert (GC.SHAPE, GC.ARG, GC.WORKSPACE) == (S.SHAPE, S.ARG, S.WORKSPACE)
    assert all(f >= GC.FACTOR for f in GC.MEASURED_FACTORS.values())


def test_tables_hold_what_they_are_there_for():
    assert all(h % 8 == 0 and w % 8 == 0 and h >= 8 and w >= 8 for _, _, h, w in GC.GLUE_SHAPES)
    assert {K for _, K, _, _ in GC.GLUE_SHAPES} == {2, 3, 4} and max(B for B, _, _, _ in GC.GLUE_SHAPES) > 3
    assert {(p, C) for _, _, _, p, C in GC.GLUE_PLANE_CASES} == {(p, C) for p in (1, 2, 3) for C in (8, 64, 256, 2048)}
    assert any(not bn and m for _, bn, m, _, _ in GC.GLUE_PLANE_CASES) and any(K > 2 for (_, K, _, _), *_ in GC.GLUE_PLANE_CASES)
    hw = {H * W for _, _, _, H, W, _, _ in GC.LOSS_ROWS}
    assert {35, 16383, 16385} <= hw and any(-(-v // 256) > 256 for v in hw)
    assert {n for n, *_ in GC.LOSS_ROWS} >= {1, 2, 16} and {K for _, _, K, *_ in GC.LOSS_ROWS} == {2, 3, 4}
    assert {B for _, B, *_ in GC.LOSS_ROWS} >= {1, 3, 8} and any(r[5] is not None for r in GC.LOSS_ROWS) and any(r[6] for r in GC.LOSS_ROWS)
    forms = GC.OBJECTIVE_FORMS
    assert {f[0] for f in forms} == set(GC.WEIGHTS) and {f[1] for f in forms} == {None, 0.37}
    assert {(f[2], f[3]) for f in forms} == {(True, True), (True, False), (False, True), (False, False)}
    for (K, h, w, Fc, C, planes), want in GC.SUPPORTED:         # the rule of csrc/refine.hip, restated
        ok = Fc == 64 and 2 <= K <= 4 and h % 8 == 0 and w % 8 == 0 and h >= 8 and w >= 8
        ok = ok and (planes == 0 or (1 <= planes <= 3 and C % 8 == 0 and C // 8 <= 256 and 256 % (C // 8) == 0))
        assert int(ok) == want, (K, h, w, Fc, C, planes)


def test_undecided_cells_stay_within_the_cap():
    """for every hard-mask case, from the float64 and float32 references alone: change the seed of a row that breaks it, never the cap"""
    cases = {(s, bn) for s, bn, m, _, _ in GC.GLUE_FWD_CASES + GC.GLUE_PLANE_CASES if m == "hard"}
    for shape, bn in sorted(cases):
        share = GC.undecided_share(shape, bn)
        print(f"undecided share {shape} bn={bn}: {share:.4f}")
        assert share <= GC.UNDECIDED_SHARE, (shape, bn, share)


def test_ref64_compositions_are_the_operator_sequence():
    """refine_glue / refine_glue_bwd against F.normalize-free torch: cosine_similarity, F.interpolate, softmax, avg_pool2d and
    autograd through the whole chain in float64; dice_ce_stats and objective against their definitions"""
    B, K, h, w = 2, 3, 8, 16
    y, scale, shift, proto = GC.glue_inputs((B, K, h, w), True)
    y[GC.ZERO_PIXEL] = rnd(5, 64)                       # no zero vector: its gradient is 1 / eps-scaled
    yd, pd = y.double().requires_grad_(True), proto.double().requires_grad_(True)
    z = torch.relu(yd * scale.double() + shift.double())
    pred = F.cosine_similarity(z.permute(0, 3, 1, 2)[:, None], pd[..., None, None], dim=2, eps=1e-8) * GC.SCALER
    logits = F.interpolate(pred, size=(4 * h, 4 * w), mode="bilinear", align_corners=False)
    p1 = torch.softmax(logits, 1)[:, 1]
    soft, hard = F.avg_pool2d(p1[:, None], 4)[:, 0], F.avg_pool2d((p1 > 0.5).double()[:, None], 4)[:, 0]
    rs, rh = R.refine_glue(y, scale, shift, proto, GC.SCALER, True), R.refine_glue(y, scale, shift, proto, GC.SCALER, False)
    for got, want in ((rs[0], z), (rs[1], pred), (rs[2], logits), (rs[3], soft)):
        assert rel_err(got, want.detach()) < 1e-13
    assert torch.equal(rh[3], hard)
    dl = rnd(6, B, K, 4 * h, 4 * w)
    zl = z.detach().requires_grad_(True)
    lg2 = F.interpolate(F.cosine_similarity(zl.permute(0, 3, 1, 2)[:, None], pd[..., None, None], dim=2, eps=1e-8) * GC.SCALER,
                        size=(4 * h, 4 * w), mode="bilinear")
    gz, gp = torch.autograd.grad(lg2, (zl, pd), dl.double())
    df, dproto = R.refine_glue_bwd(dl, z.detach(), proto, GC.SCALER)
    assert rel_err(df, gz) < 1e-12 and rel_err(dproto, gp) < 1e-12
    assert R.refine_glue(y, None, None, proto)[0] is not None and torch.equal(R.refine_glue(y, None, None, proto)[0], y.double())
    # loss
    lg, lab = rnd(7, 3, 4, 6, 5) * 2, torch.randint(0, 4, (3, 6, 5), generator=torch.Generator().manual_seed(3))
    st = R.dice_ce_stats(lg, lab)
    Kc = 4
    dice = 1 - (2 * st[-1, :Kc] / (st[-1, Kc:2 * Kc] + 1e-7)).mean()
    assert abs(float(st[-1, 2 * Kc] / st[-1, 2 * Kc + 1] + dice - R.dice_ce(lg, lab))) < 1e-13
    assert torch.equal(st[:-1].sum(0), st[-1]) and st[0, -1] == 30
    ls, tot = R.objective([lg, lg * 0.5], [2.0, 0.25], lab, torch.tensor([3.0]), 0.5)
    assert abs(float(tot) - (2.0 * float(ls[0]) + 0.25 * float(ls[1]) + 1.5)) < 1e-13
    lgd = lg.double().requires_grad_(True)          # the gradient of g0 * w_z * loss_z is g0 * w_z * dice_ce_bwd
    (gd,) = torch.autograd.grad(0.37 * 2.0 * R._dice_ce(lgd, lab, 1, -1, 0, None), lgd)
    assert rel_err(0.37 * 2.0 * R.dice_ce_bwd(lg, lab), gd) < 1e-13


def test_glue_forward_cases():
    run("glue forward", GC.GLUE_FWD_CASES, lambda *c: GC.check_glue_fwd(SIM, *c))
    run("glue forward with planes", GC.GLUE_PLANE_CASES, lambda *c: GC.check_glue_fwd(SIM, *c))
    GC.hold(GC.check_glue_tie(SIM), verbose=False)


def test_glue_backward_cases():
    run("glue backward", GC.GLUE_BWD_CASES, lambda *c: GC.check_glue_bwd(SIM, *c))
    run("glue zero patch", [(s,) for s in GC.ZERO_PATCH_SHAPES], lambda s: GC.check_glue_zero_patch(SIM, s))


def test_loss_cases():
    run("loss", [(r,) for r in GC.LOSS_ROWS], lambda r: GC.check_loss_row(SIM, r))


def test_refusal_table_is_well_formed():
    rows, outputs = GC.refusals(lambda n: torch.full((n,), 7.0), lambda n: torch.zeros(n, dtype=torch.int64))
    entries = {e for _, e, _, _ in rows}
    assert entries == {"rpnet_refine_glue_fwd", "rpnet_refine_glue_bwd", "rpnet_dice_ce_multi_fwd", "rpnet_dice_ce_multi_bwd",
                       "rpnet_objective_fwd", "rpnet_objective_bwd"}
    assert {c for _, _, _, c in rows} == {GC.SHAPE, GC.ARG, GC.WORKSPACE}
    from rpnet_amd import hip
    for _, entry, args, _ in rows:
        assert len(args) + 1 == len(hip._SIGS[entry][1]), entry
    assert GC.workspace_bytes(1, 2, 8, 8) == 512 and GC.workspace_bytes(3, 2, 16, 24) == 3 * 6 * 2 * 64 * 4


# the cases each defect is looked for in: the smallest of the tables that can show it
DEFECT_CASES = {
    "halo_clamp": lambda be: GC.check_glue_fwd(be, (1, 2, 8, 8), True, None),
    "taps_hw_swapped": lambda be: GC.check_glue_fwd(be, (2, 3, 16, 8), True, None),
    "k4_class2_twice": lambda be: GC.check_glue_fwd(be, (1, 4, 8, 8), False, "hard"),
    "threshold_ge": lambda be: GC.check_glue_tie(be),
    "mask_15_taps": lambda be: GC.check_glue_fwd(be, (1, 2, 8, 8), True, "hard") + GC.check_glue_fwd(be, (1, 2, 8, 8), False, "soft"),
    "xq_from_mask": lambda be: GC.check_glue_fwd(be, (2, 3, 16, 8), True, "soft", 3, 8) + GC.check_glue_fwd(be, (2, 3, 16, 8), True, "hard", 2, 64),
    "last_patch_dropped": lambda be: GC.check_glue_bwd(be, (2, 3, 8, 16), "random") + GC.check_glue_zero_patch(be, (1, 4, 24, 16)),
    "window_row_short": lambda be: GC.check_glue_bwd(be, (1, 2, 8, 8), "random") + GC.check_glue_bwd(be, (1, 2, 8, 8), "ring"),
    "total_ignores_weight": lambda be: GC.check_loss_row(be, GC.LOSS_ROWS[6]),
    "grad_ignores_weight": lambda be: GC.check_loss_row(be, GC.LOSS_ROWS[6]),
    "stats_stride_B": lambda be: GC.check_loss_row(be, GC.LOSS_ROWS[1]),
    "skip_pixel_16384": lambda be: GC.check_loss_row(be, GC.LOSS_ROWS[2]),
}


def test_every_defect_has_its_cases():
    assert sorted(DEFECT_CASES) == sorted(GC.DEFECTS)


@pytest.mark.parametrize("defect", GC.DEFECTS)
def test_seeded_defect_fails_the_checks(defect):
    GC.hold(DEFECT_CASES[defect](SIM), verbose=False)                     # the same cases pass without the defect
    recs = DEFECT_CASES[defect](GC.SimBackend(defect))
    bad = [r for r in recs if not r.ok]
    assert bad, f"{defect}: no check failed"
    arith = [r for r in bad if not r.exact]
    top = max(arith, key=lambda r: r.multiple) if arith else None
    print(f"DEFECT {defect}: {len(bad)} of {len(recs)} checks fail"
          + (f", the worst by {top.multiple:.3g} x its bound ({top.family} {top.what})" if top else "")
          + (f", {sum(r.exact for r in bad)} exact checks among them" if any(r.exact for r in bad) else ""))
    with pytest.raises(AssertionError):
        GC.hold(recs, verbose=False)
