"""CPU self-check of tests/corr_cases.py: (1) the bound has room for a correct float32 implementation — SimBackend, a torch
restatement that sums in the kernels' order, not torch's pairwise one, passes every arithmetic case of the tables; (2) the
checks see what they are there to see — each seeded defect of corr_cases.DEFECTS fails them, by the printed multiple of the
bound.  A defect the checks cannot see means the checks are changed, not the list."""
import inspect

import pytest
import torch

from tests import corr_cases as CC
from tests import ref64 as R
from tests.helpers import rnd

SIM = CC.SimBackend()


@pytest.fixture(autouse=True, scope="module")
def _one_thread():
    """thousands of operators on tensors of a few hundred elements: torch's thread pool costs more than it gives"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def run(family, rows, check):
    recs = []
    for row in rows:
        recs += check(*row)
    CC.hold(recs, verbose=False)
    top = max((r for r in recs if not r.exact), key=lambda r: r.ratio)
    print(f"{family}: {len(rows)} cases, {len(recs)} checks, largest ratio {top.ratio:.2f} ({top.family} {top.what}), "
          f"largest multiple of the bound {max(r.multiple for r in recs if not r.exact):.2f}")


def test_the_bound_is_the_small_ops_convention():
    from tests import test_gpu_small_ops as S
    assert CC.FLOOR == S.FLOOR and CC.FACTOR == inspect.signature(S.hold).parameters["factor"].default
    assert (CC.SHAPE, CC.ARG, CC.WORKSPACE) == (S.SHAPE, S.ARG, S.WORKSPACE)


def test_split_planes_represent_their_operand():
    x = rnd(3, 4, 5, 64) * 7
    assert torch.equal(CC.plane_values(CC.split_planes(x, 3)), x.double())                   # three bf16 planes: exact
    s = CC.pow2_scale(x.abs().max())
    assert 2.0 ** 14 < float(x.abs().max()) / s <= 2.0 ** 15
    for planes, u in ((2, CC.split_unit_roundoff(2)), (1, CC.split_unit_roundoff(1))):
        v = CC.plane_values(CC.split_planes(x, planes, s), s)
        assert 0 < (v - x.double()).abs().max() <= u * x.abs().max()
    assert CC.pow2_scale(0.0) == 2.0 ** -100 and CC.pow2_scale(1.0) == 2.0 ** -15 and CC.pow2_scale(1.5) == 2.0 ** -14


def test_transpose_window_is_the_adjoint_view():
    """sum_p dcorr[p, o] f1[p] f2[p + off(o)] = sum_q dcT[q, o] f1[q - off(o)] f2[q]: d f2 of the reference is the SIGN = -1 pass"""
    f1, f2, dc = rnd(5, 2, 9, 11, 8), rnd(6, 2, 9, 11, 8), rnd(7, 2, 9, 11, 49)
    d2 = SIM._pass(CC.transpose_window(dc.double(), 3), f1.double(), 3, -1) / 8 ** 0.5
    assert CC.rel_err(d2, R.local_corr_bwd(f1, f2, dc, 3)[1]) < 1e-12


def test_fp32_cases():
    run("fp32", CC.FP32_CASES, lambda *c: CC.check_fp32(SIM, *c))
    run("fp32 forward only", CC.FP32_FWD_ONLY, lambda *c: CC.check_fp32(SIM, *c, backward=False))


def test_split_forward_cases():
    run("split forward", CC.SPLIT_FWD_CASES, lambda *c: CC.check_split_fwd(SIM, *c))


def test_split_backward_cases():
    run("split backward", CC.SPLIT_BWD_CASES, lambda *c: CC.check_split_bwd(SIM, *c))


def test_dynamic_range_and_cross_path():
    run("dynamic range", CC.DYNAMIC_CASES, lambda *c: [CC.check_dynamic_range(SIM, *c)[i] for i in (0, 1)])
    CC.hold(CC.check_cross_path(SIM), verbose=False)


# the cases each defect is looked for in: the smallest of the tables that can show it
DEFECT_CASES = {
    "swap_ac": lambda be: CC.check_fp32(be, 1, (1, 3, 5, 64), 9) + CC.check_split_fwd(be, 3, (1, 3, 5), 32, 121),
    "right_border": lambda be: CC.check_fp32(be, 2, (3, 9, 17, 64), 25, backward=False) + CC.check_fp32(be, 7, (2, 9, 1, 64), 225, backward=False),
    "no_inv_sqrt_c": lambda be: CC.check_fp32(be, 1, (1, 1, 1, 64), 9, backward=False),
    "unmirrored": lambda be: CC.check_fp32(be, 1, (1, 1, 9, 64), 9) + CC.check_split_bwd(be, 3, (1, 3, 5), 128, 121),
    "no_df1_add": lambda be: CC.check_fp32(be, 3, (2, 8, 8, 64), 49) + CC.check_split_bwd(be, 1, (2, 8, 8), 128, 128),
    "lowest_plane": lambda be: CC.check_split_fwd(be, 3, (3, 9, 17), 128, 128) + CC.check_split_bwd(be, 3, (3, 9, 17), 128, 128),
    "neighbour_scale": lambda be: CC.check_dynamic_range(be, 2, 256) + CC.check_dynamic_range(be, 1, 256),
}


def test_every_defect_has_its_cases():
    assert sorted(DEFECT_CASES) == sorted(CC.DEFECTS)


@pytest.mark.parametrize("defect", CC.DEFECTS)
def test_seeded_defect_fails_the_checks(defect):
    CC.hold(DEFECT_CASES[defect](SIM), verbose=False)                     # the same cases pass without the defect
    recs = DEFECT_CASES[defect](CC.SimBackend(defect))
    bad = [r for r in recs if not r.ok]
    assert bad, f"{defect}: no check failed"
    arith = [r for r in bad if not r.exact]
    top = max(arith, key=lambda r: r.multiple) if arith else None
    print(f"DEFECT {defect}: {len(bad)} of {len(recs)} checks fail"
          + (f", the worst by {top.multiple:.3g} x its bound ({top.family} {top.what})" if top else "")
          + (f", {sum(r.exact for r in bad)} exact checks among them" if any(r.exact for r in bad) else ""))
    with pytest.raises(AssertionError):
        CC.hold(recs, verbose=False)


def test_the_whole_tensor_error_cannot_see_the_wrong_tile():
    """why the dynamic-range case is judged per tile: with tile (0, 0, 0) on its neighbour's scale the max-abs-over-max-abs error
    of the whole tensor stays inside the bound"""
    planes, C = 2, 256
    shape = (2, 16, 16, C)
    seed = CC.case_seed(planes, C, 77)
    p1, p2, s1, s2 = CC.make_operands(seed, shape, planes)
    v1, v2 = CC.plane_values(p1, s1), CC.plane_values(p2, s2)
    dcorr = CC.dynamic_dcorr(seed + 2, 128)
    df1, _ = CC.SimBackend("neighbour_scale").split_bwd(p1, p2, s1, s2, dcorr, planes, shape, 128, None)
    g1, q1 = R.local_corr_bwd(v1, v2, dcorr, 5)[0], R.local_corr_bwd(v1, v2, dcorr, 5, dtype=torch.float32)[0]
    x1 = CC.split_term(dcorr, v2, 5, planes)
    assert CC.measure("x", "df1", df1, g1, q1, extra=x1).ok and not CC.per_tile("x", "df1", df1, g1, q1, extra=x1).ok
