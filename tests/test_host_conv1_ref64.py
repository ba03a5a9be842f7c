"""The bound and the tables of tests/conv1_cases.py on the CPU: SimBackend, a float32 restatement of the first-layer entry points
(y by the kernels' own chain of fused multiply-adds), passes every check of every table row with the plain bound and leaves no element
of the ReLU switch undecided for any row's seed, and each seeded defect fails the check named beside it."""
import os
import re

import pytest
import torch

from tests import conv1_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = open(os.path.join(ROOT, "rpnet_amd", "csrc", "conv_first.hip")).read()


def test_the_bound_is_the_small_ops_yardstick():
    import inspect
    from tests import test_gpu_small_ops as S
    assert K.FLOOR == S.FLOOR and K.FACTOR == inspect.signature(S.hold).parameters["factor"].default
    assert K.UNDECIDED == 4 * 2.0 ** -24 and not K.MEASURED_FACTORS


def test_every_row_names_the_kernel_the_launcher_takes():
    ids = [r.id for r in K.ALL_ROWS]
    assert len(set(ids)) == len(ids)
    for r in K.ALL_ROWS + K.CAPS:
        assert K.route(r) == r.kernel, (r.id, K.route(r), r.kernel)
    # every kernel of the file is named by a row here or by the rpnet_conv1_wgrad rows of tests/wgrad_cases.py
    from tests import wgrad_cases as WC
    assert K.kernels_named(K.ALL_ROWS) == set(K.KERNELS)
    forms = {K.strips_ok(c.N, c.H, c.W, 1) for c in WC.CONV1}
    assert forms == {True, False} and len(K.KERNELS_OF_WGRAD_CASES) == 2
    for name in K.KERNELS + K.KERNELS_OF_WGRAD_CASES:
        base, _, targs = name.partition("<")
        assert re.search(r"\b%s\b" % base, SOURCE), name
    # ... and the file holds no kernel beside them
    assert set(re.findall(r"__global__[^;{]*?void (\w+)\(", SOURCE)) == {n.partition("<")[0] for n in K.KERNELS + K.KERNELS_OF_WGRAD_CASES}


def test_the_constants_are_the_sources():
    assert f"kConv1WgradBlocks = {K.WGRAD_BLOCKS}" in SOURCE and f"nb > {K.FWD_BLOCKS}" in SOURCE and f"nb > {K.BN_RELU_BLOCKS}" in SOURCE
    assert f"nb > {K.STATS_CAP} ? {K.STATS_CAP}" in SOURCE and f"(per_group + {K.STATS_PIXELS - 1}) / {K.STATS_PIXELS}" in SOURCE


def test_the_edges_stated_beside_the_rows():
    sb = K.stats_blocks
    assert sb(3, 37, 21, 1) == 5 and 2331 - 4 * 467 == 463                          # chunk = ceil(2331 / 5) = 467
    assert sb(3, 37, 21, 3) == 2 and sb(1, 25, 41, 1) == 3 and sb(2, 16, 24, 1) == 2 and sb(4, 8, 8, 3) == 0
    assert sb(1, 1024, 1028, 1) == K.STATS_CAP < -(-1024 * 1028 // 512)              # the cap row of the fused statistics
    assert K.blocks(K.CAP_WGRAD) == (1, 256, K.WGRAD_BLOCKS) and -(-512 * 516 // 256) > K.WGRAD_BLOCKS
    q, ppb, nb = K.blocks(K.CAP_WRAP)
    assert (q, ppb, nb) == (256, 1, K.FWD_BLOCKS) and K.CAP_WRAP.M > K.FWD_BLOCKS and K.CAP_WRAP.M * 1024 > 2 ** 24
    # threads per pixel 1 .. 256 and pixels (strips) per block 256 .. 1 across the channel counts of the forward table
    assert sorted({K.blocks(r)[:2] for r in K.FWD}) == [(1, 256), (4, 64), (16, 16), (64, 4), (256, 1)]
    assert {r.cout for r in K.BN_RELU} == {8, 64, 1024} and {r.cout for r in K.WGRAD_BN} == {4, 64, 256}
    assert {r.cout for r in K.DGRAD_BN if r.y == "given"} == {32, 96, 160, 256} and {r.cout for r in K.DGRAD_BN if r.y == "null"} == {32, 64, 128, 256}
    assert not K.fwd_accepts(96) and not K.fwd_accepts(160)
    # a group whose pixel count is no multiple of a block's pixels, and a statistic-group boundary inside a block's range
    assert any(r.Mg % K.blocks(r)[1] for r in K.BWD_PARTIAL if r.groups > 1)
    for N, H, W in K.IMPULSE_SHAPES[:2]:
        assert K.strips_ok(N, H, W, 1)
    assert not K.strips_ok(*K.IMPULSE_SHAPES[2], 1)


@pytest.mark.parametrize("r", K.ALL_ROWS, ids=lambda r: r.id)
def test_a_correct_float32_implementation_is_inside_the_plain_bound(r):
    K.hold(K.check_row(K.SimBackend(), r), verbose=False)


@pytest.mark.parametrize("r", [r for r in K.ALL_ROWS if r.entry in ("bwd_partial", "wgrad_bn", "dgrad_bn")], ids=lambda r: r.id)
def test_no_element_of_the_relu_switch_is_undecided(r):
    """... with four times the margin: the y of the library differs from the restatement's only where a double rounding does"""
    o = K.operands(r)
    y = K.kernel_y(K.SimBackend(), r, o)
    assert K.undecided(y, o.stats, r.groups, 4 * K.UNDECIDED) == 0, (r.id, r.seed)


@pytest.mark.parametrize("r", K.CAPS, ids=lambda r: r.id)
def test_the_cap_rows_of_a_correct_implementation(r):
    K.hold(K.check_cap(K.SimBackend(), r), verbose=False)
    if r.entry == "wgrad_bn":
        o = K.operands(r)
        assert K.undecided(K.kernel_y(K.SimBackend(), r, o), o.stats, r.groups, 4 * K.UNDECIDED) == 0


def test_the_impulses_of_a_correct_implementation():
    be = K.SimBackend()
    for nhw in K.IMPULSE_SHAPES:
        K.hold(K.check_impulses(be, nhw), verbose=False)
    K.hold(K.check_dgrad_impulses(be), verbose=False)


def _row(table, **kw):
    (r,) = [r for r in table if all(getattr(r, k) == v for k, v in kw.items())]
    return r


_S, _P = dict(N=4, H=8, W=8, groups=2, cout=64), dict(N=2, H=7, W=5, groups=2, cout=64)
# defect -> (the check that must fail, a word of its record)
SEEDED = {
    "strip_right_edge": (lambda be: K.check_impulses(be, (2, 3, 8)), "impulse at image 0 pixel 1,0"),
    "row_minus1_at_0": (lambda be: K.check_impulses(be, (2, 3, 4)), "impulse at image 0 pixel 0,3"),
    "no_bias_again": (lambda be: K.check_wgrad_bn(be, _row(K.WGRAD_BN, y="null", **_P)), "dW with y == NULL is dW with y given"),
    "group_from_block": (lambda be: K.check_bn_relu(be, _row(K.BN_RELU, N=3, H=37, W=21, groups=3)), "z of rpnet_bn_relu"),
    "mask_from_y": (lambda be: K.check_bwd_partial(be, _row(K.BWD_PARTIAL, **_S)), "sum dz m over a group's rows"),
    "swap_c1c2": (lambda be: K.check_wgrad_bn(be, _row(K.WGRAD_BN, y="given", **_S)), "dW per tap"),
    "xhat_no_invstd": (lambda be: K.check_bwd_partial(be, _row(K.BWD_PARTIAL, **_P)), "sum dz m xhat over a group's rows"),
    "stale_row": (lambda be: K.check_fwd(be, _row(K.FWD, N=3, H=37, W=21, groups=1, cout=64)), "sum y over a group's rows"),
    "drop_low_plane": (lambda be: K.check_bn_relu(be, _row(K.BN_RELU, **_S)), "the planes represent z within split_unit_roundoff"),
    "absmax_overwrite": (lambda be: K.check_fwd(be, _row(K.FWD, **_S)), "a larger out_absmax is left alone"),
    "dgrad_taps_transposed": (lambda be: K.check_dgrad_impulses(be), "dz impulse"),
}


def test_every_defect_is_seeded():
    assert sorted(SEEDED) == sorted(K.DEFECTS)


@pytest.mark.parametrize("defect", K.DEFECTS)
def test_a_seeded_defect_fails(defect):
    check, word = SEEDED[defect]
    bad = [r for r in check(K.SimBackend(defect)) if not r.ok]
    assert bad and any(word in r.what for r in bad), f"{defect}: {[r.what for r in bad]}"
    with pytest.raises(AssertionError):
        K.hold(bad, verbose=False)
    assert all(r.ok for r in check(K.SimBackend()))


def test_the_undecided_cap_is_zero_and_is_asserted():
    r = _row(K.BWD_PARTIAL, **_S)
    o = K.operands(r)
    y = K.kernel_y(K.SimBackend(), r, o)
    y[0, 0, 0, 0] = -o.stats[1, 0, 0] / o.stats[0, 0, 0]         # y scale + shift = 0 to within a rounding
    with pytest.raises(AssertionError, match=f"{r.id} seed {r.seed}: 1 elements"):
        K.assert_decided(r, y, o.stats)


def test_the_refusal_table_covers_every_require_of_the_file():
    """every RPNET_REQUIRE line of csrc/conv_first.hip: its status and the head of its message stand in a row of REFUSALS, under every
    entry point that reaches the line"""
    lines = re.findall(r"RPNET_REQUIRE\(.*?(RPNET_ERR_\w+),\s*\"(conv1_\w+:)", SOURCE, flags=re.S)
    assert len(lines) == SOURCE.count("RPNET_REQUIRE(") == K.REQUIRE_LINES
    code = {"RPNET_ERR_SHAPE": K.SHAPE, "RPNET_ERR_ARG": K.ARG, "RPNET_ERR_WORKSPACE": K.WORKSPACE}
    have = {(status, head) for _, _, _, status, head in K.REFUSALS}
    assert {(code[s], h) for s, h in lines} == have
    entries = {e for _, e, *_ in K.REFUSALS}
    assert entries == {"rpnet_conv1_fwd", "rpnet_conv1_wgrad_bn", "rpnet_conv1_bn_relu", "rpnet_conv1_bn_bwd_partial", "rpnet_conv1_dgrad_bn"}
    # the cases the table must hold, by what they change
    ch = [(e, tuple(sorted(c.items()))) for _, e, c, _, _ in K.REFUSALS]
    assert len(set(ch)) == len(ch)
    for e in entries:
        couts = {dict(c).get("cout") for ee, c in ch if ee == e}
        assert {12, 2048} <= couts and (6 in couts or e == "rpnet_conv1_dgrad_bn") and (e != "rpnet_conv1_dgrad_bn" or 16 in couts), e
    assert any(dict(c).get("N") == 65536 for e, c in ch if e == "rpnet_conv1_dgrad_bn")
    assert {dict(c).get("planes") for e, c in ch if e == "rpnet_conv1_bn_relu"} >= {0, 4, 2}
    assert any("ws_short" in dict(c) for _, c in ch) and any(dict(c).get("groups") == 1025 for _, c in ch)
    assert torch.equal(K.impulse_filter(8)[0].flatten(), 2.0 ** (torch.arange(9.0) - 4))
