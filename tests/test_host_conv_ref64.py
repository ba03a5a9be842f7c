"""The bound and the tables of tests/conv_cases.py on the CPU: SimBackend, a float32 restatement of one convolution launch on the
operand planes with the kernels' dropped products, passes every check of every table row with the plain bound (the inputs are
within reach of a correct float32 kernel), each seeded defect fails the check named beside it, and route() — the launchers'
conditions restated once — agrees with the kernel every row names."""
import pytest
import torch

from tests import conv_cases as VC
from tests import ref64 as R


def test_the_bound_is_the_small_ops_yardstick():
    import inspect
    from tests import test_gpu_small_ops as S
    assert VC.FLOOR == S.FLOOR and VC.FACTOR == inspect.signature(S.hold).parameters["factor"].default


def test_every_row_names_the_kernel_the_launcher_takes():
    ids = [c.id for c in VC.ALL_ROWS]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    rows = VC.ALL_ROWS + VC.DYNAMIC + VC.CRE_PAIRS + [VC.nine_tap_form(c) for c in VC.UP4]
    for c in rows:
        assert VC.route(c) == c.kernel, (c.id, VC.route(c), c.kernel)
        assert c.C0 % 32 == 0 and c.C1 % 32 == 0 and c.Co0 % 64 == 0 and c.Co1 % 64 == 0, c.id
        assert max(c.M * max(c.Cin, c.Cout) * 4, VC.splitk_bytes(c)) <= 64 << 20, c.id
        assert not c.has("stats") or VC.stats_blocks(c) > 0, c.id
        if c.fam == "planes" and c.tune:            # a forced variant that the launcher would not take falls back silently
            assert VC.variant(c) == c.tune - 1, (c.id, VC.variant(c))
    for _, c in VC.UP4_UNSUPPORTED:
        assert VC.route(c) == "refused", c.id


def test_every_instantiation_is_reached():
    planes = [c for c in VC.ALL_ROWS if c.fam == "planes" and not c.splitk]
    assert {VC.variant(c) for c in planes} == set(VC.VARIANT_TILE) == {0, 1, 2, 3, 7, 8, 9, 11, 12, 13, 14}
    assert {(VC.variant(c), c.planes) for c in planes} >= {(v, p) for v in range(4) for p in (3, 2, 1)} | {(7, 3), (7, 2), (7, 1), (13, 1)}
    for patch in (False, True):           # conv_epilogue_store<AFF, ROWOPS> under LinearRows and under PatchRows
        assert {VC.epilogue_instance(c) for c in VC.ALL_ROWS if VC.patch_rows(c) == patch} == {(a, r) for a in (False, True) for r in (False, True)}
    assert {(c.up4, c.planes) for c in VC.UP4} == {(1, 2), (1, 1), (2, 2), (2, 1)}
    assert {VC.route(c) for c in VC.FP32} == {k + s for k in VC.IGEMM for s in ("", "+in_scale")}
    # every fp32 shape of the issue carries every form of the gather, at both tile widths (up-sampling on the even stand-ins)
    for s in VC.FP32_SHAPES:
        for f in VC.FP32_FORMS:
            shape = VC._EVEN.get(s, s) if f.get("ups") else s
            for co in (64, 128):
                assert any((c.N, c.H, c.W) == shape and c.Co0 == co and all(getattr(c, k) == v for k, v in f.items())
                           and (f or (c.taps, c.dil, c.mode, c.C1, c.ups) == (9, 1, 0, 0, 0)) for c in VC.FP32), (s, f, co)
    assert {c.skip[4:6] for c in VC.SKIP} == {"10", "11", "20", "21"} and {c.skip[6] for c in VC.SKIP} == {"a", "t"}
    assert all(VC.variant(c) in VC.DMA_VARIANTS for c in VC.SKIP)
    # a tile of the group rows straddles the two statistic groups: the per-row lookup of the affine
    assert any(c.has("aff") and c.groups == 2 and not VC.patch_rows(c) and (c.M // 2) % VC.tile_rows(c) for c in VC.ALL_ROWS)


def test_the_tile_choices_stated_in_the_module_docstring():
    first = {}
    for cout in (64, 128, 192, 256, 320, 384):          # every M whose output stays within 64 MiB
        for M in range(1, (64 << 20) // (cout * 4) + 1):
            first.setdefault((cout, VC.choose_tile(M, cout, cout % 128 == 0)), M)
    assert first[(64, 3)] == 7873 and (64, 2) not in first and (128, 2) not in first          # <1,1> from M = 7873; <1,2> not at one column tile
    assert first[(384, 2)] == 21761 and (256, 2) not in first and 341 * 3 / 1024 > 513 / 768 + 0.02 and 21761 * 384 * 4 < 64 << 20
    assert -(-7873 // 64) == 124 and 124 / 1536 > 62 / 1024 + 0.02 > 123 / 1536
    # split K: Cin >= 128 and whole 256-pixel tiles; one tile of four chunks is the smallest, cut in two
    small = VC.SPLITK[0]
    assert VC.splitk_parts(small) == 2 and VC.splitk_bytes(small) == 2 * 256 * 64 * 4
    assert VC.splitk_parts(small.but(C0=96)) == 1 and VC.splitk_parts(small.but(H=4)) == 1 and VC.splitk_parts(small.but(tune=13)) == 1
    assert VC.splitk_parts(VC.SPLITK[1]) == 2 and VC.SPLITK[1].C0 == 96            # chunks 2 | 3 of the second part lie in x0 | x1
    assert VC.splitk_parts(VC.SPLITK[2]) == 4


def test_the_references_against_autograd():
    """conv_dgrad is the autograd of conv_fwd with respect to its input (the split, the factor, the accumulate and the 2 x 2 sum on
    top), for both tap forms and the dilated one"""
    for taps, dil, ups in ((9, 1, 0), (9, 2, 0), (1, 1, 0), (9, 1, 1)):
        k = 3 if taps == 9 else 1
        x = torch.randn(2, 3, 5, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(taps + dil), requires_grad=True)
        w = torch.randn(4, 6, k, k, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
        xu = x.repeat_interleave(2, 1).repeat_interleave(2, 2) if ups else x
        pad = dil if taps == 9 else 0
        y = torch.nn.functional.conv2d(xu.permute(0, 3, 1, 2), w, padding=pad, dilation=dil).permute(0, 2, 3, 1)
        out, pre = R.conv_fwd(x, None, w, None, taps, dil, ups)
        assert torch.allclose(out, y.detach(), rtol=1e-13, atol=1e-13) and torch.equal(out, pre)
        dy = torch.randn(y.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
        (g,) = torch.autograd.grad(y, x, dy)
        got = R.conv_dgrad(dy, w, taps, dil, (4, 2), upsample=ups)
        assert torch.allclose(torch.cat(got, -1), g, rtol=1e-12, atol=1e-12) and got[0].shape[-1] == 4


@pytest.mark.parametrize("c", VC.ALL_ROWS, ids=lambda c: c.id)
def test_a_correct_float32_implementation_is_inside_the_plain_bound(c):
    recs = VC.check_row(VC.SimBackend(), c)
    VC.hold(recs, verbose=False)
    w = VC.CC.worst([r for r in recs if not r.exact] or recs)
    print(f"worst of {c.id}: {w.what} of_bound={w.multiple:.3f}")


@pytest.mark.parametrize("c", VC.DYNAMIC, ids=lambda c: c.id)
def test_dynamic_range_of_a_correct_implementation(c):
    VC.hold(VC.check_dynamic_range(VC.SimBackend(), c), verbose=False)


@pytest.mark.parametrize("c", VC.CRE_PAIRS, ids=lambda c: c.id)
def test_the_two_masked_branches_of_a_correct_implementation(c):
    VC.hold(VC.check_cre_pair(VC.SimBackend(), c), verbose=False)


def _row(table, **kw):
    (c,) = [c for c in table if all(getattr(c, k) == v for k, v in kw.items())]
    return c


_LIN = dict(planes=2, tune=1, N=2, H=5, W=7, Co1=0)
# defect -> (the row, the check that must fail, a word of its record)
SEEDED = {
    "seam_column": (_row(VC.PATCH, planes=2, tune=12, N=2, H=16, W=64, ups=0), VC.check_impulses, "impulses"),
    "previous_image_top": (_row(VC.PATCH, planes=2, tune=12, N=2, H=32, W=32), VC.check_impulses, "impulses"),
    "bias_after_affine": (_row(VC.FP32, N=2, H=5, W=7, Co0=64, groups=2, ep="bias aff relu"), VC.check_bound, "per block"),
    "one_minus_s": (_row(VC.EPILOGUE, ep="os1", **_LIN), VC.check_bound, "per block"),
    "no_accumulate": (_row(VC.EPILOGUE, ep="acc", **_LIN), VC.check_bound, "per block"),
    "group_of_first_row": (_row(VC.EPILOGUE, ep="aff", groups=2, **_LIN), VC.check_bound, "per block"),
    "second_dest_offset": (_row(VC.EPILOGUE, planes=2, tune=1, H=5, Co1=128), VC.check_bound, "y1"),
    "drop_cross": (_row(VC.PLAIN, planes=2, tune=2, N=3, dil=1, taps=9, C1=0), VC.check_bound, "per block"),
    "up_round": (_row(VC.FP32, N=1, H=6, W=10, ups=1, Co0=64), VC.check_impulses, "impulses"),
    "no_dilation": (_row(VC.FP32, N=1, H=5, W=7, dil=2, Co0=64, C1=0), VC.check_bound, "per block"),
    "ignore_sx1": (_row(VC.PLAIN, planes=2, tune=4, sx1="own"), VC.check_bound, "per block"),
    "amax_before_out_scale": (_row(VC.EPILOGUE, ep="bias aff relu os2 acc amax ys2", groups=1, **_LIN), VC.check_bound, "out_absmax"),
    "stats_without_bias": (_row(VC.EPILOGUE, planes=2, N=2, H=8, W=8, ep="stats bias"), VC.check_bound, "stats_partial"),
    "ysplit_before_rowops": (_row(VC.EPILOGUE, ep="bias aff relu os2 acc amax ys2", groups=1, **_LIN), VC.check_bound, "y_split"),
    "splitk_part_missing": (VC.SPLITK[0], VC.check_splitk, "split K"),
}


def test_every_defect_is_seeded():
    assert sorted(SEEDED) == sorted(VC.DEFECTS)


@pytest.mark.parametrize("defect", VC.DEFECTS)
def test_a_seeded_defect_fails(defect):
    c, check, word = SEEDED[defect]
    bad = [r for r in check(VC.SimBackend(defect), c) if not r.ok]
    assert bad and any(word in r.what for r in bad), f"{defect}: {[r.what for r in bad]}"
    with pytest.raises(AssertionError):
        VC.hold(bad, verbose=False)
    assert all(r.ok for r in check(VC.SimBackend(), c))


def test_dropping_the_smallest_kept_product_of_three_planes_fails_too():
    """three bf16 planes: the l.h product is the smallest one kept (drop_cross takes it out of the sequence)"""
    c = _row(VC.PLAIN, planes=3, tune=1, N=3)
    assert any(not r.ok for r in VC.check_bound(VC.SimBackend("drop_cross"), c))


def test_a_dropped_cross_product_fails_the_collapsed_up_conv_rows_too():
    """two planes with random weights: the x_h . w_l product and the pack's second plane are held to float64 in both modes"""
    for mode in (1, 2):
        c = [c for c in VC.UP4 if c.planes == 2 and c.up4 == mode][0]
        bad = [r for r in VC.check_up4(VC.SimBackend("drop_cross"), c) if not r.ok]
        assert any(r.what.startswith("y ") for r in bad) and any("nine-tap" in r.what for r in bad), [r.what for r in bad]


def test_the_refusal_table_covers_both_entry_points():
    entries = {c.entry for _, c, *_ in VC.REFUSALS}
    assert entries == set(VC.REFUSAL_PREFIX) == {"rpnet_conv_fwd", "rpnet_conv_up4"}
    assert {r[3] for r in VC.REFUSALS} == {VC.SHAPE, VC.ARG} and all(len(r[4]) > 8 for r in VC.REFUSALS)
    labels = [(c.entry, label) for label, c, *_ in VC.REFUSALS]
    assert len(set(labels)) == len(labels)
