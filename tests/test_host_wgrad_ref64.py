"""The bound and the tables of tests/wgrad_cases.py on the CPU: SimBackend, a float32 restatement of the weight-gradient entry
points with the library's split-K plan, passes every check of every table row with the plain bound (the inputs are within reach
of a correct float32 kernel), and each seeded defect fails the check named beside it."""
import pytest
import torch

from tests import wgrad_cases as WC


def test_the_bound_is_the_small_ops_yardstick():
    import inspect
    from tests import test_gpu_small_ops as S
    assert WC.FLOOR == S.FLOOR and WC.FACTOR == inspect.signature(S.hold).parameters["factor"].default


def test_every_row_names_the_kernel_the_launcher_takes():
    ids = [c.id for c in WC.ALL_ROWS]
    assert len(set(ids)) == len(ids)
    for c in WC.ALL_ROWS + WC.DYNAMIC + list(WC.RING_EQUALS_ROW_MAJOR):
        assert WC.route(c) == c.kernel, (c.id, WC.route(c), c.kernel)
    for c in WC.ALL_ROWS:        # the launch's own plan never needs more than the query provides
        ks, _ = WC.launch_plan(c)
        per = (4 * 4 if c.fam == "up4" else c.taps) * c.Cin * c.cout * 4
        assert c.fam == "conv1" or ks * per <= WC.workspace_bytes(c), c.id


def test_the_plans_stated_beside_the_rows():
    assert WC.plan9(4800, 64, 192, 256) == (16, 10) and -(-150 // 10) == 15           # fifteen chunks hold work, one is surplus
    assert WC.plan9(8192, 64, 64, 256) == (32, 8)
    assert WC.plan9(256, 512, 512, 256) == (1, 8) and (512 // 32) * (512 // 32) >= 256
    assert WC.plan9(2304, 64, 64, 512) == (8, 9)
    assert WC.plan_tap(40960, 64, 64, 1)[2:] == (128, 10) and 1280 // 8 > WC.MAX1
    assert WC.plan1_split(40960, 64, 64) == (128, 10)
    assert WC.plan_tap(459, 128, 128, 9) == (128, 128, 1, 16)
    assert WC.plan_tap(512, 64, 64, 9)[2:] == (2, 8)


@pytest.mark.parametrize("c", WC.ALL_ROWS, ids=lambda c: c.id)
def test_a_correct_float32_implementation_is_inside_the_plain_bound(c):
    WC.hold(WC.check_row(WC.SimBackend(), c), verbose=False)


@pytest.mark.parametrize("c", WC.DYNAMIC, ids=lambda c: c.id)
def test_dynamic_range_of_a_correct_implementation(c):
    WC.hold(WC.check_dynamic_range(WC.SimBackend(), c), verbose=False)


def test_the_remaining_checks_of_a_correct_implementation():
    be = WC.SimBackend()
    WC.hold(WC.check_ring_equals_row_major(be), verbose=False)
    for c in WC.UP4:
        WC.hold(WC.check_up4_against_nine_tap(be, c), verbose=False)
    for _, c, runs in WC.UP4_UNSUPPORTED:
        if runs:
            WC.hold(WC.check_up4_against_nine_tap(be, c), verbose=False)


def _row(table, **kw):
    (c,) = [c for c in table if all(getattr(c, k) == v for k, v in kw.items())]
    return c


# defect -> (the row, the check that must fail, a word of its record)
SEEDED = {
    "drop_cross": (_row(WC.PLANES9, planes=2, tune=8), WC.check_bound, "dW per block"),
    "last_col": (_row(WC.FP32_9, N=3, H=16, W=48, mode=0), WC.check_impulses, "impulses"),
    "row_wrap": (_row(WC.PLANES9, planes=2, N=2, H=16, W=16, C1=0), WC.check_impulses, "impulses"),
    "image_wrap": (_row(WC.PLANES9, planes=3, tune=0, N=2, H=16, W=16, C1=0), WC.check_impulses, "impulses"),
    "swap_khkw": (_row(WC.FP32_TAP, dil=2, C0=64, cout=64, N=2), WC.check_impulses, "impulses"),
    "pad_rows": (_row(WC.PLANES1, planes=2, C1=64, sx1=None, map=(185, 0, 121, 128)), WC.check_bound, "dW per block"),
    "ignore_sx1": (_row(WC.PLANES1, planes=2, C1=64, sx1="own"), WC.check_bound, "dW per block"),
    "overwrite": (_row(WC.FP32_9, N=1, H=16, W=16), WC.check_accumulate, "accumulate=1"),
    "surplus": (_row(WC.PLANES9, planes=2, N=5, H=24, W=40), WC.check_bound, "dW per block"),
    "up_phase": (_row(WC.UP4, planes=2, N=2, H=32, W=32), WC.check_impulses, "impulses"),
}


def test_every_defect_is_seeded():
    assert sorted(SEEDED) == sorted(WC.DEFECTS)


@pytest.mark.parametrize("defect", WC.DEFECTS)
def test_a_seeded_defect_fails(defect):
    c, check, word = SEEDED[defect]
    bad = [r for r in check(WC.SimBackend(defect), c) if not r.ok]
    assert bad and any(word in r.what for r in bad), f"{defect}: {[r.what for r in bad]}"
    with pytest.raises(AssertionError):
        WC.hold(bad, verbose=False)
    assert all(r.ok for r in check(WC.SimBackend(), c))


def test_the_refusal_table_covers_the_three_entry_points():
    entries = {c.but(**{k: v for k, v in ch.items() if k in c.__dict__}).entry for _, c, ch, _ in WC.REFUSALS}
    assert entries == {"rpnet_conv_wgrad", "rpnet_conv_wgrad_up4", "rpnet_conv1_wgrad"}
    assert {s for *_, s in WC.REFUSALS} == {WC.SHAPE, WC.ARG, WC.WORKSPACE}
    assert torch.equal(WC.Case("planes1", (1, 1, 1), 128, 64, "", C1=64, map=(185, 0, 121, 128)).rows(),
                       torch.cat([torch.arange(121), torch.arange(128, 192)]))
