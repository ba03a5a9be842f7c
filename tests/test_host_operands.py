"""The tables of tests/operand_cases.py on the CPU: SimBackend, a restatement of the INDEX arithmetic of the operand splitters and
weight packers (element -> row division, the grid-stride loop under its 16384-block cap, the 32 x 32 tile walks of both pack forms with
their guards, the row-scale reductions, the collapse), must equal the reshape / permute references bit for bit on every row that the
GPU test runs, and each seeded defect in it must fail at least one row.  Also here: corr_cases.pow2_scale against an integer
restatement of the header's sentence, the collapsed up_conv weights against the layer they replace, and the shape of the tables."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import corr_cases, operand_cases as K


@pytest.fixture(scope="module")
def be():
    return K.SimBackend()


def ok(recs):
    return all(r.ok for r in recs)


@pytest.mark.parametrize("bound", K.POW2_BOUNDS, ids=repr)
def test_pow2_scale_is_the_headers_sentence(be, bound):
    """corr_cases.pow2_scale, the host scale of the correlation, weight-gradient and first-layer suites, in exact integer arithmetic"""
    b32 = torch.tensor([bound], dtype=torch.float32)
    e = K.pow2_exponent_from_header(int(b32.view(torch.int32)[0]) & 0xFFFFFFFF)
    assert corr_cases.pow2_scale(float(b32[0])) == 2.0 ** e, (bound, e)
    K.hold(K.check_pow2(be, bound))


def test_pow2_rows_reach_both_clamps_and_every_edge():
    e = {b: math.log2(corr_cases.pow2_scale(b)) for b in K.POW2_BOUNDS if b == b}
    assert e[0.0] == e[-1.0] == e[2.0 ** -149] == -100 and e[math.inf] == 100
    assert e[2.0 ** -85] == -100 and e[K.ulp_step(2.0 ** -85, 1)] == -99 and e[2.0 ** 115] == 100 == e[K.ulp_step(2.0 ** 115, 1)] and e[K.ulp_step(2.0 ** 115, -1)] == 100
    for k in K.POW2_K:
        assert (e[K.ulp_step(2.0 ** k, -1)], e[2.0 ** k], e[K.ulp_step(2.0 ** k, 1)]) == (k - 15, k - 15, k - 14)
    assert e[65504.0] == 1


@pytest.mark.parametrize("n,safety,check", K.PREDICT_ROWS)
def test_predict_scales(be, n, safety, check):
    K.hold(K.check_predict(be, n, safety, check))


def test_a_nan_measurement_is_a_violation_and_gives_the_floor():
    m, bound = K.predict_inputs(9, 1.0)
    assert math.isnan(float(m[6]))
    wb, ws, wv = K.ref_predict(m, bound, 9, 1.0, 1, 0)
    assert wv == 4 and float(ws[6]) == 2.0 ** -100 and float(wb[6]) == 2.0 ** -85


@pytest.mark.parametrize("r", K.SPLIT_ROWS, ids=lambda r: r.id)
def test_split(be, r):
    K.hold(K.check_split(be, r))


def test_split_rows_cover_what_they_claim():
    rows = K.SPLIT_ROWS
    assert len({r.id for r in rows}) == len(rows)
    for kernel, planes in (("bf16", 3), ("f16", 2), ("f16", 1)):
        mine = [r for r in rows if r.kernel == kernel and r.planes == planes]
        assert {(r.rows, r.C) for r in mine} >= set(K.SPLIT_SHAPES) | {K.LARGE, (0, 8)} and {r.mode for r in mine} == {0, 1, 2}
        assert any(r.offset for r in mine) and any(r.data == "decades" for r in mine)
    assert {(r.kernel, r.planes) for r in rows if (r.rows, r.C) == K.CAP} == {("bf16", 3), ("f16", 1)}
    n8 = K.CAP[0] * K.CAP[1] // 8
    assert n8 // K.BLOCK + 1 > K.GRID_CAP and K.GRID_CAP * K.BLOCK < n8 < K.GRID_CAP * K.BLOCK + 2 * K.BLOCK       # a second pass in blocks 0 and 1
    assert (K.LARGE[0] * K.LARGE[1] // 8) // K.BLOCK + 1 < K.GRID_CAP                                             # the 17 MB row stays under the cap
    f16 = [r for r in rows if r.kernel == "f16"]
    assert {r.sb for r in f16 if not r.a_is_bound} == {"none", "lo", "hi"} and {r.s_out for r in f16} == {0, 1}
    assert {r.bound for r in f16 if r.a_is_bound} == set(K.BOUNDS)
    x, mask, s_a, s_b = K.split_inputs(next(r for r in f16 if r.sb == "hi" and r.mode and r.rows >= 7))
    assert {0.0, 1.0, 2.0 ** -30} <= set(mask.tolist()) and float(s_b[0]) > float(s_a[0])
    v = (x / s_a).double()
    h = v.float().half().double()
    tie = (v - h).abs() == (torch.nextafter(h.half(), torch.tensor(math.inf).half()).double() - h) / 2              # the half-way values survive
    assert int(tie.sum()) >= 4 and bool((x == 0).any()) and bool((x.abs() < 2.0 ** -126).logical_and(x != 0).any())


@pytest.mark.parametrize("it,planes", K.PACK_ROWS, ids=lambda v: getattr(v, "id", str(v)))
def test_pack_split(be, it, planes):
    K.hold(K.check_pack(be, it, planes))


@pytest.mark.parametrize("it,planes,kind", K.IMPULSE_ROWS, ids=lambda v: getattr(v, "id", str(v)))
def test_pack_impulses(be, it, planes, kind):
    K.hold(K.check_impulse(be, it, planes, kind))


@pytest.mark.parametrize("order,planes", K.MULTI_ROWS)
def test_pack_many_layers(be, order, planes):
    K.hold(K.check_multi(be, order, planes))


@pytest.mark.parametrize("it", K.F32_ITEMS, ids=lambda i: i.id)
def test_pack_f32(be, it):
    K.hold(K.check_pack_f32(be, it))


def test_pack_rows_cover_both_walks():
    assert [K.needs_gather(i) for i in K.PACK_ITEMS] == [False] * 7 + [True] * 3
    assert any(i.cin == 377 and i.split == 121 and i.off1 == 128 and i.cin_pad == 384 for i in K.GATHER_ITEMS)
    assert {i.taps for i in K.PACK_ITEMS} == {1, 4, 9} and all(i.cin_pad % 4 == 0 and i.taps in (1, 9) for i in K.F32_ITEMS)
    w = K.weights(K.PLAIN_ITEMS[1])
    assert float(w[1].abs().max()) == 0 and float(w[:, 2].abs().max()) == 0 and float(w[0].abs().max()) == 0.5 and float(w[:, 1].abs().max()) == 2.0
    wp, wd, t, u = K.ref_pack_split(K.PLAIN_ITEMS[1], w, 2)
    assert float(t[1]) == 2.0 ** -100 == float(u[2]) and float(t[0]) == 2.0 ** -16 and float(u[1]) == 2.0 ** -14


@pytest.mark.parametrize("cout,cin", K.COLLAPSE_SHAPES)
def test_collapse(be, cout, cin):
    K.hold(K.check_collapse(be, cout, cin))


@pytest.mark.parametrize("planes", (2, 1))
def test_collapse_then_pack(be, planes):
    K.hold(K.check_collapse_then_pack(be, planes))


def test_collapsed_weights_are_the_layer():
    """nn.Upsample(scale_factor=2) -> Conv2d 3x3 in float64 equals the four-phase form built from the reference's collapsed weights"""
    g = torch.Generator().manual_seed(11)
    x, w = torch.randn(2, 5, 6, 7, dtype=torch.float64, generator=g), torch.randn(3, 5, 3, 3, dtype=torch.float64, generator=g)
    full = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1)[:, :, 2:-2, 2:-2]
    four = K.four_phase_conv(x, K.ref_collapse(w)[0], 3)
    assert four.shape == full.shape and float((four - full).abs().max()) <= 16 * 2.0 ** -53 * float(full.abs().max())
    assert K.phase_sets()[:, :, :].sum((1,)).eq(1).all() and K.phase_sets().sum((1, 2)).tolist() == [3, 3]


# the rows a defect is looked for in, cheapest first (never the 17 MB and 134 MB rows)
def _families():
    small = [r for r in K.SPLIT_ROWS if r.rows * r.C <= 1 << 16]
    return ([lambda be, b=b: K.check_pow2(be, b) for b in K.POW2_BOUNDS] + [lambda be, r=r: K.check_split(be, r) for r in small]
            + [lambda be, c=c: K.check_collapse(be, *c) for c in K.COLLAPSE_SHAPES[:2]]
            + [lambda be, a=a: K.check_pack(be, *a) for a in K.PACK_ROWS if a[0] in (K.PLAIN_ITEMS[6], K.GATHER_ITEMS[1], K.PLAIN_ITEMS[1])])


@pytest.mark.parametrize("defect", K.DEFECTS)
def test_every_seeded_defect_fails_a_row(defect):
    bad = K.SimBackend(defect)
    assert any(not ok(check(bad)) for check in _families()), f"no row notices {defect}"


def test_the_refusal_table_names_every_launcher():
    entries = {e for _, e, _, _, _ in K.REFUSALS}
    assert entries == {"rpnet_split_bf16", "rpnet_split_f16", "rpnet_pow2_scale", "rpnet_predict_scales", "rpnet_pack_conv_weight_split",
                       "rpnet_pack_conv_weights_split", "rpnet_pack_conv_weight", "rpnet_upconv_collapse_weights"}
    assert all(rc in (K.ARG, K.SHAPE) for _, _, _, rc, _ in K.REFUSALS)
    assert len({(e, label, str(a)) for label, e, a, _, _ in K.REFUSALS}) == len(K.REFUSALS)
    heads = {h for _, _, _, _, h in K.REFUSALS}
    assert {"split_f16: s_b must be NULL", "pack_conv_weights_split: channel ranges overlap", "pack_conv_weight: channel ranges overlap",
            "pack_conv_weight: cin ", "pack_conv_weights_split: cin ", "pack_conv_weight: channel ranges exceed"} <= heads
