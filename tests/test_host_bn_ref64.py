"""The references, the bounds and the tables of tests/bn_cases.py on the CPU: the new tests/ref64.py functions against
torch.nn.functional.batch_norm / nn.BatchNorm2d and the oracle; SimBackend, a float32 restatement of the BatchNorm entry points with
the library's partial / finalize split, passes every check of every table row with room (the largest of_bound stays below 0.5: the
bounds are not cut to fit), the references alone keep the excluded share of every case under its cap, and each seeded defect fails
the check named beside it."""
import pytest
import torch
import torch.nn.functional as F

from tests import bn_cases as BC
from tests import ref64 as R
from tests.helpers import rnd

F64 = torch.float64


def test_the_bound_is_the_small_ops_yardstick():
    import inspect
    from tests import test_gpu_small_ops as S
    assert BC.FLOOR == S.FLOOR and BC.FACTOR == inspect.signature(S.hold).parameters["factor"].default


def test_every_row_names_the_launches_the_entry_point_makes():
    ids = [c.id for c in BC.ALL_ROWS]
    assert len(set(ids)) == len(ids)
    for c in BC.ALL_ROWS:
        assert BC.route(c) == c.kernel, (c.id, BC.route(c), c.kernel)
    reached = {w for c in BC.ALL_ROWS for w in BC.route(c).replace("[z=NULL]", "").replace("[zp=NULL]", "").replace("[dy=NULL]", "").split()}
    assert reached == set(BC.KERNELS), (reached ^ set(BC.KERNELS))
    nulls = {t for c in BC.ALL_ROWS for t in ("[z=NULL]", "[zp=NULL]", "[dy=NULL]") if t in c.kernel}
    assert len(nulls) == 3                                    # every split form also runs without its fp32 output


def test_the_geometry_stated_beside_the_rows():
    g = lambda name: BC.geom(BC._row("stats", name, "").R, BC.SHAPES[name][1])       # noqa: E731
    assert g("c4")[:3] == (1, 256, 1) and g("c24")[:3] == (6, 42, 1) and g("c24g2")[:3] == (6, 42, 2)
    assert g("c24big")[:3] == (6, 42, 13) and g("c72")[:3] == (18, 14, 3) and g("c192g2")[:3] == (48, 5, 5)
    assert g("c512g2")[:3] == (128, 2, 3) and g("c1024")[:3] == (256, 1, 3)
    assert g("clamp") == (16, 16, 1024, 65) and BC.SHAPES["clamp"][0][2] * 2 > 1024 * 16 * 4
    assert BC.max_blocks(4) == 1024 and BC.max_blocks(192) == 682 and BC.max_blocks(1024) == 256
    for c in BC.ALL_ROWS:                                     # a group boundary inside a block of the element-wise passes
        if c.G > 1 and c.op in ("relu", "bwd") and not c.pool:
            assert (c.R * c.C) % (256 * 8) != 0, c.id
    for c in BC.FROM_PARTIAL:
        assert c.nblk != BC.geom(c.R, c.C)[2], c.id
    assert any(c.N // c.G >= 2 and c.G == 3 for c in BC.STATS) and {c.G for c in BC.STATS} == {1, 2, 3}


def test_bn_stats_is_batch_norm_called_once_per_group():
    N, H, W, C, G = 6, 5, 7, 8, 3
    y, gamma, beta = rnd(1, N, H, W, C) * 1.3 + 0.2, rnd(2, C), rnd(3, C) * 0.3
    rm0, rv0 = rnd(4, C).double(), 1 + rnd(5, C).abs().double()
    sc, sh, mu, inv, rm, rv = R.bn_stats(y, gamma, beta, rm0, rv0, 0.1, 1e-5, G)
    bn = torch.nn.BatchNorm2d(C, eps=1e-5, momentum=0.1).double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(rm0), bn.running_var.copy_(rv0)
    rmf, rvf = rm0.clone(), rv0.clone()
    for g in range(G):
        yy = y[2 * g:2 * g + 2].double().permute(0, 3, 1, 2)
        want = torch.relu(F.batch_norm(yy, rmf, rvf, gamma.double(), beta.double(), True, 0.1, 1e-5)).permute(0, 2, 3, 1)
        assert torch.allclose(torch.relu(bn(yy)).permute(0, 2, 3, 1), want, rtol=0, atol=1e-14)
        assert torch.allclose(R.bn_relu(y[2 * g:2 * g + 2], sc[g], sh[g]), want, rtol=0, atol=1e-13)
    for got in (rm, rv):
        assert got.dtype == F64
    assert torch.allclose(rm, rmf, rtol=1e-14, atol=0) and torch.allclose(rv, rvf, rtol=1e-14, atol=0)
    assert torch.allclose(rm, bn.running_mean, rtol=1e-14, atol=0) and torch.allclose(rv, bn.running_var, rtol=1e-14, atol=0)
    assert int(bn.num_batches_tracked) == G
    # eval mode: the running statistics as constants
    e_sc, e_sh = R.bn_eval_affine(gamma, beta, rm, rv, 1e-5)
    want = torch.relu(F.batch_norm(y.double().permute(0, 3, 1, 2), rm, rv, gamma.double(), beta.double(), False, 0.1, 1e-5)).permute(0, 2, 3, 1)
    z, top = R.bn_eval_relu(y.reshape(-1, C), e_sc, e_sh)
    assert torch.allclose(z.reshape(want.shape), want, rtol=0, atol=1e-13) and top == z.max()


def test_bn_bwd_is_autograd_of_batch_norm_and_the_closed_form():
    N, H, W, C, G = 4, 6, 10, 8, 2
    y, gamma, beta = rnd(11, N, H, W, C) * 1.3 + 0.2, rnd(12, C), rnd(13, C) * 0.3
    st = torch.stack(R.bn_stats(y, gamma, beta, None, None, 0.1, 1e-5, G)[:4])          # float64: the exact batch statistics
    for pooled in (False, True):
        dz = rnd(14, N, H // 2, W // 2, C) if pooled else rnd(14, N, H, W, C)
        dy, dg, db, coef = R.bn_bwd(dz, y, st, G, pooled)
        yr, gm, bt = y.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
        z = torch.cat([torch.relu(F.batch_norm(yr[2 * g:2 * g + 2].permute(0, 3, 1, 2), None, None, gm, bt, True, 0.1, 1e-5)) for g in range(G)])
        if pooled:
            z = F.max_pool2d(z, 2, 2)
        z.backward(dz.double().permute(0, 3, 1, 2))
        for got, want in ((dy, yr.grad), (dg, gm.grad), (db, bt.grad)):
            assert (got - want).abs().max() <= 1e-11 * want.abs().max()
        full = R.maxpool2_bwd(R.bn_relu(y, st[0], st[1], G), dz) if pooled else dz
        s1, s2 = R.bn_bwd_sums(full, y, st, G)
        assert torch.allclose(coef[..., 0], s1 / (2 * H * W), rtol=1e-12, atol=1e-15) and torch.allclose(coef[..., 1], s2 / (2 * H * W), rtol=1e-12, atol=1e-15)
        assert torch.allclose(dy, R.bn_dy(full, y, st, coef, G), rtol=0, atol=1e-12)
    dz = rnd(15, N, H, W, C)
    s1, s2 = R.bn_bwd_sums(dz, y, st, G)
    e_dy, e_dg, e_db = R.bn_eval_bwd(dz, y, st, G)
    assert torch.allclose(e_dy, R.bn_dy(dz, y, st, None, G), rtol=0, atol=1e-13)
    assert torch.allclose(e_dg, s2.sum(0), rtol=1e-12, atol=1e-14) and torch.allclose(e_db, s1.sum(0), rtol=1e-12, atol=1e-14)


def test_the_references_against_the_oracle():
    """oracle/rpnet_oracle.py _bn_relu, called once per group on one parameter set, train mode then eval mode"""
    from oracle import rpnet_oracle as O
    N, H, W, C, G = 4, 5, 7, 8, 2
    y, gamma, beta = rnd(21, N, H, W, C) * 1.3 + 0.2, rnd(22, C), rnd(23, C) * 0.3
    P = {"b.weight": gamma.double(), "b.bias": beta.double(), "b.running_mean": torch.zeros(C, dtype=F64),
         "b.running_var": torch.ones(C, dtype=F64), "b.num_batches_tracked": torch.tensor(0)}
    sc, sh, _, _, rm, rv = R.bn_stats(y, gamma, beta, P["b.running_mean"], P["b.running_var"], O.BN_MOMENTUM, O.BN_EPS, G)
    want = torch.cat([O._bn_relu(P, "b", y[2 * g:2 * g + 2].double().permute(0, 3, 1, 2), True) for g in range(G)]).permute(0, 2, 3, 1)
    assert torch.allclose(R.bn_relu(y, sc, sh, G), want, rtol=0, atol=1e-13)
    assert torch.allclose(R.bn_relu_pool(y[:, :4, :6], sc, sh, G), F.max_pool2d(want[:, :4, :6].permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1), rtol=0, atol=1e-13)
    assert torch.allclose(rm, P["b.running_mean"], rtol=1e-14, atol=0) and torch.allclose(rv, P["b.running_var"], rtol=1e-14, atol=0)
    assert int(P["b.num_batches_tracked"]) == G
    e_sc, e_sh = R.bn_eval_affine(gamma, beta, rm, rv, O.BN_EPS)
    want = O._bn_relu(P, "b", y.double().permute(0, 3, 1, 2), False).permute(0, 2, 3, 1)
    assert torch.allclose(R.bn_eval_relu(y.reshape(-1, C), e_sc, e_sh)[0].reshape(want.shape), want, rtol=0, atol=1e-13)


def test_pooled_reference_routes_to_the_first_maximum():
    from tests.test_gpu_small_ops import test_maxpool_reference_routes_to_the_first_maximum
    test_maxpool_reference_routes_to_the_first_maximum()
    c = [c for c in BC.BWD_POOL if "t" in c.data][0]
    d = BC.make_data(c)
    assert bool((d.y[0, :2, :2] == 1.0).all())                                    # one window tied in all four positions
    st = BC.stats_of(c, d)
    dy = R.bn_bwd(d.dz, d.y, st, c.G, True)[0]
    coef = R.bn_bwd(d.dz, d.y, st, c.G, True)[3]
    base = R.bn_dy(torch.zeros_like(d.y), d.y, st, coef, c.G)                     # dy without the routed gradient
    routed = (dy - base)[0, :2, :2]                                               # [2, 2, C]: only the first pixel may receive it
    # (1e-6: the statistics are the fp32 ones the kernels are given, so the closed form holds to their rounding only)
    want = st[0].double()[0] * d.dz[0, 0, 0].double() * (st[1][0] + st[0][0] > 0)                    # y = 1 in the tied window
    assert torch.allclose(routed[0, 0], want, rtol=0, atol=1e-6) and float(want.abs().max()) > 0.1
    assert float(routed[0, 1].abs().max()) < 1e-6 and float(routed[1].abs().max()) < 1e-6


@pytest.mark.parametrize("c", BC.ALL_ROWS, ids=lambda c: c.id)
def test_a_correct_float32_implementation_is_inside_the_bounds_with_room(c):
    recs = BC.check_row(BC.SimBackend(), c)
    BC.hold(recs, verbose=False)
    top = max((r.multiple for r in recs if not r.exact), default=0.0)
    assert top < 0.5, [(r.what, r.multiple) for r in recs if not r.exact and r.multiple >= 0.5]


@pytest.mark.parametrize("c", [c for c in BC.ALL_ROWS if c.op in ("bwd", "eval_bwd")], ids=lambda c: c.id)
def test_the_references_alone_stay_inside_the_excluded_cap(c):
    d = BC.make_data(c)
    ex = BC.excluded(c, d, BC.stats_of(c, d))
    assert float(ex.double().mean()) <= BC.EXCLUDED_CAP, (c.id, int(ex.sum()), ex.numel())


def test_the_offset_backward_row_has_no_element_inside_the_mask_zone():
    (c,) = [c for c in BC.BWD if "o" in c.data]
    d = BC.make_data(c)
    st = BC.stats_of(c, d)
    assert int(BC.excluded(c, d, st).sum()) == 0
    yg = d.y.double().reshape(c.G, -1, c.C)
    assert float((yg.mean(1) / yg.std(1)).min()) > 512                                   # xhat = (y - mean) invstd cancels nine bits or more
    # ... and with the batch statistics in float64 the closed form IS the autograd of the train-mode expression
    st64 = torch.stack(R.bn_stats(d.y, d.gamma, d.beta, None, None, BC.MOM, BC.EPS, c.G)[:4])
    s1, s2 = R.bn_bwd_sums(d.dz, d.y, st64, c.G)
    dy = R.bn_dy(d.dz, d.y, st64, torch.stack([s1, s2], -1) / c.R, c.G)
    assert float((dy - R.bn_bwd(d.dz, d.y, st64, c.G)[0]).abs().max()) <= 1e-6 * float(dy.abs().max())


def test_the_edge_data_is_what_the_tables_say():
    c = [c for c in BC.BWD if c.data == "e" and c.G == 2][0]
    d = BC.make_data(c)
    st = BC.stats_of(c, d)
    assert float(d.gamma[1]) < 0
    assert float((st[3][:, 0].double() - BC.EPS ** -0.5).abs().max()) <= BC.U * BC.EPS ** -0.5      # variance 0: one fp32 rounding
    assert float(R.bn_relu(d.y, st[0], st[1], c.G)[..., 2].abs().max()) == 0        # every y scale + shift of channel 2 is negative
    o = [c for c in BC.STATS if c.data == "o"][0]
    yo = BC.make_data(o).y.double().reshape(o.G, -1, o.C)
    assert torch.allclose(yo.mean(1) / yo.std(1), torch.tensor(1024.0, dtype=F64), rtol=0.35)
    dd = BC.make_data([c for c in BC.BWD if "d" in c.data][0]).dz
    assert 2.0 ** 17 < float(dd[..., 0].abs().max() / dd[..., -1].abs().max()) < 2.0 ** 23


def _row(table, **kw):
    (c,) = [c for c in table if all(getattr(c, k) == v for k, v in kw.items())]
    return c


_S = BC.SHAPES
# defect -> (the row, a word of the record that must fail)
SEEDED = {
    "fp32_stats": (_row(BC.STATS, N=2, C=24, data="o"), "invstd"),
    "biased_running": (_row(BC.STATS, N=2, C=72, G=1), "running_var"),
    "one_running_update": (_row(BC.STATS, N=4, C=24, G=2), "running_mean"),
    "group_from_image": (_row(BC.RELU, N=4, C=24, G=2, planes=0), "z per channel"),
    "drop_last_rows": (_row(BC.STATS, N=2, C=72, G=1), "mean"),
    "surplus_partial": (_row(BC.FROM_PARTIAL, N=4, nblk=1), "mean"),
    "mask_from_mean": (_row(BC.BWD, N=2, C=72, planes=0, red=False), "dy"),
    "ignore_accumulate": (_row(BC.BWD, N=2, C=72, planes=0, red=False), "accumulate=1"),
    "eval_coef_stale": (_row(BC.EVAL_BWD, N=2, C=72, planes=0), "coef"),
    "pool_last_max": (_row(BC.BWD_POOL, N=6, planes=3), "dy"),
    "scale_from_max": (_row(BC.BWD, N=4, C=24, planes=1), "published scale"),
    "ignore_given_rows": (_row(BC.GIVEN, N=4, given=257, planes=0), "dgamma"),
}


def test_every_defect_is_seeded():
    assert sorted(SEEDED) == sorted(BC.DEFECTS)


@pytest.mark.parametrize("defect", BC.DEFECTS)
def test_a_seeded_defect_fails(defect):
    c, word = SEEDED[defect]
    bad = [r for r in BC.check_row(BC.SimBackend(defect), c) if not r.ok]
    assert bad and any(word in r.what for r in bad), f"{defect}: {[r.what for r in bad]}"
    with pytest.raises(AssertionError):
        BC.hold(bad, verbose=False)


def test_the_forward_scale_defect_fails_too():
    c = _row(BC.RELU, N=4, C=24, G=2, planes=2)
    assert any("published scale" in r.what for r in BC.check_row(BC.SimBackend("scale_from_max"), c) if not r.ok)


def test_the_refusal_table_covers_the_entry_points():
    entries = {e for _, e, _, _ in BC.REFUSALS}
    assert entries == {"rpnet_bn_stats", "rpnet_bn_stats_from_partial", "rpnet_bn_eval_affine", "rpnet_bn_relu", "rpnet_bn_bwd",
                       "rpnet_bn_eval_relu", "rpnet_bn_eval_bwd"}
    assert {s for *_, s in BC.REFUSALS} == {BC.SHAPE, BC.ARG, BC.WORKSPACE}
    labels = [(e, lab) for lab, e, _, _ in BC.REFUSALS]
    assert len(set(labels)) == len(labels)
    for k in ("N", "HW", "C"):
        assert BC.HUGE[k] < 2 ** 31 and BC.POOL_HUGE[k] < 2 ** 31
    assert BC.HUGE["N"] * BC.HUGE["HW"] * BC.HUGE["C"] // 4 >= 2 ** 32
    assert BC.POOL_HUGE["N"] * (BC.POOL_HUGE["HW"] // 4) * BC.POOL_HUGE["C"] // 8 >= 2 ** 32
