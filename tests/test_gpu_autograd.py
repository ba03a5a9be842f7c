"""GPU: the gradients of the model contract beyond the training step — backward through eval-mode BatchNorm (running
statistics used, never written) and the gradients of the input images (eval and train mode), against the reference's own
fixture (tests/golden/autograd_m64.npz, gen_golden_autograd.py), the fp64 oracle and torch's fp64 autograd."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import episode_tensors, in_checksum, load_cfg, rel_err, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
YARD_EPS = 4e-7      # as tests/test_gpu_model.py: relative image perturbation of the fp64 yardstick
YARD_FLOOR = 5e-5


def _build(cfg, training):
    from rpnet_amd.modules import RP_Net
    from rpnet_amd.utils.seeding import seed_module_
    net = RP_Net(cfg={"align": True, "backbone": "UNet"}, backbone_cfg=cfg).to(DEV)
    seed_module_(net)
    net.train(training)
    return net


def _loss(out, ql, cfg):
    from rpnet_amd.functional import dice_ce
    loss = dice_ce(out["output"], ql)
    for v in out["refinement"].values():
        loss = loss + dice_ce(v, ql)
    return loss + cfg["align_loss_scaler"] * out["align_loss"]


def _images(si, qi):
    for way in si:
        for s in way:
            s.requires_grad_(True)
    qi[0].requires_grad_(True)


def _hip_step(cfg, inputs, training, net=None):
    """forward + backward of the HIP path with every image requiring grad -> (loss, output, {param: grad}, supp grads, qry grad)"""
    _, fg, bg, _, ql, appr = inputs
    si, qi = [[s.detach().clone() for s in w] for w in inputs[0]], [inputs[3][0].detach().clone()]
    _images(si, qi)
    net = net or _build(cfg, training)
    out = net(si, fg, bg, qi, appr_query_labels=appr)
    loss = _loss(out, ql, cfg)
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: p.grad for n, p in net.named_parameters() if p.grad is not None}
    return loss.detach(), out["output"].detach(), grads, [[s.grad for s in w] for w in si], qi[0].grad, net


def _oracle(cfg, inputs, training, noise=None):
    """the oracle in float64 through torch's own device kernels, images requiring grad -> ({name: grad}, loss, output,
    supp grads, qry grad); noise = (seed, eps): every image pixel times 1 + eps u, u uniform in [-1, 1]"""
    from oracle import rpnet_oracle as O
    si, fg, bg, qi, ql, appr = inputs
    dt = torch.float64
    P = {}
    for k, v in O.seeded_params(cfg["mask_refinement_correlation_radius"], requires_grad=True,
                                mask_feature_map=cfg.get("mask_feature_map", False)).items():
        t = v.detach().to(dt) if v.is_floating_point() else v.detach().clone()
        P[k] = t.to(DEV).clone().requires_grad_(v.requires_grad)
    gen = torch.Generator().manual_seed(noise[0]) if noise else None

    def img(t):
        t = t.detach().cpu().to(dt)
        if noise:
            t = t * (1.0 + noise[1] * (2.0 * torch.rand(t.shape, generator=gen, dtype=dt) - 1.0))
        return t.to(DEV).requires_grad_(True)
    si_d, qi_d = [[img(s) for s in w] for w in si], [img(qi[0])]
    c = lambda t: t.detach().to(dt).to(DEV)  # noqa: E731
    with torch.device(DEV):
        out = O.rp_net_forward(P, cfg, si_d, [[c(s) for s in w] for w in fg], [[c(s) for s in w] for w in bg], qi_d, c(appr),
                               training, align=True)
        loss = O.total_loss(out, ql.to(DEV), cfg["align_loss_scaler"])
        loss.backward()
    g = {k: v.grad.cpu() for k, v in P.items() if v.requires_grad and v.grad is not None}
    return g, loss.detach().cpu(), out["output"].detach().cpu(), [[s.grad.cpu() for s in w] for w in si_d], qi_d[0].grad.cpu()


def _yardstick(cfg, inputs, training, draws=4):
    """fp64 reference results and how far the fp64 gradients move (relative L2, max over draws) under YARD_EPS image noise"""
    g64, l64, o64, s64, q64 = _oracle(cfg, inputs, training)
    ref = dict(g64, **{f"img.s{i}": s for i, s in enumerate(x for w in s64 for x in w)}, **{"img.q": q64})
    yard = {}
    for d in range(draws):
        g, _, _, s, q = _oracle(cfg, inputs, training, noise=(300 + d, YARD_EPS))
        cur = dict(g, **{f"img.s{i}": v for i, v in enumerate(x for w in s for x in w)}, **{"img.q": q})
        for n, v in cur.items():
            nrm = float(ref[n].norm())
            if nrm >= 1e-4:
                yard[n] = max(yard.get(n, 0.0), float((v - ref[n]).norm()) / nrm)
    return ref, yard, l64, o64


def _check_vs_yardstick(got, ref, yard, what):
    bad = []
    for n, y in yard.items():
        e = rel_l2(got[n], ref[n])
        if e > 3.0 * y + YARD_FLOOR:
            bad.append(f"{n}: {e:.2e} (yardstick {y:.2e})")
    assert not bad, f"{what}: " + "; ".join(bad)


def _flat(grads, sgr, qgr):
    return dict({n: g.cpu() for n, g in grads.items()}, **{f"img.s{i}": s.cpu() for i, s in enumerate(x for w in sgr for x in w)},
                **{"img.q": qgr.cpu()})


@pytest.fixture(params=["bf16x3", "f16x2", "f32"])
def conv_math(request):
    from rpnet_amd import functional as RF
    from rpnet_amd import modules as RM
    RF.set_conv_math(request.param)
    RM._F16_MIN_PIXELS = 0          # the fp16 planes at every size (restored by tests/conftest.py)
    return request.param


def _fixture_inputs(golden):
    g = golden("autograd_m64")
    size, B, T, seed = (int(v) for v in g["meta"])
    inputs, ep = episode_tensors(seed, B, size, DEV)
    assert np.allclose(in_checksum(ep), g["in_checksum"], rtol=0, atol=1e-6), "synthetic inputs drifted"
    return g, load_cfg(T), inputs


_YARD = {}


def _cached_yardstick(tag, cfg, inputs, training):
    if tag not in _YARD:
        _YARD[tag] = _yardstick(cfg, inputs, training)
    return _YARD[tag]


def test_eval_gradients_vs_reference_fixture(golden, conv_math):
    """model.eval() + backward: loss, logits, gradient norms / heads and the image gradients of the reference; the running
    buffers and num_batches_tracked bit-identical before and after"""
    g, cfg, inputs = _fixture_inputs(golden)
    net = _build(cfg, False)
    bufs = {k: v.clone() for k, v in net.state_dict().items() if "running" in k or "num_batches" in k}
    loss, out, grads, sgr, qgr, _ = _hip_step(cfg, inputs, False, net)
    for k, v in net.state_dict().items():
        if k in bufs:
            assert torch.equal(v, bufs[k]), k
    assert rel_err(loss, g["eval.loss"]) < 1e-5
    assert rel_err(out, g["eval.output"]) < 1e-5
    ref, yard, _, _ = _cached_yardstick("eval64", cfg, inputs, False)
    unused = set(str(u) for u in g["eval.unused"])
    for n, rn, head in zip(g["eval.grad_names"], g["eval.grad_norms"], g["eval.grad_heads"]):
        n = str(n)
        if n in unused:
            assert n not in grads, n
            continue
        e = abs(grads[n].double().norm().item() - rn) / rn
        if n.startswith("encoder."):      # conditioned by ReLU / max-pool switches: the measured yardstick (test_model_vs_golden)
            # (floor 1e-5: the fp32 round-off of the reference's own sums — in eval mode the yardstick falls to ~1e-8)
            assert e <= 6.0 * yard[n] + 1e-5, f"grad norm {n}: rel {e:.2e}, yardstick {yard[n]:.2e}"
            continue
        assert e < 1e-3, f"grad norm {n}: rel {e:.2e}"
        k = min(32, grads[n].numel())
        hd = torch.from_numpy(head[:k])
        assert (grads[n].flatten()[:k].cpu() - hd).abs().max() / (hd.abs().max() + 1e-12) < 4e-3, f"grad head {n}"
    for got, key, yk in ((sgr[0][0], "eval.supp_img_grad", "img.s0"), (qgr, "eval.qry_img_grad", "img.q")):
        # both within 3 yardsticks of the fp64 oracle: within 6 of each other
        assert rel_l2(got, torch.from_numpy(g[key])) <= 6.0 * yard[yk] + 2 * YARD_FLOOR, key


@pytest.mark.parametrize("size", [64, 128])
def test_eval_gradients_vs_fp64_yardstick(size):
    """every parameter gradient and both image gradients of an eval-mode backward against the fp64 oracle (training=False)"""
    from rpnet_amd import modules as RM
    RM._F16_MIN_PIXELS = 0
    cfg = load_cfg(2)
    inputs, _ = episode_tensors(1021 + size, 2 if size == 64 else 1, size, DEV)
    ref, yard, l64, o64 = _yardstick(cfg, inputs, False)
    loss, out, grads, sgr, qgr, _ = _hip_step(cfg, inputs, False)
    assert rel_err(out, o64) < 1e-4 and rel_err(loss, l64) < 1e-5
    got = _flat(grads, sgr, qgr)
    assert set(got) >= set(yard)
    _check_vs_yardstick(got, ref, yard, f"eval {size}^2")


TRAIN_ROWS = {
    "default": {},
    "no_bn_fuse": {"fuse": False},
    "no_recomp": {"recomp": False},
    "mfm_x": {"mfm": "x"},
    "mfm_x2": {"mfm": "x2"},
    "mfm_x3": {"mfm": "x3"},
    "2way": {"ways": 2},
}


@pytest.mark.parametrize("row", list(TRAIN_ROWS))
def test_train_image_gradients(golden, row):
    """train mode: the gradients of the support and query images, with and without the first-layer shortcuts
    (_CONV1_BN_FUSE, _CONV1_RECOMP: the latter only runs on fp16 planes), the mask channels and a 2-way episode"""
    from rpnet_amd import functional as RF
    from rpnet_amd import modules as RM
    opt = TRAIN_ROWS[row]
    RM._F16_MIN_PIXELS = 0
    saved = (RF._CONV1_BN_FUSE, RF._CONV1_RECOMP)
    RF._CONV1_BN_FUSE, RF._CONV1_RECOMP = opt.get("fuse", True), opt.get("recomp", True)
    try:
        if row == "default":
            g, cfg, inputs = _fixture_inputs(golden)
        else:
            cfg = load_cfg(2)
            if "mfm" in opt:
                cfg["mask_feature_map"] = opt["mfm"]
            inputs, _ = episode_tensors(1031, 2, 64, DEV, n_ways=opt.get("ways", 1))
        RF.reset_arith()
        loss, out, grads, sgr, qgr, _ = _hip_step(cfg, inputs, True)
        counts = RF.arith_counts()
        if row == "default":
            assert rel_err(loss, g["train.loss"]) < 1e-4
        ref, yard, _, _ = _yardstick(cfg, inputs, True)
        got = _flat(grads, sgr, qgr)
        img = {n: y for n, y in yard.items() if n.startswith("img.")}
        assert len(img) == 1 + sum(len(w) for w in inputs[0])
        _check_vs_yardstick(got, ref, img, f"train {row}")
        if row == "default":
            for got_t, key, yk in ((sgr[0][0], "train.supp_img_grad", "img.s0"), (qgr, "train.qry_img_grad", "img.q")):
                assert rel_l2(got_t, torch.from_numpy(g[key])) <= 6.0 * yard[yk] + 2 * YARD_FLOOR, key
            # the first layer ran without its pre-BatchNorm tensor (the fp16 shortcut) and still gave the image gradient
            assert counts.get("bn_bwd", {}).get("first layer made again from the image", 0) >= 1, counts
    finally:
        RF._CONV1_BN_FUSE, RF._CONV1_RECOMP = saved


def test_instance_norm_image_gradient():
    """unet_normalize_type InstanceNorm2d (per-image statistics in both modes): Conv1's block, the image's gradient against
    torch's fp64 modules"""
    from rpnet_amd.modules import conv_block
    torch.manual_seed(5)
    m = conv_block(1, 64, "InstanceNorm2d").to(DEV)
    ref = torch.nn.Sequential(torch.nn.Conv2d(1, 64, 3, padding=1), torch.nn.InstanceNorm2d(64), torch.nn.ReLU(),
                              torch.nn.Conv2d(64, 64, 3, padding=1), torch.nn.InstanceNorm2d(64), torch.nn.ReLU()).double()
    with torch.no_grad():
        for i in (0, 3):
            ref[i].weight.copy_(m.conv[i].weight.double().cpu())
            ref[i].bias.copy_(m.conv[i].bias.double().cpu())
    for training in (True, False):
        m.train(training)
        x = torch.randn(3, 1, 48, 40, generator=torch.Generator().manual_seed(6))
        xg = x.to(DEV).requires_grad_(True)
        gz = torch.randn(3, 64, 48, 40, generator=torch.Generator().manual_seed(7))
        (m(xg) * gz.to(DEV)).sum().backward()
        xr = x.double().requires_grad_(True)
        (ref(xr) * gz.double()).sum().backward()
        assert xg.grad is not None and rel_l2(xg.grad, xr.grad) < 1e-4, training


def test_no_grad_eval_unchanged(conv_math):
    """an eval forward with autograd on gives the logits of the torch.no_grad call (bit-identical on fp32 arithmetic), and the
    no_grad calls around it are those of a model that never saw one (f16x2: the second call runs on predicted scales)"""
    cfg = load_cfg(2)
    (si, fg, bg, qi, ql, appr), _ = episode_tensors(1041, 2, 64, DEV)
    plain, net = _build(cfg, False), _build(cfg, False)
    with torch.no_grad():
        ref = [plain(si, fg, bg, qi, appr_query_labels=appr)["output"].clone() for _ in range(2)]
        first = net(si, fg, bg, qi, appr_query_labels=appr)["output"].clone()
    out = net(si, fg, bg, qi, appr_query_labels=appr)["output"]
    assert out.requires_grad
    if conv_math == "f32":
        assert torch.equal(out.detach(), ref[0])
    else:
        assert rel_err(out.detach(), ref[0]) < 1e-6
    with torch.no_grad():
        second = net(si, fg, bg, qi, appr_query_labels=appr)["output"]
    assert torch.equal(first, ref[0]) and torch.equal(second, ref[1])


def test_eval_fine_tuning():
    """test-time fine-tuning with frozen BatchNorm statistics: 20 Adam steps in eval mode lower the loss on a fixed 128^2
    episode and leave every running buffer untouched"""
    cfg = load_cfg(2)
    (si, fg, bg, qi, ql, appr), _ = episode_tensors(1051, 2, 128, DEV)
    net = _build(cfg, False)
    net.freeze_packs = True             # ignored while autograd is on: the weights change every step
    bufs = {k: v.clone() for k, v in net.state_dict().items() if "running" in k or "num_batches" in k}
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    losses = []
    for _ in range(20):
        opt.zero_grad(set_to_none=True)
        loss = _loss(net(si, fg, bg, qi, appr_query_labels=appr), ql, cfg)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < 0.9 * losses[0], losses
    for k, v in net.state_dict().items():
        if k in bufs:
            assert torch.equal(v, bufs[k]), k
    with torch.no_grad():               # a frozen call after the steps sees the new weights, not packs of an earlier step
        a = net(si, fg, bg, qi, appr_query_labels=appr)["output"].clone()
        net.freeze_packs = False
        b = net(si, fg, bg, qi, appr_query_labels=appr)["output"]
    assert torch.equal(a, b)


# ----------------------------------------------------------------------------------------------------------- kernels
def _f64_bn_eval_bwd(y, dz, gamma, beta, rm, rv):
    yd = y.double().requires_grad_(True)
    g, b = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    z = F.relu(F.batch_norm(yd, rm.double(), rv.double(), g, b, False, 0.1, 1e-5))
    z.backward(dz.double())
    return yd.grad, g.grad, b.grad


@pytest.mark.parametrize("N,H,W,C,groups", [(2, 13, 11, 72, 1), (4, 9, 7, 200, 2), (3, 16, 16, 40, 3), (2, 5, 3, 24, 1)])
def test_bn_eval_bwd_kernel(N, H, W, C, groups):
    from rpnet_amd import hip
    from rpnet_amd.hip import call, ptr, query
    torch.manual_seed(N * 1000 + C)
    y = torch.randn(N, C, H, W) * 2 + 0.3
    dz = torch.randn(N, C, H, W)
    gamma, beta = torch.randn(C), torch.randn(C)
    rm, rv = torch.randn(C) * 0.5, torch.rand(C) + 0.2
    dy64, dg64, db64 = _f64_bn_eval_bwd(y, dz, gamma, beta, rm, rv)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)  # noqa: E731
    yd, dzd = nhwc(y), nhwc(dz)
    g_, b_, rm_, rv_ = (t.to(DEV) for t in (gamma, beta, rm, rv))
    st = torch.empty(4, groups, C, device=DEV)
    sc, sh = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    call("rpnet_bn_eval_affine", ptr(g_), ptr(b_), ptr(rm_), ptr(rv_), 1e-5, ptr(sc), ptr(sh), C)
    st[0], st[1], st[2], st[3] = sc, sh, rm_, torch.rsqrt(rv_ + 1e-5)
    wsb = query("rpnet_bn_workspace_bytes", C, groups)
    ref_dy = dy64.permute(0, 2, 3, 1)
    results = []
    for planes in (0, 3, 2):
        ws = torch.empty(wsb, device=DEV, dtype=torch.uint8)
        dy = torch.empty(N, H, W, C, device=DEV)
        dys = torch.empty((planes, N, H, W, C), device=DEV, dtype=torch.float16 if planes == 2 else torch.bfloat16) if planes else None
        s = torch.zeros(1, device=DEV)
        dg, db = torch.full((C,), 0.5, device=DEV), torch.full((C,), -0.25, device=DEV)
        call("rpnet_bn_eval_bwd", ptr(dzd), ptr(yd), ptr(st[0]), ptr(st[1]), ptr(st[2]), ptr(st[3]), ptr(dy), ptr(dys), planes,
             ptr(s) if planes == 2 else None, ptr(dg), ptr(db), N, H * W, C, groups, 1, ptr(ws), wsb)
        torch.cuda.synchronize()
        assert rel_err(dy, ref_dy) < 1e-6
        assert rel_err(dg - 0.5, dg64) < 1e-5 and rel_err(db + 0.25, db64) < 1e-5      # accumulate = 1
        coef = ws[query("rpnet_bn_bwd_coef_offset", C, groups):].view(torch.float32)[:groups * C * 2]
        assert torch.all(coef == 0)
        if planes == 3:
            assert rel_err(dys.float().sum(0), ref_dy) < 1e-6
        if planes == 2:
            sv = float(s)
            assert sv > 0 and float(dy.abs().max()) <= sv * 2 ** 15        # the bound holds: no fp16 plane can overflow
            assert rel_err(dys.float().sum(0) * sv, ref_dy) < 2e-6
            assert float(dys.float().abs().max()) < 65504
        results.append((dy.clone(), dg.clone(), db.clone()))
    for a, b in zip(results[0], results[1]):       # the planes forms write the same fp32 dy / parameter gradients
        assert torch.equal(a, b)


@pytest.mark.parametrize("N,H,W,cout,groups", [(2, 64, 64, 64, 2), (3, 37, 21, 64, 1), (1, 16, 48, 128, 1)])
def test_conv1_dgrad_bn_kernel(N, H, W, cout, groups):
    from rpnet_amd.hip import call, ptr
    gen = torch.Generator().manual_seed(cout + H)
    x = torch.randn(N, 1, H, W, generator=gen)
    w = torch.randn(cout, 1, 3, 3, generator=gen) * 0.3
    bias = torch.randn(cout, generator=gen) * 0.1
    dz = torch.randn(N, H, W, cout, generator=gen)
    st = torch.stack([torch.randn(groups, cout, generator=gen), torch.randn(groups, cout, generator=gen) * 0.2,
                      torch.randn(groups, cout, generator=gen) * 0.1, torch.rand(groups, cout, generator=gen) + 0.5])
    coef = torch.randn(groups, cout, 2, generator=gen) * 0.1
    xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
    y = torch.empty(N, H, W, cout, device=DEV)
    call("rpnet_conv1_fwd", ptr(xd), ptr(wd), ptr(bd), ptr(y), None, None, N, H, W, cout, None, None, 1)
    torch.cuda.synchronize()
    # the fp64 reference: dy formed from the same y (the ReLU switch is the kernel's own), then conv_transpose2d
    yc = y.cpu().double()
    gi = torch.arange(N) // (N // groups)
    sc, sh, mu, iv = (st[i][gi][:, None, None, :].double() for i in range(4))
    c1, c2 = coef[gi][:, None, None, :, 0].double(), coef[gi][:, None, None, :, 1].double()
    m = (y.cpu() * st[0][gi][:, None, None, :] + st[1][gi][:, None, None, :] > 0).double()
    dy = sc * (dz.double() * m - c1 - (yc - mu) * iv * c2)
    ref = F.conv_transpose2d(dy.permute(0, 3, 1, 2), w.double(), padding=1)
    ref0 = F.conv_transpose2d((sc * dz.double() * m).permute(0, 3, 1, 2), w.double(), padding=1)
    dzd, std, cfd = dz.to(DEV), st.to(DEV).contiguous(), coef.to(DEV).contiguous()
    outs = []
    for given_y in (True, False, True):
        dx = torch.full((N, H, W), float("nan"), device=DEV)
        call("rpnet_conv1_dgrad_bn", ptr(dzd), ptr(y) if given_y else None, ptr(std), ptr(cfd), ptr(wd), ptr(bd),
             None if given_y else ptr(xd), ptr(dx), N, H, W, cout, groups)
        torch.cuda.synchronize()
        assert rel_err(dx, ref[:, 0]) < 1e-5, given_y
        outs.append(dx.clone())
    assert torch.equal(outs[0], outs[2])          # deterministic: two runs, the same bits
    dx0 = torch.empty(N, H, W, device=DEV)
    call("rpnet_conv1_dgrad_bn", ptr(dzd), ptr(y), ptr(std), None, ptr(wd), None, None, ptr(dx0), N, H, W, cout, groups)
    torch.cuda.synchronize()
    assert rel_err(dx0, ref0[:, 0]) < 1e-5        # coef NULL: eval mode


def test_bn_eval_relu_kernel():
    from rpnet_amd.hip import call, ptr
    y = torch.randn(3, 7, 5, 44, device=DEV) * 3
    sc, sh = torch.randn(44, device=DEV), torch.randn(44, device=DEV)
    z = torch.empty_like(y)
    mx = torch.zeros(1, device=DEV)
    call("rpnet_bn_eval_relu", ptr(y), ptr(sc), ptr(sh), ptr(z), ptr(mx), 3 * 7 * 5, 44)
    torch.cuda.synchronize()
    ref = torch.relu(y.double() * sc.double() + sh.double())
    assert rel_err(z, ref) < 1e-6 and float(mx) == float(z.max())
