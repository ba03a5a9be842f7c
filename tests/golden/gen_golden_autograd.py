#!/usr/bin/env python3
"""Generate tests/golden/autograd_m64.npz from the REFERENCE itself: the gradients that the model contract owes beyond the
training step — backward through eval-mode BatchNorm (model.eval(), running statistics used and left unchanged) and the
gradients of the input images, in eval and in train mode.

Runs ONLY where the reference is mounted (never on the GPU box); reuses gen_golden.py's loader, seeding and checks.  The
reference's RP_Net runs on the CPU with the name-seeded parameters of rpnet_amd.utils.seeding on a seeded 64^2, B = 2, T = 3
episode; the oracle (training=False / True) is checked against it at fp32 round-off, so the fixture also pins the oracle.

    python tests/golden/gen_golden_autograd.py
"""
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gen_golden as G  # noqa: E402  (loads the reference as package `refnet`)
from gen_golden import CFG, O, build_ref, close, save, to_t  # noqa: E402
from rpnet_amd.utils.synth import make_episode  # noqa: E402

SIZE, B, T, SEED = 64, 2, 3, 1011


def _case(training):
    """one forward + backward of the reference with both images requiring grad; the oracle checked against it"""
    cfg = dict(CFG)
    cfg["n_iter_refinement"] = T
    net = build_ref(cfg)
    net.train(training)
    si, fg, bg, qi, ql, appr = to_t(make_episode(SEED, B, SIZE))
    si[0][0].requires_grad_(True)
    qi[0].requires_grad_(True)
    sd0 = {k: v.clone() for k, v in net.state_dict().items() if "running" in k or "num_batches" in k}
    out = net(si, fg, bg, qi, appr_query_labels=appr)
    loss = O.total_loss(out, ql, cfg["align_loss_scaler"])
    loss.backward()
    if not training:       # eval mode: the running statistics are read, never written
        for k, v in net.state_dict().items():
            if k in sd0:
                assert torch.equal(v, sd0[k]), k
    fx = {"loss": loss.detach(), "output": out["output"].detach(), "supp_img_grad": si[0][0].grad, "qry_img_grad": qi[0].grad}
    params = dict(net.named_parameters())
    if not training:
        names = [n for n in params]
        fx["grad_names"] = np.array(names)
        fx["grad_norms"] = np.array([params[n].grad.double().norm().item() if params[n].grad is not None else 0.0 for n in names])
        fx["grad_heads"] = torch.stack([torch.nn.functional.pad(
            (params[n].grad if params[n].grad is not None else torch.zeros_like(params[n])).flatten()[:32],
            (0, max(0, 32 - params[n].numel()))) for n in names], 0)
        fx["unused"] = np.array([n for n in names if params[n].grad is None])
    # ---- the oracle on the same case, images requiring grad
    P = O.seeded_params(cfg["mask_refinement_correlation_radius"], requires_grad=True)
    osi, oqi = si[0][0].detach().clone().requires_grad_(True), qi[0].detach().clone().requires_grad_(True)
    o = O.rp_net_forward(P, cfg, [[osi]], fg, bg, [oqi], appr, training, align=True)
    ol = O.total_loss(o, ql, cfg["align_loss_scaler"])
    ol.backward()
    w = f"autograd_m64[training={training}]"
    close(o["output"], out["output"], 1e-4, w + ".output")
    close(ol, loss, 1e-5, w + ".loss")
    for nm, a, b in (("supp_img_grad", osi.grad, si[0][0].grad), ("qry_img_grad", oqi.grad, qi[0].grad)):
        e = (a - b).double().norm().item()
        assert e < 2e-3 * b.double().norm().item() + 1e-9, f"{w} {nm}: abs {e:.2e}"
    if not training:
        for n, p in params.items():
            if p.grad is None:
                assert P[n].grad is None, n
                continue
            e = (P[n].grad - p.grad).double().norm().item()
            assert e < 2e-3 * p.grad.double().norm().item() + 1e-7, f"{w} grad {n}: abs {e:.2e}"
    print(f"  oracle == reference on {w}")
    return fx


if __name__ == "__main__":
    assert os.path.isdir("/root/reference"), "gen_golden_autograd.py only runs where the reference is mounted"
    assert G.REF is not None
    ev, tr = _case(False), _case(True)
    ep = make_episode(SEED, B, SIZE)
    fx = {"meta": np.array([SIZE, B, T, SEED]),
          "in_checksum": np.array([float(ep["query_images"].astype(np.float64).sum()),
                                   float(ep["support_images"][0][0].astype(np.float64).sum()),
                                   float(ep["appr_query_labels"].sum()), float(ep["support_fg"][0][0].sum())])}
    fx.update({"eval." + k: v for k, v in ev.items()})
    fx.update({"train." + k: v for k, v in tr.items() if k in ("loss", "supp_img_grad", "qry_img_grad")})
    save("autograd_m64", **fx)
