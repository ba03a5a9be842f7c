"""CPU: the eval-mode / image-gradient fixture (tests/golden/autograd_m64.npz) against the oracle, and the ABI of the entry
points behind them (no GPU needed)."""
import os
import re

import numpy as np
import torch

from tests.helpers import episode_tensors, in_checksum, load_cfg, rel_err, rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rpnet_bn_eval_relu", "rpnet_bn_eval_bwd", "rpnet_conv1_dgrad_bn")


def _oracle_case(g, training):
    from oracle import rpnet_oracle as O
    size, B, T, seed = (int(v) for v in g["meta"])
    (si, fg, bg, qi, ql, appr), ep = episode_tensors(seed, B, size)
    assert np.allclose(in_checksum(ep), g["in_checksum"], rtol=0, atol=1e-6), "synthetic inputs drifted"
    cfg = load_cfg(T)
    P = O.seeded_params(cfg["mask_refinement_correlation_radius"], requires_grad=True)
    s0, q0 = si[0][0].clone().requires_grad_(True), qi[0].clone().requires_grad_(True)
    out = O.rp_net_forward(P, cfg, [[s0]], fg, bg, [q0], appr, training, align=True)
    loss = O.total_loss(out, ql, cfg["align_loss_scaler"])
    loss.backward()
    return P, out, loss, s0.grad, q0.grad


def test_oracle_eval_mode_matches_autograd_fixture(golden):
    """model.eval() + backward in the oracle (training=False: running statistics) == the reference's fixture, with the
    running buffers unchanged"""
    g = golden("autograd_m64")
    from oracle import rpnet_oracle as O
    before = {k: v.clone() for k, v in O.seeded_params().items() if "running" in k or "num_batches" in k}
    P, out, loss, sg, qg = _oracle_case(g, False)
    for k, v in before.items():
        assert torch.equal(P[k], v), k
    assert rel_err(loss, g["eval.loss"]) < 1e-5
    assert rel_err(out["output"], g["eval.output"]) < 1e-4
    assert rel_l2(sg, g["eval.supp_img_grad"]) < 2e-3 and rel_l2(qg, g["eval.qry_img_grad"]) < 2e-3
    unused = set(str(u) for u in g["eval.unused"])
    for n, rn in zip(g["eval.grad_names"], g["eval.grad_norms"]):
        n = str(n)
        if n in unused:
            assert P[n].grad is None, n
            continue
        assert abs(P[n].grad.double().norm().item() - rn) <= 2e-3 * rn + 1e-7, n


def test_oracle_train_image_gradients_match_autograd_fixture(golden):
    g = golden("autograd_m64")
    _, _, loss, sg, qg = _oracle_case(g, True)
    assert rel_err(loss, g["train.loss"]) < 1e-5
    assert rel_l2(sg, g["train.supp_img_grad"]) < 2e-3 and rel_l2(qg, g["train.qry_img_grad"]) < 2e-3


def test_eval_gradient_entry_points_declared_and_bound():
    from rpnet_amd import hip
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rpnet_abi.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(rf"\bint {name}\s*\(", hdr), name
        assert name in hip.ABI_SYMBOLS, name
    assert hip.ABI_VERSION >= 109
    if os.path.exists(hip.lib_path()):
        import ctypes
        lib = ctypes.CDLL(hip.lib_path())
        for name in NEW:
            assert hasattr(lib, name), name
