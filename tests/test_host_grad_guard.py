"""The host side of the gradient guard (include/rpnet_guard_abi.h; rpnet_amd/optim.py): the clip formula against
torch.nn.utils.clip_grad_norm_, the guard block rpnet_grad_guard_init writes, and every refusal that needs no GPU (the library loads
on a CPU box; the entry points check their arguments before they launch anything, so made-up addresses serve)."""
import inspect
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from rpnet_amd import hip
from rpnet_amd.optim import FusedAdam, clip_coefficient, guard_block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = 0x7F0000000000
# struct rpnet_grad_guard
GUARD = np.dtype([("max_norm", "<f8"), ("skip_nonfinite", "<i8"), ("history_capacity", "<i8"), ("sumsq", "<f8"), ("norm", "<f8"),
                  ("coef", "<f8"), ("coef_f", "<f4"), ("skip", "<i4"), ("attempt", "<i8"), ("skipped", "<i8"), ("clipped", "<i8")])


@pytest.mark.parametrize("ratio", [0.25, 0.999, 1.0, 1.001, 2.0, 1e3])
def test_clip_coefficient_is_clip_grad_norm(ratio):
    """the factor by which clip_grad_norm_ multiplied an fp64 gradient, below the threshold, at it and above it"""
    rs = np.random.RandomState(3)
    grads = [torch.from_numpy(rs.standard_normal(k)) for k in (7, 64, 513)]
    norm = math.sqrt(sum(float((g * g).sum()) for g in grads))
    max_norm = norm / ratio                                      # ratio > 1: the norm is above the threshold
    ps = [torch.nn.Parameter(torch.zeros_like(g)) for g in grads]
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    assert abs(float(total) - norm) <= 1e-14 * norm
    want = clip_coefficient(float(total), max_norm)
    assert (want < 1.0) == (float(total) + 1e-6 > max_norm)
    for p, g in zip(ps, grads):
        big = g.abs() > 1e-3
        got = (p.grad[big] / g[big]).numpy()
        assert np.abs(got - want).max() <= 4 * np.finfo(np.float64).eps * want      # a product and a quotient rounded
    if ratio < 1.0:
        assert want == 1.0 and all(torch.equal(p.grad, g) for p, g in zip(ps, grads))


def test_clip_coefficient_edges():
    assert clip_coefficient(0.0, 1.0) == 1.0 and clip_coefficient(5.0, math.inf) == 1.0
    assert clip_coefficient(1.0, 1.0) == 1.0 / (1.0 + 1e-6) < 1.0            # AT the threshold the 1e-6 already clips, as in torch
    assert clip_coefficient(math.inf, 1.0) == 0.0
    assert math.isnan(clip_coefficient(math.nan, 1.0)) and math.isnan(clip_coefficient(math.inf, math.inf))


def test_guard_block_layout_and_refusals():
    assert GUARD.itemsize == 80
    hdr = open(os.path.join(ROOT, "include", "rpnet_guard_abi.h")).read()
    assert "sizeof(struct rpnet_grad_guard) == 80" in hdr
    rec = guard_block(2.5, True, 4).numpy().view(GUARD)[0]
    assert rec["max_norm"] == 2.5 and rec["skip_nonfinite"] == 1 and rec["history_capacity"] == 4
    assert all(rec[f] == 0 for f in GUARD.names[3:])
    assert guard_block(math.inf, False, 0).numpy().view(GUARD)[0]["max_norm"] == math.inf
    lib = hip.load()
    for max_norm, cap in ((0.0, 0), (-1.0, 0), (math.nan, 0), (1.0, -1)):
        buf = np.full(10, 7.0)
        assert lib.rpnet_grad_guard_init(buf.ctypes.data, max_norm, 0, cap) != 0
        assert lib.rpnet_last_error_string().decode().startswith("grad_guard_init")
        assert (buf == 7.0).all()                                # a refused call writes nothing
        with pytest.raises(ValueError, match="grad_guard_init"):
            guard_block(max_norm, False, cap)
    assert lib.rpnet_grad_guard_init(None, 1.0, 0, 0) != 0


def _step_args(**over):
    """made-up, well-aligned, distinct addresses for rpnet_adam_step_guarded (never dereferenced: every case below is refused)"""
    a = dict(table=BASE, n_chunks=3, grad=BASE + 0x1000, m=BASE + 0x2000, v=BASE + 0x3000, hyper=BASE + 0x4000,
             partials=BASE + 0x5000, guard=BASE + 0x6000, history=BASE + 0x7000)
    a.update(over)
    return a


@pytest.mark.parametrize("what, over", [
    ("null table", dict(table=None)), ("null grad", dict(grad=None)), ("null m", dict(m=None)), ("null hyper", dict(hyper=None)),
    ("null partials", dict(partials=None)), ("null guard", dict(guard=None)),
    ("no chunks", dict(n_chunks=0)),
    ("guard not 8-byte aligned", dict(guard=BASE + 0x6004)), ("partials not 8-byte aligned", dict(partials=BASE + 0x5004)),
    ("history not 8-byte aligned", dict(history=BASE + 0x7004)), ("grad not 4-byte aligned", dict(grad=BASE + 0x1002)),
    ("m is grad", dict(m=BASE + 0x1000)), ("partials is the guard", dict(partials=BASE + 0x6000)),
    ("history is the partials", dict(history=BASE + 0x5000)), ("guard is the hyper block", dict(guard=BASE + 0x4000)),
])
def test_step_and_sumsq_refusals(what, over):
    """a status and an error string, before anything is launched: this runs on a machine without a GPU"""
    lib = hip.load()
    a = _step_args(**over)
    rc = lib.rpnet_adam_step_guarded(a["table"], a["n_chunks"], a["grad"], a["m"], a["v"], a["hyper"], a["partials"], a["guard"],
                                     a["history"], None)
    err = lib.rpnet_last_error_string().decode()
    assert rc != 0 and err.startswith("adam_step_guarded") and len(err) > 22, (what, err)
    if not ({"m", "hyper"} & set(over)) and what != "guard is the hyper block":
        rc = lib.rpnet_grad_sumsq(a["table"], a["n_chunks"], a["grad"], a["partials"], a["guard"], a["history"], None)
        err = lib.rpnet_last_error_string().decode()
        assert rc != 0 and err.startswith("grad_sumsq") and len(err) > 15, (what, err)


def test_constructor_refusals_touch_no_gpu():
    """the guard's arguments are checked first: a bucket that would fail at the first attribute access is never looked at"""
    bucket = types.SimpleNamespace()
    for kw, exc in ((dict(max_grad_norm=0.0), ValueError), (dict(max_grad_norm=-1.0), ValueError),
                    (dict(max_grad_norm=math.nan), ValueError), (dict(history=-1), ValueError), (dict(history=2.5), TypeError),
                    (dict(skip_nonfinite="yes"), TypeError)):
        with pytest.raises(exc, match="FusedAdam"):
            FusedAdam(bucket, **kw)
    with pytest.raises(AttributeError):
        FusedAdam(bucket, max_grad_norm=1.0)                    # valid guard arguments: the bucket is looked at next
    names = list(inspect.signature(FusedAdam.__init__).parameters)
    assert names == ["self", "bucket", "lr", "betas", "eps", "weight_decay", "grad_scale", "max_grad_norm", "skip_nonfinite", "history"]
    d = {k: v.default for k, v in inspect.signature(FusedAdam.__init__).parameters.items()}
    assert d["max_grad_norm"] is None and d["skip_nonfinite"] is False and d["history"] == 0


def test_driver_options_and_refusal():
    from train_rpnet import train
    sig = inspect.signature(train).parameters
    assert sig["clip_grad_norm"].default is None and sig["skip_nonfinite"].default is False and sig["optimizer"].default == "torch"
    with pytest.raises(ValueError, match="skip_nonfinite"):
        train({}, steps=1, batch=1, size=64, dev="cpu", optimizer="torch", skip_nonfinite=True)
    with pytest.raises(ValueError, match="clip_grad_norm"):
        train({}, steps=1, batch=1, size=64, dev="cpu", clip_grad_norm=0.0)
    script = os.path.join(ROOT, "train_rpnet.py")
    out = subprocess.run([sys.executable, script, "--skip_nonfinite", "--optimizer", "torch"], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 2 and "--skip_nonfinite needs --optimizer fused" in out.stderr, out.stderr
    out = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "--clip_grad_norm" in out.stdout and "--skip_nonfinite" in out.stdout
    import yaml
    cfg = yaml.load(open(os.path.join(ROOT, "yamls", "example.yml")), Loader=yaml.FullLoader)
    assert "clip_grad_norm" not in cfg and "skip_nonfinite" not in cfg          # absent keys: the feature is off by default
