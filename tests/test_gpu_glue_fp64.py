"""GPU parity of the launches that training runs per refinement iteration and per step — the fused refinement glue (csrc/refine.hip)
and the multi-tensor loss and objective (csrc/loss.hip) — against the float64 references of tests/ref64.py.  Every call goes through
rpnet_amd.hip.call directly, not the autograd Functions; every output is prefilled with NaN and stands inside a larger buffer with
GC.GUARD sentinel elements on both sides, so that an unwritten element and a write outside the output both show.  The tables, the
bound and every comparison live in tests/glue_cases.py (shared with tests/test_host_glue_ref64.py, which shows on the CPU that the
bound has room for a correct fp32 implementation and that seeded defects fail it).  Every arithmetic check prints
`PARITY glue family what err yard ratio`; profiles/glue_parity.txt keeps each family's largest ratio."""
import ctypes as C

import pytest
import torch

from tests import glue_cases as GC
from tests import operand_cases as OC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
SENTINEL = {torch.float32: -12345.0, torch.int16: 0x5A5A}


@pytest.fixture(scope="module")
def hip():
    from rpnet_amd import hip
    hip.load()
    return hip


_ALIVE = []


@pytest.fixture(autouse=True)
def _device_copies_live_until_the_test_ends():
    yield
    _ALIVE.clear()


def dv(t):
    """device copy, referenced until the test ends"""
    if t is None:
        return None
    _ALIVE.append(t.to(DEV).contiguous())
    return _ALIVE[-1]


def scalar(v):
    return None if v is None else dv(torch.tensor([v], dtype=torch.float32))


class Guarded:
    """an output of `shape`, prefilled with `fill`, between two bands of GC.GUARD sentinel elements"""

    def __init__(self, shape, dtype=torch.float32, fill=NAN):
        self.n = int(torch.Size(shape).numel())
        self.buf = torch.full((self.n + 2 * GC.GUARD,), SENTINEL[dtype], dtype=dtype, device=DEV)
        self.view = self.buf[GC.GUARD:GC.GUARD + self.n].view(shape)
        self.view.fill_(fill)
        assert self.view.data_ptr() % 16 == 0
        _ALIVE.append(self.buf)

    def ptr(self):
        return self.view.data_ptr()

    def touched(self):
        s = SENTINEL[self.buf.dtype]
        return int((self.buf[:GC.GUARD] != s).sum() + (self.buf[GC.GUARD + self.n:] != s).sum())

    def cpu(self):
        return self.view.cpu()


def gp(g):
    return None if g is None else g.ptr()


def pointer_array(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


class HipBackend:
    """the eight entry points of the library on CPU tensors (tests/glue_cases.py)"""

    def __init__(self, hip):
        self.hip = hip

    def glue_fwd(self, y, scale, shift, proto, scaler, want_mask, soft, x, xs, planes):
        hip, p = self.hip, self.hip.ptr
        B, h, w, Fc = y.shape
        K = proto.shape[1]
        Cx = x.shape[-1] if x is not None else 0
        assert hip.query("rpnet_refine_glue_supported", K, h, w, Fc, Cx, planes) == 1
        z = Guarded((B, h, w, Fc)) if scale is not None else None
        pred, logits = Guarded((B, K, h, w)), Guarded((B, K, 4 * h, 4 * w))
        mask = Guarded((B, h, w)) if want_mask else None
        xk = xq = None
        if x is not None:
            xk, xq = (Guarded((planes, B, h, w, Cx), torch.int16, OC.NAN16[planes]) for _ in range(2))
        hip.call("rpnet_refine_glue_fwd", p(dv(y)), p(dv(scale)), p(dv(shift)), p(dv(proto)), scaler, gp(z), gp(pred), gp(logits), gp(mask),
                 int(soft), p(dv(x)), p(scalar(xs)), gp(xk), gp(xq), planes, B, K, h, w, Fc, Cx)
        torch.cuda.synchronize()
        outs = {"z": z, "pred": pred, "logits": logits, "mask_next": mask, "xk": xk, "xq": xq}
        res = {k: (None if g is None else g.cpu()) for k, g in outs.items()}
        res["guards"] = sum(g.touched() for g in outs.values() if g is not None)
        return res

    def glue_bwd(self, dl, f, proto, scaler):
        hip, p = self.hip, self.hip.ptr
        B, h, w, Fc = f.shape
        K = proto.shape[1]
        wb = hip.query("rpnet_refine_glue_bwd_workspace_bytes", B, K, h, w, Fc)
        assert wb == GC.workspace_bytes(B, K, h, w)
        ws, df, dproto = Guarded((wb // 4,)), Guarded((B, h, w, Fc)), Guarded((B, K, Fc))
        hip.call("rpnet_refine_glue_bwd", p(dv(dl)), p(dv(f)), p(dv(proto)), scaler, df.ptr(), dproto.ptr(), B, K, h, w, Fc, ws.ptr(), wb)
        torch.cuda.synchronize()
        return df.cpu(), dproto.cpu(), ws.touched() + df.touched() + dproto.touched()

    def _listed(self, logits):
        """device copies of the listed tensors: a tensor listed twice is ONE device tensor, its pointer in both slots"""
        seen = {}
        for t in logits:
            if id(t) not in seen:
                seen[id(t)] = dv(t)
        return [seen[id(t)].data_ptr() for t in logits]

    def loss_fwd(self, kind, logits, weights, labels, extra, extra_scale):
        hip, p = self.hip, self.hip.ptr
        n = len(logits)
        B, K, H, W = logits[0].shape
        wb = n * hip.query("rpnet_loss_workspace_bytes", B, K, H, W)
        ws, loss, stats = Guarded((wb // 4,)), Guarded((n + 1,)), Guarded((n, B + 1, 2 * K + 2))
        ptrs = pointer_array(self._listed(logits))
        if kind == "multi":
            hip.call("rpnet_dice_ce_multi_fwd", ptrs, n, p(dv(labels)), loss.ptr(), stats.ptr(), B, K, H, W, ws.ptr(), wb)
        else:
            hip.call("rpnet_objective_fwd", ptrs, (C.c_float * n)(*weights), n, p(dv(labels)), p(dv(extra)), extra_scale, loss.ptr(),
                     stats.ptr(), B, K, H, W, ws.ptr(), wb)
        torch.cuda.synchronize()
        return loss.cpu(), stats.cpu(), ws.touched() + loss.touched() + stats.touched()

    def loss_bwd(self, kind, logits, weights, labels, stats, gscale, want_dextra, extra_scale):
        hip, p = self.hip, self.hip.ptr
        n = len(logits)
        B, K, H, W = logits[0].shape
        grads = [Guarded((B, K, H, W)) for _ in range(n)]
        dextra = Guarded((1,)) if want_dextra else None
        ptrs, gptrs = pointer_array(self._listed(logits)), pointer_array([g.ptr() for g in grads])
        if kind == "multi":
            hip.call("rpnet_dice_ce_multi_bwd", ptrs, gptrs, n, p(dv(labels)), p(dv(stats)), p(scalar(gscale)), B, K, H, W)
        else:
            hip.call("rpnet_objective_bwd", ptrs, gptrs, (C.c_float * n)(*weights), n, p(dv(labels)), p(dv(stats)), p(scalar(gscale)),
                     gp(dextra), extra_scale, B, K, H, W)
        torch.cuda.synchronize()
        touched = sum(g.touched() for g in grads) + (dextra.touched() if dextra is not None else 0)
        return [g.cpu() for g in grads], (None if dextra is None else dextra.cpu()), touched


@pytest.fixture(scope="module")
def be(hip):
    return HipBackend(hip)


def ident(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("shape,bn,mask,planes,C", GC.GLUE_FWD_CASES, ids=ident)
def test_glue_forward(be, shape, bn, mask, planes, C):
    """rpnet_refine_glue_fwd (after rpnet_refine_glue_supported says yes) without operand planes: z, pred, logits and the next mask"""
    GC.hold(GC.check_glue_fwd(be, shape, bn, mask, planes, C))


@pytest.mark.parametrize("shape,bn,mask,planes,C", GC.GLUE_PLANE_CASES, ids=ident)
def test_glue_forward_with_operand_planes(be, shape, bn, mask, planes, C):
    """rpnet_refine_glue_fwd with stage C: the planes of x * mask and x * (1 - mask), bit for bit from the kernel's own mask"""
    GC.hold(GC.check_glue_fwd(be, shape, bn, mask, planes, C))


def test_glue_hard_mask_of_a_tie_is_zero(be):
    """rpnet_refine_glue_fwd on two equal prototypes: softmax[1] is exactly 0.5 and the threshold is strict"""
    GC.hold(GC.check_glue_tie(be))


@pytest.mark.parametrize("shape,kind", GC.GLUE_BWD_CASES, ids=ident)
def test_glue_backward(be, shape, kind):
    """rpnet_refine_glue_bwd with exactly rpnet_refine_glue_bwd_workspace_bytes of workspace: df and dproto"""
    GC.hold(GC.check_glue_bwd(be, shape, kind))


@pytest.mark.parametrize("shape", GC.ZERO_PATCH_SHAPES, ids=ident)
def test_glue_zero_patch(be, shape):
    """rpnet_refine_glue_fwd and rpnet_refine_glue_bwd on a patch that is all zero after ReLU"""
    GC.hold(GC.check_glue_zero_patch(be, shape))


@pytest.mark.parametrize("row", GC.LOSS_ROWS, ids=ident)
def test_multi_loss_and_objective(be, row):
    """rpnet_dice_ce_multi_fwd / rpnet_dice_ce_multi_bwd and every form of rpnet_objective_fwd / rpnet_objective_bwd: stats, loss[z],
    total, every gradient and dextra"""
    GC.hold(GC.check_loss_row(be, row))


def test_glue_supported_answers(hip):
    """rpnet_refine_glue_supported: 0 or 1, consistently with the shapes the launchers refuse"""
    for args, want in GC.SUPPORTED:
        assert hip.query("rpnet_refine_glue_supported", *args) == want, args
    assert hip.query("rpnet_refine_glue_bwd_workspace_bytes", 3, 2, 16, 24, 64) == GC.workspace_bytes(3, 2, 16, 24)


def test_refusals(hip):
    """rpnet_refine_glue_fwd, rpnet_refine_glue_bwd, rpnet_dice_ce_multi_fwd, rpnet_dice_ce_multi_bwd, rpnet_objective_fwd and
    rpnet_objective_bwd: every refusal happens on the host, before any launch: the documented status code, a message that names the
    entry point, and no output touched"""
    def buf(n):
        _ALIVE.append(torch.full((n,), 7.0, device=DEV))
        return _ALIVE[-1]

    def ibuf(n):
        _ALIVE.append(torch.zeros(n, device=DEV, dtype=torch.int64))
        return _ALIVE[-1]

    def conv(a):
        if isinstance(a, GC.Ptrs):
            return pointer_array([None if t is None else t.data_ptr() for t in a])
        if isinstance(a, GC.Floats):
            return (C.c_float * len(a))(*a)
        return hip.ptr(a) if torch.is_tensor(a) else a

    rows, outputs = GC.refusals(buf, ibuf)
    lib = hip.load()
    for label, entry, args, want in rows:
        got = getattr(lib, entry)(*[conv(a) for a in args], hip.stream())
        msg = lib.rpnet_last_error_string().decode()
        assert got == want, f"{entry} ({label}): rc {got}, expected {want}: {msg}"
        assert msg != "" and entry[len("rpnet_"):] in msg, f"{entry} ({label}): the message does not name the entry point: {msg!r}"
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outputs)               # nothing ran
