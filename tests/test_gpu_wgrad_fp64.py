"""GPU parity of the convolution weight-gradient kernels (rpnet_conv_wgrad, rpnet_conv_wgrad_up4, rpnet_conv1_wgrad) against the
float64 reference tests/ref64.py conv_wgrad, at every branch of their dispatch.  Every call goes through rpnet_amd.hip.call with a
descriptor of RF._desc(..., wgrad=True); dw and the workspace are prefilled with NaN, the workspace is exactly as long as the
*_workspace_bytes query says, with 64 guard words behind it.  The tables, the bound and every comparison live in
tests/wgrad_cases.py (shared with tests/test_host_wgrad_ref64.py, which shows on the CPU that the bound has room for a correct fp32
implementation and that seeded defects fail it).  Every arithmetic check prints `PARITY wgrad case what err yard ratio of_bound`;
profiles/wgrad_parity.txt keeps one run's lines."""
import ctypes as C

import pytest
import torch

from tests import wgrad_cases as WC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


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


def descriptor(hip, c, x0, x1, in_scale, accumulate, sx=None, sx1=None, sdy=None):
    from rpnet_amd import functional as RF
    d = RF._desc(x0, x1, None, None, in_scale, c.mode, None, None, c.N, c.H, c.W, c.taps, c.ups, accumulate=accumulate,
                 co_split=(c.cout, 0), wgrad=True)
    d.C0, d.C1 = c.C0, c.C1
    d.in_scale_mode, d.dilation, d.split_planes, d.tune = (c.mode if in_scale is not None else 0), c.dil, c.planes, c.tune
    d.acc_scale_x, d.acc_scale_x1, d.acc_scale_dy = hip.ptr(sx), hip.ptr(sx1), hip.ptr(sdy)
    return d


def query_workspace(hip, c):
    if c.fam == "conv1":
        return hip.query("rpnet_conv1_wgrad_workspace_bytes", c.N, c.H, c.W, c.cout)
    if c.fam == "up4":
        return hip.query("rpnet_conv_wgrad_up4_workspace_bytes", c.N, c.H, c.W, c.C0, c.cout)
    return hip.query("rpnet_conv_wgrad_workspace_bytes", c.N, c.H, c.W, c.Cin, c.cout, c.taps)


class HipBackend:
    """one launch of the library on CPU tensors (tests/wgrad_cases.py)"""

    def __init__(self, hip):
        self.hip = hip

    def run(self, c, o, dw_init=None, accumulate=0, phase="both", ws=None):
        hip, p = self.hip, self.hip.ptr
        wb = query_workspace(hip, c)
        assert wb == WC.workspace_bytes(c) and wb % 4 == 0, (c.id, wb, WC.workspace_bytes(c))
        words = wb // 4
        guard = torch.arange(1, WC.GUARD + 1, dtype=torch.float32, device=DEV)
        if ws is None:
            ws = dv(torch.full((words + WC.GUARD,), WC.NAN))
            ws[words:] = guard
        dw = dv(torch.full(WC.dw_shape(c), WC.NAN) if dw_init is None else dw_init.clone())
        x0, x1, dy = dv(o.x0), dv(o.x1), dv(o.dy)
        if c.fam == "conv1":
            hip.call("rpnet_conv1_wgrad", p(x0), p(dy), p(dw), c.N, c.H, c.W, c.cout, p(ws), wb)
        else:
            d = descriptor(hip, c, x0, x1, dv(o.in_scale), accumulate, scalar(o.sx), scalar(o.sx1), scalar(o.sdy))
            dyp, dwp = (None if phase == "reduce" else p(dy)), (None if phase == "gemm" else p(dw))
            if c.fam == "up4":
                assert hip.query("rpnet_conv_wgrad_up4_supported", C.byref(d)) == 1, c.id
                hip.call("rpnet_conv_wgrad_up4", C.byref(d), dyp, dwp, p(ws), wb)
            else:
                hip.call("rpnet_conv_wgrad", C.byref(d), dyp, dwp, *c.map, p(ws), wb)
        torch.cuda.synchronize()
        return WC.Out(dw.cpu(), ws, bool(torch.equal(ws[words:], guard)))


@pytest.fixture(scope="module")
def be(hip):
    return HipBackend(hip)


def ident(c):
    return c.id


@pytest.mark.parametrize("c", WC.FP32_9, ids=ident)
def test_fp32_dense_3x3(be, c):
    """rpnet_conv_wgrad on fp32 operands, conv_wgrad9_kernel<P2, IS>, inside rpnet_conv_wgrad_workspace_bytes"""
    WC.hold(WC.check_row(be, c))


@pytest.mark.parametrize("c", WC.FP32_TAP, ids=ident)
def test_fp32_1x1_and_dilated(be, c):
    """rpnet_conv_wgrad on fp32 operands, conv_wgrad_kernel<WM, WN>: 1 x 1 and dilation 2"""
    WC.hold(WC.check_row(be, c))


@pytest.mark.parametrize("c", WC.PLANES9, ids=ident)
def test_planes_dense_3x3(be, c):
    """rpnet_conv_wgrad on three, two and one plane: the register-staged, the LDS-DMA and the ring kernel, every launch inside
    rpnet_conv_wgrad_workspace_bytes, one call and two-phase"""
    WC.hold(WC.check_row(be, c))


def test_ring_kernel_equals_the_row_major_kernel_at_w32(be):
    WC.hold(WC.check_ring_equals_row_major(be))


@pytest.mark.parametrize("c", WC.PLANES1, ids=ident)
def test_planes_1x1(be, c):
    """rpnet_conv_wgrad, conv_wgrad1_split_kernel<NP>: pad rows, acc_scale_x1, the split cap"""
    WC.hold(WC.check_row(be, c))


@pytest.mark.parametrize("c", WC.UP4, ids=ident)
def test_collapsed_up_conv(be, c):
    """rpnet_conv_wgrad_up4 inside rpnet_conv_wgrad_up4_workspace_bytes, and rpnet_conv_wgrad with d->upsample on the same operands"""
    WC.hold(WC.check_row(be, c) + WC.check_up4_against_nine_tap(be, c))


@pytest.mark.parametrize("label,c,runs", WC.UP4_UNSUPPORTED, ids=[r[0] for r in WC.UP4_UNSUPPORTED])
def test_collapsed_up_conv_turns_away(hip, be, label, c, runs):
    h, w = c.H >> 1, c.W >> 1
    x0 = dv(torch.zeros(max(c.planes, 1), c.N, h, w, c.C0, dtype=torch.int16))
    x1 = dv(torch.zeros(max(c.planes, 1), c.N, h, w, c.C1, dtype=torch.int16)) if c.C1 else None
    s = scalar(1.0)
    d = descriptor(hip, c, x0, x1, None, 0, s, None, s)
    assert hip.query("rpnet_conv_wgrad_up4_supported", C.byref(d)) == 0
    if runs:
        WC.hold(WC.check_up4_against_nine_tap(be, c))


@pytest.mark.parametrize("c", WC.CONV1, ids=ident)
def test_first_layer(be, c):
    """rpnet_conv1_wgrad inside rpnet_conv1_wgrad_workspace_bytes"""
    WC.hold(WC.check_row(be, c))


@pytest.mark.parametrize("c", WC.DYNAMIC, ids=ident)
def test_dynamic_range(be, c):
    """rpnet_conv_wgrad / rpnet_conv_wgrad_up4 on a dy whose channels span 2^-20 .. 2^0 under one tensor scale, per output channel"""
    WC.hold(WC.check_dynamic_range(be, c))


def test_refusals(hip):
    """every refusal happens on the host, before any launch: the status code, the entry point's name at the head of
    rpnet_last_error_string, and dw and the workspace untouched"""
    lib, p = hip.load(), hip.ptr
    big = 1 << 22
    x0, x1, dy, dw, ws = (dv(torch.full((big,), 7.0)) for _ in range(5))
    s = scalar(1.0)
    for label, base, ch, want in WC.REFUSALS:
        c = base.but(**{k: v for k, v in ch.items() if k in base.__dict__})
        c.map = (c.Cin, 0, c.Cin, c.Cin)
        null = set(ch.get("null", "").split(","))
        phase = ch.get("phase", "both")
        buf = {n: (None if n in null else t) for n, t in (("x0", x0), ("x1", x1), ("dy", dy), ("dw", dw), ("ws", ws))}
        if phase == "gemm":
            buf["dw"] = None
        if phase == "reduce":
            buf["dy"] = None
        if c.fam == "conv1":
            wb = big * 4 if "ws_short" not in ch else query_workspace(hip, c) - 1
            got = lib.rpnet_conv1_wgrad(p(buf["x0"]), p(buf["dy"]), p(buf["dw"]), c.N, c.H, c.W, c.cout, p(buf["ws"]), wb, hip.stream())
        else:
            d = descriptor(hip, c, x0, x1 if c.C1 else None, dy if c.mode else None, 0, *((None,) * 3 if "no_scales" in ch or not 0 < c.planes < 3 else (s, None, s)))
            d.x0, d.x1 = p(buf["x0"]), (p(buf["x1"]) if c.C1 else None)
            if "huge" in ch:
                d.N, d.H, d.W = ch["huge"]
            if c.fam == "up4":
                wb = big * 4 if "ws_short" not in ch else query_workspace(hip, c) - 1
                got = lib.rpnet_conv_wgrad_up4(C.byref(d), p(buf["dy"]), p(buf["dw"]), p(buf["ws"]), wb, hip.stream())
            else:
                wb = big * 4 if "ws_short" not in ch else WC.launch_plan(c)[0] * c.taps * c.Cin * c.cout * 4 - 1
                got = lib.rpnet_conv_wgrad(C.byref(d), p(buf["dy"]), p(buf["dw"]), *c.map, p(buf["ws"]), wb, hip.stream())
        msg = lib.rpnet_last_error_string().decode()
        assert got == want, f"{c.entry} ({label}): rc {got}, expected {want}: {msg}"
        assert msg.startswith(c.entry[len("rpnet_"):] + ":"), f"{c.entry} ({label}): the message does not start with the entry point: {msg!r}"
    torch.cuda.synchronize()
    assert bool((dw == 7.0).all()) and bool((ws == 7.0).all())               # nothing ran
