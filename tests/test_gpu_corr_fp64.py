"""GPU parity of the local-window correlation kernels (csrc/corr.hip: fp32 VALU, radius 1..7; csrc/corr_split.hip: MFMA on three
bf16 planes or two / one fp16 planes, radius 5; corr_transpose_kernel between the two backward passes) against the float64
references of tests/ref64.py, at every dispatch edge.  Every call goes through rpnet_amd.hip.call directly; outputs are prefilled
with NaN so that an unwritten element shows.  The tables, the bound and every comparison live in tests/corr_cases.py (shared with
tests/test_host_corr_ref64.py, which shows on the CPU that the bound has room for a correct fp32 implementation and that seeded
defects fail it).  Every arithmetic check prints `PARITY corr family what err yard ratio`; profiles/corr_parity.txt keeps one
run's lines."""
import pytest
import torch

from tests import corr_cases as CC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN16 = 0x7e00          # an fp16 NaN: the prefill of the planes the forward writes


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
    """device copy, referenced until the test ends: a temporary whose pointer went into a call must not be freed (and its
    memory handed to the next temporary of the same argument list) before the launch"""
    if t is None:
        return None
    _ALIVE.append(t.to(DEV).contiguous())
    return _ALIVE[-1]


def nans(*shape):
    _ALIVE.append(torch.full(shape, float("nan"), device=DEV))
    return _ALIVE[-1]


def scalar(v):
    return None if v is None else dv(torch.tensor([v], dtype=torch.float32))


class HipBackend:
    """the five entry points of the library on CPU tensors (tests/corr_cases.py)"""

    def __init__(self, hip):
        self.hip = hip

    def _ws(self, B, h, w, cstride):
        wb = self.hip.query("rpnet_local_corr_bwd_workspace_bytes", B, h, w, cstride)
        assert wb == B * h * w * cstride * 4
        _ALIVE.append(torch.empty(max(wb, 16), device=DEV, dtype=torch.uint8))
        return _ALIVE[-1], wb

    def fwd32(self, f1, f2, r, cstride):
        B, h, w, C = f1.shape
        corr, p = nans(B, h, w, cstride), self.hip.ptr
        self.hip.call("rpnet_local_corr_fwd", p(dv(f1)), p(dv(f2)), p(corr), B, h, w, C, r, cstride)
        return corr.cpu()

    def bwd32(self, f1, f2, dcorr, r, cstride, add):
        B, h, w, C = f1.shape
        df1, df2, p = nans(B, h, w, C), nans(B, h, w, C), self.hip.ptr
        ws, wb = self._ws(B, h, w, cstride)
        self.hip.call("rpnet_local_corr_bwd", p(dv(f1)), p(dv(f2)), p(dv(dcorr)), p(df1), p(df2), B, h, w, C, r, cstride, p(dv(add)),
                      p(ws), wb)
        return df1.cpu(), df2.cpu()

    def split_fwd(self, p1, p2, s1, s2, planes, shape, cstride, want_absmax, cscale):
        B, h, w, C = shape
        corr, p = nans(B, h, w, cstride), self.hip.ptr
        mx = dv(torch.zeros(1)) if want_absmax else None
        cpl = dv(torch.full((planes, B, h, w, cstride), NAN16, dtype=torch.int16)) if cscale is not None else None
        self.hip.call("rpnet_local_corr_split_fwd", p(dv(p1)), p(dv(p2)), p(corr), B, h, w, C, 5, cstride, planes, p(scalar(s1)),
                      p(scalar(s2)), p(mx), p(cpl), p(scalar(cscale)))
        return corr.cpu(), (None if mx is None else mx.cpu()), (None if cpl is None else cpl.cpu())

    def split_bwd(self, p1, p2, s1, s2, dcorr, planes, shape, cstride, add):
        B, h, w, C = shape
        df1, df2, p = nans(B, h, w, C), nans(B, h, w, C), self.hip.ptr
        ws, wb = self._ws(B, h, w, cstride)
        self.hip.call("rpnet_local_corr_split_bwd", p(dv(p1)), p(dv(p2)), p(dv(dcorr)), p(df1), p(df2), B, h, w, C, 5, cstride, planes,
                      p(scalar(s1)), p(scalar(s2)), p(dv(add)), p(ws), wb)
        return df1.cpu(), df2.cpu()

    def split_f16(self, x, scale, planes):
        """rpnet_split_f16 of the tensor on the given scale (element-wise: run over the flat tensor, padded to rows of 8)"""
        n = x.numel()
        n8 = (n + 7) // 8 * 8
        flat = torch.zeros(n8)
        flat[:n] = x.reshape(-1)
        out, p = dv(torch.full((planes, n8), NAN16, dtype=torch.int16)), self.hip.ptr
        self.hip.call("rpnet_split_f16", p(dv(flat)), None, 0, p(scalar(scale)), None, None, p(out), n8 // 8, 8, planes, 0)
        return out.cpu()[:, :n].reshape((planes,) + tuple(x.shape))


@pytest.fixture(scope="module")
def be(hip):
    return HipBackend(hip)


def ident(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("r,shape,cstride", CC.FP32_CASES, ids=ident)
def test_fp32(be, r, shape, cstride):
    CC.hold(CC.check_fp32(be, r, shape, cstride))


@pytest.mark.parametrize("r,shape,cstride", CC.FP32_FWD_ONLY, ids=ident)
def test_fp32_forward_at_channel_counts_that_are_no_multiple_of_64(be, r, shape, cstride):
    CC.hold(CC.check_fp32(be, r, shape, cstride, backward=False))


@pytest.mark.parametrize("planes,bhw,C,cstride", CC.SPLIT_FWD_CASES, ids=ident)
def test_split_forward(be, planes, bhw, C, cstride):
    CC.hold(CC.check_split_fwd(be, planes, bhw, C, cstride))


@pytest.mark.parametrize("planes,bhw,C,cstride", CC.SPLIT_BWD_CASES, ids=ident)
def test_split_backward(be, planes, bhw, C, cstride):
    CC.hold(CC.check_split_bwd(be, planes, bhw, C, cstride))


@pytest.mark.parametrize("planes,C", CC.DYNAMIC_CASES)
def test_split_backward_dynamic_range(be, planes, C):
    CC.hold(CC.check_dynamic_range(be, planes, C))


def test_cross_path(be):
    """r = 5, C = 128, 3 x 9 x 17: the fp32 kernels, the three-plane kernels and the autograd Function under each conv_math meet
    the same float64 reference; the Function's alias gradient is summed into df1"""
    from rpnet_amd import functional as RF
    assert all(RF.corr_stride(r) == CC.corr_stride(r) for r in range(1, 8))
    CC.hold(CC.check_cross_path(be))
    f1, f2, dcorr, add = CC.cross_path_inputs()
    old = RF.conv_math()
    try:
        for math in ("f32", "bf16x3", "f16x2", "f16"):
            RF.set_conv_math(math)
            a, b = dv(f1).clone().requires_grad_(True), dv(f2).clone().requires_grad_(True)
            out, alias = RF.LocalCorr.apply(a, b, 5)
            torch.autograd.backward([out, alias], [dv(dcorr), dv(add)])
            # plain tensors carry no fp16 planes: every split mode runs the Function on three bf16 planes
            CC.hold(CC.cross_path_records(f"Function({math})", out.detach().cpu(), a.grad.cpu(), b.grad.cpu(), 0 if math == "f32" else 3))
    finally:
        RF.set_conv_math(old)


def test_refusals(hip):
    """every refusal happens on the host, before any launch: the status code, the entry point's name in rpnet_last_error_string,
    and no output touched"""
    def buf(n):
        _ALIVE.append(torch.full((n,), 7.0, device=DEV))
        return _ALIVE[-1]
    rows, outputs = CC.refusals(buf)
    lib = hip.load()
    for label, entry, args, want in rows:
        got = getattr(lib, entry)(*[hip.ptr(a) if torch.is_tensor(a) else a for a in args], hip.stream())
        msg = lib.rpnet_last_error_string().decode()
        assert got == want, f"{entry} ({label}): rc {got}, expected {want}: {msg}"
        assert entry[len("rpnet_"):] in msg, f"{entry} ({label}): the message does not name the entry point: {msg!r}"
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outputs)               # nothing ran
