"""GPU parity of the first-layer (Cin = 1) kernels of csrc/conv_first.hip against the float64 references of tests/ref64.py, at every
branch of their dispatch.  Every call goes through the C ABI (rpnet_amd.hip.call / ptr), never through the autograd Functions; every
output and workspace is prefilled with NaN, is exactly as long as its query says and has 64 guard words behind it.  The tables, the
bound and every comparison live in tests/conv1_cases.py (shared with tests/test_host_conv1_ref64.py, which shows on the CPU that the
bound has room for a correct fp32 implementation, that no row leaves an element of the ReLU switch undecided and that seeded defects
fail).  Every arithmetic check prints `PARITY conv1 row what err yard ratio of_bound`; profiles/conv1_parity.txt keeps one run's lines."""
import math

import pytest
import torch

from tests import conv1_cases as K

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


class Guarded:
    """an output or workspace of exactly `shape`, prefilled (NaN; int16 planes: 0xffff, a NaN in fp16 and bf16) with 64 guard words behind it"""

    def __init__(self, shape, dtype=torch.float32, fill=K.NAN):
        n = math.prod(shape)
        g = K.GUARD * 4 // torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.full((n + g,), fill, dtype=dtype, device=DEV)
        self.pattern = torch.arange(1, g + 1, device=DEV).to(dtype)
        self.buf[n:] = self.pattern
        self.t = self.buf[:n].view(shape)
        _ALIVE.append(self)

    def cpu(self, what):
        torch.cuda.synchronize()
        assert torch.equal(self.buf[self.t.numel():], self.pattern), f"{what}: the launch wrote behind its output"
        return self.t.cpu()


class HipBackend:
    """one launch of the library on CPU tensors (tests/conv1_cases.py)"""

    def __init__(self, hip):
        self.hip = hip

    def fwd(self, r, x, w, bias, ep=None, absmax=None, stats=False, write_y=True):
        hip, p = self.hip, self.hip.ptr
        y = Guarded((r.N, r.H, r.W, r.cout))
        G = r.groups if stats else 1
        part = None
        if stats:
            rows = hip.query("rpnet_conv1_stats_blocks", r.N, r.H, r.W, r.cout, G)
            assert rows == K.stats_blocks(r.N, r.H, r.W, G), (r.id, rows)
            part = Guarded((G, rows, r.cout, 2), torch.float64)
        am = None if absmax is None else dv(torch.tensor([absmax], dtype=torch.float32))
        sc, sh = (None, None) if ep is None else (dv(ep[0]), dv(ep[1]))
        hip.call("rpnet_conv1_fwd", p(dv(x)), p(dv(w)), p(dv(bias)), p(y.t) if write_y else None, p(sc), p(sh), r.N, r.H, r.W, r.cout, p(am),
                 None if part is None else p(part.t), G)
        yc = y.cpu(r.id + " y")
        return K.Out(y=yc if write_y else None, absmax=None if am is None else am.cpu()[0], part=None if part is None else part.cpu(r.id + " stats_partial"))

    def _bn_relu_outputs(self, r, planes):
        return Guarded((r.N, r.H, r.W, r.cout)), Guarded((planes, r.N, r.H, r.W, r.cout), torch.int16, -1), dv(torch.full((1,), K.NAN))

    def _bn_relu_result(self, r, z, zs, s, planes):
        return K.Out(z=z.cpu(r.id + " z"), planes=zs.cpu(r.id + " z_split"), scale=s.cpu()[0] if planes <= 2 else None)

    def conv1_bn_relu(self, r, x, w, bias, scale, shift, planes, want_z, gamma, beta):
        hip, p = self.hip, self.hip.ptr
        z, zs, s = self._bn_relu_outputs(r, planes)
        hip.call("rpnet_conv1_bn_relu", p(dv(x)), p(dv(w)), p(dv(bias)), p(dv(scale)), p(dv(shift)), p(z.t) if want_z else None, p(zs.t), planes,
                 p(dv(gamma)), p(dv(beta)), p(s) if planes <= 2 else None, r.N, r.H, r.W, r.cout, r.groups)
        return self._bn_relu_result(r, z, zs, s, planes)

    def bn_relu(self, r, y, scale, shift, planes, want_z, gamma, beta):
        hip, p = self.hip, self.hip.ptr
        z, zs, s = self._bn_relu_outputs(r, planes)
        hip.call("rpnet_bn_relu", p(dv(y)), p(dv(scale)), p(dv(shift)), p(z.t) if want_z else None, p(zs.t), planes, p(dv(gamma)), p(dv(beta)),
                 p(s) if planes <= 2 else None, r.N, r.H * r.W, r.cout, r.groups, 0, None, 0)
        return self._bn_relu_result(r, z, zs, s, planes)

    def bwd_partial(self, r, x, w, bias, dz, stats):
        hip, p = self.hip, self.hip.ptr
        rows = hip.query("rpnet_conv1_bn_bwd_rows", r.N, r.H, r.W, r.cout, r.groups)
        assert rows == K.stats_blocks(r.N, r.H, r.W, r.groups), (r.id, rows)
        part = Guarded((r.groups, rows, r.cout, 2), torch.float64)
        hip.call("rpnet_conv1_bn_bwd_partial", p(dv(x)), p(dv(w)), p(dv(bias)), p(dv(dz)), p(dv(stats)), p(part.t), r.N, r.H, r.W, r.cout, r.groups)
        return part.cpu(r.id + " partial")

    def bn_bwd_given(self, r, dz, stats, part):
        hip, p = self.hip, self.hip.ptr
        G, C = r.groups, r.cout
        wsb, off = hip.query("rpnet_bn_workspace_bytes", C, G), hip.query("rpnet_bn_bwd_coef_offset", C, G)
        assert wsb % 4 == 0 and off % 4 == 0 and off + G * C * 2 * 4 <= wsb
        ws, dg, db, st = Guarded((wsb // 4,)), Guarded((C,)), Guarded((C,)), dv(stats)
        hip.call("rpnet_bn_bwd", p(dv(dz)), None, None, p(st[0]), p(st[1]), p(st[2]), p(st[3]), None, None, 0, None, p(dg.t), p(db.t), r.N, r.H * r.W, C, G,
                 0, p(dv(part)), None, part.shape[1], 0, p(ws.t), wsb, None, 0)
        coef = ws.cpu(r.id + " rpnet_bn_bwd workspace")[off // 4:off // 4 + G * C * 2].reshape(G, C, 2)
        return K.Out(dgamma=dg.cpu(r.id + " dgamma"), dbeta=db.cpu(r.id + " dbeta"), coef=coef)

    def wgrad_bn(self, r, x, dz, y, stats, coef, w, bias):
        hip, p = self.hip, self.hip.ptr
        wb = hip.query("rpnet_conv1_wgrad_workspace_bytes", r.N, r.H, r.W, r.cout)
        assert wb == K.WGRAD_BLOCKS * r.cout * 9 * 4, (r.id, wb)
        ws, dw = Guarded((wb // 4,)), Guarded((r.cout, 1, 3, 3))
        again = (None, None) if y is not None else (p(dv(w)), p(dv(bias)))         # the filter only where y is made again
        hip.call("rpnet_conv1_wgrad_bn", p(dv(x)), p(dv(dz)), p(dv(y)), p(dv(stats)), p(dv(coef)), p(dw.t), r.N, r.H, r.W, r.cout, r.groups, p(ws.t), wb, *again)
        ws.cpu(r.id + " workspace")
        return dw.cpu(r.id + " dw")

    def dgrad_bn(self, r, dz, y, stats, coef, w, bias, x):
        hip, p = self.hip, self.hip.ptr
        dx = Guarded((r.N, r.H, r.W))
        hip.call("rpnet_conv1_dgrad_bn", p(dv(dz)), p(dv(y)), p(dv(stats)), p(dv(coef)), p(dv(w)), p(dv(bias)), p(dv(x)), p(dx.t), r.N, r.H, r.W, r.cout, r.groups)
        return dx.cpu(r.id + " dx")


@pytest.fixture(scope="module")
def be(hip):
    return HipBackend(hip)


def ident(r):
    return r.id


@pytest.mark.parametrize("r", K.FWD, ids=ident)
def test_forward(be, r):
    """rpnet_conv1_fwd: plain with and without bias, ep_scale / ep_shift, out_absmax, stats_partial ([groups * rpnet_conv1_stats_blocks]
    rows) with y written and y == NULL"""
    K.hold(K.check_row(be, r))


@pytest.mark.parametrize("r", K.BN_RELU, ids=ident)
def test_bn_relu_made_again_from_the_image(be, r):
    """rpnet_conv1_bn_relu on planes 3, 2, 1, z given and NULL: bit for bit rpnet_bn_relu on the y of rpnet_conv1_fwd"""
    K.hold(K.check_row(be, r))


@pytest.mark.parametrize("r", K.BWD_PARTIAL, ids=ident)
def test_bn_backward_reduction_made_again_from_the_image(be, r):
    """rpnet_conv1_bn_bwd_partial ([groups * rpnet_conv1_bn_bwd_rows] rows), then rpnet_bn_bwd(y = NULL, dy = dy_split = NULL,
    given_partial, given_rows) inside rpnet_bn_workspace_bytes: dgamma, dbeta and the coefficients at rpnet_bn_bwd_coef_offset"""
    K.hold(K.check_row(be, r))


@pytest.mark.parametrize("r", K.WGRAD_BN, ids=ident)
def test_weight_gradient_from_the_bn_output_gradient(be, r):
    """rpnet_conv1_wgrad_bn inside rpnet_conv1_wgrad_workspace_bytes, y given and y == NULL"""
    K.hold(K.check_row(be, r))


@pytest.mark.parametrize("r", K.DGRAD_BN, ids=ident)
def test_input_gradient_from_the_bn_output_gradient(be, r):
    """rpnet_conv1_dgrad_bn, y given and y == NULL, coef given and NULL"""
    K.hold(K.check_row(be, r))


@pytest.mark.parametrize("nhw", K.IMPULSE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_impulses(be, nhw):
    """rpnet_conv1_fwd on one power of two in x: exact, on strips with the edge loads off (W = 4) and on (W = 8) and per pixel"""
    K.hold(K.check_impulses(be, nhw))


def test_input_gradient_impulses(be):
    """rpnet_conv1_dgrad_bn on one power of two in dz at the corners of a 16 x 16 tile: exact"""
    K.hold(K.check_dgrad_impulses(be))


@pytest.mark.parametrize("r", K.CAPS, ids=ident)
def test_block_caps(be, r):
    """the 2048-row cap of the fused statistics of rpnet_conv1_fwd, the 1024-block cap of rpnet_conv1_wgrad_bn, the 16384-block
    grid-stride wrap of the plain rpnet_conv1_fwd"""
    K.hold(K.check_cap(be, r))


def refusal_args(hip, entry, ch, buf):
    """the argument list of one refused call: REFUSAL_BASE with the row's changes, every pointer the one small buffer or NULL"""
    v = dict(K.REFUSAL_BASE)
    v.update({k: x for k, x in ch.items() if k in ("N", "H", "W", "cout", "groups", "planes")})
    v.setdefault("H", 4)
    null = set(ch.get("null", "").split(","))
    q = lambda name: None if name in null else hip.ptr(buf)         # noqa: E731
    N, H, W, C, G = v["N"], v["H"], v["W"], v["cout"], v["groups"]
    if entry == "rpnet_conv1_fwd":
        ep = hip.ptr(buf) if ch.get("ep") else None
        return [q("x"), q("w"), q("bias"), q("y"), ep, ep, N, H, W, C, q("out_absmax"), q("stats_partial"), G]
    if entry == "rpnet_conv1_wgrad_bn":
        wb = hip.query("rpnet_conv1_wgrad_workspace_bytes", 4, 4, 8, 64) - 1 if ch.get("ws_short") else buf.numel() * 4
        return [q("x"), q("dz"), q("y"), q("stats"), q("coef"), q("dw"), N, H, W, C, G, q("workspace"), wb, q("w"), q("bias")]
    if entry == "rpnet_conv1_bn_relu":
        return [q("x"), q("w"), q("bias"), q("scale"), q("shift"), q("z"), q("z_split"), v["planes"], q("gamma"), q("beta"), q("split_scale"), N, H, W, C, G]
    if entry == "rpnet_conv1_bn_bwd_partial":
        return [q("x"), q("w"), q("bias"), q("dz"), q("stats"), q("partial"), N, H, W, C, G]
    assert entry == "rpnet_conv1_dgrad_bn"
    return [q("dz"), q("y"), q("stats"), q("coef"), q("w"), q("bias"), q("x"), q("dx"), N, H, W, C, G]


def test_refusals(hip):
    """every RPNET_REQUIRE of rpnet_conv1_fwd, rpnet_conv1_wgrad_bn, rpnet_conv1_bn_relu, rpnet_conv1_bn_bwd_partial and
    rpnet_conv1_dgrad_bn refuses on the host, before any launch: the status code, the head of rpnet_last_error_string, and the
    buffers untouched"""
    lib = hip.load()
    buf = dv(torch.full((1 << 20,), 7.0))
    for label, entry, ch, want, head in K.REFUSALS:
        got = getattr(lib, entry)(*refusal_args(hip, entry, ch, buf), hip.stream())
        msg = lib.rpnet_last_error_string().decode()
        assert got == want, f"{entry} ({label}): rc {got}, expected {want}: {msg}"
        assert msg.startswith(head), f"{entry} ({label}): the message does not start with {head!r}: {msg!r}"
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())               # nothing ran
