"""GPU parity of the operand splitters and weight packers (csrc/conv_split.hip, csrc/split_bf16.h, csrc/conv_wgrad.hip,
csrc/conv_up4_dma.hip) against the bit-exact references of tests/operand_cases.py.  Every call goes through the C ABI
(rpnet_amd.hip.call / ptr); every output is prefilled with a NaN pattern (or, where the contract leaves elements to the caller, with
what the header tells the caller to put there), is exactly as long as its layout says, has 64 guard words behind it and is written a
second time by an identical call, bit for bit.  The tables, the references and every comparison live in tests/operand_cases.py, shared
with tests/test_host_operands.py (which runs them on a CPU restatement of the kernels' index arithmetic and shows that seeded defects
fail).  No written bit has a tolerance.  The module prints `OPERANDS family elements=... worst_reconstruction_of_bound=...` when it
ends; profiles/operands_parity.txt keeps one run's lines."""
import ctypes

import pytest
import torch

from tests import operand_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    from rpnet_amd import hip
    hip.load()
    yield hip
    print()
    for line in K.tally_lines():
        print(line)


_ALIVE = []


@pytest.fixture(autouse=True)
def _device_copies_live_until_the_test_ends():
    yield
    _ALIVE.clear()


def dv(t, offset=0):
    """device copy inside an allocation of its own that is 32 bytes longer (never a NULL pointer, even for no elements), `offset`
    elements in; referenced until the test ends"""
    if t is None:
        return None
    big = torch.zeros(t.numel() + 32 // t.element_size(), dtype=t.dtype, device=DEV)
    view = big[offset:offset + t.numel()].view(t.shape)
    view.copy_(t)
    _ALIVE.append(big)
    return view


class Guarded:
    """an output of exactly the shape of `prefill`, holding it, with 64 guard words behind it and `front` ELEMENTS in front"""

    def __init__(self, prefill, front=0):
        n, g = prefill.numel(), K.GUARD * 4 // prefill.element_size()
        self.buf = torch.empty(front + n + g, dtype=prefill.dtype, device=DEV)
        self.pattern = (torch.arange(front + g, device=DEV) % 97 + 1).to(prefill.dtype)
        self.buf[:front], self.buf[front + n:] = self.pattern[:front], self.pattern[front:]
        self.t = self.buf[front:front + n].view(prefill.shape)
        self.t.copy_(prefill)
        self.front = front
        _ALIVE.append(self)

    def cpu(self, what):
        torch.cuda.synchronize()
        around = torch.cat([self.buf[:self.front], self.buf[self.front + self.t.numel():]])
        assert torch.equal(around.view(torch.uint8), self.pattern.view(torch.uint8)), f"{what}: the launch wrote outside its output"
        return self.t.cpu()


def nan_planes(planes, rows, C):
    return torch.full((planes, rows, C), K.NAN16[planes], dtype=torch.int16)


class HipBackend:
    """one launch of the library on CPU tensors (tests/operand_cases.py)"""

    def __init__(self, hip):
        self.hip = hip

    def p(self, t):
        """hip.ptr; for a tensor of no elements (rows = 0, n = 0), whose data_ptr() is NULL, the address where its elements would start"""
        if t is None or t.numel():
            return self.hip.ptr(t)
        return t.untyped_storage().data_ptr() + t.storage_offset() * t.element_size()

    def split_bf16(self, x, mask, mode, offset):
        hip, p = self.hip, self.p
        rows, C = x.shape
        out = Guarded(nan_planes(3, rows, C), front=8 if offset else 0)              # 8 int16 / 4 floats: 16 bytes
        hip.call("rpnet_split_bf16", p(dv(x, 4 if offset else 0)), p(dv(mask)), mode, p(out.t), rows, C, 3)
        return out.cpu("split_bf16 out")

    def split_f16(self, x, mask, mode, s_a, s_b, planes, a_is_bound, s_out, offset):
        hip, p = self.hip, self.p
        rows, C = x.shape
        out = Guarded(nan_planes(planes, rows, C), front=8 if offset else 0)
        so = Guarded(torch.full((1,), K.NAN)) if s_out else None
        hip.call("rpnet_split_f16", p(dv(x, 4 if offset else 0)), p(dv(mask)), mode, p(dv(s_a)), p(dv(s_b)), p(so.t) if s_out else None, p(out.t),
                 rows, C, planes, a_is_bound)
        return out.cpu("split_f16 out"), (so.cpu("s_out")[0] if s_out else None)

    def pow2_scale(self, b):
        s = Guarded(torch.full((1,), K.NAN))
        self.hip.call("rpnet_pow2_scale", self.hip.ptr(dv(b)), self.hip.ptr(s.t))
        return s.cpu("pow2_scale s_out")

    def predict_scales(self, m, bound, n, safety, check, viol):
        hip, p = self.hip, self.p
        b, s = Guarded(bound), Guarded(torch.full((n,), K.NAN))
        v = Guarded(torch.tensor([viol], dtype=torch.int32)) if viol is not None else None
        hip.call("rpnet_predict_scales", p(dv(m)), p(b.t), p(s.t), n, safety, check, p(v.t) if v is not None else None)
        return b.cpu("bound"), s.cpu("scale"), (int(v.cpu("violations")[0]) if v is not None else None)

    def pack_split(self, calls, planes, single):
        hip, p = self.hip, self.p
        outs = [[Guarded(t) if t is not None else None for t in (c.wp0, c.wd0, c.t0, c.u0)] for c in calls]
        q = lambda g: p(g.t) if g is not None else None         # noqa: E731
        ws = [dv(c.w) for c in calls]
        if single:
            (c,), (o,) = calls, outs
            it = c.it
            hip.call("rpnet_pack_conv_weight_split", p(ws[0]), q(o[0]), q(o[1]), it.cout, it.cin, it.taps, it.off0, it.split, it.off1, it.cin_pad, planes,
                     q(o[2]), q(o[3]))
        else:
            items = (hip.PackItem * len(calls))()
            for k, (c, o) in enumerate(zip(calls, outs)):
                it = c.it
                items[k] = hip.PackItem(p(ws[k]), q(o[0]), q(o[1]), q(o[2]), q(o[3]), it.cout, it.cin, it.taps, it.off0, it.split, it.off1, it.cin_pad)
            hip.call("rpnet_pack_conv_weights_split", items, len(calls), planes)
        return [K.Packed(*[g.cpu(f"{c.it.id} {n}") if g is not None else None for g, n in zip(o, ("wp", "wd", "row_scale_wp", "row_scale_wd"))])
                for c, o in zip(calls, outs)]

    def pack_f32(self, it, w, wp0, wd0):
        hip, p = self.hip, self.p
        wp, wd = Guarded(wp0), (Guarded(wd0) if wd0 is not None else None)
        hip.call("rpnet_pack_conv_weight", p(dv(w)), p(wp.t), p(wd.t) if wd is not None else None, it.cout, it.cin, it.taps, it.off0, it.split, it.off1,
                 it.cin_pad)
        return wp.cpu(it.id + " wp"), (wd.cpu(it.id + " wd") if wd is not None else None)

    def collapse(self, w):
        cout, cin = w.shape[:2]
        wc = Guarded(torch.full((4 * cout, cin, 2, 2), K.NAN))
        self.hip.call("rpnet_upconv_collapse_weights", self.hip.ptr(dv(w)), self.hip.ptr(wc.t), cout, cin)
        return wc.cpu("wc")


@pytest.fixture(scope="module")
def be(hip):
    return HipBackend(hip)


def ident(v):
    return getattr(v, "id", str(v))


@pytest.mark.parametrize("bound", K.POW2_BOUNDS, ids=repr)
def test_pow2_scale(be, bound):
    """rpnet_pow2_scale at zero, negative, NaN, +inf, the smallest subnormal, both clamps and 2^k, 2^k +- 1 ulp"""
    K.hold(K.check_pow2(be, bound))


@pytest.mark.parametrize("n,safety,check", K.PREDICT_ROWS)
def test_predict_scales(be, n, safety, check):
    """rpnet_predict_scales: bound, scale and the violation count (a NaN measurement counts) exactly, n around the block edge"""
    K.hold(K.check_predict(be, n, safety, check))


@pytest.mark.parametrize("r", K.SPLIT_ROWS, ids=ident)
def test_split(be, r):
    """rpnet_split_bf16 / rpnet_split_f16 against corr_cases.split_planes on the reference product, every mode, plane count and scale form"""
    K.hold(K.check_split(be, r))


@pytest.mark.parametrize("it,planes", K.PACK_ROWS, ids=ident)
def test_pack_split(be, it, planes):
    """rpnet_pack_conv_weight_split: wp, wd, both row scales and the padding of both walks against the header's layouts"""
    K.hold(K.check_pack(be, it, planes))


@pytest.mark.parametrize("it,planes,kind", K.IMPULSE_ROWS, ids=ident)
def test_pack_impulses(be, it, planes, kind):
    """rpnet_pack_conv_weight_split on one non-zero weight: one position of wp, one of wd, the tap flipped"""
    K.hold(K.check_impulse(be, it, planes, kind))


@pytest.mark.parametrize("order,planes", K.MULTI_ROWS)
def test_pack_many_layers(be, order, planes):
    """rpnet_pack_conv_weights_split with 1, 2 and 24 items: each item bit for bit its rpnet_pack_conv_weight_split call"""
    K.hold(K.check_multi(be, order, planes))


@pytest.mark.parametrize("it", K.F32_ITEMS, ids=ident)
def test_pack_f32(be, it):
    """rpnet_pack_conv_weight: exact copies into wp [taps][cin_pad/4][cout][4] and wd [taps flipped][cout/4][cin_pad][4]"""
    K.hold(K.check_pack_f32(be, it))


@pytest.mark.parametrize("cout,cin", K.COLLAPSE_SHAPES)
def test_collapse(be, cout, cin):
    """rpnet_upconv_collapse_weights: the 0 / 1 pattern of the phase sets, the float64 sums, exact on small integers"""
    K.hold(K.check_collapse(be, cout, cin))


@pytest.mark.parametrize("planes", (2, 1))
def test_collapse_then_pack(be, planes):
    """rpnet_upconv_collapse_weights, then rpnet_pack_conv_weight_split(taps = 4): the reference pack of the reference collapse"""
    K.hold(K.check_collapse_then_pack(be, planes))


def refusal_args(hip, entry, args, buf):
    if entry == "rpnet_pack_conv_weights_split":
        dicts, n, planes = args
        if dicts is None:
            return [None, n, planes]
        items = (hip.PackItem * len(dicts))()
        for k, d in enumerate(dicts):
            items[k] = hip.PackItem(**{f: (hip.ptr(buf) if v == "P" else v) for f, v in d.items()})
        return [items, n, planes]
    return [hip.ptr(buf) if isinstance(a, str) else a for a in args]


def test_refusals(hip):
    """every RPNET_REQUIRE of rpnet_split_bf16, rpnet_split_f16, rpnet_pow2_scale, rpnet_predict_scales, rpnet_pack_conv_weight_split,
    rpnet_pack_conv_weights_split, rpnet_pack_conv_weight and rpnet_upconv_collapse_weights refuses on the host, before any launch:
    the status code, the head of rpnet_last_error_string, and the buffer untouched"""
    lib = hip.load()
    buf = dv(torch.full((1 << 20,), 7.0))
    for label, entry, args, want, head in K.REFUSALS:
        got = getattr(lib, entry)(*refusal_args(hip, entry, args, buf), hip.stream())
        msg = lib.rpnet_last_error_string().decode()
        assert got == want, f"{entry} ({label}): rc {got}, expected {want}: {msg}"
        assert msg.startswith(head), f"{entry} ({label}): the message does not start with {head!r}: {msg!r}"
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())               # nothing ran
    assert ctypes.sizeof(hip.PackItem) == 5 * 8 + 7 * 4 + 4
