"""GPU parity of the BatchNorm kernels (csrc/bn.hip: rpnet_bn_stats, rpnet_bn_stats_from_partial, rpnet_bn_eval_affine, rpnet_bn_relu,
rpnet_bn_bwd, rpnet_bn_eval_relu, rpnet_bn_eval_bwd) against the float64 references of tests/ref64.py, at every launch of their
default dispatch.  Every call goes through rpnet_amd.hip.call; outputs and the workspace are prefilled with NaN, the workspace is
exactly as long as rpnet_bn_workspace_bytes says, with 64 guard words behind it, and the coefficients are read where
rpnet_bn_bwd_coef_offset says.  The tables, the bounds and every comparison live in tests/bn_cases.py (shared with
tests/test_host_bn_ref64.py, which shows on the CPU that the bounds have room for a correct fp32 implementation and that seeded defects
fail them).  Every arithmetic check prints `PARITY bn case what err yard ratio of_bound`; profiles/bn_parity.txt keeps one run's
lines."""
import types

import pytest
import torch

from tests import bn_cases as BC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32


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


def nans(*shape, dtype=F32):
    return dv(torch.full(shape, BC.NAN, dtype=dtype))


def cpu(t):
    return None if t is None else t.cpu()


class HipBackend:
    """one entry point of the library on CPU tensors (tests/bn_cases.py)"""

    def __init__(self, hip):
        self.hip = hip

    def workspace(self, c):
        wb = self.hip.query("rpnet_bn_workspace_bytes", c.C, c.G)
        off = self.hip.query("rpnet_bn_bwd_coef_offset", c.C, c.G)
        assert wb == BC.workspace_bytes(c) and off == BC.coef_offset(c) and wb % 4 == 0 and off % 4 == 0, (c.id, wb, off)
        words = wb // 4
        ws = nans(words + BC.GUARD)
        guard = torch.arange(1, BC.GUARD + 1, dtype=F32, device=DEV)
        ws[words:] = guard
        return ws, wb, (lambda: bool(torch.equal(ws[words:], guard))), (lambda: ws[off // 4:off // 4 + c.G * c.C * 2].reshape(c.G, c.C, 2).cpu())

    def stats(self, c, d, rm0, rv0, nbt0, partial=None):
        hip, p = self.hip, self.hip.ptr
        G, C = c.G, c.C
        out = [nans(G, C) for _ in range(4)]
        rm, rv = dv(None if rm0 is None else rm0.clone()), dv(None if rv0 is None else rv0.clone())
        nbt = None if nbt0 is None else dv(torch.tensor([nbt0], dtype=torch.int64))
        gamma, beta = dv(d.gamma), dv(d.beta)
        ok = lambda: True           # noqa: E731
        if partial is None:
            ws, wb, ok, _ = self.workspace(c)
            hip.call("rpnet_bn_stats", p(dv(d.y)), c.N, c.HW, C, G, p(gamma), p(beta), p(rm), p(rv), p(nbt), BC.MOM, BC.EPS,
                     *[p(t) for t in out], p(ws), wb)
        else:
            hip.call("rpnet_bn_stats_from_partial", p(dv(partial)), c.nblk, c.N, c.HW, C, G, p(gamma), p(beta), p(rm), p(rv), p(nbt),
                     BC.MOM, BC.EPS, *[p(t) for t in out])
        torch.cuda.synchronize()
        return types.SimpleNamespace(scale=cpu(out[0]), shift=cpu(out[1]), mean=cpu(out[2]), invstd=cpu(out[3]), running_mean=cpu(rm),
                                     running_var=cpu(rv), nbt=None if nbt is None else int(nbt.item()), guard_ok=ok())

    def relu(self, c, d, st):
        hip, p = self.hip, self.hip.ptr
        shape = (c.N, c.H // 2, c.W // 2, c.C) if c.pool else (c.N, c.H, c.W, c.C)
        z = nans(*shape) if c.fp32 else None
        bits = nans(c.planes, *shape, dtype=torch.float16).view(torch.int16) if c.planes else None
        s = nans(1) if (c.f16 or c.want_scale) else None
        std = dv(st)
        needs = s is not None
        hip.call("rpnet_bn_relu", p(dv(d.y)), p(std[0]), p(std[1]), p(z), p(bits), c.planes, p(dv(d.gamma)) if needs else None,
                 p(dv(d.beta)) if needs else None, p(s), c.N, c.HW, c.C, c.G, c.W if c.pool else 0, None, 0)
        torch.cuda.synchronize()
        return types.SimpleNamespace(z=cpu(z), bits=cpu(bits), s=None if s is None else float(s.item()))

    def bwd(self, c, d, st, pre_g, pre_b, accumulate, given=None):
        hip, p = self.hip, self.hip.ptr
        shape = (c.N, c.H, c.W, c.C)
        want_dy = not c.red
        dy = nans(*shape) if (c.fp32 and want_dy) else None
        bits = nans(c.planes, *shape, dtype=torch.float16).view(torch.int16) if c.planes else None
        s = nans(1) if c.f16 else None
        dg = dv(torch.full((c.C,), BC.NAN) if pre_g is None else pre_g.clone())
        db = dv(torch.full((c.C,), BC.NAN) if pre_b is None else pre_b.clone())
        ws, wb, ok, coef = self.workspace(c)
        std = dv(st)
        y = None if c.no_y else dv(d.y)
        if c.op == "eval_bwd":
            hip.call("rpnet_bn_eval_bwd", p(dv(d.dz)), p(y), p(std[0]), p(std[1]), p(std[2]), p(std[3]), p(dy), p(bits), c.planes, p(s),
                     p(dg), p(db), c.N, c.HW, c.C, c.G, accumulate, p(ws), wb)
        else:
            gp, gm = (None, None) if given is None else (dv(given[0]), dv(given[1]))
            hip.call("rpnet_bn_bwd", p(dv(d.dz)), p(y), p(dv(d.gamma)), p(std[0]), p(std[1]), p(std[2]), p(std[3]), p(dy), p(bits), c.planes,
                     p(s), p(dg), p(db), c.N, c.HW, c.C, c.G, accumulate, p(gp), p(gm), c.given, c.W if c.pool else 0, p(ws), wb, None, 0)
        torch.cuda.synchronize()
        return types.SimpleNamespace(dy=cpu(dy), bits=cpu(bits), s=None if s is None else float(s.item()), dgamma=cpu(dg), dbeta=cpu(db),
                                     coef=coef(), guard_ok=ok())

    def eval_affine(self, c, gamma, beta, rm, rv):
        p = self.hip.ptr
        sc, sh = nans(c.C), nans(c.C)
        self.hip.call("rpnet_bn_eval_affine", p(dv(gamma)), p(dv(beta)), p(dv(rm)), p(dv(rv)), BC.EPS, p(sc), p(sh), c.C)
        torch.cuda.synchronize()
        return sc.cpu(), sh.cpu()

    def eval_relu(self, c, y2, scale, shift, absmax0):
        p = self.hip.ptr
        z, top = nans(*y2.shape), dv(torch.tensor([absmax0], dtype=F32))
        self.hip.call("rpnet_bn_eval_relu", p(dv(y2)), p(dv(scale)), p(dv(shift)), p(z), p(top), y2.shape[0], c.C)
        torch.cuda.synchronize()
        return types.SimpleNamespace(z=z.cpu(), absmax=top.cpu()[0])


@pytest.fixture(scope="module")
def be(hip):
    return HipBackend(hip)


def ident(c):
    return c.id


def row(be, c):
    assert BC.route(c) == c.kernel, (c.id, BC.route(c), c.kernel)
    print()                                     # the records start on a line of their own behind the test's name
    BC.hold(BC.check_row(be, c))


@pytest.mark.parametrize("c", BC.STATS, ids=ident)
def test_stats(be, c):
    """rpnet_bn_stats: bn_stats_partial<64> + bn_stats_finalize inside rpnet_bn_workspace_bytes"""
    row(be, c)


@pytest.mark.parametrize("c", BC.FROM_PARTIAL, ids=ident)
def test_stats_from_partial(be, c):
    """rpnet_bn_stats_from_partial on float64 partial sums of the host, with a row count bn_geom would not have chosen"""
    row(be, c)


@pytest.mark.parametrize("c", BC.RELU, ids=ident)
def test_relu(be, c):
    """rpnet_bn_relu: bn_relu_kernel and bn_relu_split_kernel<1 | 2 | 3>, with and without the fp32 output"""
    row(be, c)


@pytest.mark.parametrize("c", BC.RELU_POOL, ids=ident)
def test_relu_pooled(be, c):
    """rpnet_bn_relu(pool_w): bn_relu_pool_split_kernel<1 | 2 | 3>"""
    row(be, c)


@pytest.mark.parametrize("c", BC.BWD, ids=ident)
def test_bwd(be, c):
    """rpnet_bn_bwd: bn_bwd_partial<64> + bn_bwd_finalize + bn_bwd_apply | bn_bwd_apply_split<1 | 2 | 3>, and the reduction alone"""
    row(be, c)


@pytest.mark.parametrize("c", BC.BWD_POOL, ids=ident)
def test_bwd_pooled(be, c):
    """rpnet_bn_bwd(pool_w): bn_bwd_partial_pool<64> + bn_bwd_finalize + bn_bwd_apply_pool_split<1 | 2 | 3>"""
    row(be, c)


@pytest.mark.parametrize("c", BC.GIVEN, ids=ident)
def test_bwd_given_partial(be, c):
    """rpnet_bn_bwd on given_partial / given_pmax / given_rows, y = NULL where nothing reads it"""
    row(be, c)


@pytest.mark.parametrize("c", BC.EVAL_AFFINE, ids=ident)
def test_eval_affine(be, c):
    row(be, c)


@pytest.mark.parametrize("c", BC.EVAL_RELU, ids=ident)
def test_eval_relu(be, c):
    row(be, c)


@pytest.mark.parametrize("c", BC.EVAL_BWD, ids=ident)
def test_eval_bwd(be, c):
    """rpnet_bn_eval_bwd: bn_bwd_partial<64> + bn_eval_bwd_finalize + the train-mode apply passes on zero coefficients"""
    row(be, c)


def test_refusals(hip):
    """every refusal happens on the host, before any launch: the status code, the entry point's name at the head of
    rpnet_last_error_string, and the outputs and the workspace untouched"""
    lib, p = hip.load(), hip.ptr
    n = 1 << 20                                                     # 4 MB each: no accepted shape is passed, only sizes
    names = ("y", "dz", "z", "dy", "split", "s", "gamma", "beta", "scale", "shift", "mean", "invstd", "rm", "rv", "dgamma", "dbeta",
             "ws", "partial", "pmax")
    buf = {k: dv(torch.full((n,), 7.0)) for k in names}
    for label, entry, ch, want in BC.REFUSALS:
        g = dict(N=4, HW=16, C=8, G=2, planes=0, pool_w=0, rows=0, nblk=1)
        g.update({k: v for k, v in ch.items() if k in g})
        null = set(ch.get("null", "").split(","))
        b = {k: (None if k in null else p(t)) for k, t in buf.items()}
        split = b["split"] if ch.get("split") else None
        given = b["partial"] if ch.get("given") else None
        wb = n * 4 if "ws_short" not in ch else hip.query("rpnet_bn_workspace_bytes", g["C"], g["G"]) - 1
        y_dec = b["y"] if ch.get("y_dec") else None
        st = hip.stream()
        if entry == "rpnet_bn_stats":
            got = lib.rpnet_bn_stats(b["y"], g["N"], g["HW"], g["C"], g["G"], b["gamma"], b["beta"], b["rm"], b["rv"], None, BC.MOM, BC.EPS,
                                     b["scale"], b["shift"], b["mean"], b["invstd"], b["ws"], wb, st)
        elif entry == "rpnet_bn_stats_from_partial":
            got = lib.rpnet_bn_stats_from_partial(b["partial"], g["nblk"], g["N"], g["HW"], g["C"], g["G"], b["gamma"], b["beta"], b["rm"], b["rv"],
                                                  None, BC.MOM, BC.EPS, b["scale"], b["shift"], b["mean"], b["invstd"], st)
        elif entry == "rpnet_bn_eval_affine":
            got = lib.rpnet_bn_eval_affine(b["gamma"], b["beta"], b["rm"], b["rv"], BC.EPS, b["scale"], b["shift"], g["C"], st)
        elif entry == "rpnet_bn_relu":
            got = lib.rpnet_bn_relu(b["y"], b["scale"], b["shift"], b["z"], split, g["planes"], b["gamma"], b["beta"], b["s"], g["N"], g["HW"],
                                    g["C"], g["G"], g["pool_w"], y_dec, 0, st)
        elif entry == "rpnet_bn_bwd":
            got = lib.rpnet_bn_bwd(b["dz"], b["y"], b["gamma"], b["scale"], b["shift"], b["mean"], b["invstd"], b["dy"], split, g["planes"],
                                   b["s"], b["dgamma"], b["dbeta"], g["N"], g["HW"], g["C"], g["G"], 0, given, b["pmax"] if given else None,
                                   g["rows"], g["pool_w"], b["ws"], wb, y_dec, 0, st)
        elif entry == "rpnet_bn_eval_relu":
            got = lib.rpnet_bn_eval_relu(b["y"], b["scale"], b["shift"], b["z"], b["s"], g["N"] * g["HW"], g["C"], st)
        else:
            got = lib.rpnet_bn_eval_bwd(b["dz"], b["y"], b["scale"], b["shift"], b["mean"], b["invstd"], b["dy"], split, g["planes"], b["s"],
                                        b["dgamma"], b["dbeta"], g["N"], g["HW"], g["C"], g["G"], 0, b["ws"], wb, st)
        msg = lib.rpnet_last_error_string().decode()
        assert got == want, f"{entry} ({label}): rc {got}, expected {want}: {msg}"
        assert msg.startswith(entry[len("rpnet_"):] + ":"), f"{entry} ({label}): the message does not start with the entry point: {msg!r}"
    torch.cuda.synchronize()
    for k, t in buf.items():
        assert bool((t == 7.0).all()), f"a refused call wrote to {k}"               # nothing ran
