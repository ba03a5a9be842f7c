"""GPU parity of the convolution forward and input-gradient kernels (rpnet_conv_fwd, rpnet_conv_up4) against the float64 references
tests/ref64.py conv_fwd / conv_dgrad, at every branch of their dispatch and for every feature of the shared epilogue alone.  Every
call goes through rpnet_amd.hip.call / hip.query with a descriptor of RF._desc; y0, y1, y_split and every workspace are prefilled
with NaN (with known finite values under accumulate), the split-K workspace is exactly as long as
rpnet_conv_splitk_workspace_bytes says, and 64 guard words sit behind every output and workspace.  For plane operands the
descriptor's rpnet_conv_tile_variant is asserted to be the row's variant, so a forced variant that fell back fails.  The tables,
the bound and every comparison live in tests/conv_cases.py (shared with tests/test_host_conv_ref64.py, which shows on the CPU that
the bound has room for a correct fp32 implementation and that seeded defects fail it).  Every arithmetic check prints
`PARITY conv case what err yard ratio of_bound`; profiles/conv_parity.txt keeps one run's lines."""
import ctypes as C

import pytest
import torch

from tests import conv_cases as VC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN16 = -1                   # 0xFFFF: a NaN in fp16 and in bf16


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


def guarded(values, words=VC.GUARD):
    """a flat device buffer of `values` with guard words 1, 2, ... behind it -> (buffer, number of payload elements)"""
    v = values.reshape(-1)
    g = torch.arange(1, words + 1).to(v.dtype)
    return dv(torch.cat([v, g])), v.numel()


def guard_ok(buf, n):
    tail = buf[n:].cpu()
    return bool(torch.equal(tail, torch.arange(1, tail.numel() + 1).to(tail.dtype)))


def descriptor(hip, c, L, x0, x1, w, ys, in_scale=None):
    from rpnet_amd import functional as RF
    p = hip.ptr
    d = RF._desc(x0, x1, w, dv(L.bias), in_scale, c.mode, ys[0], ys[1] if len(ys) > 1 else None, c.N, c.H, c.W, 9 if c.fam == "up4" else c.taps,
                 int(bool(c.ups or c.up4)), c.groups, dv(L.ep_scale), dv(L.ep_shift), int(c.has("relu")), dv(L.out_scale), c.os_mode,
                 int(c.has("acc")), co_split=(c.Co0, c.Co1))
    d.C0, d.C1, d.dilation, d.split_planes, d.tune = c.C0, c.C1, c.dil, c.planes, c.tune
    d.acc_scale_col, d.acc_scale_x, d.acc_scale_x1 = p(dv(L.col)), p(scalar(L.sx)), p(scalar(L.sx1))
    return d


class HipBackend:
    """one launch of the library on CPU tensors (tests/conv_cases.py)"""

    def __init__(self, hip):
        self.hip = hip

    def run(self, c, L, arm_skip=True, ws_short=False):
        hip, p = self.hip, self.hip.ptr
        ho, wo = (c.H // 2, c.W // 2) if c.up4 == 2 else (c.H, c.W)
        rows = c.N * ho * wo
        bufs = []                    # (buffer, payload elements) of everything the launch may write
        ys = []
        for i, co in enumerate((c.Co0, c.Co1)):
            if co:
                ys.append(guarded(L.prev[i] if c.has("acc") else torch.full((rows * co,), VC.NAN)))
        bufs += ys
        d = descriptor(hip, c, L, dv(L.x0), dv(L.x1), dv(L.w), [y for y, _ in ys], dv(L.in_scale))
        stats = amax = ysplit = flags = ws = None
        if c.has("stats"):
            nb = hip.query("rpnet_conv_up4_stats_blocks" if c.fam == "up4" else "rpnet_conv_stats_blocks", C.byref(d))
            assert nb == VC.stats_blocks(c) > 0, (c.id, nb, VC.stats_blocks(c))
            stats = guarded(torch.full((c.groups * nb * c.Cout * 2,), VC.NAN, dtype=torch.float64))
            d.stats_partial = p(stats[0])
            bufs.append(stats)
        if c.has("amax"):
            amax = guarded(torch.tensor([float(L.amax0)]))
            d.out_absmax = p(amax[0])
            bufs.append(amax)
        if c.ys_planes:
            ysplit = guarded(torch.full((c.ys_planes * rows * c.Cout,), NAN16, dtype=torch.int16), 2 * VC.GUARD)
            d.y_split, d.split_out_planes, d.y_split_scale = p(ysplit[0]), c.ys_planes, p(scalar(L.ys_scale))
            bufs.append(ysplit)
        if c.skip and arm_skip:
            flags = guarded(torch.full((max(c.M // 128, 16),), 255, dtype=torch.uint8), 4 * VC.GUARD)
            d.skip_mask, d.skip_mode, d.skip_halo, d.skip_ws = p(dv(L.mask)), int(c.skip[4]), int(c.skip[5]), p(flags[0])
            bufs.append(flags)
        if c.splitk:
            wb = hip.query("rpnet_conv_splitk_workspace_bytes", C.byref(d))
            assert wb == VC.splitk_bytes(c) > 0 and wb % 4 == 0, (c.id, wb, VC.splitk_bytes(c))
            ws = guarded(torch.full((wb // 4,), VC.NAN))
            d.splitk_ws, d.splitk_ws_bytes = p(ws[0]), wb - (1 if ws_short else 0)
            bufs.append(ws)
        if c.fam == "planes":
            assert hip.query("rpnet_conv_tile_variant", C.byref(d)) == VC.variant(c), (c.id, hip.query("rpnet_conv_tile_variant", C.byref(d)))
        if c.fam == "up4":
            assert hip.query("rpnet_conv_up4_supported", C.byref(d), c.up4) == 1, c.id
            hip.call("rpnet_conv_up4", C.byref(d), c.up4)
        else:
            hip.call("rpnet_conv_fwd", C.byref(d))
        outs = ys
        if c.up_bwd:
            outs = [guarded(torch.full((rows // 4 * co,), VC.NAN)) for co in (c.Co0, c.Co1) if co]
            for (y, _), (dx, _), co in zip(ys, outs, (c.Co0, c.Co1)):
                hip.call("rpnet_upsample2_bwd", p(y), p(dx), c.N, c.H, c.W, co)
            bufs += outs
            ho, wo = ho // 2, wo // 2
        torch.cuda.synchronize()
        res = [y[:n].cpu().reshape(c.N, ho, wo, -1) for y, n in outs]
        return VC.Out(res,
                      None if stats is None else stats[0][:stats[1]].cpu().reshape(c.groups, -1, c.Cout, 2).sum(1),
                      None if amax is None else amax[0][:1].cpu(),
                      None if ysplit is None else ysplit[0][:ysplit[1]].cpu().reshape(c.ys_planes, rows, c.Cout),
                      None if flags is None else flags[0][:c.M // VC.tile_rows(c)].cpu(),
                      all(guard_ok(b, n) for b, n in bufs),
                      None if ws is None else bool(torch.isnan(ws[0][:ws[1]]).all()))


@pytest.fixture(scope="module")
def be(hip):
    return HipBackend(hip)


def ident(c):
    return c.id


@pytest.mark.parametrize("c", VC.FP32, ids=ident)
def test_fp32_operands(be, c):
    """rpnet_conv_fwd on fp32 operands: conv_igemm_kernel<WM, WN, INSCALE>, 3 x 3, 1 x 1, dilation 2, in_scale, two sources, upsample"""
    VC.hold(VC.check_row(be, c))


@pytest.mark.parametrize("c", VC.PLAIN, ids=ident)
def test_plain_split_kernels(be, c):
    """rpnet_conv_fwd on three, two and one plane, variants 0 - 3 (rpnet_conv_tile_variant asserted), dilation 2, acc_scale_x1"""
    VC.hold(VC.check_row(be, c))


@pytest.mark.parametrize("c", VC.PATCH, ids=ident)
def test_patch_kernels(be, c):
    """rpnet_conv_fwd on image patches (rpnet_conv_tile_variant asserted): variants 7, 8, 9, 11, 12, 13, 14; one patch per image, seams, two images, two sources, upsample,
    two destinations, two channel chunks"""
    VC.hold(VC.check_row(be, c))


@pytest.mark.parametrize("c", VC.SPLITK, ids=ident)
def test_split_k(be, c):
    """splitk_ws exactly as long as rpnet_conv_splitk_workspace_bytes answers, and one byte shorter"""
    VC.hold(VC.check_row(be, c))


@pytest.mark.parametrize("c", VC.EPILOGUE, ids=ident)
def test_epilogue_features(be, c):
    """rpnet_conv_fwd with each feature of csrc/conv_epilogue.h alone and all together, under LinearRows and PatchRows; stats_partial against
    rpnet_conv_stats_blocks rows"""
    VC.hold(VC.check_row(be, c))


@pytest.mark.parametrize("c", VC.SKIP, ids=ident)
def test_skip_mask(be, c):
    VC.hold(VC.check_row(be, c))


@pytest.mark.parametrize("c", VC.DGRAD, ids=ident)
def test_input_gradient(be, c):
    """rpnet_conv_fwd on the `wd` pack with dy as the source, against ref64.conv_dgrad: two destinations, rpnet_upsample2_bwd behind it"""
    VC.hold(VC.check_row(be, c))


@pytest.mark.parametrize("c", VC.CRE_PAIRS, ids=ident)
def test_input_gradient_of_the_two_masked_branches(be, c):
    VC.hold(VC.check_cre_pair(be, c))


@pytest.mark.parametrize("c", VC.UP4, ids=ident)
def test_collapsed_up_conv(be, c):
    """rpnet_conv_up4, modes 1 and 2, statistics in rpnet_conv_up4_stats_blocks rows, and the nine-tap form of rpnet_conv_fwd on the same
    operands"""
    VC.hold(VC.check_row(be, c))


@pytest.mark.parametrize("label,c", VC.UP4_UNSUPPORTED, ids=[r[0] for r in VC.UP4_UNSUPPORTED])
def test_collapsed_up_conv_turns_away(hip, label, c):
    hs, ws = c.src_hw
    L = VC.Launch()
    x0 = dv(torch.zeros(max(c.planes, 1), c.N, hs, ws, c.C0, dtype=torch.int16))
    x1 = dv(torch.zeros(max(c.planes, 1), c.N, hs, ws, c.C1, dtype=torch.int16)) if c.C1 else None
    y = dv(torch.zeros(8))
    L.sx = 1.0
    d = descriptor(hip, c, L, x0, x1, y, [y, y] if c.Co1 else [y])
    assert hip.query("rpnet_conv_up4_supported", C.byref(d), c.up4) == 0


@pytest.mark.parametrize("c", VC.DYNAMIC, ids=ident)
def test_dynamic_range(be, c):
    """source channels spanning 2^-20 .. 2^0 under one tensor scale, per output channel"""
    VC.hold(VC.check_dynamic_range(be, c))


def test_refusals(hip):
    """every refusal happens on the host, before any launch: the status code, the entry point's name at the head of
    rpnet_last_error_string followed by the words of the very RPNET_REQUIRE line the row is about, and every buffer untouched"""
    lib, p = hip.load(), hip.ptr
    big = 1 << 20
    x0, x1, w, y0, y1, aux = (dv(torch.full((big,), 7.0)) for _ in range(6))
    for label, base, ch, want, words in VC.REFUSALS:
        c = base.but(**{k: v for k, v in ch.items() if k in base.__dict__})
        L = VC.Launch()
        if 0 < c.planes < 3 and "no_scales" not in ch:
            L.sx, L.col = 1.0, aux
        null = set(ch.get("null", "").split(","))
        d = descriptor(hip, c, L, x0, x1 if c.C1 else None, w, [y0, y1] if c.Co1 else [y0], aux if c.mode else None)
        d.in_scale_mode = c.mode
        for name in null - {""}:
            setattr(d, name, None)
        for k, v in ch.get("set", {}).items():
            setattr(d, k, p(aux) if k in VC.REFUSAL_POINTERS else v)
        if "huge" in ch:
            d.N, d.H, d.W = ch["huge"]
        if c.fam == "up4":
            got = lib.rpnet_conv_up4(C.byref(d), c.up4, hip.stream())
        else:
            got = lib.rpnet_conv_fwd(C.byref(d), hip.stream())
        msg = lib.rpnet_last_error_string().decode()
        assert got == want, f"{c.entry} ({label}): rc {got}, expected {want}: {msg}"
        assert msg.startswith(VC.REFUSAL_PREFIX[c.entry]), f"{c.entry} ({label}): the message does not start with the entry point: {msg!r}"
        assert words in msg, f"{c.entry} ({label}): refused by another line than the row's ({words!r}): {msg!r}"
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (x0, x1, w, y0, y1, aux))               # nothing ran
