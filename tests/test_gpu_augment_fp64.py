"""GPU parity of the train-time augmentation (csrc/augment.hip: rpnet_slice_minmax, rpnet_augment_affine, rpnet_elastic_field,
rpnet_elastic_apply) against the numpy restatements of tests/augment_ref_cases.py, which word the four entry points as
include/rpnet_abi.h does: at an exact tie the header's pixel-space rule is the contract, not torch's normalised grid.  Every call goes
through rpnet_amd.hip.call directly, not rpnet_amd.augment; every output and every intermediate (mm, tmp, field, img_tmp, mask_tmp, the
outputs) is prefilled with NaN and stands between RC.GUARD sentinel elements, and every call is made twice.  The tables, the bounds and
every comparison live in tests/augment_ref_cases.py (shared with tests/test_host_augment_ref64.py, which shows on the CPU that a correct
implementation passes and that seeded defects fail).  Every arithmetic check prints `PARITY augment family what err bound`;
profiles/augment_parity.txt keeps each family's largest value."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import augment_ref_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
SENTINEL = -12345.0


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


def dv(a):
    """device copy of a numpy array, referenced until the test ends"""
    if a is None:
        return None
    _ALIVE.append(torch.from_numpy(np.ascontiguousarray(a)).to(DEV))
    return _ALIVE[-1]


class Guarded:
    """an output of `shape`, prefilled with NaN, between two bands of RC.GUARD sentinel elements"""

    def __init__(self, shape, dtype=torch.float32):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * RC.GUARD,), SENTINEL, dtype=dtype, device=DEV)
        self.view = self.buf[RC.GUARD:RC.GUARD + self.n].view(tuple(shape))
        self.view.fill_(NAN)
        _ALIVE.append(self.buf)

    def ptr(self):
        return self.view.data_ptr()

    def touched(self):
        return int((self.buf[:RC.GUARD] != SENTINEL).sum() + (self.buf[RC.GUARD + self.n:] != SENTINEL).sum())

    def numpy(self):
        return self.view.cpu().numpy()


def gp(g):
    return None if g is None else g.ptr()


def same_bits(a, b):
    return a.view(np.uint8).reshape(-1) == b.view(np.uint8).reshape(-1)


class HipBackend:
    """the four entry points of the library on numpy arrays (tests/augment_ref_cases.py); each is called twice on fresh guarded buffers"""

    def __init__(self, hip):
        self.hip = hip

    def _twice(self, name, shapes, args):
        """shapes: {key: (shape, dtype) or None}; args(outs) -> the argument list.  -> the first call's arrays, guards, repeat"""
        runs = []
        for _ in range(2):
            outs = {k: (None if s is None else Guarded(*s)) for k, s in shapes.items()}
            self.hip.call(name, *args(outs))
            torch.cuda.synchronize()
            runs.append(outs)
        res = {k: (None if g is None else g.numpy()) for k, g in runs[0].items()}
        res["guards"] = sum(g.touched() for r in runs for g in r.values() if g is not None)
        res["repeat"] = sum(int((~same_bits(res[k], g.numpy())).sum()) for k, g in runs[1].items() if g is not None)
        return res

    def minmax(self, x):
        S, H, W = x.shape
        d = dv(x)
        return self._twice("rpnet_slice_minmax", {"mm": ((S, 2), torch.float32)}, lambda o: (d.data_ptr(), o["mm"].ptr(), S, H, W))

    def affine(self, img, lab, params, mm):
        p = self.hip.ptr
        S, H, W = (img if img is not None else lab).shape
        di, dl, dp, dm = dv(img), dv(lab), dv(params), dv(mm)
        shapes = {"img_out": None if img is None else ((S, H, W), torch.float32), "lab_out": None if lab is None else ((S, H, W), torch.float32)}
        return self._twice("rpnet_augment_affine", shapes, lambda o: (p(di), p(dl), p(dp), p(dm), gp(o["img_out"]), gp(o["lab_out"]), S, H, W))

    def field(self, noise, w, radius, alpha):
        _, H, W = noise.shape
        dn, dw = dv(noise.astype(np.float64)), dv(np.asarray(w, dtype=np.float64))
        shapes = {"tmp": ((2, H, W), torch.float64), "field": ((2, H, W), torch.float32)}
        return self._twice("rpnet_elastic_field", shapes, lambda o: (dn.data_ptr(), dw.data_ptr(), int(radius), float(alpha), o["tmp"].ptr(),
                                                                     o["field"].ptr(), H, W))

    def elastic(self, img, mask, minv, field, pad):
        p = self.hip.ptr
        S, H, W = (img if img is not None else mask).shape
        di, dm, df = dv(img), dv(mask), dv(np.asarray(field, dtype=np.float32))
        m = (C.c_double * 6)(*[float(v) for v in np.asarray(minv, dtype=np.float64).reshape(6)])
        one = ((S, H, W), torch.float32)
        shapes = {"img_tmp": None if img is None else one, "img_out": None if img is None else one,
                  "mask_tmp": None if mask is None else one, "mask_out": None if mask is None else one}
        return self._twice("rpnet_elastic_apply", shapes, lambda o: (p(di), p(dm), m, p(df), gp(o["img_tmp"]), gp(o["mask_tmp"]), gp(o["img_out"]),
                                                                     gp(o["mask_out"]), S, H, W, float(pad)))


@pytest.fixture(scope="module")
def be(hip):
    return HipBackend(hip)


def ident(v):
    if isinstance(v, tuple):
        return "x".join(ident(i) for i in v)
    return str(v)


@pytest.mark.parametrize("plane", RC.PLANES, ids=ident)
def test_slice_minmax(be, plane):
    """rpnet_slice_minmax: {min, max} of every slice by value, at H W below, at and above the 1024-thread stride"""
    for p, S, kind in RC.MINMAX_ROWS:
        if p == plane:
            RC.hold(RC.check_minmax(be, p, S, kind))


@pytest.mark.parametrize("plane", RC.PLANES, ids=ident)
def test_affine_exact_maps(be, plane):
    """rpnet_augment_affine with dyadic maps and the power law off: labels and images bit for bit on every pixel, exact ties (half to
    even), the edge of the plane and a partial last block included; image pair alone, label pair alone, both"""
    for p, S, first, pairs in RC.EXACT_ROWS:
        if p == plane:
            RC.hold(RC.check_affine_exact(be, p, S, first, pairs))


@pytest.mark.parametrize("plane,S,seed,args", RC.RANDOM_ROWS, ids=ident)
def test_affine_drawn_maps(be, plane, S, seed, args):
    """rpnet_augment_affine with maps of draw_random_affine on odd planes: equal outside the rounding band, a candidate inside it"""
    RC.hold(RC.check_affine_random(be, plane, S, seed, args))


@pytest.mark.parametrize("case", RC.IMAGE_CASES)
def test_affine_image_path(be, case):
    """rpnet_augment_affine's image path: the power law at exponents 0.5, 1, 1.5 within 2^-22, the flag as 0 / -0.0 / another non-zero
    number, zeros and the fill taking `lo`, a constant slice, extremes at the last element"""
    for c, plane, pairs in RC.IMAGE_ROWS:
        if c == case:
            RC.hold(RC.check_image(be, c, plane, pairs))


def test_sixty_five_thousand_slices(be):
    """rpnet_slice_minmax and rpnet_augment_affine with S = 65535 on a 1 x 3 plane: blockIdx.y at its limit"""
    RC.hold(RC.check_big_s(be))


@pytest.mark.parametrize("row", RC.FIELD_ROWS, ids=ident)
def test_elastic_field(be, row):
    """rpnet_elastic_field with the caller's weights: radius 0 bit for bit, radius 1, sigma 30 on planes far smaller than the radius
    (the reflect period crossed many times), sigma 2; random planes and corner / centre impulses; within one fp32 ulp"""
    RC.hold(RC.check_field(be, *row))


@pytest.mark.parametrize("minv", list(RC.MINV))
def test_elastic_apply_crafted(be, minv):
    """rpnet_elastic_apply on dyadic coordinates and pixel values: both stages of image and mask bit for bit; rint ties in stage 1,
    floor(c + 0.5) in stage 2, landing exactly on 0 / n-1 and 2^-20 outside, either triple alone, both padding values"""
    for row in RC.ELASTIC_CRAFTED:
        if row[2] == minv:
            RC.hold(RC.check_elastic_crafted(be, *row))


@pytest.mark.parametrize("row", RC.ELASTIC_RANDOM, ids=ident)
def test_elastic_apply_drawn(be, row):
    """rpnet_elastic_apply with Minv of draw_elastic and a random fp32 field: mask equal on every pixel, image within one fp32 ulp"""
    RC.hold(RC.check_elastic_random(be, *row))


@pytest.mark.parametrize("entry", ["minmax", "affine", "field", "elastic"])
def test_production_size_once(be, entry):
    """rpnet_slice_minmax, rpnet_augment_affine, rpnet_elastic_field and rpnet_elastic_apply at 12 slices of 256 x 256, once each"""
    RC.hold(RC.check_production(be, entry))


def test_no_slices_is_success_and_writes_nothing(hip):
    """rpnet_slice_minmax, rpnet_augment_affine and rpnet_elastic_apply with S == 0: success, the prefill untouched"""
    H, W = 4, 4
    outs = [Guarded((2, H, W)) for _ in range(6)]
    src, fld, par = dv(np.ones((2, H, W), np.float32)), dv(np.zeros((2, H, W), np.float32)), dv(np.zeros((2, 8), np.float32))
    m = (C.c_double * 6)(*RC.MINV6)
    hip.call("rpnet_slice_minmax", src.data_ptr(), outs[0].ptr(), 0, H, W)
    hip.call("rpnet_augment_affine", src.data_ptr(), src.data_ptr(), par.data_ptr(), outs[0].ptr(), outs[1].ptr(), outs[2].ptr(), 0, H, W)
    hip.call("rpnet_elastic_apply", src.data_ptr(), src.data_ptr(), m, fld.data_ptr(), outs[2].ptr(), outs[3].ptr(), outs[4].ptr(), outs[5].ptr(),
             0, H, W, -1.0)
    hip.call("rpnet_slice_minmax", None, None, 0, H, W)                 # nothing is read either
    torch.cuda.synchronize()
    assert all(np.isnan(g.numpy()).all() and g.touched() == 0 for g in outs)


def test_refusals(hip):
    """rpnet_slice_minmax, rpnet_augment_affine, rpnet_elastic_field and rpnet_elastic_apply: every refusal happens on the host, before
    any launch: the documented status code, a message that names the entry point and says what was wrong, and no output touched"""
    def buf(n, dtype=torch.float32):
        _ALIVE.append(torch.full((n,), 7.0, device=DEV, dtype=dtype))
        return _ALIVE[-1]

    def conv(a):
        if isinstance(a, tuple):
            return (C.c_double * 6)(*a)
        return hip.ptr(a) if torch.is_tensor(a) else a

    rows, outputs = RC.refusals(buf, lambda n: buf(n, torch.float64))
    lib = hip.load()
    for label, entry, args, want, words in rows:
        got = getattr(lib, entry)(*[conv(a) for a in args], hip.stream())
        msg = lib.rpnet_last_error_string().decode()
        assert got == want, f"{entry} ({label}): rc {got}, expected {want}: {msg}"
        assert msg.startswith(entry[len("rpnet_"):] + ":") and words in msg, f"{entry} ({label}): expected {words!r} in {msg!r}"
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outputs)               # nothing ran
