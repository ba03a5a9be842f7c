"""The definition of rpnet_amd.smooth (include/rpnet_smooth_abi.h), as tests/smooth_cases.py restates it, against
scipy.ndimage.gaussian_filter, within a bound that is derived and not measured; the weights against scipy's kernel; the anti-aliased
resample against zoom(gaussian_filter(.)); seeded defects, each shown to fail these checks; and the aliasing the filter is there for.
Runs without a GPU."""
import numpy as np
import pytest
from scipy import ndimage

from rpnet_amd import smooth as SM
from tests import resample_cases as RC
from tests import smooth_cases as SC

SHAPES = (((5, 7, 9), (0.5, 1.0, 1.5)), ((1, 3, 2), (2.0, 2.0, 2.0)), ((6, 40, 33), (0.75, 2.0, 1.25)))


def scipy_smooth(v, sigmas, mode):
    return ndimage.gaussian_filter(np.asarray(v).astype(np.float64), sigmas, mode=mode)


def within_bound(vol, sigmas, mode, defect=()):
    """(is the restatement within twice the derived bound of scipy, the largest error over the bound)"""
    got = SC.smooth_f64(vol, sigmas, mode, defect=defect)
    want = scipy_smooth(vol, sigmas, mode)
    bound = 2.0 * SC.error_bound(vol, sigmas, mode)                     # doubled: scipy rounds too
    ratio = float(np.max(np.abs(got - want) / np.maximum(bound, np.finfo(np.float64).tiny)))
    return bool(np.all(np.abs(got - want) <= bound)), ratio


@pytest.mark.parametrize("mode", SC.MODES)
@pytest.mark.parametrize("shape,sigmas", SHAPES)
def test_restatement_is_scipy_gaussian_filter_within_the_derived_bound(shape, sigmas, mode):
    for dtype in (np.float32, np.int16):
        vol = SC.noise_image(shape, dtype)
        ok, ratio = within_bound(vol, sigmas, mode)
        print(f"{shape} {sigmas} {mode} {np.dtype(dtype).name}: largest error / bound = {ratio:.3g}")
        assert ok, ratio


def test_weights_are_scipys_kernel_and_the_radius_rule():
    from scipy.ndimage._filters import _gaussian_kernel1d
    for sigma, truncate in ((0.75, 4.0), (2.0, 4.0), (8.0, 4.0), (1.3, 3.0), (0.2, 4.0), (63.75, 4.0)):
        w, r = SM.smooth_weights(sigma, truncate)
        assert r == int(truncate * sigma + 0.5)
        assert w.dtype == np.float64 and np.array_equal(w, _gaussian_kernel1d(sigma, 0, r)[::-1]), (sigma, truncate)
        w2, r2 = SC.weights(sigma, truncate)
        assert r2 == r and np.array_equal(w, w2)
    # truncate * sigma + 0.5 exactly on an integer: 4 * 0.625 + 0.5 = 3, 4 * 0.875 + 0.5 = 4; just below it the radius is one less
    assert SM.smooth_weights(0.625)[1] == 3 and SM.smooth_weights(0.875)[1] == 4
    assert SM.smooth_weights(np.nextafter(0.625, 0))[1] == 2 and SM.smooth_weights(0.124)[1] == 0
    for sigma in (0.0, -1.0):
        w, r = SM.smooth_weights(sigma)
        assert r == 0 and np.array_equal(w, [1.0])
    assert SM.smooth_weights(63.75)[1] == 255
    assert SM.smooth_radius(63.75) == 255 and SM.smooth_radius(0.0) == 0 and SM.smooth_radius(0.9, 4.0, "x") == 4
    with pytest.raises(ValueError, match=r"of the z axis gives radius 256"):
        SM.smooth_radius(64.0, 4.0, "z")
    # the device tables are cached per (sigma, truncate, device), whatever the axis, and never evicted (a captured graph holds one)
    import inspect
    assert list(inspect.signature(SM.smooth_device_weights).parameters) == ["sigma", "truncate", "device"]
    assert SM.smooth_device_weights.cache_info().maxsize is None
    with pytest.raises(ValueError, match=r"sigma 64\.0 of the y axis gives radius 256"):
        SM.smooth_weights(64.0, axis="y")
    assert SM.antialias_sigma((64, 512, 512), (80, 205, 205)) == (0.0, (512 / 205 - 1) / 2, (512 / 205 - 1) / 2)
    assert SM.antialias_sigma((8, 20, 20), (8, 8, 8)) == (0.0, 0.75, 0.75) == SC.antialias_sigmas((8, 20, 20), (8, 8, 8))
    assert SM._smooth_sigmas(1.5, (3.0, 1.0, 0.5), "t") == (0.5, 1.5, 3.0) and SM._smooth_sigmas((1, 2, 3), None, "t") == (1.0, 2.0, 3.0)
    for bad in ("a", (1, 2), float("nan")):
        with pytest.raises(ValueError, match="sigma must be"):
            SM._smooth_sigmas(bad, None, "t")
    with pytest.raises(ValueError, match="spacing must be"):
        SM._smooth_sigmas(1.0, (1, 0, 1), "t")


def resample_bound(smoothed):
    """the bound tests/test_host_resample.py derives for the linear rule against scipy's zoom, on the volume the rule is given: the
    coordinate of an axis of length n moves by at most 2^-52 n between the two routes, which moves the interpolant by that times the
    range of the values, summed over the axes; and nine roundings of values no larger than max|v|"""
    from tests.test_host_resample import EPS
    vrange, vmax = float(smoothed.max() - smoothed.min()), float(np.abs(smoothed).max())
    return EPS * sum(smoothed.shape) * vrange + 9 * 2.0 ** -53 * vmax


@pytest.mark.parametrize("shape,new_shape", (((8, 20, 20), (8, 8, 8)), ((5, 7, 9), (8, 5, 13)), ((6, 17, 12), (3, 5, 4))))
def test_antialiased_resample_is_zoom_of_gaussian_filter(shape, new_shape):
    vol = SC.noise_image(shape, np.float32)
    sig = SC.antialias_sigmas(shape, new_shape)
    assert all((s > 0) == (m < n) for s, n, m in zip(sig, shape, new_shape))           # only shrinking axes are filtered
    smoothed = SC.smooth_f64(vol, sig, "nearest")
    got = RC.linear_f64(smoothed, new_shape, "corner")
    want = ndimage.zoom(scipy_smooth(vol, sig, "nearest"), [m / n for m, n in zip(new_shape, shape)], order=1, grid_mode=False)
    assert want.shape == tuple(new_shape)
    # the sum of the two derived bounds: the smoothing's goes through the lerps, which are convex, so its maximum bounds what arrives
    bound = 2.0 * float(np.max(SC.error_bound(vol, sig, "nearest"))) + resample_bound(smoothed)
    err = float(np.max(np.abs(got - want)))
    print(f"{shape} -> {new_shape}: error {err:.3g}, bound {bound:.3g}")
    assert err <= bound
    # and the composed restatement of the device path: the smoothed copy takes the kind of the volume before it is resampled
    np.testing.assert_array_equal(SC.ref_antialiased(vol, new_shape), RC.ref_image(SC.ref_smooth(vol, sig, "nearest"), new_shape, 1, "corner"))


@pytest.mark.parametrize("defect", SC.DEFECTS)
def test_seeded_defects_fail_the_same_checks(defect):
    shape, sigmas = (6, 40, 33), (0.75, 2.0, 1.3)
    vol = SC.noise_image(shape, np.float32)
    assert within_bound(vol, sigmas, "reflect")[0] and within_bound(vol, sigmas, "nearest")[0]
    d = {defect}
    if defect in ("mirror", "clamp for reflect", "radius without half", "unnormalised", "z and x swapped", "float32 between passes"):
        # the radius defect shows where the fraction of 4 sigma is at least a half: 4 * 0.9 = 3.6 -> 4 with the half, 3 without
        sig = (0.9, 2.0, 1.3) if defect == "radius without half" else sigmas
        assert SC.weights(0.9)[1] == 4 and SC.weights(0.9, defect={"radius without half"})[1] == 3
        ok, ratio = within_bound(vol, sig, "reflect", d)
        assert not ok and ratio > 1e3, (defect, ratio)
        assert within_bound(vol, sig, "reflect")[0]
    elif defect == "int16 truncation":
        # weights (0.25, 0.5, 0.25) on (1, 0, 1): exactly 0.5, on (3, 3, 5): 3.5 -> half to even gives 0 and 4, truncation 0 and 3
        tables = ((None, 0), (None, 0), (np.array([0.25, 0.5, 0.25]), 1))
        v = np.array([[[3, 3, 5, 3, 3, 1, 0, 1]]], np.int16)
        good, bad = SC.ref_smooth(v, None, "nearest", tables=tables), SC.ref_smooth(v, None, "nearest", tables=tables, defect=d)
        assert good[0, 0, 1] == 4 and bad[0, 0, 1] == 3 and good[0, 0, 6] == 0
        assert not np.array_equal(good, bad)
    else:
        assert defect == "radius 0 multiplies"
        v = np.array([[[-0.0, 1.5, -0.0]]], np.float32)
        good, bad = SC.ref_smooth(v, (0.0, 0.0, 0.0)), SC.ref_smooth(v, (0.0, 0.0, 0.0), defect=d)
        assert np.array_equal(good.view(np.uint32), v.view(np.uint32))                  # the identity bit for bit
        assert not np.array_equal(bad.view(np.uint32), v.view(np.uint32))               # 0 + 1 * -0.0 is +0.0


def test_int16_ties_and_saturation_of_the_restatement():
    tables = ((None, 0), (None, 0), (np.array([0.25, 0.5, 0.25]), 1))
    v = np.array([[[1, 0, 1, 0, 1, 2, 3, 2, 3, -1, 0, -1, -2, -3, -2]]], np.int16)
    got = SC.ref_smooth(v, None, "nearest", tables=tables)
    f = SC.smooth_f64(v, None, "nearest", tables=tables)
    ties = np.abs(f - np.trunc(f)) == 0.5
    assert ties.sum() >= 6 and {int(x) % 2 for x in np.floor(f[ties])} == {0, 1}        # ties above even and above odd integers
    assert np.array_equal(got[ties], np.rint(f[ties]).astype(np.int16)) and np.all(got[ties] % 2 == 0)
    big = np.array([[[32767, 32767, -32768, -32768]]], np.int16)
    wide = ((None, 0), (None, 0), (np.array([1.0, 1.0, 1.0]), 1))                       # not normalised: the sums leave the range
    assert SC.ref_smooth(big, None, "nearest", tables=wide).tolist() == [[[32767, 32766, -32768, -32768]]]


def test_the_filter_removes_the_aliasing_of_a_checkerboard():
    """1 x 64 x 64 of period 2.  Shrunk to 1 x 24 x 24 under "center" the point samples drift across the phases of the board and the
    output is a moiré of large variance: that is the aliasing, and the filter takes it down to what the Gaussian leaves of a period-2
    pattern.  Shrunk to 1 x 32 x 32 under "center" every sample lies half way between two voxels of each axis and is the mean of a
    2 x 2 block, 500 for either phase: this case shows no aliasing without the filter and is kept only to show that the filter does
    no harm there.  The phase dependence is real where the samples fall on voxel centres: stripes of period 2 along a line of 65
    taken to 33 under "corner" (coordinates 0, 2, 4, ...) give the constant 1000 or the constant 0 by phase, the pattern's energy gone
    into the mean, and the filter brings both to the true mean within what it leaves of the stripes."""
    y, x = np.mgrid[0:64, 0:64]
    board = (1000.0 * ((x + y) % 2))[None].astype(np.float32)
    mean = 500.0
    for phase in (board, np.roll(board, 1, axis=2)):
        assert np.all(RC.ref_image(phase, (1, 32, 32), 1, "center") == mean)          # 2 x 2 means: no aliasing to remove
    plain24 = RC.ref_image(board, (1, 24, 24), 1, "center")
    assert plain24.std() > 100                                        # the moiré
    for new in ((1, 32, 32), (1, 24, 24)):
        sig = SC.antialias_sigmas(board.shape, new)
        assert sig[0] == 0.0 and sig[1] == sig[2] == (64 / new[1] - 1) / 2
        w, r = SC.weights(sig[1])
        k = np.arange(-r, r + 1)
        atten = abs(float(np.sum(w * (-1.0) ** k)))                  # what one pass leaves of a period-2 pattern
        assert atten < 0.6                                           # sigma 0.5: (1 - 2 e^-2) / (1 + 2 e^-2) = 0.574
        out = SC.ref_antialiased(board, new, "center").astype(np.float64)
        # the board is the outer pattern (-1)^(x + y): the two passes leave atten^2 of its amplitude 500, and a lerp only averages.
        # That holds where no tap reaches the border (the clamp repeats the edge voxel, which is not how the board goes on): an output
        # reads the voxels within r + 1 of its coordinate, so the outputs nearer than (r + 2) / (n / m) to the edge are left out
        edge = int(np.ceil((r + 2) / (64 / new[1])))
        inner = out[:, edge:-edge, edge:-edge]
        print(f"{new}: attenuation per pass {atten:.4f}, largest deviation from the mean {np.abs(inner - mean).max():.3f} "
              f"(with the border: {np.abs(out - mean).max():.3f})")
        assert inner.size >= 16 * 16 and np.abs(inner - mean).max() <= 500.0 * atten * atten + 1e-3
    # stripes on voxel centres: the constant depends on the phase without the filter, and does not with it
    stripes = (1000.0 * (np.arange(65) % 2)).reshape(1, 1, 65).astype(np.float32)
    for phase, constant in ((stripes, 0.0), (1000.0 - stripes, 1000.0)):
        assert np.all(RC.ref_image(phase, (1, 1, 33), 1, "corner") == constant)
        sig = SC.antialias_sigmas(phase.shape, (1, 1, 33))
        assert sig[:2] == (0.0, 0.0) and sig[2] == (65 / 33 - 1) / 2
        w, r = SC.weights(sig[2])
        atten = abs(float(np.sum(w * (-1.0) ** np.arange(-r, r + 1))))
        out = SC.ref_antialiased(phase, (1, 1, 33), "corner").astype(np.float64)
        edge = int(np.ceil((r + 2) / (65 / 33)))
        print(f"stripes, plain constant {constant}: attenuation {atten:.4f}, largest deviation {np.abs(out[..., edge:-edge] - mean).max():.3f}")
        assert atten < 1 and np.abs(out[..., edge:-edge] - mean).max() <= 500.0 * atten + 1e-3 < 500.0
