"""The restatement of tests/volload_cases.py (the definitions of include/rpnet_volload_abi.h in numpy) against the host reader and numpy,
without a GPU: bit for bit FewshotVolumeReader.load_image_and_mask on every geometry row of tests/test_gpu_volload.py; numpy.percentile
of the installed numpy (2.2.6 when this was written: its virtual index is a float32 for a float32 array); the key transform keeps numpy's
order; and the seeded defects each change a row.  rpnet_amd.volume_load's host arithmetic (load_geometry, percentile_rank) is the
restatement's."""
import os

import numpy as np
import pytest

from rpnet_amd import volume_load as VL
from rpnet_amd.utils import nrrd
from rpnet_amd.utils import volume_reader as VR
from tests import volload_cases as VC

F = np.float32


def bare_reader(data_dir, cfg):
    """a FewshotVolumeReader with the two attributes load_image_and_mask reads (no csv lists)"""
    rd = object.__new__(VR.FewshotVolumeReader)
    rd.data_dir, rd.cfg = str(data_dir), cfg
    return rd


def write_pair(data_dir, pid, image, mask):
    os.makedirs(data_dir, exist_ok=True)
    nrrd.write(os.path.join(data_dir, f"{pid}_clean.nrrd"), image)
    nrrd.write(os.path.join(data_dir, f"{pid}_Liver.nrrd"), mask)


def reader_pieces(rd, image, mask, lo, hi):
    """truncate, pad to 16, [lo:hi), crop: the reader's own functions without its z range and normalize"""
    cfg = rd.cfg
    m = VR.pad2factor(rd.truncate_image(mask.astype(np.float32)), 16, 0)[None]
    v = VR.pad2factor(rd.truncate_image(image), 16, cfg["pad_value"])[None].astype(np.float32)
    v, m = VR.crop(v[:, lo:hi], m[:, lo:hi], cfg["crop_size"], cfg["pad_value"], 0)
    return v[0], m[0]


@pytest.fixture(scope="module")
def synthetic(tmp_path_factory):
    """write_synthetic_dataset volumes of the three file shapes it can write (a one-voxel volume holds no organ)"""
    out = {}
    for shape in VC.FILE_SHAPES[1:]:
        root = tmp_path_factory.mktemp("vl%dx%dx%d" % shape)
        data_dir, _, _ = VR.write_synthetic_dataset(str(root), n_volumes=2, shape=shape, seed=sum(shape))
        out[shape] = data_dir
    return out


@pytest.mark.parametrize("row", VC.GEOMETRY_ROWS[3:], ids=lambda r: "%s-%s-%s" % r)
def test_restatement_equals_the_reader_on_synthetic_volumes(row, synthetic):
    shape, window, crop = row
    cfg = VC.config(window, crop)
    rd = bare_reader(synthetic[shape], cfg)
    for pid in ("case000", "case001"):
        want = rd.load_image_and_mask(pid, "Liver")
        image, _ = nrrd.read(os.path.join(rd.data_dir, f"{pid}_clean.nrrd"))
        mask, _ = nrrd.read(os.path.join(rd.data_dir, f"{pid}_Liver.nrrd"))
        assert image.dtype == np.int16 and mask.dtype == np.uint8 and image.shape == shape
        got_i, got_m = VC.ref_load(image, mask, cfg)
        assert got_i.dtype == got_m.dtype == np.float32 and got_i.shape == want["image"][0].shape and got_i.shape[0] > 0
        assert VC.bits(got_i).tobytes() == VC.bits(want["image"][0]).tobytes(), row
        assert VC.bits(got_m).tobytes() == VC.bits(want["mask"][0]).tobytes(), row
        g = VL.load_geometry(cfg, shape)
        assert {k: g[k] for k in VC.ref_geometry(shape, window, crop)} == VC.ref_geometry(shape, window, crop)


@pytest.mark.parametrize("row", VC.GEOMETRY_ROWS, ids=lambda r: "%s-%s-%s" % r)
@pytest.mark.parametrize("kinds", [(np.int16, np.uint8), (np.float32, np.float32), (np.float32, np.int16)], ids=lambda k: k[0].__name__ + "-" + k[1].__name__)
def test_restatement_equals_the_reader_for_every_kind_and_annotation(row, kinds, tmp_path):
    """files of the test's own for every image and mask kind: annotations from the first slice, to the last slice, and two annotated
    slices (depth 1); the float mask's fractional values pass through; the one-voxel file through the reader's pieces"""
    shape, window, crop = row
    cfg = VC.config(window, crop)
    rd = bare_reader(tmp_path, cfg)
    D = shape[0]
    nz = min(D, window[0])
    image = VC.file_volume(shape, kinds[0], seed=1)
    spans = [(0, 0)] if nz == 1 else [(0, nz - 1), (nz // 2, nz // 2 + 1), (0, 1), (nz - 2, nz - 1)]
    for j, (zf, zl) in enumerate(spans):
        mask = VC.file_mask(shape, kinds[1], zf, zl, seed=j)
        g = VC.ref_geometry(shape, window, crop)
        assert VC.ref_range(mask, g)[:2] == (zf, zl)
        if zf == zl:                                                     # the reader's [lo:hi) is empty: compare the pieces at depth 1
            wi, wm = reader_pieces(rd, image, mask, 0, 1)
            gi, gm = VC.ref_gather(image, g, 0, 1, cfg["pad_value"]), VC.ref_gather(mask, g, 0, 1, 0.0)
        else:
            write_pair(str(tmp_path), f"p{j}", image, mask)
            want = rd.load_image_and_mask(f"p{j}", "Liver")
            wi, wm = want["image"][0], want["mask"][0]
            gi, gm = VC.ref_load(image, mask, cfg)
            pi, pm = reader_pieces(rd, image, mask, zf, zl)
            assert VC.bits(VC.ref_gather(image, g, zf, zl, cfg["pad_value"])).tobytes() == VC.bits(pi).tobytes()
            assert gi.shape[0] == zl - zf and (zl - zf == 1 or j != 1)
        assert gi.shape == wi.shape and VC.bits(gi).tobytes() == VC.bits(wi).tobytes(), (row, j)
        assert VC.bits(gm).tobytes() == VC.bits(wm).tobytes(), (row, j)
        if kinds[1] is np.float32 and zf != zl:
            assert ((gm > 0) & (gm < 1)).any()


def test_percentile_restatement_equals_the_installed_numpy():
    """np.percentile(x, 99.5) of numpy 2.2.6 (VC.NUMPY_PINNED; the installed version is printed and must behave alike): every selection
    case, every n up to 1200, and sizes of real volumes, where the float32 virtual index is coarse; the radix selection gives the values
    numpy's sort gives"""
    print("numpy", np.__version__, "pinned", VC.NUMPY_PINNED)
    for name, x in VC.selection_cases().items():
        with np.errstate(invalid="ignore"):
            want = np.percentile(x, 99.5)
        assert want.dtype == np.float32
        assert VC.same_bits_nan(VC.ref_percentile(x), want, zeros_by_value=True), name
        k0, k1, g = VC.ref_rank(x.size)
        a, b, n_nan = VC.ref_select(x, (k0, k1))
        s = np.sort(x)
        assert VC.same_bits_nan(F(a) + F(0), s[k0] + F(0)) and VC.same_bits_nan(F(b) + F(0), s[k1] + F(0)) and n_nan == int(np.isnan(x).sum()), name
        assert VL.percentile_rank(x.size, 99.5) == (k0, k1, g)
    rs = np.random.RandomState(9)
    for n in list(range(1, 1200)) + [4097, 65536, 1 << 20, 16 * 256 * 256 - 3]:
        x = rs.normal(0, 300, n).astype(np.float32)
        assert VC.same_bits_nan(VC.ref_percentile(x), np.percentile(x, 99.5)), n
        k0, k1, g = VL.percentile_rank(n, 99.5)
        assert (k0, k1, g) == VC.ref_rank(n) and 0 <= k0 <= k1 <= n - 1 and 0 <= g < 1
    # a whole 64 x 256 x 256 volume: the float32 index is a multiple of 0.5 here and differs from (n - 1) * 0.995 in float64
    n = 64 * 256 * 256
    x = rs.normal(0, 300, n).astype(np.float32)
    assert VC.same_bits_nan(VC.ref_percentile(x), np.percentile(x, 99.5))
    assert VC.ref_rank(n) != VC.ref_rank(n, defect="index_f64")
    # the whole normalize against the reader's, with bounds that float32 does not hold and a range below 1
    x = (rs.normal(0, 1, 5000) * 0.4).astype(np.float32)
    for mn, mx in ((-1024, 3072), (0.1, 0.7), (-0.3, 0.1), (-1024, 3076)):
        assert VC.bits(VC.ref_normalize(x, mn, mx)).tobytes() == VC.bits(VR.normalize(x, mn, mx)).tobytes(), (mn, mx)


def test_key_transform_is_order_preserving():
    specials = np.array([-np.inf, -3.4e38, -1.0, -1.2e-38, -1e-45, -0.0, 0.0, 1e-45, 1.2e-38, 1.0, 3.4e38, np.inf], np.float32)
    rs = np.random.RandomState(2)
    x = np.concatenate([specials, rs.randint(0, 1 << 32, 20000, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    x = x[~np.isnan(x)]
    key = VC.ref_key(x).astype(np.int64)
    i, j = rs.randint(0, x.size, 200000), rs.randint(0, x.size, 200000)
    assert np.array_equal(x[i] < x[j], key[i] < key[j]) and np.array_equal(x[i] == x[j], key[i] == key[j])
    assert VC.ref_key(F(-0.0)) == VC.ref_key(F(0.0)) == 0x80000000
    back = VC.ref_unkey(VC.ref_key(x))
    assert np.array_equal(back, x) and not np.signbit(back[x == 0]).any()
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001], np.uint32).view(np.float32)
    assert (VC.ref_key(nans) == 0xFFFFFFFF).all() and (VC.ref_key(nans) > VC.ref_key(F(np.inf))).all()
    assert np.isnan(VC.ref_unkey(np.array([0xFFFFFFFF], np.uint32))[0])


def _rows_that_differ(defect):
    """the rows of this file on which the restatement with `defect` gives other bits (or breaks) than the restatement"""
    rows = []
    for name, x in VC.selection_cases().items():
        try:
            bad = VC.ref_normalize(x, *VC.HU, defect=defect)
        except IndexError:
            rows.append(name)
            continue
        if not VC.same_bits_nan(bad, VC.ref_normalize(x, *VC.HU)) or not VC.same_bits_nan(VC.ref_percentile(x, defect=defect), VC.ref_percentile(x)):
            rows.append(name)
    for seed in range(200):                          # rows of noise: a double rounding of the lerp shows in a few per cent of them
        x = np.random.RandomState(seed).normal(0, 100, 257 + seed).astype(np.float32)
        try:
            if not VC.same_bits_nan(VC.ref_percentile(x, defect=defect), VC.ref_percentile(x)):
                rows.append(f"noise{seed}")
        except IndexError:
            rows.append(f"noise{seed}")
    for shape, window, crop in VC.GEOMETRY_ROWS[3:]:
        cfg = VC.config(window, crop)
        image, mask = VC.file_volume(shape, np.int16, 1), VC.file_mask(shape, np.uint8, 1, min(shape[0], window[0]) - 2)
        good, bad = VC.ref_load(image, mask, cfg), VC.ref_load(image, mask, cfg, defect=defect)
        if any(a.shape != b.shape or not VC.same_bits_nan(a, b) for a, b in zip(good, bad)):
            rows.append((shape, window, tuple(crop)))
    return rows


@pytest.mark.parametrize("defect", [d for d in VC.DEFECTS if d != "fused_map"])
def test_seeded_defects_each_fail_a_row(defect):
    """k + 1 not clamped at n - 1; floor replaced by round; the lerp in float64; the extra crop pixel at the near end; lo:hi + 1; the
    virtual index in float64: each changes the bits of at least one row"""
    rows = _rows_that_differ(defect)
    print(defect, len(rows), rows[:4])
    assert rows, defect


def test_a_fused_multiply_by_two_cannot_be_seen():
    """`r * 2 - 1` contracted into one FMA gives the same bits as two roundings for every float32 r: r * 2 is exact (a power of two, no
    overflow below 1.7e38, exact in the subnormals too), so both forms round 2r - 1 once.  The defect is seeded all the same and shown to
    change no row; what the flag -ffp-contract=off protects is the lerp, whose product is not exact (test above: lerp_f64)."""
    assert _rows_that_differ("fused_map") == []
    r = np.random.RandomState(4).randint(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32).view(np.float32)
    r = r[np.isfinite(r) & (np.abs(r) < 1e38)]
    two = (r * F(2)).astype(np.float32) - F(1)
    assert VC.bits(two).tobytes() == VC.bits((r.astype(np.float64) * 2 - 1).astype(np.float32)).tobytes()


def test_host_refusals_name_the_host_reader():
    cfg = VC.config((20, 40, 40), [32, 32])
    for bad in (dict(cfg, num_x=1), dict(cfg, num_slice=0), dict(cfg, crop_size=[0, 32]), dict(cfg, crop_size=[32, 2000])):
        with pytest.raises(ValueError, match="load_image_and_mask"):
            VL.load_geometry(bad, (22, 44, 40))
    with pytest.raises(ValueError, match="load_image_and_mask"):
        VL.load_geometry(cfg, (22, 44, 2000))
    with pytest.raises(RuntimeError, match="MI355X only"):
        VL.DeviceVolumeLoader(bare_reader(".", cfg), "cpu")
    with pytest.raises(ValueError, match="within 0..100"):
        VL.percentile_rank(10, 101.0)
