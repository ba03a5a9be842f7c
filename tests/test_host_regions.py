"""The region statistics without a GPU: the numpy restatement of tests/regions_cases.py against scipy.ndimage and against a scalar
statement of the header's summation order, `derive` and `compare` of rpnet_amd/regions.py against direct numpy on the masks, seeded
defects of the restatement shown to fail those same checks, the workspace formula and the host refusals of `region_stats`."""
import math

import numpy as np
import pytest
import torch
from scipy import ndimage

from rpnet_amd import hip
from rpnet_amd import regions as R
from tests import regions_cases as RC

U = 2.0 ** -52


def scalar_sum(n, sparse):
    """SUM of include/rpnet_region_abi.h, one Python float addition per addition of the header.  sparse: {linear index: term}; every
    other voxel adds nothing (a chunk, a lane or a partial without a term is +0.0, and x + 0.0 == x for every x that can occur)"""
    lanes = {}
    for i in sorted(sparse):
        c, t = i // 4096, (i % 4096) // 16
        lanes.setdefault(c, [0.0] * 256)
        lanes[c][t] = lanes[c][t] + sparse[i]

    def tree(a):
        a, s = list(a), 128
        while s:
            for t in range(s):
                a[t] = a[t] + a[t + s]
            s //= 2
        return a[0]
    n_chunks = (n + 4095) // 4096
    G = min(n_chunks, 1024)
    P = [0.0] * G
    for c in sorted(lanes):                 # ascending chunks: for every block its trips in ascending order
        P[c % G] = P[c % G] + tree(lanes[c])
    part = [0.0] * 256
    for b in range(G):                      # ascending blocks: for every thread its partials in ascending order
        part[b % 256] = part[b % 256] + P[b]
    return tree(part)


def wild_terms(n, seed, at=None):
    """terms whose sum depends on the order of the additions: magnitudes from 1e-3 to 1e9 of both signs"""
    rng = np.random.RandomState(seed)
    at = np.arange(n) if at is None else at
    terms = np.zeros(n, np.float64)
    terms[at] = rng.standard_normal(at.size) * 10.0 ** rng.randint(-3, 10, size=at.size)
    return terms, at


def order_checks(defect=None):
    """the vectorised SUM against the scalar one, bit for bit: a dense volume of a few chunks with a ragged end, and a sparse one whose
    block 0 makes three trips (two partial sums commute; three do not)"""
    for n, seed in ((3 * 4096 + 1234, 1), (17, 2), (4096, 3)):
        terms, at = wild_terms(n, seed)
        want = scalar_sum(n, {int(i): float(terms[i]) for i in at})
        got = RC.ordered_sum(terms, defect)
        assert np.float64(got).tobytes() == np.float64(want).tobytes(), (n, got, want)
    n = 2060 * 4096 + 5
    at = np.concatenate([(b + trip * 1024) * 4096 + np.arange(0, 4096, 97) for b in range(12) for trip in range(3)] + [np.array([n - 1])])
    terms, at = wild_terms(n, 4, at)
    want = scalar_sum(n, {int(i): float(terms[i]) for i in at})
    got = RC.ordered_sum(terms, defect)
    assert np.float64(got).tobytes() == np.float64(want).tobytes(), ("three trips", got, want)


def special_image(shape, seed):
    """finite values of both signs with -0.0, subnormals and the ends of the range, and NaN and +-inf among them"""
    rng = np.random.RandomState(seed)
    img = (rng.standard_normal(shape) * 200.0 - 30.0).astype(np.float32)
    flat = img.ravel()
    pick = rng.permutation(flat.size)[:max(flat.size // 10, 8)]
    flat[pick] = np.resize(np.array([np.nan, np.inf, -np.inf, -0.0, 1e-42, -1e-42, np.finfo(np.float32).max, -np.finfo(np.float32).max],
                                    np.float32), pick.size)
    return img


def scipy_checks(defect=None):
    """the restatement against scipy.ndimage on random label maps and images: counts, boxes, extrema and the integer moments EQUAL; S1
    and S2 within the summation bound n * 2^-52 * sum |term| (every partial sum of n terms is within that of the exact sum, whatever
    the order: Higham, Accuracy and Stability of Numerical Algorithms, section 4.2; scipy's own sum is held to the same bound)"""
    for shape, L, lo, seed, kind in (((5, 3, 17), 4, 1, 1, "f32"), ((3, 37, 41), 7, 0, 2, "f32"), ((2, 50, 60), 3, 1, 3, "i16"),
                                      ((1, 17, 241), 5, 1, 4, "special")):
        labels = RC.noise_labels(shape, L, seed, outside=2) if seed % 2 else RC.blob_labels(shape, L, seed)
        image = special_image(shape, seed) if kind == "special" else RC.image_for(shape, seed, kind)
        rows_i, rows_f, n_outside = RC.restate(labels, image, lo=lo, L=L, defect=defect)
        assert n_outside == int((labels >= L).sum())
        index = np.arange(L)
        lab = np.where(labels < L, labels, 255).astype(np.int64)        # 255: no label asked for
        ones = np.ones(shape)
        zz, yy, xx = (g.astype(np.float64) for g in np.indices(shape))
        assert rows_i.shape == (L, RC.IROW) and rows_f.shape == (L, RC.FROW) and (rows_i[:, 19] == 0).all()
        counts = ndimage.sum_labels(ones, lab, index).astype(np.int64)
        boxes = ndimage.find_objects(np.where(labels < L, labels, 0).astype(np.int64), max_label=L - 1)
        img64 = np.asarray(image, np.float64)
        finite = np.isfinite(img64)
        safe = np.where(finite, img64, 0.0)
        for l in range(L):
            row = rows_i[l]
            if l < lo or counts[l] == 0:
                assert np.array_equal(row, RC.empty_row(shape)) and (rows_f[l] == 0).all(), l
                continue
            assert row[0] == counts[l]
            if l >= 1:
                box = boxes[l - 1]
                assert [s.start for s in box] == list(row[1:4]) and [s.stop - 1 for s in box] == list(row[4:7]), l
            moments = [zz, yy, xx, zz * zz, yy * yy, xx * xx, zz * yy, zz * xx, yy * xx]
            want = [int(ndimage.sum_labels(m, lab, l)) for m in moments]            # sums of integers below 2^53: exact in float64
            assert want == list(row[7:16]), (l, want, list(row[7:16]))
            com = ndimage.center_of_mass(ones, lab, l)
            assert tuple(row[7 + a] / row[0] for a in range(3)) == tuple(float(c) for c in com)
            inside = (lab == l) & finite
            n_f = int(inside.sum())
            assert row[16] == n_f
            if not n_f:
                assert row[17] == 0xFFFFFFFF and row[18] == 0 and (rows_f[l] == 0).all()
                continue
            lab_f = np.where(inside, 1, 0)
            lo_v, hi_v = RC.key_value([row[17], row[18]])
            assert float(lo_v) == float(ndimage.minimum(safe, lab_f, 1)) and float(hi_v) == float(ndimage.maximum(safe, lab_f, 1)), l
            assert lo_v <= hi_v
            s1, s2 = float(ndimage.sum_labels(safe, lab_f, 1)), float(ndimage.sum_labels(safe * safe, lab_f, 1))
            b1, b2 = n_f * U * float(np.abs(safe[inside]).sum()), n_f * U * float((safe[inside] ** 2).sum())
            assert math.isfinite(rows_f[l, 0]) and abs(rows_f[l, 0] - s1) <= b1, (l, rows_f[l, 0], s1, b1)
            if math.isfinite(s2):
                assert abs(rows_f[l, 1] - s2) <= b2, (l, rows_f[l, 1], s2, b2)
            if kind != "special":
                # the variance S2 / n - mean^2: S2 / n is within n u (S2 / n) and mean^2 within 2 n u (S2 / n) (Cauchy-Schwarz) of
                # the exact figures; scipy's two-pass figure carries an error of the same kind: 8 n u (S2 / n) covers both
                fig = R.derive(rows_i, rows_f)[l]
                sd = float(ndimage.standard_deviation(safe, lab_f, 1))
                assert abs(fig["std"] ** 2 - sd ** 2) <= 8 * n_f * U * (s2 / n_f), (l, fig["std"], sd)
                assert abs(fig["mean"] - s1 / n_f) <= 2 * b1 / n_f


def all_checks(defect=None):
    order_checks(defect)
    scipy_checks(defect)


def test_restatement_against_scipy_and_the_scalar_order():
    all_checks()


@pytest.mark.parametrize("defect", RC.DEFECTS)
def test_seeded_defects_fail_the_same_checks(defect):
    assert len(RC.DEFECTS) >= 6
    with pytest.raises(AssertionError):
        all_checks(defect)


def test_key_orders_like_the_values_and_decodes():
    v = np.array([-np.finfo(np.float32).max, -3.5, -1e-42, -0.0, 0.0, 1e-42, 2.0, np.finfo(np.float32).max], np.float32)
    k = RC.float_key(v).astype(np.int64)
    assert (np.diff(k) >= 0).all() and k[3] == k[4] == 0x80000000 and k[0] == 0x00800000 and k[-1] == 0xFF7FFFFF
    assert np.array_equal(RC.key_value(k), np.where(v == 0, np.float32(0.0), v)) and np.array_equal(R.key_to_float(k), RC.key_value(k))
    assert np.array_equal(RC.float_key(np.array([-32768, 32767], np.int16).astype(np.float32)), RC.float_key(np.array([-32768.0, 32767.0])))


def rotated_slab(shape, angle):
    zz, yy, xx = np.indices(shape).astype(np.float64)
    c, s = math.cos(angle), math.sin(angle)
    u = (yy - shape[1] / 2) * c + (xx - shape[2] / 2) * s
    v = -(yy - shape[1] / 2) * s + (xx - shape[2] / 2) * c
    return ((np.abs(u) < 14) & (np.abs(v) < 3) & (zz >= 1) & (zz <= 4)).astype(np.uint8)


def test_derive_and_compare_against_numpy_on_the_masks():
    spacing = (2.5, 0.7, 1.3)
    box = np.zeros((8, 30, 40), np.uint8)
    box[2:6, 5:17, 9:30] = 1
    slab = rotated_slab((6, 40, 44), 0.6)
    image = RC.image_for((8, 30, 40), 5)
    for mask, img in ((box, image), (slab, None)):
        rows_i, rows_f, _ = RC.restate(mask, img, lo=1, L=3)
        figs = R.derive(rows_i, None if img is None else rows_f, spacing)
        assert len(figs) == 3
        f = figs[1]
        pts = np.argwhere(mask == 1).astype(np.float64)
        assert f["voxels"] == len(pts) and f["volume_mm3"] == len(pts) * 2.5 * 0.7 * 1.3 and f["volume_ml"] == f["volume_mm3"] / 1000.0
        assert f["bbox"] == (tuple(int(v) for v in pts.min(0)), tuple(int(v) for v in pts.max(0)))
        assert np.allclose(f["centroid"], pts.mean(0), rtol=1e-14, atol=0) and np.allclose(f["centroid_mm"], pts.mean(0) * spacing, rtol=1e-14, atol=0)
        assert np.allclose(f["extent_mm"], (pts.max(0) - pts.min(0) + 1) * spacing, rtol=1e-14, atol=0)
        cov = np.cov((pts * spacing).T, bias=True)
        assert np.allclose(f["covariance_mm2"], cov, rtol=1e-11, atol=1e-11)
        assert np.allclose(f["axes_mm"], np.sqrt(np.linalg.eigvalsh(cov)), rtol=1e-9, atol=1e-9) and list(f["axes_mm"]) == sorted(f["axes_mm"])
        if img is None:
            assert all(f[k] is None for k in ("mean", "std", "min", "max", "n_nonfinite"))
        else:
            inside = img[mask == 1].astype(np.float64)
            assert f["n_nonfinite"] == 0 and math.isclose(f["mean"], inside.mean(), rel_tol=1e-12) and math.isclose(f["std"], inside.std(), rel_tol=1e-9)
            assert f["min"] == inside.min() and f["max"] == inside.max()
        # label 0 is skipped and label 2 absent: every figure that needs a voxel is None, the volume is 0
        for e in (figs[0], figs[2]):
            assert e["voxels"] == 0 and e["volume_mm3"] == 0.0 and all(e[k] is None for k in ("bbox", "centroid", "centroid_mm", "extent_mm",
                                                                                              "covariance_mm2", "axes_mm", "mean", "std", "min", "max"))
        bare = R.derive(rows_i)[1]
        assert bare["voxels"] == f["voxels"] and bare["centroid"] == f["centroid"] and all(
            bare[k] is None for k in ("volume_mm3", "volume_ml", "centroid_mm", "extent_mm", "covariance_mm2", "axes_mm", "mean", "n_nonfinite"))
    # the slab's long axis is the rotated one: the largest principal axis is far above the two others
    assert figs[1]["axes_mm"][2] > 2 * figs[1]["axes_mm"][1] > 0
    # a label whose image values are all non-finite
    img = np.full(box.shape, np.nan, np.float32)
    rows_i, rows_f, _ = RC.restate(box, img, lo=1, L=2)
    f = R.derive(rows_i, rows_f)[1]
    assert f["n_nonfinite"] == f["voxels"] and f["mean"] is None and f["std"] is None and f["min"] is None and f["max"] is None
    # compare
    other = np.zeros_like(box)
    other[3:7, 5:17, 10:34] = 1
    p, t = (R.derive(RC.restate(m, None, lo=1, L=2)[0], None, spacing)[1] for m in (other, box))
    c = R.compare(p, t)
    cp, ct = np.argwhere(other == 1).mean(0) * spacing, np.argwhere(box == 1).mean(0) * spacing
    assert c["unit"] == "mm" and math.isclose(c["rvd"], (other.sum() - box.sum()) / box.sum(), rel_tol=1e-15)
    assert math.isclose(c["centroid_distance"], float(np.linalg.norm(cp - ct)), rel_tol=1e-13)
    pv, tv = (R.derive(RC.restate(m, None, lo=1, L=2)[0])[1] for m in (other, box))
    cv = R.compare(pv, tv)
    assert cv["unit"] == "voxels" and math.isclose(cv["centroid_distance"], float(np.linalg.norm(cp / spacing - ct / spacing)), rel_tol=1e-13)
    empty = R.derive(RC.restate(np.zeros_like(box), None, lo=1, L=2)[0], None, spacing)[1]
    assert R.compare(p, empty) == {"rvd": None, "centroid_distance": None, "unit": "mm"}
    assert R.compare(empty, t)["rvd"] == -1.0 and R.compare(empty, t)["centroid_distance"] is None
    fig = R.region_figures(np.stack([RC.restate(other, None, 1, 2)[0], RC.restate(box, None, 1, 2)[0]]), np.zeros((2, 2, 2)), spacing)[0]
    assert fig["rvd"] == c["rvd"] and R.region_line_suffix(fig, True) == (
        f" vol {p['volume_ml']:.4f} ({t['volume_ml']:.4f}) ml rvd {c['rvd']:.4f} cdist {c['centroid_distance']:.4f} mm")
    fig = R.region_figures(np.stack([RC.restate(other, None, 1, 2)[0], RC.restate(box, None, 1, 2)[0]]), np.zeros((2, 2, 2)))[0]
    assert R.region_line_suffix(fig, False) == f" vol {int(other.sum())} ({int(box.sum())}) rvd {cv['rvd']:.4f} cdist {cv['centroid_distance']:.4f}"
    with pytest.raises(ValueError):
        R.derive(np.zeros((2, 19), np.int64))
    with pytest.raises(ValueError):
        R.derive(rows_i, np.zeros((3, 2)))
    with pytest.raises(ValueError):
        R.derive(rows_i, None, (1.0, 0.0, 1.0))


def test_workspace_formula_and_the_refusals_of_the_size_query():
    lib = hip.load()
    for D, H, W in ((1, 1, 1), (1, 17, 241), (3, 9, 13), (64, 256, 256), (5, 1024, 821), (1024, 1024, 1024)):
        for L in (1, 2, 5, 256):
            G = min(-(-D * H * W // 4096), 1024)
            (o_acc, o_part), size = R._workspace_layout(D, H, W, L)
            assert (o_acc, o_part, size) == (64, 64 + 160 * L, 64 + 160 * L + 16 * G * L) and size % 16 == 0
            assert lib.rpnet_region_workspace_bytes(D, H, W, L) == size
    for bad in ((0, 1, 1, 1), (1, 1025, 1, 1), (1, 1, -3, 1), (1, 1, 1, 0), (1, 1, 1, 257)):
        assert lib.rpnet_region_workspace_bytes(*bad) == 0
        assert lib.rpnet_last_error_string().decode() == "region_workspace_bytes: D=%d H=%d W=%d L=%d (every extent 1..1024, L 1..256)" % bad


def test_host_refusals_of_region_stats_on_cpu_tensors():
    labels = torch.zeros((3, 9, 13), dtype=torch.uint8)
    image = torch.zeros((3, 9, 13), dtype=torch.float32)
    ri, rf = torch.zeros((2, 4, 20), dtype=torch.int64), torch.zeros((2, 4, 2), dtype=torch.float64)
    bad = [dict(labels=labels.numpy()), dict(labels=labels.to(torch.int16)), dict(labels=labels[0]), dict(labels=labels.permute(2, 1, 0)),
           dict(labels=torch.zeros((1, 1, 1025), dtype=torch.uint8)), dict(labels=labels.to(torch.int32)),       # n_labels is needed
           dict(n_labels=0), dict(n_labels=257), dict(n_labels=True), dict(n_labels=2.0),
           dict(image=image.double()), dict(image=image[:2]), dict(image=image.numpy()), dict(image=image.permute(0, 2, 1)),
           dict(row=1), dict(row=0.0), dict(n_labels=4, out=(ri, rf), row=2), dict(n_labels=4, out=(ri, rf), row=-1),
           dict(n_labels=4, out=(ri,)), dict(n_labels=5, out=(ri, rf)), dict(n_labels=4, out=(ri.to(torch.int32), rf)),
           dict(n_labels=4, out=(ri, rf.float())), dict(n_labels=4, out=(ri, rf[:1])), dict(n_labels=4, out=(ri, None), image=image),
           dict(n_labels=4, out=(ri[:, :, :19], rf)), dict(workspace=torch.zeros(10, dtype=torch.uint8)),
           dict(workspace=torch.zeros(100000, dtype=torch.int32)), dict(workspace=torch.zeros((1000, 100), dtype=torch.uint8))]
    for over in bad:
        kw = dict(dict(labels=labels), **over)
        with pytest.raises(ValueError):
            R.region_stats(**kw)
    # everything in order: the one thing left to refuse is the CPU tensor itself
    for kw in (dict(), dict(image=image, n_labels=4, out=(ri, rf), row=1), dict(image=image.to(torch.int16), skip_background=False),
               dict(n_labels=4, out=(ri, None)), dict(labels=labels.float(), n_labels=1)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            R.region_stats(**dict(dict(labels=labels), **kw))
    with pytest.raises(ValueError):
        R.check_regions_out((ri, rf), 2)
    R.check_regions_out((ri[:, :2].contiguous(), rf[:, :2].contiguous()), 2)
