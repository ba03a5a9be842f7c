"""Device augmentation and episode assembly (csrc/augment.hip, rpnet_amd/augment.py, rpnet_amd/episodes.py) against
the host functions of rpnet_amd/utils/volume_reader.py.  Nearest-neighbour results are compared exactly outside the
pixels whose source coordinate, recomputed here in fp64, lies within 1e-3 pixel of a rounding boundary; tolerances of
interpolated / power-law values are calibrated on the host by each test (factor 4 on the host's own fp32-vs-fp64 change)."""
import numpy as np
import pytest
import torch

from rpnet_amd import augment as A
from rpnet_amd.utils import volume_reader as VR
from tests import augment_cases as AC
from tests.reader_cases import config_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(256, 256), (64, 48)]
SEEDS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]            # gamma on for the even ones
ELASTIC_SEEDS = [0, 1, 2, 3]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check_nearest(got, src, cy, cx, cap, what, tol=0.0, post=None):
    """got[p] == src[round(cy, cx)] outside the band (zeros outside the plane), one of the candidates inside it"""
    band = AC.near_half(cy) | AC.near_half(cx)
    share = band.mean()
    print(f"{what}: excluded share {share:.4%}")
    assert share <= cap, (what, share)
    post = post or (lambda v: v)
    want = post(AC.gather(src, np.rint(cy).astype(np.int64), np.rint(cx).astype(np.int64)))
    diff = np.abs(got - want)
    assert diff[~band].max(initial=0.0) <= tol, (what, diff[~band].max(), tol)
    cands = np.stack([post(c) for c in AC.candidates(src, cy, cx)])
    assert (np.abs(cands - got[None]).min(axis=0)[band] <= tol).all(), what


@pytest.mark.parametrize("H,W", SIZES)
def test_gamma_affine_matches_host(H, W):
    """gamma_transform + random_transform and random_label_transform.  Measured on the MI355X: host calibration of the
    power law (fp32 against fp64 formula on these slices) 2.45e-7 at 256x256 / 2.26e-7 at 64x48, so the tolerance is
    9.8e-7 / 9.0e-7; the device image differs from the host functions by at most 1.8e-7 / 1.2e-7 outside the band; the
    excluded share is 0.2 - 0.6 % of a slice (cap 1 %); labels equal outside it."""
    imgs, labs, hosts, lparams, hl = [], [], [], [], []
    gam, aff = [], []
    for s in SEEDS:
        img, lab = AC.make_slice(s, H, W)
        on = s % 2 == 0
        AC.seed_all(s)
        q = VR.gamma_transform(img[None], [0.5, 1.5])[0] if on else img
        hi, hlab = VR.random_transform(torch.from_numpy(q.copy())[None, None], torch.from_numpy(lab)[None])
        hl.append(VR.random_label_transform(torch.from_numpy(lab))[0].numpy())
        st = AC.rng_state()
        AC.seed_all(s)
        gam.append(A.draw_gamma([0.5, 1.5]) if on else None)
        aff.append(A.draw_random_affine(H, W, **A.TRANSFORM_ARGS))
        lparams.append(A.draw_random_affine(H, W, **A.LABEL_TRANSFORM_ARGS))
        assert AC.rng_state() == st
        imgs.append(img), labs.append(lab), hosts.append((hi[0, 0].numpy(), hlab[0].numpy()))
    calib = max(np.abs(AC.intensity_formula(i, g, np.float32).astype(np.float64) - AC.intensity_formula(i, g, np.float64)).max()
                for i, g in zip(imgs, gam))
    tol = 4 * calib
    print(f"power-law calibration (fp32 vs fp64 host formula) {calib:.3e} -> tolerance {tol:.3e}")
    assert 0 < tol < 1e-4

    d_img, d_lab = A.augment_slices(_dev(np.stack(imgs)), _dev(np.stack(labs)), A.pack_params(aff, gam))
    d_l2 = A.label_transform(_dev(np.stack(labs)), A.pack_params(lparams))
    d_img, d_lab, d_l2 = d_img.cpu().numpy(), d_lab.cpu().numpy(), d_l2.cpu().numpy()
    worst = 0.0
    for i, s in enumerate(SEEDS):
        cy, cx = AC.affine_source(aff[i], H, W)
        _check_nearest(d_lab[i], labs[i], cy, cx, 0.01, f"label seed {s}")
        ly, lx = AC.affine_source(lparams[i], H, W)
        _check_nearest(d_l2[i], labs[i], ly, lx, 0.01, f"label-only seed {s}")
        lband = AC.near_half(ly) | AC.near_half(lx)
        assert np.array_equal(hl[i][~lband], d_l2[i][~lband])
        assert np.array_equal(np.where(AC.near_half(cy) | AC.near_half(cx), 0, hosts[i][1]),
                              np.where(AC.near_half(cy) | AC.near_half(cx), 0, d_lab[i]))
        # image: the host's own pre-sampling [0,1] image, sampled; zeros take its minimum
        u = (AC.intensity_formula(imgs[i], gam[i], np.float32) + 1) / 2
        lo = u.min()
        post = lambda v: np.where(v == 0, lo, v) * 2 - 1  # noqa: E731
        _check_nearest(d_img[i], u, cy, cx, 0.01, f"image seed {s}", tol=tol, post=post)
        band = AC.near_half(cy) | AC.near_half(cx)
        err = np.abs(d_img[i] - hosts[i][0])[~band].max()
        worst = max(worst, err)
        assert err <= tol, (s, err, tol)
    print(f"image against the host functions outside the band: max |diff| {worst:.3e} (tolerance {tol:.3e})")


@pytest.mark.parametrize("H,W", SIZES)
def test_elastic_field_matches_scipy(H, W):
    """alpha * gaussian_filter(noise, 30), fp64 sums, stored fp32; (64, 48) is smaller than the radius of 120.  Tolerance:
    4 x scipy's own change when the noise is rounded to fp32.  Measured on the MI355X: tolerance 1.4e-6 - 3.2e-6 over the
    seeds and sizes, largest difference 9.5e-7 (the fp32 rounding of a field value of magnitude 16 - 32; the fp64 sums
    themselves agree to 1e-12)."""
    from scipy.ndimage import gaussian_filter
    for s in ELASTIC_SEEDS:
        _, noise = A.draw_elastic((H, W), 0.04, np.random.RandomState(s))
        want = np.stack([gaussian_filter(noise[c], 30) * 1000 for c in range(2)])
        lossy = np.stack([gaussian_filter(noise[c].astype(np.float32).astype(np.float64), 30) * 1000 for c in range(2)])
        tol = 4 * np.abs(want - lossy).max()
        got = A.elastic_field(_dev(noise), 1000, 30).cpu().numpy()
        assert got.dtype == np.float32
        err = np.abs(got.astype(np.float64) - want).max()
        print(f"field {H}x{W} seed {s}: max |diff| {err:.3e}, calibration tolerance {tol:.3e}, max |field| {np.abs(want).max():.2f}")
        assert err <= tol, (s, err, tol)


@pytest.mark.parametrize("H,W", SIZES)
def test_elastic_slices_match_host(H, W):
    """elastic_transform_all on three slices (the middle mask empty).  Image tolerance: 4 x the host's own change under
    fp32 sampling coordinates; mask exact outside the two-stage rounding band (at most 2 % of a slice).  Measured on the
    MI355X: image within 7.2e-7 (tolerance 3.2e-5 - 4.3e-5 at 256x256, 4.9e-6 - 8.3e-6 at 64x48); mask band 0.20 - 0.59 %
    of a slice, no mismatch inside it either for these seeds."""
    for s in ELASTIC_SEEDS:
        pairs = [AC.make_slice(100 + 3 * s + j, H, W) for j in range(3)]
        image = np.stack([p[0] for p in pairs])
        mask = np.stack([p[1] for p in pairs])
        mask[1] = 0
        rs = np.random.RandomState(s)
        h_img, h_msk = VR.elastic_transform_all(image[None], mask[None], random_state=rs)
        Minv, noise = A.draw_elastic((H, W), 0.04, np.random.RandomState(s))
        tol = 4 * np.abs(AC.elastic_image_fp32_coords(image, Minv, noise) - h_img[0]).max()
        d_img, d_msk = A.elastic_slices(_dev(image), _dev(mask), Minv, noise)
        d_img, d_msk = d_img.cpu().numpy(), d_msk.cpu().numpy()
        err = np.abs(d_img - h_img[0]).max()
        band = AC.elastic_mask_band(Minv, noise, 1000, 30, H, W)
        print(f"elastic {H}x{W} seed {s}: image max |diff| {err:.3e} (tolerance {tol:.3e}); mask band {band.mean():.4%}, "
              f"mismatches inside it {(d_msk != h_msk[0])[:, band].sum()}")
        assert tol > 0 and err <= tol, (s, err, tol)
        assert band.mean() <= 0.02, band.mean()
        assert np.array_equal(d_msk[:, ~band], h_msk[0][:, ~band])
        assert set(np.unique(d_msk).tolist()) <= {0.0, 1.0} and not d_msk[1].any() and d_msk[0].any()


# ------------------------------------------------------------------------------------------------------------ episodes
CASE = {"data": dict(n_volumes=3, classes=("Liver",), shape=(22, 72, 72), seed=11),
        "cfg": dict(num_slice=20, num_x=72, num_y=72, crop_size=[64, 64], k=4)}


def _dataset(tmp_path, **over):
    data_dir, set_name, csv_dir = VR.write_synthetic_dataset(str(tmp_path), **CASE["data"])
    return data_dir, set_name, dict(config_for(CASE, csv_dir), **over)


@pytest.mark.parametrize("elastic", [False, True])
def test_device_item_matches_host_reader(tmp_path, monkeypatch, elastic):
    """DeviceEpisodeSource.item against FewshotRegReader(mode="train") under equal seeds.  Without the elastic transform the
    pre-registration pixels follow the rules of test_gamma_affine_matches_host; with it (both sides given the same seeded
    RandomState for the field) the excluded set is the composition of the two: the affine sampling's band, or a source
    pixel in the elastic transform's mask band (cap 1 % + 2 %); labels are equal outside it; the image, outside the affine
    band, is within 4 x (the power law's fp32-vs-fp64 calibration + the host's own change when its elastic image is made
    with fp32 coordinates and fed through the same gamma and affine steps).  Measured on the MI355X: composed band
    0.2 - 1.15 % of a slice; image within 4.8e-7 against tolerances of 5.1e-6 - 6.8e-6 with the elastic transform,
    within 1.2e-7 against 2.7e-7 - 4.1e-7 without (0 against 0 where gamma is off)."""
    from rpnet_amd.episodes import DeviceEpisodeSource
    from rpnet_amd.registration import get_registration_field
    data_dir, set_name, cfg = _dataset(tmp_path, do_elastic=elastic)
    host_el = VR.elastic_transform_all
    seeds = [21, 22, 23, 24, 25, 26]
    coins = 0
    for idx, s in enumerate(seeds):
        idx %= 3
        monkeypatch.setattr(VR, "elastic_transform_all", lambda i, m: host_el(i, m, random_state=np.random.RandomState(s)))
        AC.seed_all(s)
        hrd = VR.FewshotRegReader(data_dir, set_name, cfg, mode="train")
        h = hrd[idx]
        h_state = AC.rng_state()
        src = DeviceEpisodeSource(data_dir, set_name, cfg, DEV, elastic_random_state=np.random.RandomState(s))
        src.warm()
        AC.seed_all(s)
        d = src.item(idx)
        assert AC.rng_state() == h_state
        pre = src.pre
        k = cfg["k"]
        assert d["pid"] == h["pid"] and d["supp_pids"] == h["supp_pids"] and d["class_id"] == h["class_id"]
        h_pre = {"support_images": h["original_support_images"][0][0][:, [0]], "support_labels": h["original_support_labels"][0][0],
                 "query_images": h["query_images"], "query_labels": h["query_labels"]}
        for key, hv in h_pre.items():
            assert tuple(pre[key].shape) == tuple(hv.shape) and pre[key].dtype == hv.dtype == torch.float32, key
        for key in ("support_images", "support_labels", "query_images", "query_labels", "appr_query_labels"):
            hv = h[key][0][0] if key.startswith("support") else h[key]
            assert tuple(d[key].shape) == tuple(hv.shape) and d[key].dtype == hv.dtype and d[key].is_cuda, key
        # the support side is not augmented: slice picks and shuffle order, bit for bit
        assert torch.equal(pre["support_images"].cpu(), h_pre["support_images"])
        assert torch.equal(pre["support_labels"].cpu(), h_pre["support_labels"])
        q_i, q_l = pre["query_images"][:, 0].cpu().numpy(), pre["query_labels"].cpu().numpy()
        hq_i, hq_l = h_pre["query_images"][:, 0].numpy(), h_pre["query_labels"].numpy()
        coin = src.last_elastic is not None
        coins += coin
        q_raw, q_msk = [t.cpu().numpy() for t in src.volume(d["class_id"], src.reader.indices[idx][1])]
        for j in range(k):
            o = pre["order"][j]
            m, gam, z = pre["affines"][o], pre["gammas"][o], pre["slices"][o]
            # the host path of this slice restated from the source's own draws: it IS the host item, bit for bit
            a_i, a_l = AC.host_query_slice(q_raw[z], q_msk[z], src.last_elastic, gam, m)
            assert np.array_equal(a_i, hq_i[j]) and np.array_equal(a_l, hq_l[j]), (s, j)
            cy, cx = AC.affine_source(m, 64, 64)
            aband = AC.near_half(cy) | AC.near_half(cx)
            band = AC.composed_band(m, src.last_elastic, 64, 64)
            assert aband.mean() <= 0.01 and band.mean() <= (0.03 if coin else 0.01), (s, j, aband.mean(), band.mean())
            assert np.array_equal(q_l[j][~band], hq_l[j][~band]), (s, j)
            # image: the power law's calibration on the slice it is given, plus (elastic) the host's own change when the
            # elastic image is made with fp32 sampling coordinates and fed through the same gamma and affine steps
            given = q_raw[z] if not coin else VR.elastic_apply(q_raw[z][None, None], q_msk[z][None, None], *src.last_elastic)[0][0, 0]
            calib = np.abs(AC.intensity_formula(given, gam, np.float32).astype(np.float64) - AC.intensity_formula(given, gam, np.float64)).max()
            if coin:
                calib += np.abs(AC.host_query_slice(q_raw[z], q_msk[z], src.last_elastic, gam, m, fp32_coords=True)[0] - a_i).max()
            err = np.abs(q_i[j] - hq_i[j])[~aband].max()
            print(f"seed {s} slice {j} elastic {coin}: band {band.mean():.3%}, image max |diff| {err:.3e}, tolerance {4 * calib:.3e}")
            assert err <= 4 * calib, (s, j, err, calib)
        # after registration: the same launches as get_registration_field on the source's own pre-registration tensors
        field, reg, _, aff_pred, aff_src = get_registration_field(pre["query_images"].cpu(), [[pre["support_images"].cpu()]],
                                                                  [[pre["support_labels"].cpu()]], do_deformable=cfg["do_deformable"])
        assert torch.equal(d["registration_field"].cpu(), field)
        assert np.array_equal(d["support_images"][:, 0].cpu().numpy(), aff_src)
        assert torch.equal(d["support_labels"].cpu(), aff_pred[:, 0])
        assert torch.equal(d["appr_query_labels"].cpu(), (reg[:, 0] > 0.5).float())
        assert torch.equal(d["query_images"], pre["query_images"]) and torch.equal(d["query_labels"], pre["query_labels"])
    assert (coins > 0) == elastic, "the seeds must exercise the elastic coin"


def test_item_makes_no_host_synchronisation(tmp_path):
    """after warm-up an item copies nothing back: checked with torch.cuda.set_sync_debug_mode("error") around the call
    (every synchronising torch call — .cpu(), .item(), a blocking copy — raises under it)"""
    from rpnet_amd.episodes import DeviceEpisodeSource
    for deformable in (False, True):
        data_dir, set_name, cfg = _dataset(tmp_path, do_deformable=deformable)
        src = DeviceEpisodeSource(data_dir, set_name, cfg, DEV)
        src.warm()
        AC.seed_all(3)
        for idx in range(len(src)):
            src.item(idx)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for idx in range(len(src)):
                src.item(idx)
            src.batch(8)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()


def test_batches_carry_over_and_train(tmp_path):
    """batch(8) from items of k = 4 pairs ... and of k = 3 (remainder carried); train_rpnet.train runs 20 steps on the
    source as test_training_driver_learns_and_checkpoints does on synthetic episodes (without that test's margin of 0.05,
    which was set for make_episode data)."""
    from rpnet_amd.episodes import DeviceEpisodeSource
    from tests.helpers import load_cfg
    from train_rpnet import train
    data_dir, set_name, cfg = _dataset(tmp_path, k=3)
    AC.seed_all(0)
    src = DeviceEpisodeSource(data_dir, set_name, cfg, DEV)
    si, fg, bg, qi, ql, appr = src.batch(8)
    assert tuple(si[0][0].shape) == (8, 1, 64, 64) == tuple(qi[0].shape) and tuple(fg[0][0].shape) == (8, 64, 64) == tuple(ql.shape)
    assert ql.dtype == torch.int64 and appr.dtype == torch.float32 and tuple(appr.shape) == (8, 64, 64)
    assert torch.equal(bg[0][0], 1 - fg[0][0]) and set(np.unique(fg[0][0].cpu().numpy()).tolist()) <= {0.0, 1.0}
    assert src._carry is not None and src._carry[0].shape[0] == 1 and src._next == 0       # three items of 3 pairs: one left
    held = src._carry[2].clone()
    nxt = src.batch(8)
    assert torch.equal(nxt[3][0][:1], held) and src._carry[0].shape[0] == 2
    # the second of two data-parallel processes starts at item 1 and strides by 2: items 1, 0, 2 where rank 0 takes 0, 2, 1
    AC.seed_all(0)
    r1 = DeviceEpisodeSource(data_dir, set_name, cfg, DEV, rank=1, world=2)
    assert r1._next == 1
    r1.batch(3)
    assert r1._next == 0 and r1._carry is None

    model_cfg = dict(load_cfg(2), **cfg)
    torch.manual_seed(0)
    AC.seed_all(0)
    src = DeviceEpisodeSource(data_dir, set_name, dict(cfg, k=4), DEV)
    _, hist = train(model_cfg, steps=20, batch=8, size=64, dev=torch.device(DEV), lr=1e-3, log_every=0, source=src)
    print("loss history", [round(v, 4) for v in hist])
    assert len(hist) == 20 and all(np.isfinite(hist))
    assert np.mean(hist[-6:]) < np.mean(hist[:6]), hist
