"""Host side of the device augmentation path (rpnet_amd/augment.py, rpnet_amd/episodes.py): the ABI exports, the
separation of the random draws from their application, and the loud failure off the GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from rpnet_amd import augment as A
from rpnet_amd import hip
from rpnet_amd.utils import volume_reader as VR
from tests import augment_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = [0, 1, 2, 3, 11, 4100, 4207]


def test_library_exports_augmentation_entry_points():
    """the new entry points are in the built library and the ABI number moved with them"""
    lib = ctypes.CDLL(hip.lib_path())
    for name in ("rpnet_slice_minmax", "rpnet_augment_affine", "rpnet_elastic_field", "rpnet_elastic_apply"):
        assert name in hip.ABI_SYMBOLS and hasattr(lib, name), name
    assert lib.rpnet_version() == 111 == hip.ABI_VERSION


@pytest.mark.parametrize("seed", SEEDS)
def test_draws_consume_the_generators_like_the_host_functions(seed):
    """host function under a seed == draw under the same seed + the host arithmetic, bit for bit, and the three
    generators end in the same state"""
    for H, W in [(64, 48), (40, 40)]:
        img, lab = AC.make_slice_rng(seed, H, W)

        AC.seed_all(seed)
        h_img, h_lab = VR.random_transform(img.clone(), lab.clone())
        st = AC.rng_state()
        AC.seed_all(seed)
        m = A.draw_random_affine(H, W, **A.TRANSFORM_ARGS)
        assert AC.rng_state() == st and len(m) == 6
        d_img, d_lab = VR.transform_apply(img.clone(), lab.clone(), m)
        assert torch.equal(h_img, d_img) and torch.equal(h_lab, d_lab)

        AC.seed_all(seed)
        h = VR.random_label_transform(lab[0].clone())
        st = AC.rng_state()
        AC.seed_all(seed)
        m = A.draw_random_affine(H, W, **A.LABEL_TRANSFORM_ARGS)
        assert AC.rng_state() == st
        assert torch.equal(h, VR.affine_sample(lab[0].clone()[None, None], m)[:, 0])

        AC.seed_all(seed)
        h = VR.gamma_transform(img[0].numpy().copy(), [0.5, 1.5])
        st = AC.rng_state()
        AC.seed_all(seed)
        g = A.draw_gamma([0.5, 1.5])
        assert AC.rng_state() == st and 0.5 <= g <= 1.5
        assert np.array_equal(h, VR.gamma_apply(img[0].numpy().copy(), g))

        vol = np.random.RandomState(seed + 9).rand(1, 3, H, W).astype(np.float32) * 2 - 1
        msk = (vol > 0.2).astype(np.float32)
        msk[:, 1] = 0
        AC.seed_all(seed)
        rs = np.random.RandomState(seed)
        h_img, h_msk = VR.elastic_transform_all(vol, msk, random_state=rs)
        st, rst = AC.rng_state(), rs.get_state()[1].tobytes()
        AC.seed_all(seed)
        rs = np.random.RandomState(seed)
        Minv, noise = A.draw_elastic((H, W), 0.04, rs)
        assert AC.rng_state() == st and rs.get_state()[1].tobytes() == rst
        assert Minv.shape == (2, 3) and noise.shape == (2, H, W) and noise.dtype == np.float64
        d_img, d_msk = VR.elastic_apply(vol, msk, Minv, noise)
        assert np.array_equal(h_img, d_img) and np.array_equal(h_msk, d_msk) and not d_msk[:, 1].any()


def test_gaussian_weights_are_scipy_s():
    """the blur weights handed to the kernel are gaussian_filter's: filtering a unit impulse returns them"""
    from scipy.ndimage import gaussian_filter
    for sigma in (30, 2.5, 1):
        w, r = A.gaussian_weights(sigma)
        assert r == int(4 * sigma + 0.5) and len(w) == 2 * r + 1
        imp = np.zeros(4 * r + 1)
        imp[2 * r] = 1.0
        assert np.array_equal(gaussian_filter(imp, sigma)[r:3 * r + 1], w)


def test_pack_params():
    t = A.pack_params([[1, 2, 3, 4, 5, 6], [6, 5, 4, 3, 2, 1]], [None, 0.75])
    assert t.dtype == torch.float32 and tuple(t.shape) == (2, A.N_PARAMS)
    assert t[0].tolist() == [1, 2, 3, 4, 5, 6, 0, 0] and t[1].tolist() == [6, 5, 4, 3, 2, 1, 0.75, 1]


def test_no_cpu_fallback():
    """CPU tensors raise, as everywhere in the package"""
    img, lab = AC.make_slice_rng(0, 16, 16)
    p = A.pack_params([[1, 0, 0, 0, 1, 0]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.augment_slices(img[0], lab, p)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.label_transform(lab, p)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.elastic_slices(img[0], lab, np.eye(3)[:2], np.zeros((2, 16, 16)))
    from rpnet_amd.episodes import DeviceEpisodeSource
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DeviceEpisodeSource("nowhere", "nothing.csv", {}, "cpu")


def test_train_driver_lists_the_data_options():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train_rpnet.py"), "--help"], capture_output=True, text=True, check=True).stdout
    assert "--data_dir" in out and "--set_name" in out
