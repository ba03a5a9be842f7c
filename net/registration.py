"""The two `net.registration` symbols test_rpnet.py imports (test_rpnet.py:32,229-230): image
similarity metrics printed next to the Dice scores; and the DEEDS stage of the reference file under its own class names
(net/registration.py:360-381,412-471,505-518), built on the batched HIP entry points of rpnet_amd.registration (GPU tensors
only, no CPU fallback).  The affine and Demons optimisers of the reference file (net/registration.py:100-357,474-502) are reached
through rpnet_amd.registration.register_slices, not through classes of their own here."""
import torch


def MSE(y_pred, y_true, mask=None):
    """mean squared error (reference net/registration.py:147-154)."""
    value = torch.mean((y_true - y_pred) ** 2)
    if mask is not None:
        value = torch.masked_select(value, mask).mean()
    return value


def NCC(moving_image_valid, fixed_image_valid, mask=None):
    """negative normalised cross-correlation (reference net/registration.py:157-160)."""
    f = fixed_image_valid - torch.mean(fixed_image_valid)
    m = moving_image_valid - torch.mean(moving_image_valid)
    return -1.0 * torch.sum(f * m) / torch.sqrt(torch.sum(f ** 2) * torch.sum(m ** 2) + 1e-10)


class DEEDSRegistration(torch.nn.Module):
    """reference net/registration.py:360-381,412-471: train_registraion(moving, fixed) [N,1,H,W] on the GPU builds the
    sampling grid in one pass (rpnet_amd.registration.deeds_register), forward(img) warps by it (deeds_warp)."""

    def __init__(self, grid_size=128, disp_range=0.1, displacement_width=15, use_GPU=False, mode='nearest'):
        super().__init__()
        from rpnet_amd.registration import DEEDS_ALPHA
        self.grid_size = grid_size
        self.disp_range = disp_range
        self.displacement_width = displacement_width
        self.pred_xyz = None
        self.alpha = torch.nn.Parameter(torch.tensor(DEEDS_ALPHA, dtype=torch.float32))
        self.mode = mode

    def train_registraion(self, moving, fixed, verbose=False):
        from rpnet_amd.registration import deeds_register
        self.pred_xyz = deeds_register(moving[:, 0].float(), fixed[:, 0].float(), self.grid_size, self.disp_range,
                                       self.displacement_width, self.alpha.detach().tolist())

    def forward(self, img):
        from rpnet_amd.registration import deeds_warp
        assert self.pred_xyz is not None
        return deeds_warp(img[:, 0].float(), self.pred_xyz, mode=self.mode)[:, None]


class AffineDEEDSRegistration(torch.nn.Module):
    """reference net/registration.py:505-518: the affine stage, then DEEDS on the affine-warped image.  theta [N,2,3] is
    rpnet_amd.registration.affine_register's (50 Adam steps, as the reader runs it)."""

    def __init__(self, img_size, use_diffeomorphic=False, use_GPU=False, stop_shear=False):
        super().__init__()
        if stop_shear:
            raise NotImplementedError("AffineDEEDSRegistration: stop_shear (the reader never sets it)")
        self.img_size = img_size
        self.deeds = DEEDSRegistration()
        self.theta = None
        self.use_GPU = use_GPU
        self.stop_shear = stop_shear

    def train_registraion(self, moving, fixed, iters=50, verbose=False):
        from rpnet_amd.registration import affine_register, affine_warp
        self.theta, _ = affine_register(moving[:, 0].float(), fixed[:, 0].float(), iters)
        self.deeds.train_registraion(affine_warp(moving[:, 0].float(), self.theta)[:, None], fixed)

    def forward(self, x, grid=None):
        from rpnet_amd.registration import affine_warp
        assert self.theta is not None
        return self.deeds(affine_warp(x[:, 0].float(), self.theta)[:, None])
