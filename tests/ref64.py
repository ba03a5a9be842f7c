"""Plain float64 references of the small operations around the convolutions (matcher, loss, pooling), one function per
operation: stock torch operators on the CPU, restated from the reference's operator sequence (net/rp_net.py, net/unet.py,
net/vgg.py), every backward through autograd.  Test infrastructure only: nothing here imports the package under test, and
nothing is built from oracle/rpnet_oracle.py (tests/test_host_ref64.py compares the two).

Layouts are the kernels' own: feature maps NHWC ([B, h, w, C] or [B, hw, C]), logits / predictions NCHW, masks
[nmask, B, H, W].  Every function takes `dtype`: float64 is the reference, float32 the yardstick — the same operators at the
kernels' precision, whose distance from the float64 result says what fp32 round-off costs on these inputs."""
import math

import torch
import torch.nn.functional as F

F64 = torch.float64


def _c(t, dtype):
    return None if t is None else torch.as_tensor(t).detach().cpu().to(dtype)


def _nchw(f, h, w):
    """[B, h*w, C] or [B, h, w, C] -> [B, C, h, w]"""
    B, C = f.shape[0], f.shape[-1]
    return f.reshape(B, h, w, C).permute(0, 3, 1, 2)


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------- cosine match (calDist, net/rp_net.py:353-363)
def _cosine(f, proto, scaler):
    # f [B, hw, C], proto [B, K, C]: cosine_similarity over the channel axis of [B, 1, C, hw] against [B, K, C, 1]
    return F.cosine_similarity(f.transpose(1, 2)[:, None], proto[..., None], dim=2, eps=1e-8) * scaler


def cosine_match(f, proto, scaler=20.0, dtype=F64):
    """f [B, hw, C], proto [B, K, C] -> pred [B, K, hw]"""
    return _cosine(_c(f, dtype), _c(proto, dtype), scaler)


def cosine_match_bwd(f, proto, dpred, scaler=20.0, dtype=F64):
    """-> (df [B, hw, C], dproto [B, K, C])"""
    f, proto = _c(f, dtype).requires_grad_(True), _c(proto, dtype).requires_grad_(True)
    return torch.autograd.grad(_cosine(f, proto, scaler), (f, proto), _c(dpred, dtype))


# ---------------------------------------------------------------------- bilinear (F.interpolate, net/rp_net.py:303,337)
def bilinear_up(x, H, W, dtype=F64):
    """x [planes, h, w] -> [planes, H, W]"""
    return F.interpolate(_c(x, dtype)[None], size=(H, W), mode="bilinear")[0]


def bilinear_up_bwd(dout, h, w, dtype=F64):
    """dout [planes, H, W] -> din [planes, h, w]"""
    dout = _c(dout, dtype)
    x = torch.zeros(dout.shape[0], h, w, dtype=dtype, requires_grad=True)
    (g,) = torch.autograd.grad(F.interpolate(x[None], size=dout.shape[-2:], mode="bilinear")[0], x, dout)
    return g


# --------------------------------------------------------------- masked pooling (getFeatures, net/rp_net.py:366-376)
def mask_adjoint(masks, h, w, dtype=F64):
    """masks [nmask, B, H, W] -> (am [B, nmask, h*w] = U^T mask, msum [B, nmask]); U^T through autograd of the up-sampler"""
    m = _c(masks, dtype)
    nmask, B, H, W = m.shape
    x = torch.zeros(nmask * B, h, w, dtype=dtype, requires_grad=True)
    (am,) = torch.autograd.grad(F.interpolate(x[None], size=(H, W), mode="bilinear")[0], x, m.reshape(nmask * B, H, W))
    return am.reshape(nmask, B, h * w).transpose(0, 1).contiguous(), m.sum(dim=(2, 3)).t().contiguous()


def _masked_pool(f, m, h, w):
    up = F.interpolate(_nchw(f, h, w), size=m.shape[-2:], mode="bilinear")          # [B, C, H, W]
    rows = [torch.sum(up * m[k][:, None], dim=(2, 3)) / (m[k][:, None].sum(dim=(2, 3)) + 1e-5) for k in range(m.shape[0])]
    return torch.stack(rows, 1)                                                     # [B, nmask, C]


def masked_pool(f, masks, h, w, dtype=F64):
    """the as-written form: interpolate the features up, multiply, sum, divide.  f [B, h*w, C] -> proto [B, nmask, C]"""
    return _masked_pool(_c(f, dtype), _c(masks, dtype), h, w)


def masked_pool_bwd(f, masks, h, w, dproto, dtype=F64):
    """-> df [B, h*w, C]"""
    f = _c(f, dtype).requires_grad_(True)
    (g,) = torch.autograd.grad(_masked_pool(f, _c(masks, dtype), h, w), f, _c(dproto, dtype))
    return g


# -------------------------------------------------- softmax / threshold / pool (net/rp_net.py:269-272,308-311)
def _softmax_pool(logits, scale, soft):
    p1 = torch.softmax(logits, dim=1)[:, 1]
    if not soft:
        p1 = (p1 > 0.5).to(logits.dtype)
    return F.avg_pool2d(p1[:, None], scale)[:, 0]


def softmax_thresh_pool(logits, scale, soft, dtype=F64):
    """logits [B, K, H, W] -> mask [B, H/scale, W/scale]"""
    return _softmax_pool(_c(logits, dtype), scale, soft)


def softmax_pool_bwd(logits, dmask, scale, dtype=F64):
    logits = _c(logits, dtype).requires_grad_(True)
    (g,) = torch.autograd.grad(_softmax_pool(logits, scale, True), logits, _c(dmask, dtype))
    return g


def mask_avgpool(mask, scale, dtype=F64):
    """[B, H, W] -> [B, H/scale, W/scale]"""
    return F.avg_pool2d(_c(mask, dtype)[:, None], scale)[:, 0]


# ----------------------------------------------------------------------------- loss (net/rp_net.py:87-127,438,349)
def dice_loss_softmax(logits, true, eps=1e-7):
    """the num_classes > 1 branch of the reference's dice_loss_softmax"""
    K = logits.shape[1]
    one_hot = torch.eye(K, dtype=logits.dtype)[true].permute(0, 3, 1, 2)
    probas = torch.softmax(logits, dim=1)
    dims = (0, 2, 3)
    inter = torch.sum(probas * one_hot, dims)
    card = torch.sum(probas + one_hot, dims)
    return 1 - (2.0 * inter / (card + eps)).mean()


def _dice_ce(logits, labels, with_dice, ignore_index, per_sample, sample_weight):
    B = logits.shape[0]
    ign = ignore_index if ignore_index >= 0 else -100
    if per_sample:
        # alignLoss calls F.cross_entropy(ignore_index=255) once per episode (:438), the caller adds the episodes up and
        # divides by their number (:343,349); an episode whose predicted foreground is empty is skipped (:414,421)
        loss = 0
        for b in range(B):
            wb = 1.0 if sample_weight is None else float(sample_weight[b])
            if wb != 0.0:
                loss = loss + wb * F.cross_entropy(logits[[b]], labels[[b]], ignore_index=ign)
        loss = loss / B
    else:
        loss = F.cross_entropy(logits, labels, ignore_index=ign)
    if with_dice:
        loss = loss + dice_loss_softmax(logits, labels)
    return loss


def dice_ce(logits, labels, with_dice=1, ignore_index=-1, per_sample=0, sample_weight=None, dtype=F64):
    """logits [B, K, H, W], labels int64 [B, H, W] -> scalar"""
    return _dice_ce(_c(logits, dtype), torch.as_tensor(labels).cpu(), with_dice, ignore_index, per_sample,
                    None if sample_weight is None else _c(sample_weight, dtype)).detach()


def dice_ce_bwd(logits, labels, gscale=1.0, with_dice=1, ignore_index=-1, per_sample=0, sample_weight=None, dtype=F64):
    """-> gscale * d loss / d logits"""
    logits = _c(logits, dtype).requires_grad_(True)
    loss = _dice_ce(logits, torch.as_tensor(labels).cpu(), with_dice, ignore_index, per_sample,
                    None if sample_weight is None else _c(sample_weight, dtype))
    (g,) = torch.autograd.grad(loss, logits, torch.tensor(gscale, dtype=dtype))
    return g


# ------------------------------------------------------------------- alignLoss pieces (net/rp_net.py:412-417,433-436)
def argmax_masks(pred, dtype=F64):
    """pred [B, K, hw] -> (masks [B, K, hw] of 0 / 1, counts [B, K], keep [K, B])"""
    pred = _c(pred, dtype)
    am = pred.argmax(dim=1, keepdim=True)
    masks = torch.cat([am == i for i in range(pred.shape[1])], dim=1).to(dtype)
    counts = masks.sum(-1)
    return masks, counts, (counts > 0).to(dtype).t().contiguous()


def align_labels(fore, back):
    lab = torch.full_like(torch.as_tensor(fore).cpu(), 255).long()
    lab[torch.as_tensor(fore).cpu() == 1] = 1
    lab[torch.as_tensor(back).cpu() == 1] = 0
    return lab


# --------------------------------------------------------------- pooling (net/unet.py:397, net/modules.py:66, net/vgg.py)
def maxpool2(z, dtype=F64):
    """z [N, H, W, C] -> [N, H/2, W/2, C]"""
    return _nhwc(F.max_pool2d(_c(z, dtype).permute(0, 3, 1, 2), 2, 2))


def maxpool2_bwd(z, dpool, skip=None, dtype=F64):
    x = _c(z, dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    (g,) = torch.autograd.grad(F.max_pool2d(x, 2, 2), x, _c(dpool, dtype).permute(0, 3, 1, 2))
    g = _nhwc(g)
    return g if skip is None else g + _c(skip, dtype)


def upsample2_bwd(dyu, dtype=F64):
    """dyu [N, H, W, C] -> dx [N, H/2, W/2, C]: autograd of nn.Upsample(scale_factor=2) (nearest)"""
    dyu = _c(dyu, dtype).permute(0, 3, 1, 2)
    N, C, H, W = dyu.shape
    x = torch.zeros(N, C, H // 2, W // 2, dtype=dtype, requires_grad=True)
    (g,) = torch.autograd.grad(F.interpolate(x, scale_factor=2), x, dyu)
    return _nhwc(g)


def maxpool3(z, stride, dtype=F64):
    return _nhwc(F.max_pool2d(_c(z, dtype).permute(0, 3, 1, 2), 3, stride, 1))


def maxpool3_bwd(z, dpool, stride, dtype=F64):
    x = _c(z, dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    (g,) = torch.autograd.grad(F.max_pool2d(x, 3, stride, 1), x, _c(dpool, dtype).permute(0, 3, 1, 2))
    return _nhwc(g)


def bias_relu_bwd(dz, z=None, dtype=F64):
    """conv + bias (+ ReLU) backward given the OUTPUT z [P, C] (z = relu(a) and [z > 0] = [a > 0]): -> (dy [P, C], db [C])"""
    dz = _c(dz, dtype)
    a = (torch.zeros_like(dz) if z is None else _c(z, dtype)).requires_grad_(True)
    b = torch.zeros(dz.shape[1], dtype=dtype, requires_grad=True)
    out = a + b[None]
    if z is not None:
        out = torch.relu(out)
    return torch.autograd.grad(out, (a, b), dz)


# --------------------------------------------------------- soft-mask gradient (x * mask, x * (1 - mask); net/rp_net.py:283)
def rowdot_scale(g, x, s, mode, dtype=F64):
    """g, x [P, C], s [P] -> (dx [P, C], ds [P]) of y = x * s (mode 1) or x * (1 - s) (mode 2)"""
    x, s = _c(x, dtype).requires_grad_(True), _c(s, dtype).requires_grad_(True)
    y = x * (s if mode == 1 else 1 - s)[:, None]
    return torch.autograd.grad(y, (x, s), _c(g, dtype))


# ------------------------------------------------ fp16 tensor scale of a train-mode BatchNorm + ReLU output (include/rpnet_abi.h)
def bn_act_bound(gamma, beta, n, dtype=F64):
    """max_c |gamma_c| sqrt(n) + |beta_c|: |xhat| <= sqrt(n) for any batch of n values per channel"""
    return (_c(gamma, dtype).abs() * float(n) ** 0.5 + _c(beta, dtype).abs()).max()


# ------------------------------------------------- local-window correlation (Correlation(), net/rp_net.py:153-181), NHWC
def _local_corr(f1, f2, r, cstride=None):
    # f2 padded by r with zeros, one shifted product per offset: a (horizontal) is the major index of the window channel
    B, h, w, C = f1.shape
    K = 2 * r + 1
    f2p = F.pad(f2, (0, 0, r, r, r, r))
    cols = [(f1 * f2p[:, c:c + h, a:a + w]).sum(-1) for a in range(K) for c in range(K)]
    out = torch.stack(cols, -1) / math.sqrt(C)
    return out if cstride is None or cstride == K * K else F.pad(out, (0, cstride - K * K))


def local_corr(f1, f2, r, cstride=None, dtype=F64):
    """f1, f2 [B, h, w, C] -> corr [B, h, w, cstride or KK]:
    corr[b,y,x, a*K + c] = <f1[b,y,x,:], f2[b, y+c-r, x+a-r, :]> / sqrt(C), zero outside the image and in the pad channels"""
    return _local_corr(_c(f1, dtype), _c(f2, dtype), r, cstride)


def local_corr_bwd(f1, f2, dcorr, r, df1_add=None, dtype=F64):
    """dcorr [B, h, w, >= KK] (channels at or beyond KK are ignored) -> (df1 (+ df1_add), df2)"""
    f1, f2 = _c(f1, dtype).requires_grad_(True), _c(f2, dtype).requires_grad_(True)
    KK = (2 * r + 1) ** 2
    g1, g2 = torch.autograd.grad(_local_corr(f1, f2, r), (f1, f2), _c(dcorr, dtype)[..., :KK])
    return (g1 if df1_add is None else g1 + _c(df1_add, dtype)), g2


# ---------------------------------------- convolution weight gradient (autograd of nn.Conv2d wrt weight, include/rpnet_abi.h), NHWC
def conv_wgrad(x0, x1, dy, taps=9, dilation=1, upsample=0, in_scale=None, in_scale_mode=0, dtype=F64):
    """dW[cout][cin][kh][kw] = sum over pixels p of A[p + tap][cin] * dy[p][cout], written as that sum: nine shifted slices of the
    zero-padded input and one einsum each (no torch.nn.grad, no autograd).  A is gathered as the forward gathers it: the sources
    x0 | x1 [N, h, w, C0 | C1] concatenated along C (x1 None: one source), times in_scale [N, h, w] (mode 1) or 1 - in_scale
    (mode 2) per SOURCE pixel, then nearest x2 up-sampled (upsample = 1).  dy [N, H, W, cout]; taps 9 (3 x 3, tap spacing
    max(dilation, 1), zero padding of the same width) or 1 (dW [cout][cin][1][1])."""
    x = _c(x0, dtype) if x1 is None else torch.cat([_c(x0, dtype), _c(x1, dtype)], -1)
    dy = _c(dy, dtype)
    if in_scale_mode:
        s = _c(in_scale, dtype).reshape(x.shape[:3])[..., None]
        x = x * (s if in_scale_mode == 1 else 1 - s)
    if upsample:
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    N, H, W, _ = dy.shape
    assert x.shape[:3] == dy.shape[:3]
    if taps == 1:
        return torch.einsum("nhwi,nhwo->oi", x, dy)[..., None, None]
    d = max(int(dilation), 1)
    xp = F.pad(x, (0, 0, d, d, d, d))
    return torch.stack([torch.stack([torch.einsum("nhwi,nhwo->oi", xp[:, kh * d:kh * d + H, kw * d:kw * d + W], dy)
                                     for kw in range(3)], -1) for kh in range(3)], -2)


# ------------------------------ convolution forward and input gradient (nn.Conv2d and its autograd wrt the input, include/rpnet_abi.h), NHWC
def _row_factor(s, mode, shape, dtype):
    s = _c(s, dtype).reshape(shape)[..., None]
    return s if mode == 1 else 1 - s


def conv_fwd(x0, x1, w, bias=None, taps=9, dilation=1, upsample=0, in_scale=None, in_scale_mode=0, ep_scale=None, ep_shift=None,
             ep_relu=0, groups=1, out_scale=None, out_scale_mode=0, prev=None, dtype=F64):
    """one launch of rpnet_conv_fwd -> (the final output, acc + bias) [N, H, W, cout].  The sources x0 | x1 [N, h, w, C0 | C1] are
    concatenated along C (x1 None: one source), multiplied per SOURCE pixel by in_scale [N, h, w] (mode 1) or 1 - in_scale (mode 2),
    nearest x2 up-sampled (upsample = 1) and convolved with w [cout, cin, k, k] (taps 9: k = 3, tap spacing and zero padding
    max(dilation, 1); taps 1: k = 1) through F.conv2d; + bias.  That sum is what stats_partial adds up.  Then, in the kernels'
    order: * ep_scale[g] + ep_shift[g] ([groups, cout]; image n is in group n // (N / groups)), ReLU, * out_scale [N, H, W]
    (mode 1) or 1 - out_scale (mode 2) per OUTPUT pixel, + prev (accumulate)."""
    x = _c(x0, dtype) if x1 is None else torch.cat([_c(x0, dtype), _c(x1, dtype)], -1)
    if in_scale_mode:
        x = x * _row_factor(in_scale, in_scale_mode, x.shape[:3], dtype)
    if upsample:
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    d = max(int(dilation), 1) if taps == 9 else 0
    pre = _nhwc(F.conv2d(x.permute(0, 3, 1, 2), _c(w, dtype), _c(bias, dtype), padding=d, dilation=max(d, 1)))
    y = pre
    if ep_scale is not None:
        y = y * _per_image(_c(ep_scale, dtype).reshape(groups, -1), y.shape[0]) + _per_image(_c(ep_shift, dtype).reshape(groups, -1), y.shape[0])
    if ep_relu:
        y = torch.relu(y)
    if out_scale_mode:
        y = y * _row_factor(out_scale, out_scale_mode, y.shape[:3], dtype)
    if prev is not None:
        y = y + _c(prev, dtype)
    return y, pre


def conv_dgrad(dy, w, taps=9, dilation=1, co_split=None, out_scale=None, out_scale_mode=0, prev=None, upsample=0, dtype=F64):
    """the input gradient of y = conv(x, w), w [cout, cin, k, k], from dy [N, H, W, cout]: the same convolution with the transposed,
    flipped weight -> dx [N, H, W, cin], * out_scale [N, H, W] (mode 1) or 1 - out_scale (mode 2), + prev (accumulate), through
    upsample2_bwd for a layer that reads its input through the nearest x2 up-sampling, then cut along C at co_split = (Co0, Co1)
    into the gradients of the two concatenated sources -> a list of one or two tensors"""
    wt = _c(w, dtype).transpose(0, 1).flip(2, 3)
    dx, _ = conv_fwd(dy, None, wt, None, taps, dilation, 0, out_scale=out_scale, out_scale_mode=out_scale_mode, prev=prev, dtype=dtype)
    if upsample:
        dx = upsample2_bwd(dx, dtype)
    if co_split is None or not co_split[1]:
        return [dx]
    return [dx[..., :co_split[0]].contiguous(), dx[..., co_split[0]:].contiguous()]


def _upconv_collapsed(x, wc, bias):
    # phase (py, px) of the output is a 2 x 2 convolution of the zero-padded SOURCE whose window starts at (Y + py - 1, X + px - 1)
    N, h, w, _ = x.shape
    cout = wc.shape[0] // 4
    xp = F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1))
    y = torch.zeros(N, cout, 2 * h, 2 * w, dtype=x.dtype)
    for py in range(2):
        for px in range(2):
            o = F.conv2d(xp, wc[(py * 2 + px) * cout:(py * 2 + px + 1) * cout], bias)          # [N, cout, h + 1, w + 1]
            y[:, :, py::2, px::2] = o[:, :, py:py + h, px:px + w]
    return _nhwc(y)


def upconv_collapsed(x, wc, bias=None, dtype=F64):
    """nn.Upsample(2) -> Conv2d 3 x 3 from its COLLAPSED weights wc [4 cout, cin, 2, 2] (phase-major, rpnet_upconv_collapse_weights):
    x [N, h, w, cin] -> y [N, 2 h, 2 w, cout], y[2 Y + py, 2 X + px] = sum_{r, c} wc[(py, px)][r][c] x[Y + py + r - 1, X + px + c - 1]"""
    return _upconv_collapsed(_c(x, dtype), _c(wc, dtype), _c(bias, dtype))


def upconv_collapsed_dgrad(dy, wc, dtype=F64):
    """its input gradient through autograd: dy [N, 2 h, 2 w, cout] -> dx [N, h, w, cin]"""
    dy, wc = _c(dy, dtype), _c(wc, dtype)
    x = torch.zeros(dy.shape[0], dy.shape[1] // 2, dy.shape[2] // 2, wc.shape[1], dtype=dtype, requires_grad=True)
    (g,) = torch.autograd.grad(_upconv_collapsed(x, wc, None), x, dy)
    return g


# ------------------------- the first layer, Cin = 1 (Conv1.conv.0 of net/unet.py:407 with img_ch = 1, conv_block of net/modules.py:47-49)
def _per_image(v, N):
    """[groups, C] -> [N, 1, 1, C]: image n is in statistic group n // (N // groups)"""
    return v.repeat_interleave(N // v.shape[0], 0)[:, None, None]


def conv1(x, w, bias=None, dtype=F64):
    """x [N, H, W] (= [N, 1, H, W]), w [cout, 1, 3, 3], bias [cout] or None -> y [N, H, W, cout] = nn.Conv2d(1, cout, 3, padding=1)"""
    return _nhwc(F.conv2d(_c(x, dtype)[:, None], _c(w, dtype), _c(bias, dtype), padding=1))


def conv1_affine_relu(y, scale, shift, groups=1, dtype=F64):
    """relu(y * scale[g] + shift[g]), y [N, H, W, C], scale / shift [groups, C] (or [C] with groups = 1: the eval-mode epilogue)"""
    y = _c(y, dtype)
    sc, sh = _c(scale, dtype).reshape(groups, -1), _c(shift, dtype).reshape(groups, -1)
    return torch.relu(y * _per_image(sc, y.shape[0]) + _per_image(sh, y.shape[0]))


def _bn_terms(dz, y, stats, groups, dtype):
    """(dz m, xhat) with m = [y scale + shift > 0], xhat = (y - mean) invstd; stats [4][groups][C] = scale, shift, mean, invstd"""
    dz, y, st = _c(dz, dtype), _c(y, dtype), _c(stats, dtype).reshape(4, groups, -1)
    N = y.shape[0]
    sc, sh, mu, inv = (_per_image(st[i], N) for i in range(4))
    return dz * (y * sc + sh > 0).to(dtype), (y - mu) * inv, sc


def bn_bwd_sums(dz, y, stats, groups=1, dtype=F64):
    """-> (sum dz m, sum dz m xhat), each [groups, C]: the two sums of the BatchNorm + ReLU backward per (group, channel)"""
    dm, xhat, _ = _bn_terms(dz, y, stats, groups, dtype)
    C = dm.shape[-1]
    return dm.reshape(groups, -1, C).sum(1), (dm * xhat).reshape(groups, -1, C).sum(1)


def bn_dy(dz, y, stats, coef=None, groups=1, dtype=F64):
    """dy = scale (dz m - c1 - xhat c2), coef [groups, C, 2] = (c1, c2) (None: zero, the eval-mode form) -> [N, H, W, C]"""
    dm, xhat, sc = _bn_terms(dz, y, stats, groups, dtype)
    if coef is None:
        return sc * dm
    cf = _c(coef, dtype).reshape(groups, -1, 2)
    return sc * (dm - _per_image(cf[..., 0], dm.shape[0]) - xhat * _per_image(cf[..., 1], dm.shape[0]))


def conv1_dgrad(dy, w, dtype=F64):
    """dy [N, H, W, cout], w [cout, 1, 3, 3] -> dx [N, H, W]: the adjoint of conv1 with respect to the image"""
    return F.conv_transpose2d(_c(dy, dtype).permute(0, 3, 1, 2), _c(w, dtype), padding=1)[:, 0]


# ------------------------------- BatchNorm2d + ReLU, train and eval mode (net/modules.py:48-52; csrc/bn.hip), NHWC, [groups, C] statistics
def bn_stats(y, gamma, beta, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, groups=1, dtype=F64):
    """nn.BatchNorm2d in train mode called once per statistic group, in group order, on y [N, H, W, C] (group g = images
    g N/groups ...): -> (scale, shift, mean, invstd) each [groups, C] with scale = gamma invstd, shift = beta - mean scale, and the
    running buffers after one momentum update per group with the UNBIASED variance (None stays None)"""
    y, gamma, beta = _c(y, dtype), _c(gamma, dtype), _c(beta, dtype)
    yg = y.reshape(groups, -1, y.shape[-1])
    R = yg.shape[1]
    mean, var = yg.mean(1), yg.var(1, unbiased=False)
    invstd = (var + eps).rsqrt()
    scale = gamma[None] * invstd
    rm, rv = _c(running_mean, dtype), _c(running_var, dtype)
    for g in range(groups):
        if rm is not None:
            rm = (1 - momentum) * rm + momentum * mean[g]
        if rv is not None:
            rv = (1 - momentum) * rv + momentum * (var[g] * R / (R - 1) if R > 1 else var[g])
    return scale, beta[None] - mean * scale, mean, invstd, rm, rv


def bn_relu(y, scale, shift, groups=1, dtype=F64):
    """z = relu(y scale[g] + shift[g]) [N, H, W, C]"""
    return conv1_affine_relu(y, scale, shift, groups, dtype)


def bn_relu_pool(y, scale, shift, groups=1, dtype=F64):
    """max_pool2d(2, 2) of bn_relu -> [N, H/2, W/2, C]"""
    return maxpool2(bn_relu(y, scale, shift, groups, dtype), dtype)


def _pinned(value, fn):
    """`value` (a constant) with the gradient of fn: the statistic at the value the caller was given"""
    return value + (fn - fn.detach())


def bn_bwd(dz, y, stats, groups=1, pooled=False, dtype=F64):
    """autograd of the train-mode expression z = relu(gamma xhat(y) + beta) (pooled: max_pool2d(z, 2, 2), dz the pooled gradient;
    torch routes a window's gradient to its first maximum in row, column scan order), the batch mean and invstd held at the VALUES
    of stats [4][groups][C] (scale, shift, mean, invstd: what the kernels are given) while their gradients are those of the batch
    statistics.  -> (dy [N, H, W, C], dgamma [C], dbeta [C] summed over groups, coef [groups, C, 2] = (sum dz m, sum dz m xhat) / R)"""
    st = _c(stats, dtype).reshape(4, groups, -1)
    y = _c(y, dtype).clone().requires_grad_(True)
    N, C = y.shape[0], y.shape[-1]
    sc, sh, mu, inv = st
    gamma = [(sc[g] / inv[g]).clone().requires_grad_(True) for g in range(groups)]
    beta = [(sh[g] + mu[g] * sc[g]).clone().requires_grad_(True) for g in range(groups)]
    zs, xh = [], []
    for g in range(groups):
        yg = y[g * (N // groups):(g + 1) * (N // groups)]
        m = _pinned(mu[g], yg.mean((0, 1, 2)))
        d = yg - m
        v = (d * d).mean((0, 1, 2))
        istd = _pinned(inv[g], (v + (inv[g] ** -2 - v.detach())).rsqrt())
        xh.append(d * istd)
        zs.append(torch.relu(xh[-1] * gamma[g] + beta[g]))
    z = torch.cat(zs)
    if pooled:
        z = _nhwc(F.max_pool2d(z.permute(0, 3, 1, 2), 2, 2))
    grads = torch.autograd.grad(z, [y] + gamma + beta, _c(dz, dtype))
    dy, dgs, dbs = grads[0], torch.stack(grads[1:1 + groups]), torch.stack(grads[1 + groups:])
    R = y[0].numel() // C * (N // groups)
    return dy, dgs.sum(0), dbs.sum(0), torch.stack([dbs, dgs], -1) / R


def bn_eval_affine(gamma, beta, running_mean, running_var, eps=1e-5, dtype=F64):
    """-> (scale, shift) [C] of eval-mode BatchNorm: gamma / sqrt(running_var + eps), beta - running_mean scale"""
    scale = _c(gamma, dtype) / (_c(running_var, dtype) + eps).sqrt()
    return scale, _c(beta, dtype) - _c(running_mean, dtype) * scale


def bn_eval_relu(y, scale, shift, dtype=F64):
    """y [P, C] -> (z = relu(y scale + shift), max z: the running absmax starts at 0)"""
    z = torch.relu(_c(y, dtype) * _c(scale, dtype) + _c(shift, dtype))
    return z, z.max().clamp_min(0) if z.numel() else torch.zeros((), dtype=dtype)


def bn_eval_bwd(dz, y, stats, groups=1, dtype=F64):
    """autograd of z = relu(gamma (y - mean) invstd + beta) with CONSTANT statistics (stats [4][groups][C], group g's rows of it
    for the images of group g) -> (dy, dgamma [C], dbeta [C] summed over groups)"""
    st = _c(stats, dtype).reshape(4, groups, -1)
    y = _c(y, dtype).clone().requires_grad_(True)
    N = y.shape[0]
    sc, sh, mu, inv = st
    gamma = (sc / inv).clone().requires_grad_(True)
    beta = (sh + mu * sc).clone().requires_grad_(True)
    z = torch.relu((y - _per_image(mu, N)) * _per_image(inv, N) * _per_image(gamma, N) + _per_image(beta, N))
    dy, dg, db = torch.autograd.grad(z, (y, gamma, beta), _c(dz, dtype))
    return dy, dg.sum(0), db.sum(0)


# ---------------- the glue between two refinement iterations (net/rp_net.py:65-69,301-311; csrc/refine.hip): compositions of the above
def refine_glue(y, scale, shift, proto, scaler=20.0, soft=False, dtype=F64):
    """y [B, h, w, F], scale / shift [F] or None (no BatchNorm: z = y), proto [B, K, F] ->
    (z [B, h, w, F], pred [B, K, h, w], logits [B, K, 4h, 4w], mask [B, h, w])"""
    B, h, w, Fc = y.shape
    K = proto.shape[1]
    z = _c(y, dtype) if scale is None else bn_relu(y, scale, shift, dtype=dtype)
    pred = cosine_match(z.reshape(B, h * w, Fc), proto, scaler, dtype).reshape(B, K, h, w)
    logits = bilinear_up(pred.reshape(B * K, h, w), 4 * h, 4 * w, dtype).reshape(B, K, 4 * h, 4 * w)
    return z, pred, logits, softmax_thresh_pool(logits, 4, soft, dtype)


def refine_glue_bwd(dlogits, f, proto, scaler=20.0, dtype=F64):
    """dlogits [B, K, 4h, 4w], f [B, h, w, F] (the features after BatchNorm + ReLU) -> (df [B, h, w, F], dproto [B, K, F])"""
    B, K, H, W = dlogits.shape
    h, w = H // 4, W // 4
    dpred = bilinear_up_bwd(torch.as_tensor(dlogits).reshape(B * K, H, W), h, w, dtype).reshape(B, K, h * w)
    df, dproto = cosine_match_bwd(torch.as_tensor(f).reshape(B, h * w, -1), proto, dpred, scaler, dtype)
    return df.reshape(B, h, w, -1), dproto


def hard_mask_margin(logits, dtype=F64):
    """|l1 - logsumexp(the other classes)| [B, H, W]: the distance of softmax[:, 1] > 0.5 from its boundary"""
    lg = _c(logits, dtype)
    return (lg[:, 1] - torch.logsumexp(torch.cat([lg[:, :1], lg[:, 2:]], 1), 1)).abs()


# ---------------------------------------------- the multi-tensor loss and the training objective (csrc/loss.hip), per logit tensor
def dice_ce_stats(logits, labels, dtype=F64):
    """-> [B + 1, 2K + 2]: per sample, then summed over the batch: inter_k = sum p_k [label = k], card_k = sum p_k + [label = k],
    ce_sum = - sum log_softmax[label], count = the pixels (nothing ignored)"""
    lg, lab = _c(logits, dtype), torch.as_tensor(labels).cpu()
    K = lg.shape[1]
    one_hot = torch.eye(K, dtype=dtype)[lab].permute(0, 3, 1, 2)
    p = torch.softmax(lg, dim=1)
    ce = F.cross_entropy(lg, lab, reduction="none").sum(dim=(1, 2))
    rows = torch.cat([(p * one_hot).sum(dim=(2, 3)), (p + one_hot).sum(dim=(2, 3)), ce[:, None],
                      torch.full((lg.shape[0], 1), float(lg.shape[2] * lg.shape[3]), dtype=dtype)], 1)
    return torch.cat([rows, rows.sum(0, keepdim=True)], 0)


def objective(logits, weights, labels, extra=None, extra_scale=0.0, dtype=F64):
    """-> (loss_z [n] = dice_ce of every tensor, total = sum_z w_z loss_z + extra_scale * extra)"""
    losses = torch.stack([dice_ce(t, labels, dtype=dtype) for t in logits])
    total = (torch.as_tensor(weights, dtype=dtype) * losses).sum()
    return losses, total if extra is None else total + extra_scale * _c(extra, dtype).reshape(())
