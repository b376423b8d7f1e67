"""Torch restatement of the fusion loss (a008 MyLoss with its kornia operators), written from the published definitions of
MS_SSIMLoss, ssim_loss(window 11, padding "same"), Sobel and PSNRLoss for one channel.  Plain F.conv2d / F.pad, 2-D masks built as
outer products, dtype-generic (fp64 is the oracle of the HIP kernels; torch.autograd of it is the gradient oracle).  kornia itself is
not available, so parity with kornia is unpinned; this text is the contract the kernels are held to.
"""
import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2
MS_SIGMAS = (0.5, 1.0, 2.0, 4.0, 8.0)
DEFAULTS = dict(choose_ms_ssim=True, fus_ir_ssim_weight=0.2, use_psnr=False, fus_ir_psnr_weight=0.4, ssim_scale=0.305,
                texture_scale=250, intensity_scale=45, psnr_scale=0, ssim_loss_ratio=1 / 3, texture_loss_ratio=1 / 3,
                intensity_loss_ratio=1 / 3, psnr_loss_ratio=0)


def gauss_taps(size, sigma, dtype, device=None):
    k = torch.arange(size, dtype=dtype, device=device) - size // 2
    g = torch.exp(-k * k / (2 * sigma * sigma))
    return g / g.sum()


def gauss_filter(x, g, border):
    """Correlation of x (B,1,H,W) with the 2-D mask g g^T; border 'zero' or 'reflect', output the size of x."""
    r = g.numel() // 2
    mask = torch.outer(g, g)[None, None]
    if border == "zero":
        return F.conv2d(x, mask, padding=r)
    return F.conv2d(F.pad(x, (r, r, r, r), mode="reflect"), mask)


def gauss_filter_separable(x, g, border):
    """The same filter as a row pass and a column pass."""
    r = g.numel() // 2
    if border == "reflect":
        return F.conv2d(F.conv2d(F.pad(x, (r, r, r, r), mode="reflect"), g[None, None, None, :]), g[None, None, :, None])
    return F.conv2d(F.conv2d(x, g[None, None, None, :], padding=(0, r)), g[None, None, :, None], padding=(r, 0))


def _moments(x, y, g, border):
    b = x.shape[0]
    m = gauss_filter(torch.cat([x, y, x * x, y * y, x * y]), g, border)
    mux, muy, xx, yy, xy = (m[k * b:(k + 1) * b] for k in range(5))
    return mux, muy, xx - mux * mux, yy - muy * muy, xy - mux * muy


def ms_l_cs(x, y, sigma):
    g = gauss_taps(33, sigma, x.dtype, x.device)
    mux, muy, sxx, syy, sxy = _moments(x, y, g, "zero")
    l = (2 * mux * muy + C1) / (mux * mux + muy * muy + C1)
    cs = (2 * sxy + C2) / (sxx + syy + C2)
    return l, cs


def ms_ssim_l1(x, y):
    """MS_SSIMLoss() on one channel: the class holds three identical masks per sigma and, with groups = 1, multiplies all fifteen cs
    maps and the last three l maps -- hence the cubes."""
    pics = torch.ones_like(x)
    for sigma in MS_SIGMAS:
        l, cs = ms_l_cs(x, y, sigma)
        pics = pics * cs * cs * cs
    lm = l * l * l
    loss_ms = 1 - lm * pics
    l1 = gauss_filter((x - y).abs(), gauss_taps(33, MS_SIGMAS[-1], x.dtype, x.device), "zero")
    return (200 * (0.025 * loss_ms + 0.975 * l1)).mean()


def ssim_single(x, y):
    """2 * ssim_loss(x, y, window_size=11, max_val=1, reduction='mean', padding='same') (the factor 2 is a008:112)."""
    g = gauss_taps(11, 1.5, x.dtype, x.device)
    mux, muy, sxx, syy, sxy = _moments(x, y, g, "reflect")
    ssim = (2 * mux * muy + C1) * (2 * sxy + C2) / ((mux * mux + muy * muy + C1) * (sxx + syy + C2) + 1e-12)
    return 2 * torch.clamp((1 - ssim) / 2, 0, 1).mean()


def sobel_magnitude(x):
    kx = torch.tensor([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], dtype=x.dtype, device=x.device) / 8
    xp = F.pad(x, (1, 1, 1, 1), mode="replicate")
    gx, gy = F.conv2d(xp, kx[None, None]), F.conv2d(xp, kx.t()[None, None])
    return torch.sqrt(gx * gx + gy * gy + 1e-6)


def psnr_loss(x, y):
    return -10 * torch.log10(1 / ((x - y) ** 2).mean())


def components(f, i, v, ms):
    """The six pieces every term is a weighted sum of: s(f,i), s(f,v), T, I, p(f,i), p(f,v)."""
    s = ms_ssim_l1 if ms else ssim_single
    t = (sobel_magnitude(f) - torch.maximum(sobel_magnitude(i), sobel_magnitude(v))).abs().mean()
    inten = (f - torch.maximum(i, v)).abs().sum() / f.numel()
    return [s(f, i), s(f, v), t, inten, psnr_loss(f, i), psnr_loss(f, v)]


def combine(c, **kw):
    """S, T, I, P (unscaled) and total from the six components (tensors or gradients: everything is linear in them)."""
    k = dict(DEFAULTS, **kw)
    w, wp = k["fus_ir_ssim_weight"], k["fus_ir_psnr_weight"]
    S = w * c[0] + (1 - w) * c[1]
    P = wp * c[4] + (1 - wp) * c[5] if k["use_psnr"] else torch.zeros_like(c[4])
    total = (k["ssim_loss_ratio"] * k["ssim_scale"] * S + k["texture_loss_ratio"] * k["texture_scale"] * c[2]
             + k["intensity_loss_ratio"] * k["intensity_scale"] * c[3] + k["psnr_loss_ratio"] * k["psnr_scale"] * P)
    return S, c[2], c[3], P, total


def fusion_loss(f, i, v, **kw):
    """(S, T, I, P, total) of a008 MyLoss.calcu_total_loss with the given settings (defaults: the reference's)."""
    k = dict(DEFAULTS, **kw)
    return combine(components(f, i, v, k["choose_ms_ssim"]), **k)
