"""fp64 restatement of the image-quality table (the yardstick of tests/test_image_quality_gpu.py), written from the definition in the header comment
of csrc/image_quality.hip.  x, y: [B, C, H, W] (y may be [B, K, C, H, W]: frame 0), m (optional): [B, H, W], used as given.
    xh = clamp(x, 0, 1), yh = clamp(y, 0, 1), d = xh - yh
    l1 = mean |d|,  mse = mean d^2,  psnr = -10 log10(max(mse, 1e-10))
    ssim = mean over channels and the (H - 10) x (W - 10) valid window positions of
           S = (2 mx my + C1)(2 sxy + C2) / ((mx^2 + my^2 + C1)(sxx + syy + C2)),  C1 = 1e-4, C2 = 9e-4,
           f = separable 11-tap Gaussian window (sigma 1.5, sum 1), mx = f(xh), my = f(yh), sxx = f(xh^2) - mx^2, syy = f(yh^2) - my^2,
           sxy = f(xh yh) - mx my
    l1_fg = sum m |d| / (C sum m),  psnr_fg = the psnr formula on sum m d^2 / (C sum m),
    ssim_fg = sum m_c S / (C sum m_c) with m_c = m at the window centre (h + 5, w + 5);  a weight sum of 0 -> NaN;  no mask -> NaN
Columns: ssim, psnr, l1, ssim_fg, psnr_fg, l1_fg.  Test infrastructure only: plain torch on the host, never on the product path."""
import math

import torch

COLUMNS = ('ssim', 'psnr', 'l1', 'ssim_fg', 'psnr_fg', 'l1_fg')
C1, C2 = 1e-4, 9e-4
NAN = float('nan')


def taps():
    k = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-k * k / (2 * 1.5 ** 2))
    return g / g.sum()


def window(a):
    """[..., H, W] fp64 -> [..., H - 10, W - 10]: the Gaussian window at every valid position (horizontal, then vertical)"""
    g = taps()
    h, w = a.shape[-2:]
    rows = sum(g[k] * a[..., :, k:k + w - 10] for k in range(11))
    return sum(g[k] * rows[..., k:k + h - 10, :] for k in range(11))


def ssim_map(x, y):
    """S per channel and valid window position of two fp64 [B, C, H, W] images already clamped"""
    mx, my = window(x), window(y)
    sxx, syy, sxy = window(x * x) - mx * mx, window(y * y) - my * my, window(x * y) - mx * my
    return (2 * mx * my + C1) * (2 * sxy + C2) / ((mx * mx + my * my + C1) * (sxx + syy + C2))


def psnr(mse):
    return NAN if mse != mse else -10.0 * math.log10(max(mse, 1e-10))


def table(x, y, mask=None):
    """-> fp64 [B, 6]"""
    x, y = x.detach().double().cpu(), y.detach().double().cpu()
    if y.dim() == 5:
        y = y[:, 0]
    assert x.shape == y.shape and x.dim() == 4 and x.shape[-1] >= 11 and x.shape[-2] >= 11
    b, c, h, w = x.shape
    x, y = x.clamp(0.0, 1.0), y.clamp(0.0, 1.0)
    d = x - y
    S = ssim_map(x, y)
    out = torch.full((b, 6), NAN, dtype=torch.float64)
    for n in range(b):
        out[n, 0] = S[n].mean()
        out[n, 1] = psnr(d[n].pow(2).mean().item())
        out[n, 2] = d[n].abs().mean()
        if mask is None:
            continue
        m = mask[n].detach().double().cpu()
        assert tuple(m.shape) == (h, w)
        mc = m[5:h - 5, 5:w - 5]
        wsum, csum = c * m.sum().item(), c * mc.sum().item()
        if csum != 0:
            out[n, 3] = (mc[None] * S[n]).sum() / csum
        if wsum != 0:
            out[n, 4] = psnr((m[None] * d[n].pow(2)).sum().item() / wsum)
            out[n, 5] = (m[None] * d[n].abs()).sum() / wsum
    return out
