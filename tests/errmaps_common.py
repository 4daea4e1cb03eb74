"""What the error-map tests share: the seeded inputs of tests/golden/errmaps.npz (integer arithmetic and IEEE + - * / only, so every
machine builds the same bits; the file holds their digests and the reference's outputs), a torch restatement of kornia.metrics.ssim
(the stand-in tests/golden/make_golden_errmaps.py plugs into the reference's utils/visualizations.py, next to
oracle.metrics.rgb_to_lab) and restatements of the three maps themselves.  tests/test_errmaps_host.py pins the latter to the
reference's float64 outputs.  Not product code."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import metrics as om
from tests import views_common as vc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "errmaps.npz")
MAPS = ("rgbssim", "labmse", "abmse")
# (B, H, W): the reflect padding across the whole frame; one axis at the minimum; smaller than a tile with an odd width and two
# frames of different ranges; three 64 x 32 tiles either way with ragged edges
SHAPES = ((1, 6, 6), (1, 6, 37), (1, 37, 6), (2, 23, 37), (2, 70, 131))


def tag(shape):
    return "%dx%dx%d" % tuple(shape)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def _smooth(b, h, w, seed):
    """[b,3,h,w] float32 in [0, 1): uniform noise on a grid of 8-pixel cells, interpolated bilinearly"""
    gh, gw = h // 8 + 2, w // 8 + 2
    coarse = vc.uniform((b, 3, gh, gw), seed)
    ys, xs = np.arange(h, dtype=np.float32) / np.float32(8), np.arange(w, dtype=np.float32) / np.float32(8)
    y0, x0 = ys.astype(np.int64), xs.astype(np.int64)
    fy, fx = (ys - y0.astype(np.float32))[:, None], (xs - x0.astype(np.float32))[None, :]
    one = np.float32(1)
    top = coarse[:, :, y0][:, :, :, x0] * (one - fx) + coarse[:, :, y0][:, :, :, x0 + 1] * fx
    bot = coarse[:, :, y0 + 1][:, :, :, x0] * (one - fx) + coarse[:, :, y0 + 1][:, :, :, x0 + 1] * fx
    return (top * (one - fy) + bot * fy).astype(np.float32)


def inputs(shape):
    """x: a smooth texture plus noise in [0, 1]; y: x under a mild colour change (a gain and an offset per channel) plus noise of a
    few percent.  The second frame of a batch gets a weaker change and less noise: the frames' maps have different ranges."""
    b, h, w = shape
    seed = 1000 * h + w
    f = np.float32
    x = (f(0.15) + f(0.6) * _smooth(b, h, w, seed) + f(0.1) * vc.uniform((b, 3, h, w), seed + 1)).astype(np.float32)
    gain = np.array([0.93, 1.05, 0.88], dtype=np.float32)[None, :, None, None]
    offset = np.array([0.03, -0.02, 0.05], dtype=np.float32)[None, :, None, None]
    strength = np.array([1.0, 0.5][:b], dtype=np.float32)[:, None, None, None]
    noise = (vc.uniform((b, 3, h, w), seed + 2) - f(0.5)) * f(0.12)
    y = x + strength * ((x * gain + offset - x) + noise)
    return x, np.clip(y, f(0), f(1)).astype(np.float32)


# ---- kornia.metrics.ssim ----------------------------------------------------------------------------------------------------------
def kornia_ssim(img1, img2, window_size, max_val=1.0, eps=1e-12):
    """kornia.metrics.ssim restated from its published source (kornia/metrics/ssim.py, kornia/filters: get_gaussian_kernel1d,
    filter2d_separable): the normalised Gaussian exp(-k^2 / (2 * 1.5^2)) of `window_size` taps, applied per channel along the
    rows, then along the columns, under reflect padding; C1 = (0.01 max_val)^2, C2 = (0.03 max_val)^2; the SSIM map [B,C,H,W] in
    the dtype of the inputs.  Parity with kornia itself is unpinned (it is absent offline)."""
    half = window_size // 2
    k = torch.arange(window_size, dtype=img1.dtype) - half
    g = torch.exp(-k ** 2 / (2 * 1.5 ** 2))
    g = g / g.sum()
    c = img1.shape[1]

    def blur(t):
        t = F.pad(t, (half, half, half, half), mode="reflect")
        t = F.conv2d(t, g.view(1, 1, 1, -1).repeat(c, 1, 1, 1), groups=c)
        return F.conv2d(t, g.view(1, 1, -1, 1).repeat(c, 1, 1, 1), groups=c)
    c1, c2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    mu1, mu2 = blur(img1), blur(img2)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 ** 2, mu2 ** 2, mu1 * mu2
    sigma1_sq = blur(img1 ** 2) - mu1_sq
    sigma2_sq = blur(img2 ** 2) - mu2_sq
    sigma12 = blur(img1 * img2) - mu1_mu2
    num = (2.0 * mu1_mu2 + c1) * (2.0 * sigma12 + c2)
    den = (mu1_sq + mu2_sq + c1) * (sigma1_sq + sigma2_sq + c2)
    return num / (den + eps)


# ---- the three maps (utils/visualizations.py:39-60) ------------------------------------------------------------------------------
def unscaled(name, x, y):
    """the map m of one of MAPS before minmaxscale, [B,H,W], in the dtype of the torch tensors x, y"""
    if name == "rgbssim":
        return 0.5 - kornia_ssim(x, y, window_size=11).mean(dim=1) / 2
    lab = om.rgb_to_lab(torch.square(x - y))
    return lab.mean(dim=1) if name == "labmse" else lab[:, 1:].mean(dim=1)


def scaled(m):
    """utils/visualizations.py:24-28"""
    lo, hi = m.amin(dim=(-1, -2), keepdim=True), m.amax(dim=(-1, -2), keepdim=True)
    return (m - lo) / (hi - lo)


def error_gate(got, ref32, ref64):
    """A float32 result held against the reference's own float32 run: (rms, max) of |got - ref64| and of e32 = |ref32 - ref64|,
    and whether the former stay within twice the latter, with an absolute floor of 1e-6 where e32 happens to be almost nothing."""
    e = np.abs(got.astype(np.float64) - ref64)
    e32 = np.abs(ref32.astype(np.float64) - ref64)
    mine, ref = (float(np.sqrt((e ** 2).mean())), float(e.max())), (float(np.sqrt((e32 ** 2).mean())), float(e32.max()))
    ok = all(m <= max(2.0 * r, 1e-6) for m, r in zip(mine, ref))
    return mine, ref, ok
