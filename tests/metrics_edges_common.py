"""Inputs, oracle wrappers and bounds shared by tests/test_metrics_edges_host.py and tests/test_metrics_edges_gpu.py: the frame
metrics (csrc/metrics.hip, fsim.hip, fft2d.hip) at the edges of their pooling factor, their tiles and float32."""
import math

import torch

from oracle import metrics as om
from tests.test_metrics import _pair as pair          # the smooth-field-plus-noise frames of tests/test_metrics.py

METRICS = ("ssim", "icid", "fsim")
ATOL = {"ssim": 2e-6, "icid": 5e-6, "fsim": 2e-5}      # tests/test_metrics.py: device against the float64 oracle

# (batch, H, W) -> pooling factor: remainders in H and W at every factor, 640 = the one size where round-half-even shows
FACTOR_SHAPES = {(1, 385, 387): 2, (1, 640, 644): 2, (2, 641, 643): 3, (1, 899, 901): 4}

# k of |device - oracle(float64)| <= max(atol, k * |oracle(float32) - oracle(float64)|): the smallest of 2, 4, 8 with the ratio
# measured on an MI355X at most half of it ("float32 on flat frames")
K_FLAT = {"ssim": 2, "icid": 2, "fsim": 4}
K_STAGE = {"t": 4, "pc": 4}
K_FFT = 4


def oracle(name, x, y, dtype=torch.float64):
    """per-frame oracle value [B] float64 (om.icid is a mean over the batch: one frame at a time)"""
    if name == "icid":
        return torch.stack([om.icid(x[i:i + 1], y[i:i + 1], dtype=dtype).double() for i in range(x.shape[0])])
    return getattr(om, name)(x, y, dtype=dtype).double()


def device(hip, name, x, y):
    return getattr(hip, "frame_" + name)(x.cuda(), y.cuda()).cpu()


# ---- dead rim: trailing rows / columns that no metric may read -----------------------------------------------------------------
def pooled_rim(h, w):
    """(first dead row, first dead column) of SSIM / FSIM: avg_pool2d(f) drops the remainder"""
    f = om.metric_factor(h, w)
    return f * (h // f), f * (w // f)


def flip_rim(t, row0, col0):
    """t with the rows from row0 and the columns from col0 replaced by 1 - t"""
    out = t.clone()
    out[..., row0:, :] = 1 - t[..., row0:, :]
    out[..., :, col0:] = 1 - out[..., :, col0:]
    return out


def icid_rim(x, y):
    """(first dead row, first dead column) of iCID, found on the oracle: the most trailing rows, then columns, whose replacement by
    1 - x leaves om.icid EXACTLY unchanged (the bilinear taps of F.interpolate(scale_factor=1/f) never reach them)"""
    h, w = x.shape[-2:]
    f = om.metric_factor(h, w)

    def same(a, b, row0, col0):
        return torch.equal(om.icid(flip_rim(a, row0, col0), flip_rim(b, row0, col0)), om.icid(a, b))
    row0, col0 = h, w                                  # the taps are a matter of geometry: searched on the first pair ...
    while h - row0 < 2 * f and same(x[:1], y[:1], row0 - 1, w):
        row0 -= 1
    while w - col0 < 2 * f and same(x[:1], y[:1], h, col0 - 1):
        col0 -= 1
    assert same(x, y, row0, col0)                      # ... proven on the whole batch, rows and columns together
    return row0, col0


# ---- probes: 75 x 77 (f = 1), SSIM map 65 x 67 = tiles 32 | 32 | 1 by 32 | 32 | 3, iCID grid 3 x 5 ---------------------------------
PROBE_H, PROBE_W, PROBE_AMP = 75, 77, 0.3
# (row, column, rows, columns) of the raised patch: 4 x 4 in the corners, on the tile seams and one line off the lower edge, and
# two patches enlarged to 4 x 32 along the lower and the right edge -- iCID's reflect padding makes its map even about the edge
# line, so a 4 x 4 patch moves the last line against its neighbour by 8.3 (row) / 3.7 (column) tolerances only, the long ones by 18.9 / 21.6
PROBES = tuple((r, c, 4, 4) for r, c in ((0, 0), (0, 73), (71, 0), (71, 73), (35, 36), (41, 42), (30, 20), (14, 30), (70, 20))) \
    + ((71, 20, 4, 32), (20, 73, 32, 4))


def probe_gt():
    gen = torch.Generator().manual_seed(75077)
    base = torch.rand(1, 3, 12, 12, generator=gen)
    return torch.nn.functional.interpolate(base, size=(PROBE_H, PROBE_W), mode="bicubic", align_corners=True).clamp(0, 1).contiguous()


def probe(gt, patch):
    """gt with one patch raised by 0.3 (clamped): an error a seam, a halo column or a reflect index cannot lose"""
    r, c, ph, pw = patch
    assert r + ph <= PROBE_H and c + pw <= PROBE_W
    x = gt.clone()
    x[..., r:r + ph, c:c + pw] = (x[..., r:r + ph, c:c + pw] + PROBE_AMP).clamp(0, 1)
    return x


# ---- flat and saturated frames -------------------------------------------------------------------------------------------------
def flat_inputs():
    """name -> (x, gt, holds the plain atol): frames on which float32 moments cancel and FSIM's phase congruency has nothing but
    rounding noise to work on"""
    h, w = PROBE_H, PROBE_W
    gen = torch.Generator().manual_seed(98)
    shape = (1, 3, h, w)
    noise_gt = torch.rand(shape, generator=gen)
    bright = 0.98 + 1e-3 * torch.rand(shape, generator=gen)
    lgt = probe_gt()
    lx = probe(lgt, PROBES[4])                          # the smooth probe frames between black bars
    for t in (lx, lgt):
        t[..., :20, :] = 0
        t[..., 55:, :] = 0
    big = 0.98 + 1e-3 * torch.rand(1, 3, 641, 643, generator=gen)
    return {
        "noise": ((noise_gt + 0.05 * torch.randn(shape, generator=gen)).clamp(0, 1), noise_gt, False),
        "flat-bright": (bright + 1e-3 * torch.randn(shape, generator=gen), bright, False),
        "const-0.2-0.8": (torch.full(shape, 0.2), torch.full(shape, 0.8), False),
        "sat-1-254": (torch.ones(shape), torch.full(shape, 254 / 255), False),
        "zeros": (torch.zeros(shape), torch.zeros(shape), False),
        "letterbox": (lx, lgt, True),
        "flat-bright-641x643": (big + 1e-3 * torch.randn(1, 3, 641, 643, generator=gen), big, False),
    }


# ---- FSIM stages and the FFT ---------------------------------------------------------------------------------------------------
STAGE_SHAPES = ((2, 40, 56), (1, 97, 131), (1, 251, 257))      # 251 x 257: prime sides at f = 1, the FFT's plain-butterfly stage
FFT_SHAPES = ((75, 77), (251, 257), (270, 481))
FFT_BANDS = 8


def image_like_plane(h, w):
    """a luminance plane as FSIM feeds the transform: 128 + a smooth field of amplitude 60 + noise of amplitude 2, complex64"""
    gen = torch.Generator().manual_seed(h * 1000 + w)
    base = torch.rand(1, 1, h // 8 + 2, w // 8 + 2, generator=gen) * 2 - 1
    smooth = torch.nn.functional.interpolate(base, size=(h, w), mode="bicubic", align_corners=True)[0, 0].clamp(-1, 1)
    plane = 128 + 60 * smooth + 2 * (torch.rand(h, w, generator=gen) * 2 - 1)
    return torch.complex(plane, torch.zeros(h, w)).to(torch.complex64).contiguous()


def radial_bands(h, w):
    """[h, w] int64: band 0 .. FFT_BANDS - 1 by radial frequency (equal widths up to the corner), -1 at DC"""
    fy, fx = torch.fft.fftfreq(h, dtype=torch.float64), torch.fft.fftfreq(w, dtype=torch.float64)
    r = torch.sqrt(fy[:, None] ** 2 + fx[None, :] ** 2)
    band = torch.clamp((r / (math.sqrt(0.5) + 1e-12) * FFT_BANDS).long(), max=FFT_BANDS - 1)
    band[0, 0] = -1
    return band


def band_errors(got, want, band):
    """per band: RMS of |got - want| over the band / RMS of |want| over the band"""
    out = []
    for b in range(FFT_BANDS):
        m = band == b
        assert int(m.sum()) > 0
        out.append(math.sqrt(float(((got - want).abs()[m] ** 2).mean())) / math.sqrt(float((want.abs()[m] ** 2).mean())))
    return out
