"""What the colour-cube tests of the distortion kernels share: the 24-bit colour cube as an image, the exact integer grey sum behind
adjust_contrast, and the float64 evaluation of oracle/distort.py's gamma up to the truncating cast.  Not product code."""
import numpy as np
import torch

from oracle import distort as od

TO_U8 = float(np.float32(255.0 + 1.0 - 1e-3))               # the factor of convert_image_dtype as float32 arithmetic holds it
GRID = od.setup_grid_distortions()


def grid_params(name):
    """the six parameters setup_grid_distortions gives the distortion `name`"""
    return [float(p) for n, p in GRID if n == name]


def cube(r0=0, r1=256):
    """every RGB triple with r0 <= red < r1 once, uint8 [3, 16 * (r1 - r0), 4096]: pixel number red * 65536 + green * 256 + blue.
    The whole cube is [3, 4096, 4096]; 16 reds make a slab of [3, 256, 4096]."""
    i = torch.arange(r0 * 65536, r1 * 65536, dtype=torch.int32)
    return torch.stack(((i >> 16), (i >> 8) & 255, i & 255)).to(torch.uint8).view(3, 16 * (r1 - r0), 4096)


def cube_plane(red):
    """the green / blue plane of the cube at one red, uint8 [3, 256, 256]"""
    return cube(red, red + 1).view(3, 256, 256)


def bytes_image():
    """the 256 byte values in all three channels, uint8 [3, 16, 16]"""
    return torch.arange(256, dtype=torch.int32).to(torch.uint8).view(1, 16, 16).expand(3, -1, -1).contiguous()


def gray_sum(img):
    """the exact sum of the uint8 grey image of a uint8 [3, H, W] image"""
    return int(od.rgb_to_grayscale(img).to(torch.int64).sum())


def exact_mean(img):
    """float32 [1, 1, 1]: the exact grey sum over the pixel count, divided in float64 and rounded to float32 once -- gray_mean of
    csrc/ct_distort.h, and what torch.mean approximates"""
    return torch.tensor(np.float32(gray_sum(img) / (img.shape[-2] * img.shape[-1]))).view(1, 1, 1)


def contrast_exact_mean(img, factor):
    return od._blend(img, exact_mean(img), factor)


def by_red_slabs(fn, reds=16):
    """fn over the whole cube, `reds` red values at a time (the temporaries of _hsv2rgb are 24 values per pixel), concatenated"""
    return torch.cat([fn(cube(r, r + reds)) for r in range(0, 256, reds)], dim=1)


# ---- float64 statement: the value the truncating cast receives ------------------------------------------------------------------------
def gamma_f64(img, gamma):
    """adjust_gamma before .to(uint8), in float64; gamma as the kernel receives it, (float)param"""
    x = img.to(torch.float64) / 255.0
    return (x ** float(np.float32(gamma))).clamp(0, 1) * TO_U8


def near_integer(x, eps=1e-4):
    """where a float64 pre-truncation value lies within eps of an integer: there a last-bit difference can move the cast"""
    return (x - x.round()).abs() <= eps
