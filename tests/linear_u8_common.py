"""What tests/test_linear_u8_host.py and tests/test_linear_u8_gpu.py share: the fixture of the uint8 MK / Xiao path
(tests/golden/linear_u8.npz, written by tests/golden/make_golden_linear_u8.py from the real reference), the exact moments of a
uint8 image from Python integers, and the seeded frames of the device tests.  Everything here runs on the CPU and is computed
once per process."""
import functools
import os
from fractions import Fraction

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linear_u8.npz")
DECOMPS = ("MK", "sqrt", "cholesky")
RESULTS = tuple("mk_" + d for d in DECOMPS) + ("xiao",)
PAIRS = ("p37x53", "p1x257", "p64x48_hue")
TIE = 1e-4                      # a byte is compared where value * 255 is further than this from a half-integer
MAX_TIE_SHARE = 1e-3            # the generator asserts it for every stored result
PIXELS = (2, 15, 16, 17, 257, 5461, 70001)       # bases of the frames of a batch on and off the 16-byte grid, one and many workgroups
BATCHES = (1, 3)
MK_SPEC = "methods.linear.monge_kantorovitch_color_transfer"
XIAO_SPEC = "methods.linear.color_transfer_in_correlated_color_space"
REINHARD_SPEC = "methods.linear.color_transfer_between_images"


def predict(t8, coef):
    """the affine map `coef` [4, 3] of t8 / 255.0 in float64, elementwise operations in a fixed order (the generator's function)"""
    x = t8.astype(np.float64) / 255.0
    return np.stack([((x[..., 0] * coef[0, j] + x[..., 1] * coef[1, j]) + x[..., 2] * coef[2, j]) + coef[3, j] for j in range(3)], axis=-1)


@functools.lru_cache(maxsize=None)
def fixture():
    """{pair: {"target", "reference": uint8 [H,W,3]; "mk_MK", "mk_sqrt", "mk_cholesky", "xiao": the reference's float64 result;
    "<result>_u8": its bytes}}.  The file keeps a float64 result as a fit and a residual (see the generator): put together here."""
    z = np.load(GOLDEN)
    out = {}
    for p in PAIRS:
        d = {"target": z[p + "/target"], "reference": z[p + "/reference"]}
        for r in RESULTS:
            d[r] = predict(d["target"], z["%s/%s_coef" % (p, r)]) + z["%s/%s_resid" % (p, r)]
            d[r + "_u8"] = z["%s/%s_u8" % (p, r)]
        for a in d.values():
            a.setflags(write=False)
        out[p] = d
    return out


def tie_mask(ref):
    """where value * 255 lies within TIE of a half-integer: the bytes that one float32 rounding may move"""
    v = np.asarray(ref, dtype=np.float64) * 255
    return np.abs(v - np.floor(v) - 0.5) <= TIE


def exact_moments(img_u8):
    """mean[3] and cov[3][3] (ddof 1) of the image k / 255 as fractions.Fraction, from Python integers:
    mean_i = S_i / (255 N), cov_ij = (N P_ij - S_i S_j) / (N (N - 1) 255^2)."""
    k = np.asarray(img_u8).reshape(-1, 3).astype(np.int64)
    n = int(k.shape[0])
    s = [int(k[:, i].sum()) for i in range(3)]
    p = [[int((k[:, i] * k[:, j]).sum()) for j in range(3)] for i in range(3)]
    mean = [Fraction(s[i], 255 * n) for i in range(3)]
    cov = [[Fraction(n * p[i][j] - s[i] * s[j], n * (n - 1) * 255 * 255) for j in range(3)] for i in range(3)]
    return mean, cov


def rel_error(got, exact):
    """|got - exact| / |exact| of a double against a Fraction, itself exact until the final float(); an exact 0 must be 0.0"""
    if exact == 0:
        return 0.0 if got == 0.0 else float("inf")
    return float(abs(Fraction(float(got)) - exact) / abs(exact))


@functools.lru_cache(maxsize=None)
def frames(n_pixels, batch, seed=0):
    """seeded uint8 frames [batch, n_pixels, 1, 3] with unequal channel spreads (a well-conditioned covariance)"""
    rng = np.random.default_rng(1000 * n_pixels + 10 * batch + seed)
    x = rng.random((batch, n_pixels, 1, 3)) * np.array([0.9, 0.6, 0.4]) + 0.2 * rng.random((batch, n_pixels, 1, 1)) + np.array([0.0, 0.2, 0.1])
    a = np.clip(np.rint(x * 255), 0, 255).astype(np.uint8)
    a.setflags(write=False)
    return a
