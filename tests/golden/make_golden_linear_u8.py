#!/opt/conda/bin/python3.9 -B
"""Generate the golden vectors of the uint8 MK / Xiao path by running the REAL reference on k / 255.

Run in the build container only (never on the GPU box):

    /opt/conda/bin/python3.9 -B tests/golden/make_golden_linear_u8.py

The reference module is loaded by file path so that ``methods/__init__.py`` (pytorch_lightning, piq) is bypassed; it imports
``skimage.color`` (methods/linear.py:5), hence the interpreter.  Only inputs/outputs (data) are written; no reference source is
copied.

Output: tests/golden/linear_u8.npz -- three seeded uint8 pairs (37x53, 1x257, 64x48 with a target that is a hue-shifted copy of
the reference) and per pair
    <pair>/mk_<d>      monge_kantorovitch_color_transfer(t / 255.0, r / 255.0, d), d in MK, sqrt, cholesky, float64
    <pair>/xiao        color_transfer_in_correlated_color_space(t / 255.0, r / 255.0), float64
    <pair>/<name>_u8   rint(clip(., 0, 1) * 255) of each as uint8
A float64 result is kept whole, bit for bit, in a form that compresses: every result is an affine map of the target, so the file
holds <name>_coef, a least-squares fit [4, 3], and <name>_resid = result - predict(target, coef), a few units in the last place.
predict() uses elementwise products and sums only (no BLAS), which IEEE arithmetic fixes, so predict + resid is the result again
exactly (asserted here); tests/linear_u8_common.py: fixture() puts them together.  The file stays below 300 KB that way.
Only the sum is reproducible: np.linalg.lstsq may give a fit that differs at the 1e-15 level from run to run, and the residual
moves with it, so a regenerated file holds other _coef and _resid arrays that add up to the same float64 results.
The byte test (tests/test_linear_u8_gpu.py) leaves out the values whose value * 255 lies within TIE of a half-integer; this
script asserts that they are at most MAX_TIE_SHARE of any stored result (another seed otherwise).
"""
import importlib.util
import os
import sys
import warnings

import numpy as np

REF = "/root/reference/methods/linear.py"
OUT = os.path.dirname(os.path.abspath(__file__))
TIE = 1e-4
MAX_TIE_SHARE = 1e-3
DECOMPS = ("MK", "sqrt", "cholesky")

spec = importlib.util.spec_from_file_location("ref_linear", REF)
lin = importlib.util.module_from_spec(spec)
spec.loader.exec_module(lin)
import scipy  # noqa: E402
import skimage  # noqa: E402

META = dict(numpy=np.__version__, scipy=scipy.__version__, skimage=skimage.__version__, python=sys.version.split()[0])


def textured(rng, h, w, gains, offsets, common):
    """uint8 noise with unequal channel spreads and a shared component: a covariance with three distinct eigenvalues"""
    shared = rng.random((h, w, 1))
    x = rng.random((h, w, 3)) * np.asarray(gains) + common * shared + np.asarray(offsets)
    return np.clip(np.rint(x * 255), 0, 255).astype(np.uint8)


def hue_shift(img_u8, degrees):
    """rotate the chroma plane of YIQ by `degrees`, back to RGB, rounded to bytes"""
    to_yiq = np.array([[0.299, 0.587, 0.114], [0.5959, -0.2746, -0.3213], [0.2115, -0.5227, 0.3112]])
    a = np.deg2rad(degrees)
    rot = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    m = np.linalg.inv(to_yiq) @ rot @ to_yiq
    return np.clip(np.rint(img_u8.astype(np.float64) @ m.T), 0, 255).astype(np.uint8)


def pairs():
    rng = np.random.default_rng(20261019)
    out = {}
    out["p37x53"] = (textured(rng, 37, 53, (0.9, 0.6, 0.4), (0.02, 0.2, 0.1), 0.15),
                     textured(rng, 37, 53, (0.5, 0.7, 0.35), (0.3, 0.05, 0.4), 0.25))
    out["p1x257"] = (textured(rng, 1, 257, (0.7, 0.8, 0.5), (0.1, 0.0, 0.3), 0.2),
                     textured(rng, 1, 257, (0.4, 0.5, 0.8), (0.35, 0.2, 0.0), 0.1))
    yy, xx = np.mgrid[0:64, 0:48].astype(np.float64)
    base = np.stack([0.5 + 0.4 * np.sin(xx / 48 * 3.1 + 0.3) * np.cos(yy / 64 * 2.2), (xx / 48) * 0.7 + 0.15 * (yy / 64),
                     0.5 + 0.4 * np.cos((xx + 2 * yy) / 112 * 5.0)], axis=-1)
    r = np.clip(np.rint((base + 0.06 * rng.standard_normal(base.shape)) * 255), 0, 255).astype(np.uint8)
    out["p64x48_hue"] = (hue_shift(r, 40.0), r)
    return out


def predict(t8, coef):
    """the affine map `coef` of t8 / 255.0 in float64, elementwise operations in a fixed order (tests/linear_u8_common.py has the
    same function)"""
    x = t8.astype(np.float64) / 255.0
    return np.stack([((x[..., 0] * coef[0, j] + x[..., 1] * coef[1, j]) + x[..., 2] * coef[2, j]) + coef[3, j] for j in range(3)], axis=-1)


def tie_share(x):
    v = np.asarray(x, dtype=np.float64) * 255
    return float(np.mean(np.abs(v - np.floor(v) - 0.5) <= TIE))


def main():
    keep = {}
    for name, (t8, r8) in pairs().items():
        assert t8.dtype == np.uint8 and r8.dtype == np.uint8
        keep[name + "/target"], keep[name + "/reference"] = t8, r8
        t, r = t8 / 255.0, r8 / 255.0
        res = {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for d in DECOMPS:
                res["mk_" + d] = lin.monge_kantorovitch_color_transfer(t, r, d)
            res["xiao"] = lin.color_transfer_in_correlated_color_space(t, r)
        for k, v in res.items():
            v = np.real(v)
            assert v.dtype == np.float64 and v.shape == t8.shape and np.isfinite(v).all(), (name, k)
            share = tie_share(v)
            assert share <= MAX_TIE_SHARE, "%s/%s: %.3f %% of the values within %g of a tie: choose another seed" % (name, k, 100 * share, TIE)
            design = np.concatenate([t.reshape(-1, 3), np.ones((t.size // 3, 1))], axis=1)
            coef = np.linalg.lstsq(design, v.reshape(-1, 3), rcond=None)[0]
            resid = v - predict(t8, coef)
            assert np.array_equal(predict(t8, coef) + resid, v) and np.abs(resid).max() < 1e-13, (name, k)
            keep[name + "/" + k + "_coef"], keep[name + "/" + k + "_resid"] = coef, resid
            keep[name + "/" + k + "_u8"] = np.rint(np.clip(v, 0, 1) * 255).astype(np.uint8)
            print("%-12s %-12s range %.3f .. %.3f  ties %.4f %%  clipped %.1f %%"
                  % (name, k, v.min(), v.max(), 100 * share, 100 * np.mean((v < 0) | (v > 1))))
    path = os.path.join(OUT, "linear_u8.npz")
    np.savez_compressed(path, meta=str(META), **keep)
    assert os.path.getsize(path) < 300 * 1024
    print("wrote %s (%d bytes) with %s" % (path, os.path.getsize(path), META))


if __name__ == "__main__":
    main()
