"""The 8-bit Y'CbCr 4:2:0 <-> RGB rule of csrc/yuv.hip restated in int64 numpy (the oracle of tests/test_yuv_*.py), the same
rule once more per sample in fractions.Fraction, and frame builders.

Both directions are the correctly rounded value (ties to even) of an exact rational expression (include/ct_hip.h), so the
oracle is exact: `rint_div` rounds an integer quotient without ever leaving the integers."""
from fractions import Fraction

import numpy as np

MATRICES = {"bt601": (1000, 299, 114), "bt709": (10000, 2126, 722)}            # D, kr, kb
RANGES = {"limited": (16, 219, 224, 235, 240), "full": (0, 255, 255, 255, 255)}  # Yoff, Ys, Cs, Ymax, Cmax
SITINGS = ("center", "left")
CONFIGS = [(m, r, s) for m in ("bt601", "bt709") for r in ("limited", "full") for s in SITINGS]


def frame_bytes(h, w):
    return h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2)


def rint_div(n, d):
    """rint(n / d), ties to even, for int64 arrays n and an integer d > 0"""
    n = np.asarray(n, dtype=np.int64)
    q, r = np.divmod(2 * n + d, 2 * d)
    return q - ((r == 0) & (q % 2 == 1))


def planes(yuv, h, w):
    """[n, >= frame_bytes] uint8 -> Y [n,h,w], Cb, Cr [n,ch,cw] as int64"""
    ch, cw = (h + 1) // 2, (w + 1) // 2
    yuv = np.asarray(yuv)
    y = yuv[:, :h * w].reshape(-1, h, w).astype(np.int64)
    cb = yuv[:, h * w:h * w + ch * cw].reshape(-1, ch, cw).astype(np.int64)
    cr = yuv[:, h * w + ch * cw:h * w + 2 * ch * cw].reshape(-1, ch, cw).astype(np.int64)
    return y, cb, cr


def _taps(n_luma, n_chroma, kind):
    """per luma index: two chroma indices (clamped) and their weights; "center" weights in quarters (1, 3), "left" in quarters too
    (4 alone, or 2 and 2)"""
    x = np.arange(n_luma)
    j = x // 2
    odd = x % 2 == 1
    if kind == "center":       # chroma j sits at luma 2j + 1/2
        a, b = np.where(odd, j, j - 1), np.where(odd, j + 1, j)
        wa, wb = np.where(odd, 3, 1), np.where(odd, 1, 3)
    else:                      # chroma j sits at luma 2j
        a, b = j, np.where(odd, j + 1, j)
        wa, wb = np.where(odd, 2, 4), np.where(odd, 2, 0)
    return np.clip(a, 0, n_chroma - 1), np.clip(b, 0, n_chroma - 1), wa.astype(np.int64), wb.astype(np.int64)


def _c16(c, h, w, siting, rows):
    """chroma plane [n,ch,cw] at the luma positions of `rows` x all columns, in sixteenths"""
    ya, yb, wya, wyb = _taps(h, c.shape[1], "center")
    xa, xb, wxa, wxb = _taps(w, c.shape[2], siting)
    ya, yb, wya, wyb = ya[rows], yb[rows], wya[rows, None], wyb[rows, None]
    top = c[:, ya][:, :, xa] * wxa + c[:, ya][:, :, xb] * wxb
    bot = c[:, yb][:, :, xa] * wxa + c[:, yb][:, :, xb] * wxb
    return top * wya + bot * wyb


def decode_oracle(yuv, h, w, matrix, range_, siting, band=64):
    """packed I420 frames [n, >= frame_bytes] uint8 -> uint8 [n,h,w,3]"""
    d, kr, kb = MATRICES[matrix]
    kg = d - kr - kb
    yoff, ys, cs = RANGES[range_][:3]
    y, cb, cr = planes(yuv, h, w)
    out = np.empty((y.shape[0], h, w, 3), dtype=np.uint8)
    den_rb, den_g = 8 * ys * cs * d, 8 * ys * cs * d * kg
    for r0 in range(0, h, band):
        r1 = min(h, r0 + band)
        rows = np.arange(r0, r1)
        yd = y[:, r0:r1] - yoff
        cbd, crd = _c16(cb, h, w, siting, rows) - 2048, _c16(cr, h, w, siting, rows) - 2048
        nr = 8 * cs * d * yd + (d - kr) * ys * crd
        nb = 8 * cs * d * yd + (d - kb) * ys * cbd
        ng = 8 * cs * d * kg * yd - kb * (d - kb) * ys * cbd - kr * (d - kr) * ys * crd
        for k, (n_, den) in enumerate(((nr, den_rb), (ng, den_g), (nb, den_rb))):
            out[:, r0:r1, :, k] = rint_div(255 * np.clip(n_, 0, den), den)
    return out


def _footprint_sums(rgb, siting):
    """uint8 [n,h,w,3] -> (S [n,ch,cw,3] int64, total weight): the weighted sums over each chroma sample's footprint"""
    n, h, w, _ = rgb.shape
    ch, cw = (h + 1) // 2, (w + 1) // 2
    x = rgb.astype(np.int64)
    i, j = np.arange(ch), np.arange(cw)
    r0, r1 = np.minimum(2 * i, h - 1), np.minimum(2 * i + 1, h - 1)
    v = x[:, r0] + x[:, r1]
    c0, c1 = np.minimum(2 * j, w - 1), np.minimum(2 * j + 1, w - 1)
    if siting == "center":
        return v[:, :, c0] + v[:, :, c1], 4
    cm = np.clip(2 * j - 1, 0, w - 1)
    return v[:, :, cm] + 2 * v[:, :, c0] + v[:, :, c1], 8


def encode_oracle(rgb, matrix, range_, siting):
    """uint8 [n,h,w,3] -> packed I420 frames [n, frame_bytes] uint8"""
    d, kr, kb = MATRICES[matrix]
    kg = d - kr - kb
    yoff, ys, cs, ymax, cmax = RANGES[range_]
    rgb = np.asarray(rgb)
    n, h, w, _ = rgb.shape
    x = rgb.astype(np.int64)
    y = np.clip(yoff + rint_div(ys * (kr * x[..., 0] + kg * x[..., 1] + kb * x[..., 2]), 255 * d), yoff, ymax)
    s, wt = _footprint_sums(rgb, siting)
    lum = kr * s[..., 0] + kg * s[..., 1] + kb * s[..., 2]
    cb = np.clip(128 + rint_div(cs * (d * s[..., 2] - lum), 510 * wt * (d - kb)), yoff, cmax)
    cr = np.clip(128 + rint_div(cs * (d * s[..., 0] - lum), 510 * wt * (d - kr)), yoff, cmax)
    return np.concatenate([y.reshape(n, -1), cb.reshape(n, -1), cr.reshape(n, -1)], axis=1).astype(np.uint8)


# ---- the same rule per sample, straight from its statement, in exact fractions ------------------------------------------------
def _k(matrix):
    d, kr, kb = MATRICES[matrix]
    kr, kb = Fraction(kr, d), Fraction(kb, d)
    return kr, kb, 1 - kr - kb


def decode_fraction(y, cb16, cr16, matrix, range_):
    """one pixel from its luma byte and its interpolated chroma in sixteenths -> (R, G, B); round() of a Fraction ties to even"""
    kr, kb, kg = _k(matrix)
    yoff, ys, cs = RANGES[range_][:3]
    yp = Fraction(y - yoff, ys)
    cbp, crp = Fraction(cb16 - 2048, 16 * cs), Fraction(cr16 - 2048, 16 * cs)
    vals = (yp + 2 * (1 - kr) * crp, yp - (2 * kb * (1 - kb) / kg) * cbp - (2 * kr * (1 - kr) / kg) * crp, yp + 2 * (1 - kb) * cbp)
    return tuple(int(round(255 * min(max(v, 0), 1))) for v in vals)


def encode_luma_fraction(r, g, b, matrix, range_):
    kr, kb, kg = _k(matrix)
    yoff, ys, _, ymax, _ = RANGES[range_]
    return min(max(int(round(yoff + ys * (kr * r + kg * g + kb * b) / 255)), yoff), ymax)


def encode_chroma_fraction(rm, gm, bm, matrix, range_):
    """(Cb, Cr) from the exact footprint means (Fractions)"""
    kr, kb, kg = _k(matrix)
    yoff, _, cs, _, cmax = RANGES[range_]
    ym = kr * rm + kg * gm + kb * bm
    cb = int(round(128 + cs * (bm - ym) / (255 * 2 * (1 - kb))))
    cr = int(round(128 + cs * (rm - ym) / (255 * 2 * (1 - kr))))
    return min(max(cb, yoff), cmax), min(max(cr, yoff), cmax)


# ---- frame builders ---------------------------------------------------------------------------------------------------------------
def random_yuv(rng, n, h, w):
    """every byte value, nominal range or not"""
    return rng.integers(0, 256, (n, frame_bytes(h, w)), dtype=np.uint8)


def random_rgb(rng, n, h, w):
    return rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def triple_frames():
    """two 4096 x 4096 I420 frames that together hold every (Y, Cb, Cr) triple with unblended chroma: 16 x 16 luma tiles, Cb the
    tile row, Cr the tile column, Y running 0..255 inside the tile; the second frame has the luma pattern rolled by (8, 8), so the
    positions at a tile's rim (blended chroma) in one frame are interior in the other"""
    t = np.arange(256, dtype=np.uint8).reshape(16, 16)
    out = []
    for roll in (0, 8):
        y = np.tile(np.roll(t, (roll, roll), axis=(0, 1)), (256, 256))
        cb = np.repeat(np.repeat(np.arange(256, dtype=np.uint8)[:, None], 8, axis=0), 2048, axis=1)
        cr = np.repeat(np.repeat(np.arange(256, dtype=np.uint8)[None, :], 8, axis=1), 2048, axis=0)
        out.append(np.concatenate([y.reshape(-1), cb.reshape(-1), cr.reshape(-1)]))
    return np.stack(out)


def colour_cube_blocks(lo, hi):
    """the colours with red in [lo, hi) as constant 2 x 2 blocks: uint8 [hi - lo, 512, 512, 3] (frame = red, block row = green,
    block column = blue) and the colours themselves [hi - lo, 256, 256, 3]"""
    r, g, b = np.meshgrid(np.arange(lo, hi, dtype=np.uint8), np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8),
                          indexing="ij")
    colours = np.stack([r, g, b], axis=-1)
    return np.repeat(np.repeat(colours, 2, axis=1), 2, axis=2), colours


def write_y4m(path, frames_yuv, w, h, tag="C420jpeg", extra="", frame_params=""):
    """a Y4M file from packed I420 frames [n, frame_bytes]"""
    with open(path, "wb") as f:
        f.write(("YUV4MPEG2 W%d H%d F25:1 Ip A1:1%s%s\n" % (w, h, " " + tag if tag else "", " " + extra if extra else "")).encode())
        for fr in np.asarray(frames_yuv):
            f.write(b"FRAME" + frame_params.encode() + b"\n")
            f.write(fr.tobytes())
