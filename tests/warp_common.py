"""Shared by tests/test_warp_host.py and tests/test_warp_gpu.py: the numpy restatement of ct_warp_perspective_u8's rule
(include/ct_hip.h; OpenCV's fixed-point bilinear warpPerspective, INTER_BITS = 5), a float64 oracle with exact coordinates and true
bilinear weights, and the per-pixel bound between the two.

The bound is derived, not tuned: the rule rounds the source coordinate to 1/32 px, so it is off by at most 1/64 px per axis; its
fixed-point weights a * b / 1024 are exact for that rounded coordinate; the final shift rounds an exact weighted sum to the nearest
integer (0.5).  A bilinear surface moves by at most D per pixel of displacement along an axis, D the largest difference between
neighbours along that axis among the pixels the two samples can touch -- the 4 x 4 block around the exact sample.  So
    |out - exact| <= 0.5 + (Dx + Dy) / 64 + 1e-6
with Dx, Dy taken over the zero-padded crop (the 1e-6 covers the float64 evaluation of the oracle itself)."""
import numpy as np

SHAPES = ((37, 101), (16, 64), (9, 130))          # (height, width): odd sizes, exactly cv2's block, bh0 < 16 with two x0 blocks

IDENTITY = np.eye(3)


def near_identity(h, w):
    """destination -> source: a small rotation, shear, shift and perspective term; W stays near 1 over the frame"""
    return np.array([[1.01, 0.02, -1.3], [-0.015, 0.99, 0.8], [2e-5 * 100.0 / w, -1e-5 * 100.0 / h, 1.0]])


def strong(h, w):
    """a 2.3-fold reduction with rotation and a perspective term that moves W by tens of percent over the frame: the source box of
    a 64 x 16 tile is ~150 x 100 pixels, more than the staged path's LDS holds once the image is that large"""
    return np.array([[2.3, 0.9, -0.3 * w], [-0.8, 2.1, 0.1 * h], [1.5e-3, 2.5e-3, 1.0]])


def images(h, w, seed=0):
    """a smooth and a noise image, uint8 [h, w, 3]"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.stack([127.5 + 127.5 * np.sin(0.11 * xx + 0.07 * yy + k) for k in range(3)], axis=-1)
    return {"smooth": np.rint(smooth).astype(np.uint8), "noise": rng.integers(0, 256, (h, w, 3), dtype=np.uint8)}


def source_crop(raw, crop=None, flip_x=False):
    """the source image of the warp: the crop (x, y, w, h) of the -- possibly mirrored -- raw frame [H, W, 3]"""
    img = raw[:, ::-1] if flip_x else raw
    if crop is None:
        return img
    x, y, w, h = crop
    return img[y:y + h, x:x + w]


def _taps(src, sy, sx):
    """src[sy, sx] as int64 [.., 3], 0 outside the image"""
    h, w = src.shape[:2]
    inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    v = src[np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)].astype(np.int64)
    return v * inside[..., None]


def warp_fixed(src, m, window=None):
    """The rule on one source image uint8 [h, w, 3] with the destination -> source matrix m (9 values): uint8 [wh, ww, 3], the
    window (x, y, w, h) of the h x w destination (default: all of it).  Every float64 operation below is one numpy operation,
    left to right, as the header orders them."""
    m = np.asarray(m, dtype=np.float64).reshape(9)
    h, w = src.shape[:2]
    ox, oy, ow, oh = window if window is not None else (0, 0, w, h)
    bh0 = min(16, h)
    bw0 = min(1024 // bh0, w)
    c = np.arange(ox, ox + ow, dtype=np.int64)[None, :]
    r = np.arange(oy, oy + oh, dtype=np.int64)[:, None].astype(np.float64)
    x0i = (c // bw0) * bw0
    x0, x1 = x0i.astype(np.float64), (c - x0i).astype(np.float64)
    with np.errstate(all="ignore"):
        X0 = m[0] * x0 + m[1] * r + m[2]
        Y0 = m[3] * x0 + m[4] * r + m[5]
        W0 = m[6] * x0 + m[7] * r + m[8]
        W = W0 + m[6] * x1
        W = np.where(W != 0, 32.0 / np.where(W != 0, W, 1.0), 0.0)
        fX = np.maximum(-2.0 ** 31, np.minimum(2.0 ** 31 - 1, (X0 + m[0] * x1) * W))
        fY = np.maximum(-2.0 ** 31, np.minimum(2.0 ** 31 - 1, (Y0 + m[3] * x1) * W))
    X, Y = np.rint(fX).astype(np.int64), np.rint(fY).astype(np.int64)
    sx, sy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
    a, b = (X & 31)[..., None], (Y & 31)[..., None]
    acc = ((32 - a) * (32 - b) * _taps(src, sy, sx) + a * (32 - b) * _taps(src, sy, sx + 1)
           + (32 - a) * b * _taps(src, sy + 1, sx) + a * b * _taps(src, sy + 1, sx + 1) + 512) >> 10
    return acc.astype(np.uint8)


def warp_frames(raw, maps, crop=None, flip_x=False, window=None):
    """warp_fixed on a batch uint8 [B, H, W, 3]; maps [9] / [3, 3] (shared) or [B, 9] / [B, 3, 3]: what ct_hip.warp_perspective
    computes with inverse_map=True"""
    maps = np.asarray(maps, dtype=np.float64)
    maps = np.broadcast_to(maps.reshape(-1, 9), (raw.shape[0], 9))
    return np.stack([warp_fixed(source_crop(f, crop, flip_x), k, window) for f, k in zip(raw, maps)])


def warp_exact(src, m):
    """float64 oracle: (exact sample [h, w, 3], bound [h, w, 3]) for the whole destination.  Coordinates
    u = (M0 c + M1 r + M2) / (M6 c + M7 r + M8), v likewise, true bilinear weights, taps outside the image 0."""
    m = np.asarray(m, dtype=np.float64).reshape(9)
    h, w = src.shape[:2]
    c = np.arange(w, dtype=np.float64)[None, :]
    r = np.arange(h, dtype=np.float64)[:, None]
    den = m[6] * c + m[7] * r + m[8]
    u, v = (m[0] * c + m[1] * r + m[2]) / den, (m[3] * c + m[4] * r + m[5]) / den
    fu, fv = np.floor(u), np.floor(v)
    du, dv = (u - fu)[..., None], (v - fv)[..., None]
    # far outside, everything is 0: keep the integer parts in a range where the padded lookups below stay valid
    iu, iv = np.clip(fu, -4, w + 3).astype(np.int64), np.clip(fv, -4, h + 3).astype(np.int64)
    f = src.astype(np.float64)

    def tap(yy, xx):
        inside = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        return f[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)] * inside[..., None]
    exact = ((1 - du) * (1 - dv) * tap(iv, iu) + du * (1 - dv) * tap(iv, iu + 1)
             + (1 - du) * dv * tap(iv + 1, iu) + du * dv * tap(iv + 1, iu + 1))
    # Dx, Dy over the 4 x 4 block (columns iu - 1 .. iu + 2, rows iv - 1 .. iv + 2) of the zero-padded image
    pad = 8
    p = np.zeros((h + 2 * pad, w + 2 * pad, 3))
    p[pad:pad + h, pad:pad + w] = f
    gx = np.abs(np.diff(p, axis=1))                  # gx[y, x] = |p[y, x + 1] - p[y, x]|
    gy = np.abs(np.diff(p, axis=0))
    dx, dy = np.zeros_like(exact), np.zeros_like(exact)
    for j in range(4):
        for i in range(3):
            dx = np.maximum(dx, gx[iv + pad - 1 + j, iu + pad - 1 + i])
            dy = np.maximum(dy, gy[iv + pad - 1 + i, iu + pad - 1 + j])
    return exact, 0.5 + (dx + dy) / 64.0 + 1e-6
