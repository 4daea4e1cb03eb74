"""What the view tests share: the inputs of tests/golden/views.npz (made from integer arithmetic and IEEE + - * / only, so every
machine builds the same bits; the file holds their digests and the reference's outputs) and numpy restatements of the three
contracts of csrc/views.hip.  tests/test_views_host.py pins the restatements to the reference's outputs; the GPU tests use them at
shapes the file does not hold.  Not product code."""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "views.npz")
FLOW_CASES = ("amp0.5", "amp20", "zero", "unknown", "amp300")         # four of 37 x 53 and one of 96 x 160


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def hash_u32(shape, seed):
    """a portable stream of 32-bit integers: a multiplicative hash of the element index, two xorshift-multiply rounds"""
    n = int(np.prod(shape))
    x = (np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    for mul in (0x85EBCA6B, 0xC2B2AE35):
        x ^= x >> np.uint64(16)
        x = (x * np.uint64(mul)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32).reshape(shape)


def uniform(shape, seed):
    """float32 in [0, 1) on the 2^-24 grid"""
    return ((hash_u32(shape, seed) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def chess_inputs(b=1, c=1, h=60, w=77):
    """x counts its elements upwards from 0, y downwards from -1: every element of the two is distinct, so a copy from a wrong
    place or source cannot pass"""
    x = np.arange(b * c * h * w, dtype=np.float32).reshape(b, c, h, w)
    return x, (-x - np.float32(1)).astype(np.float32)


def rgbmse_inputs(shape=(2, 3, 41, 67)):
    # the second frame's error is scaled down: the frames of a batch have different extremes
    x, y = uniform(shape, 11), uniform(shape, 12)
    y[1:] = (x[1:] + (y[1:] - x[1:]) * np.float32(0.25)).astype(np.float32)
    return x, y


def flow_input(case):
    """[2, H, W] float32: a smooth rotation-plus-shear field with every direction in it, some noise, scaled to the case's amplitude"""
    h, w = (96, 160) if case == "amp300" else (37, 53)
    if case == "zero":
        return np.zeros((2, h, w), dtype=np.float32)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    cy, cx = np.float32(h / 2 - 0.25), np.float32(w / 2 + 0.25)
    amp = np.float32({"amp0.5": 0.5, "amp20": 20.0, "unknown": 20.0, "amp300": 300.0}[case])
    scale = np.float32(1.0 / max(h, w))
    seed = FLOW_CASES.index(case)
    noise = np.float32(0.01 if case == "amp300" else 0.05)               # the large case compresses better with less of it
    u = (-(yy - cy) + (xx - cx) * np.float32(0.25)) * scale + (uniform((h, w), 20 + seed) - np.float32(0.5)) * noise
    v = ((xx - cx) + (yy - cy) * (yy - cy) * scale * np.float32(0.5)) * scale + (uniform((h, w), 30 + seed) - np.float32(0.5)) * noise
    flow = (np.stack([u, v]) * amp).astype(np.float32)
    if case == "unknown":
        flow[0, 5, 7] = np.float32(1e8)
    return flow


def digest(*arrays):
    m = hashlib.sha1()
    for a in arrays:
        m.update(np.ascontiguousarray(a).tobytes())
    return m.hexdigest()


# ---- restatements -----------------------------------------------------------------------------------------------------------------
def chess_mix_ref(x, y, size=25):
    """utils/visualizations.py:9-21"""
    h, w = x.shape[-2:]
    pick = ((np.arange(h)[:, None] // size + np.arange(w)[None, :] // size) % 2) == 0
    return np.where(pick, x, y)


def minmaxscale_ref(m):
    """utils/visualizations.py:24-28 on [B,H,W] float32"""
    lo, hi = m.min(axis=(-1, -2), keepdims=True), m.max(axis=(-1, -2), keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        return ((m - lo) / (hi - lo)).astype(np.float32)


def rgbmse_ref(x, y):
    """utils/visualizations.py:31-36: the channels are added in their order, the sum is divided by 3 (float32 throughout)"""
    d = (x - y).astype(np.float32)
    m = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) / np.float32(3)
    out = np.zeros_like(x)
    out[:, 0] = minmaxscale_ref(m)
    return out


def gray_ref(x):
    """[B,1,H,W] -> [B,3,H,W]: minmaxscale in three channels"""
    return np.repeat(minmaxscale_ref(x[:, 0])[:, None], 3, axis=1)


def colorwheel():
    """flow_viz.py:134-181 from the six segment lengths"""
    wheel, col = np.zeros((55, 3)), 0
    for n, full, ramp, down in ((15, 0, 1, False), (6, 1, 0, True), (4, 1, 2, False), (11, 2, 1, True), (13, 2, 0, False), (6, 0, 2, True)):
        r = np.floor(255 * np.arange(0, n) / n)
        wheel[col:col + n, full] = 255
        wheel[col:col + n, ramp] = 255 - r if down else r
        col += n
    return wheel


def flow_to_image_ref(flow, parts=False, dtype=np.float64):
    """utils/flow_viz.py:184-264 on one [2,H,W] float32 flow -> [H,W,3] uint8, the same numpy calls in the precisions numpy >= 2
    gives them: float32 up to the maximum radius, float64 from the division by the float64 scalar `maxrad + eps` on.  NaN counts
    as unknown (the reference does not survive it).  dtype=np.float32 is what numpy < 2 computed (value-based casting kept the
    division, the radius, the angle and fk in float32).  parts: also the normalised radius and fk, for the knife-edge masks."""
    u, v = flow[0].astype(np.float32).copy(), flow[1].astype(np.float32).copy()
    with np.errstate(invalid="ignore"):
        unknown = ~((np.abs(u) <= 1e7) & (np.abs(v) <= 1e7))
    u[unknown] = 0
    v[unknown] = 0
    rad = np.sqrt(u ** 2 + v ** 2)
    maxrad = max(-1, np.max(rad))
    den = dtype(np.float64(maxrad) + np.finfo(float).eps)
    u, v = u.astype(dtype) / den, v.astype(dtype) / den
    wheel = colorwheel()
    ncols = 55
    rad = np.sqrt(u ** 2 + v ** 2)
    a = np.arctan2(-v, -u) / dtype(np.pi)
    fk = (a + 1) / 2 * (ncols - 1) + 1
    k0 = np.floor(fk).astype(int)
    k1 = k0 + 1
    k1[k1 == ncols + 1] = 1
    f = fk - k0                                                       # float64 in either mode
    img = np.zeros(u.shape + (3,), dtype=np.uint8)
    for i in range(3):
        tmp = wheel[:, i]
        col0, col1 = tmp[k0 - 1] / 255, tmp[k1 - 1] / 255
        col = (1 - f) * col0 + f * col1
        idx = rad <= 1
        col[idx] = 1 - rad[idx] * (1 - col[idx])
        col[~idx] *= 0.75
        img[:, :, i] = np.uint8(np.floor(255 * col))
    img[unknown] = 0
    return (img, rad, fk, unknown) if parts else img


def flow_gate(got, want, flow):
    """The comparison of a flow image computed with other roundings (a device atan2 / sqrt, float32) with the reference's bytes:
    (worst grey-level difference, share of differing pixels), both over the pixels OFF the knife edges.  On a knife edge either
    branch is allowed: a normalised radius >= 1 - 1e-5 (the frame's largest flow sits where `rad <= 1` switches to the x 0.75
    branch), or fk within 1e-4 of 1 or 55 (the wheel's seam)."""
    _, rad, fk, _ = flow_to_image_ref(flow, parts=True)
    edge = (rad >= 1 - 1e-5) | (np.abs(fk - 1) < 1e-4) | (np.abs(fk - 55) < 1e-4)
    diff = np.abs(got.astype(int) - want.astype(int)).max(axis=2)[~edge]
    return (int(diff.max()), float((diff > 0).mean())) if diff.size else (0, 0.0)
