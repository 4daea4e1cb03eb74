"""What tests/test_icid_options_host.py and tests/test_icid_options_gpu.py share: a torch restatement of the reference's
utils.icid.icid(img1, img2, intent, omit_maps67, downsampling) with all three arguments -- oracle.metrics.icid is the default call
only, and stays as it is --, the option combinations, the golden tables and the frames of the edge cases.

The restatement is oracle.metrics.icid's statements with the weights of utils/icid.py:42-47, maps 6 and 7 left out of the product
when omit_maps67 (the reference raises them to the power 0, which is exactly 1) and the resize skipped when not downsampling.  At
the defaults it is bitwise oracle.metrics.icid; with options it is pinned by tests/golden/icid_options.npz, runs of the reference's
own file (tests/golden/make_golden_icid_options.py)."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import metrics as om
from tests.test_metrics import _pair as pair          # the smooth-field-plus-noise frames of tests/test_metrics.py

INTENTS = ("perceptual", "hue-preserving", "chromatic")
OMIT = (False, True)
DOWN = (True, False)
# (intent, omit_maps67, downsampling) and its index in a golden table [3][2][2]
COMBOS = tuple(((i, o, d), (ii, oi, di)) for ii, i in enumerate(INTENTS) for oi, o in enumerate(OMIT) for di, d in enumerate(DOWN))
WEIGHTS = {"perceptual": [0.002, 10, 10, 0.002, 0.002, 10, 10], "hue-preserving": [0.002, 10, 10, 0.002, 0.02, 10, 10],
           "chromatic": [0.002, 10, 10, 0.02, 0.02, 10, 10]}
BAD_INTENT = "Intent should be either 'perceptual', 'hue-preserving', or 'chromatic'"
ATOL = 5e-6                                            # tests/metrics_edges_common.py ATOL["icid"]: device against float64
K_F32 = 2                                              # ... K_FLAT["icid"]: |device - f64| <= max(ATOL, 2 |restatement f32 - f64|)


def icid(img1, img2, intent="perceptual", omit_maps67=False, downsampling=True, dtype=torch.float64):
    """utils/icid.py:28-152 -> scalar (mean over the batch and positions); dtype=torch.float32: the reference as it runs"""
    if intent not in WEIGHTS:
        raise ValueError(BAD_INTENT)
    img1, img2 = img1.to(dtype), img2.to(dtype)
    # torch.tensor([...]) -> float32 weights whatever the dtype of the images (utils/icid.py:43-47)
    w = [float(v) for v in torch.tensor(WEIGHTS[intent], dtype=torch.float32)]
    h, wd = img1.shape[-2:]
    f = om.metric_factor(h, wd) if downsampling else 1
    if f > 1:
        img1 = F.interpolate(img1, scale_factor=1 / f, mode="bilinear")
        img2 = F.interpolate(img2, scale_factor=1 / f, mode="bilinear")
    img1, img2 = om.rgb_to_lab(img1), om.rgb_to_lab(img2)
    L1, A1, B1 = img1[..., 0, :, :], img1[..., 1, :, :], img1[..., 2, :, :]
    L2, A2, B2 = img2[..., 0, :, :], img2[..., 1, :, :], img2[..., 2, :, :]
    C1, C2 = torch.sqrt(A1 ** 2 + B1 ** 2), torch.sqrt(A2 ** 2 + B2 ** 2)
    ks, sg = [11, 11], [2.0, 2.0]
    blur = lambda t: om.gaussian_blur(t, ks, sg)     # noqa: E731
    muL1, muC1, muL2, muC2 = blur(L1), blur(C1), blur(L2), blur(C2)
    sL1q = (blur(L1 ** 2) - muL1 ** 2).clamp(min=0)
    sL2q = (blur(L2 ** 2) - muL2 ** 2).clamp(min=0)
    sC1q = (blur(C1 ** 2) - muC1 ** 2).clamp(min=0)
    sC2q = (blur(C2 ** 2) - muC2 ** 2).clamp(min=0)
    sL1, sL2, sC1, sC2 = sL1q.sqrt(), sL2q.sqrt(), sC1q.sqrt(), sC2q.sqrt()
    dLq, dCq = (muL1 - muL2) ** 2, (muC1 - muC2) ** 2
    H = ((A1 - A2) ** 2 + (B1 - B2) ** 2 - (C1 - C2) ** 2).clamp(min=0)
    dHq = blur(torch.sqrt(H)) ** 2
    sL12 = blur(L1 * L2) - muL1 * muL2
    sC12 = blur(C1 * C2) - muC1 * muC2
    maps = [1 / (w[0] * dLq + 1), (w[1] + 2 * sL1 * sL2) / (w[1] + sL1q + sL2q), ((w[2] + sL12.abs()) / (w[2] + sL1 * sL2)) ** 3,
            1 / (w[3] * dCq + 1), 1 / (w[4] * dHq + 1), (w[5] + 2 * sC1 * sC2) / (w[5] + sC1 ** 2 + sC2 ** 2),
            (w[6] + sC12.abs()) / (w[6] + sC1 * sC2)]
    if omit_maps67:
        maps = maps[:5]
    prod = maps[0]
    for m in maps[1:]:
        prod = prod * m
    return 1 - prod.mean()


def per_frame(x, y, intent, omit, down, dtype=torch.float64):
    """the restatement one frame at a time -> float64 [B]"""
    return torch.stack([icid(x[i:i + 1], y[i:i + 1], intent, omit, down, dtype=dtype).double() for i in range(x.shape[0])])


def golden_frames(golden_dir):
    """tag -> (x, y) float32 [B,3,H,W]: pairs a-d of icid.npz and the batch of two 48 x 64 pairs (a, the top left corner of b)"""
    g = np.load(os.path.join(golden_dir, "icid.npz"), allow_pickle=False)
    u8 = lambda a: torch.from_numpy(a.astype(np.float32) / np.float32(255))      # noqa: E731
    frames = {tag: (u8(g[tag + "/x_u8"]), u8(g[tag + "/y_u8"])) for tag in "abcd"}
    frames["batch"] = tuple(torch.cat([frames["a"][k], frames["b"][k][..., :48, :64]]).contiguous() for k in (0, 1))
    return frames


def golden_values(golden_dir):
    g = np.load(os.path.join(golden_dir, "icid_options.npz"), allow_pickle=False)
    assert tuple(str(s) for s in g["intents"]) == INTENTS
    return g


# (batch, H, W): the smallest grid, two frames of 2 x 2 tiles, one past a tile both ways, and two sizes with f = 2 whose full-size
# grid has many more tiles (and a larger workspace) than the down-sampled one
EDGE_SHAPES = ((1, 6, 6), (2, 37, 53), (1, 17, 33), (1, 385, 387), (1, 640, 644))
EDGE_OPTIONS = (("chromatic", True), ("hue-preserving", False))
_edge = {}


def edge_case(shape):
    """(x, y, {(intent, omit, down): (f64 [B], f32 [B])}) of one edge shape, made once and never changed"""
    if shape not in _edge:
        b, h, w = shape
        x, y = pair(h * 3 + w, b, h, w)
        ref = {(i, o, d): (per_frame(x, y, i, o, d), per_frame(x, y, i, o, d, dtype=torch.float32)) for i, o in EDGE_OPTIONS for d in DOWN}
        _edge[shape] = (x, y, ref)
    return _edge[shape]
