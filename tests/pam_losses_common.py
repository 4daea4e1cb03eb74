"""The three parallax-attention losses of the reference's step (methods/dcmcs3di.py:75-77) restated in torch from their formulas, in
the dtype of their inputs (float64: the yardstick; float32: what the reference's own run computes), plus the seeded cases of
tests/golden/pam_losses.npz and the error rule of the GPU tests.  tests/test_pam_losses_host.py holds the restatement to the values
the real reference gave.

    masked L1        sum(|x - y| * mask) / sum(mask), the mask NOT broadcast in the denominator
    photometric      masked L1 of (left, att_r2l @ right, valid_left) + masked L1 of (right, att_l2r @ left, valid_right)
    cycle            masked L1 of (att_r2l @ att_l2r, I, valid_left) + masked L1 of (att_l2r @ att_r2l, I, valid_right)
    smoothness       for both maps: mean |att[h] - att[h+1]| + mean |att[i][j] - att[i+1][j+1]|   (an empty mean is NaN)
"""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pam_losses.npz")
LOSSES = ("photometric", "cycle", "smoothness")
# name -> ((B, H, W), mask override of the left view): the cases of tests/golden/pam_losses.npz
CASES = {
    "2x4x70": ((2, 4, 70), None),                  # two 32-tiles plus a ragged 6; rows not 16-byte aligned
    "1x3x33": ((1, 3, 33), None),                  # one past a tile
    "1x2x96": ((1, 2, 96), None),                  # whole tiles
    "1x1x40": ((1, 1, 40), None),                  # no vertical pair: NaN
    "1x2x1": ((1, 2, 1), None),                    # no diagonal pair: NaN
    "1x3x33_none_valid": ((1, 3, 33), "none"),     # an all-false left mask: NaN
    "1x3x33_one_valid": ((1, 3, 33), "one"),       # a count of one
}
FIELDS = ("att_r2l", "att_l2r", "left", "right", "valid_left", "valid_right")


def build_case(shape, seed, left_mask=None):
    """Seeded inputs: att_r2l / att_l2r float32 [B,H,W,W] = softmax of a cost peaked 3 columns off the diagonal (to either side) with
    noise, left / right float32 [B,3,H,W] images, valid_left / valid_right uint8 [B,1,H,W] = column sums of the OTHER map > 0.1 (the
    columns the peaks never reach are invalid).  left_mask: "none" = all false, "one" = a single valid pixel."""
    b, h, w = shape
    g = torch.Generator().manual_seed(seed)
    i = torch.arange(w, dtype=torch.float32).view(w, 1)
    j = torch.arange(w, dtype=torch.float32).view(1, w)
    atts = []
    for shift in (-3.0, 3.0):
        cost = -2.0 * (j - (i + shift)).abs() + torch.randn(b, h, w, w, generator=g)
        atts.append(torch.softmax(cost, dim=-1).contiguous())
    left = torch.rand(b, 3, h, w, generator=g)
    right = (left * 0.8 + 0.2 * torch.rand(b, 3, h, w, generator=g)).contiguous()
    valid_left = (atts[1].sum(dim=-2) > 0.1).unsqueeze(1)
    valid_right = (atts[0].sum(dim=-2) > 0.1).unsqueeze(1)
    if left_mask == "none":
        valid_left = torch.zeros_like(valid_left)
    elif left_mask == "one":
        valid_left = torch.zeros_like(valid_left)
        valid_left[0, 0, h - 1, w // 2] = True
    return dict(att_r2l=atts[0], att_l2r=atts[1], left=left, right=right, valid_left=valid_left.to(torch.uint8),
                valid_right=valid_right.to(torch.uint8))


def case_seed(name):
    return 1000 + sorted(CASES).index(name)


def load_golden():
    """{case: dict of torch tensors: the FIELDS, ref64 [3] and ref32 [3] (float64; LOSSES order)}"""
    z = np.load(GOLDEN)
    return {name: {k: torch.from_numpy(z["%s/%s" % (name, k)]) for k in FIELDS + ("ref64", "ref32")} for name in CASES}


def _as(case, dtype):
    att = (case["att_r2l"].to(dtype), case["att_l2r"].to(dtype))
    valid = (case["valid_left"].to(dtype), case["valid_right"].to(dtype))
    return case["left"].to(dtype), case["right"].to(dtype), att, valid


def masked_l1(x, y, mask):
    return ((x - y).abs() * mask).sum() / mask.sum()


def warp(image, att):
    """[B,C,H,W] under att [B,H,W,W]: out[c][h][i] = sum_j att[h][i][j] image[c][h][j]"""
    return torch.matmul(att, image.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)


def cycle_maps(att):
    return torch.matmul(att[0], att[1]), torch.matmul(att[1], att[0])


def photometric(left, right, att, valid):
    return masked_l1(left, warp(right, att[0]), valid[0]) + masked_l1(right, warp(left, att[1]), valid[1])


def cycle(att_cycle, valid):
    eye = torch.eye(att_cycle[0].shape[-1], dtype=att_cycle[0].dtype, device=att_cycle[0].device)
    return sum(masked_l1(c, eye, v.permute(0, 2, 3, 1)) for c, v in zip(att_cycle, valid))


def smoothness(att):
    return sum((a[:, :-1] - a[:, 1:]).abs().mean() + (a[:, :, :-1, :-1] - a[:, :, 1:, 1:]).abs().mean() for a in att)


def restate(case, dtype, device="cpu"):
    """float64 [3] (LOSSES order) of the restatement evaluated in `dtype` on `device`"""
    left, right, att, valid = _as({k: v.to(device) for k, v in case.items() if k in FIELDS}, dtype)
    with torch.no_grad():
        vals = (photometric(left, right, att, valid), cycle(cycle_maps(att), valid), smoothness(att))
    return torch.stack([v.double().cpu() for v in vals])


def within_rule(got, ref64, ref32):
    """The error rule of the GPU tests: |got - ref64| <= max(2 |ref32 - ref64|, 2^-23 |ref64|) -- twice the error of the float32 run
    (this project's margin for float32-grade restatements), and never tighter than one float32 ulp of the value; NaN exactly where
    the float64 value is NaN.  Returns (ok, error, allowed)."""
    got, ref64, ref32 = float(got), float(ref64), float(ref32)
    if ref64 != ref64:
        return got != got, float("nan"), float("nan")
    err, allowed = abs(got - ref64), max(2.0 * abs(ref32 - ref64), 2.0 ** -23 * abs(ref64))
    return err <= allowed, err, allowed
