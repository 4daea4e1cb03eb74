#!/usr/bin/env python3
"""Times the perspective warp of uint8 frames (csrc/warp.hip) and utils.postprocess.process_frames, 1080p frames resident in HBM,
in ONE session (HIP events, median of rounds, the legs alternating round by round):
  warp staged   ct_hip.warp_perspective, source rows of every tile through LDS      3 B read + 3 B written per surviving pixel
  warp global   the same call with every tap from memory                             (the byte model of DESIGN 4.21)
  process       process_frames: two warps, the double crop of left_gt, MK on bytes   2 x 6 + 6 (crop copy) + 12 (MK u8 -> u8) = 30 B
  pack ceiling  ct_hip.pack_u8 (HWC float32 -> bytes) on the same pixel count         12 B read + 3 B written: the project's
                streaming kernel of this shape, the yardstick for "how fast can bytes leave a kernel here"
bbox = the frame less 16 px, a near-identity homography, the flip on.  Prints frames/s, bytes/s on the byte model, the fraction of
the HBM peak (8 TB/s) and the share of the pack kernel's byte rate.
usage: tools/bench_warp.py [frames=16]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "color-transfer_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ct_hip  # noqa: E402
from utils import postprocess as pp  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
H, W = 1080, 1920
PEAK = 8e12
BBOX = (8, 8, W - 16, H - 16)
WINDOW = pp.second_crop(BBOX)
HOMOGRAPHY = np.array([[1.004, 0.003, -2.5], [-0.002, 0.997, 1.75], [1.5e-6, -1e-6, 1.0]])
g = torch.Generator(device="cuda").manual_seed(0)
left, gt, right = (torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device="cuda", generator=g) for _ in range(3))
n_out = WINDOW[2] * WINDOW[3]
out = torch.empty((B, WINDOW[3], WINDOW[2], 3), dtype=torch.uint8, device="cuda")
f32 = torch.rand((B, WINDOW[3], WINDOW[2], 3), dtype=torch.float32, device="cuda", generator=g)
pack8 = torch.empty_like(out)


def warp(path):
    return lambda: ct_hip.warp_perspective(left, HOMOGRAPHY, crop=BBOX, flip_x=True, window=WINDOW, out=out, path=path)


LEGS = (("warp staged", warp("staged"), 6),
        ("warp global", warp("global"), 6),
        ("process", lambda: pp.process_frames(left, gt, right, HOMOGRAPHY, HOMOGRAPHY, BBOX), 30),
        ("pack ceiling", lambda: ct_hip.pack_u8(f32, "hwc", out=pack8), 15))


def one_round(fn, n=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e-3


for _, fn, _ in LEGS:
    for _ in range(3):
        fn()
torch.cuda.synchronize()
times = {name: [] for name, _, _ in LEGS}
for _ in range(7):
    for name, fn, _ in LEGS:
        times[name].append(one_round(fn))
rate = {}
for name, _, bytes_per_pixel in LEGS:
    med, best = float(np.median(times[name])), float(np.min(times[name]))
    moved = bytes_per_pixel * n_out * B
    rate[name] = moved / med
    print("[B=%d 1080p, window %dx%d] %-12s %8.1f us/call  %7.2f us/frame  %8.0f frames/s (best %8.0f)  %2d B/pixel  %.3f TB/s  frac of 8 TB/s %.3f"
          % (B, WINDOW[2], WINDOW[3], name, med * 1e6, med / B * 1e6, B / med, B / best, bytes_per_pixel, moved / med / 1e12, moved / med / PEAK), flush=True)
for name in ("warp staged", "warp global", "process"):
    print("%-12s moves bytes at %.2f of the pack kernel's rate" % (name, rate[name] / rate["pack ceiling"]))
a = ct_hip.warp_perspective(left, HOMOGRAPHY, crop=BBOX, flip_x=True, window=WINDOW, path="staged")
b = ct_hip.warp_perspective(left, HOMOGRAPHY, crop=BBOX, flip_x=True, window=WINDOW, path="global")
print("staged vs global taps: %d of %d bytes differ" % (int((a != b).sum()), a.numel()))
