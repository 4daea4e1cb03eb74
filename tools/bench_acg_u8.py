#!/usr/bin/env python3
"""Times automated colour grading (IDT + regrain) on groups of uint8 frames against the per-frame float32 route on the same
frames, 1080p pairs resident in HBM, in ONE session (HIP events, median of rounds, the legs alternating round by round):
  (a) u8 -> u8 + PSNR   ct_acg_u8 on the whole group, bytes out, with ground truth
  (b) u8 -> f32         ct_acg_u8 on the whole group, float32 out
  (c) per frame + pack  automated_color_grading_cuda on the float32 image of each frame (made before the clock starts), .float(),
                        ct_pack_u8_f32 -- the route of a Runner without grading_groups
The same rotations for every leg; every leg is warmed up at the timed shape, and a round times `--calls` calls of one leg between
two events.  Checks that the bytes of (a) and (c) are equal over the whole batch, prints pairs/s and their ratio, and writes a
stamped summary (tools/stamp.py).  No time is gated.
usage: tools/bench_acg_u8.py [--pairs 16] [--frames-per-call N] [--rounds 5] [--calls 2] [--out profiles/acg_u8_timing.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "color-transfer_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ct_hip  # noqa: E402
from methods.iterative import automated_color_grading_cuda, draw_group_rotations  # noqa: E402
from stamp import source_stamp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=16)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--frames-per-call", type=int, default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--calls", type=int, default=2)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "acg_u8_timing.json"))
opt = ap.parse_args()

B, H, W = opt.pairs, opt.height, opt.width
if not torch.cuda.is_available():
    sys.exit("bench_acg_u8 measures on the GPU: no device is visible")
g = torch.Generator(device="cuda").manual_seed(0)
t8, r8, g8 = (torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device="cuda", generator=g) for _ in range(3))
np.random.seed(0)
rot = draw_group_rotations(B)
out8, out32, pack8 = torch.empty_like(t8), torch.empty((B, H, W, 3), dtype=torch.float32, device="cuda"), torch.empty_like(t8)
psnr = torch.empty((B, 2), dtype=torch.float64, device="cuda")
d255 = torch.tensor(255.0, device="cuda")        # a device divisor: `x / 255` on the device is x * (1 / 255), not the rounded quotient
t32, r32 = t8.float() / d255, r8.float() / d255


def per_frame_route():
    for b in range(B):
        ct_hip.pack_u8(automated_color_grading_cuda(t32[b], r32[b], rotations=rot[b]).float()[None], "hwc", out=pack8[b:b + 1])


LEGS = (("u8 -> u8 + PSNR", lambda: ct_hip.acg_u8(t8, r8, rot, out=out8, gt=g8, psnr_out=psnr, frames_per_call=opt.frames_per_call)),
        ("u8 -> f32", lambda: ct_hip.acg_u8(t8, r8, rot, out=out32, frames_per_call=opt.frames_per_call)),
        ("per frame + pack", per_frame_route))


def one_round(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e-3


for _, fn in LEGS:
    for _ in range(2):
        fn()
torch.cuda.synchronize()
times = {name: [] for name, _ in LEGS}
for _ in range(opt.rounds):
    for name, fn in LEGS:
        times[name].append(one_round(fn, opt.calls))
res = {"source_stamp": source_stamp(), "device": torch.cuda.get_device_name(0), "pairs": B, "height": H, "width": W,
       "frames_per_call": opt.frames_per_call or B, "rounds": opt.rounds, "calls_per_round": opt.calls, "legs": {}}
for name, _ in LEGS:
    med, best, worst = float(np.median(times[name])), float(np.min(times[name])), float(np.max(times[name]))
    res["legs"][name] = {"ms_per_call": med * 1e3, "ms_per_call_min": best * 1e3, "ms_per_call_max": worst * 1e3, "pairs_per_s": B / med}
    print("[B=%d %dx%d] %-18s %9.2f ms/call (min %.2f, max %.2f)  %8.2f ms/pair  %7.1f pairs/s"
          % (B, W, H, name, med * 1e3, best * 1e3, worst * 1e3, med / B * 1e3, B / med), flush=True)
ratio = res["legs"]["per frame + pack"]["ms_per_call"] / res["legs"]["u8 -> u8 + PSNR"]["ms_per_call"]
res["grouped_over_per_frame"] = ratio
print("grouped (a) over per frame (c): %.2fx the pairs/s" % ratio)
LEGS[0][1]()
per_frame_route()
diff = int((out8 != pack8).sum())
res["bytes_equal"] = diff == 0
print("bytes of (a) vs (c): %d of %d differ" % (diff, out8.numel()))
os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
json.dump(res, open(opt.out, "w"), indent=1, sort_keys=True)
print("wrote", opt.out)
if diff:
    sys.exit("the bytes of the grouped uint8 route and of the per-frame float32 route differ")
