#!/usr/bin/env python3
"""Times the iterative distribution transfer on uint8 frames against the float32 route on the same bytes, 1080p pairs resident in
HBM, in ONE session (HIP events, median of rounds, the three legs alternating round by round), per pixel of a pair:
  (a) u8 -> u8 + PSNR   ct_idt_u8, bytes out, with ground truth      246 B: lo/hi 3 + 3, four histogram sweeps 6 + 3 * 27, apply
                                                                     27 + 2 * 48, the last apply 24 + 3 + 3
  (b) u8 -> f32         ct_idt_u8, float32 out                       252 B: the last apply 24 + 12
  (c) f32 + pack        uint8 -> float32 by a true division by 255 (both frames), ct_idt_f32, .float(), ct_pack_u8_f32 -- the
                        route of a Runner without iterative_groups   417 B: 30 + 336 + 36 + 15
The same rotations for every leg.  Checks that the bytes of (a) and (c) are equal over the whole batch, prints pairs/s and the
fraction of the HBM peak (8 TB/s) on the bytes each leg moves, and writes a stamped summary (tools/stamp.py).  No time is gated.
usage: tools/bench_idt_u8.py [--pairs 16] [--out profiles/idt_u8_timing.json]
       tools/bench_idt_u8.py --kernels-only            leg (a) alone, three calls: the program of a `rocprofv3 --kernel-trace --stats` run
       tools/bench_idt_u8.py --kernel-stats stats.csv  also fold that run's kernel_stats.csv (Name, Calls, AverageNs) into the summary"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "color-transfer_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ct_hip  # noqa: E402
from methods.iterative import draw_group_rotations  # noqa: E402
from stamp import source_stamp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=16)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "idt_u8_timing.json"))
ap.add_argument("--kernels-only", action="store_true")
ap.add_argument("--kernel-stats", default=None)
opt = ap.parse_args()

B, H, W, PEAK = opt.pairs, 1080, 1920, 8e12
g = torch.Generator(device="cuda").manual_seed(0)
t8, r8, g8 = (torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device="cuda", generator=g) for _ in range(3))
np.random.seed(0)
rot = draw_group_rotations(B)
out8, out32, pack8 = torch.empty_like(t8), torch.empty((B, H, W, 3), dtype=torch.float32, device="cuda"), torch.empty_like(t8)
out64 = torch.empty((B, H, W, 3), dtype=torch.float64, device="cuda")
psnr = torch.empty((B, 2), dtype=torch.float64, device="cuda")


d255 = torch.tensor(255.0, device="cuda")      # a device divisor: torch turns `x / 255` on the device into x * (1 / 255), which is not
                                               # the correctly rounded quotient the datasets compute on the host (126 of 256 values differ)


def f32_route():
    ct_hip.idt(t8.float() / d255, r8.float() / d255, rot, out=out64)
    ct_hip.pack_u8(out64.float(), "hwc", out=pack8)


LEGS = (("u8 -> u8 + PSNR", lambda: ct_hip.idt_u8(t8, r8, rot, out=out8, gt=g8, psnr_out=psnr), 246),
        ("u8 -> f32", lambda: ct_hip.idt_u8(t8, r8, rot, out=out32), 252),
        ("f32 + pack", f32_route, 417))
# bytes per pixel of a pair that each kernel of leg (a) reads and writes
KERNEL_BYTES = (("idt_minmax_kernel<unsigned char", 6), ("idt_hist_kernel<unsigned char, unsigned char>", 6),
                ("idt_hist_kernel<double, unsigned char>", 27), ("idt_apply_kernel<unsigned char, false>", 27),
                ("idt_apply_kernel<double, false>", 48), ("idt_apply_kernel<double, true>", 30), ("idt_lut_kernel", 0),
                ("psnr_finish_kernel", 0), ("ct_zero_words_kernel", 0))

if opt.kernels_only:
    for _ in range(3):
        LEGS[0][1]()
    torch.cuda.synchronize()
    sys.exit(0)


def one_round(fn, n=3):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e-3


for _, fn, _ in LEGS:
    for _ in range(2):
        fn()
torch.cuda.synchronize()
times = {name: [] for name, _, _ in LEGS}
for _ in range(5):
    for name, fn, _ in LEGS:
        times[name].append(one_round(fn))
res = {"source_stamp": source_stamp(), "device": torch.cuda.get_device_name(0), "pairs": B, "height": H, "width": W,
       "hbm_peak_tb_per_s": PEAK / 1e12, "legs": {}}
for name, _, bytes_per_pixel in LEGS:
    med, best = float(np.median(times[name])), float(np.min(times[name]))
    moved = bytes_per_pixel * H * W * B
    res["legs"][name] = {"us_per_call": med * 1e6, "pairs_per_s": B / med, "bytes_per_pixel": bytes_per_pixel, "hbm_frac": moved / med / PEAK}
    print("[B=%d 1080p] %-16s %9.1f us/call  %8.1f us/pair  %7.0f pairs/s (best %7.0f)  %3d B/pixel  frac of 8 TB/s %.3f"
          % (B, name, med * 1e6, med / B * 1e6, B / med, B / best, bytes_per_pixel, moved / med / PEAK), flush=True)
LEGS[0][1]()
f32_route()
diff = int((out8 != pack8).sum())
res["bytes_equal"] = diff == 0
print("bytes of (a) vs (c): %d of %d differ" % (diff, out8.numel()))
if opt.kernel_stats:
    res["kernels"] = {}
    for row in csv.DictReader(line for line in open(opt.kernel_stats) if not line.startswith("#")):
        for key, bpp in KERNEL_BYTES:
            if key in row["Name"]:
                us = float(row["AverageNs"]) * 1e-3
                res["kernels"][row["Name"]] = {"calls": int(row["Calls"]), "us": us, "bytes_per_pixel": bpp,
                                               "hbm_frac": bpp * H * W * B / (us * 1e-6) / PEAK}
                print("%-90s %4d calls  %9.1f us  %2d B/pixel  frac of 8 TB/s %.3f" % (row["Name"][:90], int(row["Calls"]), us, bpp,
                                                                                     res["kernels"][row["Name"]]["hbm_frac"]))
json.dump(res, open(opt.out, "w"), indent=1, sort_keys=True)
print("wrote", opt.out)
if diff:
    sys.exit("the bytes of the uint8 route and of the float32 route differ")
