#!/usr/bin/env python3
"""Times iCID with its options (ct_frame_icid_opt_f32 / ct_frame_icid_opt_hwc_u8) on 1080p frames resident in HBM, in ONE session
(HIP events, median of rounds, the legs alternating round by round): the default call (maps on the 270 x 480 grid of f = 4) against
`downsampling=False` (maps on the 1080 x 1920 grid: 16 x the map pixels, 4080 tiles of 32 x 16 per frame instead of 255), each
with and without `omit_maps67` (8 instead of 11 blurred planes), for the planar entry (24 B read per pixel) and the entry on a frame
group's own buffers (15 B per pixel).  Prints frames/s, the ratio to the default call of the same entry and the fraction of the HBM
peak (8 TB/s) on the bytes a leg reads, and writes a stamped summary (tools/stamp.py).  No time is gated.
usage: tools/bench_icid_options.py [--frames 16] [--out profiles/icid_options_timing.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "color-transfer_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ct_hip  # noqa: E402
from stamp import source_stamp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=16)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icid_options_timing.json"))
opt = ap.parse_args()

B, H, W, PEAK = opt.frames, 1080, 1920, 8e12
g = torch.Generator(device="cuda").manual_seed(0)
gt8 = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
# an unclamped float32 HWC result, as a grouped transfer leaves it: the ground truth with a gain about mid-grey and noise
res_hwc = ((gt8.float() / 255 - 0.5) * 1.25 + 0.5 + 0.03 * torch.randn((B, H, W, 3), device="cuda", generator=g)).contiguous()
x = res_hwc.clamp(0, 1).permute(0, 3, 1, 2).contiguous()
y = (gt8.float() / 255).permute(0, 3, 1, 2).contiguous()

ENTRIES = (("planar", lambda **kw: ct_hip.frame_icid(x, y, **kw), 24), ("hwc_u8", lambda **kw: ct_hip.frame_icid_hwc(res_hwc, gt8, **kw), 15))
OPTIONS = (("default", {}), ("omit_maps67", {"omit_maps67": True}), ("full size", {"downsampling": False}),
           ("full size, omit_maps67", {"downsampling": False, "omit_maps67": True}))
LEGS = tuple(("%s, %s" % (ename, oname), (lambda fn=fn, kw=kw: fn(**kw)), bpp, ename, oname) for ename, fn, bpp in ENTRIES for oname, kw in OPTIONS)


def one_round(fn, n=3):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e-3


for leg in LEGS:
    for _ in range(2):
        leg[1]()
torch.cuda.synchronize()
times = {leg[0]: [] for leg in LEGS}
for _ in range(7):
    for leg in LEGS:
        times[leg[0]].append(one_round(leg[1]))
out = {"source_stamp": source_stamp(), "device": torch.cuda.get_device_name(0), "frames": B, "height": H, "width": W,
       "hbm_peak_tb_per_s": PEAK / 1e12, "legs": {}}
med = {leg[0]: float(np.median(times[leg[0]])) for leg in LEGS}
for name, _, bpp, ename, oname in LEGS:
    best, ratio = float(np.min(times[name])), med[name] / med[ename + ", default"]
    moved = bpp * H * W * B
    out["legs"][name] = {"us_per_call": med[name] * 1e6, "frames_per_s": B / med[name], "time_vs_default": ratio, "bytes_per_pixel": bpp,
                         "hbm_frac": moved / med[name] / PEAK}
    print("[B=%d 1080p] %-32s %9.1f us/call  %8.0f frames/s (best %8.0f)  %5.2f x the default call  %2d B/pixel  frac of 8 TB/s %.4f"
          % (B, name, med[name] * 1e6, B / med[name], B / best, ratio, bpp, moved / med[name] / PEAK), flush=True)
# what was timed: the two entries agree closely (torch's device `/ 255` is a multiplication by a reciprocal, so not bitwise here; the
# bitwise contract is tests/test_icid_options_gpu.py, converted on the host), and the flag moves the value at f = 4
for oname, kw in OPTIONS:
    a, b = ENTRIES[0][1](**kw), ENTRIES[1][1](**kw)
    out["legs"]["planar, " + oname]["value_frame0"] = float(a[0])
    print("    %-24s iCID of frame 0: %.6f; max |planar - hwc_u8| %.3g" % (oname, float(a[0]), float((a - b).abs().max())), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
with open(opt.out, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print("wrote", opt.out)
