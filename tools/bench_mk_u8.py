#!/usr/bin/env python3
"""Times MK on uint8 frames against the float32 route on the same frames, 1080p pairs resident in HBM, in ONE session
(HIP events, median of rounds, the three legs alternating round by round):
  u8 -> u8     ct_mk_u8 with uint8 out           3 + 3 + 3 + 3 = 12 B per pixel of a pair (moments of both frames, the target again, the bytes)
  u8 -> f32    ct_mk_u8 with float32 out         3 + 3 + 3 + 12 = 21 B
  f32 + pack   ct_mk_f32_f32 then ct_pack_u8_f32 12 + 12 + 12 + 12 (MK) + 12 + 3 (pack) = 63 B; the uint8 -> float32 conversion that
               feeds it in `utils.cli` (another 3 + 12 B per frame) is NOT in the timed loop
Prints pairs/s and the fraction of the HBM peak (8 TB/s) on the bytes each leg moves; compares the bytes of the first two legs.
usage: tools/bench_mk_u8.py [pairs=16]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "color-transfer_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ct_hip  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
H, W = 1080, 1920
PEAK = 8e12
g = torch.Generator(device="cuda").manual_seed(0)
t8, r8 = (torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device="cuda", generator=g) for _ in range(2))
t32, r32 = t8.float() / 255, r8.float() / 255
out8, out32 = torch.empty_like(t8), torch.empty_like(t32)
pack8 = torch.empty_like(t8)


def f32_route():
    ct_hip.mk(t32, r32, out=out32)
    ct_hip.pack_u8(out32, "hwc", out=pack8)


LEGS = (("u8 -> u8", lambda: ct_hip.mk(t8, r8, out=out8), 12),
        ("u8 -> f32", lambda: ct_hip.mk(t8, r8, out=out32), 21),
        ("f32 + pack", f32_route, 63))


def one_round(fn, n=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e-3


for _, fn, _ in LEGS:
    for _ in range(5):
        fn()
torch.cuda.synchronize()
times = {name: [] for name, _, _ in LEGS}
for _ in range(7):
    for name, fn, _ in LEGS:
        times[name].append(one_round(fn))
for name, _, bytes_per_pixel in LEGS:
    med, best = float(np.median(times[name])), float(np.min(times[name]))
    moved = bytes_per_pixel * H * W * B
    print("[B=%d 1080p] %-10s %8.1f us/call  %7.2f us/pair  %8.0f pairs/s (best %8.0f)  %2d B/pixel  frac of 8 TB/s %.3f"
          % (B, name, med * 1e6, med / B * 1e6, B / med, B / best, bytes_per_pixel, moved / med / PEAK), flush=True)
ct_hip.mk(t8, r8, out=out8)
f32_route()
diff = (out8.int() - pack8.int()).abs()
print("bytes of the u8 route vs the f32 route: %d of %d differ, max |difference| %d (float32 moments vs exact ones)"
      % (int((diff > 0).sum()), diff.numel(), int(diff.max())))
