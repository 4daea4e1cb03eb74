#!/usr/bin/env python3
"""Times the Y'CbCr 4:2:0 path (csrc/yuv.hip) in ONE session:
  kernels   ct_hip.yuv420_to_rgb and ct_hip.rgb_to_yuv420 on 1080p frames resident in HBM, next to ct_hip.pack_u8 (HIP events,
            median of rounds, the legs alternating round by round).  Byte model: 1.5 B of YUV + 3 B of RGB = 4.5 B/pixel for the
            two conversions, 12 + 3 = 15 B/pixel for the pack; printed against the HBM peak (8 TB/s).
  test      `utils.cli test --model.metrics psnr` on --data.synthetic video_yuv against video_u8: the upload is 9.3 MB against
            18.7 MB per 1080p frame triple, so the bound on the ratio of frame rates is 2x (what the link allows, no promise).
  predict   `utils.cli predict --format y4m` against `--format raw` on video_yuv / video_u8: 3.1 against 6.2 MB per frame down.
usage: tools/bench_yuv.py [frames=24] [video_frames=200]"""
import contextlib
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "color-transfer_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ct_hip  # noqa: E402
from utils import cli  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 24
N_VIDEO = int(sys.argv[2]) if len(sys.argv) > 2 else 200
H, W = 1080, 1920
PEAK = 8e12
FB = ct_hip.yuv420_frame_bytes(H, W)
g = torch.Generator(device="cuda").manual_seed(0)
yuv = torch.randint(0, 256, (B, FB), dtype=torch.uint8, device="cuda", generator=g)
rgb = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
f32 = torch.rand((B, H, W, 3), dtype=torch.float32, device="cuda", generator=g)
rgb_out, yuv_out, pack_out = torch.empty_like(rgb), torch.empty_like(yuv), torch.empty_like(rgb)

LEGS = (("yuv420_to_rgb", lambda: ct_hip.yuv420_to_rgb(yuv, H, W, out=rgb_out), 4.5),
        ("rgb_to_yuv420", lambda: ct_hip.rgb_to_yuv420(rgb, out=yuv_out), 4.5),
        ("to_rgb left", lambda: ct_hip.yuv420_to_rgb(yuv, H, W, siting="left", matrix="bt601", range="full", out=rgb_out), 4.5),
        ("pack_u8", lambda: ct_hip.pack_u8(f32, "hwc", out=pack_out), 15.0))


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
for name, _, bpp in LEGS:
    med, best = float(np.median(times[name])), float(np.min(times[name]))
    moved = bpp * H * W * B
    print("[B=%d 1080p] %-14s %8.1f us/call  %7.2f us/frame  %8.0f frames/s (best %8.0f)  %4.1f B/pixel  %.3f TB/s  frac of 8 TB/s %.3f"
          % (B, name, med * 1e6, med / B * 1e6, B / med, B / best, bpp, moved / med / 1e12, moved / med / PEAK), flush=True)

CFG = os.path.join(ROOT, "color-transfer_amd", "configs", "others.yaml")
BASE = ["--config", CFG, "--model.metrics", "psnr", "--data.data_dir", "null", "--data.n_frames", str(N_VIDEO), "--data.height", str(H),
        "--data.width", str(W)]


def run(cmd, synthetic, fmt=None):
    t = {}
    with tempfile.TemporaryDirectory() as out, contextlib.redirect_stdout(sys.stderr):
        extra = ["--output", out, "--format", fmt] if fmt else []
        cli.main([cmd] + BASE + ["--data.synthetic", synthetic] + extra, timing=t)
    return t


rates = {}
for rnd in range(2):
    for key, args in (("test video_u8", ("test", "video_u8")), ("test video_yuv", ("test", "video_yuv")),
                      ("predict u8 -> raw", ("predict", "video_u8", "raw")), ("predict yuv -> y4m", ("predict", "video_yuv", "y4m"))):
        t = run(*args)
        rates.setdefault(key, []).append(t["frames"] / t["seconds"])
        print("[%d frames 1080p, round %d] %-20s %8.0f frames/s   up %6.2f GB/s (%5.2f MB/frame)   down %6.2f GB/s"
              % (N_VIDEO, rnd, key, t["frames"] / t["seconds"], t["h2d_bytes"] / t["seconds"] / 1e9, t["h2d_bytes"] / t["frames_local"] / 1e6,
                 t.get("d2h_bytes", 0) / t["seconds"] / 1e9), flush=True)
print("test:    video_yuv / video_u8 = %.2f (bound 2.0: 9.3 against 18.7 MB per frame up)" % (max(rates["test video_yuv"]) / max(rates["test video_u8"])))
print("predict: y4m / raw            = %.2f (bound 2.0: 9.3 + 3.1 against 18.7 + 6.2 MB per frame)"
      % (max(rates["predict yuv -> y4m"]) / max(rates["predict u8 -> raw"])))
