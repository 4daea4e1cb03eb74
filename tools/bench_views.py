#!/usr/bin/env python3
"""Time the diagnostic-view kernels (csrc/views.hip, csrc/errmaps.hip) at 1080p with events, next to ct_pack_u8_f32 in the same session, and write a
stamped summary (tools/stamp.py).  Per entry: microseconds per call, the bytes the call has to move (inputs read once per pass,
outputs written once), the achieved TB/s and the fraction of the 8 TB/s HBM peak:

    chess_mix      [1,3,H,W]: one source read + one write per element                                     8 B / element
    rgbmse_view    two passes over x and y (reduce, map) + three output planes                     (48 + 12) B / pixel
    gray_view      two passes over one plane + three output planes                                   (8 + 12) B / pixel
    flow_to_image  two passes over u and v + three bytes                                             (16 + 3) B / pixel
    pack_u8 (chw)  4 read + 1 written per element: the yardstick                                          5 B / element
    rgbssim_view / labmse_view / abmse_view (csrc/errmaps.hip), a group of 8 frames per call: the 6 planes of x and y read once,
                   channel 0 written, then read and rewritten in place with channels 1 and 2  (24 + 16) B / pixel and frame

The inputs rotate through a pool larger than the 256 MB last-level cache, so that a frame comes from HBM.  Nothing here is on a timed
path and no time is gated; the numbers say where each kernel sits relative to the pack kernel on the same box.

usage: tools/bench_views.py [--out profiles/views_timing.json] [--reps 5]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "color-transfer_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import torch  # noqa: E402

import ct_hip  # noqa: E402
from stamp import source_stamp  # noqa: E402

HBM_PEAK = 8.0e12
H, W = 1080, 1920
CACHE_BYTES = 256 << 20


def timed(fn, pool, reps):
    """best-of-reps milliseconds per call of fn(i) over a pool of inputs, two untimed passes first"""
    for _ in range(2):
        for i in range(pool):
            fn(i)
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(pool):
            fn(i)
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b) / pool
        best = ms if best is None else min(best, ms)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    plane = H * W
    pool = 2 * CACHE_BYTES // (12 * plane) + 2                    # frames of 3 float32 planes: beyond twice the cache
    xs = [torch.rand(1, 3, H, W, device="cuda") for _ in range(pool)]
    ys = [torch.rand(1, 3, H, W, device="cuda") for _ in range(pool)]
    flows = [(x[:, :2] * 40 - 20).contiguous() for x in xs]
    disps = [(x[:, :1] * 200 - 100).contiguous() for x in xs]
    o8 = torch.empty((1, H, W, 3), dtype=torch.uint8, device="cuda")
    group = 8                                                      # the error maps: a group of 8 frames per call
    gpool = max(2, -(-pool // group))
    gx = [torch.rand(group, 3, H, W, device="cuda") for _ in range(gpool)]
    gy = [(g * 0.9 + 0.05 * torch.rand_like(g)).contiguous() for g in gx]
    cases = {
        "pack_u8_chw": (lambda i: ct_hip.pack_u8(xs[i], "chw", out=o8), 15 * plane),
        "chess_mix_25": (lambda i: ct_hip.chess_mix(xs[i], ys[i], 25), 24 * plane),
        "chess_mix_32": (lambda i: ct_hip.chess_mix(xs[i], ys[i], 32), 24 * plane),
        "rgbmse_view": (lambda i: ct_hip.rgbmse_view(xs[i], ys[i]), 60 * plane),
        "gray_view": (lambda i: ct_hip.gray_view(disps[i]), 20 * plane),
        "flow_to_image": (lambda i: ct_hip.flow_to_image(flows[i]), 19 * plane),
        "rgbssim_view_x8": (lambda i: ct_hip.rgbssim_view(gx[i % gpool], gy[i % gpool]), 40 * plane * group),
        "labmse_view_x8": (lambda i: ct_hip.labmse_view(gx[i % gpool], gy[i % gpool]), 40 * plane * group),
        "abmse_view_x8": (lambda i: ct_hip.abmse_view(gx[i % gpool], gy[i % gpool]), 40 * plane * group),
    }
    res = {"source_stamp": source_stamp(), "device": torch.cuda.get_device_name(0), "height": H, "width": W, "input_pool": pool,
           "hbm_peak_tb_per_s": HBM_PEAK / 1e12, "note": "times include the binding's allocation of the result (and, for the min-max "
           "family and the flow image, the three launches of a call)", "kernels": {}}
    for name, (fn, nbytes) in cases.items():
        ms = timed(fn, pool, a.reps)
        res["kernels"][name] = {"us_per_call": 1e3 * ms, "bytes_per_call": nbytes, "tb_per_s": nbytes / (ms * 1e-3) / 1e12,
                                "hbm_frac": nbytes / (ms * 1e-3) / HBM_PEAK}
        print("%-16s %8.1f us  %6.2f TB/s  %5.1f %% of peak" % (name, 1e3 * ms, res["kernels"][name]["tb_per_s"], 100 * res["kernels"][name]["hbm_frac"]))
    pack = res["kernels"]["pack_u8_chw"]["tb_per_s"]
    for k, v in res["kernels"].items():
        v["over_pack_tb_per_s"] = v["tb_per_s"] / pack
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")
        print("wrote", a.out)


if __name__ == "__main__":
    main()
