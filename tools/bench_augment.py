#!/usr/bin/env python3
"""Time the training / validation sample kernels (csrc/augment.hip) and the step losses (csrc/losses.hip) with events, and write a
stamped summary (tools/stamp.py).  Nothing here is on a timed path and no time is gated.

    augment_u8       a batch of 8 crops of 256 x 480 from 1080p sources, a full chain of the six operations in a different order per
                     sample: one call (zeroing + one grey-sum launch + one apply launch).  Bytes a call has to move per crop pixel:
                     3 + 3 read for the apply pass, 3 more for the grey sum, 3 x 12 written = 45 B
    composition      the same batch from single-operation calls fed one into the next (the identity chain for the geometry, then six
                     calls on uint8 intermediates): what a caller without the chain would have to run
    frame_losses     one 1080p frame pair, beside frame_ssim (ct_frame_ssim_f32, piq's SSIM at the same size): 24 B / pixel read

The inputs rotate through a pool larger than the 256 MB last-level cache.

usage: tools/bench_augment.py [--out profiles/augment_timing.json] [--reps 5]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "color-transfer_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ct_hip  # noqa: E402
from bench_views import CACHE_BYTES, HBM_PEAK, timed  # noqa: E402
from stamp import source_stamp  # noqa: E402

H, W, CROP, BATCH = 1080, 1920, (256, 480), 8
OPS = {"brightness": 1.2, "contrast": 0.8, "saturation": 1.3, "hue": 0.1, "gamma": 0.9, "sharpness": 1.4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    pool = 2 * CACHE_BYTES // (2 * BATCH * 3 * H * W) + 2            # batches of 8 uint8 pairs: beyond twice the cache
    gts = [torch.randint(0, 256, (BATCH, 3, H, W), dtype=torch.uint8, device="cuda") for _ in range(pool)]
    refs = [torch.randint(0, 256, (BATCH, 3, H, W), dtype=torch.uint8, device="cuda") for _ in range(pool)]
    names = list(OPS)
    params = [{"top": int(rng.integers(0, H - CROP[0])), "left": int(rng.integers(0, W - CROP[1])), "swap_hflip": bool(i & 1), "vflip": bool(i & 2),
               "ops": [(names[j], OPS[names[j]]) for j in rng.permutation(6)]} for i in range(BATCH)]
    table = ct_hip.augment_table(params)

    def chain(i):
        return ct_hip.augment_u8(gts[i], refs[i], table, CROP)

    def composition(i):
        cur = ct_hip.augment_u8(gts[i], refs[i], [dict(p, ops=[]) for p in params], CROP, want_u8=True)["target_u8"]
        for k in range(6):
            cur = ct_hip.augment_u8(cur, cur, [{"top": 0, "left": 0, "swap_hflip": False, "vflip": False, "ops": p["ops"][k:k + 1]} for p in params],
                                    CROP, want_u8=True)["target_u8"]
        return cur

    want = composition(0)
    got = ct_hip.augment_u8(gts[0], refs[0], table, CROP, want_u8=True)["target_u8"]
    assert torch.equal(got, want), "the chain and the composition disagree"
    fpool = 2 * CACHE_BYTES // (24 * H * W) + 2
    xs = [torch.rand(1, 3, H, W, device="cuda") for _ in range(fpool)]
    ys = [(x * 0.9 + 0.05 * torch.rand_like(x)).contiguous() for x in xs]
    crop_px = BATCH * CROP[0] * CROP[1]
    cases = {
        "augment_u8_x8": (chain, pool, 45 * crop_px),
        "composition_x8": (composition, pool, None),
        "frame_losses_1080p": (lambda i: ct_hip.frame_losses(xs[i], ys[i]), fpool, 24 * H * W),
        "frame_ssim_1080p": (lambda i: ct_hip.frame_ssim(xs[i], ys[i]), fpool, 24 * H * W),
    }
    res = {"source_stamp": source_stamp(), "device": torch.cuda.get_device_name(0), "height": H, "width": W, "crop": list(CROP), "batch": BATCH,
           "hbm_peak_tb_per_s": HBM_PEAK / 1e12, "note": "times include the binding's work per call (the table upload, the allocation of "
           "the results) and every launch of a call", "kernels": {}}
    for name, (fn, n, nbytes) in cases.items():
        ms = timed(fn, n, a.reps)
        res["kernels"][name] = {"us_per_call": 1e3 * ms, "input_pool": n}
        if nbytes:
            res["kernels"][name].update(bytes_per_call=nbytes, tb_per_s=nbytes / (ms * 1e-3) / 1e12, hbm_frac=nbytes / (ms * 1e-3) / HBM_PEAK)
        print("%-20s %9.1f us per call%s" % (name, 1e3 * ms, "  %5.2f TB/s" % res["kernels"][name]["tb_per_s"] if nbytes else ""))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")
        print("wrote", a.out)


if __name__ == "__main__":
    main()
