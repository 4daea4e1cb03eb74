#!/usr/bin/env python3
"""Time the bicubic resampling (csrc/resize.hip) and DCMCS3DI's reduced-scale inference (DCMCS3DI.forward_scaled, the reference's
demo notebook, cell 24) on the GPU and write a stamped summary (tools/stamp.py):

  * ct_bicubic_resize_f32 alone, with events, on a [2,3,H,W] batch (the two views): 1080p -> 810x1440, 810x1440 -> 1080p,
    2160p <-> 1080p, with and without antialias: microseconds per launch and the share of the 8 TB/s HBM peak on bytes in + bytes
    out (with antialias the float32 intermediate is cache traffic where it fits and is not counted);
  * DCMCS3DI at 1080p, full depth: the plain forward against forward_scaled at 0.75 and 0.5, interleaved in one process, three
    rounds, best of each; the ratio reached against the bound 1 / factor^2; the resize launches' share of the scaled forward;
  * PSNR of the scaled result (clamped) against the full-size result on SyntheticStereoFrames -- the quality cost, reported only.

usage: tools/bench_scaled.py [--out profiles/scaled_timing.json] [--reps N] [--kernels-only]"""
import argparse
import json
import math
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


def event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def kernels(reps, res):
    g = torch.Generator().manual_seed(0)
    rows = {}
    for name, (h, w), (ho, wo) in (("1080p->810x1440", (1080, 1920), (810, 1440)), ("810x1440->1080p", (810, 1440), (1080, 1920)),
                                   ("2160p->1080p", (2160, 3840), (1080, 1920)), ("1080p->2160p", (1080, 1920), (2160, 3840))):
        x = torch.rand(2, 3, h, w, generator=g).cuda()
        out = torch.empty(2, 3, ho, wo, device="cuda")
        nbytes = 4.0 * 6 * (h * w + ho * wo)
        for aa in (False, True):
            us = 1e3 * min(event_ms(lambda: ct_hip.bicubic_resize(x, size=(ho, wo), antialias=aa, out=out), reps * 4) for _ in range(3))
            rows[name + (" antialias" if aa else "")] = {"us": us, "bytes": nbytes, "hbm_frac": nbytes / (us * 1e-6) / HBM_PEAK}
        del x, out
    res["resize_2x3_planes"] = rows


def forward(reps, res):
    from tests.dcmcs3di_common import build_model
    from utils.data import SyntheticStereoFrames
    m = build_model(seed=11).cuda()
    g = torch.Generator().manual_seed(12)
    left, right = torch.rand(1, 3, 1080, 1920, generator=g).cuda(), torch.rand(1, 3, 1080, 1920, generator=g).cuda()
    legs = {"plain": lambda: m(left, right, inference=True), "scaled_0.75": lambda: m.forward_scaled(left, right, 0.75),
            "scaled_0.5": lambda: m.forward_scaled(left, right, 0.5)}
    t = {k: [] for k in legs}
    for _ in range(3):                                   # interleaved in one process
        for k, fn in legs.items():
            t[k].append(event_ms(fn, reps))
    best = {k: min(v) for k, v in t.items()}
    res["forward_1080p_ms"], res["forward_1080p_ms_all"] = best, t
    res["forward_1080p_pairs_per_s"] = {k: 1e3 / v for k, v in best.items()}
    both = torch.cat([left, right])
    for f in (0.75, 0.5):
        key = "scaled_%s" % f
        low = ct_hip.bicubic_resize(both, scale_factor=f)
        one = low[:1].contiguous()
        down = min(event_ms(lambda: ct_hip.bicubic_resize(both, scale_factor=f), reps * 4) for _ in range(3))
        up = min(event_ms(lambda: ct_hip.bicubic_resize(one, size=(1080, 1920)), reps * 4) for _ in range(3))
        inner = min(event_ms(lambda: m(low[:1], low[1:], inference=True), reps) for _ in range(2))
        res[key] = {"speedup_vs_plain": best["plain"] / best[key], "bound": 1.0 / (f * f), "resize_down_ms": down, "resize_up_ms": up,
                    "resize_share": (down + up) / best[key], "forward_at_reduced_size_ms": inner}
    # the quality cost on frames with structure (noise has nothing a reduced size could keep)
    fr = SyntheticStereoFrames(4, 1080, 1920)
    q = {"scaled_0.75": [], "scaled_0.5": []}
    for i in range(4):
        l, r = fr[i]["target"][None].cuda(), fr[i]["reference"][None].cuda()
        full = m(l, r, inference=True)[0]
        for f in (0.75, 0.5):
            mse = float(((m.forward_scaled(l, r, f)[0].clamp(0, 1) - full).double() ** 2).mean())
            q["scaled_%s" % f].append(10 * math.log10(1.0 / mse) if mse > 0 else float("inf"))
    res["psnr_vs_full_size_db"] = {k: {"mean": sum(v) / len(v), "min": min(v)} for k, v in q.items()}
    res["psnr_note"] = "seeded (untrained) weights on SyntheticStereoFrames(4, 1080, 1920); reported only"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    res = {"source_stamp": source_stamp(), "device": torch.cuda.get_device_name(0)}
    kernels(a.reps, res)
    if not a.kernels_only:
        forward(a.reps, res)
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
