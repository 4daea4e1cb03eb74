#!/usr/bin/env python3
"""Time the parallax-attention loss kernels (csrc/pam_losses.hip) at the reference's training crop (configs/dcmcs3di.yaml: batch 8,
160 x 320: two attention maps of 524 MB) with events, beside the same statements written in torch on device tensors (the restatement of
tests/pam_losses_common.py on `cuda`), and write a stamped summary (tools/stamp.py).  Nothing here is on a timed path and no time is
gated.

    cycle_fused      ct_hip.pam_cycle_l1 in both directions (pasmnet.losses.loss_pam_cycle_from_att): 2 x 8 x 160 products of
                     320 x 320 x 320 = 1.68e11 flop on the exact-f32 MFMA; no cycle map is stored
    cycle_torch      two torch.matmul, the identity tensor and the masked L1 of the restatement
    sweeps           ct_hip.pam_map_sweep of both maps with every term on (loss_pam_photometric + loss_pam_smoothness need the
                     same two passes): 2 x 524 MB read
    sweeps_torch     the photometric and the smoothness loss of the restatement

A map is twice the 256 MB last-level cache, so one pair of maps serves every repetition.

usage: tools/bench_pam_losses.py [--out profiles/pam_losses_timing.json] [--reps 5] [--batch 8 --height 160 --width 320]"""
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
from bench_views import HBM_PEAK, timed  # noqa: E402
from pasmnet import losses  # noqa: E402
from stamp import source_stamp  # noqa: E402
from tests import pam_losses_common as plc  # noqa: E402

MFMA_F32_PEAK = 157e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=160)
    ap.add_argument("--width", type=int, default=320)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    b, h, w = a.batch, a.height, a.width
    g = torch.Generator(device="cuda").manual_seed(0)
    i = torch.arange(w, dtype=torch.float32, device="cuda").view(w, 1)
    j = torch.arange(w, dtype=torch.float32, device="cuda").view(1, w)
    att = tuple(torch.softmax(-2.0 * (j - (i + s)).abs() + torch.randn(b, h, w, w, generator=g, device="cuda"), dim=-1) for s in (-3.0, 3.0))
    left = torch.rand(b, 3, h, w, generator=g, device="cuda")
    right = (left * 0.8 + 0.2 * torch.rand(b, 3, h, w, generator=g, device="cuda")).contiguous()
    valid = ((att[1].sum(dim=-2) > 0.1).unsqueeze(1), (att[0].sum(dim=-2) > 0.1).unsqueeze(1))
    valid_f = tuple(v.float() for v in valid)

    def sweeps(_):
        return (ct_hip.pam_map_sweep(att[0], src=right, dst=left, mask=valid_f[0]), ct_hip.pam_map_sweep(att[1], src=left, dst=right, mask=valid_f[1]))

    def sweeps_torch(_):
        return plc.photometric(left, right, att, valid_f) + plc.smoothness(att)

    # the two sides agree before anything is timed
    s = sweeps(0)
    mine = sum(x["photometric"].sum() / x["mask_sum"].sum() + x["vertical"].sum() / float(x["vertical_count"].sum()) + x["diagonal"].sum() / float(x["diagonal_count"].sum())
               for x in s)
    theirs = sweeps_torch(0)
    assert abs(float(mine) - float(theirs)) <= 1e-5 * abs(float(theirs)), (float(mine), float(theirs))
    cyc, cyc_t = losses.loss_pam_cycle_from_att(att, valid_f), plc.cycle(plc.cycle_maps(att), valid_f)
    assert abs(float(cyc) - float(cyc_t)) <= 1e-5 * abs(float(cyc_t)), (float(cyc), float(cyc_t))
    map_bytes, flop = 4 * b * h * w * w, 2 * 2.0 * b * h * w * w * w
    cases = {
        "cycle_fused": (lambda _: losses.loss_pam_cycle_from_att(att, valid_f), None, flop),
        "cycle_torch": (lambda _: plc.cycle(plc.cycle_maps(att), valid_f), None, flop),
        "sweeps": (sweeps, 2 * map_bytes, None),
        "sweeps_torch": (sweeps_torch, 2 * map_bytes, None),
    }
    res = {"source_stamp": source_stamp(), "device": torch.cuda.get_device_name(0), "batch": b, "height": h, "width": w,
           "hbm_peak_tb_per_s": HBM_PEAK / 1e12, "mfma_f32_peak_tflops": MFMA_F32_PEAK / 1e12,
           "note": "times include the binding's work per call (allocating the results and the partial sums) and every launch of a call; "
                   "bytes are the maps alone, once each", "kernels": {}}
    for name, (fn, nbytes, nflop) in cases.items():
        ms = timed(fn, 1, a.reps)
        k = res["kernels"][name] = {"us_per_call": 1e3 * ms}
        if nbytes:
            k.update(bytes_per_call=nbytes, tb_per_s=nbytes / (ms * 1e-3) / 1e12, hbm_frac=nbytes / (ms * 1e-3) / HBM_PEAK)
        if nflop:
            k.update(flop_per_call=nflop, tflops=nflop / (ms * 1e-3) / 1e12, mfma_f32_frac=nflop / (ms * 1e-3) / MFMA_F32_PEAK)
        print("%-14s %10.1f us per call%s%s" % (name, 1e3 * ms, "  %5.2f TB/s" % k["tb_per_s"] if nbytes else "",
                                                "  %6.1f TF" % k["tflops"] if nflop else ""))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")
        print("wrote", a.out)


if __name__ == "__main__":
    main()
