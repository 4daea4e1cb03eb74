#!/usr/bin/env python3
"""Generate golden values for the three parallax-attention losses by running the REAL reference `pasmnet/losses.py`
(loss_pam_photometric, loss_pam_cycle, loss_pam_smoothness, as methods/dcmcs3di.py:75-77 calls them) on CPU (build container only):

    python3 -B tests/golden/make_golden_pam_losses.py

Only data is written (tests/golden/pam_losses.npz), per case of tests/pam_losses_common.CASES:
  * "<case>/att_r2l", "<case>/att_l2r" float32 [B,H,W,W], "<case>/left", "<case>/right" float32 [B,3,H,W], "<case>/valid_left",
    "<case>/valid_right" uint8 [B,1,H,W]: the seeded inputs of pam_losses_common.build_case;
  * "<case>/ref64", "<case>/ref32" float64 [3]: photometric, cycle and smoothness loss of the reference on these inputs as float64
    and as float32 tensors (the cycle maps by torch.matmul in that dtype, as the reference's pasmnet/utils.py output() makes them).
Every case with masks of its own has valid and invalid pixels in both of them (asserted).
"""
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)

import make_golden_dcmcs3di as mgd  # noqa: E402,F401  (registers the stub modules, puts the reference root first on sys.path)
import pasmnet.losses as ref_losses  # noqa: E402  (the reference's module)

sys.path.append(os.path.dirname(os.path.dirname(OUT)))
from tests import pam_losses_common as plc  # noqa: E402

assert hasattr(ref_losses, "masked_l1_loss") and not hasattr(ref_losses, "loss_pam_cycle_from_att"), "not the reference's pasmnet/losses.py"


def run_ref(case, dtype):
    att = (case["att_r2l"].to(dtype), case["att_l2r"].to(dtype))
    valid = (case["valid_left"].to(dtype), case["valid_right"].to(dtype))
    left, right = case["left"].to(dtype), case["right"].to(dtype)
    with torch.no_grad():
        att_cycle = (torch.matmul(att[0], att[1]), torch.matmul(att[1], att[0]))
        vals = (ref_losses.loss_pam_photometric(left, right, att, valid), ref_losses.loss_pam_cycle(att_cycle, valid),
                ref_losses.loss_pam_smoothness(att))
    return np.array([float(v.double()) for v in vals], dtype=np.float64)


def main():
    out = {}
    for name, (shape, left_mask) in plc.CASES.items():
        case = plc.build_case(shape, plc.case_seed(name), left_mask)
        for side in ("valid_left", "valid_right"):
            frac = float(case[side].float().mean())
            if shape[2] > 1 and not (side == "valid_left" and left_mask):
                assert 0.0 < frac < 1.0, (name, side, frac)
            print("%-18s %s valid fraction %.3f" % (name, side, frac))
        for k in plc.FIELDS:
            out["%s/%s" % (name, k)] = case[k].numpy()
        out[name + "/ref64"] = run_ref(case, torch.float64)
        out[name + "/ref32"] = run_ref(case, torch.float32)
        print("%-18s float64 %s\n%-18s float32 %s" % (name, out[name + "/ref64"], "", out[name + "/ref32"]))
    path = os.path.join(OUT, "pam_losses.npz")
    np.savez_compressed(path, torch=torch.__version__, **out)
    print("wrote pam_losses.npz, torch", torch.__version__, "%d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
