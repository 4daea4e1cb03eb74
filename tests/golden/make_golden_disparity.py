#!/usr/bin/env python3
"""Generate golden vectors for the disparity of the parallax attention by running the REAL reference
`pasmnet.utils.regress_disp` (pasmnet/utils.py:55-105) on CPU (build container only):

    python3 -B tests/golden/make_golden_disparity.py

Only data is written (tests/golden/disparity.npz):
  * one-hot attention maps, stored as their column indices ("onehot<W>/cols" [rows, W] int16), with masks
    ("onehot<W>/valid" [rows, W] uint8) and the reference's output ("onehot<W>/disp" [rows, W] float32), widths 1, 37, 64,
    130, 300; the masks cover empty and full rows, a single valid pixel first / last, holes of 100 px and more, holes at
    both row ends, alternating pixels and random masks;
  * "soft/att" [2, 8, 70, 70]: a softmax of a seeded random cost, "soft/valid" [2, 1, 8, 70] and "soft/disp";
  * "model_<a|b>/disp", "model_<a|b>/valid": regress_disp(att[0], valid[0].float()) of the reference DCMCS3DI of
    make_golden_dcmcs3di.build() (seed 0) on the dcmcs3di_small inputs a and b, as the reference's log_images calls it
    (methods/dcmcs3di.py:126), with "model_<a|b>/disp_ini" = the same under an all-valid mask.
"""
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)

import make_golden_dcmcs3di as mgd  # noqa: E402  (registers the stub modules, puts the reference root first on sys.path)
import pasmnet.utils as ref_utils  # noqa: E402  (the reference's module, imported by make_golden_dcmcs3di already)

assert hasattr(ref_utils, "output") and hasattr(ref_utils, "regress_disp"), "not the reference's pasmnet/utils.py"


def masks(w, rng):
    """rows of 0/1 masks for a row width w"""
    out = [np.zeros(w, np.uint8), np.ones(w, np.uint8)]
    one = np.zeros(w, np.uint8); one[0] = 1; out.append(one)
    one = np.zeros(w, np.uint8); one[-1] = 1; out.append(one)
    if w >= 3:
        m = np.ones(w, np.uint8); m[0] = 0; m[-1] = 0; out.append(m)                # holes at both row ends
        m = np.zeros(w, np.uint8); m[w // 2] = 1; out.append(m)                    # a single valid pixel inside
        out.append((np.arange(w) % 2).astype(np.uint8))                            # alternating
        out.append((1 - np.arange(w) % 2).astype(np.uint8))
    if w >= 37:
        m = np.ones(w, np.uint8); m[: w // 3] = 0; m[-(w // 4):] = 0; out.append(m)
    if w >= 130:
        m = np.ones(w, np.uint8); m[10:10 + 100] = 0; out.append(m)                # a hole of 100 px
        m = np.ones(w, np.uint8); m[w - 110:] = 0; out.append(m)                   # 110 px at the row's end
        m = np.ones(w, np.uint8); m[:105] = 0; out.append(m)                       # 105 px at the row's start
    if w >= 300:
        m = np.zeros(w, np.uint8); m[150] = 1; m[290] = 1; out.append(m)           # holes of 150 and 139 px
    for p in (0.1, 0.5, 0.9):
        for _ in range(3):
            out.append((rng.random(w) < p).astype(np.uint8))
    return np.stack(out)


def run_ref(att, valid):
    with torch.no_grad():
        return ref_utils.regress_disp(att, valid)


def main():
    out = {}
    rng = np.random.default_rng(2024)
    for w in (1, 37, 64, 130, 300):
        valid = masks(w, rng)
        rows = valid.shape[0]
        cols = rng.integers(0, w, size=(rows, w)).astype(np.int16)
        att = torch.zeros(1, rows, w, w)
        att.scatter_(3, torch.from_numpy(cols.astype(np.int64)).view(1, rows, w, 1), 1.0)
        disp = run_ref(att, torch.from_numpy(valid).float().view(1, 1, rows, w))
        out["onehot%d/cols" % w] = cols
        out["onehot%d/valid" % w] = valid
        out["onehot%d/disp" % w] = disp.view(rows, w).numpy()
    g = torch.Generator().manual_seed(7)
    cost = torch.randn(2, 8, 70, 70, generator=g) * 3
    att = torch.softmax(cost, dim=-1)
    valid = (torch.rand(2, 1, 8, 70, generator=g) < 0.7).float()
    valid[0, 0, 0] = 0
    valid[0, 0, 1] = 1
    valid[1, 0, 2, :40] = 0
    out["soft/att"] = att.numpy()
    out["soft/valid"] = valid.numpy().astype(np.uint8)
    out["soft/disp"] = run_ref(att, valid).numpy()
    m = mgd.build()
    small = np.load(os.path.join(OUT, "dcmcs3di_small.npz"))
    for name in ("a", "b"):
        left, right = torch.from_numpy(small[name + "/left"]), torch.from_numpy(small[name + "/right"])
        with torch.no_grad():
            _, (att, _, valid, _) = m(left, right, inference=True)
        out["model_%s/disp" % name] = run_ref(att[0], valid[0].float()).numpy()
        out["model_%s/disp_ini" % name] = run_ref(att[0], torch.ones_like(valid[0]).float()).numpy()
        out["model_%s/valid" % name] = valid[0].numpy().astype(np.uint8)
        print(name, "valid frac %.3f" % float(valid[0].float().mean()))
    np.savez_compressed(os.path.join(OUT, "disparity.npz"), torch=torch.__version__, **out)
    print("wrote disparity.npz, torch", torch.__version__, "%d bytes" % os.path.getsize(os.path.join(OUT, "disparity.npz")))


if __name__ == "__main__":
    main()
