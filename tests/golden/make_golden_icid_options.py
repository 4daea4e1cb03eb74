#!/usr/bin/env python3
"""Golden values for iCID's three arguments by RUNNING the reference's utils/icid.py (build container only):

    python3 -B tests/golden/make_golden_icid_options.py

The recipe is make_golden_icid.py's: kornia.color.rgb_to_lab and torchvision's gaussian_blur, both absent offline, are stood in by
oracle.metrics.rgb_to_lab / gaussian_blur ("parity unpinned" for those two); every line of the reference's icid() itself is executed
as written, for intent in (perceptual, hue-preserving, chromatic) x omit_maps67 in (False, True) x downsampling in (True, False).
The frames are pairs a-d of icid.npz (read from there, not stored again), and a batch of two 48 x 64 pairs -- pair a and the top
left corner of pair b -- that pins the reference's mean over the batch.  Only values are written:

    <tag>/f64, <tag>/f32   float64 [3 intents][2: omit_maps67 False, True][2: downsampling True, False], tag in a b c d batch
                           (the reference on float64 tensors / as it runs, on float32 tensors)
    batch/frames_f64       the same for the two frames of the batch one at a time, [2][3][2][2]"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from oracle import metrics as om  # noqa: E402

for name in ("kornia", "kornia.color", "torchvision", "torchvision.transforms", "torchvision.transforms.functional"):
    sys.modules[name] = types.ModuleType(name)
sys.modules["kornia.color"].rgb_to_lab = om.rgb_to_lab
sys.modules["torchvision.transforms.functional"].gaussian_blur = om.gaussian_blur
spec = importlib.util.spec_from_file_location("ref_icid", "/root/reference/utils/icid.py")
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

INTENTS = ("perceptual", "hue-preserving", "chromatic")
OMIT = (False, True)
DOWN = (True, False)


def table(x, y):
    """[3][2][2] float64 of ref.icid(x, y, intent, omit, down)"""
    return np.array([[[np.float64(ref.icid(x, y, intent=i, omit_maps67=o, downsampling=d)) for d in DOWN] for o in OMIT] for i in INTENTS])


def main():
    g = np.load(os.path.join(OUT, "icid.npz"), allow_pickle=False)
    u8 = lambda a: torch.from_numpy(a.astype(np.float32) / np.float32(255))      # noqa: E731
    frames = {tag: (u8(g[tag + "/x_u8"]), u8(g[tag + "/y_u8"])) for tag in "abcd"}
    frames["batch"] = tuple(torch.cat([frames["a"][k], frames["b"][k][..., :48, :64]]).contiguous() for k in (0, 1))
    fix = {}
    for tag, (x, y) in frames.items():
        fix[tag + "/f32"] = table(x, y)
        fix[tag + "/f64"] = table(x.double(), y.double())
        print(tag, tuple(x.shape), "f64 min %.6f max %.6f, max |f32 - f64| %.2e"
              % (fix[tag + "/f64"].min(), fix[tag + "/f64"].max(), np.abs(fix[tag + "/f32"] - fix[tag + "/f64"]).max()))
    x, y = frames["batch"]
    fix["batch/frames_f64"] = np.stack([table(x[i:i + 1].double(), y[i:i + 1].double()) for i in range(2)])
    # the defaults are what icid.npz already holds, and the batch value is the mean of its frames' (one size)
    for tag in "abcd":
        assert fix[tag + "/f64"][0, 0, 0] == g[tag + "/icid_f64"] and fix[tag + "/f32"][0, 0, 0] == g[tag + "/icid_f32"], tag
    assert np.abs(fix["batch/frames_f64"].mean(0) - fix["batch/f64"]).max() < 1e-14
    np.savez_compressed(os.path.join(OUT, "icid_options.npz"), torch=torch.__version__, intents=np.array(INTENTS), **fix)
    print("wrote icid_options.npz")


if __name__ == "__main__":
    main()
