#!/usr/bin/env python3
"""Diagnostic: phase breakdown (in-kernel s_memtime stamps, csrc/ct_stamps.h) of one convolution kernel on a C -> C 3x3 conv.

usage: tools/prof_conv.py <exact|split|ws|wino|wino4> [N C H W] [res|nores]
  (defaults: batch 2, 64 channels; 512x512 for exact / split, 1080p for the strip kernels; skip tensor as in KERNELS below)

The kernel must come from a library whose source was built with -DCT_STAMPS (one source per library):
    SRC=conv_<kernel> tools/build_variant.sh <kernel>_stamps -DCT_STAMPS        (e.g. SRC=conv_wino4 ... wino4_stamps -DCT_STAMPS)
-> color-transfer_amd/ct_hip/libct_tune_<kernel>_stamps.so, which this script selects (CT_HIP_LIB overrides it)."""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "color-transfer_amd"))

# per kernel: what the launch writes -- prof[block][wave of `waves`][slot of `slots`] -- the stamped waves to print as
# (wave, label, phase slots), the phase names by slot, and how ct_hip.conv2d is steered to the kernel
KERNELS = {
    "exact": dict(
        kernel="conv_mfma_kernel<3, 3, 2>", blocks=512, waves=1, slots=8, size=(512, 512), act=0, res=True,
        show=[(0, "wave 0", range(5))],
        names=["store_tile/acc-init", "barrier (tile visible)", "tap loop (MFMA + prefetch issue)", "epilogue", "barrier (tile free)"],
        steer=lambda ct: ct.set_conv_mode("exact")),
    "split": dict(      # bf16 three-piece form; CT_HIP_CONV_WS=0 keeps 3x3 / cin <= 64 on the tile kernel
        kernel="conv_split_kernel", blocks=512, waves=2, slots=8, size=(512, 512), act=0, res=False, env={"CT_HIP_CONV_WS": "0"},
        show=[(0, "wave 0", range(6)), (1, "wave 3 (weight streamer)", range(7))],
        names=["store_tile/acc-init", "barrier (tile visible)", "tap work (LDS reads + MFMA)", "epilogue", "barrier (tile free)",
               "per-tap barriers", "weights landed wait (wave 3)"],
        steer=lambda ct: (ct.set_conv_mode("split"), ct.set_conv_ws16(False))),
    "ws": dict(         # fp16 two-piece form by default; CT_HIP_CONV_WS16=0 = bf16 three-piece form
        kernel="conv_ws_kernel", blocks=256, waves=8, slots=8, size=(1080, 1920), act=1, res=True,
        show=[(0, "wave 0 (mt = 0)", range(7)), (4, "wave 4 (mt = 1)", range(7))],
        names=["X: partial sums -> LDS", "barrier (one per step)", "Y: staging (scale, pieces -> LDS)", "Y: requests (skip row, input row)",
               "other (prologue, weights)", "Y: row maximum", "X: reduce r-1 + MFMAs"],
        steer=lambda ct: ct.set_conv_wino(False)),
    "wino": dict(
        kernel="conv_wino_kernel", blocks=256, waves=8, slots=8, size=(1080, 1920), act=1, res=True,
        show=[(0, "wave 0", range(8)), (7, "wave 7", range(8))],
        names=["requests + scale", "T: transform, pieces -> B image", "barrier after T", "fragment reads + barrier", "MFMAs + M image",
               "barrier after C", "D: output transform, epilogue, stores", "staging of the next rows + 2 barriers"],
        steer=lambda ct: (ct.set_conv_wino(True), ct.set_conv_wino_form(1))),
    "wino4": dict(
        kernel="conv_wino4_kernel", blocks=256, waves=4, slots=10, size=(1080, 1920), act=1, res=True,
        show=[(0, "wave 0", range(6)), (3, "wave 3", range(6))],
        names=["head: maxima, touches, skip requests, fragments", "phase X: M A (blocks 0, 1), 48 MFMAs, T(s + 1)", "M A of blocks 2, 3 -> LDS",
               "barrier 1", "phase Y: 48 MFMAs of step s + 1, output side of s", "landed pair (wait, fix-ups, maximum) + barrier 2"],
        steer=lambda ct: (ct.set_conv_wino(True), ct.set_conv_wino_form(0))),
}


def main(argv):
    if len(argv) < 2 or argv[1] not in KERNELS:
        sys.exit(__doc__)
    which, k = argv[1], KERNELS[argv[1]]
    nums = [int(v) for v in argv[2:] if v.isdigit()]
    N, C, H, W = (nums + [2, 64, k["size"][0], k["size"][1]][len(nums):])[:4]
    use_res = {"res": True, "nores": False}.get(argv[-1], k["res"])
    os.environ.setdefault("CT_HIP_LIB", os.path.join(ROOT, "color-transfer_amd", "ct_hip", "libct_tune_%s_stamps.so" % which))
    os.environ.update(k.get("env", {}))
    import numpy as np
    import torch
    import ct_hip
    k["steer"](ct_hip)
    x = torch.randn(N, C, H, W, device="cuda")
    wt = torch.randn(C, C, 3, 3, device="cuda") / 24
    b = torch.randn(C, device="cuda")
    wp, bp = ct_hip.pack_conv_weight(wt, b)
    out = torch.empty_like(x)
    prof = torch.zeros((k["blocks"], k["waves"], k["slots"]), dtype=torch.int64, device="cuda")
    set_buffer = ct_hip.lib().ct_set_stamp_buffer       # only a -DCT_STAMPS build has it
    set_buffer.argtypes, set_buffer.restype = [ctypes.c_void_p], None
    set_buffer(ctypes.c_void_p(prof.data_ptr()))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(4):
        if i == 3:
            e0.record()
        ct_hip.conv2d(x, wp, bp, C, 3, act=k["act"], residual=x if use_res else None, out=out)
    e1.record(); torch.cuda.synchronize()
    set_buffer(None)
    p = prof.cpu().numpy().astype(np.float64)
    print("%s: kernel %.1f us (stamped build, [%d, %d, %d, %d], skip=%s); s_memtime ticks per wave, median over workgroups"
          % (k["kernel"], e0.elapsed_time(e1) * 1e3, N, C, H, W, use_res))
    width = max(len(n) for n in k["names"])
    for wave, label, phases in k["show"]:
        q = p[:, wave, :][:, list(phases)]
        q = q[q.sum(axis=1) > 0]                        # workgroups that had no work stamp nothing
        if not len(q):
            sys.exit("no stamps: is %s a -DCT_STAMPS build of this kernel's source?" % os.environ["CT_HIP_LIB"])
        tot = q.sum(axis=1)
        print("  %s" % label)
        for j, i in enumerate(phases):
            print("    %-*s %10.0f  (%5.1f %%)" % (width, k["names"][i], np.median(q[:, j]), 100 * np.median(q[:, j] / tot)))
        print("    total %.0f" % np.median(tot))


if __name__ == "__main__":
    main(sys.argv)
