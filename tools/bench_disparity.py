#!/usr/bin/env python3
"""Time the disparity of the parallax attention (csrc/disparity.hip, the IDX variants of csrc/attention16.hip) on the GPU and write
a stamped summary (tools/stamp.py):

  * DCMCS3DI forward_parts at 1080p (full depth, default config) with and without want_disp, alternated in one process;
  * the attend pass at 1080p rows alone, plain (ct_attention_rows64_f32) against fused (ct_attention_rows64_disp_f32), and the
    index-only pass;
  * ct_pam_disp_fill_f32 at 1080 x 1920 on a mask with holes;
  * ct_pam_regress_disp_f32 at 512 x 512 (B = 1) as a share of the 8 TB/s HBM peak on its 4 W^2 H bytes of attention.

usage: tools/bench_disparity.py [--out profiles/disparity.json] [--reps N]
For the kernel-level numbers use rocprofv3 --kernel-trace --stats -- python3 tools/bench_disparity.py --kernels-only."""
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
    lib = ct_hip.lib()
    torch.manual_seed(0)
    n, w = 1080, 1920
    q, k = torch.randn(n, w, 64, device="cuda") * 2, torch.randn(n, w, 64, device="cuda") * 2
    v = torch.randn(n, w, 96, device="cuda")
    out, disp = torch.empty(n, w, 96, device="cuda"), torch.empty(n, w, device="cuda")
    s = 1.0 / 64
    st = ct_hip._stream()
    plain = lambda: ct_hip.check(lib.ct_attention_rows64_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), None, n, w, s, st))
    fused = lambda: ct_hip.check(lib.ct_attention_rows64_disp_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), disp.data_ptr(), n, w, s, st))
    index = lambda: ct_hip.check(lib.ct_attention_rows64_disp_f32(q.data_ptr(), k.data_ptr(), None, None, disp.data_ptr(), n, w, s, st))
    t = {"plain": [], "fused": []}
    for _ in range(3):                                   # alternated
        t["plain"].append(event_ms(plain, reps))
        t["fused"].append(event_ms(fused, reps))
    res["attend_1080p_rows_ms"] = {kk: min(vv) for kk, vv in t.items()}
    res["attend_1080p_rows_ms"]["index_only"] = event_ms(index, reps)
    # the fill on a 1080p mask with holes (10 % of the pixels in holes of 1..64 px, a few long ones)
    g = torch.Generator(device="cuda").manual_seed(1)
    valid = (torch.rand(1, 1, 1080, 1920, device="cuda", generator=g) > 0.02).float()
    valid = (torch.nn.functional.max_pool2d(1 - valid, (1, 9), 1, (0, 4)) < 0.5).float()
    valid[0, 0, ::50, 300:900] = 0
    dini = torch.randn(1, 1, 1080, 1920, device="cuda", generator=g) * 40
    dout = torch.empty_like(dini)
    fill = lambda: ct_hip.check(lib.ct_pam_disp_fill_f32(dini.data_ptr(), valid.data_ptr(), dout.data_ptr(), 1, 1080, 1920, st))
    res["disp_fill_1080p_us"] = 1e3 * min(event_ms(fill, reps * 4) for _ in range(3))
    res["disp_fill_1080p_invalid_frac"] = float(1 - valid.mean())
    # regress_disp at 512^2: one pass over 4 W^2 H bytes
    h = w2 = 512
    att = torch.softmax(torch.randn(1, h, w2, w2, device="cuda", generator=g) * 4, dim=-1)
    v2 = (torch.rand(1, 1, h, w2, device="cuda", generator=g) > 0.2).float()
    d2 = torch.empty(1, 1, h, w2, device="cuda")
    reg = lambda: ct_hip.check(lib.ct_pam_regress_disp_f32(att.data_ptr(), v2.data_ptr(), d2.data_ptr(), 1, h, w2, st))
    ms = min(event_ms(reg, reps) for _ in range(3))
    nbytes = 4.0 * w2 * w2 * h
    res["regress_disp_512_us"] = 1e3 * ms
    res["regress_disp_512_hbm_frac"] = nbytes / (ms * 1e-3) / HBM_PEAK


def forward(reps, res):
    sys.path.insert(0, ROOT)
    from tests.dcmcs3di_common import build_model
    m = build_model(seed=11).cuda()
    g = torch.Generator().manual_seed(12)
    left, right = torch.rand(1, 3, 1080, 1920, generator=g).cuda(), torch.rand(1, 3, 1080, 1920, generator=g).cuda()
    t = {"plain": [], "want_disp": [], "disparity()": []}
    for _ in range(3):                                   # alternated in one process
        t["plain"].append(event_ms(lambda: m.forward_parts(left, right), reps))
        t["want_disp"].append(event_ms(lambda: m.forward_parts(left, right, want_disp=True), reps))
        t["disparity()"].append(event_ms(lambda: m.disparity(left, right), reps))
    res["forward_1080p_ms"] = {kk: min(vv) for kk, vv in t.items()}
    res["forward_1080p_ms_all"] = t
    res["forward_1080p_want_disp_added_frac"] = res["forward_1080p_ms"]["want_disp"] / res["forward_1080p_ms"]["plain"] - 1


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
