#!/usr/bin/env python3
"""Times the metric entries on frame groups (ct_frame_*_hwc_u8) and the route behind `--model.metric_groups true`, 1080p frames
resident in HBM, in ONE session (HIP events, median of rounds, the legs alternating round by round):
  (a) per metric (SSIM, FSIM, iCID): the new entry on the group's own buffers -- 12 + 3 = 15 B read per pixel -- against the planar
      entry WITH the passes that feed it from a group: clamp + permute of the result (12 + 12 B), convert + permute of the ground
      truth (3 + 12 B), then 24 B read = 63 B per pixel by the count of the shapes (torch makes the clamp and the permute two
      passes each, so it moves more than that)
  (b) Runner(REINHARD, metric_groups=True).test_group_metrics with all four metrics against test_group alone (transfer + PSNR)
  (c) `utils.cli test` on `synthetic: video_u8` with all four metrics, `--model.metric_groups true` against the same command without
      the flag (the per-frame route: what the command did before the flag existed), through utils.cli.main(..., timing=...); each
      command twice, alternating, the second runs reported (the first ones load code objects and build the FSIM filter bank)
Prints frames/s and, where the bytes of a leg are known, the fraction of the HBM peak (8 TB/s) on them.
usage: tools/bench_metric_groups.py [frames=16] [cli_frames=48]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "color-transfer_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ct_hip  # noqa: E402
from methods import REINHARD_SPEC, Runner  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
CLI_FRAMES = int(sys.argv[2]) if len(sys.argv) > 2 else 48
H, W = 1080, 1920
PEAK = 8e12
g = torch.Generator(device="cuda").manual_seed(0)
group = torch.randint(0, 256, (3, B, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
gt8 = group[2]
# an unclamped float32 HWC result, as a grouped transfer leaves it: the ground truth with a gain about mid-grey and noise
res = ((gt8.float() / 255 - 0.5) * 1.25 + 0.5 + 0.03 * torch.randn((B, H, W, 3), device="cuda", generator=g)).contiguous()


def one_round(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e-3


def race(legs, n, rounds=7):
    """legs: (name, fn, bytes per pixel or None); prints one line per leg, returns {name: median seconds per call}"""
    for _, fn, _ in legs:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in legs}
    for _ in range(rounds):
        for name, fn, _ in legs:
            times[name].append(one_round(fn, n))
    med = {}
    for name, _, bpp in legs:
        med[name], best = float(np.median(times[name])), float(np.min(times[name]))
        share = "  %2d B/pixel  frac of 8 TB/s %.3f" % (bpp, bpp * H * W * B / med[name] / PEAK) if bpp else ""
        print("[B=%d 1080p] %-28s %9.1f us/call  %8.0f frames/s (best %8.0f)%s" % (B, name, med[name] * 1e6, B / med[name], B / best, share),
              flush=True)
    return med


# ---- (a) the entries ------------------------------------------------------------------------------------------------------------------
def planar_route(fn):
    def run():
        x = res.clamp(0, 1).permute(0, 3, 1, 2).contiguous()
        y = (gt8.float() / 255).permute(0, 3, 1, 2).contiguous()
        return fn(x, y)
    return run


for name, new, old in (("ssim", ct_hip.frame_ssim_hwc, ct_hip.frame_ssim), ("icid", ct_hip.frame_icid_hwc, ct_hip.frame_icid),
                       ("fsim", ct_hip.frame_fsim_hwc, ct_hip.frame_fsim)):
    m = race(((name + " hwc_u8", lambda new=new: new(res, gt8), 15), (name + " passes + planar", planar_route(old), 63)), n=5)
    # torch's device `/ 255` is a multiplication by a reciprocal: the planar leg sees a ground truth that is off by an ulp here and
    # there, so the two legs agree closely, not bitwise (the bitwise contract is tests/test_metric_groups_gpu.py, converted on the host)
    diff = float((new(res, gt8) - planar_route(old)()).abs().max())
    print("    %s: the passes + the planar entry take %.2f x the time of the entry on the group's buffers; max |difference| of the results %.3g"
          % (name, m[name + " passes + planar"] / m[name + " hwc_u8"], diff), flush=True)

# ---- (b) the Runner --------------------------------------------------------------------------------------------------------------------
model = Runner(REINHARD_SPEC, metric_groups=True)
rec = torch.zeros((B, 2), dtype=torch.float64, device="cuda")
table = torch.zeros((B, 4), dtype=torch.float64, device="cuda")
m = race((("test_group (transfer + PSNR)", lambda: model.test_group(group, rec), None),
          ("test_group_metrics (all four)", lambda: model.test_group_metrics(group, table), None)), n=3)
print("    the three further metrics add %.1f us per frame to test_group's %.1f us per frame"
      % ((m["test_group_metrics (all four)"] - m["test_group (transfer + PSNR)"]) / B * 1e6, m["test_group (transfer + PSNR)"] / B * 1e6), flush=True)
del group, res, gt8
torch.cuda.empty_cache()

# ---- (c) the command --------------------------------------------------------------------------------------------------------------------
import utils.data as data  # noqa: E402
from utils import cli  # noqa: E402

# every cli.main builds its own dataset, and the per-frame route would generate the synthetic chunks inside its timed loop (the
# grouped route's prepare() makes them before the clock starts): one pool for the whole session, made before the first command
_pool, _make = {}, data.SyntheticStereoVideoU8._chunk


def _chunk(self, i):
    key = (i, self.group, self.height, self.width)
    if key not in _pool:
        self._chunks = None
        _pool[key] = _make(self, i)
    return _pool[key]


data.SyntheticStereoVideoU8._chunk = _chunk
video = data.SyntheticStereoVideoU8(CLI_FRAMES, H, W)
for f in range(CLI_FRAMES):
    video.host_chunk(f)
ARGS = ["test", "--config", os.path.join(ROOT, "color-transfer_amd", "configs", "others.yaml"), "--model.func_spec", REINHARD_SPEC,
        "--data.data_dir", "null", "--data.synthetic", "video_u8", "--data.n_frames", str(CLI_FRAMES), "--data.height", str(H), "--data.width", str(W)]
runs = {"flagged": [], "plain": []}
for _ in range(2):
    for name, extra in (("flagged", ["--model.metric_groups", "true"]), ("plain", [])):
        timing = {}
        cli.main(ARGS + extra, timing=timing)
        assert timing["grouped"] is (name == "flagged")
        runs[name].append(timing["frames"] / timing["seconds"])
print("[cli test, %d frames 1080p, all four metrics] --model.metric_groups true %8.1f frames/s (first run %.1f);  without the flag %8.1f frames/s "
      "(first run %.1f);  ratio %.2f" % (CLI_FRAMES, runs["flagged"][1], runs["flagged"][0], runs["plain"][1], runs["plain"][0],
                                         runs["flagged"][1] / runs["plain"][1]), flush=True)
