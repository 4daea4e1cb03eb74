#!/usr/bin/env python3
"""Time the output path of `utils.cli predict` on the GPU and write a stamped summary (tools/stamp.py):

  * ct_pack_u8_f32 (csrc/pack.hip) alone, with events, at 1080p, n = 1 and 8, both layouts: bytes per call = 5 * n * H * W * 3
    (4 read + 1 written per element; 31 104 000 per 1080p frame), achieved TB/s and the fraction of the 8 TB/s HBM peak.  The
    inputs rotate through a pool larger than the 256 MB last-level cache, so that a frame is read from HBM, as in the pipeline;
  * `utils.cli predict --format null` (the download ring without the disk) and `--format raw` (+ the box's disk / page cache)
    against `utils.cli test` on the same loader in the same process, alternated: `synthetic: video_u8`, --frames frames, group 8,
    `metrics: psnr`; the timing is main(..., timing=...)'s (one untimed warm pass inside it);
  * `--format png` on --png-frames frames with both encoders, same session, same frames, 16 workers: `host` (PIL encodes on the
    writer's workers) and `device` (`--writer.png_encoder device`: ct_png_deflate_u8, csrc/png.hip, the workers only wrap the streams),
    on the synthetic video (uniform random bytes) through `predict`; the sizes of the files of both encoders;
  * ct_png_deflate_u8 alone, with events, on a group of 8 1080p frames of noise (stored chunks) and of a smooth ramp (Huffman
    chunks): us per group, bytes in and out.

usage: tools/bench_predict.py [--out profiles/predict_timing.json] [--frames 1000] [--reps 3] [--kernels-only] [--workdir DIR]
For the copy / kernel overlap use rocprofv3 --kernel-trace --memory-copy-trace --stats -- python3 tools/bench_predict.py --trace-run
(or --trace-png for the device PNG encoder)."""
import argparse
import contextlib
import io
import json
import os
import shutil
import sys
import tempfile

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


def kernels(reps, res):
    out = {}
    for n in (1, 8):
        in_bytes = 4 * n * H * W * 3
        pool = max(2, (2 * CACHE_BYTES + in_bytes - 1) // in_bytes)
        for layout in ("hwc", "chw"):
            shape = (n, H, W, 3) if layout == "hwc" else (n, 3, H, W)
            xs = [torch.rand(shape, device="cuda") for _ in range(pool)]
            o = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
            for x in xs:
                ct_hip.pack_u8(x, layout, out=o)
            torch.cuda.synchronize()
            best = None
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(4):
                    for x in xs:
                        ct_hip.pack_u8(x, layout, out=o)
                b.record()
                torch.cuda.synchronize()
                ms = a.elapsed_time(b) / (4 * pool)
                best = ms if best is None else min(best, ms)
            nbytes = 5 * n * H * W * 3
            out["%s_n%d" % (layout, n)] = {"us_per_call": 1e3 * best, "bytes_per_call": nbytes, "tb_per_s": nbytes / (best * 1e-3) / 1e12,
                                            "hbm_frac": nbytes / (best * 1e-3) / HBM_PEAK, "input_pool": pool}
            del xs
    res["pack_1080p"] = out
    res["pack_bytes_per_1080p_frame"] = 5 * H * W * 3
    res["hbm_peak_tb_per_s"] = HBM_PEAK / 1e12


def png_kernel(reps, res):
    """ct_png_deflate_u8 alone on groups of 8: uniform noise (what the synthetic video holds: every chunk ends up stored) and
    smooth frames (a ramp with +-3 grey levels of noise: every chunk Huffman-coded)"""
    ramp = (torch.arange(W, device="cuda")[None, :, None] * 0.1 + torch.arange(H, device="cuda")[:, None, None] * 0.15 + torch.tensor([0.0, 40.0, 90.0], device="cuda"))
    smooth = (ramp[None] + torch.randint(-3, 4, (8, H, W, 3), device="cuda")).clamp(0, 255).to(torch.uint8).contiguous()
    groups = {"noise": torch.randint(0, 256, (8, H, W, 3), dtype=torch.uint8, device="cuda"), "smooth": smooth}
    out = {}
    for name, frames in groups.items():
        bufs = ct_hip.png_deflate(frames)
        torch.cuda.synchronize()
        best = None
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(10):
                ct_hip.png_deflate(frames, out=bufs)
            b.record()
            torch.cuda.synchronize()
            ms = a.elapsed_time(b) / 10
            best = ms if best is None else min(best, ms)
        out[name] = {"us_per_group_of_8": 1e3 * best, "bytes_in": frames.numel(), "bytes_out": int(bufs[1].sum().item()),
                     "chunks": int(bufs[1].numel()), "frames_per_s_kernel_alone": 8 / (best * 1e-3)}
    res["png_deflate_1080p"] = out


def _cli(cmd, frames, extra):
    from utils import cli
    timing = {}
    args = [cmd, "--config", os.path.join(ROOT, "color-transfer_amd", "configs", "others.yaml"), "--model.metrics", "psnr",
            "--data.data_dir", "null", "--data.synthetic", "video_u8", "--data.n_frames", str(frames), "--data.height", str(H),
            "--data.width", str(W)] + extra
    with contextlib.redirect_stdout(io.StringIO()):
        cli.main(args, timing=timing)
    return timing["frames"] / timing["seconds"]


def pipeline(frames, png_frames, reps, workdir, res):
    runs = {"test": [], "predict_null": [], "predict_raw": []}
    for _ in range(reps):                                   # alternated in one process
        runs["test"].append(_cli("test", frames, []))
        runs["predict_null"].append(_cli("predict", frames, ["--output", os.path.join(workdir, "null"), "--format", "null"]))
        runs["predict_raw"].append(_cli("predict", frames, ["--output", os.path.join(workdir, "raw"), "--format", "raw"]))
        shutil.rmtree(os.path.join(workdir, "raw"), ignore_errors=True)
    workers = 16
    png = _cli("predict", png_frames, ["--output", os.path.join(workdir, "png"), "--format", "png", "--writer.workers", str(workers)])
    png_dev, sizes = [], {}
    for _ in range(reps):
        png_dev.append(_cli("predict", frames, ["--output", os.path.join(workdir, "png_dev"), "--format", "png", "--writer.workers", str(workers),
                                                "--writer.png_encoder", "device"]))
    for name in ("png", "png_dev"):                         # the first --png-frames files of both encoders: the same frames
        d = os.path.join(workdir, name)
        sizes[name] = sum(os.path.getsize(os.path.join(d, "%06d.png" % f)) for f in range(png_frames)) / png_frames
        shutil.rmtree(d, ignore_errors=True)
    best = {k: max(v) for k, v in runs.items()}
    res["cli_video_u8_1080p"] = {
        "frames": frames, "group": 8, "frames_per_s_all": runs, "frames_per_s": best,
        "predict_null_over_test": best["predict_null"] / best["test"],
        "predict_raw_over_test": best["predict_raw"] / best["test"],
        "serialised_link_ratio": 18.7 / (18.7 + 6.2),
        "h2d_gb_per_s_test": best["test"] * 3 * H * W * 3 / 1e9,
        "h2d_gb_per_s_predict_null": best["predict_null"] * 3 * H * W * 3 / 1e9,
        "d2h_gb_per_s_predict_null": best["predict_null"] * H * W * 3 / 1e9,
        "raw_note": "predict_raw also measures this box's disk / page cache",
        "png": {"frames": png_frames, "frames_per_s": png, "workers": workers, "note": "host-bound: PIL encodes on the writer's workers"},
        "png_device": {"frames": frames, "frames_per_s_all": png_dev, "frames_per_s": max(png_dev), "workers": workers,
                       "over_png_host": max(png_dev) / png, "over_predict_null": max(png_dev) / best["predict_null"],
                       "over_predict_raw": max(png_dev) / best["predict_raw"],
                       "file_bytes_host": sizes["png"], "file_bytes_device": sizes["png_dev"], "file_size_ratio": sizes["png_dev"] / sizes["png"]},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--png-frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--trace-run", action="store_true", help="one short predict --format null pass and nothing else (for rocprofv3)")
    ap.add_argument("--trace-png", action="store_true", help="one short predict --format png --writer.png_encoder device pass (for rocprofv3)")
    ap.add_argument("--workdir", default=None, help="where predict writes (default: a temporary directory, removed afterwards)")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    workdir = a.workdir or tempfile.mkdtemp(prefix="bench_predict_")
    try:
        if a.trace_png:
            print("predict png (device encoder): %.1f frames/s" % _cli("predict", min(a.frames, 96), [
                "--output", os.path.join(workdir, "png"), "--format", "png", "--writer.workers", "16", "--writer.png_encoder", "device"]))
            return
        if a.trace_run:
            print("predict null: %.1f frames/s" % _cli("predict", min(a.frames, 96), ["--output", os.path.join(workdir, "null"), "--format", "null"]))
            return
        res = {"source_stamp": source_stamp(), "device": torch.cuda.get_device_name(0)}
        kernels(a.reps, res)
        png_kernel(a.reps, res)
        if not a.kernels_only:
            pipeline(a.frames, a.png_frames, a.reps, workdir, res)
    finally:
        if not a.workdir:
            shutil.rmtree(workdir, ignore_errors=True)
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
