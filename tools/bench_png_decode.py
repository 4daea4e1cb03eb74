#!/usr/bin/env python3
"""Time the device PNG decoder (csrc/png_decode.hip: ct_hip.png_decode = inflate + unfilter) against PIL on the same bytes, and write
a stamped summary (tools/stamp.py).  Nothing here is on a timed path and no time is gated: one stream occupies one wave, nobody has
measured how many symbols per second a wave decodes, and the comparison that matters is device frames/s against 16 host threads.

    inputs   PIL-written 1080p PNG files of SyntheticArtificialTest's texture (structured, not noise), compress levels 1 and 6,
             `--pool` distinct frames each, cycled to fill a call
    device   ct_hip.png_decode of 3, 24, 96 and 384 files per call, between events (the upload of the compressed bytes inside,
             as utils.data.prefetch_decoded pays it); best of `--reps`
    host     PIL (Image.open + convert + load) of 96 of the same files with 1 thread and with 16 (zlib releases the GIL)

usage: tools/bench_png_decode.py [--out profiles/png_decode_timing.json] [--reps 3] [--height 1080 --width 1920] [--pool 6]"""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "color-transfer_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ct_hip  # noqa: E402
from stamp import source_stamp  # noqa: E402
from utils import png  # noqa: E402
from utils.data import SyntheticArtificialTest  # noqa: E402

BATCHES = (3, 24, 96, 384)


def pil_decode(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--pool", type=int, default=6)
    a = ap.parse_args()
    from PIL import Image
    torch.cuda.set_device(0)
    frames = SyntheticArtificialTest(a.pool, a.height, a.width)
    res = {"source_stamp": source_stamp(), "device": torch.cuda.get_device_name(0), "height": a.height, "width": a.width, "levels": {}}
    for level in (1, 6):
        files = []
        for i in range(a.pool):
            buf = io.BytesIO()
            Image.fromarray(frames.load_pair(i)[0].permute(1, 2, 0).numpy()).save(buf, format="PNG", compress_level=level)
            files.append(buf.getvalue())
        items = [(torch.frombuffer(bytearray(info.payload), dtype=torch.uint8), info.height, info.width) for info in map(png.parse, files)]
        got = ct_hip.png_decode(items[:1])[0].cpu().numpy()
        assert np.array_equal(got, pil_decode(files[0]).transpose(2, 0, 1)), "the device decoder and PIL disagree"
        entry = {"file_bytes": int(np.mean([len(f) for f in files])), "device": {}, "pil": {}}
        for n in BATCHES:
            batch = [items[i % a.pool] for i in range(n)]
            times = []
            for r in range(a.reps + 1):                     # the first pass untimed
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                ct_hip.png_decode(batch, check=False)
                t1.record()
                torch.cuda.synchronize()
                if r:
                    times.append(t0.elapsed_time(t1))
            best = min(times)
            entry["device"][str(n)] = {"ms_per_call": best, "frames_per_s": 1e3 * n / best}
            print("level %d, %3d files per call: %.1f ms, %.0f frames/s" % (level, n, best, 1e3 * n / best), flush=True)
        work = [files[i % a.pool] for i in range(96)]
        for threads in (1, 16):
            with ThreadPoolExecutor(threads) as pool:
                list(pool.map(pil_decode, work[:threads]))
                t0 = time.perf_counter()
                list(pool.map(pil_decode, work))
                dt = time.perf_counter() - t0
            entry["pil"][str(threads)] = {"frames_per_s": len(work) / dt}
            print("level %d, PIL with %d threads: %.0f frames/s" % (level, threads, len(work) / dt), flush=True)
        res["levels"][str(level)] = entry
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
