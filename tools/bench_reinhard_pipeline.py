#!/usr/bin/env python3
"""The float32 Reinhard sweeps over chunks of pairs (ct_set_reinhard_pipeline): pairs/s of ct_reinhard_psnr_f32 per setting, one
process, the caller on the legacy default stream like bench.py.  Settings: off, the built-in plan, then chunk_pairs 1, 2, 4, 8 x both
target-load policies; they ALTERNATE over the rounds (a drifting clock or a noisy neighbour then hits every setting alike) and each is reported
as median and range over the rounds.
usage: bench_reinhard_pipeline.py [--pairs 16] [--size 1080x1920] [--rounds 5] [--calls 100] [--json FILE]
With --json the table is also written as a stamped summary (tools/stamp.py) for profiles/."""
import argparse, json, os, socket, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "color-transfer_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import torch
import ct_hip
import stamp

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, nargs="+", default=[16])
ap.add_argument("--size", nargs="+", default=["1080x1920"])
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--calls", type=int, default=100)
ap.add_argument("--json", default=None)
args = ap.parse_args()

SETTINGS = [(0, "nt"), (-1, -1)] + [(c, p) for c in (1, 2, 4, 8) for p in ("nt", "plain")]


def name(c, p):
    return "off" if c == 0 else "built-in plan" if c < 0 else "chunk %d %s" % (c, p)


def rate(call, n):
    for _ in range(10):
        call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        call()
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


torch.manual_seed(0)
tables = []
for size in args.size:
    H, W = (int(v) for v in size.split("x"))
    for B in args.pairs:
        t, r, g = (torch.rand(B, H, W, 3, device="cuda") for _ in range(3))
        out, ps = torch.empty_like(t), torch.zeros(B, 2, dtype=torch.float64, device="cuda")
        call = lambda: ct_hip.reinhard_psnr(t, r, g, out=out, psnr_out=ps)
        got = {s: [] for s in SETTINGS}
        try:
            for rnd in range(args.rounds):
                order = SETTINGS if rnd % 2 == 0 else SETTINGS[::-1]
                for s in order:
                    ct_hip.set_reinhard_pipeline(*s)
                    got[s].append(B * rate(call, args.calls))
        finally:
            ct_hip.set_reinhard_pipeline(-1, -1)
        rows = []
        print("%dx%d, %d pairs per call, %d rounds of %d calls: pairs/s median (min .. max)" % (H, W, B, args.rounds, args.calls))
        for s in SETTINGS:
            v = got[s]
            rows.append({"setting": name(*s), "chunk_pairs": s[0], "t_policy": s[1],
                         "chunk_pairs_run": ct_hip.reinhard_pipeline_chunk(H * W, B) if s[0] < 0 else min(s[0], B), "pairs_per_s_median": statistics.median(v),
                         "pairs_per_s_min": min(v), "pairs_per_s_max": max(v), "rounds": v})
            print("  %-14s %8.0f (%8.0f .. %8.0f)" % (name(*s), statistics.median(v), min(v), max(v)), flush=True)
        tables.append({"height": H, "width": W, "pairs_per_call": B, "settings": rows})
        del t, r, g, out, ps
        torch.cuda.empty_cache()
if args.json:
    with open(args.json, "w") as f:
        json.dump({"source_stamp": stamp.source_stamp(), "box": socket.gethostname(), "device": torch.cuda.get_device_name(0),
                   "entry": "ct_reinhard_psnr_f32, caller on the legacy default stream", "rounds": args.rounds, "calls_per_round": args.calls,
                   "tables": tables}, f, indent=1)
        f.write("\n")
