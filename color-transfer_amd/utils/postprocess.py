"""The per-frame loop of the reference's dataset postprocessing (utils/postprocess.py:91-144) on the device, bytes in, bytes out:

    left  = flip(left)[bbox] -> warpPerspective(H1) -> [bbox again]                        -> %04d_LD.png
    gt    = left_gt[bbox][bbox again]                                                       -> %04d_L.png
    right = right[bbox]      -> warpPerspective(H2) -> [bbox again] -> MK colour transfer to gt, as bytes -> %04d_R.png

`process_frames` is that loop body for a group of frames: two ct_hip.warp_perspective calls (the flip, the crop, the warp and the
second crop in one kernel each), one slice and one ct_hip.mk on bytes.  The command line reads the frames, groups them and writes
the three PNG files of every selected frame through utils.writer.FrameWriter.

What is NOT here: the homography estimation of lines 36-75 and 121-123 (SIFT, LoFTR, MAGSAC: once per sample, on libraries that
are absent offline).  The two matrices are an input, `homographies` in the sample's params.json.  cv2.VideoCapture's stand-in is the
Y4M container (utils/y4m.py; `ffmpeg -i left.mp4 -f yuv4mpegpipe left.y4m`): a stream is the file left.y4m / left_gt.y4m / right.y4m in
the sample directory, 8-bit 4:2:0, converted to RGB on the device (ct_hip.yuv420_to_rgb, `--yuv_matrix`; siting and range from the
file's header) -- or, as before, a folder of PNG frames (left/, left_gt/, right/, in sorted order).  Pixels keep the order of the PNG
files (RGB) where the reference works on cv2's BGR: the warp treats the channels alike, and MK differs only in the order in which
its 3 x 3 moments are summed, not in what it states.  cv2's fixed-point warp is restated, not linked (include/ct_hip.h: parity
unpinned).

    python -m utils.postprocess --root R --output O [--samples a,b] [--rate 10] [--frames 7] [--png_encoder host|device] [--yuv_matrix bt709|bt601]
"""
import argparse
import json
import os
from typing import NamedTuple

import numpy as np
import torch

STREAMS = ("left", "left_gt", "right")


def second_crop(bbox):
    """the window (x, y, w - x, h - y) that lines 134-136 keep of the w x h warped crop; x >= w or y >= h: ValueError (the
    reference would hand MK an empty array)"""
    x, y, w, h = (int(v) for v in bbox)
    if x < 0 or y < 0 or x >= w or y >= h:
        raise ValueError("bbox %r: the second crop [y:y+h, x:x+w] of the h x w warped crop is empty (needs 0 <= x < w, 0 <= y < h)" % (tuple(bbox),))
    return x, y, w - x, h - y


def process_frames(left, left_gt, right, H1, H2, bbox):
    """uint8 [B,H,W,3] device frames as decoded (left NOT yet flipped), H1 / H2 3 x 3 host matrices as cv2.warpPerspective takes
    them, bbox = (x, y, w, h).  Returns the byte tensors that lines 142-144 write, (LD, L, R), each [B, h - y, w - x, 3]."""
    import ct_hip
    x, y, w, h = (int(v) for v in bbox)
    window = second_crop(bbox)
    ld = ct_hip.warp_perspective(left, H1, crop=(x, y, w, h), flip_x=True, window=window)
    gt = left_gt[:, y:y + h, x:x + w][:, y:y + h, x:x + w].contiguous()
    if tuple(gt.shape) != tuple(ld.shape):
        raise ValueError("left_gt of shape %s does not hold bbox %r" % (tuple(left_gt.shape), (x, y, w, h)))
    warped = ct_hip.warp_perspective(right, H2, crop=(x, y, w, h), window=window)
    return ld, gt, ct_hip.mk(warped, gt, out_dtype=torch.uint8)


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Script for processing all samples")
    parser.add_argument("--root", type=str, required=True, help="Path to folder with all samples")
    parser.add_argument("--output", type=str, required=True, help="Path to output folder to save processed samples")
    parser.add_argument("--samples", type=str, help="Comma separated list of samples to process", required=False)
    parser.add_argument("--rate", type=int, default=10, help="Use each `rate` frame from sequences")
    parser.add_argument("--frames", type=int, default=7, help="How many frames select from each sample")
    parser.add_argument("--png_encoder", choices=("host", "device"), default="host", help="Where the PNG files are compressed")
    parser.add_argument("--yuv_matrix", choices=("bt601", "bt709"), default="bt709", help="Y'CbCr matrix of .y4m streams")
    return parser.parse_args(argv)


def select_frames(params, counts, rate, frames):
    """[(output number, {stream: index into its sorted frame list})] of one sample: frame_idx % rate == 0 for frame_idx <
    frames * rate, stream frame offsets.all + offsets.<stream> + frame_idx (lines 87-91, 124); a stream that ends early ends the
    sample, as a failed cap.read() would."""
    if rate < 1 or frames < 0:
        raise ValueError("rate must be >= 1 and frames >= 0 (got %r, %r)" % (rate, frames))
    first = {s: int(params["offsets"]["all"]) + int(params["offsets"][s]) for s in STREAMS}
    if any(v < 0 for v in first.values()):
        raise ValueError("negative first frame: offsets %r" % (params["offsets"],))
    picks = []
    for frame_idx in range(0, frames * rate, rate):
        at = {s: first[s] + frame_idx for s in STREAMS}
        if any(at[s] >= counts[s] for s in STREAMS):
            break
        picks.append((frame_idx // rate, at))
    return picks


class Y4MFrame(NamedTuple):
    """one frame of a .y4m stream, in the place of a PNG file's name"""
    path: str
    offset: int                 # of its first plane byte
    header: object              # utils.y4m.Header


def list_streams(sample_dir):
    """{stream: its frames in order}: the names of the PNG files in the folder <stream>/, or, when the sample directory holds
    <stream>.y4m, a Y4MFrame per frame of that file"""
    from utils import y4m
    out = {}
    for s in STREAMS:
        video = os.path.join(sample_dir, s + ".y4m")
        if os.path.isfile(video):
            head, offsets = y4m.frame_offsets(video)
            out[s] = [Y4MFrame(video, o, head) for o in offsets]
        else:
            out[s] = sorted(f for f in os.listdir(os.path.join(sample_dir, s)) if f.lower().endswith(".png"))
    return out


def frame_source(sample_dir, stream, entry):
    """what load_frames takes for one entry of list_streams"""
    return entry if isinstance(entry, Y4MFrame) else os.path.join(sample_dir, stream, entry)


def load_y4m_frames(frames, device, matrix="bt709"):
    """Y4MFrames of one stream -> uint8 [k,H,W,3] on `device`: the planes are read into one pinned buffer, uploaded in one
    asynchronous copy (1.5 bytes per pixel) and converted by one ct_hip.yuv420_to_rgb launch"""
    import ct_hip
    if torch.device(device).type != "cuda":
        raise ValueError(".y4m streams are converted on the GPU (ct_hip.yuv420_to_rgb): there is no CPU path")
    head = frames[0].header
    fb = head.frame_bytes
    host = torch.empty((len(frames), fb), dtype=torch.uint8).pin_memory()
    arr = host.numpy()
    for j, fr in enumerate(frames):
        with open(fr.path, "rb") as fh:
            fh.seek(fr.offset)
            if fh.readinto(memoryview(arr[j])) != fb:
                raise IOError("%s: a frame ends early" % fr.path)
    return ct_hip.yuv420_to_rgb(host.to(device, non_blocking=True), head.height, head.width, matrix=matrix,
                                range=head.color_range or "limited", siting=head.siting)


def load_frames(paths, device, yuv_matrix="bt709"):
    """PNG files -> uint8 [k,H,W,3] on `device`, through one pinned buffer and one asynchronous copy; Y4MFrames (list_streams of a
    .y4m stream) through load_y4m_frames"""
    if paths and isinstance(paths[0], Y4MFrame):
        return load_y4m_frames(paths, device, yuv_matrix)
    from PIL import Image
    arrays = [np.asarray(Image.open(p).convert("RGB")) for p in paths]
    host = torch.from_numpy(np.stack(arrays))
    if torch.device(device).type == "cuda":
        return host.pin_memory().to(device, non_blocking=True)
    return host


def process_sample(root, output, sample, rate, frames, png_encoder="host", device="cuda", yuv_matrix="bt709"):
    """one sample directory -> its %04d_{LD,L,R}.png files; returns the number of frames written"""
    from utils.writer import FrameWriter
    sample_dir = os.path.join(root, sample)
    with open(os.path.join(sample_dir, "params.json"), "r") as f:
        params = json.load(f)
    bbox = tuple(int(params["bbox"][k]) for k in ("x", "y", "w", "h"))
    H1 = np.asarray(params["homographies"]["left"], dtype=np.float64)
    H2 = np.asarray(params["homographies"]["right"], dtype=np.float64)
    names = list_streams(sample_dir)
    picks = select_frames(params, {s: len(names[s]) for s in STREAMS}, rate, frames)
    if not picks:
        return 0
    group = {}
    for s in STREAMS:
        sources = [frame_source(sample_dir, s, names[s][at[s]]) for _, at in picks]
        group[s] = load_y4m_frames(sources, device, yuv_matrix) if isinstance(sources[0], Y4MFrame) else load_frames(sources, device)
    outputs = process_frames(group["left"], group["left_gt"], group["right"], H1, H2, bbox)
    numbers = [number for number, _ in picks]
    with FrameWriter(os.path.join(output, sample), fmt="png", depth=3, png_encoder=png_encoder) as writer:
        for tag, frames_u8 in zip(("LD", "L", "R"), outputs):
            writer.submit(numbers, frames_u8, suffix=tag)
    # FrameWriter names frames %06d.<suffix>.png; the reference's names are %04d_<suffix>.png
    for number in numbers:
        for tag in ("LD", "L", "R"):
            os.replace(os.path.join(output, sample, "%06d.%s.png" % (number, tag)), os.path.join(output, sample, "%04d_%s.png" % (number, tag)))
    return len(numbers)


def main(argv=None):
    args = parse_args(argv)
    samples = args.samples.split(",") if isinstance(args.samples, str) else sorted(os.listdir(args.root))
    total = 0
    for sample in samples:
        total += process_sample(args.root, args.output, sample, args.rate, args.frames, args.png_encoder, yuv_matrix=args.yuv_matrix)
    print("postprocess: %d frames of %d samples written to %s" % (total, len(samples), args.output))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
