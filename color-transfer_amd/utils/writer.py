"""`FrameWriter` -- the download half of the data path: corrected uint8 frames leave the GPU and land in files, the mirror image
of `utils.data.prefetch_groups` (the reference writes its results with img_as_ubyte + PNG files, utils/postprocess.py:138-144).

    with FrameWriter(out_dir, fmt="png", depth=3, workers=4) as w:
        done = w.submit([17, 18], frames_u8)        # uint8 [k,H,W,3], device or host; frame numbers name the files

A ring of `depth` PINNED host buffers: `submit` takes the next slot (blocking while its previous frames are still being written:
that is the back-pressure, host memory stays at `depth` slots), lets a copy stream wait for the caller's stream, issues ONE
asynchronous copy of the whole group into the slot and returns the copy's event; the caller's stream is never synchronised.
Worker threads wait for that event, write the slot's frames and release the slot.  Host tensors skip the copy (they are held by
reference until written: the caller must not modify them).

Files are named by FRAME INDEX (`%06d.png`, `%06d.npy`; `raw`: frame f at offset f*H*W*3 of `frames.rgb`, rgb24, what
`ffmpeg -f rawvideo -pix_fmt rgb24 -s WxH` reads), so the ranks of a sharded run write disjoint files -- or disjoint ranges of
the one raw file -- into one directory and the result does not depend on the world size.  `null` downloads and drops.
`submit(..., suffix="chess")` names its frames `%06d.chess.png` / `.npy` instead: further images of the same frame (the diagnostic
views of `predict --views`) go through the same ring beside the frame itself; a raw video is one file and takes no suffix.

`png_encoder="device"` (with `fmt="png"`): the compressed bytes of a PNG file are made on the GPU.  `submit` of a DEVICE tensor runs
`ct_hip.png_deflate` on the caller's stream into a device buffer of the slot (filtered rows -> Huffman-coded deflate streams, one per
16 rows), the slot's one asynchronous copy downloads the streams with their sizes and Adler-32 parts instead of the frames, and the
workers only wrap them (`utils.png.assemble`: ~60 bytes of container and one CRC-32) and write the file.  The files decode to the
same pixels as the host encoder's; they are larger (no LZ77 matching).  HOST tensors have no device to encode on: they keep the PIL
path under `"device"` too.  Back-pressure, errors, suffixes and the returned event are those of the host encoder; the other formats
ignore the option.

`fmt="y4m"` (with `n_frames` and `y4m=dict(fps=, aspect=, matrix=, range=, siting=)`): ONE file `frames.y4m`, 8-bit 4:2:0, that an
encoder takes directly.  `submit` of DEVICE frames runs `ct_hip.rgb_to_yuv420` on the caller's stream into a device buffer of the slot,
the slot's one asynchronous copy downloads the [k, frame_bytes] planes (1.5 bytes per pixel instead of 3) and the workers `pwrite`
`FRAME\n` + planes at header_len + f * (6 + frame_bytes).  `truncate_y4m` writes the header once per run, as `truncate_raw` does for
the raw file; sharded ranks write only their own frames and `close()` sets the full length.  Suffixed frames and host tensors are
refused.

The first error of a worker (unwritable directory, full disk) is kept and raised from the next `submit` or from `close()`."""
import os
import queue
import threading

import numpy as np
import torch

FORMATS = ("png", "npy", "raw", "y4m", "null")
PNG_ENCODERS = ("host", "device")
MAX_WORKERS = 16
RAW_NAME = "frames.rgb"
Y4M_NAME = "frames.y4m"
Y4M_KEYS = ("fps", "aspect", "matrix", "range", "siting")
Y4M_DEFAULTS = {"fps": "25:1", "aspect": "1:1", "matrix": "bt709", "range": "limited", "siting": "center"}
Y4M_CHOICES = {"matrix": ("bt601", "bt709"), "range": ("limited", "full"), "siting": ("center", "left")}


def frame_name(index, fmt, suffix=None):
    return "%06d.%s" % (index, fmt) if suffix is None else "%06d.%s.%s" % (index, suffix, fmt)


def truncate_raw(out_dir):
    """Create `out_dir`/frames.rgb empty.  ONE process of a sharded run does this before the others open the file (and before a
    barrier): the writers themselves never truncate, they only write their frames' ranges."""
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, RAW_NAME), "wb"):
        pass


def y4m_options(y4m=None):
    """the `y4m` argument of FrameWriter / truncate_y4m -> the complete dict; unknown keys and values raise ValueError"""
    opts = dict(Y4M_DEFAULTS)
    for k, v in (y4m or {}).items():
        if k not in Y4M_KEYS:
            raise ValueError("y4m option %r: one of %s" % (k, ", ".join(Y4M_KEYS)))
        if v is not None:
            opts[k] = v
    for k, choices in Y4M_CHOICES.items():
        if opts[k] not in choices:
            raise ValueError("y4m %s %r: one of %s" % (k, opts[k], ", ".join(choices)))
    from utils import y4m as container
    container.header(2, 2, opts["fps"], opts["aspect"], opts["siting"], opts["range"])       # the ratios: refused here, not in a worker
    return opts


def y4m_header(height, width, y4m=None):
    from utils import y4m as container
    o = y4m_options(y4m)
    return container.header(int(width), int(height), o["fps"], o["aspect"], o["siting"], o["range"])


def truncate_y4m(out_dir, height, width, y4m=None):
    """Create `out_dir`/frames.y4m holding the stream header alone; returns the header's length.  ONE process of a sharded run does
    this before the others open the file (and before a barrier): the writers never truncate or write the header, they only write
    their frames' ranges."""
    os.makedirs(out_dir, exist_ok=True)
    head = y4m_header(height, width, y4m)
    with open(os.path.join(out_dir, Y4M_NAME), "wb") as fh:
        fh.write(head)
    return len(head)


class _EncodedFrame:
    """frame j of a downloaded group of device-encoded frames"""
    def __init__(self, group, j):
        self.group, self.j = group, j

    def file(self):
        from utils import png
        g, j = self.group, self.j
        sizes, streams = g.sizes[j].tolist(), g.streams[j].numpy()
        parts = [(s1, s2, rows * (1 + 3 * g.width)) for (s1, s2), rows in zip(g.adler[j].tolist(), png.chunk_rows(g.height, g.rows_per_chunk))]
        return png.assemble(g.height, g.width, [streams[c, :size].tobytes() for c, size in enumerate(sizes)], parts)


class _EncodedGroup:
    """what the workers read of a device-encoded group: host views of the slot's pinned bytes (sizes, Adler-32 parts, streams)"""
    def __init__(self, height, width, rows_per_chunk, sizes, adler, streams):
        self.height, self.width, self.rows_per_chunk = height, width, rows_per_chunk
        self.sizes, self.adler, self.streams = sizes, adler, streams

    def __getitem__(self, j):
        return _EncodedFrame(self, j)


def _encoded_views(flat, k, chunks, cap):
    """one flat uint8 buffer -> (sizes int32 [k, chunks], adler int32 [k, chunks, 2], streams uint8 [k, chunks, cap]) views of it"""
    a, b = 4 * k * chunks, 12 * k * chunks
    return (flat[:a].view(torch.int32).view(k, chunks), flat[a:b].view(torch.int32).view(k, chunks, 2),
            flat[b:b + k * chunks * cap].view(k, chunks, cap))


class _Slot:
    def __init__(self):
        self.buf = None             # pinned uint8 [capacity, H, W, 3] (device frames only)
        self.dev = None             # device encoder: flat device bytes (sizes, Adler-32 parts, streams of a group)
        self.enc = None             # device encoder: the pinned image of `dev`
        self.frames = None          # what the workers read: a view of buf, or the caller's host tensor
        self.event = None           # the download of `frames`
        self.pending = 0            # frames of this slot not yet written


class FrameWriter:
    def __init__(self, out_dir, fmt="png", depth=3, workers=4, n_frames=None, device=None, png_encoder="host", y4m=None):
        """workers: an explicit small number (capped at 16), never derived from the machine's CPU count.  n_frames: the length of
        the video, required for `raw` (the size of the file).  device: the GPU whose frames are submitted (default: the frames').
        png_encoder: "host" (PIL on the workers) or "device" (ct_hip.png_deflate; device tensors only, host tensors keep the PIL
        path); only `png` looks at it.  y4m: the stream's fps / aspect ("num:den") and the conversion's matrix / range / siting;
        only `y4m` takes it."""
        if fmt not in FORMATS:
            raise ValueError("format %r: one of %s" % (fmt, ", ".join(FORMATS)))
        if png_encoder not in PNG_ENCODERS:
            raise ValueError("png_encoder %r: one of %s" % (png_encoder, ", ".join(PNG_ENCODERS)))
        if int(depth) < 1 or int(workers) < 1:
            raise ValueError("depth and workers must be >= 1 (got %r, %r)" % (depth, workers))
        if fmt == "raw" and n_frames is None:
            raise ValueError("format raw needs n_frames (frame f lives at offset f*H*W*3 of one file)")
        if fmt == "y4m" and n_frames is None:
            raise ValueError("format y4m needs n_frames (frame f lives at header_len + f * (6 + frame_bytes) of one file)")
        if y4m is not None and fmt != "y4m":
            raise ValueError("the y4m options go with format y4m only (got format %r)" % fmt)
        self.y4m = y4m_options(y4m) if fmt == "y4m" else None
        self.out_dir, self.fmt, self.png_encoder = os.fspath(out_dir), fmt, png_encoder
        self.n_frames = None if n_frames is None else int(n_frames)
        self.device = None if device is None else torch.device(device)
        self._slots = [_Slot() for _ in range(int(depth))]
        self._next = 0
        self._cond = threading.Condition()
        self._error = None              # the first worker error, until it has been raised
        self._failed = False            # sticky: after an error nothing more is written
        self._frame_shape = None            # raw: the one [H, W, 3] of the file
        self._raw_fd = None
        self._dir_made = False
        self._copy_stream = None
        self._closed = False
        self._tasks = queue.Queue()
        self._threads = [threading.Thread(target=self._work, name="FrameWriter-%d" % i) for i in range(min(int(workers), MAX_WORKERS))]
        for t in self._threads:
            t.start()

    # ---- caller's side ---------------------------------------------------------------------------------------------------------
    def submit(self, indices, frames_u8, suffix=None):
        """Queue frames_u8[j] for writing as frame indices[j].  Returns the event of the download (None for host tensors): a device
        buffer handed in here may be overwritten by work that waits for it.  suffix: None, or a name that goes between the frame
        number and the extension (`%06d.<suffix>.png`); not with `raw`."""
        if self._closed:
            raise RuntimeError("FrameWriter is closed")
        self._raise_pending()
        indices = [int(i) for i in indices]
        if not isinstance(frames_u8, torch.Tensor) or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
            raise ValueError("frames must be a uint8 [k,H,W,3] tensor")
        if len(indices) != frames_u8.shape[0]:
            raise ValueError("%d frame indices for %d frames" % (len(indices), frames_u8.shape[0]))
        if any(i < 0 or (self.n_frames is not None and i >= self.n_frames) for i in indices):
            raise ValueError("frame index outside [0, %s)" % ("inf" if self.n_frames is None else self.n_frames))
        if suffix is not None:
            if not isinstance(suffix, str) or not suffix or any(ch in suffix for ch in "/\\.") or suffix != suffix.strip():
                raise ValueError("suffix %r: a plain name without dots or path separators" % (suffix,))
            if self.fmt in ("raw", "y4m"):
                raise ValueError("a %s video is one file: it takes no suffixed frames (suffix %r)" % (self.fmt, suffix))
        if self.fmt == "y4m" and not frames_u8.is_cuda:
            raise ValueError("format y4m converts on the device (ct_hip.rgb_to_yuv420): it takes device frames, not host tensors")
        if self.fmt in ("raw", "y4m"):
            shape = tuple(frames_u8.shape[1:])
            if self._frame_shape is None:
                self._frame_shape = shape
            elif shape != self._frame_shape:
                raise ValueError("%s video: frames of %s after frames of %s" % (self.fmt, shape, self._frame_shape))
        if not indices:
            return None
        slot = self._slots[self._next]
        self._next = (self._next + 1) % len(self._slots)
        with self._cond:                                    # back-pressure: the slot's previous frames are still being written
            while slot.pending:
                self._cond.wait()
        self._raise_pending()
        k = len(indices)
        if frames_u8.is_cuda and self.fmt == "png" and self.png_encoder == "device":
            self._submit_encoded(slot, frames_u8)
        elif self.fmt == "y4m":
            self._submit_y4m(slot, frames_u8)
        elif frames_u8.is_cuda:
            dev = frames_u8.device
            if slot.buf is None or slot.buf.shape[1:] != frames_u8.shape[1:] or slot.buf.shape[0] < k:
                slot.buf = torch.empty(tuple(frames_u8.shape), dtype=torch.uint8, pin_memory=True)
            if self._copy_stream is None:
                self._copy_stream = torch.cuda.Stream(device=self.device if self.device is not None else dev)
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream(dev))
            self._copy_stream.wait_event(ready)
            slot.frames = slot.buf[:k]
            with torch.cuda.stream(self._copy_stream):
                slot.frames.copy_(frames_u8, non_blocking=True)
                slot.event = torch.cuda.Event()
                slot.event.record(self._copy_stream)
            frames_u8.record_stream(self._copy_stream)
        else:
            slot.frames, slot.event = frames_u8, None
        slot.pending = k
        for j, index in enumerate(indices):
            self._tasks.put((slot, j, index, suffix))
        return slot.event

    def _submit_encoded(self, slot, frames_u8):
        """the device encoder: one png_deflate launch for the group on the caller's stream, then the slot's one copy"""
        import ct_hip
        dev = frames_u8.device
        k, h, w, _ = frames_u8.shape
        frames_u8 = frames_u8.contiguous()
        chunks, cap = ct_hip.png_geometry(h, w, ct_hip.PNG_ROWS_PER_CHUNK)
        need = k * chunks * (12 + cap)
        if slot.dev is None or slot.dev.numel() < need or slot.dev.device != dev:
            slot.dev = torch.empty(need, dtype=torch.uint8, device=dev)        # the old one is idle: the slot has nothing pending
            slot.enc = torch.empty(need, dtype=torch.uint8, pin_memory=True)
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(device=self.device if self.device is not None else dev)
        sizes, adler, streams = _encoded_views(slot.dev, k, chunks, cap)
        ct_hip.png_deflate(frames_u8, ct_hip.PNG_ROWS_PER_CHUNK, out=(streams, sizes, adler))
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(dev))
        self._copy_stream.wait_event(ready)
        with torch.cuda.stream(self._copy_stream):
            slot.enc[:need].copy_(slot.dev[:need], non_blocking=True)
            slot.event = torch.cuda.Event()
            slot.event.record(self._copy_stream)
        host_sizes, host_adler, host_streams = _encoded_views(slot.enc, k, chunks, cap)
        slot.frames = _EncodedGroup(h, w, ct_hip.PNG_ROWS_PER_CHUNK, host_sizes, host_adler, host_streams)

    def _submit_y4m(self, slot, frames_u8):
        """the YUV file: one rgb_to_yuv420 launch for the group on the caller's stream, then the slot's one copy of [k, frame_bytes]"""
        import ct_hip
        dev = frames_u8.device
        k, h, w, _ = frames_u8.shape
        fb = ct_hip.yuv420_frame_bytes(h, w)
        if slot.dev is None or slot.dev.numel() < k * fb or slot.dev.device != dev:
            slot.dev = torch.empty(k * fb, dtype=torch.uint8, device=dev)      # the old one is idle: the slot has nothing pending
            slot.enc = torch.empty(k * fb, dtype=torch.uint8, pin_memory=True)
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(device=self.device if self.device is not None else dev)
        planes = slot.dev[:k * fb].view(k, fb)
        ct_hip.rgb_to_yuv420(frames_u8.contiguous(), matrix=self.y4m["matrix"], range=self.y4m["range"], siting=self.y4m["siting"], out=planes)
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(dev))
        self._copy_stream.wait_event(ready)
        slot.frames = slot.enc[:k * fb].view(k, fb)
        with torch.cuda.stream(self._copy_stream):
            slot.frames.copy_(planes, non_blocking=True)
            slot.event = torch.cuda.Event()
            slot.event.record(self._copy_stream)
        frames_u8.record_stream(self._copy_stream)

    def close(self):
        """Drain the queue, join the workers, close the raw file, raise the first writer error.  Safe to call twice."""
        if not self._closed:
            self._closed = True
            for _ in self._threads:
                self._tasks.put(None)
            for t in self._threads:
                t.join()
            if self._raw_fd is not None:
                try:
                    if not self._failed and self._frame_shape is not None:
                        # every rank sets the same full size: frames nobody wrote read as zeros, a longer stale file is cut
                        os.ftruncate(self._raw_fd, self._file_bytes())
                except OSError as e:
                    self._failed, self._error = True, e
                finally:
                    os.close(self._raw_fd)
                    self._raw_fd = None
        self._raise_pending()

    def _file_bytes(self):
        """the full length of the one file of `raw` / `y4m`"""
        if self.fmt == "raw":
            return self.n_frames * int(np.prod(self._frame_shape))
        h, w = self._frame_shape[:2]
        return len(y4m_header(h, w, self.y4m)) + self.n_frames * (6 + h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2))

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:                                               # the caller's own exception wins; the threads are joined all the same
            try:
                self.close()
            except Exception:
                pass
        return False

    def _raise_pending(self):
        with self._cond:
            err, self._error = self._error, None
        if err is not None:
            raise err

    # ---- workers ---------------------------------------------------------------------------------------------------------------
    def _work(self):
        while True:
            task = self._tasks.get()
            if task is None:
                return
            slot, j, index, suffix = task
            try:
                if not self._failed:                              # after an error the queue is only drained
                    if slot.event is not None:
                        slot.event.synchronize()
                    self._write(index, slot.frames[j], suffix)
            except BaseException as e:                      # kept for the caller: never swallowed
                with self._cond:
                    if not self._failed:
                        self._failed, self._error = True, e
            finally:
                with self._cond:
                    slot.pending -= 1
                    if slot.pending == 0:
                        slot.frames = None
                        self._cond.notify_all()

    def _ensure_dir(self):
        if not self._dir_made:
            os.makedirs(self.out_dir, exist_ok=True)
            self._dir_made = True

    def _write(self, index, frame, suffix=None):
        if self.fmt == "null":
            return
        self._ensure_dir()
        if isinstance(frame, _EncodedFrame):
            with open(os.path.join(self.out_dir, frame_name(index, "png", suffix)), "wb") as fh:
                fh.write(frame.file())
            return
        arr = frame.numpy()
        if self.fmt == "png":
            from PIL import Image
            Image.fromarray(arr).save(os.path.join(self.out_dir, frame_name(index, "png", suffix)))
        elif self.fmt == "npy":
            np.save(os.path.join(self.out_dir, frame_name(index, "npy", suffix)), arr)
        else:
            with self._cond:
                if self._raw_fd is None:
                    self._raw_fd = os.open(os.path.join(self.out_dir, Y4M_NAME if self.fmt == "y4m" else RAW_NAME), os.O_WRONLY | os.O_CREAT, 0o666)
            data = memoryview(np.ascontiguousarray(arr)).cast("B")
            if self.fmt == "y4m":                           # `arr`: the frame's planes; its FRAME line goes in front of them
                h, w = self._frame_shape[:2]
                offset = len(y4m_header(h, w, self.y4m)) + index * (6 + len(data))
                done = 0
                while done < 6:
                    done += os.pwrite(self._raw_fd, b"FRAME\n"[done:], offset + done)
                offset += 6
            else:
                offset = index * len(data)
            done = 0
            while done < len(data):
                done += os.pwrite(self._raw_fd, data[done:], offset + done)
