"""Test-time data path of the reference (utils/data.py:12-22,87-125,168-179) for this stack.

* `setup_grid_distortions` -- the 31 deterministic distortions of `ArtificialTestDataset` (identity + brightness / contrast /
  saturation / hue / gamma at 6 magnitudes), as (name, parameter) pairs; they are APPLIED on the GPU (ct_distort_u8:
  torchvision's uint8 tensor arithmetic restated) to the uint8 ground-truth frame, index -> (image index // 31, distortion
  index % 31) exactly like the reference.
* `ArtificialTestDataset(image_dir)` / `RealWorldTestDataset(image_dir)` -- the reference's file layouts (`*_L.*`, `*_R.*`,
  `*/*_LD.*`); PNG decoding is on the host by default (PIL here, libpng behind torchvision.io.read_image there).
* `SyntheticArtificialTest` / `SyntheticStereoFrames` -- stand-ins when the Kaggle / MSU datasets are not on disk (they are not
  available offline): synthetic uint8 stereo pairs through the same 31 distortions, or a synthetic float video.
* `ArtificialTrainValDataset(image_dir, crop_size, image_repeats)` / `SyntheticTrainVal` -- the training / validation set
  (utils/data.py:25-84): `sample_params` draws the crop corner, the two flips, the order and the strengths of the six adjustments on
  the host, in the reference's order from the reference's generators; ct_augment_u8 applies them, a whole batch per call
  (`BatchLoader`, `DataModule.val_dataloader()`).
* `png_decoder="device"` on the file datasets and `DataModule`: `host_frames` hands over each file's zlib payload instead of its
  pixels (files that ct_hip.png_decode does not take are decoded by PIL as before) and `finish` decodes on the GPU;
  `prefetch_decoded(dataset, indices, device, ahead)` reads `ahead` samples' files, uploads them in one copy and decodes all their
  streams in ONE call (a stream occupies one wave: a call needs many to fill the GPU).
* `prefetch(dataset, indices, device)` -- yields device-resident samples while the next one is decoded into PINNED host
  memory and uploaded on a second stream (double buffer), so that the transfer kernels never wait for PCIe.
* `StereoY4MVideo(target, reference, gt=None)` / `SyntheticStereoVideoYUV` -- stereo video as 8-bit Y'CbCr 4:2:0: Y4M files (utils/y4m.py,
  the stand-in for the reference's cv2.VideoCapture) or synthetic I420 chunks.  `prefetch_groups` uploads the YUV bytes (1.5 per pixel
  instead of 3) and decodes a whole chunk with ONE ct_hip.yuv420_to_rgb launch into the [3,k,H,W,3] RGB groups every grouped method takes.
Seeds are derived from the FRAME index (world-size independent)."""
import os
from pathlib import Path

import numpy as np
import torch

from utils.sharding import frame_seed


def setup_grid_distortions(max_magnitude=0.5, num=6):
    """utils/data.py:12-22: identity, then per magnitude in linspace(-m, m, num): brightness, contrast, saturation (factor
    1 + magnitude), hue (factor = magnitude), gamma (1 + magnitude)."""
    specs = [("identity", 0.0)]
    for magnitude in np.linspace(-max_magnitude, max_magnitude, num):
        specs += [("brightness", 1 + magnitude), ("contrast", 1 + magnitude), ("saturation", 1 + magnitude),
                  ("hue", magnitude), ("gamma", 1 + magnitude)]
    return specs


def read_image(path):
    """uint8 [3,H,W] like torchvision.io.read_image (RGB)"""
    from PIL import Image
    with Image.open(path) as im:
        arr = np.asarray(im.convert("RGB"))
    return torch.from_numpy(np.ascontiguousarray(arr.transpose(2, 0, 1)))


PNG_DECODERS = ("host", "device")


def check_png_decoder(value):
    if value not in PNG_DECODERS:
        raise ValueError("png_decoder %r: one of %s" % (value, ", ".join(PNG_DECODERS)))
    return value


class Encoded:
    """what `host_frames` hands over with png_decoder="device": the dataset's own extra and, per frame that is still a zlib
    payload (a 1-D uint8 tensor), its (height, width); frames that PIL decoded are uint8 [3,H,W] and have no entry"""

    def __init__(self, extra, dims):
        self.extra, self.dims = extra, dims


def read_encoded(path):
    """(the file's zlib payload as a 1-D uint8 tensor, (height, width)) where ct_hip.png_decode takes the file -- 8-bit RGB, no
    interlace, a sound container -- and otherwise (read_image(path), None): PIL decodes it, or raises what it raises today"""
    from utils import png
    from ct_hip.png import PNG_MAX_WIDTH
    with open(path, "rb") as fh:
        data = fh.read()
    try:
        info = png.parse(data)
    except ValueError:
        info = None
    if info is None or not png.device_decodable(info) or info.width > PNG_MAX_WIDTH or info.height * (1 + 3 * info.width) > 0x7fffffff:
        return read_image(path), None
    return torch.frombuffer(bytearray(info.payload), dtype=torch.uint8), (info.height, info.width)


def read_frames(paths, extra, png_decoder):
    """{name: path} -> (host dict, extra) as `host_frames` returns them, for either decoder"""
    if png_decoder != "device":
        return {k: read_image(str(p)) for k, p in paths.items()}, extra
    host, dims = {}, {}
    for k, p in paths.items():
        host[k], d = read_encoded(str(p))
        if d is not None:
            dims[k] = d
    return host, Encoded(extra, dims)


def decode_samples(samples):
    """[(device dict, extra)] -> the same with every zlib payload decoded to uint8 [3,H,W] and the dataset's own extra back in
    place: ONE ct_hip.png_decode call for all of them.  Samples of a host-decoder dataset pass through."""
    todo = [(n, k) for n, (dev, extra) in enumerate(samples) if isinstance(extra, Encoded) for k in sorted(extra.dims)]
    frames = []
    if todo:
        import ct_hip
        frames = ct_hip.png_decode([(samples[n][0][k],) + tuple(samples[n][1].dims[k]) for n, k in todo])
    out = [(dict(dev), extra.extra if isinstance(extra, Encoded) else extra) for dev, extra in samples]
    for (n, k), frame in zip(todo, frames):
        out[n][0][k] = frame
    return out


class _Distorted:
    """common part of the artificial test sets: sample index -> (image, distortion); uint8 host frames in, device floats out"""

    def __init__(self):
        self.distortions = setup_grid_distortions()

    def __len__(self):
        return self.n_images() * len(self.distortions)

    def host_frames(self, index):
        """uint8 CHW (gt, reference) of sample `index` on the host + the distortion to apply to gt"""
        gt, reference = self.load_pair(index // len(self.distortions))
        return {"gt": gt, "reference": reference}, self.distortions[index % len(self.distortions)]

    @staticmethod
    def finish(dev_u8, distortion):
        """device uint8 frames -> the reference's sample dict (utils/data.py:125): gt / 255, reference / 255, target / 255"""
        import ct_hip
        (dev_u8, distortion), = decode_samples([(dev_u8, distortion)])
        out = {k: ct_hip.distort_u8(v.contiguous(), "identity", 0.0) for k, v in dev_u8.items()}      # x / 255 in float32
        out["target"] = ct_hip.distort_u8(dev_u8["gt"].contiguous(), distortion[0], distortion[1])
        return out

    def __getitem__(self, index):
        host, d = self.host_frames(index)
        return self.finish({k: v.cuda() for k, v in host.items()}, d)


class ArtificialTestDataset(_Distorted):                      # utils/data.py:107-125
    def __init__(self, image_dir, png_decoder="host"):
        super().__init__()
        self.png_decoder = check_png_decoder(png_decoder)
        image_dir = Path(image_dir)
        self.gts = sorted(image_dir.glob("*_L.*"))
        self.references = sorted(image_dir.glob("*_R.*"))
        assert len(self.gts) == len(self.references)

    def n_images(self):
        return len(self.gts)

    def load_pair(self, i):
        return read_image(str(self.gts[i])), read_image(str(self.references[i]))

    def host_frames(self, index):
        if self.png_decoder != "device":
            return super().host_frames(index)
        i, d = divmod(index, len(self.distortions))
        return read_frames({"gt": self.gts[i], "reference": self.references[i]}, self.distortions[d], self.png_decoder)


class SyntheticArtificialTest(_Distorted):
    """synthetic uint8 stereo pairs (a textured left view and a shifted right view) through the 31 test distortions"""

    def __init__(self, n_images=2, height=270, width=480):
        super().__init__()
        self._n, self.height, self.width = int(n_images), int(height), int(width)
        self._cache = {}

    def n_images(self):
        return self._n

    def load_pair(self, i):
        if i not in self._cache:
            rng = np.random.default_rng(frame_seed(i))
            coarse = rng.integers(0, 256, (3, self.height // 16 + 2, self.width // 16 + 2)).astype(np.float32)
            up = torch.nn.functional.interpolate(torch.from_numpy(coarse)[None], size=(self.height, self.width + 16), mode="bilinear",
                                                 align_corners=True)[0]
            up = (up + torch.from_numpy(rng.integers(-12, 13, up.shape).astype(np.float32))).clamp(0, 255).to(torch.uint8)
            self._cache = {i: (up[:, :, :self.width].contiguous(), up[:, :, 16:].contiguous())}        # keep one pair
        return self._cache[i]


class RealWorldTestDataset:                                   # utils/data.py:128-145
    def __init__(self, image_dir, png_decoder="host"):
        self.png_decoder = check_png_decoder(png_decoder)
        image_dir = Path(image_dir)
        self.gts = sorted(image_dir.glob("*/*_L.*"))
        self.targets = sorted(image_dir.glob("*/*_LD.*"))
        self.references = sorted(image_dir.glob("*/*_R.*"))
        assert len(self.gts) == len(self.targets) == len(self.references)

    def __len__(self):
        return len(self.gts)

    def host_frames(self, index):
        return read_frames({"gt": self.gts[index], "reference": self.references[index], "target": self.targets[index]}, None, self.png_decoder)

    @staticmethod
    def finish(dev_u8, extra):
        import ct_hip
        (dev_u8, _), = decode_samples([(dev_u8, extra)])
        return {k: ct_hip.distort_u8(v.contiguous(), "identity", 0.0) for k, v in dev_u8.items()}

    def __getitem__(self, index):
        host, extra = self.host_frames(index)
        return self.finish({k: v.cuda() for k, v in host.items()}, extra)


class _TrainVal:
    """common part of the training / validation sets (utils/data.py:52-84): sample index -> image index // image_repeats, a random
    crop, the two flips and a random chain of the six adjustments, all drawn on the host and APPLIED on the GPU (ct_augment_u8)"""
    # apply_uniform_distortions' fn_id -> the operation (utils/data.py:35-47)
    OPS = ("brightness", "contrast", "saturation", "hue", "gamma", "sharpness")

    def __init__(self, crop_size, image_repeats):
        self.crop_size = (int(crop_size[-2]), int(crop_size[-1]))
        self.image_repeats = int(image_repeats)

    def __len__(self):
        return self.n_images() * self.image_repeats

    def sample_params(self, index, max_magnitude=0.5):
        """The random draws of sample `index`, in the reference's order from the reference's generators (utils/data.py:69-80,
        26-33): numpy's global generator for the corner (top, then left; a source no larger than the crop raises numpy's own
        ValueError), the two flips and the six strengths (brightness, contrast, saturation, hue, gamma, sharpness), torch's
        global generator for the order in between.  Seeding both reproduces the reference's samples in a single process."""
        height, width = self.source_size(index // self.image_repeats)
        top = np.random.randint(0, height - self.crop_size[0])
        left = np.random.randint(0, width - self.crop_size[1])
        swap_hflip = np.random.random() > 0.5
        vflip = np.random.random() > 0.5
        order = torch.randperm(6).tolist()
        lo, hi = 1 - max_magnitude, 1 + max_magnitude
        strength = [np.random.uniform(lo, hi), np.random.uniform(lo, hi), np.random.uniform(lo, hi),
                    np.random.uniform(-max_magnitude, max_magnitude), np.random.uniform(lo, hi), np.random.uniform(lo, hi)]
        return {"top": int(top), "left": int(left), "swap_hflip": bool(swap_hflip), "vflip": bool(vflip),
                "ops": [(self.OPS[i], float(strength[i])) for i in order]}

    def host_frames(self, index):
        """uint8 CHW (gt, reference) of sample `index` on the host + its draws"""
        gt, reference = self.load_pair(index // self.image_repeats)
        return {"gt": gt, "reference": reference}, self.sample_params(index)

    def finish(self, dev_u8, params):
        """device uint8 frames [3,H,W] (one sample, params a dict) or [n,3,H,W] (a batch, params a list) -> the reference's sample
        dict (utils/data.py:84) of that shape: ONE ct_hip.augment_u8 call either way"""
        import ct_hip
        if isinstance(params, Encoded):
            (dev_u8, params), = decode_samples([(dev_u8, params)])
        single = isinstance(params, dict)
        gt, reference = dev_u8["gt"], dev_u8["reference"]
        out = ct_hip.augment_u8((gt[None] if single else gt).contiguous(), (reference[None] if single else reference).contiguous(),
                                [params] if single else params, self.crop_size)
        return {k: v[0] for k, v in out.items()} if single else out

    def __getitem__(self, index):
        host, params = self.host_frames(index)
        return self.finish({k: v.cuda() for k, v in host.items()}, params)


class ArtificialTrainValDataset(_TrainVal):                   # utils/data.py:52-84
    def __init__(self, image_dir, crop_size, image_repeats, png_decoder="host"):
        super().__init__(crop_size, image_repeats)
        self.png_decoder = check_png_decoder(png_decoder)
        image_dir = Path(image_dir)
        self.gts = sorted(image_dir.glob("*_L.*"))
        self.references = sorted(image_dir.glob("*_R.*"))
        assert len(self.gts) == len(self.references)

    def n_images(self):
        return len(self.gts)

    def source_size(self, i):
        from PIL import Image
        with Image.open(str(self.gts[i])) as im:              # the header only
            return im.height, im.width

    def load_pair(self, i):
        return read_image(str(self.gts[i])), read_image(str(self.references[i]))

    def host_frames(self, index):
        if self.png_decoder != "device":
            return super().host_frames(index)
        i = index // self.image_repeats
        return read_frames({"gt": self.gts[i], "reference": self.references[i]}, self.sample_params(index), self.png_decoder)


class SyntheticTrainVal(_TrainVal):
    """SyntheticArtificialTest's uint8 stereo pairs through the training / validation augmentation, for offline runs"""

    def __init__(self, n_images=2, height=270, width=480, crop_size=(256, 448), image_repeats=1):
        super().__init__(crop_size, image_repeats)
        self._pairs = SyntheticArtificialTest(n_images, height, width)

    def n_images(self):
        return self._pairs.n_images()

    def source_size(self, i):
        return self._pairs.height, self._pairs.width

    def load_pair(self, i):
        return self._pairs.load_pair(i)


class BatchLoader:
    """What `validate` iterates: the samples of `dataset` in batches of `batch_size` consecutive samples of the caller's index list.
    batches(indices, device) yields (the batch's sample indices, {target, reference, gt}: float32 [B,3,h,w] on the device).  A
    training / validation set is batched BEFORE the GPU work: the uint8 sources are stacked and one ct_hip.augment_u8 call makes
    the batch (its sources must have one size); any other dataset yields its samples one by one through `prefetch`.  With
    png_decoder="device" the files of a whole batch are decoded by one ct_hip.png_decode call (`prefetch_decoded` for the others)."""

    def __init__(self, dataset, batch_size=1, name="loader", decode_ahead=16):
        self.dataset, self.batch_size, self.name, self.decode_ahead = dataset, max(int(batch_size or 1), 1), name, decode_ahead

    def __len__(self):
        return len(self.dataset)

    def batches(self, indices, device):
        indices = list(indices)
        on_device = getattr(self.dataset, "png_decoder", "host") == "device"
        if not isinstance(self.dataset, _TrainVal):
            samples = prefetch_decoded(self.dataset, indices, device, self.decode_ahead) if on_device else prefetch(self.dataset, indices, device)
            for index, sample in samples:
                yield [index], {k: v.unsqueeze(0) for k, v in sample.items()}
            return
        for c in range(0, len(indices), self.batch_size):
            ids = indices[c:c + self.batch_size]
            hosts, params = zip(*(self.dataset.host_frames(i) for i in ids))
            if on_device:                                       # the batch's files: one upload, one decode
                decoded = decode_samples(upload_samples(list(zip(hosts, params)), device))
                if len({d["gt"].shape for d, _ in decoded}) > 1:
                    raise ValueError("a batch is made by one augment_u8 call: its source pairs need one size (got %s)"
                                     % sorted({tuple(d["gt"].shape) for d, _ in decoded}))
                dev = {k: torch.stack([d[k] for d, _ in decoded]) for k in ("gt", "reference")}
                yield ids, self.dataset.finish(dev, [p for _, p in decoded])
                continue
            if len({h["gt"].shape for h in hosts}) > 1:
                raise ValueError("a batch is made by one augment_u8 call: its source pairs need one size (got %s)"
                                 % sorted({tuple(h["gt"].shape) for h in hosts}))
            dev = {k: torch.stack([h[k] for h in hosts]).to(device) for k in ("gt", "reference")}
            yield ids, self.dataset.finish(dev, list(params))


class SyntheticStereoFrames:
    """a synthetic float video: dict(target, reference, gt) of float32 [3,H,W] in [0,1]; the distortion is a fixed
    gain / gamma / hue-like matrix so that PSNR is meaningful"""

    def __init__(self, n_frames=8, height=270, width=480):
        self.n_frames, self.height, self.width = int(n_frames), int(height), int(width)

    def __len__(self):
        return self.n_frames

    def __getitem__(self, f):
        rng = np.random.default_rng(frame_seed(f))
        yy, xx = np.mgrid[0:self.height, 0:self.width].astype(np.float32)
        base = np.stack([0.5 + 0.4 * np.sin(xx / self.width * 6.0 + f * 0.1) * np.cos(yy / self.height * 4.0),
                         0.2 + 0.6 * xx / self.width, 0.5 + 0.4 * np.cos((xx + yy) / (self.width + self.height) * 9.0)])
        gt = np.clip(base + 0.05 * rng.standard_normal(base.shape).astype(np.float32), 0, 1).astype(np.float32)
        reference = np.clip(np.roll(gt, 7, axis=2) + 0.02 * rng.standard_normal(base.shape).astype(np.float32), 0, 1)
        mix = np.array([[0.9, 0.08, 0.0], [0.05, 0.8, 0.05], [0.0, 0.1, 1.05]], dtype=np.float32)
        target = np.clip(np.einsum("ij,jhw->ihw", mix, gt) ** 1.15 + 0.03, 0, 1).astype(np.float32)
        return {"target": torch.from_numpy(target), "reference": torch.from_numpy(reference.astype(np.float32)),
                "gt": torch.from_numpy(gt)}


def prefetch(dataset, indices, device):
    """Yield (index, sample) with every tensor of `sample` resident on `device` as [3,H,W] float32.  Datasets with
    `host_frames` (uint8 files / synthetic uint8) go through two pinned staging buffers and a copy stream: while the caller
    works on sample i, sample i+1 is decoded on the host and uploaded; the uint8 -> float conversion and the distortion run
    on the GPU.  Other datasets (host float tensors) are uploaded the same way, converted nowhere."""
    indices = list(indices)
    if not indices:
        return
    if torch.device(device).type == "cpu":          # utils.cli's CT_CLI_DEVICE=cpu test mode: host float datasets as they are
        for index in indices:
            yield index, dataset[index]
        return
    copy_stream = torch.cuda.Stream(device=device)
    staged = [None, None]
    pinned = [{}, {}]
    slot_done = [None, None]                        # event of the last upload issued from each slot's pinned buffers

    def stage(slot, index):
        if hasattr(dataset, "host_frames"):
            host, extra = dataset.host_frames(index)
        else:
            host, extra = dataset[index], "float"
        dev = {}
        # the pinned buffers of this slot are the SOURCE of the asynchronous copy issued two samples ago: the host must not
        # refill them before that DMA has finished (the consumer stream waits on the event, the host so far did not)
        if slot_done[slot] is not None:
            slot_done[slot].synchronize()
        with torch.cuda.stream(copy_stream):
            for k, v in host.items():
                buf = pinned[slot].get(k)
                if buf is None or buf.shape != v.shape or buf.dtype != v.dtype:
                    buf = pinned[slot][k] = torch.empty(v.shape, dtype=v.dtype).pin_memory()
                buf.copy_(v)
                dev[k] = buf.to(device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(copy_stream)
        slot_done[slot] = ev
        staged[slot] = (index, dev, extra, ev)

    stage(0, indices[0])
    for n, _ in enumerate(indices):
        slot = n & 1
        if n + 1 < len(indices):
            stage(slot ^ 1, indices[n + 1])          # decode + upload the next sample while this one is processed
        index, dev, extra, ev = staged[slot]
        torch.cuda.current_stream(device).wait_event(ev)
        for v in dev.values():
            v.record_stream(torch.cuda.current_stream(device))
        yield index, (dev if extra == "float" else dataset.finish(dev, extra))


def upload_samples(samples, device):
    """[(host dict of uint8 tensors, extra)] -> the same on `device`: every tensor of every sample through ONE pinned buffer and
    one copy on the current stream (the pinned block is not reused before the copy has been made: torch's host allocator)"""
    tensors = [v for host, _ in samples for v in host.values()]
    total = sum(t.numel() for t in tensors)
    pinned = torch.empty(max(total, 1), dtype=torch.uint8).pin_memory()
    at = 0
    for t in tensors:
        pinned[at:at + t.numel()] = t.reshape(-1)
        at += t.numel()
    dev_all = pinned.to(device, non_blocking=True)
    out, at = [], 0
    for host, extra in samples:
        dev = {}
        for k, v in host.items():
            dev[k] = dev_all[at:at + v.numel()].view(v.shape)
            at += v.numel()
        out.append((dev, extra))
    return out


def prefetch_decoded(dataset, indices, device, ahead=16):
    """Yield (index, sample) like `prefetch`, for a dataset with png_decoder="device": the files of `ahead` samples are read and
    parsed on the host, uploaded in one copy, ALL their zlib streams decoded by one ct_hip.png_decode call (one wave per stream: three
    streams would use 3 of some 2000 wave slots), and the samples yielded one by one through `finish`.  A dataset with the host
    decoder takes the same route with nothing left to decode."""
    indices = list(indices)
    ahead = max(int(ahead), 1)
    if torch.device(device).type == "cpu":
        raise ValueError("prefetch_decoded decodes on the GPU: there is no CPU path")
    for c in range(0, len(indices), ahead):
        ids = indices[c:c + ahead]
        decoded = decode_samples(upload_samples([dataset.host_frames(i) for i in ids], device))
        for index, (dev, extra) in zip(ids, decoded):
            yield index, dataset.finish(dev, extra)


class SyntheticStereoVideoU8:
    """BASELINE.json configs[4]: a synthetic 1080p stereo video of uint8 frames -- what every real frame is (the reference's
    datasets decode to uint8 and divide by 255, utils/data.py:84,106,125) -- handed over as PINNED HOST chunks of `group`
    consecutive frames per rank (default 8), [3 roles: target, reference, gt][group][H][W][3].  Decoding / generating 1000 distinct frames on
    the host would measure the host, so the frames cycle through a pool of `pool` distinct chunks (seeded 4321 + i)."""
    roles = ("target", "reference", "gt")

    def __init__(self, n_frames=1000, height=1080, width=1920, group=8, pool=8):
        self.n_frames, self.height, self.width, self.group, self.pool = int(n_frames), int(height), int(width), int(group), int(pool)
        self._chunks = None

    def __len__(self):
        return self.n_frames

    def _chunk(self, i):
        """pinned chunk i of the pool, generated on first use (a run that touches two chunks pins two: 149 MB each at 1080p)"""
        if self._chunks is None:
            self._chunks = [None] * self.pool
        if self._chunks[i] is None:
            rng = np.random.default_rng(4321 + i)
            trip = rng.integers(0, 256, (3, self.group, self.height, self.width, 3), dtype=np.uint8)
            t = torch.from_numpy(trip)
            self._chunks[i] = t.pin_memory() if torch.cuda.is_available() else t
        return self._chunks[i]

    def _pool_index(self, first_frame):
        """which pool chunk a group that starts at `first_frame` takes: a multiplicative hash of the frame index, so that the pool
        cycles whatever the stride between a rank's groups is (round 5 indexed by first_frame % pool: with group = pool = 8 every
        group of a rank got the same chunk) -- a function of the frame index only, not of rank or world size"""
        return ((int(first_frame) * 2654435761) >> 9) % self.pool

    def prepare(self, indices):
        """generate (and pin) every pool chunk the groups of `indices` will take -- a caller that times its loop does this first:
        generating frames on the host would measure the host (class docstring)"""
        idx = list(indices)
        for c in range(0, len(idx), self.group):
            self._chunk(self._pool_index(idx[c]))

    def host_chunk(self, first_frame):
        """the pinned chunk of the group of frames that starts at `first_frame`.  Synthetic data: a group's CONTENT is defined by its
        first frame (chunk _pool_index(first_frame), slots 0..group-1 in order), so per-frame tables depend on how frames are
        grouped (group size, world size); throughput does not."""
        return self._chunk(self._pool_index(first_frame))

    def __getitem__(self, f):
        """one frame as the reference's sample dict (float32 CHW in [0,1]): the per-sample path of utils.cli = a group of one
        (slot 0 of the chunk host_chunk(f) would hand over)"""
        c = self.host_chunk(f)[:, 0]
        return {k: (c[i].permute(2, 0, 1).float() / 255) for i, k in enumerate(self.roles)}


YUV_ROLES = ("target", "reference", "gt")


class _YuvGroups:
    """what the two YUV datasets share: the geometry, the decode of an uploaded chunk and the per-frame sample"""

    def _init_yuv(self, height, width, group, matrix, range_, siting, n_roles):
        import ct_hip
        if matrix not in ct_hip.YUV_MATRICES or range_ not in ct_hip.YUV_RANGES or siting not in ct_hip.YUV_SITINGS:
            raise ValueError("yuv_matrix %r / yuv_range %r / siting %r: one of %s / %s / %s"
                             % (matrix, range_, siting, sorted(ct_hip.YUV_MATRICES), sorted(ct_hip.YUV_RANGES), sorted(ct_hip.YUV_SITINGS)))
        if int(group) < 1:
            raise ValueError("group must be >= 1 (got %r)" % (group,))
        self.height, self.width, self.group = int(height), int(width), int(group)
        self.matrix, self.range, self.siting = matrix, range_, siting
        self.frame_bytes = ct_hip.yuv420_frame_bytes(self.height, self.width)
        self.roles = YUV_ROLES[:n_roles]
        self.has_gt = n_roles == 3
        self.upload_bytes_per_frame = n_roles * self.frame_bytes        # what one frame of every role costs on the host link

    def decode_group(self, dev, k, out):
        """dev: the uploaded chunk, device uint8 [roles][group][frame_bytes], its first k frames per role valid; out: device uint8
        [roles][group][H][W][3].  A full chunk is ONE ct_hip.yuv420_to_rgb launch over roles * group frames, a ragged one a launch
        per role.  Returns out[:, :k]."""
        import ct_hip
        roles, g = dev.shape[0], dev.shape[1]
        kw = dict(matrix=self.matrix, range=self.range, siting=self.siting)
        if k == g:
            ct_hip.yuv420_to_rgb(dev.view(roles * g, self.frame_bytes), self.height, self.width, out=out.view(roles * g, self.height, self.width, 3), **kw)
        else:
            for r in range(roles):
                ct_hip.yuv420_to_rgb(dev[r, :k], self.height, self.width, out=out[r, :k], **kw)
        return out[:, :k]

    def __getitem__(self, f):
        """one frame as the reference's sample dict (float32 CHW in [0,1], on the device): float32(byte) / 255 of the same
        kernel's bytes.  Without a gt stream the gt role is the target's frame."""
        if not torch.cuda.is_available():
            raise RuntimeError("%s decodes on the GPU (ct_hip.yuv420_to_rgb): there is no CPU path" % type(self).__name__)
        f = int(f)
        if not 0 <= f < len(self):
            raise IndexError(f)
        device = torch.device("cuda", torch.cuda.current_device())
        dev = self.stage_chunk([f], None)[:, :1].to(device).contiguous()       # a blocking copy: the pinned buffer is reused by the next call
        rgb = torch.empty((dev.shape[0], 1, self.height, self.width, 3), dtype=torch.uint8, device=device)
        self.decode_group(dev, 1, rgb)
        # float32(byte) / 255 correctly rounded, from a host-made table (a device division need not round like the host's)
        table = (torch.arange(256, dtype=torch.float32) / 255).to(device)
        chw = table[rgb[:, 0].permute(0, 3, 1, 2).long()]
        sample = {k: chw[i] for i, k in enumerate(self.roles)}
        sample.setdefault("gt", sample["target"])
        return sample


class StereoY4MVideo(_YuvGroups):
    """Stereo video from Y4M files (utils/y4m.py): the distorted view `target`, the other view `reference` and, for `test`, the
    ground truth `gt`, 8-bit 4:2:0 progressive, of one size, siting and range; the length is the shortest file's.  Frames travel
    as YUV: `stage_chunk` preads the frames of a group straight into a pinned [roles][group][frame_bytes] buffer, `prefetch_groups`
    uploads it and `decode_group` makes the RGB group on the device.  range: None follows the files' XCOLORRANGE, else "limited".
    Without gt, `predict` works (two roles are uploaded) and `test` is refused."""

    def __init__(self, target, reference, gt=None, group=8, matrix="bt709", range=None):
        from utils import y4m
        paths = [os.fspath(p) for p in (target, reference) + ((gt,) if gt else ())]
        parsed = [y4m.frame_offsets(p) for p in paths]
        heads = [h for h, _ in parsed]
        for p, h in zip(paths[1:], heads[1:]):
            if (h.width, h.height) != (heads[0].width, heads[0].height):
                raise ValueError("%s is %d x %d, %s is %d x %d: the streams must agree in size"
                                 % (paths[0], heads[0].width, heads[0].height, p, h.width, h.height))
            if h.siting != heads[0].siting or h.color_range != heads[0].color_range:
                raise ValueError("%s and %s differ in chroma siting or XCOLORRANGE: one decode serves a whole group" % (paths[0], p))
        self.header = heads[0]
        self.paths = paths
        self._offsets = [o for _, o in parsed]
        self.n_frames = min(len(o) for o in self._offsets)
        self._init_yuv(heads[0].height, heads[0].width, group, matrix, range or heads[0].color_range or "limited", heads[0].siting,
                       len(paths))
        self._fds = [os.open(p, os.O_RDONLY) for p in paths]
        self._pinned = {}

    def __len__(self):
        return self.n_frames

    def close(self):
        for fd in self._fds:
            os.close(fd)
        self._fds = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stage_chunk(self, ids, slot):
        """the frames `ids` (at most `group`) of every role, read into the pinned buffer of `slot` ([roles][group][frame_bytes];
        the caller keeps a slot's previous upload from being overwritten) and returned"""
        buf = self._pinned.get(slot)
        if buf is None:
            buf = torch.empty((len(self.roles), self.group, self.frame_bytes), dtype=torch.uint8)
            buf = self._pinned[slot] = buf.pin_memory() if torch.cuda.is_available() else buf
        arr = buf.numpy()
        for r, (fd, offsets) in enumerate(zip(self._fds, self._offsets)):
            for j, f in enumerate(ids):
                view, done = memoryview(arr[r, j]), 0
                while done < self.frame_bytes:
                    got = os.preadv(fd, [view[done:]], offsets[f] + done)
                    if got <= 0:
                        raise IOError("%s: frame %d ends early" % (self.paths[r], f))
                    done += got
        return buf

    def host_chunk(self, first_frame):
        """the pinned chunk of the `group` consecutive frames from `first_frame` (fewer at the end of the video), as YUV bytes"""
        first_frame = int(first_frame)
        return self.stage_chunk(range(first_frame, min(first_frame + self.group, self.n_frames)), "host_chunk")


class SyntheticStereoVideoYUV(_YuvGroups):
    """`--data.synthetic video_yuv`: SyntheticStereoVideoU8's pinned-pool scheme with packed I420 chunks,
    [3 roles][group][frame_bytes] of random bytes: the same frames-per-second question at 1.5 bytes per pixel on the link, with no
    disk in the measurement."""

    def __init__(self, n_frames=1000, height=1080, width=1920, group=8, pool=8, matrix="bt709", range="limited", siting="center"):
        self.n_frames, self.pool = int(n_frames), int(pool)
        self._init_yuv(height, width, group, matrix, range or "limited", siting, 3)
        self._chunks = None

    def __len__(self):
        return self.n_frames

    def _chunk(self, i):
        if self._chunks is None:
            self._chunks = [None] * self.pool
        if self._chunks[i] is None:
            rng = np.random.default_rng(8765 + i)
            t = torch.from_numpy(rng.integers(0, 256, (3, self.group, self.frame_bytes), dtype=np.uint8))
            self._chunks[i] = t.pin_memory() if torch.cuda.is_available() else t
        return self._chunks[i]

    _pool_index = SyntheticStereoVideoU8._pool_index

    def prepare(self, indices):
        idx = list(indices)
        for c in range(0, len(idx), self.group):
            self._chunk(self._pool_index(idx[c]))

    def host_chunk(self, first_frame):
        """as SyntheticStereoVideoU8.host_chunk: a group's content is defined by its first frame"""
        return self._chunk(self._pool_index(first_frame))

    def stage_chunk(self, ids, slot):
        return self.host_chunk(list(ids)[0])


def _prefetch_yuv_groups(dataset, indices, device, depth=3):
    """prefetch_groups for a dataset of YUV chunks (`stage_chunk`, `decode_group`): the same copy stream and ring of `depth` device
    buffers, of [roles][group][frame_bytes] YUV bytes; after a chunk's upload event the consumer's stream runs the dataset's decode
    (one launch for a full chunk) into a ring of RGB buffers of its own and the [roles,k,H,W,3] RGB group is yielded.  The YUV
    buffer is free again once that decode has run, the RGB buffer when the consumer's stream reaches its next use."""
    indices = list(indices)
    g = dataset.group
    n_chunks = (len(indices) + g - 1) // g
    if n_chunks == 0:
        return
    copy_stream = torch.cuda.Stream(device=device)
    main = torch.cuda.current_stream(device)
    roles, fb = len(dataset.roles), dataset.frame_bytes
    ring = [torch.empty((roles, g, fb), dtype=torch.uint8, device=device) for _ in range(depth)]
    rgb = [torch.empty((roles, g, dataset.height, dataset.width, 3), dtype=torch.uint8, device=device) for _ in range(depth)]
    uploaded = [torch.cuda.Event() for _ in range(depth)]
    consumed = [torch.cuda.Event() for _ in range(depth)]

    def ids_of(c):
        return indices[c * g:c * g + g]

    def upload(c):
        slot, ids = c % depth, ids_of(c)
        if c >= depth:
            uploaded[slot].synchronize()            # host: the pinned buffer of this slot is the source of that earlier copy
        src = dataset.stage_chunk(ids, slot)
        with torch.cuda.stream(copy_stream):
            if c >= depth:
                copy_stream.wait_event(consumed[slot])
            if len(ids) == g:
                ring[slot].copy_(src, non_blocking=True)
            else:
                ring[slot][:, :len(ids)].copy_(src[:, :len(ids)], non_blocking=True)
            uploaded[slot].record(copy_stream)

    for c in range(min(depth - 1, n_chunks)):
        upload(c)
    for c in range(n_chunks):
        if c + depth - 1 < n_chunks:
            upload(c + depth - 1)
        slot, ids = c % depth, ids_of(c)
        main.wait_event(uploaded[slot])
        frames = dataset.decode_group(ring[slot], len(ids), rgb[slot])
        consumed[slot].record(main)
        yield ids, frames


def prefetch_groups(dataset, indices, device, depth=3):
    """Yield (frame indices of the group, device uint8 tensor [3, k, H, W, 3]) for a dataset with `host_chunk` (pinned uint8 chunks
    of `dataset.group` frames): the uploads run on a copy stream, depth - 1 uploads ahead of the consumer, through a ring of
    `depth` device buffers; a buffer is overwritten only after the kernels that read its previous chunk are done (the consumer's
    stream is the current one when the generator is advanced).  Copy size is what the PCIe rate hangs on (measured round 5,
    1080p triples, same box): one triple per copy 47.8 GB/s, four (75 MB) 49-52, eight (149 MB, the default group) 56."""
    if hasattr(dataset, "decode_group"):            # YUV chunks (StereoY4MVideo, SyntheticStereoVideoYUV): decoded on the device
        yield from _prefetch_yuv_groups(dataset, indices, device, depth)
        return
    indices = list(indices)
    g = dataset.group
    n_chunks = (len(indices) + g - 1) // g
    if n_chunks == 0:
        return
    copy_stream = torch.cuda.Stream(device=device)
    main = torch.cuda.current_stream(device)
    first = dataset.host_chunk(indices[0])
    ring = [torch.empty(first.shape, dtype=first.dtype, device=device) for _ in range(depth)]
    uploaded = [torch.cuda.Event() for _ in range(depth)]
    consumed = [torch.cuda.Event() for _ in range(depth)]

    def count(c):
        return min(g, len(indices) - c * g)

    def upload(c):
        slot, k = c % depth, count(c)
        with torch.cuda.stream(copy_stream):
            if c >= depth:
                copy_stream.wait_event(consumed[slot])
            src = dataset.host_chunk(indices[c * g])
            if k == g:
                ring[slot].copy_(src, non_blocking=True)
            else:                                               # ragged last chunk: only the frames that exist
                ring[slot][:, :k].copy_(src[:, :k], non_blocking=True)
            uploaded[slot].record(copy_stream)

    for c in range(min(depth - 1, n_chunks)):
        upload(c)
    for c in range(n_chunks):
        if c + depth - 1 < n_chunks:
            upload(c + depth - 1)
        slot, k = c % depth, count(c)
        main.wait_event(uploaded[slot])
        yield indices[c * g:c * g + k], ring[slot][:, :k]
        consumed[slot].record(main)


class DataModule:
    """Accepts the reference's init_args (data_dir, num_workers, crop_size, ...).  `test_frames()` = the reference's first test
    loader (ArtificialTestDataset over data_dir / "Test") when that directory exists; otherwise a synthetic stand-in:
    `synthetic: video` (default, n_frames float frames), `synthetic: artificial` (n_frames uint8 pairs x 31 distortions) or
    `synthetic: video_u8` (n_frames uint8 frames in pinned groups of `group` = 8: configs[4]) or `synthetic: video_yuv` (the same as
    packed I420 chunks, decoded on the device).  `y4m_target` (+ `y4m_reference`, optional `y4m_gt`): the dataset is StereoY4MVideo
    over those Y4M files, whatever else is given; `yuv_matrix` ("bt709") and `yuv_range` (None: the files' XCOLORRANGE, else limited)
    choose the conversion.
    `val_dataloader()` = the reference's two validation loaders (utils/data.py:150-166): ArtificialTrainValDataset over data_dir /
    "Validation" in batches of `batch_size`, and the real-world set one frame per batch; without those directories `synthetic:
    trainval` stands in (n_frames uint8 pairs x image_repeats crops; n_frames float frames for the real-world loader).  `crop_size`,
    `image_repeats` and `batch_size` are read by that path only.
    `png_decoder`: "host" (default: PIL on the calling thread) or "device" (ct_hip.png_decode, `decode_ahead` samples per call) for
    the datasets that read files; the synthetic ones have nothing to decode."""

    def __init__(self, data_dir=None, num_workers=0, crop_size=None, image_repeats=None, batch_size=None,
                 n_frames=8, height=270, width=480, synthetic="video", group=8, png_decoder="host", decode_ahead=16,
                 y4m_target=None, y4m_reference=None, y4m_gt=None, yuv_matrix="bt709", yuv_range=None, **_):
        self.png_decoder, self.decode_ahead = check_png_decoder(png_decoder), max(int(decode_ahead), 1)
        self.data_dir = Path(data_dir) if data_dir else None
        self.crop_size, self.image_repeats, self.batch_size = crop_size, image_repeats, batch_size
        self._synthetic = (synthetic, n_frames, height, width)
        if y4m_target:
            if not y4m_reference:
                raise ValueError("data.y4m_target needs data.y4m_reference (the other view)")
            self.dataset = StereoY4MVideo(y4m_target, y4m_reference, y4m_gt, group=group, matrix=yuv_matrix, range=yuv_range)
        elif self.data_dir is not None and (self.data_dir / "Test").is_dir():
            self.dataset = ArtificialTestDataset(self.data_dir / "Test", self.png_decoder)
        elif synthetic == "artificial":
            self.dataset = SyntheticArtificialTest(n_frames, height, width)
        elif synthetic == "video_u8":
            self.dataset = SyntheticStereoVideoU8(n_frames, height, width, group=group)
        elif synthetic == "video_yuv":
            self.dataset = SyntheticStereoVideoYUV(n_frames, height, width, group=group, matrix=yuv_matrix, range=yuv_range)
        else:
            self.dataset = SyntheticStereoFrames(n_frames, height, width)

    def test_frames(self):
        return self.dataset

    def test_dataloader(self):
        """[artificial, real-world] like utils/data.py:168-179 (the second only when its directory exists)"""
        loaders = [self.dataset]
        if self.data_dir is not None and (self.data_dir / "Real-World Test").is_dir():
            loaders.append(RealWorldTestDataset(self.data_dir / "Real-World Test", self.png_decoder))
        return loaders

    def val_dataloader(self):
        """[artificial, real-world] like utils/data.py:150-166, as BatchLoaders"""
        synthetic, n_frames, height, width = self._synthetic
        if self.crop_size is None:
            raise ValueError("val_dataloader needs data.crop_size (and takes data.image_repeats, data.batch_size)")
        repeats = 1 if self.image_repeats is None else self.image_repeats
        if self.data_dir is not None and (self.data_dir / "Validation").is_dir():
            artificial = ArtificialTrainValDataset(self.data_dir / "Validation", self.crop_size, repeats, self.png_decoder)
        elif synthetic == "trainval":
            artificial = SyntheticTrainVal(n_frames, height, width, self.crop_size, repeats)
        else:
            raise ValueError("no %s directory: `data.synthetic: trainval` makes a synthetic validation set"
                             % (self.data_dir / "Validation" if self.data_dir is not None else "data_dir / Validation"))
        if self.data_dir is not None and (self.data_dir / "Real-World Test").is_dir():
            real = RealWorldTestDataset(self.data_dir / "Real-World Test", self.png_decoder)
        else:
            real = SyntheticStereoFrames(n_frames, height, width)
        return [BatchLoader(artificial, self.batch_size, "artificial", self.decode_ahead), BatchLoader(real, 1, "real-world", self.decode_ahead)]
