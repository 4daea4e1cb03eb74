"""`python -m utils.cli test --config <yaml> [--model.func_spec ...] [--data.n_frames N] [--ckpt_path P]`
`python -m utils.cli predict --config <yaml> --output DIR [--format png|npy|raw|y4m|null] [--views a,b,c] [--writer.depth D] [--writer.workers N] [--writer.png_encoder host|device] [...]`
both with `[--inference.scale_factor S] [--inference.antialias B]`
`python -m utils.cli validate --config <yaml> [--ckpt_path P] [--data.synthetic trainval] [--data.crop_size [H,W]] [--data.image_repeats R] [--data.batch_size B] [--seed_everything N]`

A minimal look-alike of the reference's LightningCLI entry point (utils/cli.py:1-3, README.md:69-71) for the
`test` and `predict` sub-commands (Lightning/jsonargparse are not part of this stack): YAML with `class_path/init_args`
for model and data, dotted `--section.key value` overrides, `trainer.*` keys accepted and ignored.  Frames are
sharded over ranks when launched with torch.distributed.run (frame f -> rank f % world).

`test`: the per-frame metrics (PSNR, SSIM, FSIM, iCID: the reference's Test PSNR / Test SSIM / Test FSIM / Test iCID) are gathered
with ONE collective (utils/sharding.py); rank 0 prints their means.

`predict`: the corrected frames themselves, as bytes -- rint(clamp(x, 0, 1) * 255) on the device (ct_hip.pack_u8, the reference's
img_as_ubyte(x.clip(0, 1)), utils/postprocess.py:138-144), downloaded through a ring of pinned buffers and written by frame index
(utils/writer.py): every rank writes its own frames into the one directory, the result does not depend on the world size.

`predict --views corrected,chess,rgbmse,rgbssim,...`: next to every corrected frame `%06d.<ext>` the listed diagnostic views of that frame, as
`%06d.<view>.<ext>` -- the image panel of the reference's log_images, from the model's `views()` (methods/__init__.py, methods/dcmcs3di.py,
methods/dmsct.py), one forward per frame for all of them.  Which views exist depends on the model; one it does not offer is refused
before the first frame.  Not with `--format raw` (one file) and not with the `inference` section.  Without `--views` nothing changes.

`inference` (optional section, `inference: {scale_factor: 0.75, antialias: false}` or `--inference.scale_factor 0.75`): the model runs
at a reduced size through its `forward_scaled` -- bicubic down, forward, bicubic back up, the reference's demo notebook, cell 24 -- and
metrics / frames are those of the full-size result.  A model without `forward_scaled` is refused.  Without the section nothing changes.

`validate`: the reference's validation epoch (`validation_step` over the two loaders of DataModule.val_dataloader(): random crops of
the artificial validation set in batches of data.batch_size -- crop, flips and the chain of colour adjustments of a whole batch in
one ct_hip.augment_u8 call -- and the real-world set frame by frame).  Per loader, rank 0 prints what the model's validation_step
returns (methods.dmsct.DMSCT: MSE Loss, SSIM Loss, PSNR, SSIM, FSIM, iCID, loss) as `Validation <name>/dataloader_idx_<i>`: the mean
over samples, every batch weighted by its size, as Lightning reduces an epoch.  Samples are sharded like frames (sample f -> rank
f % world; a rank batches its own samples), one collective per loader.  `seed_everything: N` seeds numpy's and torch's global
generators, from which the dataset draws, before the first loader.  The `inference` section is not used.  A model without
`validation_step` (Runner: the reference has none), one that lacks losses (DCMCS3DI) and CT_CLI_DEVICE=cpu are refused before the
first frame.

`predict --writer.png_encoder device` (with `--format png`, the default): the PNG files are compressed on the GPU -- row filters and
a Huffman code per 16 rows (ct_hip.png_deflate, csrc/png.hip), one launch per group of frames or per view -- and the writer's threads
only wrap the downloaded streams into the container (utils/png.py).  The files decode to the same pixels; they are larger than the
host encoder's (no LZ77 matching).  It goes with `--views`; under CT_CLI_DEVICE=cpu it is refused before the first frame.  The default
is `host`: PIL on the writer's threads, as before.

`--data.png_decoder device [--data.decode_ahead N]` (test, validate, predict; datasets that read PNG files): the files are inflated
and unfiltered on the GPU (ct_hip.png_decode, csrc/png_decode.hip), N samples' files per call (default 16,
utils.data.prefetch_decoded); what the device decoder does not take (anything but 8-bit RGB without interlace) is decoded by PIL as
before, file by file.  Under CT_CLI_DEVICE=cpu it is refused before the first frame.  The default is `host`: nothing changes.

`--data.y4m_target T.y4m --data.y4m_reference R.y4m [--data.y4m_gt G.y4m] [--data.yuv_matrix bt709|bt601] [--data.yuv_range limited|full]`
(test, predict) and `--data.synthetic video_yuv`: stereo video as 8-bit Y'CbCr 4:2:0 (utils.data.StereoY4MVideo over Y4M files, the
stand-in for the reference's cv2.VideoCapture; or synthetic I420 chunks).  The frames are uploaded as YUV, 1.5 bytes per pixel, and a
whole group is converted by one ct_hip.yuv420_to_rgb launch into the uint8 RGB group every grouped method takes.  Without `y4m_gt`,
`predict` works and `test` is refused before the first frame.  `predict --format y4m [--writer.y4m_fps 25:1] [--writer.y4m_aspect 1:1]`:
the corrected frames leave as ONE file `frames.y4m` (ct_hip.rgb_to_yuv420 on the device, 1.5 bytes per pixel downloaded), by
definition the YUV of the bytes `--format png` would have written; with a Y4M input the rate, aspect, siting and range are inherited
from it, the matrix from `--data.yuv_matrix`.  Not with `--views`.  Under CT_CLI_DEVICE=cpu the format and the YUV datasets are refused
before the first frame.

`--model.byte_groups true`, `--model.iterative_groups true`, `--model.grading_groups true` (test, predict; `Runner` with
`--model.metrics psnr` on a loader of uint8 groups): MK and Xiao, the iterative distribution transfer, automated colour grading take a
whole group of uint8 frames per call (`Runner.takes_groups()`, `test_group`, `predict_group`) instead of one float32 frame.  Each flag
touches its own methods only; without them nothing changes.

`--model.metric_groups true` (test, predict; `Runner` on a loader of uint8 groups): the grouped route is taken with ANY metric list, the
default four included.  `test` fills its [n, 4] table through `Runner.test_group_metrics`: the grouped transfer + PSNR as above, then
SSIM, FSIM and iCID read the group's float32 result and the ground-truth bytes where they lie (ct_hip.frame_*_hwc), no clamp, permute
or conversion pass in between.  Which methods are grouped still depends on the three flags above; with `--model.metrics psnr` the flag
changes nothing.  `predict` follows `Runner.takes_groups()` and is therefore grouped under the flag for any metric list (it computes no
metric).  Under CT_CLI_DEVICE=cpu the flag is accepted and the per-frame route runs as before.  Without the flag nothing changes.

`--model.icid_intent perceptual|hue-preserving|chromatic`, `--model.icid_omit_maps67 true`, `--model.icid_downsampling false` (test;
`Runner`): the other arguments of the reference's `utils.icid.icid(img1, img2, intent, omit_maps67, downsampling)` for the `Test iCID`
column, on the per-frame route (`test_step`) and on the grouped one (`test_group_metrics`) alike.  hue-preserving and chromatic weight
the hue (and chroma) difference ten times more; omit_maps67 drops chroma contrast and chroma structure; `icid_downsampling false`
scores the frame at its own size instead of after the resize by 1 / max(1, round(min(H, W) / 256)).  An unknown intent is refused when
the model is built, with the reference's message.  The defaults are the reference's: without the flags nothing changes.
"""
import importlib
import inspect
import os
import sys
import types

import torch
import yaml


def _set(cfg, dotted, value):
    """`--model.func_spec X`, `--model.init_args.func_spec X` (LightningCLI's canonical form) and `--model.class_path X`"""
    keys = dotted.split(".")
    node, in_init = cfg, False
    for k in keys[:-1]:
        if in_init and k == "init_args":
            continue                                  # already inside init_args: the explicit component is redundant
        node = node.setdefault(k, {})
        if k in ("model", "data") and keys[-1] != "class_path":
            node = node.setdefault("init_args", {})
            in_init = True
    # a ratio like 25:1 is a sexagesimal integer to YAML 1.1: these keys keep their text
    node[keys[-1]] = value if keys[-1] in ("y4m_fps", "y4m_aspect") else yaml.safe_load(value)


def _instantiate(section):
    module, cls = section["class_path"].rsplit(".", 1)
    return getattr(importlib.import_module(module), cls)(**section.get("init_args", {}))


def quantise_u8(x):
    """ct_hip.pack_u8's rule in torch, for the CT_CLI_DEVICE=cpu test mode only (torch.round is ties-to-even)"""
    return (x.clamp(0, 1).nan_to_num(0) * 255).round().to(torch.uint8)


ALL_VIEWS = ("corrected", "chess", "rgbmse", "disparity", "flow", "warped_right", "occlusions", "rgbssim", "labmse", "abmse")     # over all models
CPU_VIEWS = ("corrected", "chess", "rgbmse")
DEVICE_ONLY_VIEWS = ("rgbssim", "labmse", "abmse")     # methods.EXTRA_VIEWS: every model's views() takes them by name, no CPU stand-in


def chess_mix_cpu(x, y, size=25):
    """ct_hip.chess_mix's rule in torch, for the CT_CLI_DEVICE=cpu test mode only"""
    h, w = x.shape[-2:]
    pick = (torch.arange(h)[:, None] // size + torch.arange(w)[None, :] // size) % 2 == 0
    return torch.where(pick, x, y)


def rgbmse_cpu(x, y):
    """ct_hip.rgbmse_view's rule in torch (the channels added in their order, divided by 3), for the CT_CLI_DEVICE=cpu test mode only"""
    d = x - y
    m = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) / 3
    lo, hi = m.amin(dim=(-1, -2), keepdim=True), m.amax(dim=(-1, -2), keepdim=True)
    out = torch.zeros_like(x)
    out[:, 0] = (m - lo) / (hi - lo)
    return out


def _view_names(value, fmt):
    """the `--views` option -> a tuple of known view names; refused with `raw` (one file holds one image per frame)"""
    names = tuple(n.strip() for n in str(value).split(","))
    if not all(names):
        raise SystemExit("--views %r: a comma-separated list of view names (%s)" % (value, ", ".join(ALL_VIEWS)))
    bad = [n for n in names if n not in ALL_VIEWS]
    if bad:
        raise SystemExit("--views: unknown view %s; the views are %s" % (", ".join(map(repr, bad)), ", ".join(ALL_VIEWS)))
    if len(set(names)) != len(names):
        raise SystemExit("--views %r names a view twice" % (value,))
    if fmt in ("raw", "y4m"):
        raise SystemExit("--views does not go with --format %s: a %s video is one file with one image per frame; use png or npy" % (fmt, fmt))
    return names


def _check_views(ctx, names):
    """before the first frame: the model offers every view asked for (CT_CLI_DEVICE=cpu: the torch restatements above, no more)"""
    model = ctx.model
    if ctx.scaled:
        raise SystemExit("--views does not combine with the `inference` section (reduced-scale inference has no views())")
    if ctx.on_cpu and any(n in DEVICE_ONLY_VIEWS for n in names):
        raise ValueError("--views: %s run on the device only (csrc/errmaps.hip): not under CT_CLI_DEVICE=cpu"
                         % ", ".join(n for n in names if n in DEVICE_ONLY_VIEWS))
    offered = CPU_VIEWS if ctx.on_cpu else tuple(getattr(model, "VIEWS", ())) + DEVICE_ONLY_VIEWS if hasattr(model, "views") else ()
    missing = [n for n in names if n not in offered]
    if missing:
        where = " under CT_CLI_DEVICE=cpu" if ctx.on_cpu else ""
        raise SystemExit("--views: %s does not offer the view %s%s (it offers: %s)"
                         % (type(model).__name__, ", ".join(map(repr, missing)), where, ", ".join(offered) or "none"))


def _inference(cfg, model):
    """the optional `inference` section -> None, or the keyword arguments of model.forward_scaled"""
    sec = cfg.get("inference")
    if not sec:
        return None
    if not isinstance(sec, dict) or set(sec) - {"scale_factor", "antialias"} or "scale_factor" not in sec:
        raise SystemExit("the `inference` section takes `scale_factor` (required) and `antialias`; got %r" % (sec,))
    sf, aa = sec["scale_factor"], sec.get("antialias", False)
    if isinstance(sf, bool) or not isinstance(sf, (int, float)) or not 0 < sf < float("inf") or not isinstance(aa, bool):
        raise SystemExit("inference.scale_factor must be a positive number and inference.antialias true or false; got %r" % (sec,))
    if not hasattr(model, "forward_scaled"):
        raise SystemExit("the `inference` section (reduced-scale inference) needs a model with `forward_scaled`; %s has none "
                         "(methods.dcmcs3di.DCMCS3DI does)" % type(model).__name__)
    return {"scale_factor": float(sf), "antialias": aa}


def _parse(argv):
    """argv after the sub-command -> (cfg, ckpt_path, {"output", "format"}); everything else is a dotted override of the YAML"""
    cfg, ckpt, opts, i = {}, None, {}, 1
    if (len(argv) - 1) % 2:
        raise SystemExit("arguments come in `--key value` pairs; got a dangling %r" % argv[-1])
    while i < len(argv):
        key, val = argv[i], argv[i + 1]
        if key == "--config":
            with open(val) as fh:
                cfg = yaml.safe_load(fh) or {}
        elif key == "--ckpt_path":
            ckpt = val
        elif argv[0] == "predict" and key in ("--output", "--format", "--views"):
            opts[key[2:]] = val
        elif key.startswith("--"):
            _set(cfg, key[2:], val)
        i += 2
    return cfg, ckpt, opts


def _model_class(cfg):
    module, cls = cfg["model"]["class_path"].rsplit(".", 1)
    return getattr(importlib.import_module(module), cls)


VALIDATION = ("MSE Loss", "SSIM Loss", "PSNR", "SSIM", "FSIM", "iCID", "loss")      # what a validation_step returns, in the reference's order


def _check_validate(cfg):
    """before anything touches a device: `validate` needs a GPU and a model class with a complete validation_step"""
    if "class_path" not in (cfg.get("model") or {}):
        raise SystemExit("validate needs `--config <yaml>` with a `model` section (class_path / init_args), like `test` and `predict`")
    if os.environ.get("CT_CLI_DEVICE", "cuda") == "cpu":
        raise SystemExit("validate needs a GPU: the samples are made and the losses computed on the device (ct_hip.augment_u8, "
                         "ct_hip.frame_losses); there is no CT_CLI_DEVICE=cpu stand-in")
    if "inference" in cfg:
        raise SystemExit("validate does not use the `inference` section (the reference validates at the size of its crops)")
    cls = _model_class(cfg)
    if not hasattr(cls, "validation_step"):
        raise SystemExit("validate needs a model with `validation_step`; %s has none (the reference's Runner has none either; "
                         "methods.dmsct.DMSCT does)" % cls.__name__)
    missing = getattr(cls, "VALIDATION_MISSING", ())
    if missing:
        raise SystemExit("validate: %s.validation_step lacks %s of the reference's step; methods.dmsct.DMSCT validates"
                         % (cls.__name__, ", ".join(missing)))


def _setup(cfg, ckpt, validate=False):
    """what the sub-commands share: rank / device selection, the process group, the model (+ checkpoint) and the loaders"""
    import torch.distributed as dist
    from utils import sharding as sh
    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    sh.pin_rank_to_cpus(int(os.environ.get("LOCAL_RANK", 0)), int(os.environ.get("LOCAL_WORLD_SIZE", world)))   # before any GPU call
    # CT_CLI_DEVICE=cpu: the host logic (argv / YAML handling, sharding, the one gather, the printed means) on CPU tensors with
    # the gloo backend -- for tests of a multi-rank run without GPUs.  It is no compute fallback: methods.* still need the
    # HIP library and raise without it; only a model whose test_step works on CPU tensors (a test stub) runs this way.
    on_cpu = os.environ.get("CT_CLI_DEVICE", "cuda") == "cpu"
    device = torch.device("cpu") if on_cpu else torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)))
    if not on_cpu:
        torch.cuda.set_device(device)
    own_group = world > 1 and not dist.is_initialized()          # a caller (bench.py) may have built the communicator already
    if own_group:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if on_cpu:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
    if world > 1 and dist.get_world_size() != world:
        raise SystemExit("WORLD_SIZE=%d but the process group has %d ranks" % (world, dist.get_world_size()))
    model = _instantiate(cfg["model"]).to(device).eval()
    scaled = _inference(cfg, model)
    if ckpt:
        # Lightning checkpoints carry hyper-parameters / optimizer state next to "state_dict"; weights_only=True refuses the
        # ones that pickle arbitrary objects.  Falling back to the unsafe loader executes whatever the file pickles, so it
        # happens only for that one error class and never silently; CT_TRUST_CKPT=0 forbids it.
        import pickle
        try:
            state = torch.load(ckpt, map_location=device, weights_only=True)
        except pickle.UnpicklingError as e:
            if os.environ.get("CT_TRUST_CKPT", "1") == "0":
                raise
            print("warning: %s is not loadable with weights_only=True (%s); loading it as a TRUSTED pickle "
                  "(set CT_TRUST_CKPT=0 to refuse)" % (ckpt, str(e).splitlines()[0][:120]), file=sys.stderr)
            state = torch.load(ckpt, map_location=device, weights_only=False)
        model.load_state_dict(state["state_dict"] if "state_dict" in state else state, strict=True)
    data_cfg = dict(cfg.get("data", {}))
    data_cfg["class_path"] = "utils.data.DataModule"
    dm = _instantiate(data_cfg)
    loaders = dm.val_dataloader() if validate else dm.test_dataloader()

    def fence():
        if world > 1:
            dist.barrier()
        if not on_cpu:
            torch.cuda.synchronize()

    def samples(frames, indices):
        """(index, sample) of a loader: `prefetch`, or `prefetch_decoded` for a file dataset with --data.png_decoder device"""
        from utils.data import prefetch, prefetch_decoded
        if not on_cpu and getattr(frames, "png_decoder", "host") == "device":
            return prefetch_decoded(frames, indices, device, dm.decode_ahead)
        return prefetch(frames, indices, device)

    return types.SimpleNamespace(rank=rank, world=world, on_cpu=on_cpu, device=device, own_group=own_group, model=model,
                                 loaders=loaders, fence=fence, scaled=scaled, samples=samples)


def main(argv=None, timing=None):
    """`test` returns the [n_frames, 4] metric table of the first loader, `predict` the number of frames written, `validate` the list
    of its loaders' [n_samples, 7] tables (cli.VALIDATION; a sample's row holds the values of its batch).
    timing: None, or a dict that receives {"seconds", "frames", "frames_local", "h2d_bytes"} of the first loader's loop --
    barrier + synchronize on both sides, the gather inside, an untimed first pass over a few groups before it (code objects,
    clocks, the communicator) -- for bench.py's configs[4] leg, which measures THIS entry point rather than a loop of its own.
    `predict` fills it the same way (+ "d2h_bytes"), the writer's drain inside the measurement."""
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] not in ("test", "predict", "validate"):
        raise SystemExit("only the `test`, `predict` and `validate` sub-commands exist here (fit is Lightning's training path)")
    cfg, ckpt, opts = _parse(argv)
    if argv[0] == "validate":
        _check_validate(cfg)
    if argv[0] == "predict":
        from utils.writer import FORMATS
        if not opts.get("output"):
            raise SystemExit("predict needs `--output DIR`: the directory the corrected frames are written to")
        if opts.setdefault("format", "png") not in FORMATS:
            raise SystemExit("--format %r: one of %s" % (opts["format"], ", ".join(FORMATS)))
        if opts["format"] == "y4m" and os.environ.get("CT_CLI_DEVICE", "cuda") == "cpu":
            raise SystemExit("--format y4m needs a GPU: the frames are converted on the device (ct_hip.rgb_to_yuv420); under "
                             "CT_CLI_DEVICE=cpu there is none; use png, npy or raw")
        views = _view_names(opts["views"], opts["format"]) if "views" in opts else None
        from utils.writer import PNG_ENCODERS
        encoder = (cfg.get("writer") or {}).get("png_encoder", "host")
        if encoder not in PNG_ENCODERS:
            raise SystemExit("--writer.png_encoder %r: one of %s" % (encoder, ", ".join(PNG_ENCODERS)))
        if encoder == "device" and os.environ.get("CT_CLI_DEVICE", "cuda") == "cpu":
            raise SystemExit("--writer.png_encoder device needs a GPU: under CT_CLI_DEVICE=cpu the frames are host tensors and there "
                             "is no device to encode on; use the default `host` encoder")
    from utils.data import PNG_DECODERS
    decoder = ((cfg.get("data") or {}).get("init_args") or {}).get("png_decoder", "host")
    if decoder not in PNG_DECODERS:
        raise SystemExit("--data.png_decoder %r: one of %s" % (decoder, ", ".join(PNG_DECODERS)))
    if decoder == "device" and os.environ.get("CT_CLI_DEVICE", "cuda") == "cpu":
        raise SystemExit("--data.png_decoder device needs a GPU: under CT_CLI_DEVICE=cpu the frames are host tensors and there "
                         "is no device to decode on; use the default `host` decoder")
    data_args = (cfg.get("data") or {}).get("init_args") or {}
    if (data_args.get("y4m_target") or data_args.get("synthetic") == "video_yuv") and os.environ.get("CT_CLI_DEVICE", "cuda") == "cpu":
        raise SystemExit("--data.y4m_target / --data.synthetic video_yuv need a GPU: the frames are converted on the device "
                         "(ct_hip.yuv420_to_rgb); there is no CT_CLI_DEVICE=cpu stand-in")
    ctx = _setup(cfg, ckpt, validate=argv[0] == "validate")
    import torch.distributed as dist
    try:
        if argv[0] == "validate":
            return _validate(ctx, cfg.get("seed_everything"))
        if argv[0] == "predict":
            if views:
                _check_views(ctx, views)
            return _predict(ctx, opts["output"], opts["format"], cfg.get("writer") or {}, timing, views)
        return _test(ctx, timing)
    finally:
        if ctx.own_group:
            dist.destroy_process_group()


def _test(ctx, timing):
    import torch.distributed as dist
    from utils import sharding as sh
    from methods import METRICS, fsim, icid, psnr, ssim
    from utils.data import prefetch_groups
    rank, world, on_cpu, device, model, loaders, fence = ctx.rank, ctx.world, ctx.on_cpu, ctx.device, ctx.model, ctx.loaders, ctx.fence
    # the reference's test_dataloader() returns [artificial, real-world] (utils/data.py:168-179) and Lightning logs each
    # metric once per loader ("Test PSNR/dataloader_idx_1"); a single loader prints the bare names like Lightning does
    tables = []
    for frames in loaders:
        if getattr(frames, "has_gt", True) is False:        # before the first frame
            raise SystemExit("test needs a ground truth: pass --data.y4m_gt (without it only `predict` works)")
    for li, frames in enumerate(loaders):
        mine = sh.frames_of_rank(len(frames), rank, world)
        grouped = (not ctx.scaled and not on_cpu and hasattr(frames, "host_chunk") and hasattr(model, "test_group") and model.takes_groups())
        if grouped:
            # uint8 frames in pinned groups (configs[4]): one upload and ONE fused call per group -- transfer + clamp + PSNR of
            # Runner.test_step (methods/__init__.py:29-32) -- no torch kernel in the loop, one gather at the end
            # --model.metric_groups: the [n, 4] table itself, filled by test_group_metrics (SSIM, FSIM, iCID from the group's buffers)
            # (with PSNR alone the flag changes nothing: the route above)
            whole = bool(getattr(model, "metric_groups", False)) and tuple(getattr(model, "metrics", ())) != ("psnr",)
            rec = (torch.full((len(mine), len(METRICS)), float("nan"), dtype=torch.float64, device=device) if whole else
                   torch.zeros((max(len(mine), 1), 2), dtype=torch.float64, device=device))
            score = model.test_group_metrics if whole else model.test_group

            def run(indices):
                n = 0
                for ids, dev in prefetch_groups(frames, indices, device):
                    score(dev, rec[n:n + len(ids)])
                    n += len(ids)

            if timing is not None and li == 0:
                if hasattr(frames, "prepare"):
                    frames.prepare(mine)                        # the synthetic frames themselves: made before the clock starts
                run(mine[:3 * frames.group])                    # initialisation, not part of the measurement
                fence()
                import time
                t0 = time.perf_counter()
            run(mine)
            if whole:
                local = rec
            else:
                local = torch.full((len(mine), len(METRICS)), float("nan"), dtype=torch.float64, device=device)
                local[:, 0] = rec[:len(mine), 1]
        else:
            if timing is not None and li == 0:
                fence()
                import time
                t0 = time.perf_counter()
            rows = []
            for f, sample in ctx.samples(frames, mine):            # pinned double-buffered uploads on a second stream (prefetch)
                batch = {k: v.unsqueeze(0) for k, v in sample.items()}
                if ctx.scaled:                          # reduced-scale inference, scored at full size like the branch below
                    corrected = model.forward_scaled(batch["target"], batch["reference"], **ctx.scaled)[0].clamp(0, 1)
                    rows.append(torch.stack([fn(corrected, batch["gt"]).reshape(()) for fn in (psnr, ssim, fsim, icid)]))
                elif hasattr(model, "test_step"):
                    m = model.test_step(batch, f)
                    nan = torch.full((), float("nan"), device=device)
                    rows.append(torch.stack([m[k].reshape(()).to(device) if k in m else nan for k in METRICS]))
                else:                                   # CNN modules: forward(target, reference, inference=True)
                    corrected, _ = model(batch["target"], batch["reference"], inference=True)
                    corrected = corrected.clamp(0, 1)
                    rows.append(torch.stack([fn(corrected, batch["gt"]).reshape(()) for fn in (psnr, ssim, fsim, icid)]))
            local = torch.stack(rows).double() if rows else torch.zeros((0, len(METRICS)), dtype=torch.float64, device=device)
        table = sh.gather_frame_metrics(local, len(frames), rank, world)        # [n_frames, 4]: PSNR, SSIM, FSIM, iCID per frame
        if timing is not None and li == 0:
            fence()
            dt = time.perf_counter() - t0
            if world > 1:
                tmax = torch.tensor([dt], dtype=torch.float64, device=device)
                dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
                dt = float(tmax.item())
            per_frame = getattr(frames, "upload_bytes_per_frame", 3 * frames.height * frames.width * 3) if grouped else 0
            timing.update({"seconds": dt, "frames": len(frames), "frames_local": len(mine), "h2d_bytes": per_frame * len(mine),
                           "grouped": grouped, "frames_per_call": frames.group if grouped else 1})
        tables.append(table)
        if rank == 0:
            suffix = "/dataloader_idx_%d" % li if len(loaders) > 1 else ""
            cols = [(i, name) for i, name in enumerate(METRICS) if not bool(torch.isnan(table[:, i]).all())]
            for j, (i, name) in enumerate(cols):
                print("%s%s: %.4f" % (name, suffix, float(table[:, i].mean())), end="   " if j + 1 < len(cols) else "")
            print("  (%d frames, %d GPU%s)" % (len(frames), world, "" if world == 1 else "s"))
    return tables[0]


def _validate(ctx, seed):
    from utils import sharding as sh
    rank, world, device, model = ctx.rank, ctx.world, ctx.device, ctx.model
    if seed is not None:                                    # the generators the dataset draws from (utils/data.py: sample_params)
        import numpy as np
        np.random.seed(int(seed))
        torch.manual_seed(int(seed))
    tables = []
    for li, loader in enumerate(ctx.loaders):
        mine = sh.frames_of_rank(len(loader), rank, world)
        rows = []
        for n, (ids, batch) in enumerate(loader.batches(mine, device)):
            m = model.validation_step(batch, n, li)
            # every sample carries the values of its batch: the mean over samples weights the batches by their size (Lightning's epoch mean)
            rows.append(torch.stack([m[k].reshape(()).double() for k in VALIDATION]).expand(len(ids), -1))
        local = torch.cat(rows) if rows else torch.zeros((0, len(VALIDATION)), dtype=torch.float64, device=device)
        table = sh.gather_frame_metrics(local, len(loader), rank, world)
        tables.append(table)
        if rank == 0:
            for j, name in enumerate(VALIDATION):
                print("Validation %s/dataloader_idx_%d: %.4f" % (name, li, float(table[:, j].mean())), end="   " if j + 1 < len(VALIDATION) else "")
            print("  (%d samples, %d GPU%s)" % (len(loader), world, "" if world == 1 else "s"))
    return tables


def _predict(ctx, output, fmt, writer_cfg, timing, views=None):
    import time
    import torch.distributed as dist
    from utils import sharding as sh
    from utils.data import prefetch_groups
    from utils.writer import FrameWriter, truncate_raw, truncate_y4m, y4m_options
    rank, world, on_cpu, device, model, loaders, fence = ctx.rank, ctx.world, ctx.on_cpu, ctx.device, ctx.model, ctx.loaders, ctx.fence
    depth, workers = int(writer_cfg.get("depth", 3)), int(writer_cfg.get("workers", 4))
    if not on_cpu:
        import ct_hip
    takes_batch = bool(views) and not on_cpu and "batch" in inspect.signature(model.views).parameters
    written = 0
    for li, frames in enumerate(loaders):
        out_dir = os.path.join(output, "idx_%d" % li) if len(loaders) > 1 else output
        mine = sh.frames_of_rank(len(frames), rank, world)
        grouped = (not views and not ctx.scaled and not on_cpu and hasattr(frames, "host_chunk") and hasattr(model, "predict_group")
                   and model.takes_groups())
        y4m = None
        if fmt == "y4m":
            # with a Y4M input the stream's rate, aspect, siting and range are its own; the command line's rate / aspect win
            if not hasattr(frames, "height") or not hasattr(frames, "width"):
                raise SystemExit("--format y4m needs a loader of ONE frame size (a video); %s has none" % type(frames).__name__)
            head = getattr(frames, "header", None)
            y4m = {"fps": writer_cfg.get("y4m_fps") or (head.fps if head is not None and head.fps != "0:0" else None),
                   "aspect": writer_cfg.get("y4m_aspect") or (head.aspect if head is not None and head.aspect != "0:0" else None),
                   "matrix": getattr(frames, "matrix", None), "range": getattr(frames, "range", None), "siting": getattr(frames, "siting", None)}
            try:
                y4m_options(y4m)                            # every rank refuses a bad ratio, before any of them waits for another
            except ValueError as e:
                raise SystemExit("--format y4m: %s" % e)
        if rank == 0:
            os.makedirs(out_dir, exist_ok=True)
            if fmt == "raw":
                truncate_raw(out_dir)                       # once, before any rank opens the file
            elif fmt == "y4m":
                truncate_y4m(out_dir, frames.height, frames.width, y4m)
        fence()
        # device uint8 ring, one slot per writer slot: a slot is packed into again only after its download has completed (the
        # stream waits for the event, the host does not)
        ring, downloaded = [None] * depth, [None] * depth

        def pack(n, x, layout):
            k, (h, w) = x.shape[0], (x.shape[1:3] if layout == "hwc" else x.shape[2:4])
            slot = n % depth
            if downloaded[slot] is not None:
                torch.cuda.current_stream(device).wait_event(downloaded[slot])
            if ring[slot] is None or ring[slot].shape[1:] != (h, w, 3) or ring[slot].shape[0] < k:
                ring[slot] = torch.empty((k, h, w, 3), dtype=torch.uint8, device=device)       # the old one: record_stream in submit
            return slot, ct_hip.pack_u8(x, layout, out=ring[slot][:k])

        def run(indices, writer):
            with torch.no_grad():
                if grouped:
                    # uint8 frames in pinned groups: one upload, ONE transfer call, one pack and ONE download per group of k frames
                    for n, (ids, dev) in enumerate(prefetch_groups(frames, indices, device)):
                        frames_out = model.predict_group(dev)
                        if frames_out.dtype == torch.uint8:     # --model.byte_groups / iterative_groups / grading_groups: bytes already, freshly allocated (as views are)
                            writer.submit(ids, frames_out)
                            continue
                        slot, u8 = pack(n, frames_out, "hwc")
                        downloaded[slot] = writer.submit(ids, u8)
                    return
                for n, (f, sample) in enumerate(ctx.samples(frames, indices)):
                    batch = {k: v.unsqueeze(0) for k, v in sample.items()}
                    if views and not on_cpu:
                        # ONE forward for the frame and all its views (freshly allocated uint8 frames: submit() holds them until
                        # their download has run); the plain file is the `corrected` view, the bytes of the branches below
                        want = views if "corrected" in views else ("corrected",) + views
                        vs = (model.views(batch, names=want) if takes_batch else             # the Runner interface / the CNN modules
                              model.views(batch["target"], batch["reference"], gt=batch.get("gt"), names=want))
                        writer.submit([f], vs["corrected"])
                        for name in views:
                            writer.submit([f], vs[name], suffix=name)
                        continue
                    if ctx.scaled:                              # reduced-scale inference: the full-size frame, clamped by the pack
                        corrected = model.forward_scaled(batch["target"], batch["reference"], **ctx.scaled)[0]
                    elif hasattr(model, "test_step"):           # the Runner interface: what test_step scores (methods/__init__.py:30)
                        corrected = model(batch).clamp(0, 1)
                    else:                                       # CNN modules: forward(target, reference, inference=True)
                        corrected = model(batch["target"], batch["reference"], inference=True)[0]
                    if on_cpu:
                        writer.submit([f], quantise_u8(corrected).permute(0, 2, 3, 1).contiguous())
                        for name in views or ():
                            img = corrected if name == "corrected" else (chess_mix_cpu if name == "chess" else rgbmse_cpu)(batch["gt"], corrected)
                            writer.submit([f], quantise_u8(img).permute(0, 2, 3, 1).contiguous(), suffix=name)
                        continue
                    corrected = corrected.float()
                    hwc = corrected.permute(0, 2, 3, 1)         # Runner.forward hands out a CHW view of HWC memory: no transpose then
                    slot, u8 = pack(n, hwc, "hwc") if hwc.is_contiguous() else pack(n, corrected.contiguous(), "chw")
                    downloaded[slot] = writer.submit([f], u8)

        writer = FrameWriter(out_dir, fmt, depth=depth, workers=workers, n_frames=len(frames), device=None if on_cpu else device,
                             png_encoder=writer_cfg.get("png_encoder", "host"), y4m=y4m)
        with writer:
            if timing is not None and li == 0:
                if grouped:
                    if hasattr(frames, "prepare"):
                        frames.prepare(mine)                    # the synthetic frames themselves: made before the clock starts
                    run(mine[:3 * frames.group], writer)        # initialisation, not part of the measurement
                fence()
                t0 = time.perf_counter()
            run(mine, writer)
            writer.close()                                      # drained: every frame of this rank is in its file
        fence()
        if timing is not None and li == 0:
            dt = time.perf_counter() - t0
            if world > 1:
                tmax = torch.tensor([dt], dtype=torch.float64, device=device)
                dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
                dt = float(tmax.item())
            per_frame = frames.height * frames.width * 3 if grouped else 0
            up = getattr(frames, "upload_bytes_per_frame", 3 * per_frame) if grouped else 0
            if fmt == "y4m" and grouped:
                down = frames.height * frames.width + 2 * ((frames.height + 1) // 2) * ((frames.width + 1) // 2)
            else:
                down = per_frame
            timing.update({"seconds": dt, "frames": len(frames), "frames_local": len(mine), "h2d_bytes": up * len(mine),
                           "d2h_bytes": down * len(mine), "grouped": grouped, "frames_per_call": frames.group if grouped else 1})
        written += len(frames)
        if rank == 0:
            suffix = "/dataloader_idx_%d" % li if len(loaders) > 1 else ""
            print("wrote %d frames to %s (%s, %d GPU%s)%s" % (len(frames), out_dir, fmt, world, "" if world == 1 else "s", suffix))
    return written


if __name__ == "__main__":
    main()
