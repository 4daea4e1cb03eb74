"""`Runner` -- the plugin loader of the reference (methods/__init__.py:10-40) without Lightning.

`Runner(func_spec)` resolves a dotted path "pkg.mod.func" with importlib exactly like the reference
(methods/__init__.py:14-16); `forward(batch)` applies it to every sample of the batch
(methods/__init__.py:18-27) and `test_step` clamps and scores the result (methods/__init__.py:29-40):
PSNR, SSIM, FSIM and iCID per frame on the GPU (ct_frame_*_f32; piq / kornia / torchvision arithmetic restated, see
oracle/metrics.py).  Whole groups of uint8 frames go through `test_group` / `predict_group` instead (`takes_groups()`); with
`metric_groups=True` for any metric list: `test_group_metrics` scores a group's own buffers (ct_frame_*_hwc_u8).

If the resolved module also offers a device-resident variant `<func>_cuda`, the batch never leaves
the GPU; otherwise the numpy callable is used through the same host round trip as the reference.
"""
import importlib

import torch


def psnr(x, y, data_range=1.0):
    """Peak signal-to-noise ratio per sample, [B] (piq.psnr semantics: mean over C,H,W, then 10 log10(1/mse)); the
    reduction runs in ct_frame_psnr_f32 (deterministic float64 sums) when the tensors live on the GPU."""
    if x.is_cuda and data_range == 1.0:
        import ct_hip
        return ct_hip.frame_psnr(x.float().contiguous(), y.float().contiguous())[:, 1]
    mse = ((x.double() - y.double()) ** 2).flatten(1).mean(dim=1)
    return 10.0 * torch.log10(data_range ** 2 / mse.clamp_min(1e-300))


def ssim(x, y):
    """piq.ssim(x, y) with piq's defaults, per sample [B] (GPU only: ct_frame_ssim_f32)."""
    import ct_hip
    return ct_hip.frame_ssim(x.float().contiguous(), y.float().contiguous())


def icid(x, y, intent="perceptual", omit_maps67=False, downsampling=True):
    """utils.icid.icid(x, y, intent, omit_maps67, downsampling), per sample [B] (GPU only: ct_frame_icid_f32, with other than
    the default arguments ct_frame_icid_opt_f32).  The reference returns the mean over the batch (utils.icid.icid here does
    too); test loaders use batch size 1 (utils/data.py:168-179), where the two coincide.  An unknown intent raises the
    reference's ValueError before the tensors are looked at."""
    import ct_hip
    ct_hip.icid_intent(intent)
    return ct_hip.frame_icid(x.float().contiguous(), y.float().contiguous(), intent=intent, omit_maps67=omit_maps67, downsampling=downsampling)


def fsim(x, y):
    """piq.fsim(x, y) with piq's defaults (chromatic), per sample [B] (GPU only: ct_frame_fsim_f32)."""
    import ct_hip
    return ct_hip.frame_fsim(x.float().contiguous(), y.float().contiguous())


EXTRA_VIEWS = ("rgbssim", "labmse", "abmse")                      # every model with a ground truth has them, but only when named
GT_VIEWS = ("chess", "rgbmse") + EXTRA_VIEWS                      # the views that compare with the ground truth


def select_views(offered, names, have_gt):
    """The `names` argument of a model's views(): None = every offered view (without a ground truth: those that need none), a
    comma-separated string or a sequence.  The EXTRA_VIEWS are never part of the default: they come when named.  Unknown names,
    and a view that needs gt without one, raise ValueError."""
    if names is None:
        return tuple(v for v in offered if have_gt or v not in GT_VIEWS)
    names = tuple(n.strip() for n in names.split(",")) if isinstance(names, str) else tuple(names)
    bad = [n for n in names if n not in offered and n not in EXTRA_VIEWS]
    if bad:
        raise ValueError("unknown view%s %s: this model offers %s, and by name only %s"
                         % ("s" if len(bad) > 1 else "", ", ".join(map(repr, bad)), ", ".join(offered), ", ".join(EXTRA_VIEWS)))
    if not have_gt and any(n in GT_VIEWS for n in names):
        raise ValueError("the views %s compare with the ground truth: pass gt" % " and ".join(n for n in names if n in GT_VIEWS))
    return names


def gt_views(view, corrected, gt):
    """`corrected`, `chess`, `rgbmse`, `rgbssim`, `labmse` or `abmse` of float32 [B,3,H,W] device tensors as uint8 [B,H,W,3], the
    panel of the reference's log_images (methods/dcmcs3di.py:131-135): pack_u8 of the frame, of chess_mix(gt, corrected), of
    rgbmse(gt, corrected), of rgbssim(gt, corrected); labmse and abmse are the two maps of utils/visualizations.py it does not log"""
    import ct_hip
    if view == "corrected":
        return ct_hip.pack_u8(corrected, "chw")
    fn = {"chess": ct_hip.chess_mix, "rgbmse": ct_hip.rgbmse_view, "rgbssim": ct_hip.rgbssim_view, "labmse": ct_hip.labmse_view,
          "abmse": ct_hip.abmse_view}[view]
    return ct_hip.pack_u8(fn(gt, corrected), "chw")


def mask_view(mask):
    """a 0/1 float mask [B,1,H,W] -> uint8 [B,H,W,3], 255 where it is set"""
    import ct_hip
    return ct_hip.pack_u8(mask.expand(-1, 3, -1, -1).contiguous(), "chw")


METRICS = ("Test PSNR", "Test SSIM", "Test FSIM", "Test iCID")        # what test_step logs, in its order (methods/__init__.py:37-40)


REINHARD_SPEC = "methods.linear.color_transfer_between_images"
MK_SPEC = "methods.linear.monge_kantorovitch_color_transfer"
XIAO_SPEC = "methods.linear.color_transfer_in_correlated_color_space"
IDT_SPEC = "methods.iterative.iterative_distribution_transfer"
ACG_SPEC = "methods.iterative.automated_color_grading"


class Runner(torch.nn.Module):
    def __init__(self, func_spec, metrics=None, byte_groups=False, iterative_groups=False, grading_groups=False, metric_groups=False,
                 icid_intent="perceptual", icid_omit_maps67=False, icid_downsampling=True):
        """func_spec: the reference's only argument (methods/__init__.py:12).  metrics (not in the reference): which of psnr, ssim,
        fsim, icid test_step computes -- default all four, like the reference; `psnr` alone lets the Reinhard transfer take its
        fused uint8 entry (test_group).  byte_groups (not in the reference; `--model.byte_groups true`): with `psnr` alone, MK
        (default decomposition) and Xiao take whole groups of uint8 frames as well, and predict_group hands out bytes.
        iterative_groups (not in the reference; `--model.iterative_groups true`): with `psnr` alone, the iterative distribution
        transfer takes whole groups of uint8 frames (ct_hip.idt_u8, one draw of rotations per frame in frame order).
        grading_groups (not in the reference; `--model.grading_groups true`): the same for automated_color_grading (ct_hip.acg_u8:
        the grouped IDT, then the regrain of the whole group in the launches of one frame).
        metric_groups (not in the reference; `--model.metric_groups true`): whole groups of uint8 frames are taken with ANY metric
        list, the default four included -- SSIM, FSIM and iCID then read the group's own buffers (test_group_metrics).  Which spec
        is grouped still depends on the three flags above.
        icid_intent, icid_omit_maps67, icid_downsampling (the reference calls utils.icid.icid with its defaults, which these are;
        `--model.icid_intent chromatic` etc.): the other arguments of utils.icid.icid, for test_step and test_group_metrics.  An
        unknown intent raises the reference's ValueError here."""
        super().__init__()
        import ct_hip
        ct_hip.icid_intent(icid_intent)
        self.icid_intent = icid_intent
        self.icid_omit_maps67 = bool(icid_omit_maps67)
        self.icid_downsampling = bool(icid_downsampling)
        self.metric_groups = bool(metric_groups)
        self.byte_groups = bool(byte_groups)
        self.iterative_groups = bool(iterative_groups)
        self.grading_groups = bool(grading_groups)
        specs = func_spec.split(".")
        module, func = ".".join(specs[:-1]), specs[-1]
        mod = importlib.import_module(module)
        self.func = getattr(mod, func)
        self.func_cuda = getattr(mod, func + "_cuda", None)
        self.func_spec = func_spec
        names = ("psnr", "ssim", "fsim", "icid") if metrics is None else tuple(m.strip() for m in (metrics.split(",") if isinstance(metrics, str) else metrics))
        if not names or any(m not in ("psnr", "ssim", "fsim", "icid") for m in names):
            raise ValueError("metrics: a subset of psnr, ssim, fsim, icid (got %r)" % (metrics,))
        self.metrics = names
        self._out = None

    def takes_groups(self):
        """True when whole groups of uint8 frames go through test_group / predict_group, which needs PSNR as the only metric (or
        metric_groups: then test_group_metrics scores the group): the
        Reinhard transfer (ONE fused call: ct_reinhard_psnr_u8 reads the bytes; k / 255 and its gamma expansion come from tables
        inside the kernel), with byte_groups MK in its default decomposition (ct_mk_u8) and Xiao (its pieces on bytes), and with
        iterative_groups the iterative distribution transfer (ct_idt_u8), with grading_groups automated_color_grading (ct_acg_u8)."""
        if self.metrics != ("psnr",) and not self.metric_groups:
            return False
        if self.func_spec == IDT_SPEC:
            return self.iterative_groups
        if self.func_spec == ACG_SPEC:
            return self.grading_groups
        return self.func_spec == REINHARD_SPEC or (self.byte_groups and self.func_spec in (MK_SPEC, XIAO_SPEC))

    def _group_buffer(self, group_u8, k):
        """float32 [k][H][W][3] on the group's device: one buffer, kept and reused while the frame size fits"""
        if self._out is None or self._out.shape[1:] != group_u8.shape[2:] or self._out.shape[0] < k or self._out.device != group_u8.device:
            self._out = torch.empty((k,) + tuple(group_u8.shape[2:]), dtype=torch.float32, device=group_u8.device)
        return self._out[:k]

    def _icid_options(self):
        return {"intent": self.icid_intent, "omit_maps67": self.icid_omit_maps67, "downsampling": self.icid_downsampling}

    def _iterative_u8(self):
        """the grouped entry of an iterative method (the two have one signature), else None"""
        import ct_hip
        return {IDT_SPEC: ct_hip.idt_u8, ACG_SPEC: ct_hip.acg_u8}.get(self.func_spec)

    def test_group(self, group_u8, psnr_out):
        """group_u8: device uint8 [3 roles: target, reference, gt][k][H][W][3]; psnr_out: float64 [k, 2] rows of the caller's table,
        filled with (mse, PSNR) per frame -- Runner.test_step's clamp + piq.psnr (methods/__init__.py:30-32) for k frames in one
        asynchronous call, nothing else on the stream.  byte_groups: MK is one ct_hip.mk call with gt; Xiao is its three pieces
        (moments of the bytes, the host SVDs, the affine map on the bytes) and ct_hip.frame_psnr."""
        import ct_hip
        k = group_u8.shape[1]
        out = self._group_buffer(group_u8, k)
        iterative_u8 = self._iterative_u8()
        if iterative_u8 is not None:
            # one draw per frame in frame order, like forward()'s loop: a seeded np.random gives the per-frame route's matrices
            from methods.iterative import draw_group_rotations
            iterative_u8(group_u8[0], group_u8[1], draw_group_rotations(k), input_f32=True, out=out, gt=group_u8[2], psnr_out=psnr_out)
            return out
        if self.func_spec == MK_SPEC:
            ct_hip.mk(group_u8[0], group_u8[1], out=out, gt=group_u8[2], psnr_out=psnr_out)
        elif self.func_spec == XIAO_SPEC:
            self.func_cuda(group_u8[0], group_u8[1], out=out)
            psnr_out.copy_(ct_hip.frame_psnr(out.clamp(0, 1), group_u8[2].float() / 255))
        else:
            ct_hip.reinhard_persist(group_u8[0], group_u8[1], gt=group_u8[2], out=out, psnr_out=psnr_out)
        return out

    def test_group_metrics(self, group_u8, table):
        """group_u8 as for test_group; table: float64 [k, 4] rows of the caller's table in METRICS order (PSNR, SSIM, FSIM, iCID).
        test_group as it is, into a [k, 2] record; then the requested columns from that record and from ct_hip.frame_ssim_hwc /
        frame_fsim_hwc / frame_icid_hwc on test_group's float32 result (clamped as it is read) and the ground-truth bytes
        group_u8[2].  Columns that were not requested become NaN.  No torch kernel between the calls but the column copies, no host
        synchronisation.  Returns test_group's result."""
        import ct_hip
        k = group_u8.shape[1]
        rec = torch.empty((k, 2), dtype=torch.float64, device=group_u8.device)
        out = self.test_group(group_u8, rec)
        gt = group_u8[2]
        table.fill_(float("nan"))
        if "psnr" in self.metrics:
            table[:, 0].copy_(rec[:, 1])
        for col, name, fn in ((1, "ssim", ct_hip.frame_ssim_hwc), (2, "fsim", ct_hip.frame_fsim_hwc)):
            if name in self.metrics:
                table[:, col].copy_(fn(out, gt))
        if "icid" in self.metrics:
            table[:, 3].copy_(ct_hip.frame_icid_hwc(out, gt, **self._icid_options()))
        return out

    def predict_group(self, group_u8):
        """group_u8 as for test_group ([2 or 3 roles: target, reference(, gt)][k][H][W][3], gt is not read) -> the corrected frames,
        float32 [k][H][W][3], from ONE asynchronous call; the buffer is reused by the next call (stream order keeps a reader
        on the same stream safe).  `utils.cli predict` packs them to bytes with ct_hip.pack_u8.  byte_groups (MK, Xiao): the
        corrected frames as bytes already, uint8 [k][H][W][3], freshly allocated (the writer holds them until their download)."""
        import ct_hip
        k = group_u8.shape[1]
        iterative_u8 = self._iterative_u8()
        if iterative_u8 is not None:
            from methods.iterative import draw_group_rotations
            return iterative_u8(group_u8[0], group_u8[1], draw_group_rotations(k), input_f32=True, out_dtype=torch.uint8)
        if self.func_spec != REINHARD_SPEC:
            return self.func_cuda(group_u8[0], group_u8[1], out_dtype=torch.uint8)
        return ct_hip.reinhard_persist(group_u8[0], group_u8[1], out=self._group_buffer(group_u8, k))

    def forward(self, batch):
        target, reference = batch["target"], batch["reference"]
        if self.func_cuda is not None and target.is_cuda:
            # [B,3,H,W] -> HWC on the device; one call per sample like the reference's loop (so that e.g. IDT draws
            # fresh rotations per sample exactly as methods/__init__.py:20-25 + iterative.py:32 do)
            t = target.permute(0, 2, 3, 1).contiguous()
            r = reference.permute(0, 2, 3, 1).contiguous()
            out = torch.stack([self.func_cuda(a, b) for a, b in zip(t, r)])
            return out.float().permute(0, 3, 1, 2)
        outputs = []
        for t, r in zip(target, reference):
            t = t.permute(1, 2, 0).detach().cpu().numpy()
            r = r.permute(1, 2, 0).detach().cpu().numpy()
            outputs.append(torch.from_numpy(self.func(t, r)).float().permute(2, 0, 1))
        return torch.stack(outputs).to(target.device)

    VIEWS = ("corrected", "chess", "rgbmse")

    @torch.no_grad()
    def views(self, batch, names=None):
        """Diagnostic images of one batch as an ordered dict of uint8 [B,H,W,3] device tensors: `corrected` =
        pack_u8(forward(batch).clamp(0, 1)), and with batch["gt"] `chess` = pack_u8(chess_mix(gt, corrected)) and `rgbmse` =
        pack_u8(rgbmse_view(gt, corrected)).  One forward serves every view; each is bitwise what those public calls give one after
        the other.  names: a subset (sequence or comma-separated string); `rgbssim`, `labmse`, `abmse` = pack_u8(<name>_view(gt,
        corrected)) come only when named (methods.EXTRA_VIEWS).  GPU only."""
        gt = batch.get("gt")
        names = select_views(self.VIEWS, names, gt is not None)
        corrected = self(batch).clamp(0, 1).float().contiguous()
        if gt is not None:
            gt = gt.to(corrected.device).float().contiguous()
        return {n: gt_views(n, corrected, gt) for n in names}

    def test_step(self, batch, batch_idx=0, dataloader_idx=0):
        result = self(batch).clamp(0, 1)
        gt = batch["gt"].to(result.device)
        out = {}
        fns = {"psnr": ("Test PSNR", psnr), "ssim": ("Test SSIM", ssim), "fsim": ("Test FSIM", fsim),
               "icid": ("Test iCID", lambda x, y: icid(x, y, **self._icid_options()))}
        for m in self.metrics:
            if m == "psnr" or result.is_cuda:        # SSIM / FSIM / iCID exist on the GPU only
                out[fns[m][0]] = fns[m][1](result, gt)
        return out
