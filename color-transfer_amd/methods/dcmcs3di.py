"""Deep Color Mismatch Correction in Stereoscopic 3D Images (Croci et al. 2021) -- MI355X drop-in
for the FORWARD pass of the reference's methods/dcmcs3di.py:29-66.

Same constructor arguments, parameter names/shapes (reference checkpoints `load_state_dict`
strictly) and `forward(left, right, inference)` return structure.  The ResB convolutions run in
ct_conv3x3_ws16_f32 (weights stationary in registers, two fp16 pieces per float32 operand), the
other convolutions in ct_conv2d_split_f32 (three bf16 pieces) -- or all of them in ct_conv2d_f32
(exact-f32 MFMA) in `exact` mode; the parallax attention in the streaming kernels behind
ct_hip.pam_streaming (ct_pam_attend_f32 / ct_pam_valid_f32 when the [B,H,W,W] maps are wanted); torch
only allocates tensors.  `step(batch)` gives what the reference's step logs for a batch (dcmcs3di.py:68-92), the three
parallax-attention losses from pasmnet.losses (csrc/pam_losses.hip), without autograd; training itself is out of scope.
`disparity(left, right)` gives the left view's disparity of the reference's log_images (dcmcs3di.py:126,
pasmnet/utils.py:55-105) from the streaming attention, at any width and without a [B,H,W,W] map.
`forward_scaled(left, right, scale_factor)` is the calling convention of the reference's demo notebook (cell 24): bicubic down, the
forward at the reduced size, bicubic back up (ct_hip.bicubic_resize).
`views(left, right, gt)` gives the image panel of the reference's log_images (dcmcs3di.py:116-144) as uint8 frames on the device.
No CPU fallback.
"""
import torch

import ct_hip
from pasmnet.attention import PAB
from pasmnet.backbone import ResB, conv_forward, conv_forward_rows, resb_forward


def sequential_forward(seq, x):
    for m in seq:
        if isinstance(m, ResB):
            x = resb_forward(m, x)
        elif isinstance(m, torch.nn.Conv2d):
            x = conv_forward(m, x)
        else:
            raise TypeError("unexpected module %r" % (m,))
    return x


class DCMCS3DI(torch.nn.Module):
    VIEWS = ("corrected", "chess", "rgbmse", "disparity", "warped_right", "occlusions")

    def __init__(self, extraction_layers=18, transfer_layers=6, channels=64):
        super().__init__()
        self.hparams = type("HParams", (), dict(extraction_layers=extraction_layers, transfer_layers=transfer_layers,
                                                channels=channels))()
        # the reference takes any width (dcmcs3di.py:30-51).  64 (configs/dcmcs3di.yaml) runs on the kernels built for it (Winograd ResB
        # convolutions, streaming attention at any image width); other widths take the generic paths: tile convolutions, and the
        # LDS-tile attention (images up to ~1000 columns).  The three-source 1x1 convolution of transfer[0] wants channel counts that are
        # multiples of 16; the attention kernels contract over 64 query / key channels (narrower ones are zero-padded, see forward_parts).
        if channels % 16 or not 16 <= channels <= 64:
            raise ValueError("channels must be 16, 32, 48 or 64 (the reference's configs/dcmcs3di.yaml uses 64)")
        # construction order == reference (dcmcs3di.py:41-51): torch.manual_seed(s) gives the same init
        self.extraction = torch.nn.Sequential(torch.nn.Conv2d(3, channels, kernel_size=3, padding=1))
        for _ in range(extraction_layers):
            self.extraction.append(ResB(channels, channels))
        self.matcher = PAB(channels)
        self.transfer = torch.nn.Sequential(torch.nn.Conv2d(2 * channels + 1, channels, kernel_size=1))
        for _ in range(transfer_layers):
            self.transfer.append(ResB(channels, channels))
        self.transfer.append(torch.nn.Conv2d(channels, channels // 2, kernel_size=3, padding=1))
        self.transfer.append(torch.nn.Conv2d(channels // 2, 3, kernel_size=3, padding=1))

    @torch.no_grad()
    def forward_parts(self, left, right, want_att=False, want_valid_right=False, want_disp=False):
        """The forward pass with its intermediates (used by forward() and by the parity tests).  want_disp adds disp_ini_left
        (i - E[j] under att_r2l) and disp_left (regress_disp's occlusion fill of it under valid_left), [B,1,H,W] float32; every
        other part is bitwise the same as without it."""
        if not left.is_cuda:
            raise ct_hip.CtHipError("DCMCS3DI runs on the GPU only (no CPU fallback)")
        left = left.contiguous().float()
        right = right.contiguous().float()
        B = left.shape[0]
        both = torch.cat([left, right], dim=0)
        fea = sequential_forward(self.extraction, both)                    # dcmcs3di.py:54-55
        head = resb_forward(self.matcher.head, fea)                        # attention.py:35-36
        fea_left, fea_right = fea[:B], fea[B:]
        H, W = left.shape[2], left.shape[3]
        tile_path = want_att or self.hparams.channels != 64      # the streaming kernels are built for 64 channels
        if tile_path or want_valid_right:
            q = conv_forward(self.matcher.query, head)                     # attention.py:39,44
            k = conv_forward(self.matcher.key, head)                       # attention.py:40,45
            c = q.shape[1]
            if c != 64:
                # the attention kernels contract over 64 channels and scale the scores by 1 / 64; the reference scales by 1 / c
                # (attention.py:41): zero channels add nothing to a score, and q * (64 / c) puts the scale right
                q64, k64 = q.new_zeros((q.shape[0], 64) + tuple(q.shape[2:])), k.new_zeros((k.shape[0], 64) + tuple(k.shape[2:]))
                q64[:, :c] = q * (64.0 / c)
                k64[:, :c] = k
                q, k = q64, k64
        if tile_path:
            # the [B,H,W,W] maps are wanted (or the width is not 64): LDS-tile kernels that can write them out
            v = conv_forward(self.matcher.value, fea_right)                # dcmcs3di.py:58
            # right-to-left: Q(left) . K(right)
            fea_warped, warped_rgb, att_r2l = ct_hip.pam_attend(q[:B].contiguous(), k[B:].contiguous(), v, right, want_att=want_att)
            # left-to-right softmax, column sums -> valid mask of the LEFT view (utils.py:31,34-35)
            valid_left, colsum_left, att_l2r = ct_hip.pam_valid(q[B:].contiguous(), k[:B].contiguous(), want_att=want_att)
            if want_disp and want_att:
                # one pass over the materialised map; an all-valid mask leaves the unfilled disparity
                disp_ini_left = ct_hip.regress_disp(att_r2l, torch.ones_like(valid_left))
            elif want_disp:
                # the index-only streaming pass on the zero-padded 64-channel query / key rows (zero channels add nothing to a score)
                disp_ini_left = ct_hip.attention_rows64_index(ct_hip.nchw_to_rows(q[:B]), ct_hip.nchw_to_rows(k[B:]), B, H, W)
        else:
            # streaming (online-softmax) kernels: no score tile in LDS, any width, K/V rows fetched with 16-byte loads.  They read
            # token rows [B*H, W, C]; the three 1x1 convolutions store that layout from their epilogues (no NCHW q/k/v, no
            # transposes)
            att_r2l = att_l2r = None
            qt = conv_forward_rows(self.matcher.query, head)               # [2B*H, W, 64]: Q(left) rows then Q(right) rows
            kt = conv_forward_rows(self.matcher.key, head)
            vt = conv_forward_rows(self.matcher.value, fea_right, channels=96)
            n = B * H
            res = ct_hip.pam_streaming_rows(qt[:n], kt[n:], vt, right, qt[n:], kt[:n], want_disp=want_disp)
            fea_warped, warped_rgb, valid_left, colsum_left = res[:4]
            if want_disp:
                disp_ini_left = res[4]                                     # from the attend pass itself
        # dcmcs3di.py:59,47: transfer[0] (1x1, 129 -> 64) reads cat([fea_left, fea_warped, valid_left]) straight from its
        # three tensors (a three-source K loop in ct_conv2d_split_f32; the 129-channel tensor is never built)
        x = conv_forward(self.transfer[0], fea_left, x2=fea_warped, x3=valid_left)
        n_t = len(self.transfer)
        for i in range(1, n_t - 1):
            m = self.transfer[i]
            x = resb_forward(m, x) if isinstance(m, ResB) else conv_forward(m, x)
        pre_clamp = conv_forward(self.transfer[n_t - 1], x)
        parts = dict(fea_left=fea_left, fea_right=fea_right, fea_warped=fea_warped, warped_rgb=warped_rgb,
                     att_r2l=att_r2l, att_l2r=att_l2r, valid_left=valid_left, colsum_left=colsum_left,
                     pre_clamp=pre_clamp, corrected=pre_clamp.clamp(min=0, max=1))
        if want_valid_right:
            parts["valid_right"], parts["colsum_right"], _ = ct_hip.pam_valid(q[:B], k[B:])
        if want_disp:
            parts["disp_ini_left"] = disp_ini_left
            parts["disp_left"] = ct_hip.pam_disp_fill(disp_ini_left, valid_left)
        return parts

    @torch.no_grad()
    def disparity(self, left, right):
        """Disparity of the left view (the reference's regress_disp(att_right2left, valid_mask_left), dcmcs3di.py:126) at
        inference: (disp_left [B,1,H,W] float32, valid_left [B,1,H,W] bool).  Streaming kernels only -- the feature extractor,
        the attention head, the index-only attention pass and the valid-mask passes -- so any width, no [B,H,W,W] tensor and no
        colour-transfer half.  For 16 / 32 / 48 channels the query / key are zero-padded to 64 as in forward_parts."""
        if not left.is_cuda:
            raise ct_hip.CtHipError("DCMCS3DI runs on the GPU only (no CPU fallback)")
        left = left.contiguous().float()
        right = right.contiguous().float()
        B, H, W = left.shape[0], left.shape[2], left.shape[3]
        fea = sequential_forward(self.extraction, torch.cat([left, right], dim=0))
        head = resb_forward(self.matcher.head, fea)
        if self.hparams.channels == 64:
            qt = conv_forward_rows(self.matcher.query, head)               # [2B*H, W, 64]
            kt = conv_forward_rows(self.matcher.key, head)
        else:
            q = conv_forward(self.matcher.query, head)
            k = conv_forward(self.matcher.key, head)
            c = q.shape[1]
            q64, k64 = q.new_zeros((q.shape[0], 64) + tuple(q.shape[2:])), k.new_zeros((k.shape[0], 64) + tuple(k.shape[2:]))
            q64[:, :c] = q * (64.0 / c)
            k64[:, :c] = k
            qt, kt = ct_hip.nchw_to_rows(q64), ct_hip.nchw_to_rows(k64)
        n = B * H
        disp_ini = ct_hip.attention_rows64_index(qt[:n], kt[n:], B, H, W)   # Q(left) . K(right)
        valid, _ = ct_hip.pam_valid_rows(qt[n:], kt[:n], B, H, W)         # Q(right) . K(left) column sums
        return ct_hip.pam_disp_fill(disp_ini, valid), valid > 0.5

    def forward(self, left, right, inference=False, return_attention=None):
        """Same return structure as the reference (dcmcs3di.py:61-66):
        (corrected, ((att_r2l, att_l2r), (cycle_l, cycle_r), (valid_left, valid_right), warp(right, att_r2l))).
        The [B,H,W,W] attention maps (15.9 GB each at 1080p) are materialised only when
        `return_attention` is true (default: only in training mode, inference=False)."""
        want_att = (not inference) if return_attention is None else bool(return_attention)
        p = self.forward_parts(left, right, want_att=want_att, want_valid_right=not inference)
        valid_left = p["valid_left"] > 0.5
        if inference:
            att_cycle = (None, None)
            valid = (valid_left, None)
        else:
            att_cycle = (torch.matmul(p["att_r2l"], p["att_l2r"]), torch.matmul(p["att_l2r"], p["att_r2l"])) \
                if want_att else (None, None)
            valid = (valid_left, p["valid_right"] > 0.5)
        return p["corrected"], ((p["att_r2l"], p["att_l2r"]), att_cycle, valid, p["warped_rgb"])

    @torch.no_grad()
    def views(self, left, right, gt=None, names=None):
        """The image panel of the reference's log_images (dcmcs3di.py:116-144) at inference, as an ordered dict of uint8 [B,H,W,3]
        device tensors (what utils.writer.FrameWriter takes):
            corrected     pack_u8 of the corrected left view
            chess         pack_u8(chess_mix(gt, corrected))                      needs gt
            rgbmse        pack_u8(rgbmse_view(gt, corrected))                    needs gt
            disparity     pack_u8(gray_view(disp_left)), forward_parts(want_disp=True)'s filled disparity, min-max scaled per frame
            warped_right  pack_u8(warped_rgb), the right view under the parallax attention
            occlusions    255 where valid_left is false
            rgbssim, labmse, abmse    pack_u8(<name>_view(gt, corrected)): only when named (methods.EXTRA_VIEWS), need gt
        names: a subset (sequence or comma-separated string; default: all, without gt those that need none).  Unknown names and
        a gt view without gt raise ValueError.  ONE forward serves every view, and each is bitwise what the public pieces named
        above give when called one after the other."""
        from methods import gt_views, mask_view, select_views
        names = select_views(self.VIEWS, names, gt is not None)
        p = self.forward_parts(left, right, want_disp="disparity" in names)
        corrected = p["corrected"]
        if gt is not None:
            gt = gt.to(corrected.device).float().contiguous()
        out = {}
        for n in names:
            if n == "disparity":
                out[n] = ct_hip.pack_u8(ct_hip.gray_view(p["disp_left"]), "chw")
            elif n == "warped_right":
                out[n] = ct_hip.pack_u8(p["warped_rgb"].contiguous(), "chw")
            elif n == "occlusions":
                out[n] = mask_view((~(p["valid_left"] > 0.5)).float())
            else:
                out[n] = gt_views(n, corrected, gt)
        return out

    @torch.no_grad()
    def forward_scaled(self, left, right, scale_factor=0.75, antialias=False):
        """Inference at a reduced size, as the reference's demo notebook runs this model (cell 24):
            target, reference = F.interpolate(., scale_factor=scale_factor, mode="bicubic")      both views, ONE launch
            result, _ = model(target, reference, inference=True)                                  the streaming path
            result = F.interpolate(result, size=(H, W), mode="bicubic")
        Returns (corrected_full [B,3,H,W] float32, valid_left_lowres [B,1,h,w] bool).  corrected_full is NOT clamped: the bicubic
        kernel overshoots [0, 1], and the notebook leaves that to whoever writes the frame.  antialias is F.interpolate's flag, for
        both resamplings (the notebook does not set it).  Bitwise what the public pieces give when called one after the other."""
        if not left.is_cuda:
            raise ct_hip.CtHipError("DCMCS3DI runs on the GPU only (no CPU fallback)")
        if left.dim() != 4 or left.shape != right.shape:
            raise ValueError("forward_scaled needs two [B,3,H,W] views of one shape")
        B, H, W = left.shape[0], left.shape[2], left.shape[3]
        both = torch.cat([left.float(), right.float()], dim=0)             # [2B,3,H,W]: one resize launch for the two views
        low = ct_hip.bicubic_resize(both, scale_factor=scale_factor, antialias=antialias)
        corrected, (_, _, (valid_left, _), _) = self.forward(low[:B], low[B:], inference=True)
        return ct_hip.bicubic_resize(corrected, size=(H, W), antialias=antialias), valid_left

    @torch.no_grad()
    def step(self, batch, prefix="Validation"):
        """The reference's step (dcmcs3di.py:68-92) for one batch {"target", "reference", "gt"} of [B,3,H,W] device tensors: what it
        logs, in its logging order and under its names without the prefix (as DMSCT.validation_step) -- `L1 Loss`, `MSE Loss`,
        `SSIM Loss` (ct_hip.frame_losses; unscaled here, dcmcs3di.py:73), `Photometric Loss`, `Cycle Loss`, `Smoothness Loss` (pasmnet.losses,
        each x 0.005), `PSNR`, `SSIM`, `FSIM`, `iCID` (batch means) -- and `loss`, the sum of the six losses that step() returns.
        float64 scalars on the device, nothing synchronises.

        The forward is the training-mode one (inference=False): forward_parts(want_att=True, want_valid_right=True), masks > 0.5.
        The cycle loss comes from the two attention maps through the fused kernel (pasmnet.losses.loss_pam_cycle_from_att), so the
        two cycle maps of forward()'s return value are never built.  Memory: the two [B,H,W,W] float32 attention maps (524 MB each
        at the training crop of configs/dcmcs3di.yaml, batch 8 of 160 x 320) plus a few KB of partial sums.

        Runs under no_grad: NO autograd is offered, the values are for logging and validation, not for a backward pass.  `prefix`
        is accepted for the reference's signature and does not change the keys."""
        from methods import fsim, icid, psnr, ssim
        from pasmnet import losses as pam
        left = batch["target"].contiguous().float()
        right = batch["reference"].to(left.device).contiguous().float()
        p = self.forward_parts(left, right, want_att=True, want_valid_right=True)
        result = p["corrected"].float().contiguous()
        gt = batch["gt"].to(result.device).float().contiguous()
        att = (p["att_r2l"], p["att_l2r"])
        valid = (p["valid_left"] > 0.5, p["valid_right"] > 0.5)
        frame, _ = ct_hip.frame_losses(result, gt)
        out = {"L1 Loss": frame[0], "MSE Loss": frame[1], "SSIM Loss": frame[2],
               "Photometric Loss": 0.005 * pam.loss_pam_photometric(left, right, att, valid),
               "Cycle Loss": 0.005 * pam.loss_pam_cycle_from_att(att, valid),
               "Smoothness Loss": 0.005 * pam.loss_pam_smoothness(att)}
        loss = out["L1 Loss"] + out["MSE Loss"] + out["SSIM Loss"] + out["Photometric Loss"] + out["Cycle Loss"] + out["Smoothness Loss"]
        for name, fn in (("PSNR", psnr), ("SSIM", ssim), ("FSIM", fsim), ("iCID", icid)):
            out[name] = fn(result, gt).mean()
        out["loss"] = loss
        return out

    VALIDATION_MISSING = ("Photometric Loss", "Cycle Loss", "Smoothness Loss")     # utils.cli validate refuses before the first frame

    def validation_step(self, batch, batch_idx=0, dataloader_idx=0):
        """dcmcs3di.py:97-98 is step(batch, "Validation").  step() above computes all of it, the three PAM losses included
        (pasmnet.losses), but `utils.cli validate` is not wired to it yet: validation_step and VALIDATION_MISSING keep refusing until it is
        """
        raise NotImplementedError("DCMCS3DI.validation_step is not wired to DCMCS3DI.step yet: step(batch) returns the reference's "
                                  "quantities, %s (pasmnet.losses: loss_pam_photometric, loss_pam_cycle, loss_pam_smoothness) "
                                  "included, but `utils.cli validate` does not call it; methods.dmsct.DMSCT validates"
                                  % ", ".join(DCMCS3DI.VALIDATION_MISSING))
