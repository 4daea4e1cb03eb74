"""Drop-in for the reference's pasmnet/losses.py (the three parallax-attention losses of methods/dcmcs3di.py:75-77) on the GPU.

Same names, argument structure and batch semantics as the reference: every loss is ONE sum over the batch divided by ONE count over
the batch, and masked_l1_loss divides by the sum of the UNBROADCAST mask (the photometric numerator runs over 3 channels, the cycle
numerator over W columns, both are divided by the number of valid pixels only).  A count of zero gives the reference's 0 / 0 = NaN
(an all-false mask, H == 1 for the vertical smoothness term, W == 1 for the diagonal one).

The sums come from csrc/pam_losses.hip through ct_hip.pam_map_sweep / ct_hip.pam_cycle_l1 / ct_hip.masked_l1_sums: terms in float32
as torch forms them, added in float64 in a fixed order.  Each loss is a float64 scalar on the device, returned without
synchronising.  Inputs are float32 CUDA tensors (masks: bool or 0/1 float); there is no CPU path (ct_hip.CtHipError) and no autograd.

loss_pam_cycle_from_att(att, valid_mask) is loss_pam_cycle(att_cycle, valid_mask) without the two [B,H,W,W] cycle maps: the
products att_r2l @ att_l2r and att_l2r @ att_r2l run on the exact-f32 MFMA and go straight into the sum.
"""
import ct_hip


def _ratio(num, count):
    """per-image sums and counts -> one sum over the batch / one count over the batch (float64; 0 / 0 = NaN)"""
    count = count.sum()
    return num.sum() / (count if count.is_cuda else float(count))


def masked_l1_loss(x, y, mask):
    """sum(|x - y| * mask) / sum(mask) for the layouts the reference calls it with: x, y [B,3,H,W] with mask [B,1,H,W], or
    x, y [B,H,W,W] with mask [B,H,W,1]"""
    return _ratio(*ct_hip.masked_l1_sums(x, y, mask))


def loss_pam_photometric(img_left, img_right, att, valid_mask):
    att_right2left, att_left2right = att
    valid_mask_left, valid_mask_right = valid_mask
    left = ct_hip.pam_map_sweep(att_right2left, src=img_right, dst=img_left, mask=valid_mask_left)
    right = ct_hip.pam_map_sweep(att_left2right, src=img_left, dst=img_right, mask=valid_mask_right)
    return _ratio(left["photometric"], left["mask_sum"]) + _ratio(right["photometric"], right["mask_sum"])


def loss_pam_cycle(att_cycle, valid_mask):
    att_left2right2left, att_right2left2right = att_cycle
    valid_mask_left, valid_mask_right = valid_mask
    left = ct_hip.pam_map_sweep(att_left2right2left, mask=valid_mask_left)
    right = ct_hip.pam_map_sweep(att_right2left2right, mask=valid_mask_right)
    return _ratio(left["identity"], left["mask_sum"]) + _ratio(right["identity"], right["mask_sum"])


def loss_pam_cycle_from_att(att, valid_mask):
    """loss_pam_cycle((att_right2left @ att_left2right, att_left2right @ att_right2left), valid_mask), the cycle maps of the
    reference's pasmnet/utils.py output(), without building them"""
    att_right2left, att_left2right = att
    valid_mask_left, valid_mask_right = valid_mask
    return (_ratio(*ct_hip.pam_cycle_l1(att_right2left, att_left2right, valid_mask_left)) +
            _ratio(*ct_hip.pam_cycle_l1(att_left2right, att_right2left, valid_mask_right)))


def loss_pam_smoothness(att):
    total = None
    for a in att:                                            # right-to-left, then left-to-right; vertical then diagonal, as the reference adds them
        s = ct_hip.pam_map_sweep(a)
        for name in ("vertical", "diagonal"):
            term = _ratio(s[name], s[name + "_count"])
            total = term if total is None else total + term
    return total
