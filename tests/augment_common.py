"""What the augmentation, loss and `validate` tests share: CPU restatements of torchvision's adjust_sharpness (from its published
_functional_tensor.py: adjust_sharpness, _blurred_degenerate_image, _cast_squeeze_out -- parity unpinned, torchvision is absent
offline), of the reference's crop / flip geometry and chain (utils/data.py:25-84) on top of oracle/distort.py, and of the step losses
in the dtype of their inputs.  Not product code."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import distort as od
from tests import errmaps_common as ec

KINDS = ("identity", "brightness", "contrast", "saturation", "hue", "gamma", "sharpness")


# ---- torchvision.transforms.functional.adjust_sharpness on a uint8 [3,H,W] tensor --------------------------------------------------
def blurred_degenerate_image(img):
    kernel = torch.ones((3, 3), dtype=torch.float32)
    kernel[1, 1] = 5.0
    kernel /= kernel.sum()
    kernel = kernel.expand(img.shape[-3], 1, 3, 3)
    tmp = F.conv2d(img.to(torch.float32)[None], kernel, groups=img.shape[-3])[0]
    tmp = torch.round(tmp).to(img.dtype)                     # _cast_squeeze_out for an integer image
    result = img.clone()
    result[..., 1:-1, 1:-1] = tmp
    return result


def adjust_sharpness(img, factor):
    if factor < 0:
        raise ValueError("sharpness_factor (%s) is not non-negative." % factor)
    if img.shape[-1] <= 2 or img.shape[-2] <= 2:
        return img
    return od._blend(img, blurred_degenerate_image(img), factor)


def apply_op(img, kind, param):
    kind = KINDS[kind] if isinstance(kind, int) else kind
    return adjust_sharpness(img, float(param)) if kind == "sharpness" else od.apply(img, kind, param)


def apply_chain(img, ops):
    for kind, param in ops:
        img = apply_op(img, kind, param)
    return img


# ---- utils/data.py:69-84 for one sample, uint8 in, uint8 out -----------------------------------------------------------------------
def geometry(gt, ref, p, crop):
    """(new gt, new reference) uint8 [3,ch,cw] of a source pair [3,H,W] under the draws p"""
    ch, cw = crop
    g = gt[:, p["top"]:p["top"] + ch, p["left"]:p["left"] + cw]
    r = ref[:, p["top"]:p["top"] + ch, p["left"]:p["left"] + cw]
    if p["swap_hflip"]:
        g, r = r.flip(-1), g.flip(-1)
    if p["vflip"]:
        g, r = g.flip(-2), r.flip(-2)
    return g.contiguous(), r.contiguous()


def sample(gt, ref, p, crop):
    g, r = geometry(gt, ref, p, crop)
    return g, r, apply_chain(g, p.get("ops", ()))


def params(top=0, left=0, swap_hflip=False, vflip=False, ops=()):
    return {"top": top, "left": left, "swap_hflip": swap_hflip, "vflip": vflip, "ops": list(ops)}


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def textured_u8(shape, seed):
    """the image recipe of tests/test_data_path.py: a smooth texture plus noise, with black, white and pure red patches; [3,H,W] or
    [n,3,H,W] uint8"""
    g = torch.Generator().manual_seed(seed)
    lead, (h, w) = tuple(shape[:-2]), shape[-2:]
    n = int(np.prod(lead[:-1])) if len(lead) > 1 else 1
    coarse = torch.randint(0, 256, (n, 3, max(h // 22, 2), max(w // 28, 2)), generator=g).float()
    img = F.interpolate(coarse, size=(h, w), mode="bilinear", align_corners=True)
    img = (img + torch.randint(-20, 21, img.shape, generator=g)).clamp(0, 255).to(torch.uint8)
    if h >= 12 and w >= 4:
        img[:, :, :4, :4] = 0
        img[:, :, 4:8, :4] = 255
        img[:, :, 8:12, :4] = torch.tensor([255, 0, 0], dtype=torch.uint8).view(3, 1, 1)
    return img.reshape(tuple(shape))


# ---- the step losses -------------------------------------------------------------------------------------------------------------------
def losses(a, b):
    """[B,3] per frame: F.l1_loss, F.mse_loss and kornia.losses.ssim_loss(window_size=11, reduction="mean") -- mean(clamp((1 -
    ssim_map) / 2, 0, 1)), kornia/losses/ssim.py restated over tests/errmaps_common.kornia_ssim -- in the dtype of a and b"""
    d = a - b
    ssim_map = ec.kornia_ssim(a, b, window_size=11)
    loss_map = torch.clamp((1.0 - ssim_map) / 2, min=0, max=1)
    return torch.stack([d.abs().mean(dim=(1, 2, 3)), (d * d).mean(dim=(1, 2, 3)), loss_map.mean(dim=(1, 2, 3))], dim=1)
