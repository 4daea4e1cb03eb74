"""The reference's utils/icid.py on the device: `icid(img1, img2, intent="perceptual", omit_maps67=False, downsampling=True)`, the
improved colour-image-difference metric (Preiss, Fernandes, Urban 2014), with the reference's signature and the reference's
quantity -- ONE number for the batch, 1 - mean over the batch and the map pixels of the product of the maps.  The maps are
computed by ct_hip.frame_icid (csrc/metrics.hip: float32 arithmetic like the reference's torch code, float64 sums), one value per
frame; the frames of a batch have one size, so the mean of those values IS the mean over batch and pixels.  No CPU path.

kornia's `rgb_to_lab` and torchvision's `gaussian_blur`, on which the reference's file rests, are third-party code that is not
part of this stack: their arithmetic is restated on the device from the published sources (parity unpinned for those two calls);
every line of the reference's own icid() is pinned by tests/golden/icid.npz and icid_options.npz, runs of that file."""
import ct_hip


def icid(img1, img2, intent="perceptual", omit_maps67=False, downsampling=True):
    """utils/icid.py:28-152 on CUDA tensors [B,3,H,W] (or one [3,H,W] frame) with values in [0, 1] -> a 0-dim float64 tensor on
    their device.  intent: 'perceptual', 'hue-preserving' or 'chromatic' (anything else: the reference's ValueError, before the
    tensors are looked at); omit_maps67: drop chroma contrast and chroma structure; downsampling=False: the maps at the frames'
    own size instead of after the bilinear resize by 1 / max(1, round(min(H, W) / 256)).  Host tensors raise ct_hip.CtHipError."""
    ct_hip.icid_intent(intent)
    if img1.dim() == 3 and img2.dim() == 3:
        img1, img2 = img1.unsqueeze(0), img2.unsqueeze(0)
    per_frame = ct_hip.frame_icid(img1.float().contiguous(), img2.float().contiguous(), intent=intent, omit_maps67=omit_maps67,
                                  downsampling=downsampling)
    return per_frame.mean()
