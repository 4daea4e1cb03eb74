"""The reference's utils/visualizations.py on the device: `chess_mix`, `minmaxscale` and `rgbmse` with its signatures, on float32
CUDA tensors (ct_hip.chess_mix / ct_hip.rgbmse_view / ct_hip.gray_view, csrc/views.hip).  No CPU path.

`rgbssim`, `labmse` and `abmse` are not built: they rest on kornia's `ssim` / `rgb_to_lab`, third-party code that is not part of
this stack and whose arithmetic could not be pinned; they raise NotImplementedError."""
import ct_hip


def chess_mix(x, y, size=25):
    """visualizations.py:9-21: [B,C,H,W] (or one [C,H,W] frame) -> the checkerboard of x and y"""
    if x.dim() == 3:
        return ct_hip.chess_mix(x.unsqueeze(0).contiguous(), y.unsqueeze(0).contiguous(), size)[0]
    return ct_hip.chess_mix(x.contiguous(), y.contiguous(), size)


def minmaxscale(x, dim=(-1, -2)):
    """visualizations.py:24-28 for the one use the reference makes of it: the last two axes of a [B,H,W] tensor"""
    if x.dim() != 3 or tuple(sorted(d % 3 for d in dim)) != (1, 2):
        raise NotImplementedError("minmaxscale on the device scales [B,H,W] planes over their last two axes (dim=(-1, -2))")
    return ct_hip.gray_view(x.unsqueeze(1).contiguous())[:, 0]


def rgbmse(x, y):
    """visualizations.py:31-36: [B,3,H,W] -> the min-max scaled squared error in channel 0, zeros in channels 1 and 2"""
    return ct_hip.rgbmse_view(x.contiguous(), y.contiguous())


def _needs_kornia(name, what):
    def fn(x, y):
        raise NotImplementedError("%s needs kornia's %s, which this stack does not carry; rgbmse is the error map built here" % (name, what))
    fn.__name__ = name
    return fn


labmse = _needs_kornia("labmse", "rgb_to_lab")
abmse = _needs_kornia("abmse", "rgb_to_lab")
rgbssim = _needs_kornia("rgbssim", "ssim")
