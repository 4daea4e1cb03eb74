"""The reference's utils/visualizations.py on the device: `chess_mix`, `minmaxscale`, `rgbmse`, `rgbssim`, `labmse` and `abmse` with
its signatures, on float32 CUDA tensors (ct_hip.chess_mix / rgbmse_view / gray_view, csrc/views.hip; ct_hip.rgbssim_view /
labmse_view / abmse_view, csrc/errmaps.hip).  No CPU path.

`rgbssim`, `labmse` and `abmse` rest on kornia's `ssim` / `rgb_to_lab`, third-party code that is not part of this stack: on the
device its arithmetic is restated from the published source (parity unpinned for those two calls; the reference's own lines are
pinned by tests/golden/errmaps.npz).  On the host the arithmetic would be kornia's itself: host tensors raise
NotImplementedError."""
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


def _on_device(name, what, view):
    def fn(x, y):
        if not x.is_cuda:
            raise NotImplementedError("%s on host tensors needs kornia's %s, which this stack does not carry; on CUDA tensors it runs "
                                      "as ct_hip.%s" % (name, what, view.__name__))
        return view(x.contiguous(), y.contiguous())
    fn.__name__ = name
    fn.__doc__ = "visualizations.py (%s): [B,3,H,W] CUDA tensors -> ct_hip.%s" % (name, view.__name__)
    return fn


labmse = _on_device("labmse", "rgb_to_lab", ct_hip.labmse_view)
abmse = _on_device("abmse", "rgb_to_lab", ct_hip.abmse_view)
rgbssim = _on_device("rgbssim", "ssim", ct_hip.rgbssim_view)
