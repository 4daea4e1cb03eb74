#!/usr/bin/env python3
"""Golden vectors for the diagnostic views by RUNNING the reference's utils/visualizations.py and utils/flow_viz.py (build
container only):

    python3 -B tests/golden/make_golden_views.py <reference root>

utils/visualizations.py imports kornia.metrics.ssim and kornia.color.rgb_to_lab, both absent offline and both used only by the
three functions this project does not build (rgbssim, labmse, abmse): empty stand-in modules whose two names raise let the file
import; chess_mix, minmaxscale and rgbmse run as written.  flow_viz.py needs nothing but numpy and PIL.

The inputs come from tests/views_common.py (integer arithmetic and IEEE + - * /: the same bits everywhere), so the file holds only
their digests and the reference's outputs.  Only data is written."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from tests import views_common as vc  # noqa: E402


def _absent(*_a, **_k):
    raise NotImplementedError("kornia is not part of this stack")


def load(root, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    root = sys.argv[1]
    for name in ("kornia", "kornia.metrics", "kornia.color"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["kornia.metrics"].ssim = _absent
    sys.modules["kornia.color"].rgb_to_lab = _absent
    viz = load(root, "utils/visualizations.py", "ref_visualizations")
    fv = load(root, "utils/flow_viz.py", "ref_flow_viz")
    fix = {}
    # chess_mix: the inputs hold integers, the outputs are stored as such
    x, y = vc.chess_inputs()
    fix["chess/in_sha1"] = vc.digest(x, y)
    for size in (25, 7):
        got = viz.chess_mix(torch.from_numpy(x), torch.from_numpy(y), size=size).numpy()
        assert np.array_equal(got, got.astype(np.int16).astype(np.float32))
        fix["chess/out_%d" % size] = got.astype(np.int16)
    # rgbmse: channel 0 only (the reference leaves the other two at zero, asserted here)
    x, y = vc.rgbmse_inputs()
    fix["rgbmse/in_sha1"] = vc.digest(x, y)
    got = viz.rgbmse(torch.from_numpy(x), torch.from_numpy(y)).numpy()
    assert got.dtype == np.float32 and not got[:, 1:].any()
    fix["rgbmse/out_ch0"] = got[:, 0]
    # flow_to_image, through the tensor entry the models' logging calls; it zeroes unknown pixels of its argument in place
    for case in vc.FLOW_CASES:
        flow = vc.flow_input(case)
        fix["flow/%s/in_sha1" % case] = vc.digest(flow)
        img = fv.flow_tensor_to_image(torch.from_numpy(flow.copy()))
        assert img.dtype == np.uint8 and img.shape == (3,) + flow.shape[1:]
        fix["flow/%s/out" % case] = np.ascontiguousarray(img.transpose(1, 2, 0))
        # the reference against itself, inputs perturbed by 2^-22 relative: how many pixels a last-bit difference can move
        pert = (flow.astype(np.float64) * (1 + 2.0 ** -22 * (2.0 * vc.uniform(flow.shape, 99) - 1))).astype(np.float32)
        img2 = fv.flow_tensor_to_image(torch.from_numpy(pert)).transpose(1, 2, 0)
        fix["flow/%s/perturbed_share" % case] = np.float64((img2 != fix["flow/%s/out" % case]).any(axis=2).mean())
        print(case, flow.shape, "perturbed share %.2e" % fix["flow/%s/perturbed_share" % case])
    path = os.path.join(OUT, "views.npz")
    np.savez_compressed(path, numpy=np.__version__, torch=torch.__version__, **fix)
    print("wrote views.npz: %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
