#!/usr/bin/env python3
"""Golden vectors for the error maps rgbssim, labmse and abmse by RUNNING the reference's utils/visualizations.py (build container
only):

    python3 -B tests/golden/make_golden_errmaps.py <reference root>

utils/visualizations.py imports kornia.metrics.ssim and kornia.color.rgb_to_lab, both absent offline.  They are stood in by
tests.errmaps_common.kornia_ssim and oracle.metrics.rgb_to_lab (restatements of those two third-party functions from their published
sources, "parity unpinned" for them); every line of the reference's rgbssim, labmse, abmse and minmaxscale themselves
(utils/visualizations.py:24-60) is executed as written, once on float64 and once on float32 inputs, on the CPU.

The inputs come from tests/errmaps_common.py (integer arithmetic and IEEE + - * /: the same bits everywhere), so the file holds only
their digests and channel 0 of the reference's outputs (it leaves the other two at zero, asserted here).  Only data is written."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from oracle import metrics as om  # noqa: E402
from tests import errmaps_common as ec  # noqa: E402
from tests import views_common as vc  # noqa: E402


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    for name in ("kornia", "kornia.metrics", "kornia.color"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["kornia.metrics"].ssim = ec.kornia_ssim
    sys.modules["kornia.color"].rgb_to_lab = om.rgb_to_lab
    spec = importlib.util.spec_from_file_location("ref_visualizations", os.path.join(sys.argv[1], "utils/visualizations.py"))
    viz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(viz)
    fix = {}
    for shape in ec.SHAPES:
        x, y = ec.inputs(shape)
        assert x.dtype == np.float32 and x.min() >= 0 and x.max() <= 1 and y.min() >= 0 and y.max() <= 1
        fix["%s/in_sha1" % ec.tag(shape)] = vc.digest(x, y)
        for name in ec.MAPS:
            fn = getattr(viz, name)
            r64 = fn(torch.from_numpy(x).double(), torch.from_numpy(y).double()).numpy()
            r32 = fn(torch.from_numpy(x), torch.from_numpy(y)).numpy()
            assert r64.dtype == np.float64 and r32.dtype == np.float32 and not r64[:, 1:].any() and not r32[:, 1:].any()
            fix["%s/%s/f64" % (ec.tag(shape), name)], fix["%s/%s/f32" % (ec.tag(shape), name)] = r64[:, 0], r32[:, 0]
            m = ec.unscaled(name, torch.from_numpy(x).double(), torch.from_numpy(y).double())
            span = float((m.amax(dim=(-1, -2)) - m.amin(dim=(-1, -2))).min())
            e32 = np.abs(r32[:, 0] - r64[:, 0])
            print("%-10s %-8s unscaled range >= %.3g   float32 run: rms %.2e max %.2e" % (ec.tag(shape), name, span, np.sqrt((e32 ** 2).mean()), e32.max()))
            assert span > 1e-2
    path = os.path.join(OUT, "errmaps.npz")
    np.savez_compressed(path, numpy=np.__version__, torch=torch.__version__, **fix)
    print("wrote errmaps.npz: %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
