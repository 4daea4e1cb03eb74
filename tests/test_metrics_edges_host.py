"""The frame metrics at their edges, host side (no GPU): the pooling factor and the sizes it gives against the oracle's, the
workspace against both tile grids, and the resolving power of the probes that tests/test_metrics_edges_gpu.py holds the kernels
to -- an oracle whose SSIM / iCID map is wrong in one edge row, edge column or seam row must leave the tolerance by 10x."""
import ctypes
import math

import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F     # noqa: E402

from oracle import metrics as om     # noqa: E402
from tests import metrics_edges_common as mc     # noqa: E402


@pytest.fixture(scope="module")
def lib():
    import ct_hip
    return ct_hip.lib()


def test_oracle_factor_at_the_rounding_edges():
    got = {m: om.metric_factor(m, m + 4) for m in (383, 384, 639, 640, 641, 895, 896)}
    assert got == {383: 1, 384: 2, 639: 2, 640: 2, 641: 3, 895: 3, 896: 4}
    assert {s: om.metric_factor(*s[1:]) for s in mc.FACTOR_SHAPES} == mc.FACTOR_SHAPES


@pytest.mark.parametrize("m", [127, 128, 129, 383, 384, 385, 639, 640, 641, 895, 896, 897])
def test_pooled_size_follows_the_oracle_factor(lib, m):
    f = om.metric_factor(m, m + 4)
    hp, wp = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.ct_fsim_pooled_size(m, m + 4, ctypes.byref(hp), ctypes.byref(wp)) == 0
    assert (hp.value, wp.value) == (m // f, (m + 4) // f)
    assert lib.ct_fsim_pooled_size(m + 4, m, ctypes.byref(hp), ctypes.byref(wp)) == 0          # the minimum side, whichever it is
    assert (hp.value, wp.value) == ((m + 4) // f, m // f)


def test_icid_size_rule_is_interpolates():
    """ct_frame_icid_f32 sizes its map as floor(H * (1 / f)) in float64; F.interpolate(scale_factor=1 / f) must agree for every
    frame height a factor can meet (a mismatch would shift every bilinear tap)"""
    bad = []
    for f in range(2, 8):
        for h in range(6 * f, 2201):
            want = F.interpolate(torch.zeros(1, 1, h, f), scale_factor=1 / f, mode="bilinear").shape[-2]
            if math.floor(h * (1.0 / f)) != want:
                bad.append((f, h, want))
    assert not bad, bad[:10]


@pytest.mark.parametrize("shape", list(mc.FACTOR_SHAPES) + [(3, mc.PROBE_H, mc.PROBE_W)] + list(mc.STAGE_SHAPES))
def test_metric_workspace_holds_both_tile_grids(lib, shape):
    b, h, w = shape
    f = om.metric_factor(h, w)
    ssim_tiles = math.ceil((w // f - 10) / 32) * math.ceil((h // f - 10) / 32) * 3        # 32 x 32 tiles of the valid map, 3 planes
    hi, wi = math.floor(h * (1.0 / f)), math.floor(w * (1.0 / f))
    icid_tiles = math.ceil(wi / 32) * math.ceil(hi / 16)                                      # 32 x 16 tiles of the whole map
    assert lib.ct_metric_workspace_bytes(h, w, b) >= 8 * b * max(ssim_tiles, icid_tiles)


def test_fsim_stage_offsets(lib):
    off = (ctypes.c_size_t * 4)()
    b, h, w = 2, 641, 643
    assert lib.ct_fsim_stage_offsets(b, h, w, off) == 0
    p = (h // 3) * (w // 3)
    iq, grad, pc, thr = list(off)
    assert iq % 256 == grad % 256 == pc % 256 == thr % 256 == 0
    assert grad - iq >= 2 * b * 2 * p * 4 and pc - grad >= 2 * b * p * 4 and thr - pc >= 2 * b * p * 4      # regions do not overlap
    assert iq >= 2 * b * 17 * p * 8 and thr + 2 * b * 4 * 4 <= lib.ct_fsim_workspace_bytes(b, h, w)
    assert lib.ct_fsim_stage_offsets(1, 1, 40, off) != 0 and lib.ct_fsim_stage_offsets(0, 64, 64, off) != 0


# ---- probe resolving power -------------------------------------------------------------------------------------------------------
def _corrupt(m, kind):
    """the map with one row / column replaced by its neighbour: what a lost halo line, a wrong reflect index or a seam slip does"""
    m = m.clone()
    if kind == "last-row":
        m[..., -1, :] = m[..., -2, :]
    elif kind == "last-col":
        m[..., :, -1] = m[..., :, -2]
    else:
        m[..., 32, :] = m[..., 31, :]
    return m


@pytest.mark.parametrize("kind", ["last-row", "last-col", "row-32"])
@pytest.mark.parametrize("name", ["ssim", "icid"])
def test_probes_resolve_a_wrong_map_line(name, kind):
    gt = mc.probe_gt()
    fn = om.ssim if name == "ssim" else om.icid
    best = 0.0
    for origin in mc.PROBES:
        m = fn(mc.probe(gt, origin), gt, return_map=True)
        assert m.shape[-2:] == ((65, 67) if name == "ssim" else (75, 77))
        best = max(best, abs(float(m.mean()) - float(_corrupt(m, kind).mean())))
    assert best > 10 * mc.ATOL[name], (name, kind, best)


def test_probe_values_are_far_above_the_tolerances():
    gt = mc.probe_gt()
    for origin in mc.PROBES:
        x = mc.probe(gt, origin)
        for name in mc.METRICS:
            v = float(mc.oracle(name, x, gt)[0])
            d = v if name == "icid" else 1 - v
            assert d > 10 * mc.ATOL[name], (origin, name, d)


def test_return_map_is_what_the_value_averages():
    x, y = mc.pair(3, 2, 40, 56)
    assert torch.allclose(om.ssim(x, y, return_map=True).mean(dim=(-1, -2)).mean(dim=1), om.ssim(x, y), rtol=0, atol=1e-15)
    assert abs(float(1 - om.icid(x, y, return_map=True).mean()) - float(om.icid(x, y))) < 1e-15
    st = om.fsim_stages(x)
    assert st["t"].shape == (2, 4) and all(st[k].shape == (2, 40, 56) for k in ("y", "i", "q", "grad", "pc"))
    assert om.ssim(x, y, dtype=torch.float32).dtype == torch.float32 and om.fsim(x, y, dtype=torch.float32).dtype == torch.float32
