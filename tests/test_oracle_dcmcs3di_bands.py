"""oracle/dcmcs3di.py: forward_band (the banded form that makes a 1920 x 1080 pair affordable in float64) equals forward on the
band's rows.  Full depth (18 + 6 residual blocks), so the 53-row dependence is the real one; an image tall enough (200 rows)
that an interior band's crop is cut artificially on both sides.  CPU only."""
import pytest

torch = pytest.importorskip("torch")

from oracle import dcmcs3di as odc                      # noqa: E402
from tests.dcmcs3di_common import build_model            # noqa: E402

H, W = 200, 64
TOL = 1e-12
MAPS = ("cost_r2l", "cost_l2r", "att_r2l", "att_l2r", "colsum")      # [B, H, ...]; every other key is [B, C, H, W]


@pytest.fixture(scope="module")
def case():
    sd = {k: v.detach() for k, v in build_model(seed=21).state_dict().items()}
    gen = torch.Generator().manual_seed(22)
    left, right = torch.rand(2, 3, H, W, generator=gen), torch.rand(2, 3, H, W, generator=gen)
    override = torch.rand(2, 1, H, W, generator=gen) > 0.4
    return sd, left, right, override, odc.forward(sd, left, right, valid_override=override)


def test_margins():
    assert odc.band_margin() == 53 and odc.attention_margin() == 14
    assert odc.band_margin(3, 2) == 1 + 6 + 2 + 6


@pytest.mark.parametrize("y0,y1", [(0, 8), (96, 108), (H - 8, H), (50, 60), (0, H)],
                         ids=["top", "interior", "bottom", "cut-below-only-attention-at-edge", "whole"])
def test_band_equals_full(case, y0, y1):
    sd, left, right, override, full = case
    band, state = odc.forward_band(sd, left, right, y0, y1, valid_override=override, return_state=True)
    assert set(band) == set(full)
    for k, want in full.items():
        want = want[:, y0:y1] if k in MAPS else want[:, :, y0:y1]
        assert band[k].shape == want.shape, k
        if want.dtype == torch.bool:
            assert torch.equal(band[k], want), k
        else:
            assert float((band[k] - want).abs().max()) <= TOL, (k, float((band[k] - want).abs().max()))
    # without the override the key is absent, like in forward; the maps can be left out; the transfer stage re-runs alone
    plain = odc.forward_band(sd, left, right, y0, y1, keep_maps=False)
    assert set(plain) == set(full) - {"pre_clamp_override", "cost_r2l", "cost_l2r", "att_r2l", "att_l2r"}
    assert torch.equal(plain["pre_clamp"], band["pre_clamp"])
    again = odc.band_transfer(sd, state, override)
    assert torch.equal(again, band["pre_clamp_override"])
    own = odc.band_transfer(sd, state, full["valid_left"])
    assert float((own - full["pre_clamp"][:, :, y0:y1]).abs().max()) <= TOL


def test_band_margin_is_needed(case):
    """one row less of context changes an interior band: the margin is the dependence, not a loose guess"""
    sd, left, right, _, full = case
    y0, y1 = 96, 108
    cut = odc.forward_band(sd, left[:, :, y0 - 52:y1 + 52], right[:, :, y0 - 52:y1 + 52], 52, 52 + y1 - y0, keep_maps=False)
    assert float((cut["pre_clamp"] - full["pre_clamp"][:, :, y0:y1]).abs().max()) > 0
    ok = odc.forward_band(sd, left[:, :, y0 - 53:y1 + 53], right[:, :, y0 - 53:y1 + 53], 53, 53 + y1 - y0, keep_maps=False)
    assert float((ok["pre_clamp"] - full["pre_clamp"][:, :, y0:y1]).abs().max()) <= TOL


def test_band_rows_checked(case):
    sd, left, right, _, _ = case
    for y0, y1 in ((-1, 4), (10, 10), (190, H + 1)):
        with pytest.raises(ValueError):
            odc.forward_band(sd, left, right, y0, y1)
