"""The cases of tests/gmflow_glue_common.py meet, on the CPU and on the oracle alone, every condition that
tests/test_gmflow_glue_gpu.py relies on: the gate of each continuous case is at most 1e-3 of its output range, the out-of-image
flows leave through every side, the occlusion masks are mixed and decided away from the threshold, huge finite flows sample
nothing in float64 and in float32."""
import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F   # noqa: E402

from oracle import gmflow as og   # noqa: E402
from tests import gmflow_glue_common as C   # noqa: E402


def assert_cap(case):
    ok, gt, scale = C.gate_cap_ok(case)
    assert ok, "%s: gate %.3g is above 1e-3 of the output range %.3g -- wrong data for this case" % (case.name, gt, scale)


@pytest.mark.parametrize("shape", C.WARP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_flow_warp_cases(shape):
    n, c, h, w = shape
    for name in C.warp_case_names(shape):
        case = C.warp_case(shape, name)
        assert_cap(case)
        assert torch.isfinite(case.flow).all()
        zero = case.zero[:, None].expand_as(case.y64)
        assert case.y64[zero].abs().max().item() == 0.0 if zero.any() else True      # >= 1.5 px outside: no tap, float64 ...
        assert case.y32[zero].abs().max().item() == 0.0 if zero.any() else True      # ... and the reference's float32
        left, right, top, bottom = C.outside_masks(case.flow)
        out = left | right | top | bottom
        if name == "outside":
            assert 0.2 <= out.float().mean().item() <= 0.6, (case.name, out.float().mean().item())
            for i in range(n):                                                  # every image of the batch leaves through every side
                assert left[i].any() and right[i].any() and top[i].any() and bottom[i].any(), case.name
                corners = [(left[i] & top[i]).any(), (right[i] & top[i]).any(), (left[i] & bottom[i]).any(), (right[i] & bottom[i]).any()]
                assert all(corners) if h * w >= 8 else (corners[0] and corners[3]), case.name
            if h * w >= 8:
                assert (out & ~case.zero).any() and case.zero.any()             # partial taps at the border and pixels without any tap
        if name == "outside_corners":
            assert (left & top).any() and (right & top).any() and (left & bottom).any() and (right & bottom).any() and out.all()
        if name in ("const6", "const7"):      # (W, 0) and (0, -H), one whole image away: nothing but the rounding of the grid's round trip
            assert case.y64.abs().max().item() <= 1e-12 * case.scale
        if case.huge is not None:
            huge = case.huge
            assert abs(huge.float().mean().item() - 0.25) <= 0.01 or h * w < 8
            assert (case.zero | ~huge).all()                                    # every huge pixel is far outside ...
            hm = huge[:, None].expand_as(case.y64)
            assert case.y64[hm].abs().max().item() == 0.0 and case.y32[hm].abs().max().item() == 0.0    # ... and samples nothing
            assert case.y64[~hm].abs().max().item() > 0.1
    if h * w >= 24:                                                             # all six huge values, on both components
        flow, huge = C.huge_flow(n, h, w, 1, 0)
        vals = {(comp, v) for comp in range(2) for v in flow[:, comp][huge].tolist() if abs(v) >= 1e4}
        assert vals == {(comp, float(torch.tensor(v, dtype=torch.float32))) for comp in range(2) for v in C.HUGE_FLOWS}


@pytest.mark.parametrize("name", sorted(C.RESIZE_CASES))
def test_bilinear_resize_cases(name):
    case = C.resize_case(name)
    assert_cap(case)
    n, c = case.x.shape[:2]
    assert case.y64.shape == (n, c) + tuple(case.size)
    if "n2c3" in name or "n3c2" in name:
        assert n > 1 and case.mul0 != case.mul1                                  # a wrong nc % C shows only with N > 1
        swapped = C.resize_ref(case.x.double(), case.size, case.mul1, case.mul0)
        assert (swapped - case.y64).abs().max().item() > 1e3 * C.gate(case.y32, case.y64, case.g)[0]


@pytest.mark.parametrize("cfg", sorted(C.CONVEX_CASES), ids=lambda s: "x".join(map(str, s)))
def test_convex_upsample_cases(cfg):
    b, h, w, f = cfg
    for kind in C.CONVEX_CASES[cfg]:
        case = C.convex_case(cfg, kind)
        assert_cap(case)
        assert torch.isfinite(case.y64).all() and torch.isfinite(case.y32).all()
        if kind == "equal":                                                     # uniform 1/9 over the zero-padded 3 x 3 window
            want = C.up_nearest(F.avg_pool2d(f * case.flow.double(), 3, stride=1, padding=1, count_include_pad=True), f)
            assert (case.y64 - want).abs().max().item() <= 1e-12
        if case.tap is not None:
            nb, inside = C.neighbour(case.flow.double(), case.tap)
            level = float(kind[3:kind.index("_")])
            rest = 8 * torch.exp(torch.tensor(-level, dtype=torch.float64)).item() * f * case.flow.abs().max().item()
            assert (case.y64 - C.up_nearest(f * nb, f)).abs().max().item() <= rest
            if kind.startswith("tap120"):                                       # e^-120 is below float32: the reference gives an exact 0
                assert case.y32[~C.up_nearest(inside, f).expand_as(case.y32)].abs().sum().item() == 0.0


@pytest.mark.parametrize("shape", C.FB_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fb_check_cases(shape):
    fwd, bwd = C.fb_flows(shape)
    focc, bocc, fband, bband = C.fb_reference(fwd, bwd)
    f32, b32 = og.forward_backward_consistency_check(fwd, bwd)
    f64, b64 = og.forward_backward_consistency_check(fwd.double(), bwd.double())
    assert torch.equal(f64, focc) and torch.equal(b64, bocc)                    # fb_reference restates the oracle
    for occ, band, o32 in ((focc, fband, f32), (bocc, bband, b32)):
        assert 0.1 <= occ.mean().item() <= 0.6, (shape, occ.mean().item())
        assert band.float().mean().item() <= 0.005
        assert torch.equal(o32.double()[~band], occ[~band])                     # the reference's float32 decides the same outside the band


def test_fb_check_threshold_is_strict():
    """alpha = 0, beta = 0.5: a difference of exactly 0.5 is NOT occluded (geometry.py:96 compares with >), the next float32 is.
    W - 1 and H - 1 are powers of two, so the reference's normalise / un-normalise of the pixel grid is exact and the warp of a
    constant field is that constant."""
    fwd, bwd = torch.zeros(2, 2, 5, 257), torch.zeros(2, 2, 5, 257)
    fwd[:, 0] = 0.5
    fo, bo = og.forward_backward_consistency_check(fwd, bwd, alpha=0.0, beta=0.5)
    assert fo.abs().max().item() == 0.0 and bo.abs().max().item() == 0.0
    fwd[:, 0] = 0.50000006
    assert fwd.max().item() > 0.5
    fo, _ = og.forward_backward_consistency_check(fwd, bwd, alpha=0.0, beta=0.5)
    assert fo.min().item() == 1.0


@pytest.mark.parametrize("name", sorted(C.INORM_SHAPES))
def test_instance_norm_cases(name):
    kinds = ["randn"] + (["tiny", "constant", "offset"] if name in C.INORM_SPECIAL_SHAPES else [])
    for kind in kinds:
        case = C.inorm_case(name, kind)
        plane = case.x.shape[2] * case.x.shape[3]
        if kind == "constant" or plane == 1:                                    # a constant plane (a 1-pixel plane is one) normalises to 0
            assert case.y64.abs().max().item() <= 1e-9 and not torch.isnan(case.y32).any()
            continue
        if kind == "offset":       # held to inorm_offset_bound, not to the gate: float32 torch adds the summation error of its mean
            assert torch.isfinite(C.inorm_offset_bound(case.x, case.y64)).all()
            continue
        for y64, y32 in zip(C.inorm_modes(case.y64, case.skip), C.inorm_modes(case.y32, case.skip)):
            assert_cap(C.SimpleNamespace(name=case.name, y64=y64, y32=y32, g=case.g))


def test_instance_norm_nan_reference():
    """one NaN in a plane: F.instance_norm + relu give a NaN plane on the CPU and leave the other planes alone"""
    x, skip = C.inorm_data("p257", "randn")
    x[1, 2, 0, 100] = float("nan")
    for y in C.inorm_modes(C.inorm_plain(x), skip)[1:]:
        bad = torch.isnan(y)
        assert bad[1, 2].all() and bad.sum().item() == 257


def test_eltwise_and_layernorm_cases():
    for plane in (35, 8160):
        assert_cap(C.normalize_case(plane))
    for chans, split, plane in ((256, 128, 68 * 120), (6, 0, 35), (6, 6, 35)):
        assert_cap(C.tanh_relu_case(chans, split, plane))
    for tokens in C.LN_TOKENS:
        for res in (False, True):
            assert_cap(C.ln_case(tokens, 1, res))
            assert_cap(C.ln_case(tokens, 1, res, "constant"))
            for partials in C.LN_PARTIALS[1:]:
                assert_cap(C.ln_case(tokens, partials, res))
        case = C.ln_case(tokens, 1, False, "offset")
        assert ((case.y32.double() - case.y64).abs() <= C.ln_offset_bound(case)).all()
