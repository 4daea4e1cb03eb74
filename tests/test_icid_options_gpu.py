"""iCID with the reference's full signature on the GPU (ct_frame_icid_opt_f32 / ct_frame_icid_opt_hwc_u8, csrc/metrics.hip): the
twelve option combinations against runs of the reference's own utils/icid.py (tests/golden/icid_options.npz), the tile and factor
edges against the restatement of tests/icid_options_common.py, and the bitwise contracts -- the default options are the entries
without options, downsampling changes nothing at f = 1, the hwc_u8 form is the f32 form on the converted tensors -- up to
methods.icid, utils.icid.icid and the Runner."""
import pytest

torch = pytest.importorskip("torch")
from tests import icid_options_common as ic     # noqa: E402
from tests.metric_groups_common import make_case, planar     # noqa: E402

pytestmark = pytest.mark.gpu
REINHARD_SPEC = "methods.linear.color_transfer_between_images"
ALL = tuple(c for c, _ in ic.COMBOS)


@pytest.fixture(scope="module")
def hip():
    import ct_hip
    ct_hip.lib()
    return ct_hip


def kw(combo):
    return {"intent": combo[0], "omit_maps67": combo[1], "downsampling": combo[2]}


# ---- 1. the reference's own runs ----------------------------------------------------------------------------------------------------
def test_goldens(hip, golden_dir):
    from utils.icid import icid
    frames, g = ic.golden_frames(golden_dir), ic.golden_values(golden_dir)
    for tag in "abcd":
        x, y = (t.cuda() for t in frames[tag])
        for combo, idx in ic.COMBOS:
            got, want = float(hip.frame_icid(x, y, **kw(combo))[0]), float(g[tag + "/f64"][idx])
            print("[golden %s %s] device %.9f reference f64 %.9f err %.2e" % (tag, combo, got, want, abs(got - want)))
            assert abs(got - want) <= ic.ATOL, (tag, combo, got, want)
    x, y = (t.cuda() for t in frames["batch"])
    for combo, idx in ic.COMBOS:
        got = icid(x, y, *combo)
        assert got.dim() == 0 and got.device == x.device
        assert abs(float(got) - float(g["batch/f64"][idx])) <= ic.ATOL, (combo, float(got))
        per = hip.frame_icid(x, y, **kw(combo)).cpu()
        assert float((per - torch.from_numpy(g["batch/frames_f64"][(slice(None),) + idx])).abs().max()) <= ic.ATOL
    one = icid(x[0], y[0], "chromatic", True, False)                     # a single [3,H,W] frame
    assert one.dim() == 0 and abs(float(one) - float(g["batch/frames_f64"][0][2, 1, 1])) <= ic.ATOL


# ---- 2. tile and factor edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ic.EDGE_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_edges_vs_restatement(hip, shape):
    x, y, ref = ic.edge_case(shape)
    xd, yd = x.cuda(), y.cuda()
    for (intent, omit, down), (f64, f32) in ref.items():
        got = hip.frame_icid(xd, yd, intent, omit, down)
        assert torch.equal(got, hip.frame_icid(xd, yd, intent, omit, down))                   # deterministic
        got = got.cpu()
        for i in range(shape[0]):
            err, bound = abs(float(got[i] - f64[i])), max(ic.ATOL, ic.K_F32 * abs(float(f32[i] - f64[i])))
            print("[edge %s %s %s down=%s frame %d] device %.9f f64 %.9f err %.2e bound %.2e" % (shape, intent, omit, down, i, float(got[i]),
                                                                                               float(f64[i]), err, bound))
            assert err <= bound, (shape, intent, omit, down, i, err, bound)
    if shape[1] >= 384:                                                                       # f = 2: the flag matters
        for intent, omit in ic.EDGE_OPTIONS:
            assert abs(float(ref[(intent, omit, True)][0][0] - ref[(intent, omit, False)][0][0])) > 100 * ic.ATOL


# ---- 3. the default options are the entries without options -------------------------------------------------------------------------
def _direct(hip, entry, a, b, h, w, opts=None, ws_bytes=None):
    """a direct call of one C entry -> (return code, out [B])"""
    from ct_hip._core import CT_WS_LAB_STATS, _ptr, _stream, workspace
    B = a.shape[0]
    out = torch.full((B,), -7.0, dtype=torch.float64, device="cuda")
    ws = workspace(CT_WS_LAB_STATS, 0, B, a.device, need=1 << 20)
    args = (_ptr(a), _ptr(b), h, w, B) + (tuple(opts) if opts is not None else ()) + (_ptr(out), _ptr(ws), ws.numel() if ws_bytes is None else ws_bytes,
                                                                                      _stream())
    rc = getattr(hip.lib(), entry)(*args)
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("shape", [(2, 37, 53), (1, 385, 387)], ids=lambda s: "%dx%dx%d" % s)
def test_default_options_are_the_plain_entries(hip, shape):
    b, h, w = shape
    result, gt = make_case(b, h, w)
    x, y = planar(result, gt)
    xd, yd, rd, gd = x.cuda(), y.cuda(), result.cuda(), gt.cuda()
    rc0, plain = _direct(hip, "ct_frame_icid_f32", xd, yd, h, w)
    rc1, opt = _direct(hip, "ct_frame_icid_opt_f32", xd, yd, h, w, (0, 0, 1))
    assert rc0 == 0 and rc1 == 0 and torch.equal(plain, opt) and bool(torch.isfinite(opt).all()) and float(opt.min()) > 0
    rc0, plain_hwc = _direct(hip, "ct_frame_icid_hwc_u8", rd, gd, h, w)
    rc1, opt_hwc = _direct(hip, "ct_frame_icid_opt_hwc_u8", rd, gd, h, w, (0, 0, 1))
    assert rc0 == 0 and rc1 == 0 and torch.equal(plain_hwc, opt_hwc) and torch.equal(plain_hwc, plain)
    # and the binding's defaults go through the plain entries
    assert torch.equal(hip.frame_icid(xd, yd), plain) and torch.equal(hip.frame_icid_hwc(rd, gd), plain)


# ---- 4. f = 1: downsampling changes nothing -----------------------------------------------------------------------------------------
def test_downsampling_is_idle_at_factor_one(hip):
    x, y, _ = ic.edge_case((2, 37, 53))
    xd, yd = x.cuda(), y.cuda()
    seen = set()
    for intent in ic.INTENTS:
        for omit in ic.OMIT:
            on, off = hip.frame_icid(xd, yd, intent, omit, True), hip.frame_icid(xd, yd, intent, omit, False)
            assert torch.equal(on, off), (intent, omit)
            seen.add(round(float(on[0]), 5))
    assert len(seen) == 6                                                                     # the six kernels are six kernels


# ---- 5. the two frame sources -------------------------------------------------------------------------------------------------------
def test_frame_sources_agree_bitwise(hip):
    b, h, w = 2, 37, 53
    result, gt = make_case(b, h, w)
    assert float(result.min()) < 0 and float(result.max()) > 1
    x, y = planar(result, gt)
    xd, yd, rd, gd = x.cuda(), y.cuda(), result.cuda(), gt.cuda()
    bad = result.clone()
    bad[1] = float("nan")
    bx, _ = planar(bad, gt)
    for combo in ALL:
        a, p = hip.frame_icid_hwc(rd, gd, **kw(combo)), hip.frame_icid(xd, yd, **kw(combo))
        assert torch.equal(a, p) and bool(torch.isfinite(a).all()), combo
        want = ic.per_frame(x, y, *combo)
        assert float((a.cpu() - want).abs().max()) <= ic.ATOL, (combo, a.tolist(), want.tolist())
        n = hip.frame_icid_hwc(bad.cuda(), gd, **kw(combo))
        assert torch.equal(n[0], a[0]) and bool(torch.isnan(n[1])), (combo, n.tolist())
        n = hip.frame_icid(bx.cuda(), yd, **kw(combo))
        assert torch.equal(n[0], a[0]) and bool(torch.isnan(n[1])), (combo, n.tolist())


# ---- 6. identical frames ------------------------------------------------------------------------------------------------------------
def test_identical_frames(hip):
    for shape in ((2, 37, 53), (1, 385, 387)):
        x, _, _ = ic.edge_case(shape)
        xd = x.cuda()
        for combo in ALL:
            v = hip.frame_icid(xd, xd, **kw(combo))
            assert float(v.abs().max()) < 1e-6, (shape, combo, v.tolist())


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    from methods import icid as methods_icid
    small = torch.rand(1, 3, 5, 9).cuda()
    for options in ({}, {"intent": "chromatic"}, {"downsampling": False}):
        with pytest.raises(hip.CtHipError):
            hip.frame_icid(small, small, **options)
    with pytest.raises(ValueError):
        hip.frame_icid(small, small, intent="hue")
    with pytest.raises(ValueError):
        methods_icid(small, small, intent="hue")
    b, h, w = 1, 385, 387
    x, y, _ = ic.edge_case((b, h, w))
    xd, yd = x.cuda(), y.cuda()
    lib = hip.lib()
    short, need = lib.ct_metric_workspace_bytes(h, w, b), lib.ct_icid_workspace_bytes(h, w, b, 0)
    assert short < need
    rc, out = _direct(hip, "ct_frame_icid_opt_f32", xd, yd, h, w, (2, 1, 0), ws_bytes=short)
    assert rc == -2 and bool((out == -7.0).all())                                             # CT_E_WORKSPACE, and nothing was written
    rc, out = _direct(hip, "ct_frame_icid_opt_f32", xd, yd, h, w, (2, 1, 1), ws_bytes=short)   # with downsampling it is enough
    assert rc == 0 and bool(torch.isfinite(out).all())
    rc, out = _direct(hip, "ct_frame_icid_opt_f32", xd, yd, h, w, (2, 1, 0), ws_bytes=need)
    assert rc == 0 and torch.equal(out, hip.frame_icid(xd, yd, "chromatic", True, False))
    rc, out = _direct(hip, "ct_frame_icid_opt_f32", xd, yd, h, w, (3, 0, 1))
    assert rc == -1 and bool((out == -7.0).all())                                             # CT_E_BADARG


# ---- 8. Runner ----------------------------------------------------------------------------------------------------------------------
def test_runner_passes_the_options(hip):
    from methods import Runner, icid as methods_icid
    from utils.data import SyntheticStereoVideoU8
    options = {"intent": "chromatic", "omit_maps67": False, "downsampling": False}
    x, y, _ = ic.edge_case((2, 37, 53))
    batch = {"target": x.cuda(), "reference": y.flip(3).contiguous().cuda(), "gt": y.cuda()}
    model = Runner(REINHARD_SPEC, icid_intent="chromatic", icid_downsampling=False)
    m = model.test_step(batch)
    result = model(batch).clamp(0, 1)
    assert torch.equal(m["Test iCID"], methods_icid(result, batch["gt"], intent="chromatic", downsampling=False))
    plain = Runner(REINHARD_SPEC).test_step(batch)
    assert torch.equal(plain["Test iCID"], methods_icid(result, batch["gt"])) and not torch.equal(plain["Test iCID"], m["Test iCID"])
    for name in ("Test PSNR", "Test SSIM", "Test FSIM"):
        assert torch.equal(plain[name], m[name])
    # the grouped route: column 3 from the group's own buffers, with the same options
    group = SyntheticStereoVideoU8(2, 40, 56, group=2, pool=2).host_chunk(0)[:, :2].contiguous().cuda()
    grouped = Runner(REINHARD_SPEC, metric_groups=True, icid_intent="chromatic", icid_downsampling=False)
    table = torch.zeros((2, 4), dtype=torch.float64, device="cuda")
    out = grouped.test_group_metrics(group, table)
    assert torch.equal(table[:, 3], hip.frame_icid_hwc(out, group[2], **options))
    table0 = torch.zeros((2, 4), dtype=torch.float64, device="cuda")
    Runner(REINHARD_SPEC, metric_groups=True).test_group_metrics(group, table0)
    assert torch.equal(table0[:, :3], table[:, :3]) and not torch.equal(table0[:, 3], table[:, 3])
    assert torch.equal(table0[:, 3], hip.frame_icid_hwc(out, group[2]))
