"""The frame metrics (ct_frame_ssim_f32 / icid / fsim / psnr, ct_fft2d_c2c_f32) against the float64 oracle at their edges: every
pooling factor with remainder rows and columns, the rim no metric may read, single-patch probes on the tile seams and the frame
edge, flat and saturated frames (where float32 moments cancel), PSNR's tail / unaligned / zero paths, FSIM's stages behind its
weighted mean, and the FFT on a plane with FSIM's dynamic range.  Every figure is printed before it is asserted (pytest -s)."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from oracle import metrics as om     # noqa: E402
from tests import metrics_edges_common as mc     # noqa: E402

pytestmark = pytest.mark.gpu
EPS32 = float(torch.finfo(torch.float32).eps)


@pytest.fixture(scope="module")
def hip():
    import ct_hip
    ct_hip.lib()
    return ct_hip


_frames = {}


def _factor_frames(shape):
    if shape not in _frames:
        b, h, w = shape
        _frames[shape] = mc.pair(h + 2 * w, b, h, w)
    return _frames[shape]


# ---- every factor, with remainders; the dead rim -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(mc.FACTOR_SHAPES))
@pytest.mark.parametrize("name", mc.METRICS)
def test_every_factor_with_remainders(hip, name, shape):
    x, y = _factor_frames(shape)
    got, want = mc.device(hip, name, x, y), mc.oracle(name, x, y)
    print("\n[%s %s f=%d] device %s oracle %s" % (name, shape, mc.FACTOR_SHAPES[shape], got.tolist(), want.tolist()))
    assert got.shape == (shape[0],) and torch.allclose(got, want, rtol=0, atol=mc.ATOL[name]), (got, want)


_rims = {}


@pytest.mark.parametrize("shape", list(mc.FACTOR_SHAPES))
@pytest.mark.parametrize("name", mc.METRICS)
def test_dead_rim_has_no_effect(hip, name, shape):
    """the rows and columns the oracle proves dead, replaced by 1 - x in both frames: the device value may not move by one bit"""
    x, y = _factor_frames(shape)
    _, h, w = shape
    if name == "icid":
        if shape not in _rims:
            _rims[shape] = mc.icid_rim(x, y)
        row0, col0 = _rims[shape]
        assert h - row0 >= h % mc.FACTOR_SHAPES[shape] and w - col0 >= w % mc.FACTOR_SHAPES[shape]
    else:
        row0, col0 = mc.pooled_rim(h, w)
        x2, y2 = mc.flip_rim(x, row0, col0), mc.flip_rim(y, row0, col0)
        assert torch.equal(mc.oracle(name, x2, y2), mc.oracle(name, x, y))
    print("\n[%s %s] dead rows %d.., dead columns %d.." % (name, shape, row0, col0))
    x2, y2 = mc.flip_rim(x, row0, col0), mc.flip_rim(y, row0, col0)
    if (row0, col0) != (h, w):
        assert not torch.equal(x2, x)
    assert torch.equal(mc.device(hip, name, x2, y2), mc.device(hip, name, x, y))


def test_dead_rim_cases_are_not_empty():
    dead = [s for s in mc.FACTOR_SHAPES if mc.pooled_rim(*s[1:]) != s[1:]]
    assert len(dead) == 3 and (1, 640, 644) not in dead


# ---- probes at 75 x 77 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.METRICS)
def test_probes_vs_oracle(hip, name):
    gt = mc.probe_gt()
    singles = []
    for patch in mc.PROBES:
        x = mc.probe(gt, patch)
        got, want = mc.device(hip, name, x, gt), mc.oracle(name, x, gt)
        print("\n[%s probe %s] device %.9f oracle %.9f diff %.2g" % (name, patch, float(got[0]), float(want[0]), float(got[0] - want[0])))
        assert torch.allclose(got, want, rtol=0, atol=mc.ATOL[name]), (patch, got, want)
        singles.append(got)
    # three probes in one call: each batch item is its single-frame call, bit for bit
    pick = (1, 5, 9)
    xb = torch.cat([mc.probe(gt, mc.PROBES[i]) for i in pick])
    got = mc.device(hip, name, xb, gt.expand(3, -1, -1, -1).contiguous())
    assert torch.equal(got, torch.cat([singles[i] for i in pick]))


# ---- flat and saturated frames ---------------------------------------------------------------------------------------------------------
_flat = {}


def _flat_inputs():
    if not _flat:
        _flat.update(mc.flat_inputs())
    return _flat


@pytest.mark.parametrize("case", ["noise", "flat-bright", "const-0.2-0.8", "sat-1-254", "zeros", "letterbox", "flat-bright-641x643"])
def test_flat_and_saturated_frames(hip, case):
    """|device - oracle(float64)| <= max(atol, k * |oracle(float32) - oracle(float64)|): where the reference's own float32 run
    leaves float64 the device may follow it, no further"""
    x, gt, plain = _flat_inputs()[case]
    bad = []
    for name in mc.METRICS:
        got = float(mc.device(hip, name, x, gt)[0])
        o64, o32 = float(mc.oracle(name, x, gt)[0]), float(mc.oracle(name, x, gt, dtype=torch.float32)[0])
        gap, err = abs(o32 - o64), abs(got - o64)
        bound = mc.ATOL[name] if plain else max(mc.ATOL[name], mc.K_FLAT[name] * gap)
        print("\n[flat %s %s] device %.9f oracle64 %.9f oracle32 %.9f gap %.3g err %.3g err/gap %.3g bound %.3g"
              % (case, name, got, o64, o32, gap, err, err / gap if gap else float("nan"), bound))
        if not (math.isfinite(got) and 0.0 <= got <= 1 + 1e-6):
            bad.append((name, "range", got))
        if plain and gap > mc.ATOL[name] / 10:      # black bars do not make float32 leave float64: the plain tolerance holds
            bad.append((name, "letterbox gap", gap))
        if err > bound:
            bad.append((name, "bound", got, o64, gap))
        if case == "zeros" and got != (0.0 if name == "icid" else 1.0):
            bad.append((name, "zeros", got))
    assert not bad, bad


# ---- PSNR alone ----------------------------------------------------------------------------------------------------------------------
PSNR_SHAPES = [(1, 1), (1, 3), (3, 5), (2, 1023), (3, 70001), (2, 3, 37, 53)]


def _offset_view(t):
    """the same values, contiguous, starting one float into a larger buffer: no frame is 16-byte aligned -> the scalar path"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("shape", PSNR_SHAPES)
def test_psnr_vs_float64(hip, shape, offset):
    gen = torch.Generator().manual_seed(sum(shape))
    a = torch.rand(shape, generator=gen)
    b = (a + 0.1 * torch.randn(shape, generator=gen)).clamp(0, 1)
    da, db = a.cuda(), b.cuda()
    if offset:
        da, db = _offset_view(da), _offset_view(db)
    got = hip.frame_psnr(da, db).cpu()
    a64, b64 = a.numpy().astype(np.float64).reshape(shape[0], -1), b.numpy().astype(np.float64).reshape(shape[0], -1)
    mse = ((a64 - b64) ** 2).mean(axis=1)
    print("\n[psnr %s offset=%s] mse %s want %s" % (shape, offset, got[:, 0].tolist(), mse.tolist()))
    assert got.shape == (shape[0], 2) and got.dtype == torch.float64
    assert np.allclose(got[:, 0].numpy(), mse, rtol=1e-12, atol=0)
    assert torch.allclose(got[:, 1], om.psnr(a, b), rtol=0, atol=1e-9)
    assert np.allclose(got[:, 1].numpy(), 10 * np.log10(1 / mse), rtol=0, atol=1e-9)
    # identical frames: mse 0, the clamp at 1e-300; 0 against 1: mse 1, 0 dB
    same = hip.frame_psnr(da, da.clone() if not offset else _offset_view(da.clone())).cpu()
    assert torch.equal(same[:, 0], torch.zeros(shape[0], dtype=torch.float64))
    assert same[:, 1].tolist() == [10 * math.log10(1e300)] * shape[0] == [3000.0] * shape[0]
    zero, one = torch.zeros_like(da), torch.ones_like(da)
    if offset:
        zero, one = _offset_view(zero), _offset_view(one)
    far = hip.frame_psnr(zero, one).cpu()
    assert far[:, 0].tolist() == [1.0] * shape[0] and far[:, 1].tolist() == [0.0] * shape[0]


# ---- FSIM's stages --------------------------------------------------------------------------------------------------------------------
def _ring(t):
    m = torch.zeros(t.shape[-2:], dtype=torch.bool)
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = True
    return m


@pytest.mark.parametrize("shape", list(mc.STAGE_SHAPES))
def test_fsim_stages_vs_oracle(hip, shape):
    b, h, w = shape
    x, y = mc.pair(2 * h + w, b, h, w)
    st = hip._fsim_stages(x.cuda(), y.cuda())
    imgs = torch.stack([x, y], dim=1).reshape(2 * b, 3, h, w)                 # image index 2 * pair + (0: a, 1: b)
    o64, o32 = om.fsim_stages(imgs), om.fsim_stages(imgs, dtype=torch.float32)
    want = om.fsim(x, y)
    assert torch.equal(st["score"].cpu(), hip.frame_fsim(x.cuda(), y.cuda()).cpu())
    assert torch.allclose(st["score"].cpu(), want, rtol=0, atol=mc.ATOL["fsim"]), (st["score"], want)
    iq, grad, pc, thr = st["iq"].cpu().double(), st["grad"].cpu().double(), st["pc"].cpu().double(), st["thr"].cpu().double()
    assert iq.shape == (2 * b, 2, h, w) and grad.shape == pc.shape == (2 * b, h, w) and thr.shape == (2 * b, 4)
    e_i, e_q = float((iq[:, 0] - o64["i"]).abs().max()), float((iq[:, 1] - o64["q"]).abs().max())
    eg = (grad - o64["grad"]).abs()
    ring = _ring(eg)
    eg_ring, eg_in = float(eg[:, ring].max()), float(eg[:, ~ring].max())
    print("\n[fsim stages %s] I %.3g Q %.3g grad ring %.3g interior %.3g" % (shape, e_i, e_q, eg_ring, eg_in))
    assert e_i <= 1e-3 and e_q <= 1e-3
    assert max(eg_ring, eg_in) <= 1e-3 and eg_ring <= 4 * eg_in
    # thresholds (relative) and the PC map (absolute) within k x what the float32 oracle itself leaves float64 by
    t_err, t_gap = float(((thr - o64["t"]) / o64["t"]).abs().max()), float(((o32["t"].double() - o64["t"]) / o64["t"]).abs().max())
    p_err, p_gap = float((pc - o64["pc"]).abs().max()), float((o32["pc"].double() - o64["pc"]).abs().max())
    print("[fsim stages %s] T rel err %.3g gap %.3g ratio %.3g | PC err %.3g gap %.3g ratio %.3g"
          % (shape, t_err, t_gap, t_err / t_gap, p_err, p_gap, p_err / p_gap))
    assert t_err <= max(8 * EPS32, mc.K_STAGE["t"] * t_gap)
    assert p_err <= max(8 * EPS32, mc.K_STAGE["pc"] * p_gap)


# ---- the FFT on image-like input ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(mc.FFT_SHAPES))
def test_fft2d_bands_on_image_like_input(hip, shape):
    """error per radial band relative to the band's own RMS (not to the DC bin, five orders above the bins the log-Gabor bank
    keeps), against torch.fft.fft2's complex64 error on the same input and band"""
    h, w = shape
    x = mc.image_like_plane(h, w)
    want = torch.fft.fft2(x.to(torch.complex128))
    got = hip.fft2d_(x.cuda().clone()).cpu().to(torch.complex128)
    cpu32 = torch.fft.fft2(x).to(torch.complex128)
    band = mc.radial_bands(h, w)
    e_dev, e_cpu = mc.band_errors(got, want, band), mc.band_errors(cpu32, want, band)
    ratios = [d / c for d, c in zip(e_dev, e_cpu)]
    print("\n[fft bands %s] device %s\n  complex64 torch %s\n  ratio %s" % (shape, ["%.2g" % v for v in e_dev], ["%.2g" % v for v in e_cpu],
                                                                        ["%.2f" % v for v in ratios]))
    # DC: a sum of h w positive terms; worst case of float32 summation along a row and then a column
    assert abs(got[0, 0] - want[0, 0]) <= (h + w) * EPS32 / 2 * abs(want[0, 0])
    assert max(ratios) <= mc.K_FFT, ratios


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    def r(*s):
        return torch.rand(*s).cuda()
    with pytest.raises(hip.CtHipError):
        hip.frame_icid(r(1, 3, 5, 40), r(1, 3, 5, 40))          # reflect padding of 5 needs 6 rows
    with pytest.raises(hip.CtHipError):
        hip.frame_fsim(r(1, 3, 1, 40), r(1, 3, 1, 40))
    with pytest.raises(hip.CtHipError):
        hip.frame_ssim(r(1, 3, 10, 40), r(1, 3, 10, 40))        # smaller than the 11 x 11 window
    for fn in (hip.frame_ssim, hip.frame_icid, hip.frame_fsim, hip.frame_psnr):
        with pytest.raises(hip.CtHipError):
            fn(r(1, 3, 40, 56), r(1, 3, 40, 57))
        with pytest.raises(hip.CtHipError):
            fn(r(1, 3, 40, 56).double(), r(1, 3, 40, 56).double())
        out = fn(r(0, 3, 40, 56), r(0, 3, 40, 56))
        assert out.dtype == torch.float64 and out.numel() == 0 and out.shape[0] == 0
