"""GPU tests of the disparity of the parallax attention (pasmnet/utils.py:55-105 regress_disp; csrc/disparity.hip, the IDX
variants of csrc/attention16.hip) against the reference's goldens (tests/golden/disparity.npz) and the restatement of the
contract in tests/disparity_common.py.

Gates: the occlusion fill is bitwise (float32 divisions in the reference's order); an expected index computed from a
materialised map is float32-grade (<= 1e-3 px); an expected index from the streaming attention is held to 2e-5 * W px --
the 2e-5 gate of the streaming warp(rgb) test (tests/test_dcmcs3di_gpu.py) scaled to a value range of W."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import disparity_common as dc                 # noqa: E402
from tests.dcmcs3di_common import build_model            # noqa: E402

WIDTHS = (1, 37, 64, 130, 300)


def _g(golden_dir):
    return np.load(os.path.join(golden_dir, "disparity.npz"), allow_pickle=False)


def bitwise_equal(a, b):
    """float32 bit patterns equal, +0 and -0 counted equal"""
    a = np.asarray(a, np.float32) + np.float32(0)
    b = np.asarray(b, np.float32) + np.float32(0)
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def onehot_att(cols):
    c = torch.from_numpy(cols.astype(np.int64)).cuda()
    rows, w = c.shape
    att = torch.zeros((1, rows, w, w), dtype=torch.float32, device="cuda")
    att.scatter_(3, c.view(1, rows, w, 1), 1.0)
    return att


@pytest.mark.parametrize("w", WIDTHS)
def test_regress_disp_onehot_golden_bitwise(golden_dir, w):
    import ct_hip
    from pasmnet.utils import regress_disp
    g = _g(golden_dir)
    cols, valid, want = g["onehot%d/cols" % w], g["onehot%d/valid" % w], g["onehot%d/disp" % w]
    rows = cols.shape[0]
    att = onehot_att(cols)
    vb = torch.from_numpy(valid.astype(bool)).cuda().view(1, 1, rows, w)
    got = ct_hip.regress_disp(att, vb).cpu().numpy().reshape(rows, w)
    assert bitwise_equal(got, want), np.abs(got - want).max()
    got2 = regress_disp(att, vb.float()).cpu().numpy().reshape(rows, w)      # the drop-in, float mask
    assert bitwise_equal(got2, want)


def test_regress_disp_softmax_golden(golden_dir):
    import ct_hip
    from pasmnet.utils import regress_disp
    g = _g(golden_dir)
    att, valid, want = g["soft/att"], g["soft/valid"], g["soft/disp"]
    got = regress_disp(torch.from_numpy(att).cuda(), torch.from_numpy(valid).cuda().float()).cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32
    err = np.abs(got - want).max()
    print("\n[regress_disp softmax B=2 H=8 W=70] max-abs vs reference %.3g px" % err)
    assert err <= 1e-3
    # a width that is no multiple of 4 on a row base that is not 16-byte aligned (scalar head / tail of the loads)
    a = torch.from_numpy(att[:, :, :69, :69].copy()).cuda()
    v = torch.from_numpy(valid[:, :, :, :69].copy()).cuda().bool()
    want2 = dc.regress_disp(a.cpu().numpy(), v.cpu().numpy()[:, 0], np.float64)[:, None]
    assert np.abs(ct_hip.regress_disp(a, v).cpu().numpy() - want2).max() <= 1e-3


@pytest.mark.parametrize("h,w", [(4, 512), (2, 1920), (2, 2100)])
def test_pam_streaming_disp_ini(h, w):
    import ct_hip
    gen = torch.Generator().manual_seed(w + 3)
    ql, kr, qr, kl = (torch.randn(1, 64, h, w, generator=gen) * 2 for _ in range(4))
    v = torch.randn(1, 64, h, w, generator=gen)
    rgb = torch.rand(1, 3, h, w, generator=gen)
    args = [t.cuda() for t in (ql, kr, v, rgb, qr, kl)]
    plain = ct_hip.pam_streaming(*args)
    res = ct_hip.pam_streaming(*args, want_disp=True)
    assert len(plain) == 4 and len(res) == 5
    for name, a, b in zip(("fea", "wrgb", "valid", "colsum"), plain, res[:4]):
        assert torch.equal(a, b), name
    att = torch.softmax(torch.matmul(ql.double().permute(0, 2, 3, 1), kr.double().permute(0, 2, 1, 3)) / 64, dim=-1)
    want = dc.expected_index(att.numpy())[:, None]
    err = np.abs(res[4].cpu().double().numpy() - want).max()
    print("\n[pam_streaming want_disp %dx%d] disp_ini max-abs vs float64 %.3g px (gate %.3g)" % (h, w, err, 2e-5 * w))
    assert err <= 2e-5 * w


@pytest.mark.parametrize("w", [1, 63, 1920])
def test_disp_fill_random_masks_bitwise(w):
    import ct_hip
    rng = np.random.default_rng(w)
    rows = 64
    disp_ini = (rng.standard_normal((1, 1, rows, w)) * w).astype(np.float32)
    p = rng.random((rows, 1)) ** 2                                          # rows from mostly invalid to mostly valid
    valid = (rng.random((1, 1, rows, w)) < p[None, None]).astype(np.float32)
    valid[0, 0, 0] = 0
    valid[0, 0, 1] = 1
    got = ct_hip.pam_disp_fill(torch.from_numpy(disp_ini).cuda(), torch.from_numpy(valid).cuda()).cpu().numpy()
    assert bitwise_equal(got, dc.fill(disp_ini, valid, np.float32))


def test_disp_fill_1080p_long_holes_bitwise():
    import ct_hip
    rng = np.random.default_rng(1080)
    h, w = 1080, 1920
    disp_ini = (rng.standard_normal((1, 1, h, w)) * 40).astype(np.float32)
    valid = np.ones((h, w), np.float32)
    for y in range(h):
        for _ in range(rng.integers(0, 4)):
            a = int(rng.integers(0, w))
            valid[y, a:a + int(rng.integers(1, 600))] = 0
    valid[::97] = 0                                                         # rows without a valid pixel
    valid[5, 1:] = 0                                                        # only the first pixel valid
    valid[6, :-1] = 0                                                       # only the last pixel valid
    valid = valid[None, None]
    got = ct_hip.pam_disp_fill(torch.from_numpy(disp_ini).cuda(), torch.from_numpy(valid).cuda().bool()).cpu().numpy()
    assert bitwise_equal(got, dc.fill(disp_ini, valid, np.float32))


@pytest.mark.parametrize("name", ["a", "b"])
def test_dcmcs3di_disparity_vs_reference_model(golden_dir, name, conv_mode):
    small = np.load(os.path.join(golden_dir, "dcmcs3di_small.npz"), allow_pickle=False)
    g = _g(golden_dir)
    m = build_model().cuda()
    disp, valid = m.disparity(torch.from_numpy(small[name + "/left"]).cuda(), torch.from_numpy(small[name + "/right"]).cuda())
    assert disp.dtype == torch.float32 and valid.dtype == torch.bool and disp.shape == valid.shape
    want, want_valid = g["model_%s/disp" % name], g["model_%s/valid" % name].astype(bool)
    same = (valid.cpu().numpy() == want_valid).all(axis=-1)                 # rows whose whole mask agrees
    assert same.mean() >= 0.9, same.mean()
    w = want.shape[-1]
    err = np.abs(disp.cpu().numpy() - want)[same].max()
    print("\n[DCMCS3DI.disparity %s, %s] max-abs vs reference %.3g px over %.0f%% of the rows" % (name, conv_mode, err, 100 * same.mean()))
    assert err <= 1e-4 * w


def test_dcmcs3di_512_full_depth_disp_vs_oracle():
    from oracle import dcmcs3di as odc
    m = build_model().cuda()
    gen = torch.Generator().manual_seed(3)
    left, right = torch.rand(1, 3, 512, 512, generator=gen), torch.rand(1, 3, 512, 512, generator=gen)
    p = m.forward_parts(left.cuda(), right.cuda(), want_disp=True)
    dev_valid = p["valid_left"].cpu().numpy() > 0.5
    ref = odc.forward({k: v.detach().cpu() for k, v in m.state_dict().items()}, left, right)
    ini = dc.expected_index(ref["att_r2l"].numpy())[:, None]
    del ref
    e_ini = np.abs(p["disp_ini_left"].cpu().double().numpy() - ini).max()
    e_disp = np.abs(p["disp_left"].cpu().double().numpy() - dc.fill(ini, dev_valid, np.float64)).max()
    print("\n[dcmcs3di 512x512 disparity] disp_ini max-abs vs float64 oracle %.3g px, disp_left %.3g px (gate %.3g)"
          % (e_ini, e_disp, 2e-5 * 512))
    assert e_ini <= 2e-5 * 512 and e_disp <= 2e-5 * 512


@pytest.mark.parametrize("channels", [32, 64])
def test_disp_paths_agree(channels):
    """the three ways forward_parts makes disp_ini_left (fused attend, index-only pass on zero-padded rows, one pass over the
    materialised map) and DCMCS3DI.disparity against the contract on the materialised att_r2l"""
    m = build_model(seed=7, extraction_layers=2, transfer_layers=1, channels=channels).cuda()
    gen = torch.Generator().manual_seed(channels)
    left, right = torch.rand(1, 3, 24, 300, generator=gen).cuda(), torch.rand(1, 3, 24, 300, generator=gen).cuda()
    w = 300
    gate = 2e-5 * w
    pa = m.forward_parts(left, right, want_att=True, want_disp=True)
    ps = m.forward_parts(left, right, want_disp=True)
    ini = dc.expected_index(pa["att_r2l"].cpu().numpy())[:, None]
    disp, valid = m.disparity(left, right)
    for tag, ini_got, disp_got, vmask in (("att", pa["disp_ini_left"], pa["disp_left"], pa["valid_left"]),
                                          ("stream", ps["disp_ini_left"], ps["disp_left"], ps["valid_left"]),
                                          ("disparity()", None, disp, valid)):
        vm = vmask.cpu().numpy() > 0.5
        if ini_got is not None:
            e = np.abs(ini_got.cpu().double().numpy() - ini).max()
            assert e <= gate, (tag, e)
        e = np.abs(disp_got.cpu().double().numpy() - dc.fill(ini, vm, np.float64)).max()
        assert e <= gate, (tag, e)


@pytest.mark.parametrize("h,w", [(512, 512), (1080, 1920)])
def test_want_disp_leaves_every_part_unchanged(h, w):
    m = build_model(seed=11).cuda()
    gen = torch.Generator().manual_seed(h)
    left, right = torch.rand(1, 3, h, w, generator=gen).cuda(), torch.rand(1, 3, h, w, generator=gen).cuda()
    p0 = m.forward_parts(left, right)
    p1 = m.forward_parts(left, right, want_disp=True)
    assert set(p1) == set(p0) | {"disp_ini_left", "disp_left"}
    for k, v in p0.items():
        if v is None:
            assert p1[k] is None, k
        else:
            assert torch.equal(v, p1[k]), k
    assert p1["disp_left"].shape == (1, 1, h, w) and p1["disp_left"].dtype == torch.float32
    assert torch.isfinite(p1["disp_left"]).all()
    corrected, (atts, cyc, valid, warped) = m(left, right, inference=True)
    assert torch.equal(corrected, p0["corrected"]) and torch.equal(warped, p0["warped_rgb"])
    assert atts == (None, None) and cyc == (None, None) and torch.equal(valid[0], p0["valid_left"] > 0.5)
    # the public disparity (index-only pass) against the fused one, same mask
    disp, vmask = m.disparity(left, right)
    assert torch.equal(vmask, p0["valid_left"] > 0.5)
    e = (disp - p1["disp_left"]).abs().max().item()
    print("\n[%dx%d] disparity() vs forward_parts(want_disp) max-abs %.3g px" % (h, w, e))
    assert e <= 2e-5 * w
