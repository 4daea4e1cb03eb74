"""ct_hip.frame_losses (csrc/losses.hip) against float64 restatements of F.l1_loss, F.mse_loss and kornia's ssim_loss(window_size=11)
(tests/augment_common.losses) on frames of the 8-bit grid.

L1 and MSE: the kernel forms the differences in float32 like torch and adds them in float64, so its error against the float64 value
must not exceed that of F.l1_loss / F.mse_loss on the same float32 tensors.  SSIM loss: within twice the error of the float32 torch
restatement, the margin of the error maps (tests/test_errmaps_gpu.py), with the same absolute floor of 1e-6 where the float32
restatement happens to be almost exact.  The test prints the figures (-s).

Measured on an MI355X (error against float64: kernel / torch float32; for the SSIM loss also their ratio):
    2x3x24x40 frame 0   L1 0 / 1.7e-09          MSE 3.9e-12 / 1.2e-10   SSIM loss 3.6e-07 / 6.6e-07 (0.55)
    2x3x24x40 frame 1   L1 2.6e-12 / 2.0e-10    MSE 4.3e-12 / 4.2e-11   SSIM loss 3.1e-07 / 4.7e-07 (0.65)
    1x3x6x6             L1 1.7e-11 / 1.5e-09    MSE 5.4e-12 / 1.4e-11   SSIM loss 1.1e-07 / 5.3e-08 (2.08: under the 1e-6 floor)
    1x3x40x70           L1 5.0e-12 / 4.4e-10    MSE 6.8e-12 / 7.8e-12   SSIM loss 1.2e-08 / 3.7e-09 (3.22: under the 1e-6 floor)"""
import pytest
import torch
import torch.nn.functional as F

from tests import augment_common as ac

pytestmark = pytest.mark.gpu
SHAPES = ((2, 3, 24, 40), (1, 3, 6, 6), (1, 3, 40, 70))          # the last: two 64 x 32 tiles either way, ragged


def _frames(shape, seed):
    """a result and a ground truth on the 8-bit grid: a texture, and the same texture under a gain with some noise"""
    gt = ac.textured_u8(shape, seed)
    g = torch.Generator().manual_seed(seed + 1)
    res = (gt.float() * 0.9 + 12 + torch.randint(-9, 10, gt.shape, generator=g)).clamp(0, 255).to(torch.uint8)
    return res.float() / 255, gt.float() / 255


@pytest.fixture(scope="module")
def cases():
    out = {}
    for shape in SHAPES:
        a, b = _frames(shape, 100 + shape[-1])
        out[shape] = (a, b, ac.losses(a.double(), b.double()), ac.losses(a, b))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_losses_against_float64(cases, shape):
    import ct_hip
    a, b, ref64, ref32 = cases[shape]
    batch, per_frame = ct_hip.frame_losses(a.cuda(), b.cuda())
    assert per_frame.shape == (shape[0], 3) and per_frame.dtype == torch.float64 and batch.shape == (3,)
    got = per_frame.cpu()
    assert torch.equal(batch.cpu(), got.mean(dim=0))                                  # the batch value: the mean of the per-frame values
    assert torch.equal(ct_hip.frame_losses(a.cuda(), b.cuda())[1].cpu(), got)         # deterministic
    for i in range(shape[0]):
        torch32 = (F.l1_loss(a[i], b[i]), F.mse_loss(a[i], b[i]))
        for q, name in enumerate(("L1", "MSE")):
            mine, theirs = abs(float(got[i, q]) - float(ref64[i, q])), abs(float(torch32[q].double()) - float(ref64[i, q]))
            print("%s frame %d of %s: %.6g, error %.3g (torch float32: %.3g)" % (name, i, shape, float(got[i, q]), mine, theirs))
            assert mine <= theirs, (name, i)
        mine, theirs = abs(float(got[i, 2]) - float(ref64[i, 2])), abs(float(ref32[i, 2].double()) - float(ref64[i, 2]))
        print("SSIM loss frame %d of %s: %.6g, error %.3g (torch float32 restatement: %.3g, ratio %.2f)"
              % (i, shape, float(got[i, 2]), mine, theirs, mine / theirs if theirs else float("inf")))
        assert mine <= max(2.0 * theirs, 1e-6), i
        assert 0 < float(got[i, 2]) < 0.5 and float(got[i, 1]) < float(got[i, 0])


def test_identical_frames_lose_nothing():
    import ct_hip
    a, _ = _frames((2, 3, 24, 40), 7)
    a = a.clamp(min=64 / 255).cuda()                          # bright enough for the 1e-12 of the denominator to vanish in float32
    batch, per_frame = ct_hip.frame_losses(a, a.clone())
    assert not per_frame.any() and not batch.any()


def test_binding_and_abi_refusals():
    import ctypes
    import ct_hip
    from ct_hip import _core
    x = torch.rand(2, 3, 24, 40, generator=torch.Generator().manual_seed(1)).cuda()
    for bad in ((x, x[:, :, :, :39].contiguous()), (x, x.double()), (x[:, :, :, ::2], x[:, :, :, ::2]), (x[:, :2].contiguous(), x[:, :2].contiguous()),
                (x[:, :, :5].contiguous(), x[:, :, :5].contiguous()), (x[:, :, :, :5].contiguous(), x[:, :, :, :5].contiguous())):
        with pytest.raises(ct_hip.CtHipError):
            ct_hip.frame_losses(*bad)
    lib = ct_hip.lib()
    need = lib.ct_frame_losses_workspace_bytes(2, 24, 40)
    assert need == 2 * 1 * 1 * 3 * 8 and lib.ct_frame_losses_workspace_bytes(1, 33, 65) == 2 * 2 * 3 * 8
    out = torch.full((2, 3), -1.0, dtype=torch.float64, device="cuda")
    ws = torch.zeros(64, dtype=torch.float64, device="cuda")
    p, null, s = _core._ptr, ctypes.c_void_p(0), _core._stream()
    assert lib.ct_frame_losses_f32(null, p(x), p(out), p(ws), need, 2, 24, 40, s) == -1
    assert lib.ct_frame_losses_f32(p(x), p(x), null, p(ws), need, 2, 24, 40, s) == -1
    assert lib.ct_frame_losses_f32(p(x), p(x), p(out), p(ws), need, 0, 24, 40, s) == -1
    assert lib.ct_frame_losses_f32(p(x), p(x), p(out), p(ws), need, 2, 5, 40, s) == -1
    assert lib.ct_frame_losses_f32(p(x), p(x), p(out), p(ws), need, 2, 24, 5, s) == -1
    assert lib.ct_frame_losses_f32(p(x), p(x), p(out), null, need, 2, 24, 40, s) == -2
    assert lib.ct_frame_losses_f32(p(x), p(x), p(out), p(ws), need - 1, 2, 24, 40, s) == -2
    assert lib.ct_frame_losses_f32(p(x), p(x), p(out), ctypes.c_void_p(ws.data_ptr() + 4), need, 2, 24, 40, s) == -2
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())                          # nothing was launched
