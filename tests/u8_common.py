"""What the GPU tests of the entries on uint8 frame groups share (tests/test_linear_u8_gpu.py, test_idt_u8_gpu.py,
test_acg_u8_gpu.py): uploads, bitwise comparison, the image that bytes stand for, seeded rotations, and the per-frame Runner route
that the grouped routes are held to."""
import numpy as np
import pytest

from oracle import iterative as oit

torch = pytest.importorskip("torch")

ULP = 2.0 ** -53


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()


def bits(t):
    """an integer view: equal bits, a NaN for the same NaN"""
    return t.view({torch.float64: torch.int64, torch.float32: torch.int32}.get(t.dtype, t.dtype))


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


def image(k, f32):
    """the float image the bytes stand for"""
    return k.astype(np.float32) / np.float32(255) if f32 else k / 255.0


def rotations(n_iter, seed, batch=None):
    np.random.seed(seed)
    return oit.draw_rotations(n_iter) if batch is None else np.stack([oit.draw_rotations(n_iter) for _ in range(batch)])


def psnr_close(got, want, n):
    """PSNR values of mse values that agree within 3 n 2^-53 relative: d(10 log10(1 / mse)) = 10 / ln 10 * d(mse) / mse, plus the
    1e-12 relative that test_mk_psnr allows for the logarithm itself"""
    got, want = np.asarray(got), np.asarray(want)
    return bool((np.abs(got - want) <= 10 / np.log(10) * 3 * n * ULP + 1e-12 * np.maximum(1.0, np.abs(want))).all())


def grouped_frames(video, n_frames):
    """the frames as the grouped route sees them (a group's content is defined by its first frame): [(target, reference, gt)] uint8 HWC"""
    out = []
    for first in range(0, n_frames, video.group):
        chunk = video.host_chunk(first)
        out += [tuple(chunk[i, j] for i in range(3)) for j in range(min(video.group, n_frames - first))]
    return out


def per_frame_route(spec, triples, seed, skip=0):
    """the per-frame Runner of `spec` (forward, clamp, pack_u8; test_step) on a seeded np.random, for uint8 HWC (target, reference, gt)
    triples made float32 CHW as the datasets make them: (bytes [n,H,W,3], rows [n,2] of (mse, PSNR) as methods.psnr computes them);
    skip: that many frames' draws discarded first"""
    import ct_hip
    import methods.iterative as it
    from methods import Runner
    model = Runner(spec, metrics="psnr")
    assert not model.takes_groups()
    batches = [{k: (x.permute(2, 0, 1).float() / 255)[None].cuda() for k, x in zip(("target", "reference", "gt"), tr)} for tr in triples]
    np.random.seed(seed)
    it.draw_group_rotations(skip)
    frames_u8 = [ct_hip.pack_u8(model(b).clamp(0, 1).contiguous(), "chw")[0].cpu().numpy() for b in batches]
    np.random.seed(seed)
    it.draw_group_rotations(skip)
    rows = [ct_hip.frame_psnr(model(b).clamp(0, 1).float().contiguous(), b["gt"].float().contiguous())[0].cpu().numpy() for b in batches]
    return np.stack(frames_u8), np.stack(rows)
