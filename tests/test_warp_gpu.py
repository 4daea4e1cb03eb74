"""ct_hip.warp_perspective (csrc/warp.hip) and utils.postprocess on the GPU: the bytes must EQUAL the numpy restatement of the
rule (tests/warp_common.py, which tests/test_warp_host.py holds to the float64 oracle) on every path of the kernel -- staged and
global taps, 16-byte and element stores -- at the sizes where cv2's block grid changes, and at the rule's edges (ties, W == 0,
saturation).  Small shapes: every case is a handful of launches."""
import json
import os

import numpy as np
import pytest
import torch

from tests import warp_common as wc

pytestmark = pytest.mark.gpu

WIDTHS = (1, 63, 64, 65, 130)           # the x0 block boundaries (bw0 = 64 when the crop is 16 rows or more)
HEIGHTS = (1, 15, 16, 17)               # bh0 < 16 changes bw0
MATRICES = {"identity": lambda h, w: wc.IDENTITY, "near": wc.near_identity, "strong": wc.strong}


def _raw(h, w, seed, n=1):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _warp(raw, maps, **kw):
    import ct_hip
    return ct_hip.warp_perspective(_gpu(raw), maps, inverse_map=True, **kw).cpu().numpy()


@pytest.mark.parametrize("kind", sorted(MATRICES))
def test_block_grid_sizes_equal_the_restatement(kind):
    """every width x height of the block grid, as a crop of a wider frame whose rows are on the 16-byte grid (where path="staged"
    does stage; the default takes global taps) and as a whole frame of exactly that size"""
    for h in HEIGHTS:
        for w in WIDTHS:
            m = MATRICES[kind](h, w)
            wide = _raw(h + 5, (w + 9 + 15) // 16 * 16, seed=h * 1000 + w)
            crop = (7, 3, w, h)
            want = wc.warp_frames(wide, m, crop=crop)
            for path in ("staged", None):
                assert np.array_equal(_warp(wide, m, crop=crop, path=path), want), (kind, h, w, "crop", path)
            whole = _raw(h, w, seed=h * 1000 + w + 1)
            assert np.array_equal(_warp(whole, m), wc.warp_frames(whole, m)), (kind, h, w, "whole")


def test_strong_map_on_a_box_beyond_the_lds_budget():
    """130 x 48 with the strong map: the source box of the first tiles is the whole crop, 48 rows of 400 bytes, more than the
    16 KB the staged path holds -- those tiles take their taps from memory inside the staged kernel"""
    raw = _raw(52, 144, seed=5)
    crop = (9, 2, 130, 48)
    m = wc.strong(48, 130)
    want = wc.warp_frames(raw, m, crop=crop)
    assert want.any()
    for path in ("staged", "global"):
        assert np.array_equal(_warp(raw, m, crop=crop, path=path), want), path


def test_batch_of_three_maps_equals_three_calls_and_shared_flag():
    raw = _raw(40, 144, seed=7, n=3)
    crop = (5, 1, 130, 37)
    maps = np.stack([wc.near_identity(37, 130), wc.strong(37, 130), wc.IDENTITY])
    got = _warp(raw, maps, crop=crop)
    for k in range(3):
        assert np.array_equal(got[k], _warp(raw[k], maps[k], crop=crop)), k
    assert np.array_equal(got, wc.warp_frames(raw, maps, crop=crop))
    shared = _warp(raw, maps[0], crop=crop)
    assert np.array_equal(shared, wc.warp_frames(raw, maps[0], crop=crop))
    assert np.array_equal(shared[0], got[0]) and not np.array_equal(shared[1], got[1])


@pytest.mark.parametrize("crop", [None, (8, 4, 40, 20)])
def test_flip_and_taps_outside_the_crop_read_zero(crop):
    """a white raw frame, the source shifted by 3.5 px: the last columns of the destination reach past the crop's right edge --
    where the raw frame still has (white) pixels when the crop is offset -- and must read 0; then noise against the restatement"""
    shift = np.array([[1.0, 0, 3.5], [0, 1.0, 0], [0, 0, 1.0]])
    white = np.full((1, 32, 64, 3), 255, dtype=np.uint8)
    w = 64 if crop is None else crop[2]
    for flip in (False, True):
        got = _warp(white, shift, crop=crop, flip_x=flip)
        assert (got[:, :, :w - 4] == 255).all() and (got[:, :, w - 4] == 128).all() and (got[:, :, w - 3:] == 0).all(), flip
        noise = _raw(32, 64, seed=11, n=2)
        for m in (shift, wc.near_identity(32, w)):
            for path in ("staged", "global"):
                assert np.array_equal(_warp(noise, m, crop=crop, flip_x=flip, path=path), wc.warp_frames(noise, m, crop=crop, flip_x=flip)), (flip, path)
    flipped = _warp(_raw(32, 64, seed=12), wc.IDENTITY, crop=crop, flip_x=True)
    assert np.array_equal(flipped, wc.source_crop(_raw(32, 64, seed=12)[0], crop, True)[None])


def test_window_off_the_grid_and_misaligned_out_take_the_element_path():
    import ct_hip
    raw = _raw(40, 144, seed=13, n=2)
    crop = (5, 1, 130, 37)
    m = wc.near_identity(37, 130)
    for window in ((3, 2, 37, 9), (64, 16, 66, 21), (0, 0, 128, 37)):
        want = wc.warp_frames(raw, m, crop=crop, window=window)
        assert np.array_equal(_warp(raw, m, crop=crop, window=window), want), window
        x, y, w, h = window
        buf = torch.zeros(2 * h * w * 3 + 8, dtype=torch.uint8, device="cuda")
        out = buf[4:4 + 2 * h * w * 3]                           # base 4 bytes off the grid
        got = ct_hip.warp_perspective(_gpu(raw), m, crop=crop, window=window, inverse_map=True, out=out)
        assert got.data_ptr() == out.data_ptr() and np.array_equal(got.cpu().numpy(), want), window
        assert not buf[:4].any() and not buf[-4:].any()


def test_ties_round_to_even():
    """M2 = 1/64: fX = 32 c + 0.5 -> X = 32 c (even), the source itself; rounding the tie up would blend 1/32 of the next column,
    2 grey levels on steps of 64.  M2 = 3/64: fX = 32 c + 1.5 -> 32 c + 2."""
    cols = (np.arange(96) % 4 * 64).astype(np.uint8)
    raw = np.broadcast_to(cols[None, None, :, None], (1, 20, 96, 3)).copy()
    got = _warp(raw, np.array([[1.0, 0, 1 / 64], [0, 1.0, 0], [0, 0, 1.0]]))
    assert np.array_equal(got, raw)
    got = _warp(raw, np.array([[1.0, 0, 3 / 64], [0, 1.0, 0], [0, 0, 1.0]]))
    p0 = raw[0].astype(np.int64)
    p1 = np.concatenate([p0[:, 1:], np.zeros_like(p0[:, :1])], axis=1)
    assert np.array_equal(got[0], ((30 * 32 * p0 + 2 * 32 * p1 + 512) >> 10).astype(np.uint8))


def test_w_zero_reads_the_first_pixel():
    raw = _raw(20, 64, seed=17)
    m = np.array([[1.0, 0, 0], [0, 1.0, 0], [1.0, 0, -5.0]])
    got = _warp(raw, m)
    assert (got[0, :, 5] == raw[0, 0, 0]).all()
    assert np.array_equal(got, wc.warp_frames(raw, m))


def test_saturation_is_all_zero():
    """a scale of 1e12 with a translation of +-1e15: every coordinate saturates far outside, both signs in one call"""
    raw = _raw(20, 80, seed=19, n=2)
    maps = np.array([[[1e12, 0, 1e15], [0, 1e12, -1e15], [0, 0, 1.0]], [[1e12, 0, -1e15], [0, 1e12, 1e15], [0, 0, 1.0]]])
    got = _warp(raw, maps)
    assert not got.any() and np.array_equal(got, wc.warp_frames(raw, maps))


def test_staged_and_global_taps_give_identical_bytes():
    raw = _raw(44, 144, seed=23, n=2)
    crop = (6, 2, 130, 40)
    m = wc.near_identity(40, 130)
    for flip in (False, True):
        staged = _warp(raw, m, crop=crop, flip_x=flip, path="staged")
        assert np.array_equal(staged, _warp(raw, m, crop=crop, flip_x=flip, path="global")), flip
        assert np.array_equal(staged, _warp(raw, m, crop=crop, flip_x=flip)), flip
        assert np.array_equal(staged, wc.warp_frames(raw, m, crop=crop, flip_x=flip)), flip


def _sample_frames():
    left, gt, right = (_raw(48, 80, seed=s, n=2) for s in (29, 31, 37))
    h1 = np.array([[1.02, 0.01, -0.7], [-0.02, 0.98, 0.9], [1e-5, -2e-5, 1.0]])
    h2 = np.array([[0.97, -0.03, 1.1], [0.01, 1.03, -0.4], [-1e-5, 3e-5, 1.0]])
    return left, gt, right, h1, h2, (4, 6, 64, 36)


def test_process_frames_equals_the_public_pieces():
    import ct_hip
    from utils import postprocess as pp
    left, gt, right, h1, h2, bbox = _sample_frames()
    x, y, w, h = bbox
    dl, dg, dr = _gpu(left), _gpu(gt), _gpu(right)
    ld, l, r = pp.process_frames(dl, dg, dr, h1, h2, bbox)
    assert tuple(ld.shape) == tuple(l.shape) == tuple(r.shape) == (2, 36 - 6, 64 - 4, 3)
    assert ld.dtype == l.dtype == r.dtype == torch.uint8
    # the reference's own order: flip, crop, warp to the crop's size, crop again
    flipped_crop = dl.flip(2)[:, y:y + h, x:x + w].contiguous()
    assert torch.equal(ld, ct_hip.warp_perspective(flipped_crop, h1)[:, y:y + h, x:x + w])
    assert np.array_equal(ld.cpu().numpy(), wc.warp_frames(left, ct_hip.invert3x3(h1), crop=bbox, flip_x=True, window=(x, y, w - x, h - y)))
    assert np.array_equal(l.cpu().numpy(), gt[:, y:y + h, x:x + w][:, y:y + h, x:x + w])
    warped = ct_hip.warp_perspective(dr[:, y:y + h, x:x + w].contiguous(), h2)[:, y:y + h, x:x + w].contiguous()
    assert np.array_equal(warped.cpu().numpy(), wc.warp_frames(right, ct_hip.invert3x3(h2), crop=bbox, window=(x, y, w - x, h - y)))
    assert torch.equal(r, ct_hip.mk(warped, l, out_dtype=torch.uint8))


@pytest.mark.parametrize("encoder", ["host", "device"])
def test_cli_writes_what_process_frames_returns(tmp_path, encoder):
    from PIL import Image
    from utils import postprocess as pp
    left, gt, right, h1, h2, bbox = _sample_frames()
    root, out = str(tmp_path / "in"), str(tmp_path / "out")
    for name, frames in (("left", left), ("left_gt", gt), ("right", right)):
        os.makedirs(os.path.join(root, "s0", name))
        for k, frame in enumerate(frames):
            Image.fromarray(frame).save(os.path.join(root, "s0", name, "%03d.png" % k))
    with open(os.path.join(root, "s0", "params.json"), "w") as f:
        json.dump({"bbox": dict(zip("xywh", bbox)), "offsets": {"all": 0, "left": 0, "left_gt": 0, "right": 0},
                   "homographies": {"left": h1.tolist(), "right": h2.tolist()}}, f)
    assert pp.main(["--root", root, "--output", out, "--rate", "1", "--frames", "2", "--png_encoder", encoder]) == 0
    want = pp.process_frames(_gpu(left), _gpu(gt), _gpu(right), h1, h2, bbox)
    assert sorted(os.listdir(os.path.join(out, "s0"))) == sorted("%04d_%s.png" % (k, t) for k in range(2) for t in ("LD", "L", "R"))
    for tag, frames in zip(("LD", "L", "R"), want):
        for k in range(2):
            got = np.asarray(Image.open(os.path.join(out, "s0", "%04d_%s.png" % (k, tag))))
            assert np.array_equal(got, frames[k].cpu().numpy()), (tag, k)
