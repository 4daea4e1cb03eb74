"""CPU-only checks of the perspective warp (csrc/warp.hip, ct_hip/warp.py, utils/postprocess.py): the numpy restatement of the
rule against the float64 oracle within the derived bound (tests/warp_common.py), the host 3 x 3 inverse, the argument checks of
the C entry and of the Python layer, and the command line's frame selection with the device calls stubbed out."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import warp_common as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("h,w", wc.SHAPES)
def test_restatement_within_the_derived_bound_of_the_float64_oracle(h, w):
    for name, img in wc.images(h, w).items():
        for label, m in (("identity", wc.IDENTITY), ("near", wc.near_identity(h, w)), ("strong", wc.strong(h, w))):
            got = wc.warp_fixed(img, m).astype(np.float64)
            exact, bound = wc.warp_exact(img, m)
            err = np.abs(got - exact)
            worst = np.unravel_index(np.argmax(err - bound), err.shape)
            print("%dx%d %s %s: max err %.3f, at the worst margin err %.3f bound %.3f" % (h, w, name, label, err.max(), err[worst], bound[worst]))
            assert (err <= bound).all(), (h, w, name, label, worst, err[worst], bound[worst])


@pytest.mark.parametrize("h,w", wc.SHAPES + ((1, 1), (1, 130), (17, 1)))
def test_identity_is_exact(h, w):
    img = wc.images(h, w)["noise"]
    assert np.array_equal(wc.warp_fixed(img, wc.IDENTITY), img)
    assert np.array_equal(wc.warp_fixed(img, wc.IDENTITY, window=(w // 2, h // 3, w - w // 2, h - h // 3)), img[h // 3:, w // 2:])


def test_host_inverse_is_cv2s_closed_form():
    import ct_hip
    rng = np.random.default_rng(3)
    for _ in range(20):
        m = np.eye(3) + 0.3 * rng.standard_normal((3, 3))
        if np.linalg.cond(m) > 50:
            continue
        inv = ct_hip.invert3x3(m)
        assert inv.dtype == np.float64 and np.abs(inv - np.linalg.inv(m)).max() <= 1e-12 * np.abs(np.linalg.inv(m)).max()
    singular = np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.5, 0.25, 1.0]])
    assert np.array_equal(ct_hip.invert3x3(singular), np.zeros((3, 3)))
    maps, shared = ct_hip.warp_maps(np.diag([2.0, 4.0, 1.0]), 3)
    assert shared and maps.shape == (1, 9) and np.array_equal(maps[0], [0.5, 0, 0, 0, 0.25, 0, 0, 0, 1.0])
    maps, shared = ct_hip.warp_maps(np.stack([np.eye(3)] * 3), 3, inverse_map=True)
    assert not shared and maps.shape == (3, 9)


def test_symbol_exported_and_declared():
    import ct_hip
    assert "ct_warp_perspective_u8" in ct_hip.SIGNATURES
    assert hasattr(ctypes.CDLL(ct_hip.LIB_PATH), "ct_warp_perspective_u8")
    header = open(os.path.join(ROOT, "include", "ct_hip.h")).read()
    assert re.search(r"\bint ct_warp_perspective_u8\(", header)
    for name in ("CT_WARP_AUTO", "CT_WARP_STAGED", "CT_WARP_GLOBAL"):
        assert re.search(r"#define %s %d\b" % (name, getattr(ct_hip, name)), header)
    assert callable(ct_hip.warp_perspective)
    assert "warp.hip" in open(os.path.join(ROOT, "color-transfer_amd", "csrc", "Makefile")).read()


def test_c_entry_refuses_bad_arguments_without_a_gpu():
    """every CT_E_BADARG / CT_E_ALIGN case of the header returns before anything touches the device (there is none here)"""
    import ct_hip
    fn = ct_hip.lib().ct_warp_perspective_u8
    host = (ctypes.c_char * 256)()
    p = ctypes.c_void_p((ctypes.addressof(host) + 15) & ~15)
    good = dict(raw=p, n=1, src_h=40, src_w=60, flip_x=0, crop_x=4, crop_y=6, crop_w=50, crop_h=30, maps=p, shared=1,
                out_x=2, out_y=3, out_w=40, out_h=20, out=p, path=0, stream=None)

    def call(**change):
        a = dict(good, **change)
        return fn(*[a[k] for k in good])
    bad = [dict(raw=None), dict(maps=None), dict(out=None), dict(n=0), dict(src_h=0), dict(src_w=0), dict(crop_w=0), dict(crop_h=0),
           dict(out_w=0), dict(out_h=0), dict(n=-1), dict(out_w=-3),
           dict(crop_x=-1), dict(crop_y=-1), dict(crop_x=11), dict(crop_y=11), dict(crop_w=61, crop_x=0), dict(crop_h=41, crop_y=0),
           dict(out_x=-1), dict(out_y=-1), dict(out_x=11), dict(out_y=11), dict(out_w=51, out_x=0), dict(out_h=31, out_y=0),
           dict(src_w=40000, crop_x=0, crop_w=32768), dict(src_h=40000, crop_y=0, crop_h=32768),
           dict(crop_x=2 ** 31 - 1), dict(out_x=2 ** 31 - 1), dict(path=3), dict(path=-1)]
    for change in bad:
        assert call(**change) == -1, change
    assert call(maps=ctypes.c_void_p(p.value + 4)) == -3
    assert call(maps=ctypes.c_void_p(p.value + 1)) == -3
    assert call(maps=None, out=ctypes.c_void_p(p.value + 4)) == -1          # the null pointer wins over anything later


def test_python_layer_value_errors():
    import ct_hip
    frames = torch.zeros((2, 40, 60, 3), dtype=torch.uint8)
    eye = np.eye(3)
    bad_m = eye.copy()
    bad_m[1, 2] = np.nan
    inf_m = eye.copy()
    inf_m[0, 0] = np.inf
    for kw in (dict(matrices=bad_m), dict(matrices=inf_m), dict(matrices=np.eye(4)), dict(matrices=np.stack([eye] * 3)),
               dict(crop=(0, 0, 61, 40)), dict(crop=(-1, 0, 10, 10)), dict(crop=(0, 0, 0, 10)), dict(crop=(0, 0, 10)), dict(crop=(0, 0, 10.0, 10)),
               dict(window=(0, 0, 61, 40)), dict(crop=(4, 6, 50, 30), window=(0, 0, 51, 30)), dict(window=(0, -1, 10, 10)), dict(window=(5, 5, 0, 1)),
               dict(path="lds")):
        args = dict(matrices=eye)
        args.update(kw)
        with pytest.raises(ValueError):
            ct_hip.warp_perspective(frames, **args)
    for frames_bad in (torch.zeros((2, 40, 60, 3)), torch.zeros((40, 60, 4), dtype=torch.uint8), torch.zeros((40, 60), dtype=torch.uint8),
                       np.zeros((40, 60, 3), np.uint8), torch.zeros((0, 40, 60, 3), dtype=torch.uint8)):
        with pytest.raises(ValueError):
            ct_hip.warp_perspective(frames_bad, eye)
    if not torch.cuda.is_available():
        with pytest.raises(ct_hip.CtHipError):                              # valid arguments, host frames: no CPU path
            ct_hip.warp_perspective(frames, eye)
    from utils import postprocess as pp
    for bbox in ((64, 6, 64, 36), (4, 36, 64, 36), (70, 6, 64, 36), (-1, 6, 64, 36)):
        with pytest.raises(ValueError):
            pp.process_frames(frames, frames, frames, eye, eye, bbox)
    assert pp.second_crop((4, 6, 64, 36)) == (4, 6, 60, 30)


def _fake_sample(root, name, n_frames, offsets, bbox, size=(20, 24)):
    from PIL import Image
    d = os.path.join(root, name)
    for s in ("left", "left_gt", "right"):
        os.makedirs(os.path.join(d, s))
        for i in range(n_frames):
            Image.fromarray(np.full(size + (3,), i, dtype=np.uint8)).save(os.path.join(d, s, "f%03d.png" % i))
    with open(os.path.join(d, "params.json"), "w") as f:
        json.dump({"bbox": dict(zip("xywh", bbox)), "offsets": offsets,
                   "homographies": {"left": np.eye(3).tolist(), "right": (2 * np.eye(3)).tolist()}}, f)


def test_cli_frame_selection_with_the_device_calls_stubbed(tmp_path, monkeypatch):
    """rate, frames and the offsets pick the frames, every sample is one process_frames call, the files carry the reference's
    names; process_frames itself is a stub that returns the first pixel of each stream's frames (their index in the stream)"""
    from PIL import Image
    from utils import postprocess as pp
    root, out = str(tmp_path / "in"), str(tmp_path / "out")
    _fake_sample(root, "a", 40, {"all": 2, "left": 1, "left_gt": 0, "right": 3}, (1, 2, 12, 10))
    _fake_sample(root, "b", 9, {"all": 0, "left": 0, "left_gt": 0, "right": 4}, (0, 0, 8, 8))
    calls = []

    def stub(left, left_gt, right, H1, H2, bbox):
        calls.append((tuple(left.shape), H1.tolist(), H2.tolist(), tuple(bbox)))
        return tuple(t[:, :4, :5].contiguous() for t in (left, left_gt, right))
    monkeypatch.setattr(pp, "process_frames", stub)
    monkeypatch.setattr(pp, "load_frames", lambda paths, device: torch.from_numpy(np.stack([np.asarray(Image.open(p)) for p in paths])))
    assert pp.main(["--root", root, "--output", out, "--rate", "5", "--frames", "4"]) == 0
    assert [c[0] for c in calls] == [(4, 20, 24, 3), (1, 20, 24, 3)]        # b: right ends after frame_idx 0 (4 + 5 >= 9)
    assert calls[0][1] == np.eye(3).tolist() and calls[0][2] == (2 * np.eye(3)).tolist() and calls[0][3] == (1, 2, 12, 10)
    assert sorted(os.listdir(os.path.join(out, "a"))) == sorted("%04d_%s.png" % (k, t) for k in range(4) for t in ("LD", "L", "R"))
    assert sorted(os.listdir(os.path.join(out, "b"))) == ["0000_L.png", "0000_LD.png", "0000_R.png"]
    for k in range(4):                                                      # frame_idx 5 k of a: left 3 + 5 k, left_gt 2 + 5 k, right 5 + 5 k
        for tag, first in (("LD", 3), ("L", 2), ("R", 5)):
            got = np.asarray(Image.open(os.path.join(out, "a", "%04d_%s.png" % (k, tag))))
            assert got.shape == (4, 5, 3) and (got == first + 5 * k).all(), (k, tag, got[0, 0])
    calls.clear()
    assert pp.main(["--root", root, "--output", out, "--samples", "b", "--rate", "2", "--frames", "7"]) == 0
    assert [c[0] for c in calls] == [(3, 20, 24, 3)]                        # frame_idx 0, 2, 4: right 4, 6, 8; frame_idx 6 would need right 10
    picks = pp.select_frames({"offsets": {"all": 1, "left": 0, "left_gt": 2, "right": 0}}, {"left": 100, "left_gt": 100, "right": 100}, 10, 7)
    assert [n for n, _ in picks] == list(range(7)) and picks[3][1] == {"left": 31, "left_gt": 33, "right": 31}
    with pytest.raises(ValueError):
        pp.select_frames({"offsets": {"all": 0, "left": 0, "left_gt": 0, "right": 0}}, {"left": 1, "left_gt": 1, "right": 1}, 0, 7)
