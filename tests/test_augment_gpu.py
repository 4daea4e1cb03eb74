"""ct_hip.augment_u8 (csrc/augment.hip) on the GPU: single operations against ct_hip.distort_u8 and the CPU restatement of
adjust_sharpness, the crop / flip geometry against slicing, chains of exact operations against the CPU chain, every chain against the
kernel's own single-operation calls fed one into the next, and the error codes.  Everything is compared bit for bit."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests import augment_common as ac

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import ct_hip
    ct_hip.lib()
    return ct_hip


@pytest.fixture(scope="module")
def frame():
    """the 271 x 483 image of tests/test_data_path.py's recipe and a second view, uint8 [1,3,271,483] on the host"""
    return ac.textured_u8((1, 3, 271, 483), 3), ac.textured_u8((1, 3, 271, 483), 4)


@pytest.fixture(scope="module")
def pair():
    """source pairs of 37 x 53, uint8 [2,3,37,53] on the host"""
    return ac.textured_u8((2, 3, 37, 53), 11), ac.textured_u8((2, 3, 37, 53), 12)


def _run(hip, gt, ref, params, crop):
    out = hip.augment_u8(gt.cuda(), ref.cuda(), params, crop, want_u8=True)
    out = {k: v.cpu() for k, v in out.items()}
    assert torch.equal(out["target"], out["target_u8"].float() / 255)                 # the float32 division of the uint8 target
    return out


# ---- 1. single operations -------------------------------------------------------------------------------------------------------------
SINGLE = [("identity", 0.0), ("brightness", 0.5), ("brightness", 1.3), ("contrast", 0.5), ("contrast", 1.5), ("saturation", 0.7),
          ("saturation", 1.5), ("hue", -0.5), ("hue", 0.1), ("hue", 0.5), ("gamma", 0.5), ("gamma", 1.3)]


def test_kinds_0_to_5_are_distort_u8_bit_for_bit(hip, frame):
    gt, ref = frame
    dev = gt[0].cuda()
    params = [ac.params(ops=[op]) for op in SINGLE]
    # one call for all of them: the same frame twelve times, a different chain per sample
    out = _run(hip, gt.expand(len(SINGLE), -1, -1, -1).contiguous(), ref.expand(len(SINGLE), -1, -1, -1).contiguous(), params, (271, 483))
    for i, (kind, value) in enumerate(SINGLE):
        want_f, want_u = hip.distort_u8(dev, kind, value, want_u8=True)
        assert torch.equal(out["target_u8"][i], want_u.cpu()) and torch.equal(out["target"][i], want_f.cpu()), (kind, value)
        assert torch.equal(out["gt"][i], gt[0].float() / 255) and torch.equal(out["reference"][i], ref[0].float() / 255)


def test_sharpness_is_the_cpu_restatement_bit_for_bit(hip, frame):
    gt, ref = frame
    factors = (0.0, 0.5, 1.0, 1.5, 2.0)
    out = _run(hip, gt.expand(5, -1, -1, -1).contiguous(), ref.expand(5, -1, -1, -1).contiguous(),
               [ac.params(ops=[("sharpness", f)]) for f in factors], (271, 483))
    for i, f in enumerate(factors):
        assert torch.equal(out["target_u8"][i], ac.adjust_sharpness(gt[0], f)), f
    assert torch.equal(out["target_u8"][2], gt[0])


# ---- 2. geometry ----------------------------------------------------------------------------------------------------------------------
CROPS = [((19, 23), (0, 0)), ((19, 23), (18, 30)), ((19, 23), (7, 11)), ((3, 3), (34, 50)), ((2, 7), (5, 46)), ((7, 2), (30, 0)), ((1, 1), (36, 52)),
         ((37, 53), (0, 0))]


@pytest.mark.parametrize("crop,corner", CROPS, ids=["%dx%d_at_%d_%d" % (c + k) for c, k in CROPS])
def test_crop_and_flips_are_slicing(hip, pair, crop, corner):
    gt, ref = pair
    flips = list(itertools.product((False, True), repeat=2))
    params = [ac.params(corner[0], corner[1], s, v) for s, v in flips]
    for b in range(2):
        out = _run(hip, gt[b:b + 1].expand(4, -1, -1, -1).contiguous(), ref[b:b + 1].expand(4, -1, -1, -1).contiguous(), params, crop)
        for i, p in enumerate(params):
            g, r = ac.geometry(gt[b], ref[b], p, crop)
            assert torch.equal(out["gt"][i], g.float() / 255) and torch.equal(out["reference"][i], r.float() / 255), p
            assert torch.equal(out["target_u8"][i], g), p                               # the identity chain


# ---- 3. chains of exact operations against the CPU chain -------------------------------------------------------------------------------
def test_exact_chains_are_the_cpu_chain(hip, pair):
    gt, ref = pair
    ops = {"brightness": 1.3, "saturation": 0.6, "sharpness": 1.7}
    orders = list(itertools.permutations(ops))
    flips = list(itertools.product((False, True), repeat=2))
    params = [ac.params(3 + i, 2 * i, *flips[i % 4], ops=[(k, ops[k]) for k in order]) for i, order in enumerate(orders)]
    src = [i % 2 for i in range(len(orders))]
    out = _run(hip, gt[src].contiguous(), ref[src].contiguous(), params, (19, 23))
    for i, p in enumerate(params):
        g, r, t = ac.sample(gt[src[i]], ref[src[i]], p, (19, 23))
        assert torch.equal(out["target_u8"][i], t), p
        assert torch.equal(out["gt"][i], g.float() / 255) and torch.equal(out["reference"][i], r.float() / 255)


# ---- 4. every chain against the kernel's own single operations ------------------------------------------------------------------------
V = {"identity": 0.0, "brightness": 1.25, "contrast": 0.7, "saturation": 1.4, "hue": -0.2, "gamma": 0.8, "sharpness": 1.6}


def _chain(*kinds):
    return [(k, V[k]) for k in kinds]


# every kind first and last; sharpness directly before and directly after contrast; contrast first and last; different lengths
CHAINS = [
    _chain("contrast", "sharpness", "hue", "gamma", "saturation", "brightness"),
    _chain("brightness", "gamma", "sharpness", "contrast", "hue", "saturation"),
    _chain("saturation", "hue", "brightness", "gamma", "sharpness", "contrast"),
    _chain("hue", "brightness", "saturation", "contrast", "sharpness", "gamma"),
    _chain("gamma", "saturation", "contrast", "brightness", "hue", "sharpness"),
    _chain("sharpness", "contrast", "gamma", "saturation", "brightness", "hue"),
    _chain("identity", "contrast", "identity"),
    _chain("sharpness"),
    [],
    _chain("contrast", "contrast", "sharpness", "contrast"),          # the interface does not need the kinds to differ
    _chain("hue", "identity"),
    _chain("gamma", "contrast"),
]


def _composition(hip, gt, ref, params, crop):
    """the same samples from single-operation calls: the geometry with the identity chain, then one call per operation on the uint8
    result of the one before, without crop or flips"""
    n = len(params)
    cur = hip.augment_u8(gt, ref, [dict(p, ops=[]) for p in params], crop, want_u8=True)["target_u8"]
    for k in range(max(len(p["ops"]) for p in params)):
        step = [ac.params(ops=p["ops"][k:k + 1]) for p in params]
        cur = hip.augment_u8(cur, cur, step, crop, want_u8=True)["target_u8"]
    assert cur.shape == (n, 3) + tuple(crop)
    return cur


@pytest.mark.parametrize("crop", [(21, 75), (3, 3)], ids=["three_by_three_tiles_ragged", "3x3"])
def test_chains_are_the_composition_of_single_operations(hip, pair, crop):
    gt, ref = pair                                           # 21 x 75: 8 + 8 + 5 rows, 32 + 32 + 11 columns of the 32 x 8 tile
    big = (ac.textured_u8((2, 3, 40, 90), 21).cuda(), ac.textured_u8((2, 3, 40, 90), 22).cuda()) if crop[1] > 53 else (gt.cuda(), ref.cuda())
    height, width = big[0].shape[2:]
    flips = list(itertools.product((False, True), repeat=2))
    for first in (0, 6):                                     # two batches: their samples differ in order and in length
        chains = CHAINS[first:first + 6]
        params = [ac.params((5 * i) % (height - crop[0] + 1), (7 * i) % (width - crop[1] + 1), *flips[i % 4], ops=c) for i, c in enumerate(chains)]
        src = [i % 2 for i in range(len(chains))]
        g, r = big[0][src].contiguous(), big[1][src].contiguous()
        out = hip.augment_u8(g, r, params, crop, want_u8=True)
        want = _composition(hip, g, r, params, crop)
        for i in range(len(chains)):
            assert torch.equal(out["target_u8"][i], want[i]), (crop, chains[i])
        assert torch.equal(out["target"].cpu(), out["target_u8"].cpu().float() / 255)   # on the host: a true float32 division
        again = hip.augment_u8(g, r, params, crop, want_u8=True)
        assert all(torch.equal(out[k], again[k]) for k in out)                         # two runs of one call


def test_binding_checks(hip, pair):
    gt, ref = (t.cuda() for t in pair)
    with pytest.raises(hip.CtHipError):
        hip.augment_u8(gt, ref, [ac.params()], (19, 23))                               # two pairs, one record
    with pytest.raises(hip.CtHipError):
        hip.augment_u8(gt.float(), ref.float(), [ac.params()] * 2, (19, 23))
    with pytest.raises(hip.CtHipError):
        hip.augment_u8(gt, ref[:, :, :, :50].contiguous(), [ac.params()] * 2, (19, 23))
    with pytest.raises(ValueError):
        hip.augment_u8(gt, ref, [ac.params(), ac.params(ops=[("hue", 0.7)])], (19, 23))
    with pytest.raises(ValueError):
        hip.augment_u8(gt, ref, [ac.params(19, 0), ac.params()], (19, 23))             # the last legal corner is (18, 30)


# ---- 5. the error codes, through the C ABI ------------------------------------------------------------------------------------------------
def _table(hip, **fields):
    t = hip.augment_table([ac.params(ops=fields.pop("ops", [("gamma", 1.2)]))])
    for k, v in fields.items():
        t[0][k] = v
    return t


def test_every_refusal_comes_before_any_launch(hip, pair):
    from ct_hip import _core
    lib, BAD, WS = hip.lib(), -1, -2
    gt, ref = (t[:1].cuda().contiguous() for t in pair)
    crop = (19, 23)
    outs = [torch.full((1, 3) + crop, 7.5, dtype=torch.float32, device="cuda") for _ in range(3)]
    out_u8 = torch.full((1, 3) + crop, 77, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(16, dtype=torch.int64, device="cuda")
    need = lib.ct_augment_workspace_bytes(1)
    assert need == 48 and lib.ct_augment_workspace_bytes(5) == 240 and lib.ct_augment_workspace_bytes(0) == 0
    good = _table(hip)

    def call(table=good, n=1, h=37, w=53, ch=crop[0], cw=crop[1], null=None, ws_ptr=None, ws_bytes=128, dev=True):
        dev_table = _core._upload_small(np.ascontiguousarray(table).view(np.int64), gt.device)
        args = [_core._ptr(gt), _core._ptr(ref), n, h, w, table.ctypes.data, _core._ptr(dev_table), ch, cw, _core._ptr(outs[0]),
                _core._ptr(outs[1]), _core._ptr(outs[2]), _core._ptr(out_u8), ctypes.c_void_p(ws.data_ptr() if ws_ptr is None else ws_ptr), ws_bytes,
                _core._stream()]
        if null is not None:
            args[null] = ctypes.c_void_p(0)
        return lib.ct_augment_u8(*args)

    for null in (0, 1, 5, 6, 9, 10, 11):                     # gt, ref, samples, samples_dev, out_gt, out_ref, out_target
        assert call(null=null) == BAD, null
    for kw in (dict(n=0), dict(h=0), dict(w=-1), dict(ch=0), dict(cw=0), dict(ch=38), dict(cw=54)):
        assert call(**kw) == BAD, kw
    refused = [dict(top=19), dict(top=-1), dict(left=31), dict(left=-1), dict(swap_hflip=2), dict(vflip=-1), dict(n_ops=7), dict(n_ops=-1),
               dict(ops=[("gamma", 1.0), (7, 1.0)]), dict(ops=[(-1, 1.0)]), dict(ops=[("hue", 0.51)]), dict(ops=[("hue", -0.6)]),
               dict(ops=[("hue", float("nan"))]), dict(ops=[("sharpness", 1.0), ("gamma", 1.0), ("sharpness", 1.0)])]
    refused += [dict(ops=[("identity", 0.0), (k, -0.01)]) for k in ("brightness", "contrast", "saturation", "gamma", "sharpness")]
    for fields in refused:
        assert call(table=_table(hip, **fields)) == BAD, fields
    assert call(ws_ptr=0) == WS and call(ws_bytes=need - 1) == WS and call(ws_ptr=ws.data_ptr() + 4) == WS
    torch.cuda.synchronize()
    assert all(bool((o == 7.5).all()) for o in outs) and bool((out_u8 == 77).all())      # nothing was launched
    # and the call they were refused from runs: the last legal corner, a hue at the end of its range, a zero factor
    ok = _table(hip, top=18, left=30, ops=[("hue", 0.5), ("sharpness", 0.0), ("contrast", 0.0)])
    assert call(table=ok, ws_bytes=need) == 0
    torch.cuda.synchronize()
    want = ac.sample(pair[0][0], pair[1][0], ac.params(18, 30), crop)
    assert torch.equal(outs[0].cpu()[0], want[0].float() / 255) and torch.equal(outs[1].cpu()[0], want[1].float() / 255)
    assert torch.equal(outs[2].cpu(), out_u8.cpu().float() / 255)
