"""The iterative distribution transfer on uint8 frames (ct_idt_u8, ct_hip.idt_u8) on the GPU, and its route through
methods.iterative, Runner(iterative_groups=True) and `utils.cli --model.iterative_groups true`.

Bounds, none of them taken from the code under test:
  probes, float64 out   bitwise the C oracle (oracle/idt_oracle.c) and ct_idt_f32 / ct_idt_f64 on the image the bytes stand for:
                        float32(k) / float32(255) (input_f32) or k / 255.0 -- the byte sweeps run the float sweeps' statements
  float32 out           bitwise `.float()` of the float64 output (one rounding); bytes bitwise ct_hip.pack_u8 of that
  mse                   3 N 2^-53 relative to numpy's float64 mean of the squared differences of the entry's own float32 output
                        (clamped) and float32(gt) / float32(255), N pixels: what test_mk_psnr allows (other partial sums, same terms)
"""
import os

import numpy as np
import pytest

from oracle import iterative as oit
from tests.u8_common import ULP, dev, grouped_frames, image, per_frame_route, psnr_close, rotations, same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "color-transfer_amd", "configs")
IDT_SPEC = "methods.iterative.iterative_distribution_transfer"
PROBES = ("hist", "lut", "par", "binidx")


def frames(n, batch, seed):
    """seeded random bytes [batch, n, 1, 3]"""
    return np.random.default_rng(100003 * seed + 17 * n + batch).integers(0, 256, (batch, n, 1, 3), dtype=np.uint8)


def same_probes(d, want):
    return all(same(d[k], want[k]) for k in PROBES)


def assert_bitwise_vs_oracle(out, d, t, r, rot, bins):
    o_out, o = oit.iterative_distribution_transfer(t, r, bins=bins, n_iter=rot.shape[0], rotations=rot, debug=True)
    d = {k: v.cpu().numpy() for k, v in d.items()}
    assert np.array_equal(d["par"][0, :, :, 0:2], o["lohi"]), "lo/hi differ"
    assert np.array_equal(d["binidx"][0].astype(np.uint16), o["binidx"]), "bin indices differ"
    assert np.array_equal(d["hist"][0, :, 0].astype(np.int64), o["hist0"]), "target histogram counts differ"
    assert np.array_equal(d["hist"][0, :, 1].astype(np.int64), o["hist1"]), "reference histogram counts differ"
    assert np.array_equal(d["lut"][0, :, :, :, 0], o["lut"]), "LUT f differs"
    assert np.array_equal(out.cpu().numpy(), o_out), "float64 output not bitwise equal to the oracle"


# n_t, n_r, bins, n_iter: every pixel count (the head / run / tail / tile paths), both size orders, the bin counts, and the
# iteration counts -- 5 crosses the four-rotation group of the lo/hi sweep, 1 makes the byte-reading sweep the last one
CASES = [(n, n, 255, 4) for n in (1, 2, 15, 16, 17, 255, 1000, 4099, 70002)] + [
    (1000, 4099, 255, 4), (4099, 1000, 255, 4), (17, 70002, 255, 4), (4099, 4099, 7, 4), (4099, 1000, 1024, 4), (4099, 4099, 255, 1),
    (1000, 4099, 255, 5), (70002, 255, 1024, 5), (16, 17, 7, 1)]


@pytest.mark.parametrize("f32", (True, False))
@pytest.mark.parametrize("n_t,n_r,bins,n_iter", CASES)
def test_bitwise_against_the_oracle(n_t, n_r, bins, n_iter, f32):
    import ct_hip
    t, r, rot = frames(n_t, 1, 1)[0], frames(n_r, 1, 2)[0], rotations(n_iter, n_t + n_r + bins)
    out, d = ct_hip.idt_u8(dev(t), dev(r), rot, bins=bins, input_f32=f32, out_dtype=torch.float64, debug=True)
    assert out.dtype == torch.float64 and tuple(out.shape) == t.shape
    assert_bitwise_vs_oracle(out, d, image(t, f32), image(r, f32), rot, bins)
    # and the float entry on the converted image, probe for probe
    want, dw = ct_hip.idt(dev(image(t, f32)), dev(image(r, f32)), rot, bins=bins, debug=True)
    assert same(out, want) and same_probes(d, dw)


def test_every_table_entry():
    """every byte value in every channel: the float32 division of all 256 table entries"""
    import ct_hip
    rng = np.random.default_rng(5)
    t = np.stack([rng.permutation(np.repeat(np.arange(256), 2)) for _ in range(3)], axis=-1).astype(np.uint8).reshape(512, 1, 3)
    r = np.stack([rng.permutation(256) for _ in range(3)], axis=-1).astype(np.uint8).reshape(256, 1, 3)
    assert all(len(np.unique(a[..., c])) == 256 for a in (t, r) for c in range(3))
    rot = rotations(4, 11)
    out, d = ct_hip.idt_u8(dev(t), dev(r), rot, input_f32=True, out_dtype=torch.float64, debug=True)
    want, dw = ct_hip.idt(dev(image(t, True)), dev(image(r, True)), rot, debug=True)
    assert same(out, want) and same_probes(d, dw)
    # the two conventions differ in the table, and the results show it
    assert not same(out, ct_hip.idt_u8(dev(t), dev(r), rot, input_f32=False, round_dr_f32=True, out_dtype=torch.float64))


def test_every_base_alignment():
    """3 * 4099 = 9 (mod 16): the 16 frame bases of the batch cover every residue"""
    import ct_hip
    n, batch = 4099, 16
    t, r, g, rot = dev(frames(n, batch, 3)), dev(frames(n, batch, 4)), dev(frames(n, batch, 5)), rotations(4, 21, batch)
    assert sorted((3 * n * b) % 16 for b in range(batch)) == list(range(16))
    (o64, o32, o8), ps, d = ct_hip.idt_u8(t, r, rot, out=[torch.empty((batch, n, 1, 3), dtype=dt, device="cuda")
                                                          for dt in (torch.float64, torch.float32, torch.uint8)], gt=g, debug=True)
    for b in range(batch):
        (a64, a32, a8), ps1, d1 = ct_hip.idt_u8(t[b], r[b], rot[b], out=[torch.empty((n, 1, 3), dtype=dt, device="cuda")
                                                                         for dt in (torch.float64, torch.float32, torch.uint8)], gt=g[b], debug=True)
        assert same(a64, o64[b]) and same(a32, o32[b]) and same(a8, o8[b]), b
        assert all(same(d1[k][0], d[k][b]) for k in PROBES), b
        assert abs(float(ps1[0, 0]) - float(ps[b, 0])) <= 3 * n * ULP * float(ps[b, 0])          # other partial sums, the same terms


def test_views_off_the_16_byte_grid():
    """every buffer at a base of its own off the grid: the tiles take byte accesses, the same bits come out"""
    import ct_hip
    n, batch = 4099, 2
    t, r, g, rot = frames(n, batch, 26), frames(n, batch, 27), frames(n, batch, 28), rotations(4, 111, batch)
    want, ps = ct_hip.idt_u8(dev(t), dev(r), rot, gt=dev(g))

    def shifted(a, by):
        buf = torch.zeros(a.size + 32, dtype=torch.uint8, device="cuda")
        view = buf[by:by + a.size].view(a.shape)
        view.copy_(dev(a))
        assert view.data_ptr() % 16 == by and view.is_contiguous()
        return view

    buf = torch.zeros(t.size + 32, dtype=torch.uint8, device="cuda")
    got, ps1 = ct_hip.idt_u8(shifted(t, 1), shifted(r, 5), rot, out=buf[3:3 + t.size].view(t.shape), gt=shifted(g, 7))
    assert same(got, want) and same(ps1, ps)
    assert not bool(buf[:3].any()) and not bool(buf[3 + t.size:].any())      # nothing written around the view
    o64 = ct_hip.idt_u8(shifted(t, 9), shifted(r, 2), rot, out_dtype=torch.float64)
    assert same(o64, ct_hip.idt_u8(dev(t), dev(r), rot, out_dtype=torch.float64))


@pytest.mark.parametrize("f32", (True, False))
@pytest.mark.parametrize("flat_t,flat_r", ((True, False), (False, True), (True, True)))
def test_degenerate_pairs(flat_t, flat_r, f32):
    import ct_hip
    n = 1000
    t, r = frames(n, 1, 6)[0], frames(n, 1, 7)[0]
    if flat_t:
        t[:] = (200, 30, 101)
    if flat_r:
        r[:] = (200, 30, 101) if flat_t else (7, 255, 0)          # both flat: the same colour, so that lo == hi
    rot = rotations(4, 31)
    (o64, o32, o8), d = ct_hip.idt_u8(dev(t), dev(r), rot, input_f32=f32, out=[torch.empty((n, 1, 3), dtype=dt, device="cuda")
                                                                           for dt in (torch.float64, torch.float32, torch.uint8)], debug=True)
    want, dw = ct_hip.idt(dev(image(t, f32)), dev(image(r, f32)), rot, debug=True)
    assert same(o64, want) and same_probes(d, dw)                # NaN for NaN
    assert same(o32, want.float()) and same(o8, ct_hip.pack_u8(want.float().contiguous(), "hwc"))


@pytest.mark.parametrize("n,n_iter", ((4099, 4), (1000, 1), (70002, 2)))
def test_outputs(n, n_iter):
    import ct_hip
    t, r, g, rot = dev(frames(n, 2, 8)), dev(frames(n, 2, 9)), dev(frames(n, 2, 10)), rotations(n_iter, 41)
    o64 = ct_hip.idt_u8(t, r, rot, out_dtype=torch.float64)
    o32 = ct_hip.idt_u8(t, r, rot, out_dtype=torch.float32)
    o8 = ct_hip.idt_u8(t, r, rot)                                  # bytes by default; no float64 output: the state is in the workspace
    assert o64.dtype == torch.float64 and o32.dtype == torch.float32 and o8.dtype == torch.uint8
    assert same(o32, o64.float()) and same(o8, ct_hip.pack_u8(o32, "hwc"))
    kinds = (torch.float64, torch.float32, torch.uint8)
    want = dict(zip(kinds, (o64, o32, o8)))
    psnr = None
    for mask in range(1, 8):                                       # every combination of the three outputs, with the metric
        outs = [torch.empty(t.shape, dtype=dt, device="cuda") for i, dt in enumerate(kinds) if mask >> i & 1]
        got, ps = ct_hip.idt_u8(t, r, rot, out=outs, gt=g)
        assert all(same(o, want[o.dtype]) for o in got), mask
        psnr = ps if psnr is None else psnr
        assert same(ps, psnr), mask                                # the same sums whichever outputs are written
    again = ct_hip.idt_u8(t, r, rot)
    assert same(again, o8)                                         # two calls in a row
    # out=: the tensor handed in is the one written and returned
    mine = torch.empty_like(o8)
    assert ct_hip.idt_u8(t, r, rot, out=mine).data_ptr() == mine.data_ptr() and same(mine, o8)


@pytest.mark.parametrize("n", (17, 1000, 4099, 70002))
def test_metric(n):
    import ct_hip
    batch = 3
    t, r, g, rot = frames(n, batch, 11), frames(n, batch, 12), frames(n, batch, 13), rotations(4, 51)
    out, ps = ct_hip.idt_u8(dev(t), dev(r), rot, out_dtype=torch.float32, gt=dev(g))
    assert ps.dtype == torch.float64 and tuple(ps.shape) == (batch, 2)
    o, ps = out.cpu().numpy(), ps.cpu().numpy()
    for b in range(batch):
        d = np.clip(o[b], 0, 1).astype(np.float64) - (g[b].astype(np.float32) / np.float32(255)).astype(np.float64)
        mse = float(np.mean(d * d))
        err = abs(ps[b, 0] - mse) / mse
        print("n %d frame %d: mse %.17g, relative error %.3g (bound %.3g)" % (n, b, mse, err, 3 * n * ULP))
        assert err <= 3 * n * ULP
        assert abs(ps[b, 1] - 10 * np.log10(1 / mse)) <= 1e-12 * max(1.0, abs(ps[b, 1]))


def test_metric_of_a_nan_frame():
    import ct_hip
    n = 1000
    t, r, g = frames(n, 2, 14), frames(n, 2, 15), frames(n, 2, 16)
    rot = rotations(4, 61, 2)
    rot[1, 0, 0, 0] = np.nan                                       # frame 1: a NaN rotation makes every pixel NaN
    out, ps = ct_hip.idt_u8(dev(t), dev(r), rot, out_dtype=torch.float32, gt=dev(g))
    assert bool(torch.isnan(out[1]).all()) and not bool(torch.isnan(out[0]).any())
    ps = ps.cpu().numpy()
    assert np.isnan(ps[1, 0]) and np.isfinite(ps[0]).all()
    assert not ct_hip.idt_u8(dev(t), dev(r), rot)[1].any()         # NaN packs to 0


def test_grid_stride_loops_of_a_large_batch():
    """128 pairs leave each pair 8 or 16 workgroups per sweep: every pair equals the call on that pair alone"""
    import ct_hip
    n, batch = 1000, 128
    t, r, g, rot = dev(frames(n, batch, 17)), dev(frames(n, batch, 18)), dev(frames(n, batch, 19)), rotations(4, 71, batch)
    o8, ps = ct_hip.idt_u8(t, r, rot, gt=g)
    o64 = ct_hip.idt_u8(t, r, rot, out_dtype=torch.float64)
    assert same(o8, ct_hip.pack_u8(o64.float(), "hwc"))
    for b in range(batch):
        one, ps1 = ct_hip.idt_u8(t[b], r[b], rot[b], gt=g[b])
        assert same(one, o8[b]), b
        assert abs(float(ps1[0, 0]) - float(ps[b, 0])) <= 3 * n * ULP * float(ps[b, 0])
    for b in (0, 77, 127):
        assert same(ct_hip.idt_u8(t[b], r[b], rot[b], out_dtype=torch.float64), o64[b])


def test_one_pair_at_1080p():
    import ct_hip
    h, w = 1080, 1920
    rng = np.random.default_rng(9)
    tk, rk = rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    t, r = dev(tk), dev(rk)
    rot = rotations(4, 81)
    want = ct_hip.idt(dev(image(tk, True)), dev(image(rk, True)), rot)          # numpy's float32 division: correctly rounded
    o64, o8 = ct_hip.idt_u8(t, r, rot, out=[torch.empty((h, w, 3), dtype=torch.float64, device="cuda"), torch.empty_like(t)])
    assert same(o64, want) and same(o8, ct_hip.pack_u8(want.float()[None], "hwc")[0])
    assert same(ct_hip.idt_u8(t, r, rot), o8)                      # the state in the workspace


def test_argument_errors_are_raised_before_the_call():
    import ct_hip
    E = ct_hip.CtHipError
    n, B = 257, 3
    t, r, g, rot = dev(frames(n, B, 20)), dev(frames(n, B, 21)), dev(frames(n, B, 22)), rotations(4, 91)
    wide = dev(frames(n, B, 23).repeat(2, axis=2))                 # [3, 257, 2, 3]: every other column is not contiguous
    calls = [
        lambda: ct_hip.idt_u8(t.float(), r, rot), lambda: ct_hip.idt_u8(t, r.float(), rot),            # dtypes
        lambda: ct_hip.idt_u8(t, r[:2], rot),                                                          # batch sizes
        lambda: ct_hip.idt_u8(t.cpu(), r.cpu(), rot), lambda: ct_hip.idt_u8(t, r.cpu(), rot),          # devices
        lambda: ct_hip.idt_u8(wide[:, :, ::2], r, rot), lambda: ct_hip.idt_u8(t, wide[:, :, ::2], rot),  # strides
        lambda: ct_hip.idt_u8(t[..., :2].contiguous(), r, rot), lambda: ct_hip.idt_u8(t[0, :, 0], r[0, :, 0], rot),    # shapes
        lambda: ct_hip.idt_u8(t[:, :0], r, rot), lambda: ct_hip.idt_u8(t, r[:, :0], rot),              # empty frames
        lambda: ct_hip.idt_u8(t, r, rot[:, :2]), lambda: ct_hip.idt_u8(t, r, rot[0]), lambda: ct_hip.idt_u8(t, r, rot[:0]),
        lambda: ct_hip.idt_u8(t, r, np.stack([rot] * 2)),                                              # rotations of another batch
        lambda: ct_hip.idt_u8(t, r, rot, bins=0), lambda: ct_hip.idt_u8(t, r, rot, bins=1025), lambda: ct_hip.idt_u8(t, r, rot, bins=2.5),
        lambda: ct_hip.idt_u8(t, r, rot, out_dtype=torch.float16), lambda: ct_hip.idt_u8(t, r, rot, out_dtype=torch.int16),
        lambda: ct_hip.idt_u8(t, r, rot, out=torch.empty((B, n - 1, 1, 3), dtype=torch.uint8, device="cuda")),
        lambda: ct_hip.idt_u8(t, r, rot, out=torch.empty((B, n, 1, 3), dtype=torch.uint8)),
        lambda: ct_hip.idt_u8(t, r, rot, out=torch.empty((B, n, 1, 3), dtype=torch.int16, device="cuda")),
        lambda: ct_hip.idt_u8(t, r, rot, out=torch.empty_like(wide)[:, :, ::2]),
        lambda: ct_hip.idt_u8(t, r, rot, out=[torch.empty_like(t), torch.empty_like(t)]),             # one dtype twice
        lambda: ct_hip.idt_u8(t, r, rot, out=[]),
        lambda: ct_hip.idt_u8(t, r, rot, gt=g.float()), lambda: ct_hip.idt_u8(t, r, rot, gt=g[:2]), lambda: ct_hip.idt_u8(t, r, rot, gt=g.cpu()),
        lambda: ct_hip.idt_u8(t, r, rot, gt=g, psnr_out=torch.empty((B, 2), dtype=torch.float32, device="cuda")),
        lambda: ct_hip.idt_u8(t, r, rot, gt=g, psnr_out=torch.empty((B - 1, 2), dtype=torch.float64, device="cuda")),
        lambda: ct_hip.idt_u8(t, r, rot, psnr_out=torch.empty((B, 2), dtype=torch.float64, device="cuda")),      # psnr_out without gt
    ]
    for i, call in enumerate(calls):
        with pytest.raises(E):
            call()
            pytest.fail("call %d raised nothing" % i)
    # the C entry answers for itself too, before anything touches the device
    lib, null = ct_hip.lib(), None
    both = dev(np.stack([np.broadcast_to(rot, (B, 4, 3, 3)), np.linalg.inv(np.broadcast_to(rot, (B, 4, 3, 3)))]).reshape(2, B, 4, 9))
    out, o64 = torch.empty_like(t), torch.empty(t.shape, dtype=torch.float64, device="cuda")
    ps = torch.empty((B, 2), dtype=torch.float64, device="cuda")
    need1, need0 = lib.ct_idt_u8_workspace_bytes(B, 4, 255, n, 1), lib.ct_idt_u8_workspace_bytes(B, 4, 255, n, 0)
    ws = torch.empty(need1 + 16, dtype=torch.uint8, device="cuda")

    def entry(gt=null, n_iter=4, bins=255, f64=null, f32=null, u8=null, psnr=null, wsp=ws.data_ptr(), wsb=need1, n_t=n):
        return lib.ct_idt_u8(t.data_ptr(), n_t, r.data_ptr(), n, gt, B, both[0].data_ptr(), both[1].data_ptr(), n_iter, bins, 1, 1,
                             f64, f32, u8, psnr, wsp, wsb, null, null)

    assert entry() == -1                                                           # all three outputs absent
    assert entry(u8=out.data_ptr(), gt=g.data_ptr()) == -1                         # gt without psnr_out
    assert entry(u8=out.data_ptr(), bins=1025) == -1 and entry(u8=out.data_ptr(), bins=0) == -1
    assert entry(u8=out.data_ptr(), n_iter=0) == -1 and entry(u8=out.data_ptr(), n_t=-1) == -1
    assert entry(u8=out.data_ptr(), wsb=need1 - 1) == -2                           # the state does not fit
    assert entry(u8=out.data_ptr(), f64=o64.data_ptr(), wsb=need0 - 1) == -2
    assert entry(u8=out.data_ptr(), wsp=null) == -2 and entry(u8=out.data_ptr(), wsp=ws.data_ptr() + 8) == -2
    assert entry(f64=o64.data_ptr() + 4) == -3 and entry(f32=o64.data_ptr() + 2) == -3
    assert entry(u8=out.data_ptr(), f64=o64.data_ptr(), wsb=need0, gt=g.data_ptr(), psnr=ps.data_ptr()) == 0
    torch.cuda.synchronize()
    assert same(out, ct_hip.idt_u8(t, r, rot))


def test_methods_route():
    import ct_hip
    import methods.iterative as it
    t, r, rot = dev(frames(1000, 1, 24)[0]), dev(frames(1000, 1, 25)[0]), rotations(4, 101)
    assert same(it.iterative_distribution_transfer_cuda(t, r, rotations=rot), ct_hip.idt_u8(t, r, rot, out_dtype=torch.float64))
    assert same(it.iterative_distribution_transfer_cuda(t, r, rotations=rot, out_dtype=torch.uint8), ct_hip.idt_u8(t, r, rot))
    assert same(it.iterative_distribution_transfer_cuda(t, r, rotations=rot, input_f32=False, out_dtype=torch.float32),
                ct_hip.idt_u8(t, r, rot, input_f32=False, out_dtype=torch.float32))
    # float frames go where they went
    tf, rf = t.float() / 255, r.float() / 255
    assert same(it.iterative_distribution_transfer_cuda(tf, rf, rotations=rot), ct_hip.idt(tf, rf, rot))
    np.random.seed(5)
    drawn = it.iterative_distribution_transfer_cuda(t, r, out_dtype=torch.uint8)
    np.random.seed(5)
    assert same(drawn, ct_hip.idt_u8(t, r, it.draw_rotations(4)))


# --------------------------------------------------------------------------------------------------------- Runner and CLI
H, W, FRAMES, GROUP = 24, 40, 5, 3               # two groups, the second one ragged


def test_runner_groups():
    from methods import Runner
    from utils.data import SyntheticStereoVideoU8, prefetch_groups
    video = SyntheticStereoVideoU8(FRAMES, H, W, group=FRAMES, pool=2)
    want8, want_psnr = per_frame_route(IDT_SPEC, grouped_frames(video, FRAMES), 77)
    model = Runner(IDT_SPEC, metrics="psnr", iterative_groups=True)
    assert model.takes_groups() and not Runner(IDT_SPEC, metrics="psnr", byte_groups=True).takes_groups()
    device = torch.device("cuda", torch.cuda.current_device())
    rec = torch.zeros((FRAMES, 2), dtype=torch.float64, device=device)
    (ids, group), = list(prefetch_groups(video, range(FRAMES), device))
    assert len(ids) == FRAMES
    np.random.seed(77)
    got8 = model.predict_group(group)
    assert got8.dtype == torch.uint8 and tuple(got8.shape) == (FRAMES, H, W, 3)
    assert np.array_equal(got8.cpu().numpy(), want8)
    assert model.predict_group(group).data_ptr() != got8.data_ptr()                 # freshly allocated frames
    np.random.seed(77)
    model.test_group(group, rec)
    got = rec.cpu().numpy()
    for f in range(FRAMES):
        err = abs(got[f, 0] - want_psnr[f, 0]) / want_psnr[f, 0]
        print("frame %d: mse %.17g, relative difference %.3g (bound %.3g)" % (f, got[f, 0], err, 3 * H * W * ULP))
        assert err <= 3 * H * W * ULP
    assert psnr_close(got[:, 1], want_psnr[:, 1], H * W)


def cli_args(command):
    args = [command, "--config", os.path.join(CFG, "others.yaml"), "--model.func_spec", IDT_SPEC, "--model.metrics", "psnr",
            "--data.data_dir", "null", "--data.synthetic", "video_u8", "--data.n_frames", str(FRAMES), "--data.height", str(H),
            "--data.width", str(W), "--data.group", str(GROUP)]
    return args + (["--format", "npy"] if command == "predict" else [])


def test_cli_predict_iterative_groups(tmp_path):
    from utils import cli
    from utils.data import SyntheticStereoVideoU8
    video = SyntheticStereoVideoU8(FRAMES, H, W, group=GROUP)
    args = cli_args("predict")
    # with a timing dict a grouped run makes an untimed first pass over min(FRAMES, 3 GROUP) frames, which draws as well
    warm = min(FRAMES, 3 * GROUP)
    np.random.seed(123)
    timing = {}
    assert cli.main(args + ["--model.iterative_groups", "true", "--output", str(tmp_path / "groups")], timing=timing) == FRAMES
    assert timing["grouped"] is True and timing["frames_per_call"] == GROUP
    want8, _ = per_frame_route(IDT_SPEC, grouped_frames(video, FRAMES), 123, skip=warm)                # the per-frame route on the same frames
    for f in range(FRAMES):
        got = np.load(tmp_path / "groups" / ("%06d.npy" % f))
        assert got.dtype == np.uint8 and np.array_equal(got, want8[f]), f
    # without the flag: the per-frame float32 route, byte for byte what it is today
    np.random.seed(123)
    timing = {}
    assert cli.main(args + ["--output", str(tmp_path / "plain")], timing=timing) == FRAMES
    assert timing["grouped"] is False
    plain8, _ = per_frame_route(IDT_SPEC, [tuple(video.host_chunk(f)[i, 0] for i in range(3)) for f in range(FRAMES)], 123)
    for f in range(FRAMES):
        got = np.load(tmp_path / "plain" / ("%06d.npy" % f))
        assert got.dtype == np.uint8 and np.array_equal(got, plain8[f]), f


def test_cli_test_iterative_groups():
    from utils import cli
    from utils.data import SyntheticStereoVideoU8
    np.random.seed(321)
    grouped = cli.main(cli_args("test") + ["--model.iterative_groups", "true"])
    _, want = per_frame_route(IDT_SPEC, grouped_frames(SyntheticStereoVideoU8(FRAMES, H, W, group=GROUP), FRAMES), 321)
    assert tuple(grouped.shape) == (FRAMES, 4)
    assert psnr_close(grouped[:, 0].cpu().numpy(), want[:, 1], H * W)
    assert bool(torch.isnan(grouped[:, 1:]).all())
    # without the flag the table is the per-frame route's own
    np.random.seed(321)
    plain = cli.main(cli_args("test"))
    assert not bool(torch.isnan(plain[:, 0]).any()) and tuple(plain.shape) == (FRAMES, 4)
