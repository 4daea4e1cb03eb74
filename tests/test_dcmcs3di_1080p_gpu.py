"""The DCMCS3DI forward at BASELINE.json's full size, 1920 x 1080 and full depth, held against the float64 oracle.

A whole 1080p pair is out of the oracle's reach (one [H,W,W] float64 attention map is 32 GB), but the network is convolutional
down the rows and attends along a row only, so a band of output rows depends on 53 more input rows on either side
(oracle/dcmcs3di.py: forward_band; tests/test_oracle_dcmcs3di_bands.py pins the banded form to the whole one).  Three bands of
all 1920 columns -- every column strip of every kernel and both side edges -- are compared per convolution mode:

  rows    0..8      the top edge (real zero padding)
  rows 1072..1080   the bottom edge; of the last pair of a batch: the highest addresses of every tensor
  rows  264..276    an interior band across two row-segment boundaries of conv_wino4, which splits the rows of a launch into
                    even segments by the number of images N it is given (csrc/conv_wino4.hip:686-698, the loop that picks
                    n_seg / seg from `imgs = N * groups`; the kernel starts a segment at y0 = sy * seg, :407):
                      N = 2 (the two-view launches of extraction and matcher head at batch 1; methods/dcmcs3di.py:65-67 run both
                             views in one batch): 4 segments of 270 rows -> boundaries 270 / 540 / 810
                      N = 1 (the one-view launches of the transfer ResBs at batch 1; methods/dcmcs3di.py:112-114):
                             8 segments of 136 rows -> boundaries 136 / 272 / ...
                    so rows 269|270 and 271|272 both lie inside the band.  (At batch 2 the launches see N = 4 and N = 2: segments
                    of 540 and 270 rows.)  In `split-ws` mode the same convolutions run on conv_ws.hip, in `exact` on conv_exact.hip.

Held per band and mode, max-abs against the oracle: fea_left, fea_right, fea_warped, warped_rgb <= 1e-4 (the project's gate,
SURVEY 8c); pre_clamp and corrected <= 1e-4 against the oracle's transfer branch fed the DEVICE's valid mask (the threshold
`colsum > 0.1` is discontinuous; tests/test_configs_gpu.py does the same at 512 x 512); the column sums <= 5e-3 (this recipe scales
the logits by 256: float32 rounding of the features moves a sum by ~2e-3, the float32 reference sits on the same floor -- at this
width the float32 oracle's sums, which reach 72, are 8.8e-5 from float64); the mask equal to the oracle's wherever the oracle's sum
is further than 5e-3 from the threshold, which must be more than 0.9 of the band.  As a locator for a column-sum miss, every band
also prints the distance of the device's column sums from the oracle's head + attention stage run in float64 on the device's OWN
feature rows: that leaves the attention kernels' error alone, without the amplified rounding of the 19 layers before them.

Batches (default mode): the bottom band of the last pair against the oracle, and pair 0's three bands bitwise equal to the batch-1
run.  With B = 2 the two-view activation tensors and the token rows are 4 x 64 x 1080 x 1920 floats = 2 123 366 400 bytes, which
is 1.1 % SHORT of 2^31 (at B = 1 likewise 1.1 % short of 2^30), so B = 5 is run as well: 5.3e9 bytes, beyond 2^32.

Measured on an MI355X (max-abs against float64; `att` = column sums against float64 attention on the device's features):

  mode, band            fea_left fea_right fea_warped warped_rgb pre_clamp corrected  colsum (max sum)      att   flips  sure
  split    top          7.94e-07 8.35e-07  1.37e-06   9.10e-07   2.20e-07  2.20e-07   4.81e-05 (55.7)  2.78e-05   0     0.9866
  split    interior     8.59e-07 1.07e-06  1.32e-06   1.02e-06   2.58e-07  2.58e-07   4.60e-05 (48.1)  3.12e-05   0     0.9831
  split    bottom       8.07e-07 8.33e-07  1.37e-06   9.34e-07   2.23e-07  2.23e-07   9.36e-05 (98.5)  2.60e-05   0     0.9852
  split-ws top          8.01e-07 8.59e-07  1.35e-06   1.04e-06   2.59e-07  2.59e-07   6.04e-05         2.31e-05   0     0.9866
  split-ws interior     8.52e-07 8.64e-07  1.34e-06   1.01e-06   2.38e-07  2.38e-07   5.96e-05         4.80e-05   0     0.9831
  split-ws bottom       8.38e-07 8.26e-07  1.25e-06   9.84e-07   2.27e-07  2.27e-07   5.19e-05         4.75e-05   0     0.9852
  exact    top          1.35e-05 1.39e-05  1.95e-06   2.20e-06   1.67e-06  1.67e-06   6.80e-04         1.20e-04   0     0.9866
  exact    interior     1.63e-05 1.28e-05  1.78e-06   1.81e-06   1.95e-06  1.95e-06   8.08e-04         2.11e-04   0     0.9831
  exact    bottom       1.29e-05 1.46e-05  2.39e-06   2.15e-06   1.73e-06  1.73e-06   9.86e-04         2.16e-04   0     0.9852
  split B=2 pair 1 bot. 9.91e-07 8.68e-07  1.39e-06   9.76e-07   2.41e-07  2.41e-07   5.59e-05 (37.4)  2.74e-05   0     0.9870
  split B=5 pair 4 bot. the same content as the row above (the second pair is the last of either batch), the same eleven figures

Every bound is the one stated above; none was met narrowly, none was adjusted.  The column sums stay 50 times below their bound at this
width, so the locator had nothing to locate: most of their error is the attention kernels' own (`att`), not amplified feature rounding.
Pair 0 of both batches equals the batch-1 run bit for bit.  The oracle's bands take 12 + 19 + 11 s of CPU once per module, + 11 s
once for both batch cases; the module runs in 75 s, tests/test_configs_gpu.py::test_dcmcs3di_512_full_depth_vs_oracle in 84 s (its three
modes, 30 + 28 + 26 s) on the same machine.
"""
import time

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import dcmcs3di as odc                      # noqa: E402
from tests.dcmcs3di_common import build_model            # noqa: E402

H, W = 1080, 1920
TOL = 1e-4                # SURVEY 8c; tests/test_dcmcs3di_gpu.py: TOL
TOL_COLSUM = 5e-3         # tests/test_configs_gpu.py::test_dcmcs3di_512_full_depth_vs_oracle, same recipe
BANDS = {"top": (0, 8), "interior": (264, 276), "bottom": (H - 8, H)}
FEATURES = ("fea_left", "fea_right", "fea_warped", "warped_rgb")
PARTS = FEATURES + ("colsum_left", "valid_left", "pre_clamp", "corrected")


def _pair(seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(1, 3, H, W, generator=gen), torch.rand(1, 3, H, W, generator=gen)


@pytest.fixture(scope="module")
def model():
    return build_model(seed=11).cuda()


@pytest.fixture(scope="module")
def sd(model):
    return {k: v.detach().cpu() for k, v in model.state_dict().items()}


@pytest.fixture(scope="module")
def pairs():
    return _pair(12), _pair(13)


def _oracle_band(sd, pair, y0, y1):
    t0 = time.time()
    ref, state = odc.forward_band(sd, pair[0], pair[1], y0, y1, keep_maps=False, return_state=True)
    return ref, state, time.time() - t0


@pytest.fixture(scope="module")
def oracle_bands(sd, pairs):
    """the three bands of pair 0 in float64, once for all convolution modes (the oracle does not depend on the mode)"""
    return {name: _oracle_band(sd, pairs[0], y0, y1) for name, (y0, y1) in BANDS.items()}


@pytest.fixture(scope="module")
def oracle_bottom_pair1(sd, pairs):
    """the bottom band of the second pair, once for both batch sizes (it is the last pair of either batch)"""
    return _oracle_band(sd, pairs[1], *BANDS["bottom"])


def _rows(p, b, y0, y1):
    """rows y0..y1 of image b of every compared part, on the CPU"""
    return {k: p[k][b:b + 1, :, y0:y1].cpu() for k in PARTS}


def _check_band(tag, sd, got, dev_valid, dev_fea, ref, state, t_cpu, y0, y1):
    """got: _rows() of the device's run; dev_valid: its whole [1,1,H,W] mask; dev_fea: (fea_left, fea_right) rows
    [max(0, y0 - 2), min(H, y1 + 2)) of the device for the attention-only comparison"""
    err = {k: float((got[k].double() - ref[k]).abs().max()) for k in FEATURES}
    override = odc.band_transfer(sd, state, dev_valid)
    err["pre_clamp"] = float((got["pre_clamp"].double() - override).abs().max())
    err["corrected"] = float((got["corrected"].double() - override.clamp(0, 1)).abs().max())
    e_colsum = float((got["colsum_left"][:, 0].double() - ref["colsum"]).abs().max())
    band_valid = got["valid_left"] > 0.5
    sure = ((ref["colsum"] - 0.1).abs() > TOL_COLSUM).unsqueeze(1)
    flips = int((band_valid != ref["valid_left"]).sum())
    agree = bool((band_valid == ref["valid_left"])[sure].all())
    # the attention kernels alone: float64 head + attention on the device's own features (2 more rows for the head's ResB)
    f0 = max(0, y0 - 2)
    fl, fr = (t.double() for t in dev_fea)
    # (three feature channels stand in for the right image: warped_rgb of this run is not looked at)
    att = odc.attention_stage(sd, fr, odc.head_stage(sd, fl), odc.head_stage(sd, fr), fr[:, :3], rows=slice(y0 - f0, y1 - f0))
    e_att = float((got["colsum_left"][:, 0].double() - att["colsum"]).abs().max())
    print("\n[dcmcs3di 1080p %s rows %d..%d] oracle %.0f s on CPU; max-abs %s; column sums %.2e (max sum %.1f; against float64 "
          "attention on the device's features %.2e); valid mask: %d of %d pixels differ, sure share %.4f, agree where sure: %s"
          % (tag, y0, y1, t_cpu, {k: "%.2e" % v for k, v in err.items()}, e_colsum, float(ref["colsum"].max()), e_att, flips,
             band_valid.numel(), float(sure.float().mean()), agree))
    for k, v in err.items():
        assert v <= TOL, (tag, k, v)
    assert e_colsum <= TOL_COLSUM, (tag, e_colsum, e_att)
    assert agree, tag
    assert float(sure.float().mean()) > 0.9, tag


def _fea_rows(p, b, y0, y1):
    f0, f1 = max(0, y0 - 2), min(H, y1 + 2)
    return p["fea_left"][b:b + 1, :, f0:f1].cpu(), p["fea_right"][b:b + 1, :, f0:f1].cpu()


def test_forward_1080p_bands_vs_oracle(conv_mode, request, model, sd, pairs, oracle_bands):
    """batch 1, every convolution mode: the three bands against the float64 oracle (module docstring)"""
    mode = request.node.callspec.params["conv_mode"]
    left, right = pairs[0][0].cuda(), pairs[0][1].cuda()
    p = model.forward_parts(left, right)
    dev_valid = p["valid_left"].cpu() > 0.5
    corrected = model(left, right, inference=True)[0]
    for name, (y0, y1) in BANDS.items():
        ref, state, t_cpu = oracle_bands[name]
        _check_band("%s, %s" % (mode, name), sd, _rows(p, 0, y0, y1), dev_valid, _fea_rows(p, 0, y0, y1), ref, state, t_cpu, y0, y1)
        # the public call (dcmcs3di.py:61-66) gives the same picture
        assert float((corrected[:, :, y0:y1] - p["corrected"][:, :, y0:y1]).abs().max()) <= 2e-5, name


@pytest.mark.parametrize("batch", [2, 5])
def test_forward_1080p_batched(batch, model, sd, pairs, oracle_bottom_pair1):
    """One forward with B pairs (default mode).  The bottom band of the LAST pair -- the highest addresses of every tensor --
    against the oracle; pair 0's three bands bitwise equal to the batch-1 run (the summation order of every kernel is fixed and
    does not depend on the number of images: a batch offset must not change a value).
    B = 2: the two-view activation tensors and the token rows [2B*H, W, 64] are 2 123 366 400 bytes, 1.1 % short of 2^31.
    B = 5 (the second pair last again, so one oracle band serves both sizes): they are 5.3e9 bytes, so the last view starts beyond 2^32 bytes, and the one-view tensors of the transfer branch
    (2.65e9 bytes) end beyond 2^31: offsets a 32-bit integer, signed or not, cannot hold."""
    import ct_hip
    assert ct_hip.conv_mode() == "split" and ct_hip.conv_wino()
    every = [pairs[0]] + [_pair(12 + i) for i in range(2, batch)] + [pairs[1]]      # the second pair last: one oracle band for both sizes
    left = torch.cat([q[0] for q in every]).cuda()
    right = torch.cat([q[1] for q in every]).cuda()
    two_view_bytes = 2 * batch * 64 * H * W * 4
    assert two_view_bytes > (2 ** 32 if batch == 5 else 0.98 * 2 ** 31)
    p = model.forward_parts(left, right)
    last = batch - 1
    y0, y1 = BANDS["bottom"]
    ref, state, t_cpu = oracle_bottom_pair1
    _check_band("split, batch %d, pair %d, bottom" % (batch, last), sd, _rows(p, last, y0, y1),
                p["valid_left"][last:last + 1].cpu() > 0.5, _fea_rows(p, last, y0, y1), ref, state, t_cpu, y0, y1)
    got0 = {name: _rows(p, 0, *rows) for name, rows in BANDS.items()}
    del p
    p1 = model.forward_parts(left[:1], right[:1])
    for name, rows in BANDS.items():
        want = _rows(p1, 0, *rows)
        for k in PARTS:
            assert torch.equal(got0[name][k], want[k]), (name, k, float((got0[name][k] - want[k]).abs().max()))
    assert ct_hip.device_status() == 0
