"""The parallax attention at its edges, host side (no GPU): the inputs of tests/pam_edges_common.py are what
tests/test_pam_edges_gpu.py assumes (one-hot rows, occluded columns, split probabilities, nothing on the mask's knife edge), the
float32 CPU evaluation of the reference formula stays inside the bounds while it leaves the old absolute tolerances, wrong
references leave the bounds by 10x, and the tile geometry of csrc/pam.hip as its public entry reports it."""
import pytest

torch = pytest.importorskip("torch")

from tests import pam_edges_common as pc     # noqa: E402

HOST_L = (33, 129, 257)                      # lengths the GPU file uses, for the statistics of the inputs
GPU_CASES = ([(name, 3, L) for name in pc.CASES for L in (1, 2, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 255, 256, 257, 385)]
             + [("twin", n, L) for L, n in ((129, 4), (33, 9), (33, 17), (385, 6), (257, 11))]
             + [(name, 6, W) for name in ("flat", "peaked", "twin") for W in (1, 2, 3, 4, 5, 7, 8, 31, 32, 33, 63, 64, 65, 127, 128,
                                                                              129, 130, 191, 257)])


@pytest.mark.parametrize("L", HOST_L + (959, 1983))
def test_peaked_inputs_look_like_a_matcher(L):
    n = 3 if L < 900 else 2
    q, k, v = pc.inputs("peaked", n, L)
    ref = pc.reference(q, k, v)
    assert float(ref["p"].amax(dim=-1).median()) > 0.99                         # one-hot rows
    occluded = float((ref["colsum"] < 0.1).double().mean())
    assert 0.10 <= occluded <= 0.40, occluded                                   # columns under the valid threshold
    assert float(ref["colsum"].max()) > 2.0                                     # one key collects several queries
    assert 30.0 < float(ref["smax"].max()) < 90.0                               # logits of 40-80
    q, k, v = pc.inputs("twin", n, L)
    split = float((pc.reference(q, k, v)["p"].amax(dim=-1) < 0.9).double().mean())
    assert split >= 0.30, split                                                 # rows that share their probability between two tiles


@pytest.mark.parametrize("rising", [True, False])
def test_ramp_scores_span_thirty(rising):
    q, k, v = pc.inputs("ramp-up" if rising else "ramp-down", 3, 129)
    sc = pc.reference(q, k, v)["sc"]
    assert 29.0 < float(sc.max()) < 31.0 and -31.0 < float(sc.min()) < -29.0
    tile_max = torch.stack([sc[:, :, j:j + 32].amax(dim=-1) for j in range(0, 129, 32)], dim=-1)
    steps = tile_max[..., 1:] - tile_max[..., :-1]
    assert (steps > 0.2).all() if rising else (steps < -0.2).all()              # the running maximum grows in every tile (the last holds one key) / never


def test_nothing_sits_on_the_knife_edge():
    worst = max((pc.knife_share(pc.case(*c)[3]), c) for c in GPU_CASES)
    assert worst[0] <= pc.KNIFE_SHARE, worst


def test_ratio_is_the_imported_bound():
    """pc.out_ratio restates tests/test_gmflow_kernels_gpu.py::assert_attention_bound (which the GPU file asserts through) only to
    print a figure: the two must agree on which side of 1 a result lies"""
    from tests.test_gmflow_kernels_gpu import assert_attention_bound
    q, k, v, ref = pc.case("twin", 3, 129)
    live = slice(0, pc.CLIVE)
    for eps, ok in ((0.5, True), (0.98, True), (1.02, False), (3.0, False)):
        v_live = ref["v"][:, :, live]
        bound = (pc.A_REL + pc.A_SMAX * ref["smax"]) * torch.matmul(ref["p"], v_live.abs()) + pc.A_FLOOR * v_live.abs().sum(dim=1, keepdim=True)
        out = ref["out"].clone()
        out[:, :, live] += eps * bound
        assert abs(pc.out_ratio(out, ref) - eps) < 1e-6
        if ok:
            assert_attention_bound(out[:, :, live], ref["out"][:, :, live], ref["sc"], ref["p"], v_live, "eps %g" % eps)
        else:
            with pytest.raises(AssertionError):
                assert_attention_bound(out[:, :, live], ref["out"][:, :, live], ref["sc"], ref["p"], v_live, "eps %g" % eps)


@pytest.mark.parametrize("L", HOST_L + (959, 1983))
def test_float32_evaluation_stays_inside_the_bounds(L):
    """the reference formula in plain float32 on the CPU (the yardstick of the map's R) at the lengths whose statistics are checked
    above: <= 0.6 of the bound on outputs and on column sums in every case.  Printed, not asserted: its statistics and disparity
    ratios, and R.  (Away from these lengths it comes closer: 0.70 on outputs and 1.13 -- outside -- on the statistics at twin,
    L = 65, where the kernels of csrc/attention16.hip reach 0.31 and 0.36: they accumulate wider than a float32 dot product.)"""
    n = 3 if L < 900 else 2
    for name in pc.CASES:
        q, k, v = pc.inputs(name, n, L)
        ref = pc.reference(q, k, v)
        r = pc.ratios(pc.as_kernel_outputs(pc.reference32(q, k, v)), ref)
        print("[pam-edges host] float32 CPU evaluation %s L=%d: %s R=%.3g" % (name, L, " ".join("%s=%.3f" % kv for kv in r.items()),
                                                                            max(1.0, pc.R_FACTOR * r["att"])))
        assert r["out"] <= 0.6 and r["colsum"] <= 0.6, (name, L, r)


def test_old_absolute_tolerances_cannot_be_reused():
    """on the twin case the float32 CPU evaluation is further from float64 than the tolerances of the flat-score tests (2e-5 on
    outputs, 1e-6 on the map: tests/test_dcmcs3di_gpu.py::test_pam_kernels_vs_torch_reference) allow: they hold no peaked input"""
    out_err, map_err = [], []
    for L in (129, 257, 959, 1983):
        q, k, v = pc.inputs("twin", 2, L)
        ref, ev = pc.reference(q, k, v), pc.reference32(q, k, v)
        out_err.append(float((ev["out"] - ref["out"]).abs().max()))
        map_err.append(float((ev["p"] - ref["p"]).abs().max()))
    print("[pam-edges host] float32 CPU evaluation, twin, max-abs error: out %s map %s" % (out_err, map_err))
    assert max(out_err) > 2e-5 and min(map_err) > 1e-6, (out_err, map_err)


# ---- resolving power: a kernel that is wrong in one of these ways must leave a bound by 10x ----------------------------------------
def _wrong(kind, q, k, v):
    n, L, _ = q.shape
    good = pc.reference(q, k, v)
    if kind == "last-key-dropped":
        ev = pc.reference(q, k[:, :-1], v[:, :-1])
        ev["colsum"] = torch.cat([ev["colsum"], torch.zeros(n, 1, dtype=torch.float64)], dim=1)
        ev["p"] = torch.cat([ev["p"], torch.zeros(n, L, 1, dtype=torch.float64)], dim=2)
    elif kind == "keys-shifted":
        ev = pc.reference(q, torch.roll(k, 1, dims=1), v)
    elif kind == "rows-swapped":
        ev = {name: t.clone() for name, t in good.items()}
        for name in ("out", "m", "l", "colsum", "disp", "p"):
            ev[name][[0, 1]] = good[name][[1, 0]]
    elif kind == "tile-softmax-without-running-max":
        sc = good["sc"]
        e = torch.cat([torch.exp(sc[:, :, j:j + 32] - sc[:, :, j:j + 32].amax(dim=-1, keepdim=True)) for j in range(0, L, 32)], dim=-1)
        p = e / e.sum(dim=-1, keepdim=True)
        j = torch.arange(L, dtype=torch.float64)
        ev = dict(good, p=p, out=torch.matmul(p, good["v"]), l=e.sum(dim=-1), colsum=p.sum(dim=1), disp=j[None] - torch.matmul(p, j))
    elif kind == "query-31-dropped-from-colsum":
        ev = dict(good, colsum=good["colsum"] - good["p"][:, 31, :])
    else:
        assert kind == "stats-of-the-row-before"
        m, l = torch.roll(good["m"], 1, dims=0), torch.roll(good["l"], 1, dims=0)
        ev = dict(good, m=m, l=l, colsum=(torch.exp(good["sc"] - m[..., None]) / l[..., None]).sum(dim=1))
    return pc.as_kernel_outputs(ev), good


@pytest.mark.parametrize("kind", ["last-key-dropped", "keys-shifted", "rows-swapped", "tile-softmax-without-running-max",
                                  "query-31-dropped-from-colsum", "stats-of-the-row-before"])
@pytest.mark.parametrize("name", ["flat", "peaked", "twin", "ramp-up"])
def test_bounds_resolve_a_wrong_kernel(name, kind):
    q, k, v = pc.inputs(name, 3, 129)
    wrong, good = _wrong(kind, q, k, v)
    r = pc.ratios(wrong, good)
    r["att"] /= pc.map_R(q, k, v, good)
    assert max(r.values()) >= 10.0, (name, kind, r)


# ---- geometry from the public entry -------------------------------------------------------------------------------------------------
def test_pam_tile_geometry_from_the_workspace_entry():
    heights, w32, wmax = pc.pam_geometry()
    seq = [heights[w] for w in sorted(heights)]
    assert seq == sorted(seq, reverse=True) and set(seq) == {32, 16, 0}          # 32 -> 16 -> refused, no holes
    assert seq[0] == 32 and seq[-1] == 0
    # one TQ x (W | 1) tile of scores + the Q tile (64 x TQ) + a 64 x 128 key chunk, in floats, within the 160 KiB LDS
    fits = lambda tq, w: (tq * (w | 1) + 64 * tq + 64 * 128) * 4 <= 160 * 1024
    assert fits(32, w32) and not fits(32, w32 + 1) and fits(16, wmax) and not fits(16, wmax + 1)
    assert (w32, wmax) == (959, 1983)                                            # what csrc/pam.hip and the docstrings state
    import ct_hip
    lib = ct_hip.lib()
    assert lib.ct_pam_workspace_bytes(2, 3, wmax) == 2 * 3 * ((wmax + 15) // 16) * wmax * 4
    assert lib.ct_pam_workspace_bytes(2, 3, wmax + 1) == 0 and lib.ct_pam_workspace_bytes(-1, 1, 8) == 0
