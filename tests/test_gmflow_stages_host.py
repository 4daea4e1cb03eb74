"""On the CPU: (a) the host tables of color-transfer_amd/unimatch/__init__.py bit for bit against oracle/gmflow.py, (b) every case of
tests/gmflow_stages_common.py is admitted (its gate is at most 1e-3 of its output range), (c) a stage test cannot pass a wrong
stage: the float64 oracle with one named alteration moves the expected output by at least 100 gates.

The tables are imported from the `unimatch` package, whose module imports ct_hip (ctypes declarations; no library is loaded and no
kernel runs: the tables accept a CPU device)."""
import pytest

torch = pytest.importorskip("torch")

from oracle import gmflow as og   # noqa: E402
from tests import gmflow_stages_common as C   # noqa: E402

# (h, w, splits); (8, 16, 8): a window one row high, wh // 2 == 0, the slices -0: degenerate (a 32-row frame gets there)
TABLE_SIZES = [(8, 12, 2), (16, 24, 8), (64, 112, 2), (128, 224, 8), (8, 16, 8)]
CPU = torch.device("cpu")
MOVE = 100.0


@pytest.fixture(scope="module")
def um():
    return pytest.importorskip("unimatch")


@pytest.mark.parametrize("h,w,splits", TABLE_SIZES)
def test_region_ids_induce_the_shift_window_mask(um, h, w, splits):
    reg = um._region_ids(h, w, splits, CPU)
    assert reg.dtype == torch.int32 and tuple(reg.shape) == (splits * splits, (h // splits) * (w // splits)) and reg.is_contiguous()
    want = og.shift_window_mask(h, w, h // splits, w // splits)
    # what ct_hip.attention_tokens adds to a score: -100 where the regions of query and key differ.  The oracle's mask is
    # m[win, i, j] = f(region[j] - region[i]); the rule is symmetric, the comparison is made in the oracle's index order
    induced = torch.where(reg[:, None, :] != reg[:, :, None], -100.0, 0.0)
    assert induced.dtype == want.dtype and torch.equal(induced, want)


@pytest.mark.parametrize("h,w,splits", TABLE_SIZES)
def test_position_table_is_the_sine_embedding(um, h, w, splits):
    wh, ww = h // splits, w // splits
    got = um._position_table(wh, ww, 64, CPU)
    want = og.position_embedding_sine(1, wh, ww, 64, torch.float32)
    assert got.dtype == torch.float32 and got.is_contiguous() and torch.equal(got, want)
    # as _add_position tiles it over the frame: the oracle's split / add / merge of a zero feature map
    zero = torch.zeros(2, 128, h, w)
    tiled = um._position_table(wh, ww, 64, CPU).repeat(2, 1, splits, splits)
    assert torch.equal(tiled, og.feature_add_position(zero, zero, splits, 128)[0])


@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("h,w,splits", TABLE_SIZES)
def test_window_rowmap_is_split_roll_split_feature(um, h, w, splits, shift):
    b, c = 3, 2
    wh, ww = h // splits, w // splits
    rowmap = um._window_rowmap(b, h, w, splits, shift, CPU)
    assert rowmap.dtype == torch.int32 and tuple(rowmap.shape) == (b * splits * splits, wh * ww) and rowmap.is_contiguous()
    assert torch.equal(rowmap.flatten().sort().values, torch.arange(b * h * w, dtype=torch.int32))       # a permutation: no row read twice
    x = torch.randn(b, h * w, c, generator=C.gen(1))
    got = x.reshape(b * h * w, c)[rowmap.long()]                                  # [b k k, wh ww, c]
    img = x.view(b, h, w, c)
    if shift:
        img = torch.roll(img, shifts=(-(wh // 2), -(ww // 2)), dims=(1, 2))
    want = og.split_feature(img.permute(0, 3, 1, 2).contiguous(), splits)        # [b k k, c, wh, ww]
    assert torch.equal(got, want.flatten(2).transpose(1, 2))
    # and the scatter back through the same table is merge_splits + the roll back (attention.py:100-107)
    back = torch.empty(b * h * w, c)
    back[rowmap.long().flatten()] = got.reshape(-1, c)
    assert torch.equal(back.view(b, h * w, c), x)


@pytest.mark.parametrize("h,w,splits", TABLE_SIZES)
def test_coords_tokens_is_coords_grid(um, h, w, splits):
    b = 3
    got = um._coords_tokens(b, h, w, CPU)
    want = og.coords_grid(b, h, w, torch.float32).flatten(2).transpose(1, 2)
    assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == (b, h * w, 2) and torch.equal(got, want)


def test_table_cache_keys_keep_sizes_apart(um):
    """the tables are cached by every argument that shapes them: two sizes asked for in turn do not serve each other's table"""
    a = um._window_rowmap(1, 8, 12, 2, True, CPU)
    b = um._window_rowmap(2, 8, 12, 2, True, CPU)
    c = um._window_rowmap(1, 8, 12, 2, False, CPU)
    assert a.shape != b.shape and not torch.equal(a, c)
    assert um._region_ids(8, 12, 2, CPU).shape != um._region_ids(16, 24, 8, CPU).shape


def test_update_block_restatement_is_the_oracle():
    """gmflow_stages_common.update_block (the carrier of the alterations) with no alteration is og.basic_update_block bit for bit"""
    case = C.update_case(C.UPDATE_SHAPES[1], True)
    for sd, cast in ((C.state(), lambda t: t), (C.state64(), lambda t: t.double())):
        args = [cast(t) for t in (case.net, case.inp, case.corr, case.flow)]
        for a, b in zip(C.update_block(sd, *args, True), og.basic_update_block(sd, *args, True)):
            assert torch.equal(a, b)


CASES = C.all_cases()


@pytest.mark.parametrize("build", [b for _, b in CASES], ids=[i for i, _ in CASES])
def test_case_is_admitted_and_discriminates(build):
    case = build()
    outs = list(case.outs) + list(getattr(case, "outs2", []))
    for o in outs:
        ok, gt, scale = C.admitted(o)
        _, floor, _ = C.gate(o.y32, o.y64)
        print("%-60s gate %.2e  floor %.2e  range %.3g  gate / range %.1e" % (case.name + " / " + o.label, gt, floor, scale, gt / scale))
        assert torch.isfinite(o.y64).all() and torch.isfinite(o.y32).all() and o.y32.dtype == torch.float32 and o.y64.dtype == torch.float64
        assert ok, "%s / %s: gate %.3g is above 1e-3 of the output range %.3g -- wrong data for this case" % (case.name, o.label, gt, scale)
        if o.model is not None:                    # a modelled rms floor never makes the rms rule the looser of the two rules
            assert 0.0 < max(C.F64_RATIO[m][0] for m in C.F64_RATIO) * o.model <= gt, (case.name, o.label, o.model, gt)
    assert case.alts, case.name
    for name, fn in case.alts.items():
        moved = fn()
        assert len(moved) == len(case.outs), (case.name, name)
        worst = max((m - o.y64).abs().max().item() / C.gate(o.y32, o.y64)[0] for m, o in zip(moved, case.outs))
        print("   %-45s moves the output by %.3g gates" % (name, worst))
        assert worst >= MOVE, "%s: '%s' moves the expected output by %.3g gates only" % (case.name, name, worst)


def test_halved_convz1_is_another_case():
    """the in-place weight update of the device test is visible: halving gru.convz1.weight moves every output by over 100 gates"""
    before, after = C.update_case(C.UPDATE_SHAPES[0], True), C.update_case(C.UPDATE_SHAPES[0], True, 0.5)
    for a, b in zip(before.outs, after.outs):
        assert (a.y64 - b.y64).abs().max().item() >= MOVE * max(C.gate(a.y32, a.y64)[0], C.gate(b.y32, b.y64)[0]), a.label


def test_matched_cases_are_peaked():
    """the matched pairs reach the logits the gate's description names: about 16, and above 100 where the float32 oracle is one-hot"""
    soft, hard = C.match_case("matched x1", True), C.match_case("matched x3", True)
    assert 10 <= soft.logit <= 30 and hard.logit >= 100
    o = hard.outs[0]
    assert C.rms(o.y32.double() - o.y64) == 0.0 and C.gate(o.y32, o.y64)[0] == C.G_REL * o.y64.abs().max().item()
    assert C.rms(soft.outs[0].y32.double() - soft.outs[0].y64) > 0.0
