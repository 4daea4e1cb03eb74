"""Both parallax-attention kernel families against float64 at their edges, on inputs that look like a trained matcher's
(tests/pam_edges_common.py: one-hot rows, logits of 40-80, occluded columns, probabilities split between key tiles, ramps that move
the running maximum in every tile):

* the streaming family (csrc/attention16.hip, or the three-piece bf16 kernels of csrc/attention_tokens.hip under CT_HIP_ATT16=0)
  through ct_attention_rows64_f32 / ct_attention_rows64_disp_f32 / ct_attention_colsum64_f32: every length around its 32-key tile
  and 128-query workgroup, the workgroup remap of xcd_order, stray writes, NaN locality, refusals;
* the LDS-tile family (csrc/pam.hip) through ct_hip.pam_attend / pam_valid: widths around its 4-float vectors and 64 / 128-key
  chunks, misaligned bases, the 32 -> 16 query switch and the width limit as tests/test_pam_edges_host.py derives them, value widths.

Every bound comes from tests/pam_edges_common.py; every test prints its worst error / bound ratio on a line starting with
`[pam-edges]` (DESIGN 4.4 has the table)."""
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import pam_edges_common as pc                                  # noqa: E402
from tests.test_gmflow_kernels_gpu import assert_attention_bound          # noqa: E402

CT_OK, CT_E_BADARG, CT_E_ALIGN = 0, -1, -3      # include/ct_hip.h
LENGTHS = (1, 2, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 255, 256, 257, 385)
GRIDS = ((129, 4), (33, 9), (33, 17), (385, 6), (257, 11))      # (L, n): 8, 9, 17, 24 and 33 workgroups
WIDTHS = (1, 2, 3, 4, 5, 7, 8, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130, 191, 257)
SENT = -7.25                                     # sentinel of the stray-write checks


@pytest.fixture(scope="module")
def hip():
    import ct_hip
    ct_hip.lib()
    return ct_hip


def report(family, what, r):
    print("\n[pam-edges] %s %s: %s" % (family, what, " ".join("%s=%.4g" % kv for kv in r.items())))


# ---- the streaming family -------------------------------------------------------------------------------------------------------------
def streaming(hip, q, k, v):
    """every entry of the family on token rows q, k [n, L, 64], v [n, L, 96]; results on the CPU"""
    lib, (n, L, _) = hip.lib(), q.shape
    qc, kc, vc = q.cuda(), k.cuda(), v.cuda()
    out, out_d = torch.empty(n, L, 96, device="cuda"), torch.empty(n, L, 96, device="cuda")
    stats, colsum = torch.empty(n, L, 2, device="cuda"), torch.empty(n, L, device="cuda")
    disp, disp_i = torch.empty(n, L, device="cuda"), torch.empty(n, L, device="cuda")
    hip.check(lib.ct_attention_rows64_f32(qc.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), None, n, L, pc.SCALE, None))
    hip.check(lib.ct_attention_rows64_f32(qc.data_ptr(), kc.data_ptr(), None, None, stats.data_ptr(), n, L, pc.SCALE, None))
    hip.check(lib.ct_attention_colsum64_f32(qc.data_ptr(), kc.data_ptr(), stats.data_ptr(), colsum.data_ptr(), n, L, pc.SCALE, None))
    hip.check(lib.ct_attention_rows64_disp_f32(qc.data_ptr(), kc.data_ptr(), vc.data_ptr(), out_d.data_ptr(), disp.data_ptr(), n, L, pc.SCALE, None))
    hip.check(lib.ct_attention_rows64_disp_f32(qc.data_ptr(), kc.data_ptr(), None, None, disp_i.data_ptr(), n, L, pc.SCALE, None))
    return {name: t.cpu() for name, t in (("out", out), ("out_disp", out_d), ("stats", stats), ("colsum", colsum), ("disp", disp),
                                          ("disp_index_only", disp_i))}


def hold_streaming(got, ref, what, family="streaming"):
    """out, statistics, column sums, both disparities and the mask under the bounds of tests/pam_edges_common.py"""
    r = pc.ratios(got, ref)
    r["disp_index_only"] = pc.disp_ratio(got["disp_index_only"], ref)
    report(family, what, r)
    live = slice(0, pc.CLIVE)
    assert_attention_bound(got["out"][:, :, live].double(), ref["out"][:, :, live], ref["sc"], ref["p"], ref["v"][:, :, live], what)
    assert r["stats"] < 1.0 and r["colsum"] < 1.0 and r["disp"] < 1.0 and r["disp_index_only"] < 1.0, (what, r)
    assert pc.knife_share(ref) <= pc.KNIFE_SHARE and pc.mask_mismatches(got["colsum"] > 0.1, ref) == 0, what
    assert (got["out"][:, :, pc.CLIVE:] == 0).all(), "%s: the padding channels of out are not exactly zero" % what
    assert torch.equal(got["out_disp"], got["out"]), "%s: out of the _disp entry is not bitwise out of the plain one" % what
    return r


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("name", pc.CASES)
def test_streaming_lengths(hip, name, L):
    """3 rows at every edge of the 32-key tile and the 128-query workgroup: full tiles, one key more, one key less, a ragged last
    tile together with live and dead queries in one wave"""
    q, k, v, ref = pc.case(name, 3, L)
    hold_streaming(streaming(hip, q, k, v), ref, "%s L=%d" % (name, L))


@pytest.mark.parametrize("L,n", GRIDS)
def test_streaming_grid_order(hip, L, n):
    """xcd_order remaps workgroups from 8 of them on and leaves the last total % 8 alone: a row computed alone (one or a few
    workgroups, no remap below 8) is bitwise the same row of the batched call (grids of 8, 9, 17, 24, 33), twice"""
    q, k, v, ref = pc.case("twin", n, L)
    got = streaming(hip, q, k, v)
    hold_streaming(got, ref, "twin L=%d n=%d" % (L, n))
    again = streaming(hip, q, k, v)
    for name in got:
        assert torch.equal(again[name], got[name]), "two batched calls differ in %s" % name
    for r in range(n):
        alone = streaming(hip, q[r:r + 1], k[r:r + 1], v[r:r + 1])
        for name in got:
            assert torch.equal(alone[name][0], got[name][r]), "row %d alone differs from the batch in %s" % (r, name)


@pytest.mark.parametrize("L", [33, 129])
def test_streaming_writes_only_its_output(hip, L):
    """every output is a slice of a larger buffer: the four rows before and after it keep their sentinel"""
    lib, n = hip.lib(), 3
    q, k, v, ref = pc.case("peaked", n, L)
    qc, kc, vc = q.cuda(), k.cuda(), v.cuda()
    big = {name: torch.full((n + 8, L, c), SENT, device="cuda") for name, c in (("out", 96), ("out_disp", 96), ("stats", 2), ("colsum", 1),
                                                                                ("disp", 1), ("disp_index_only", 1))}
    p = {name: t[4:4 + n].data_ptr() for name, t in big.items()}
    hip.check(lib.ct_attention_rows64_f32(qc.data_ptr(), kc.data_ptr(), vc.data_ptr(), p["out"], None, n, L, pc.SCALE, None))
    hip.check(lib.ct_attention_rows64_f32(qc.data_ptr(), kc.data_ptr(), None, None, p["stats"], n, L, pc.SCALE, None))
    hip.check(lib.ct_attention_colsum64_f32(qc.data_ptr(), kc.data_ptr(), p["stats"], p["colsum"], n, L, pc.SCALE, None))
    hip.check(lib.ct_attention_rows64_disp_f32(qc.data_ptr(), kc.data_ptr(), vc.data_ptr(), p["out_disp"], p["disp"], n, L, pc.SCALE, None))
    hip.check(lib.ct_attention_rows64_disp_f32(qc.data_ptr(), kc.data_ptr(), None, None, p["disp_index_only"], n, L, pc.SCALE, None))
    got = {}
    for name, t in big.items():
        t = t.cpu()
        assert (t[:4] == SENT).all() and (t[4 + n:] == SENT).all(), "%s: written outside its %d rows" % (name, n)
        got[name] = t[4:4 + n] if name in ("out", "out_disp", "stats") else t[4:4 + n, :, 0]
    hold_streaming(got, ref, "peaked L=%d inside sentinels" % L)


@pytest.mark.parametrize("where", ["query", "key", "value"])
def test_streaming_nan_stays_where_the_reference_puts_it(hip, where):
    """row 2 of 4 carries one NaN.  In a query: that query's outputs only; in a key: every output of the row; in one value channel
    of a key: that channel of every output of the row (the column sums and the disparity do not read the values).  The float64
    reference decides; what it leaves finite stays inside the bounds, and the three clean rows are bitwise what they are without
    the NaN.  Of the row statistics the sum is held to the same rule (exp(NaN - m) is NaN whatever m is); the maximum is not compared
    in the poisoned row: torch.max propagates a NaN, IEEE's maxNum -- v_max_f32 -- returns the other operand."""
    n, L, row, at, ch = 4, 129, 2, 70, 9
    q, k, v, clean_ref = pc.case("twin", n, L)
    clean = streaming(hip, q, k, v)
    q, k, v = q.clone(), k.clone(), v.clone()
    {"query": q, "key": k, "value": v}[where][row, at, ch] = float("nan")
    ref = pc.reference(q, k, v)
    got = streaming(hip, q, k, v)
    others = [r for r in range(n) if r != row]
    for name in ("out", "out_disp", "stats", "colsum", "disp", "disp_index_only"):
        assert torch.equal(got[name][others], clean[name][others]), "%s of a clean row changed" % name
    got["l"] = got["stats"][..., 1]
    for name, want in (("out", ref["out"]), ("out_disp", ref["out"]), ("l", ref["l"]), ("colsum", ref["colsum"]), ("disp", ref["disp"]),
                       ("disp_index_only", ref["disp"])):
        assert torch.equal(torch.isnan(got[name][row]), torch.isnan(want[row])), "%s: NaN pattern of %s differs from float64's" % (where, name)
    assert (got["out"][:, :, pc.CLIVE:][~torch.isnan(got["out"][:, :, pc.CLIVE:])] == 0).all()
    # what the reference leaves finite in the poisoned row, under the same bounds (from the clean reference restricted to it)
    qs = [i for i in range(L) if i != at] if where == "query" else list(range(L))
    cs = [c for c in range(pc.CLIVE) if not (where == "value" and c == ch)]
    if where != "key":
        pick = lambda t: t[row:row + 1][:, qs]
        assert_attention_bound(pick(got["out"])[:, :, cs].double(), pick(clean_ref["out"])[:, :, cs], pick(clean_ref["sc"]),
                               pick(clean_ref["p"]), clean_ref["v"][row:row + 1][:, :, cs], "finite outputs beside the NaN (%s)" % where)
        assert float((pick(got["disp"]).double() - pick(clean_ref["disp"])).abs().max()) <= pc.DISP_TOL * L
    if where == "value":
        one = {name: t[row:row + 1] for name, t in clean_ref.items()}
        assert pc.colsum_ratio(got["colsum"][row:row + 1], one) < 1.0 and pc.stats_ratio(got["stats"][row:row + 1], one) < 1.0
    report("streaming", "NaN in one %s" % where, {"nan_outputs": float(torch.isnan(got["out"]).sum())})


def test_streaming_refusals(hip):
    """misaligned q / k / v / out: CT_E_ALIGN; len < 1 and missing pointers: CT_E_BADARG; batch == 0: CT_OK -- and nothing written"""
    lib, n, L = hip.lib(), 2, 33
    q, k, v, _ = pc.case("peaked", 3, L)
    qc, kc, vc = q[:n].cuda(), k[:n].cuda(), v[:n].cuda()
    spare = torch.zeros(n * L * 96 + 4, device="cuda")              # an operand that starts one float into its storage
    off = spare.data_ptr() + 4
    out, stats = torch.full((n, L, 96), SENT, device="cuda"), torch.full((n, L, 2), SENT, device="cuda")
    colsum, disp = torch.full((n, L), SENT, device="cuda"), torch.full((n, L), SENT, device="cuda")
    Q, K, V, O, S, C, D = (t.data_ptr() for t in (qc, kc, vc, out, stats, colsum, disp))
    rows64, rows64_disp, colsum64 = lib.ct_attention_rows64_f32, lib.ct_attention_rows64_disp_f32, lib.ct_attention_colsum64_f32
    for args in ((off, K, V, O), (Q, off, V, O), (Q, K, off, O), (Q, K, V, off)):
        assert rows64(*args, None, n, L, pc.SCALE, None) == CT_E_ALIGN
        assert rows64_disp(*args, D, n, L, pc.SCALE, None) == CT_E_ALIGN
    assert rows64(off, K, None, None, S, n, L, pc.SCALE, None) == CT_E_ALIGN
    assert colsum64(off, K, S, C, n, L, pc.SCALE, None) == CT_E_ALIGN and colsum64(Q, off, S, C, n, L, pc.SCALE, None) == CT_E_ALIGN
    for length in (0, -1):
        assert rows64(Q, K, V, O, None, n, length, pc.SCALE, None) == CT_E_BADARG
        assert rows64_disp(Q, K, V, O, D, n, length, pc.SCALE, None) == CT_E_BADARG
        assert colsum64(Q, K, S, C, n, length, pc.SCALE, None) == CT_E_BADARG
    assert rows64(None, K, V, O, None, n, L, pc.SCALE, None) == CT_E_BADARG and rows64(Q, None, V, O, None, n, L, pc.SCALE, None) == CT_E_BADARG
    assert rows64(Q, K, V, None, None, n, L, pc.SCALE, None) == CT_E_BADARG           # values without an output
    assert rows64(Q, K, None, None, None, n, L, pc.SCALE, None) == CT_E_BADARG        # neither values nor statistics
    assert rows64(Q, K, V, O, None, -1, L, pc.SCALE, None) == CT_E_BADARG
    assert rows64_disp(None, K, V, O, D, n, L, pc.SCALE, None) == CT_E_BADARG and rows64_disp(Q, K, V, O, None, n, L, pc.SCALE, None) == CT_E_BADARG
    assert rows64_disp(Q, K, V, None, D, n, L, pc.SCALE, None) == CT_E_BADARG
    assert colsum64(Q, K, None, C, n, L, pc.SCALE, None) == CT_E_BADARG and colsum64(Q, K, S, None, n, L, pc.SCALE, None) == CT_E_BADARG
    assert rows64(Q, K, V, O, None, 0, L, pc.SCALE, None) == CT_OK and rows64(Q, K, None, None, S, 0, L, pc.SCALE, None) == CT_OK
    assert rows64_disp(Q, K, V, O, D, 0, L, pc.SCALE, None) == CT_OK and colsum64(Q, K, S, C, 0, L, pc.SCALE, None) == CT_OK
    torch.cuda.synchronize()
    for name, t in (("out", out), ("stats", stats), ("colsum", colsum), ("disp", disp)):
        assert (t == SENT).all(), "a refused or empty call wrote to %s" % name


@pytest.mark.parametrize("h,w", [(3, 33), (2, 129)])
def test_streaming_through_the_binding(hip, h, w):
    """ct_hip.pam_streaming on NCHW tensors (2 images): the row transposes, the rgb channels of the 96-channel value and the 0.1
    threshold of the mask are part of what is compared"""
    b = 2
    q, k, v, ref = pc.case("peaked", b * h, w)
    qo, ko, _, ref_o = pc.case("twin", b * h, w)                  # the other direction: only its column sums are used
    nchw = lambda t: pc.rows_to_nchw(t, b, h).cuda()
    fea, wrgb, valid, colsum, disp = hip.pam_streaming(nchw(q), nchw(k), nchw(v[:, :, :64]), nchw(v[:, :, 64:67]), nchw(qo), nchw(ko),
                                                       want_disp=True)
    assert fea.shape == (b, 64, h, w) and wrgb.shape == (b, 3, h, w) and valid.shape == colsum.shape == disp.shape == (b, 1, h, w)
    out = torch.cat([pc.nchw_to_rows(fea.cpu()), pc.nchw_to_rows(wrgb.cpu())], dim=2)
    live = slice(0, pc.CLIVE)
    cs, va, di = (pc.nchw_to_rows(t.cpu())[:, :, 0] for t in (colsum, valid, disp))
    r = {"out": pc.out_ratio(out, ref), "colsum": pc.colsum_ratio(cs, ref_o), "disp": pc.disp_ratio(di, ref)}
    report("streaming", "pam_streaming %dx%d" % (h, w), r)
    assert_attention_bound(out.double(), ref["out"][:, :, live], ref["sc"], ref["p"], ref["v"][:, :, live], "pam_streaming")
    assert r["colsum"] < 1.0 and r["disp"] < 1.0, r
    assert ((va == 0) | (va == 1)).all() and pc.knife_share(ref_o) <= pc.KNIFE_SHARE and pc.mask_mismatches(va, ref_o) == 0


# ---- the LDS-tile family --------------------------------------------------------------------------------------------------------------
def tiles(hip, q, k, v, n, h, want_att=True, prepare=lambda t: t.cuda()):
    """ct_hip.pam_attend + pam_valid on the NCHW views of token rows q, k [n h, W, 64], v [n h, W, cv + 3]; results as rows on the CPU"""
    cv = v.shape[2] - 3
    qn, kn = prepare(pc.rows_to_nchw(q, n, h)), prepare(pc.rows_to_nchw(k, n, h))
    vn, rgb = prepare(pc.rows_to_nchw(v[:, :, :cv].contiguous(), n, h)), prepare(pc.rows_to_nchw(v[:, :, cv:].contiguous(), n, h))
    out_v, out_rgb, att = hip.pam_attend(qn, kn, vn, rgb, want_att=want_att)
    valid, colsum, att2 = hip.pam_valid(qn, kn, want_att=want_att)
    got = {"out": torch.cat([pc.nchw_to_rows(out_v.cpu()), pc.nchw_to_rows(out_rgb.cpu())], dim=2),
           "colsum": pc.nchw_to_rows(colsum.cpu())[:, :, 0], "valid": pc.nchw_to_rows(valid.cpu())[:, :, 0]}
    if want_att:
        W = q.shape[1]
        got["att"], got["att_valid"] = att.cpu().view(n * h, W, W), att2.cpu().view(n * h, W, W)
    return got


def hold_tiles(got, q, k, v, ref, what):
    live = v.shape[2]
    r = {"out": pc.out_ratio(got["out"], ref, live), "colsum": pc.colsum_ratio(got["colsum"], ref)}
    R = pc.map_R(q, k, v, ref)
    for name in ("att", "att_valid"):
        if name in got:
            r[name] = pc.map_ratio(got[name], ref) / R                  # relative to R x the bound: < 1 passes
    r["R"] = R
    report("tiles", what, r)
    assert_attention_bound(got["out"].double(), ref["out"][:, :, :live], ref["sc"], ref["p"], ref["v"][:, :, :live], what)
    assert r["colsum"] < 1.0, (what, r)
    assert ((got["valid"] == 0) | (got["valid"] == 1)).all()
    assert pc.knife_share(ref) <= pc.KNIFE_SHARE and pc.mask_mismatches(got["valid"], ref) == 0, what
    for name in ("att", "att_valid"):
        if name in got:
            assert r[name] < 1.0, (what, name, r)
            assert float((got[name].double().sum(dim=-1) - 1.0).abs().max()) <= pc.ROWSUM_TOL, "%s: a row of %s does not sum to one" % (what, name)
            assert float(got[name].min()) >= 0.0 and float(got[name].max()) <= 1.0, "%s: %s leaves [0, 1]" % (what, name)
    return r


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("name", ["flat", "peaked", "twin"])
def test_tiles_widths(hip, name, W):
    """2 images of 3 rows at W < 4, W = 1, 2, 3 mod 4 around the 64-key (P.V) and 128-key (scores) chunks, one and several query
    tiles: warped features and rgb, both materialised maps, column sums, mask"""
    q, k, v, ref = pc.case(name, 6, W)
    v = v[:, :, :pc.CLIVE]
    hold_tiles(tiles(hip, q, k, v, 2, 3), q, k, v, dict(ref, v=ref["v"][:, :, :pc.CLIVE], out=ref["out"][:, :, :pc.CLIVE]),
               "%s W=%d" % (name, W))


@pytest.mark.parametrize("which", ["W32", "W32+1", "Wmax-1", "Wmax"])
def test_tiles_switch_and_limit(hip, which):
    """the last width on 32-query tiles, the first on 16, and the two widest the family accepts, as the host derivation gives them
    (tests/test_pam_edges_host.py), one row, maps included"""
    _, w32, wmax = pc.pam_geometry()
    W = {"W32": w32, "W32+1": w32 + 1, "Wmax-1": wmax - 1, "Wmax": wmax}[which]
    q, k, v = pc.inputs("twin", 1, W)
    v = v[:, :, :pc.CLIVE].contiguous()
    ref = pc.reference(q, k, v)
    hold_tiles(tiles(hip, q, k, v, 1, 1), q, k, v, ref, "twin %s=%d" % (which, W))


def test_tiles_refuse_one_past_the_limit(hip):
    lib = hip.lib()
    _, _, wmax = pc.pam_geometry()
    W = wmax + 1
    assert lib.ct_pam_workspace_bytes(1, 1, W) == 0
    q, k = torch.zeros(1, 64, 1, W, device="cuda"), torch.zeros(1, 64, 1, W, device="cuda")
    v, rgb = torch.zeros(1, 64, 1, W, device="cuda"), torch.zeros(1, 3, 1, W, device="cuda")
    outs = [torch.full(s, SENT, device="cuda") for s in ((1, 64, 1, W), (1, 3, 1, W), (1, 1, 1, W), (1, 1, 1, W))]
    ws = torch.zeros(1024, device="cuda")
    assert lib.ct_pam_attend_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), rgb.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), None,
                                 1, 64, 64, 1, W, None) == CT_E_BADARG
    assert lib.ct_pam_valid_f32(q.data_ptr(), k.data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), None, 1, 64, 1, W, ws.data_ptr(),
                                ws.numel() * 4, None) == CT_E_BADARG
    with pytest.raises(hip.CtHipError):
        hip.pam_attend(q, k, v, rgb)
    torch.cuda.synchronize()
    assert all((t == SENT).all() for t in outs)


@pytest.mark.parametrize("W", [64, 128])
def test_tiles_misaligned_bases(hip, W):
    """W % 4 == 0 with every input starting one float into its storage: the `vec` / `vecv` predicates must send it down the scalar
    staging path, whose result is bitwise the aligned call's"""
    q, k, v, ref = pc.case("twin", 6, W)
    v = v[:, :, :pc.CLIVE]

    def shifted(t):
        store = torch.empty(t.numel() + 1, device="cuda")
        view = store[1:].view(t.shape)
        view.copy_(t)
        assert view.is_contiguous() and view.data_ptr() % 16 == 4
        return view
    aligned = tiles(hip, q, k, v, 2, 3)
    off = tiles(hip, q, k, v, 2, 3, prepare=shifted)
    for name in aligned:
        assert torch.equal(off[name], aligned[name]), "%s differs between aligned and misaligned bases" % name
    hold_tiles(off, q, k, v, dict(ref, v=ref["v"][:, :, :pc.CLIVE], out=ref["out"][:, :, :pc.CLIVE]), "twin W=%d misaligned" % W)


@pytest.mark.parametrize("cv", [1, 16, 93])
def test_tiles_value_widths(hip, cv):
    W, n, h = 65, 2, 3
    q, k, _, _ = pc.case("twin", n * h, W)
    v = pc.values(n * h, W, 500 + cv, cv=cv, pad=False)
    ref = pc.reference(q, k, v)
    hold_tiles(tiles(hip, q, k, v, n, h, want_att=False), q, k, v, ref, "twin W=65 cv=%d" % cv)


def test_tiles_refuse_other_channel_counts(hip):
    lib, W = hip.lib(), 65
    z = lambda c: torch.zeros(1, c, 1, W, device="cuda")
    q, k, rgb, ws = z(64), z(64), z(3), torch.zeros(1024, device="cuda")
    ov, orgb, valid = torch.full((1, 94, 1, W), SENT, device="cuda"), torch.full((1, 3, 1, W), SENT, device="cuda"), torch.full((1, 1, 1, W), SENT, device="cuda")
    v = z(94)
    attend = lambda c, cv: lib.ct_pam_attend_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), rgb.data_ptr(), ov.data_ptr(), orgb.data_ptr(),
                                                 None, 1, c, cv, 1, W, None)
    assert attend(64, 94) == CT_E_BADARG and attend(64, 0) == CT_E_BADARG
    for c in (32, 63, 65, 128):
        assert attend(c, 64) == CT_E_BADARG
        assert lib.ct_pam_valid_f32(q.data_ptr(), k.data_ptr(), valid.data_ptr(), None, None, 1, c, 1, W, ws.data_ptr(), ws.numel() * 4,
                                    None) == CT_E_BADARG
    torch.cuda.synchronize()
    assert (ov == SENT).all() and (orgb == SENT).all() and (valid == SENT).all()


def test_tiles_row_independence(hip):
    """2 images x 3 rows against the six rows run one at a time: bit for bit"""
    W = 129
    q, k, v, _ = pc.case("twin", 6, W)
    v = v[:, :, :pc.CLIVE]
    batch = tiles(hip, q, k, v, 2, 3)
    for r in range(6):
        alone = tiles(hip, q[r:r + 1], k[r:r + 1], v[r:r + 1], 1, 1)
        for name in batch:
            assert torch.equal(alone[name][0], batch[name][r]), "row %d alone differs from the batch in %s" % (r, name)


@pytest.mark.parametrize("W", [33, 129, 257])
def test_families_agree(hip, W):
    """what forward(inference=True) against forward_parts(want_att=True) relies on: each family within its bound of float64, hence
    within the sum of the two bounds of the other"""
    q, k, v, ref = pc.case("twin", 6, W)
    live = slice(0, pc.CLIVE)
    s = streaming(hip, q, k, v)
    t = tiles(hip, q, k, v[:, :, live], 2, 3, want_att=False)
    ref_live = dict(ref, v=ref["v"][:, :, live], out=ref["out"][:, :, live])
    for got, what in ((s["out"][:, :, live], "streaming"), (t["out"], "tiles")):
        assert_attention_bound(got.double(), ref_live["out"], ref["sc"], ref["p"], ref_live["v"], what)
    assert pc.colsum_ratio(s["colsum"], ref) < 1.0 and pc.colsum_ratio(t["colsum"], ref) < 1.0
    vabs = ref_live["v"].abs()
    bound = (pc.A_REL + pc.A_SMAX * ref["smax"]) * torch.matmul(ref["p"], vabs) + pc.A_FLOOR * vabs.sum(dim=1, keepdim=True) + 1e-300
    d_out = (s["out"][:, :, live].double() - t["out"].double()).abs()
    d_cs = (s["colsum"].double() - t["colsum"].double()).abs()
    cs_bound = (pc.A_REL + pc.A_SMAX * ref["smax"][:, :, 0]) * ref["colsum"] + pc.TINY
    r = {"out_diff_over_2_bounds": float((d_out / (2 * bound)).max()), "colsum_diff_over_2_bounds": float((d_cs / (2 * cs_bound)).max()),
         "out_diff_max_abs": float(d_out.max()), "colsum_diff_max_abs": float(d_cs.max())}
    report("both", "twin W=%d streaming vs tiles" % W, r)
    assert r["out_diff_over_2_bounds"] < 1.0 and r["colsum_diff_over_2_bounds"] < 1.0
    assert pc.mask_mismatches(t["valid"], ref) == 0 and pc.mask_mismatches(s["colsum"] > 0.1, ref) == 0
