"""Shared by tests/test_pam_edges_host.py and tests/test_pam_edges_gpu.py: parallax-attention inputs that look like a trained
matcher's (one key per query, logits of tens, occluded columns), the float64 reference of everything the two kernel families
(csrc/attention16.hip + its bf16 fallback, csrc/pam.hip) compute from them, the same formula in float32 as a yardstick, and
every bound the GPU file holds the kernels to -- in one place, each with its source.  Torch on the CPU only."""
import functools

import torch

SCALE = 1.0 / 64                  # the reference scales by 1 / c (pasmnet/attention.py:41)
CV, CLIVE, CPAD = 64, 67, 96      # feature channels; + rgb = live channels; the padded value row of pam_streaming_rows

# ---- bounds (the only ones the new files use) ----------------------------------------------------------------------------
# outputs, column sums, map: the error model at the top of csrc/attention16.hip, with the constants of
# tests/test_gmflow_kernels_gpu.py::assert_attention_bound -- (A_REL + A_SMAX smax) sum_j p |v| + A_FLOOR sum_j |v|
A_REL, A_SMAX, A_FLOOR = 5e-6, 4e-7, 2e-12
TINY = 1e-30                      # keeps 0 / 0 out of the elementwise forms (column sums, map)
STAT_TOL = 2e-5                   # row statistics: tests/test_gmflow_kernels_gpu.py::test_attention_rows64_wide_dynamic_range
DISP_TOL = 2e-5                   # x L px: DESIGN 4.10, tests/test_disparity_gpu.py
ROWSUM_TOL = 1e-5                 # a row of a map sums to one: tests/test_dcmcs3di_gpu.py::test_forward_vs_reference_small
KNIFE = 1e-3                      # the mask is compared where |colsum_ref - 0.1| > KNIFE (tests/test_dcmcs3di_gpu.py) ...
KNIFE_SHARE = 0.01                # ... and that may exclude at most this share of a case
R_FACTOR = 2.0                    # map: R = max(1, R_FACTOR x the float32 CPU evaluation's ratio): two independent float32 roundings

CASES = ("flat", "mid", "peaked", "twin", "ramp-up", "ramp-down")
BETA = {"flat": 0.0, "mid": 4.0, "peaked": 40.0, "twin": 40.0}


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def stereo(n, L, beta, seed, twin=False):
    """token rows q, k [n, L, 64]: k ~ N(0,1); a piecewise-constant disparity d per row (segments of length 1..max(2, L//6), shifts
    0..max(1, L//8)); q_i = beta k_pi(i) + N(0,1) with pi(i) = clamp(i - d(i), 0, L-1): a matched logit of about beta over a
    background of standard deviation beta / 8.  twin: every fourth key j has a near-copy at j + 37 (j + L//2 when L <= 74; modulo L): a matched
    query splits its probability between keys of different 32-key tiles."""
    g = torch.Generator().manual_seed(seed)
    k = _randn(g, n, L, 64)
    if twin:
        off = 37 if L > 74 else L // 2
        for j in range(0, L, 4):                   # in key order, so that a copy of a copy is still a near-copy; past the end: wraps
            t = (j + off) % L
            if t != j:
                k[:, t] = k[:, j] + 0.02 * _randn(g, n, 64)
    pi = torch.empty(n, L, dtype=torch.long)
    for r in range(n):
        i = 0
        while i < L:
            seg = int(torch.randint(1, max(2, L // 6) + 1, (1,), generator=g))
            d = int(torch.randint(0, max(1, L // 8) + 1, (1,), generator=g))
            idx = torch.arange(i, min(i + seg, L))
            pi[r, idx] = (idx - d).clamp(0, L - 1)
            i += seg
    q = beta * torch.gather(k, 1, pi[:, :, None].expand(n, L, 64)) + _randn(g, n, L, 64)
    return q, k


def ramp(n, L, seed, rising):
    """k_j = a_j u + 0.01 N(0,1) with a_j linear from -1 to 1 (rising) or 1 to -1 along the keys, q_i = g_i u with g_i in
    [0.5, 1] and |u|^2 / 64 = 30: scores span +-30; rising, the running maximum grows in every key tile"""
    g = torch.Generator().manual_seed(seed)
    u = _randn(g, n, 1, 64)
    u = u * (30.0 * 64) ** 0.5 / u.norm(dim=-1, keepdim=True)
    a = torch.linspace(-1.0, 1.0, L) if rising else torch.linspace(1.0, -1.0, L)
    k = a[None, :, None] * u + 0.01 * _randn(g, n, L, 64)
    gq = 0.5 + 0.5 * torch.rand(n, L, 1, generator=g)
    gq[:, -1] = 1.0
    return gq * u, k


def values(n, L, seed, cv=CV, pad=True):
    """value rows [n, L, 96]: N(0,1) features in channels 0..cv-1, rgb in [0,1] in the next three, zero padding -- the layout
    pam_streaming_rows builds (pad=False: [n, L, cv + 3])"""
    g = torch.Generator().manual_seed(seed)
    v = torch.zeros(n, L, CPAD if pad else cv + 3)
    v[:, :, :cv] = _randn(g, n, L, cv)
    v[:, :, cv:cv + 3] = torch.rand(n, L, 3, generator=g)
    return v


def case_seed(name, L):
    return 7919 * (CASES.index(name) + 1) + L


def inputs(name, n, L):
    seed = case_seed(name, L)
    if name in BETA:
        q, k = stereo(n, L, BETA[name], seed, twin=(name == "twin"))
    else:
        q, k = ramp(n, L, seed + 2, rising=(name == "ramp-up"))
    return q, k, values(n, L, seed + 1)


def rows_to_nchw(t, n, h):
    """[n h, W, C] token rows -> [n, C, h, W] (CPU)"""
    return t.reshape(n, h, t.shape[1], t.shape[2]).permute(0, 3, 1, 2).contiguous()


def nchw_to_rows(t):
    """[n, C, h, W] -> [n h, W, C] (CPU)"""
    n, c, h, w = t.shape
    return t.permute(0, 2, 3, 1).reshape(n * h, w, c).contiguous()


# ---- the reference ------------------------------------------------------------------------------------------------------------
def _evaluate(q, k, v, dtype):
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    sc = torch.matmul(q, k.transpose(1, 2)) / 64
    p = torch.softmax(sc, dim=-1)
    m = sc.max(dim=-1).values
    i, j = torch.arange(q.shape[1], dtype=dtype), torch.arange(k.shape[1], dtype=dtype)
    return {"p": p, "out": torch.matmul(p, v), "m": m, "l": torch.exp(sc - m[..., None]).sum(-1), "colsum": p.sum(dim=1),
            "disp": i[None, :] - torch.matmul(p, j), "smax": sc.abs().amax(dim=(1, 2), keepdim=True), "sc": sc, "v": v}


def reference(q, k, v):
    """float64: p [n,L,L], out = p v, row statistics m = max_j s and l = sum_j exp(s - m), column sums, disp = i - sum_j p_ij j,
    smax = max |s| per row of the batch [n,1,1] (+ the scores and the values it was made from)"""
    return _evaluate(q, k, v, torch.float64)


def reference32(q, k, v):
    """the same formula in float32 on the CPU (matmul / 64, softmax, matmul), results as float64: the yardstick"""
    return {name: t.double() for name, t in _evaluate(q, k, v, torch.float32).items()}


@functools.lru_cache(maxsize=None)
def case(name, n, L):
    """(q, k, v, float64 reference) of a named case, computed once and shared; nobody writes to it"""
    q, k, v = inputs(name, n, L)
    return q, k, v, reference(q, k, v)


# ---- error / bound ratios -----------------------------------------------------------------------------------------------------
def _worst(err, bound):
    return float((err / bound).max()) if err.numel() else 0.0


def out_ratio(out, ref, live=CLIVE):
    """assert_attention_bound's error / bound on the live channels (the GPU file asserts through the imported function itself)"""
    v = ref["v"][:, :, :live]
    bound = (A_REL + A_SMAX * ref["smax"]) * torch.matmul(ref["p"], v.abs()) + A_FLOOR * v.abs().sum(dim=1, keepdim=True) + 1e-300
    return _worst((out[:, :, :live].double() - ref["out"][:, :, :live]).abs(), bound)


def colsum_ratio(colsum, ref):
    bound = (A_REL + A_SMAX * ref["smax"][:, :, 0]) * ref["colsum"] + TINY
    return _worst((colsum.double() - ref["colsum"]).abs(), bound)


def stats_ratio(stats, ref):
    """max of the two: |m - m_ref| / (STAT_TOL max(1, max |m|)) and the relative error of l / STAT_TOL"""
    st = stats.double()
    rm = float((st[..., 0] - ref["m"]).abs().max()) / (STAT_TOL * max(1.0, float(ref["m"].abs().max())))
    rl = float(((st[..., 1] - ref["l"]).abs() / ref["l"]).max()) / STAT_TOL
    return max(rm, rl)


def disp_ratio(disp, ref):
    return float((disp.double() - ref["disp"]).abs().max()) / (DISP_TOL * ref["disp"].shape[1])


def map_ratio(att, ref):
    """|att - p| / ((A_REL + A_SMAX smax) p + TINY): to be held under map_R(...)"""
    return _worst((att.double() - ref["p"]).abs(), (A_REL + A_SMAX * ref["smax"]) * ref["p"] + TINY)


def map_R(q, k, v, ref):
    """R of the materialised map: from the float32 CPU evaluation of the same inputs, never from a kernel"""
    return max(1.0, R_FACTOR * map_ratio(reference32(q, k, v)["p"], ref))


def knife_share(ref):
    return float(((ref["colsum"] - 0.1).abs() <= KNIFE).double().mean())


def mask_mismatches(valid, ref):
    """entries of a 0/1 (or bool) mask that differ from colsum_ref > 0.1 away from the knife edge"""
    safe = (ref["colsum"] - 0.1).abs() > KNIFE
    return int(((valid.double() > 0.5) != (ref["colsum"] > 0.1))[safe].sum())


def ratios(got, ref):
    """error / bound of every quantity present in `got` (out, stats, colsum, disp, att)"""
    fn = {"out": out_ratio, "stats": stats_ratio, "colsum": colsum_ratio, "disp": disp_ratio, "att": map_ratio}
    return {name: fn[name](got[name], ref) for name in fn if name in got}


def as_kernel_outputs(ev):
    """an evaluation (reference32, or a deliberately wrong one) in the form of a kernel's outputs"""
    return {"out": ev["out"], "stats": torch.stack([ev["m"], ev["l"]], dim=-1), "colsum": ev["colsum"], "disp": ev["disp"], "att": ev["p"]}


# ---- geometry of the LDS-tile family from its public entry ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pam_geometry(sweep=2100):
    """(heights, W32, Wmax): ct_pam_workspace_bytes(1, 1, W) / (4 W) is the number of query tiles of width W, zero = refused;
    heights[W] in {32, 16, 0}; W32 = last width on 32-query tiles, Wmax = last accepted width"""
    import ct_hip
    lib = ct_hip.lib()
    heights = {}
    for w in range(1, sweep + 1):
        b = lib.ct_pam_workspace_bytes(1, 1, w)
        assert b % (4 * w) == 0, (w, b)
        tiles = b // (4 * w)
        if tiles == 0:
            heights[w] = 0
        elif tiles == (w + 31) // 32:
            heights[w] = 32
        else:
            assert tiles == (w + 15) // 16, (w, tiles)
            heights[w] = 16
    w32 = max(w for w, t in heights.items() if t == 32)
    wmax = max(w for w, t in heights.items() if t != 0)
    return heights, w32, wmax
