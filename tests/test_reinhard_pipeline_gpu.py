"""The fused float32 Reinhard entries with their two table sweeps run over chunks of pairs on two lanes, the caller's stream and a library-owned one
(csrc/linear.hip: reinhard_pipelined; include/ct_hip.h: ct_set_reinhard_pipeline): ragged frames and ragged chunk counts against
the float64 oracle and against the whole-batch launches of the same build, determinism, aliasing, every case that must keep the
whole-batch launches, graph capture, several callers.

Bounds (tests/test_linear_gpu.py, table arithmetic): Lab of the result <= 5e-5 (the gate is 1e-4), float32 RGB <= 6e-6, statistics
<= 3e-6.  The PSNR record has no bound of its own there; it follows from the RGB one: with d = ref - gt and e = out - ref,
|mean((d + e)^2) - mean(d^2)| <= 2 max|e| mean|d| + max|e|^2, and the float64 sums themselves add ~1e-16 relative."""
import contextlib
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import lab as olab        # noqa: E402
from oracle import linear as olin     # noqa: E402

LAB_TIGHT, STATS_TOL, RGB_TOL = 5e-5, 3e-6, 6e-6
SHAPES = [(37, 53), (16, 16), (5, 7)]        # 7 tiles + a ragged tail; exactly one tile; no full tile
BATCHES = [1, 2, 5, 7]
CHUNKS = [1, 2, 3]                            # ragged last chunk, batch < one chunk, odd chunk counts on two streams
POLICIES = ["nt", "plain"]
# frames big enough that the per-image workgroup count of a chunk launch differs from the whole-batch launch's (468 tiles, 59
# workgroups wanted; 14 images share the chip at 36 each): there the two forms differ in the last bits of the statistics, so a
# byte-for-byte match with the whole-batch form shows which form ran
BIG, BIG_BATCH = (300, 400), 7


@pytest.fixture(scope="module")
def hip():
    import ct_hip
    ct_hip.lib()
    return ct_hip


@contextlib.contextmanager
def plan(hip, chunk_pairs, policy=-1):
    hip.set_reinhard_pipeline(chunk_pairs, policy)
    try:
        yield
    finally:
        hip.set_reinhard_pipeline(-1, -1)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def frames(seed, batch, shape):
    """targets over the whole range, references and ground truth in narrower ones (distinct statistics per pair)"""
    rng = np.random.default_rng(seed)
    t = rng.random((batch,) + shape + (3,), dtype=np.float32)
    r = (rng.random((batch,) + shape + (3,), dtype=np.float32) * np.float32(0.5) + np.float32(0.25)).astype(np.float32)
    g = (rng.random((batch,) + shape + (3,), dtype=np.float32) * np.float32(0.8) + np.float32(0.1)).astype(np.float32)
    return t, r, g


def run(hip, t, r, g=None, out=None):
    """one call on device tensors -> (out, records [2B, 8], psnr [B, 2] or None), all cloned to the host after a synchronise"""
    B = t.shape[0]
    st = torch.zeros((2 * B, 8), dtype=torch.float64, device="cuda")
    if g is None:
        o = hip.reinhard(t, r, out=out, stats_out=st)
        ps = None
    else:
        o, ps = hip.reinhard_psnr(t, r, g, out=out, stats_out=st)
    torch.cuda.synchronize()
    return o.cpu().numpy().copy(), st.cpu().numpy().copy(), None if ps is None else ps.cpu().numpy().copy()


def same_bytes(a, b):
    return all((x is None and y is None) or (x.tobytes() == y.tobytes()) for x, y in zip(a, b))


def mse_bound(ref, g, tol):
    return 2.0 * tol * np.abs(ref.astype(np.float64) - g).mean() + tol * tol + 1e-15


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("shape", SHAPES)
def test_chunks_vs_oracle_and_whole_batch(hip, shape, batch):
    t, r, g = frames(1000 * shape[0] + batch, batch, shape)
    ref = np.stack([olin.color_transfer_between_images(t[b], r[b]) for b in range(batch)])
    rec = np.zeros((2 * batch, 6))
    for b in range(batch):
        for row, img in ((b, t[b]), (batch + b, r[b])):
            m, s = olin.lab_stats(img)
            rec[row, 0:3], rec[row, 3:6] = m, s
    lab_ref = olab.rgb2lab(ref.astype(np.float64))
    mse_ref = ((ref.astype(np.float64) - g) ** 2).reshape(batch, -1).mean(axis=1)
    dt, dr, dg = dev(t), dev(r), dev(g)
    with plan(hip, 0):
        whole = {False: run(hip, dt, dr), True: run(hip, dt, dr, dg)}
    n = shape[0] * shape[1]
    for chunk in CHUNKS:
        for policy in POLICIES:
            for with_gt in (False, True):
                what = "chunk %d, %s, gt %s" % (chunk, policy, with_gt)
                with plan(hip, chunk, policy):
                    assert hip.reinhard_pipeline_chunk(n, batch) == chunk
                    out, st, ps = run(hip, dt, dr, dg if with_gt else None)
                    again = run(hip, dt, dr, dg if with_gt else None)
                assert same_bytes((out, st, ps), again), what + ": two runs differ"
                # against the float64 oracle
                e_rgb = np.abs(out.astype(np.float64) - ref).max()
                e_lab = np.abs(olab.rgb2lab(out.astype(np.float64)) - lab_ref).max()
                e_st = np.abs(st[:, 0:6] - rec).max()
                print("%s %s x %d: rgb %.3g lab %.3g stats %.3g" % (what, shape, batch, e_rgb, e_lab, e_st))
                assert e_rgb <= RGB_TOL and e_lab <= LAB_TIGHT and e_st <= STATS_TOL, what
                assert (st[:, 6] == n).all(), what
                # against the whole-batch launches of the same build
                w_out, w_st, w_ps = whole[with_gt]
                assert np.abs(out.astype(np.float64) - w_out).max() <= RGB_TOL, what
                assert np.abs(st[:, 0:6] - w_st[:, 0:6]).max() <= STATS_TOL, what
                if with_gt:
                    for b in range(batch):
                        bound = mse_bound(ref[b], g[b], RGB_TOL)
                        assert abs(ps[b, 0] - mse_ref[b]) <= bound, what
                        assert abs(ps[b, 0] - w_ps[b, 0]) <= 2 * bound, what            # both within `bound` of the oracle
                        assert abs(ps[b, 1] - 10.0 * np.log10(1.0 / ps[b, 0])) <= 1e-9, what


@pytest.fixture(scope="module")
def big(hip):
    """BIG frames: the device tensors, the whole-batch result and one forced-chunk result, which must differ from it somewhere
    (otherwise the byte-for-byte tests below would show nothing)"""
    t, r, g = (dev(a) for a in frames(77, BIG_BATCH, BIG))
    with plan(hip, 0):
        whole = run(hip, t, r, g)
    with plan(hip, 2, "nt"):
        piped = run(hip, t, r, g)
    assert not same_bytes(whole, piped), "chunk launches and whole-batch launches agree bit for bit: these frames tell nothing"
    assert np.abs(piped[0].astype(np.float64) - whole[0]).max() <= RGB_TOL
    assert np.abs(piped[1][:, 0:6] - whole[1][:, 0:6]).max() <= STATS_TOL
    return t, r, g, whole, piped


@pytest.mark.parametrize("policy", POLICIES)
def test_out_is_target(hip, big, policy):
    t, r, g, _, _ = big
    with plan(hip, 2, policy):
        want = run(hip, t, r, g)
        tt = t.clone()
        got = run(hip, tt, r, g, out=tt)
    assert same_bytes(want, got)


def test_shifted_overlap_keeps_whole_batch_launches(hip, big):
    """`out` overlapping the reference frames, shifted by a third of a frame: the whole-batch form has read every reference
    before it writes (the result is well defined), chunks would not -- the call must take the whole-batch form"""
    t, r, g, _, _ = big
    n = r.numel()
    shift = r[0].numel() // 3
    flat = torch.empty(n + shift, dtype=torch.float32, device="cuda")
    got = {}
    for chunk in (0, 2):
        flat[shift:].copy_(r.reshape(-1))
        with plan(hip, chunk, "nt"):
            got[chunk] = run(hip, t, flat[shift:].view(r.shape), g, out=flat[:n].view(r.shape))
    assert same_bytes(got[0], got[2])


def test_default_plan_below_thresholds_is_whole_batch(hip, big):
    t, r, g, whole, _ = big
    assert hip.reinhard_pipeline()[0] == -1
    assert hip.reinhard_pipeline_chunk(BIG[0] * BIG[1], BIG_BATCH) == 0
    assert same_bytes(whole, run(hip, t, r, g))
    assert hip.reinhard_pipeline_chunk(1080 * 1920, 1) == 0            # a batch below two chunks
    assert [hip.reinhard_pipeline_chunk(1080 * 1920, b) for b in (6, 8, 12, 16, 32)] == [0, 4, 3, 4, 4]      # the measured plan
    assert hip.reinhard_pipeline_chunk(720 * 1280, 16) == 8 and hip.reinhard_pipeline_chunk(2160 * 3840, 8) == 1


def test_exact_mode_keeps_whole_batch_launches(hip, big):
    t, r, g, _, _ = big
    hip.set_lab_mode("exact")
    try:
        with plan(hip, 0):
            want = run(hip, t, r, g)
        with plan(hip, 2, "plain"):
            got = run(hip, t, r, g)
    finally:
        hip.set_lab_mode("table")
    assert same_bytes(want, got)


def test_armed_profile_events_keep_whole_batch_launches(hip, big):
    t, r, g, whole, _ = big
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for e in ev:
        e.record()
    torch.cuda.synchronize()
    hip.profile_events(ev)
    try:
        with plan(hip, 2, "nt"):
            got = run(hip, t, r, g)
    finally:
        hip.profile_events(None)
    assert same_bytes(whole, got)
    assert ev[0].elapsed_time(ev[1]) > 0 and ev[2].elapsed_time(ev[3]) > 0        # and they timed the two launches


def test_thread_override_and_bad_arguments(hip):
    lib = hip.lib()
    assert lib.ct_set_reinhard_pipeline(-2, 0) != 0 and lib.ct_set_reinhard_pipeline(1, 2) != 0
    before = hip.reinhard_pipeline()
    hip.set_reinhard_pipeline(3, "plain", thread=True)
    try:
        assert hip.reinhard_pipeline() == (3, hip.CT_PIPE_T_PLAIN)
        seen = []
        th = threading.Thread(target=lambda: seen.append(hip.reinhard_pipeline()))
        th.start()
        th.join()
        assert seen == [before]                      # another thread reads the process default
    finally:
        hip.set_reinhard_pipeline(None, thread=True)
    assert hip.reinhard_pipeline() == before


def test_graph_capture(hip):
    shape, batch = (37, 53), 5
    t, r, g = (dev(a) for a in frames(5, batch, shape))
    out = torch.empty_like(t)
    ps = torch.zeros((batch, 2), dtype=torch.float64, device="cuda")
    st = torch.zeros((2 * batch, 8), dtype=torch.float64, device="cuda")
    cap = torch.cuda.Stream()
    with plan(hip, 2, "plain"):
        cap.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(cap):                 # warm-up outside the capture: the library's stream, the capture stream's workspace
            hip.reinhard_psnr(t, r, g, out=out, psnr_out=ps, stats_out=st)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=cap):
            hip.reinhard_psnr(t, r, g, out=out, psnr_out=ps, stats_out=st)
        for k in range(2):
            t2, r2, g2 = (dev(a) for a in frames(50 + k, batch, shape))
            want = run(hip, t2, r2, g2)
            t.copy_(t2); r.copy_(r2); g.copy_(g2)
            out.zero_(); ps.zero_(); st.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert same_bytes(want, (out.cpu().numpy(), st.cpu().numpy(), ps.cpu().numpy()))
        del graph


def test_two_threads_on_two_streams(hip, big):
    """each thread has its own torch stream (and with it its own workspace) and its own library stream beside it"""
    t, r, g, _, piped = big
    sets = [(t, r, g, piped)]
    t2, r2, g2 = (dev(a) for a in frames(78, BIG_BATCH, BIG))
    with plan(hip, 2, "nt"):
        sets.append((t2, r2, g2, run(hip, t2, r2, g2)))
        errors = []

        def worker(k):
            try:
                a, b, c, want = sets[k]
                with torch.cuda.stream(torch.cuda.Stream()):
                    for _ in range(10):
                        B = a.shape[0]
                        st = torch.zeros((2 * B, 8), dtype=torch.float64, device="cuda")
                        o, ps = hip.reinhard_psnr(a, b, c, stats_out=st)
                        torch.cuda.current_stream().synchronize()
                        if not same_bytes(want, (o.cpu().numpy(), st.cpu().numpy(), ps.cpu().numpy())):
                            errors.append((k, "differs from the serial result"))
                            break
            except Exception as e:                   # noqa: BLE001
                errors.append((k, repr(e)))

        torch.cuda.synchronize()
        ts = [threading.Thread(target=worker, args=(k,)) for k in (0, 1)]
        for th in ts:
            th.start()
        for th in ts:
            th.join()
    assert not errors, errors


def test_back_to_back_calls_share_one_workspace(hip, big):
    """two calls in a row on one caller stream use the same workspace: the second call's chunks must wait for the first call's
    PSNR finish, which the join into the caller's stream orders"""
    t, r, g, _, piped = big
    t2, r2, g2 = (dev(a) for a in frames(79, BIG_BATCH, BIG))
    B = BIG_BATCH
    with plan(hip, 2, "nt"):
        want2 = run(hip, t2, r2, g2)
        st1, st2 = (torch.zeros((2 * B, 8), dtype=torch.float64, device="cuda") for _ in range(2))
        o1, p1 = hip.reinhard_psnr(t, r, g, stats_out=st1)
        o2, p2 = hip.reinhard_psnr(t2, r2, g2, stats_out=st2)
        torch.cuda.synchronize()
    assert same_bytes(piped, (o1.cpu().numpy(), st1.cpu().numpy(), p1.cpu().numpy()))
    assert same_bytes(want2, (o2.cpu().numpy(), st2.cpu().numpy(), p2.cpu().numpy()))
