"""Every kernel variant that libct_hip.so selects from an environment switch at start-up, held to the oracles of the default form.

A switch is read once per process (a function-local static behind ct::env_int / ct::env_str, csrc/ct_env.h), so this process
cannot toggle it: each GROUP below runs existing checks -- unchanged, with their own float64 / bitwise gates -- in ONE child
interpreter with the group's switches set, the way test_local_corr_per_pixel_kernels does for CT_HIP_LCF_TILE.  The child also
gets CT_HIP_ENV_TRACE=1: every consult of a switch writes `ct_hip env NAME=<text> -> <value>` to stderr, and the parent asserts
that line for every switch of the group, so a misspelt name or a node list that never reaches the launcher that owns the
switch fails instead of passing vacuously.  (The child runs with --capture=no: pytest's capture would otherwise keep the stderr
of passing tests to itself.)

The nodes of this module whose names start with test_child_ only mean something inside such a child and skip elsewhere.
tests/test_kernel_variants_host.py keeps the table complete: a switch in csrc/ that no group sets fails there."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import linear as olin     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RGB_TOL = 6.0e-6        # tests/test_reinhard_persist_gpu.py / tests/test_linear_gpu.py: float32 output of the table arithmetic

GM = "tests/test_gmflow_kernels_gpu.py::"
WS = "tests/test_conv_ws_gpu.py::"
LIN = "tests/test_linear_gpu.py::"
MET = "tests/test_metrics.py::"
PRED = "tests/test_predict_gpu.py::"
VIEWS = "tests/test_views_gpu.py::"
RES = "tests/test_resize_gpu.py::"
IDT = "tests/test_idt_gpu.py::"
RG = "tests/test_regrain.py::"
RP = "tests/test_reinhard_persist_gpu.py::"
EDGE = "tests/test_pam_edges_gpu.py::"
ME = "tests/test_kernel_variants_gpu.py::"

# test_gconv's geometries that csrc/conv_direct.hip takes: cout <= 4 (cfg10, cfg17 - cfg19) and the 7x7 kernels on <= 3 channels
# (cfg0, cfg7, cfg20, cfg21); ct_gconv2d_f32 reaches it in the split and in the exact convolution mode alike
DIRECT_CFGS = (0, 7, 10, 17, 18, 19, 20, 21)
PERSIST_SMALL = [RP + "test_small_and_ragged_sizes[%d]" % n for n in (256, 257, 511, 1000, 70001, 90300)]

GROUPS = {
    # the three-piece bf16 attention kernels (attention_tokens_kernel<128,128|2,mapped>, <64,96>, <64,0>, attention_colsum_kernel<64>,
    # the mixed fallback of ct_attention_rows64_disp_f32), small-cout / 7x7 convolutions on the generic and tile kernels, the bf16
    # convolutions of 33..64 input channels on the tile kernel instead of conv_ws
    "fallback-kernels": (
        {"CT_HIP_ATT16": "0", "CT_HIP_CONV_DIRECT": "0", "CT_HIP_CONV_WS": "0"},
        [GM + "test_attention_tokens[2-160-128-False]", GM + "test_attention_tokens[3-448-128-True]", GM + "test_attention_tokens[2-700-2-False]"]
        + [GM + "test_attention_rowmap_is_window_partition[%s]" % p for p in ("128-False", "128-True", "2-True")]
        + [GM + "test_attention_tiny_sequences[%d]" % l for l in (1, 7, 28, 33, 65)]
        + [GM + "test_attention_kv_shift_is_the_swapped_concat", GM + "test_attention_tokens_wide_dynamic_range[128]",
           GM + "test_attention_tokens_wide_dynamic_range[2]", GM + "test_attention_rows64_wide_dynamic_range"]
        + [GM + "test_gconv[%s-cfg%d]" % (m, c) for m in ("split", "exact") for c in DIRECT_CFGS]
        + [GM + "test_small_cout_conv_zero_padding_is_a_select[cfg%d]" % c for c in range(3)]
        + ["tests/test_disparity_gpu.py::test_pam_streaming_disp_ini[4-512]", "tests/test_dcmcs3di_gpu.py::test_pam_streaming_vs_torch_reference[3-70]"]
        + [WS + "test_conv_ws_vs_float64[cfg%d-False]" % c for c in range(6)]
        + [WS + "test_conv_ws_writes_only_its_output[cfg%d]" % c for c in range(3)]
        # the streaming family on peaked inputs (tests/pam_edges_common.py), same bounds: lengths at the tile / workgroup edges, every
        # grid of the workgroup-order test, NaN locality
        + [EDGE + "test_streaming_lengths[%s-%d]" % (c, l) for c in ("flat", "mid", "peaked", "twin", "ramp-up", "ramp-down") for l in (33, 128, 129)]
        + [EDGE + "test_streaming_grid_order[%d-%d]" % g for g in ((129, 4), (33, 9), (33, 17), (385, 6), (257, 11))]
        + [EDGE + "test_streaming_nan_stays_where_the_reference_puts_it[%s]" % w for w in ("query", "key", "value")]),
    # every launch-geometry cap at its floor: grid-stride loops take several trips on 17x31 .. 273x481 frames, seven persistent
    # workgroups hold more tiles than fit their LDS (300x301: 51 slots), conv_ws cuts its 5..50-row images into 3-row segments
    "small-grids": (
        {"CT_HIP_TARGET_BLOCKS": "1", "CT_HIP_LUT_BLOCKS": "1", "CT_IDT_MINMAX_BLOCKS": "1", "CT_IDT_APPLY_BLOCKS": "1",
         "CT_IDT_HIST_BLOCKS": "1", "CT_HIP_REGRAIN_K": "1", "CT_HIP_WS_SEG": "3", "CT_HIP_PERSIST_WGS": "7"},
        [LIN + "test_ragged_sizes_vs_oracle[%s-%s-shape%d]" % (m, d, s) for m in ("table", "exact") for d in ("float32", "float64") for s in (6, 7)]
        + [LIN + "test_lab_gate_all_branches_vs_oracle[%s-size1]" % m for m in ("table", "exact")]
        + [LIN + "test_batched_misaligned_images[%s]" % m for m in ("table", "exact")]
        + [LIN + "test_u8_256_vs_reference[%s]" % m for m in ("table", "exact")]
        + [MET + "test_fused_reinhard_psnr[table]", MET + "test_fused_reinhard_psnr[exact]", MET + "test_hip_ssim_vs_oracle[shape2]",
           MET + "test_hip_icid_vs_oracle[shape0]"]
        + [PRED + "test_pack_random_frames_bitwise[3-270-480]", PRED + "test_pack_tie_set_bitwise[64-96-4099]",
           PRED + "test_pack_misaligned_bases_take_the_fallback"]
        + [VIEWS + "test_chess_mix_bitwise[shape1-7]"] + [VIEWS + "test_rgbmse_and_gray_bitwise[shape%d]" % s for s in range(3)]
        + [RES + "test_small_and_odd_shapes_every_pixel[False]", RES + "test_small_and_odd_shapes_every_pixel[True]",
           RES + "test_case_b_inexact_coordinates_down_and_back_up[273-481-0.6]"]
        + [IDT + "test_idt_u8_256_vs_reference"]
        + [IDT + "test_idt_small_bitwise_and_vs_reference[%s]" % c for c in ("f64-255-4", "f32-255-4", "odd-64-2")]
        + [IDT + "test_idt_batch_of_pairs", IDT + "test_idt_ragged_sizes_bitwise[shape4]"]
        + [RG + "test_hip_regrain_vs_reference_run"] + [RG + "test_hip_regrain_vs_oracle_sizes[shape%d]" % s for s in (1, 2, 3)]
        # fp16 conv_ws itself (the module's autouse fixture keeps the Winograd form off): CT_HIP_WS_SEG's trace line proves it
        + [WS + "test_conv_ws_vs_float64[cfg%d-True]" % c for c in range(6)]
        + PERSIST_SMALL
        + [RP + "test_all_branches_vs_oracle[size1]", RP + "test_nan_inf_huge_and_constant_frames", RP + "test_more_pairs_than_one_launch_holds",
           ME + "test_child_seven_workgroups_refuse_1080p"]),
    # the 8-wave float32 instantiations of reinhard_persist_kernel, and the fused float32 entries routed into the persistent launch
    "persist-forms": (
        {"CT_HIP_PERSIST_WAVES": "8", "CT_HIP_REINHARD_PERSIST": "1"},
        [ME + "test_child_1080p_fused_entries_take_persist"]          # = test_1080p_vs_oracle_every_pixel_and_two_sweep, branch asserted live
        + PERSIST_SMALL
        + [RP + "test_all_branches_vs_oracle[size0]", RP + "test_all_branches_vs_oracle[size1]", RP + "test_nan_inf_huge_and_constant_frames",
           RP + "test_u8_front_door", RP + "test_graph_capture_and_replay", RP + "test_output_must_not_overlap_an_input",
           MET + "test_fused_reinhard_psnr[table]", MET + "test_fused_reinhard_psnr[exact]",
           ME + "test_child_fused_entries_allow_out_equal_target"]),
}

FAULT_CODES = (134, 139, 124, 137)
_child_faulted = False


@pytest.mark.parametrize("group", list(GROUPS))
def test_kernel_variants(group):
    global _child_faulted
    switches, ids = GROUPS[group]
    if _child_faulted:
        pytest.skip("an earlier variant child faulted; not starting more GPU work")
    already = [k for k in switches if k in os.environ]
    if already:
        pytest.skip("%s already set in this process: it is the child of this test, or a run with a preset of its own" % ", ".join(already))
    cmd = [sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "--capture=no"] + ids
    t0 = time.perf_counter()
    try:
        p = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, CT_HIP_ENV_TRACE="1", **switches), capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired as e:
        _child_faulted = True
        tail = lambda b: (b.decode(errors="replace") if isinstance(b, bytes) else (b or ""))[-3000:]
        pytest.fail("variant child %s hung (300 s); not starting more GPU work\n%s\n%s" % (group, tail(e.stdout), tail(e.stderr)))
    tails = "\n---- stdout ----\n%s\n---- stderr ----\n%s" % (p.stdout[-6000:], p.stderr[-3000:])
    if p.returncode < 0 or p.returncode in FAULT_CODES:
        _child_faulted = True
        pytest.fail("variant child %s ended with return code %d (fault / abort / time limit); not starting more GPU work%s"
                    % (group, p.returncode, tails))
    assert p.returncode == 0 and "%d passed" % len(ids) in p.stdout, "return code %d%s" % (p.returncode, tails)
    assert "skipped" not in p.stdout.splitlines()[-1] and "deselected" not in p.stdout.splitlines()[-1], tails
    for name, value in switches.items():
        assert "ct_hip env %s=%s ->" % (name, value) in p.stderr, "no node of %s consulted %s%s" % (group, name, tails)
    print("variant child %s: %.1f s wall; %s" % (group, time.perf_counter() - t0, p.stdout.splitlines()[-1]))


# ---- nodes that run inside a child only ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip():
    import ct_hip
    ct_hip.lib()
    ct_hip.set_lab_mode("table")
    return ct_hip


def _child_of(group):
    switches = GROUPS[group][0]
    if any(os.environ.get(k) != v for k, v in switches.items()):
        pytest.skip("runs in the %s child of test_kernel_variants only" % group)


def test_child_seven_workgroups_refuse_1080p(hip):
    """small-grids: with 7 workgroups a 1080p frame needs 1158 tiles per workgroup, more than the raw-tile masks hold -- the persistent
    launch must say so, and reinhard() must still run its two sweeps (here with every grid cap at its floor) and match the oracle"""
    _child_of("small-grids")
    assert hip.reinhard_persist_supported(300 * 301)
    assert not hip.reinhard_persist_supported(1920 * 1080)
    assert not hip.reinhard_takes_persist(1920 * 1080)
    rng = np.random.default_rng(17)
    t = rng.random((1080, 1920, 3), dtype=np.float32)
    r = (rng.random((1080, 1920, 3), dtype=np.float32) * 0.6 + 0.2).astype(np.float32)
    out = hip.reinhard(torch.from_numpy(t).cuda(), torch.from_numpy(r).cuda()).cpu().numpy()
    assert np.abs(out - olin.color_transfer_between_images(t, r)).max() <= RGB_TOL


def test_child_1080p_fused_entries_take_persist(hip):
    """persist-forms: test_1080p_vs_oracle_every_pixel_and_two_sweep with its `if hip.reinhard_takes_persist(...)` branch live (the fused
    entries bitwise equal to the explicit persistent entry), on the 8-wave instantiation"""
    _child_of("persist-forms")
    from tests.test_reinhard_persist_gpu import test_1080p_vs_oracle_every_pixel_and_two_sweep as body
    assert hip.reinhard_takes_persist(1080 * 1920)
    body(hip)


def test_child_fused_entries_allow_out_equal_target(hip):
    """persist-forms: include/ct_hip.h promises that ct_reinhard_f32 / ct_reinhard_psnr_f32 allow out == target.  Routed into the
    persistent launch (which re-reads its input after storing and so refuses an overlapping output) they returned CT_E_BADARG;
    such a call now runs the two sweeps as the separate entries do (csrc/linear.hip: reinhard_separate_sweeps = ct_lab_stats_f32 on
    targets and references + ct_reinhard_apply_f32), hence bit for bit two_sweep().  The explicit persistent entry still refuses."""
    _child_of("persist-forms")
    from tests.test_reinhard_persist_gpu import two_sweep
    rng = np.random.default_rng(41)
    t, r, g = (torch.from_numpy(rng.random((1, 1080, 1920, 3), dtype=np.float32)).cuda() for _ in range(3))
    assert hip.reinhard_takes_persist(1080 * 1920)
    want = two_sweep(hip, t, r)[0]
    buf = t.clone()
    out = hip.reinhard(buf, r, out=buf)
    assert out.data_ptr() == buf.data_ptr() and torch.equal(out, want)
    buf = t.clone()
    out, ps = hip.reinhard_psnr(buf, r, g, out=buf)
    assert out.data_ptr() == buf.data_ptr() and torch.equal(out, want)
    assert torch.allclose(ps, hip.frame_psnr(want, g), rtol=1e-6, atol=0)       # tests/test_metrics.py::test_fused_reinhard_psnr's gate
    with pytest.raises(hip.CtHipError):
        hip.reinhard_persist(t, r, out=t)
