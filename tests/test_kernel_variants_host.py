"""The table of start-up switches stays complete (no GPU): every environment switch that csrc/ reads is either set by a group of
tests/test_kernel_variants_gpu.py -- whose child process then holds the kernels behind it to the oracles -- or listed here with
the reason why another test covers it.  A switch added later cannot ship unnoticed with nothing running its variant."""
import ast
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "color-transfer_amd", "csrc")

COVERED_ELSEWHERE = {
    "CT_HIP_LAB": "preset of ct_set_lab_mode's state: the `mode` fixtures of test_linear_gpu / test_metrics drive both values",
    "CT_HIP_WINO_FORM": "preset of ct_set_conv_wino_form's state: the `wino_form` fixture of test_conv_ws_gpu drives both values",
    "CT_HIP_SPLIT_SK": "the kernel path of set_conv_stream_k(False), which test_conv_split_stream_k compares with the shared form",
    "CT_HIP_SPLIT_WGS": "its minimum is a full grid of 256 workgroups: no effect on a small shape",
    "CT_HIP_LCF_TILE": "test_gmflow_kernels_gpu.py::test_local_corr_per_pixel_kernels (a child process of its own)",
    "CT_HIP_ENV_TRACE": "the trace itself: every case of test_kernel_variants asserts its lines",
}


def _groups():
    """GROUPS of tests/test_kernel_variants_gpu.py, read from its source (importing that module needs torch)"""
    src = open(os.path.join(ROOT, "tests", "test_kernel_variants_gpu.py")).read()
    for node in ast.parse(src).body:
        if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "GROUPS" for t in node.targets):
            return {ast.literal_eval(k): ast.literal_eval(v.elts[0]) for k, v in zip(node.value.keys, node.value.values)}
    raise AssertionError("GROUPS not found")


def _sources():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert len(files) > 30
    return [(os.path.basename(f), open(f).read()) for f in files]


def test_every_switch_is_tested_or_accounted_for():
    names = {}
    for fname, src in _sources():
        for m in re.finditer(r'\b(?:env_int|env_str|getenv)\(\s*"([^"]+)"', src):
            names.setdefault(m.group(1), fname)
    assert len(names) >= 19, names                      # the scan itself works
    grouped = {}
    for group, switches in _groups().items():
        for k in switches:
            assert k not in grouped, "%s is set by two groups: a failing node would not name the culprit" % k
            grouped[k] = group
    for name, fname in sorted(names.items()):
        assert (name in grouped) != (name in COVERED_ELSEWHERE), \
            "%s (csrc/%s) must be a switch of exactly one group of test_kernel_variants or an entry of COVERED_ELSEWHERE" % (name, fname)
    stale = (set(grouped) | set(COVERED_ELSEWHERE)) - set(names)
    assert not stale, "not read by csrc/ any more: %s" % sorted(stale)


def test_switches_are_read_through_the_helper_only():
    """getenv appears in ct::env_trace / env_int / env_str (csrc/ct_env.h, part of ct_common.h) and nowhere else, and never with a computed name
    outside the helpers: the scan above sees every switch"""
    for fname, src in _sources():
        code = re.sub(r"//[^\n]*", "", src)
        n = len(re.findall(r"\bgetenv\s*\(", code))
        assert n == (3 if fname == "ct_env.h" else 0), "%d raw getenv( in csrc/%s" % (n, fname)
        for m in re.finditer(r"\benv_(?:int|str)\(\s*([^,)]*)", code):
            arg = m.group(1).strip()
            assert arg.startswith('"') or (fname == "ct_env.h" and arg == "const char *name"), "csrc/%s: env switch named by %r" % (fname, arg)


def test_fp16_and_wave_primitives_have_one_copy():
    """The fp16 two-piece primitives live in csrc/ct_split16.h and the DPP wave maximum in csrc/ct_wave.h, once: a kernel file
    that grows a private copy again (a fix to one would not reach the others) fails here.  The three-MFMA product is written out
    only where its MFMAs are interleaved with other work by hand."""
    code = {fname: re.sub(r"//[^\n]*", "", src) for fname, src in _sources()}

    def holders(text):
        return sorted(fname for fname, c in code.items() if text in c)

    assert holders("v_cvt_pk_f16_f32") == ["ct_split16.h"]
    assert holders("CT_DPP_MAX") == ["ct_wave.h"]
    assert holders("__builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh") == ["conv_split.hip", "conv_ws.hip", "ct_split16.h"]
