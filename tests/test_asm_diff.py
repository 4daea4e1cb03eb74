"""tools/asm_diff.py on small hand-written assembly texts (no GPU): comment padding, the function index of block labels and the
file a kernel stands in do not count; one changed instruction, one changed descriptor field, a missing or a new kernel do."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "asm_diff.py")
SUFFIX = "-hip-amdgcn-amd-amdhsa-gfx950.s"

KERNEL = """\t.text
\t.globl\t{name}
\t.p2align\t8
\t.type\t{name},@function
{name}:{pad}; @{name}
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\ts_waitcnt lgkmcnt(0){pad}; wait for the pointer
\tv_cmp_gt_u32_e32 vcc, s0, v0
\ts_and_saveexec_b64 s[2:3], vcc
\ts_cbranch_execz .LBB{idx}_2
; %bb.1:{pad}; %then
\t{insn}
.LBB{idx}_2:{pad}; %exit
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel {name}
\t\t.amdhsa_group_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr {vgprs}
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{idx}:
\t.size\t{name}, .Lfunc_end{idx}-{name}
{pad}; -- End function
"""


def kernel(name, idx, pad=" ", insn="v_mov_b32_e32 v1, 0", vgprs=2):
    return KERNEL.format(name=name, idx=idx, pad=pad, insn=insn, vgprs=vgprs)


def run(tmp_path, old_files, new_files):
    for side, files in (("old", old_files), ("new", new_files)):
        os.makedirs(str(tmp_path / side))
        for stem, text in files.items():
            with open(str(tmp_path / side / (stem + SUFFIX)), "w") as fh:
                fh.write(text)
    done = subprocess.run([sys.executable, TOOL, str(tmp_path / "old"), str(tmp_path / "new")], capture_output=True, text=True, timeout=60)
    assert done.stderr == ""
    return done.returncode, done.stdout


def test_equal_modulo_comments_label_index_and_file(tmp_path):
    old = {"both": kernel("_Z1av", 0) + kernel("_Z1bv", 1)}
    new = {"first": kernel("_Z1bv", 0, pad="      \t   "), "second": kernel("_Z1av", 3, pad="\t\t")}      # split in two, other order
    rc, out = run(tmp_path, old, new)
    assert rc == 0, out
    assert "4 functions and descriptors compared: 0 differ, 0 missing, 0 new" in out


def test_one_changed_instruction_fails(tmp_path):
    old = {"k": kernel("_Z1av", 0) + kernel("_Z1bv", 1)}
    new = {"k": kernel("_Z1av", 0) + kernel("_Z1bv", 1, insn="v_mov_b32_e32 v1, 1")}
    rc, out = run(tmp_path, old, new)
    assert rc == 1
    assert "differs  _Z1bv\n" in out and "_Z1av" not in out
    assert "1 differ, 0 missing, 0 new" in out


def test_changed_descriptor_missing_and_new_kernels_fail(tmp_path):
    old = {"k": kernel("_Z1av", 0) + kernel("_Z1bv", 1)}
    new = {"k": kernel("_Z1av", 0, vgprs=3) + kernel("_Z1cv", 1)}
    rc, out = run(tmp_path, old, new)
    assert rc == 1
    assert "differs  _Z1av (descriptor)\n" in out and "missing  _Z1bv\n" in out and "new      _Z1cv\n" in out
    assert "1 differ, 2 missing, 2 new" in out
