#!/usr/bin/env python3
"""Compare the gfx950 device code of two `make asm` output directories, function by function.

usage: tools/asm_diff.py OLD_DIR NEW_DIR        (e.g. two copies of color-transfer_amd/csrc/build_asm)

Every *-hip-amdgcn-amd-amdhsa-gfx950.s of a directory is cut into functions (`NAME: ; @NAME` up to `.Lfunc_end`) and kernel
descriptors (`.amdhsa_kernel NAME` .. `.end_amdhsa_kernel`), keyed by mangled name whatever file they stand in -- a kernel
that moved to another source compares against itself.  `;` comments and trailing blanks are dropped and the function index
of `.LBB<n>_` labels is normalised; nothing else is: one changed instruction, register or descriptor field is a difference.
A name defined in several files (a static helper kernel per translation unit) compares as the set of its distinct copies.
Only code and descriptors are compared: device data outside functions (.rodata constant tables, the .amdgpu_metadata kernel-argument
layout) is not seen, so "0 differ" is not a proof that whole code objects are identical.
Prints the names that differ, are missing or are new; exit status 1 if there are any."""
import glob, os, re, sys

SUFFIX = "-hip-amdgcn-amd-amdhsa-gfx950.s"
HEAD = re.compile(r"^([A-Za-z_$][\w$.]*):\s*; @\1\s*$")
LBB = re.compile(r"\.LBB\d+_")


def clean(line):
    return LBB.sub(".LBB_", line.split(";", 1)[0]).rstrip()


def functions(text):
    """{name: [body, ..]}: function bodies under NAME, kernel descriptors under "NAME (descriptor)"."""
    out = {}
    name, body, desc = None, [], None
    for raw in text.split("\n"):
        m = HEAD.match(raw)
        if m:
            name, body = m.group(1), []
            continue
        line = clean(raw)
        s = line.strip()
        if s.startswith(".amdhsa_kernel "):
            desc = (s.split()[1], [])
        if desc is not None:
            desc[1].append(s)
            if s == ".end_amdhsa_kernel":
                out.setdefault(desc[0] + " (descriptor)", []).append("\n".join(desc[1]))
                desc = None
            continue
        if name is None:
            continue
        if s.startswith(".Lfunc_end"):
            out.setdefault(name, []).append("\n".join(body))
            name = None
        elif s:
            body.append(line)
    return out


def load(directory):
    files = sorted(glob.glob(os.path.join(directory, "*" + SUFFIX)))
    if not files:
        sys.exit("asm_diff: no *%s in %s" % (SUFFIX, directory))
    out = {}
    for f in files:
        with open(f) as fh:
            for k, v in functions(fh.read()).items():
                out.setdefault(k, []).extend(v)
    return {k: sorted(set(v)) for k, v in out.items()}


def compare(old, new):
    """(differ, missing, new): sorted name lists"""
    differ = sorted(k for k in old if k in new and old[k] != new[k])
    return differ, sorted(k for k in old if k not in new), sorted(k for k in new if k not in old)


def main(argv):
    if len(argv) != 3:
        sys.exit(__doc__)
    old, new = load(argv[1]), load(argv[2])
    differ, missing, added = compare(old, new)
    for label, names in (("differs", differ), ("missing", missing), ("new", added)):
        for n in names:
            print("%-8s %s" % (label, n))
    print("%d functions and descriptors compared: %d differ, %d missing, %d new" % (len(old), len(differ), len(missing), len(added)))
    return 1 if (differ or missing or added) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
