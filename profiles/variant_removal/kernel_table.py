#!/usr/bin/env python3
"""Per-kernel resource table of a source tree, from the code objects' symbol and note tables.

    kernel_table.py <package dir with csrc/ and ../include> <out.tsv>
    kernel_table.py --compare parent.tsv new.tsv rename_map.tsv > mismatches.txt

Each csrc/*.hip is compiled device-only for gfx950 with the Makefile's optimisation flags,
unbundled, and read with llvm-readobj: the FUNC symbol's size, and from the AMDGPU metadata
note .vgpr_count, .sgpr_count, .group_segment_fixed_size, .private_segment_fixed_size.  No
instruction text is read.  Rows: file, demangled kernel name without its argument list, the
five numbers.

--compare matches every kernel of the new table to the parent's by name, through
rename_map.tsv (regular expression on the new name <TAB> replacement giving the parent
name) where a template parameter list shrank, and prints kernels without a counterpart and
kernels whose numbers differ.  Exit status 1 if a new kernel has no parent counterpart or
any number grew.
"""
import glob
import os
import re
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
FIELDS = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def kernel_name(demangled):
    """`void wh::k<A, B>(args)` -> `wh::k<A, B>`: the argument list starts at the first `(` outside the `<>`."""
    depth = 0
    for i, c in enumerate(demangled):
        depth += (c == "<") - (c == ">")
        if c == "(" and depth == 0:
            demangled = demangled[:i]
            break
    return demangled[5:] if demangled.startswith("void ") else demangled


def table(pkg):
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for src in sorted(glob.glob(os.path.join(pkg, "csrc", "*.hip"))):
            base = os.path.basename(src)
            obj, elf = os.path.join(tmp, base + ".o"), os.path.join(tmp, base + ".elf")
            run(os.path.join(ROCM, "bin", "hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                "-I" + os.path.join(pkg, "..", "include"), "-I" + os.path.join(pkg, "csrc"), "--offload-device-only",
                "-c", src, "-o", obj)
            run(os.path.join(ROCM, "llvm", "bin", "clang-offload-bundler"), "--unbundle", "--type=o",
                "--targets=hip-amdgcn-amd-amdhsa--gfx950", "--input=" + obj, "--output=" + elf)
            readobj = os.path.join(ROCM, "llvm", "bin", "llvm-readobj")
            size, plain = {}, {}  # by mangled name; the demangled names from a second listing, row by row
            syms = run(readobj, "--elf-output-style=GNU", "--symbols", elf).splitlines()
            for line, dline in zip(syms, run(readobj, "--elf-output-style=GNU", "--symbols", "--demangle", elf).splitlines()):
                f = line.split()
                if len(f) == 8 and f[3] == "FUNC":
                    size[f[7]] = int(f[2])
                    plain[f[7]] = dline.split(None, 7)[7]
            kernels, cur = [], None
            for line in run(readobj, "--notes", elf).splitlines():
                if re.match(r"\s+- \.\w+:", line):  # first key of a list item: a kernel, or one of its args
                    if line.startswith("  - "):
                        cur = {}
                        kernels.append(cur)
                    line = line.replace("- ", "  ", 1)
                m = re.match(r"    (\.\w+):\s+(\S+)$", line)
                if m and cur is not None:
                    cur[m.group(1)] = m.group(2).strip("'\"")
            for k in kernels:
                sym = k[".symbol"][:-3]  # without ".kd"
                rows.append([base, kernel_name(plain[sym]), str(size[sym])] + [k[f] for f in FIELDS])
    return rows


def load(path):
    out = {}
    for line in open(path):
        f = line.rstrip("\n").split("\t")
        out[(f[0], f[1])] = [int(v) for v in f[2:]]
    return out


def compare(parent, new, renames):
    old, cur = load(parent), load(new)
    rules = [line.rstrip("\n").split("\t") for line in open(renames) if line.strip() and not line.startswith("#")]
    bad = False
    cols = ("code_bytes",) + FIELDS
    n_same = 0
    for (f, name), vals in sorted(cur.items()):
        was = name
        for pat, repl in rules:
            if re.fullmatch(pat, name):
                was = re.sub(pat, repl, name)
                break
        if (f, was) not in old:
            print(f"NO PARENT\t{f}\t{name}\t(looked for {was})")
            bad = True
            continue
        diff = [(c, a, b) for c, a, b in zip(cols, old[(f, was)], vals) if a != b]
        if not diff:
            n_same += 1
            continue
        grew = any(b > a for _, a, b in diff)
        bad |= grew
        print(("GREW" if grew else "SMALLER") + f"\t{f}\t{name}\t" + ", ".join(f"{c} {a} -> {b}" for c, a, b in diff))
    print(f"# {len(cur)} kernels in the new table, {n_same} identical to their parent instantiation, "
          f"{len(old)} kernels in the parent table")
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(*sys.argv[2:5]))
    with open(sys.argv[2], "w") as out:
        for r in table(sys.argv[1]):
            out.write("\t".join(r) + "\n")
