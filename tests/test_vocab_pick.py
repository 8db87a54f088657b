"""The choice of the vocabulary projection's kernel (csrc/wh_vocab_pick.h: vocab_kernel), on the
CPU: tools/vocab_pick_host_check.cpp holds the table of shapes at every boundary of the choice
(8 / 9, 16 / 17 in fp32, 32 / 33 and 112 / 113 rows, K = 1280 against the other widths, the
LayerNorm prologue, the 8-bit step) with the kernel each must get, written out by hand.  The
launchers and wh_step_kernels' `vocab=` field call the same function, so the kernel a GPU test
reads from step_kernels is the kernel that ran."""
import os
import subprocess

from conftest import PKG_ROOT


def test_vocab_kernel_table(tmp_path):
    """g++ is what the package Makefile compiles its host sources with."""
    exe = str(tmp_path / "vocab_pick_host_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(PKG_ROOT, "csrc"),
                    os.path.join(PKG_ROOT, "tools", "vocab_pick_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("vocab_pick_host_check: ok")
