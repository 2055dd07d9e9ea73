"""The layout of a rollout's device buffers and the trajectory a handle holds of it (eicos_amd/csrc/rollout_layout.hpp), checked without
a GPU through a stand-alone program built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

from conftest import ROOT


def test_rollout_layout_under_sanitizers(tmp_path):
    """tests/host/rollout_layout_check.cpp: for the three buffers of a rollout over the smallest shape and over B = 3, T = 2, k = 3,
    r = 2 on a pattern with n = 5, m = 4 and p = 0 or 2 (w given, recording off and on, fused and not) every part inside its buffer,
    aligned, overlapping no other and written whole inside a block of exactly the total; the totals against the hand-laid sums; the
    six record widths and where row t of instance b lies; the one step's rows exactly where the rollout records and is not fused; the
    refusal of batch * steps beyond an int; the three messages of the held trajectory.  Its own process; nothing is loaded into
    this one.  The header compiles without a HIP include path."""
    exe = str(tmp_path / "rollout_layout_check")
    # (the sanitizer runtimes linked statically: the program then also starts where the environment preloads a library into every process)
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "eicos_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "rollout_layout_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
