"""The rule "may this step run inside the solve launch" (eicos_amd/csrc/fused_fit.hpp), checked without a GPU through a stand-alone
program built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

from conftest import ROOT


def test_fused_fit_rule_under_sanitizers(tmp_path):
    """tests/host/fused_fit_check.cpp: every boundary of the accumulator limit, the LDS-vector count and the theta row, for the four step
    kinds and the updateData kernels, against the three expressions the rule replaced.  Its own process; nothing is loaded into this one."""
    exe = str(tmp_path / "fused_fit_check")
    # (the sanitizer runtimes linked statically: the program then also starts where the environment preloads a library into every process)
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "eicos_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "fused_fit_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
