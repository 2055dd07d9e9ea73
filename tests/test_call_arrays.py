"""The arrays of a sensitivity or rollout call (eicos_amd/csrc/call_arrays.hpp), checked without a GPU through a stand-alone program built
with the address and undefined-behaviour sanitizers."""
import os
import subprocess

from conftest import ROOT


def test_call_arrays_under_sanitizers(tmp_path):
    """tests/host/call_arrays_check.cpp: placement (64-byte boundaries, no overlap, every part written whole inside a block of exactly
    bytes()), absent and zero-width arrays, the device form, the copies of the host form and the kind fault, over the declarations of
    the real calls and a policy that logs every copy.  Its own process; nothing is loaded into this one.  The header compiles without a
    HIP include path."""
    exe = str(tmp_path / "call_arrays_check")
    # (the sanitizer runtimes linked statically: the program then also starts where the environment preloads a library into every process)
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "eicos_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "call_arrays_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
