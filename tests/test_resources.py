"""The handle's owning buffer types (eicos_amd/csrc/resources.hpp), checked without a GPU through a stand-alone program built with the
address and undefined-behaviour sanitizers."""
import os
import subprocess

from conftest import ROOT


def test_buffer_and_pinned_slot_under_sanitizers(tmp_path):
    """tests/host/resources_check.cpp: the grow rule (no call when large enough; synchronise, free, allocate in that order when not; empty
    after a failed allocation), moves, reset and destruction of Buffer, and the wait / mark / reserve protocol of PinnedSlot, over policies
    that log every call.  Its own process; nothing is loaded into this one."""
    exe = str(tmp_path / "resources_check")
    # (the sanitizer runtimes linked statically: the program then also starts where the environment preloads a library into every process)
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "eicos_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "resources_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
