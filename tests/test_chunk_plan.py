"""The description of chunked transfers (eicos_amd/csrc/chunk_plan.hpp: the packed layout of a chunk under its two padding rules, the
sizes of the staging areas, the chunk-size rules), checked without a GPU through a stand-alone program built with the address and
undefined-behaviour sanitizers."""
import os
import subprocess

from conftest import ROOT


def test_chunk_plan_under_sanitizers(tmp_path):
    """tests/host/chunk_plan_check.cpp: every subset of the five arrays over five sets of widths (zeros among them) and row counts for
    which rows * w is and is not a multiple of 8, under both padding rules -- every array inside the total, in order, overlapping no
    other, the offsets and totals those of the walks the call sites held, the totals inside the areas as they are reserved; layouts,
    area sizes and every chunk-size rule against numbers laid out by hand: counts 0, 1, 15, 16, 17 and around one and two chunks,
    the even split on both sides of its interval, rows wide enough for the floor and narrow enough for the count to decide.  Its own
    process; nothing is loaded into this one.  The header compiles without a HIP include path."""
    exe = str(tmp_path / "chunk_plan_check")
    # (the sanitizer runtimes linked statically: the program then also starts where the environment preloads a library into every process)
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "eicos_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "chunk_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
