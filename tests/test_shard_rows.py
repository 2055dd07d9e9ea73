"""The row routing of the multi-GPU layer (eicos_amd/csrc/shard_rows.hpp: the shard layout, the split of a list of global ids, the
columns of a list-indexed call and the routine that serves one shard's share), run without a GPU through a stand-alone program built
with the address and undefined-behaviour sanitizers: tests/host/shard_rows_check.cpp.  It compiles the header multi.cpp includes, plays
the shard with a callable and compares every output with a plain loop over the caller's list.  The program is built once and runs in
its own process per case; nothing sanitized is loaded into this one."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "eicos_amd", "csrc")


@pytest.fixture(scope="module")
def shard_rows_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("shard_rows") / "shard_rows_check")
    # (the sanitizer runtimes linked statically: the program then also starts where the environment preloads a library into every process)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-Wall", "-Wno-unused-parameter",
                           "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "shard_rows_check.cpp"), "-o", exe])
    return exe


def _run(exe, mode):
    out = subprocess.run([exe, mode], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr
    assert ", 0 failures" in out.stdout and "FAIL" not in out.stdout, out.stdout
    return out.stdout


def test_shard_layout(shard_rows_check):
    """Batch 5 over 2 shards: (0, 3), (3, 2); 7 over 3: (0, 3), (3, 2), (5, 2); 3 over 3: one instance each; 4 over 1."""
    _run(shard_rows_check, "layout")


def test_rows_reach_their_shard_and_come_back_in_list_order(shard_rows_check):
    """Batch 5 over 2 shards with the list [4, 0, 3] and columns of width 3, of width 0 and given, NULL, of int codes and of eicos_info
    records; batch 3 over 3 with [1] (one call, shard 1); one shard; count 0 (no call); idx NULL = instances 0 .. count-1 with count
    0, 2 and batch.  Every output byte equals the plain loop's."""
    _run(shard_rows_check, "routing")


def test_a_refused_list_reaches_no_shard(shard_rows_check):
    """A duplicate, -1, an index equal to batch, count > batch, NULL idx with count > 0, the idx-NULL form with count = batch + 1: the
    callable never runs, every output keeps its sentinel, the text is index_list_fault's behind the caller's name."""
    _run(shard_rows_check, "refusals")


def test_a_failing_shard_leaves_its_rows_untouched(shard_rows_check):
    """The callable returns EICOS_E_INVALID for one shard of two after writing its scratch: the code comes back, that shard's rows of
    the outputs keep their sentinel, the other shard's are written."""
    _run(shard_rows_check, "failing")


def test_column_rules_at_width_zero(shard_rows_check):
    """An output of width 0 reaches the callable as NULL (exact), as the caller's pointer (given) or as one writable element of scratch
    (at least one); a given input of width 0 as the caller's pointer; a column that was not given as NULL."""
    _run(shard_rows_check, "rules")


def test_seeded_sweep_against_the_plain_loop(shard_rows_check):
    """200 seeds: batch <= 9, up to 4 shards, a random duplicate-free list of random length (0 included), 1 to 4 columns of widths 0 to 3
    of every element type and rule, now and then a failing shard; every output compared byte by byte."""
    _run(shard_rows_check, "sweep")
