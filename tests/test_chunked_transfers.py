"""The transfers that go through a staging area in chunks (eicos_amd/csrc/chunk_plan.hpp), run with at least three chunks and a short
last one: the pageable bounce in, the pageable result out and the matrix-map staging.  How many chunks a shape gives is asked of the
header itself, through tests/host/chunk_plan_check.cpp.  The bounce in and the matrix-map staging reach such shapes in
test_gpu_parity.py (MPC02, 600 instances) and test_matrix_param.py (MPC02, 600 instances under a cap of 32 MB) -- the first test
below says so from the rules, so that a change of a rule or of those shapes shows; the GPU test adds the result path, whose chunked
rows no test compared with rows that came another way, and runs the bounce in at the smallest batch that gives 2 * chunk + 1 rows."""
import os
import subprocess

import numpy as np
import pytest

import eicos_amd
import test_rhs_update as R  # (its _data, _device_arrays, _free_device, KEYS)
from conftest import ROOT
from eicos_amd.binding import _dp

KEYS = R.KEYS


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    """chunk(which, a, count[, cap]) -> what chunk_plan.hpp gives."""
    exe = str(tmp_path_factory.mktemp("chunk_plan") / "chunk_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "eicos_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "chunk_plan_check.cpp"), "-o", exe])

    def chunk(which, *args):
        out = subprocess.run([exe, which] + [str(a) for a in args], capture_output=True, text=True, check=True).stdout.split()
        return [int(v) for v in out]
    return chunk


def _widths(dims):
    return [dims[k] for k in ("nnzG", "nnzA", "n", "m", "p")]


def _chunks(count, chunk):
    """(number of chunks, rows of the last one)"""
    n = -(-count // chunk)
    return n, count - (n - 1) * chunk


def _three_and_a_short_one(count, chunk):
    n, last = _chunks(count, chunk)
    return n >= 3 and 0 < last < chunk


def test_the_shapes_of_the_gpu_tests_give_three_chunks_and_a_short_last_one(rule):
    pat, _ = eicos_amd.read_epb(os.path.join(ROOT, "tests", "golden", "MPC02.epb"))
    w = [pat.nnzG, pat.nnzA, pat.n, pat.m, pat.p]
    assert (pat.n, pat.m, pat.p) == (1496, 3996, 499) and sum(w) == 15470  # (124 KB of inputs an instance)
    # test_gpu_parity.py::test_host_pointer_update_and_result_paths_are_bit_identical: all five arrays of 600 instances, pageable
    chunk, = rule("in", sum(w), 600)
    assert chunk == 135 and _chunks(600, chunk) == (5, 60)
    # test_matrix_param.py, the case of 600 instances under EICOS_MATRIX_STAGE_MB=32: all five groups mapped
    chunk, = rule("matrix", sum(w) + 5 * 8, 600, 32 * (1 << 20) // 8)
    assert chunk == 270 and _chunks(600, chunk) == (3, 60)
    assert (270 * w[1]) % 8 != 0  # (rows * w is no multiple of 8 there: the round-up of that layout is at work)
    # the GPU test below: 271 instances in, z and s of 271 instances out
    chunk, = rule("in", sum(w), 271)
    assert chunk == 135 and _chunks(271, chunk) == (3, 1)
    chunk, small = rule("out", pat.m * 8, 271)
    assert chunk == 131 and not small and _chunks(271, chunk) == (3, 9)


@pytest.mark.gpu
def test_chunked_bounce_in_and_result_out_match_the_device_pointer_and_pinned_paths(rule):
    """MPC02, 271 instances = 2 * 135 + 1.  In: the five pageable arrays through the bounce buffers (chunks of 135, 135 and 1) against
    update_device on device copies of the same arrays: the same KKT values in the last chunk's instance, the same solve.  Out: y, z and
    s into pageable arrays (z, s: chunks of 131, 131 and 9 rows of 3996 doubles through the bounce buffers) against the same rows
    fetched into pinned arrays, which take one strided copy each; x likewise (one chunk)."""
    B = 271
    pat, d = R._data("MPC02", B)
    g, ref = eicos_amd.BatchSolver(pat, B), eicos_amd.BatchSolver(pat, B)
    w = _widths(g.dims())
    assert _three_and_a_short_one(B, rule("in", sum(w), B)[0])
    chunk, small = rule("out", pat.m * 8, B)
    assert not small and _three_and_a_short_one(B, chunk)
    dev = R._device_arrays([d[k] for k in KEYS])
    pins = [eicos_amd.PinnedArray((B, width)) for width in (pat.n, pat.p, pat.m, pat.m)]
    try:
        g.update(*[d[k] for k in KEYS])
        assert g.last_update_path() == "pinned bounce"
        ref.update_device(*dev)
        for i in (0, 134, 135, 269, B - 1):  # the first and last instance of every chunk
            assert np.array_equal(g.debug_kkt(i)[2], ref.debug_kkt(i)[2]), i
        codes, codes_ref = g.solve(), ref.solve()
        assert np.array_equal(codes, codes_ref) and np.all(codes == 0)
        x, (y, z, s) = g.solution(), g.duals()
        px, py, pz, ps = [p.a for p in pins]
        for a in (px, py, pz, ps):
            a[...] = np.nan
        g.solution_into(px)
        g._call("duals", _dp(py), _dp(pz), _dp(ps))  # (duals() itself, on the pinned arrays)
        for name, got, want in (("x", x, px), ("y", y, py), ("z", z, pz), ("s", s, ps)):
            assert np.array_equal(got, want), name
            assert np.all(np.isfinite(got)) and len(np.unique(got[[0, 130, 131, 261, 262, B - 1]], axis=0)) > 1, name
        xr, (yr, zr, sr) = ref.solution(), ref.duals()
        for name, got, want in (("x", x, xr), ("y", y, yr), ("z", z, zr), ("s", s, sr)):
            assert np.array_equal(got, want), name
    finally:
        R._free_device(dev)
        for p in pins:
            p.close()
        g.close(); ref.close()
