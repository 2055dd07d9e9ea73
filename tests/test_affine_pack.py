"""The one path of the five affine maps (parameter, output, plant, matrix, shift), checked without a GPU: the host validator and packer of
eicos_amd/csrc/affine_pack.hpp through a stand-alone program built with the address and undefined-behaviour sanitizers, and the one
evaluator of the binding, bit for bit against a plain loop in Python floats."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from eicos_amd.binding import MatrixMap, OutputMap, ParamMap, PlantMap, ShiftMap, _affine_eval, _as_group


def test_host_validator_and_packer_under_sanitizers(tmp_path):
    """tests/host/affine_pack_check.cpp: every message of the validation ladder as the setters report it, the first of two faults, and
    the packed layout offset by offset (with and without a gap).  Its own process; nothing is loaded into this one."""
    exe = str(tmp_path / "affine_pack_check")
    # (the sanitizer runtimes linked statically: the program then also starts where the environment preloads a library into every process)
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "eicos_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "affine_pack_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


# ---- the evaluator --------------------------------------------------------------------------------------------------------------

def _loop(group, v):
    """The contract, restated with nothing but Python floats: row by row, entry by entry in stored order, acc = acc + (val * v[col])."""
    base, rowptr, col, val = group
    out = np.empty((len(v), len(base)))
    for q in range(len(v)):
        for r in range(len(base)):
            acc = float(base[r])
            for t in range(int(rowptr[r]), int(rowptr[r + 1])):
                acc = acc + float(val[t]) * float(v[q][int(col[t])])
            out[q, r] = acc
    return out


def _group(rows, cols, seed, entries=True):
    """rows x cols: row 0 holds one column three times among others, row 1 is empty, the others hold 0..4 entries in random column order;
    magnitudes spread over ten decades, so that any other order of the sums shows in the last bits.  entries = False: no entry at all."""
    rng = np.random.default_rng(seed)
    lengths = np.zeros(rows, np.int64)
    if entries:
        lengths[:] = rng.integers(0, 5, rows)
        lengths[0] = 6
        if rows > 1:
            lengths[1] = 0
    rowptr = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
    col = rng.integers(0, cols, int(rowptr[-1])).astype(np.int32)
    if entries:
        col[[0, 2, 5]] = cols - 1
    val = rng.standard_normal(col.size) * 10.0 ** rng.integers(-5, 6, col.size)
    base = rng.standard_normal(rows) * 10.0 ** rng.integers(-5, 6, rows)
    return base, rowptr, col, val


def _rows(B, width, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, width)) * 10.0 ** rng.integers(-3, 4, (B, width))


def _same(a, b):
    return a.dtype == b.dtype == np.float64 and a.shape == b.shape and a.tobytes() == b.tobytes()


BATCHES = (1, 3)


def test_group_has_the_rows_the_cases_need():
    base, rowptr, col, val = _group(7, 4, 0)
    assert rowptr[1] == 6 and list(col[:6]).count(3) >= 3 and rowptr[2] == rowptr[1] and rowptr[-1] == col.size == val.size
    assert _group(7, 4, 0, entries=False)[1].tolist() == [0] * 8


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("entries", (True, False))
def test_affine_eval_equals_the_plain_loop(B, entries):
    g = _as_group(_group(7, 4, 1, entries))
    v = _rows(B, 4, 2)
    assert _same(_affine_eval(g, v), _loop(g, v))
    # lists come out as the arrays the C side reads; None stays None
    lists = _as_group(tuple(a.tolist() for a in g))
    assert [a.dtype for a in lists] == [np.float64, np.int32, np.int32, np.float64] and all(a.flags.c_contiguous for a in lists)
    assert _same(_affine_eval(lists, v), _loop(g, v)) and _as_group(None) is None


@pytest.mark.parametrize("B", BATCHES)
def test_param_map_evaluate(B):
    k = 4
    gc, gb = _group(7, k, 3), _group(2, k, 4, entries=False)
    theta = _rows(B, k, 5)
    c, h, b = ParamMap(k, c=gc, b=gb).evaluate(theta)
    assert h is None and _same(c, _loop(gc, theta)) and _same(b, _loop(gb, theta))


@pytest.mark.parametrize("B", BATCHES)
def test_output_map_evaluate(B):
    n = 9
    for entries in (True, False):
        g = _group(3, n, 6, entries)
        x = _rows(B, n, 7)
        om = OutputMap(n, g)
        assert om.r == 3 and _same(om.evaluate(x), _loop(g, x))


@pytest.mark.parametrize("B", BATCHES)
def test_plant_map_evaluate(B):
    k, r = 5, 2
    for entries in (True, False):
        g = _group(k, k + r, 8, entries)
        theta, u, w = _rows(B, k, 9), _rows(B, r, 10), _rows(B, k, 11)
        z = [list(theta[q]) + list(u[q]) for q in range(B)]  # z = [theta | u]
        ref = _loop(g, z)
        fm = PlantMap(k, r, g)
        assert _same(fm.evaluate(theta, u), ref)
        with_w = np.array([[float(ref[q, j]) + float(w[q, j]) for j in range(k)] for q in range(B)]).reshape(B, k)  # the disturbance last
        assert _same(fm.evaluate(theta, u, w), with_w)


@pytest.mark.parametrize("B", BATCHES)
def test_matrix_map_evaluate(B):
    k = 3
    gG, gA = _group(11, k, 12), _group(4, k, 13, entries=False)
    theta = _rows(B, k, 14)
    G, A = MatrixMap(k, G=gG, A=gA).evaluate(theta)
    assert _same(G, _loop(gG, theta)) and _same(A, _loop(gA, theta))
    G, A = MatrixMap(k, A=gA).evaluate(theta)
    assert G is None and _same(A, _loop(gA, theta))


@pytest.mark.parametrize("B", BATCHES)
def test_shift_map_evaluate(B):
    n, p, m = 6, 2, 4
    gx, gs = _group(n, n, 15), _group(m, m, 16, entries=False)
    x, y, z, s = _rows(B, n, 17), _rows(B, p, 18), _rows(B, m, 19), _rows(B, m, 20)
    sm = ShiftMap(n, p, m, x=gx, s=gs)
    x1, y1, z1, s1 = sm.evaluate(x, y, z, s)
    assert _same(x1, _loop(gx, x)) and _same(s1, _loop(gs, s))
    assert y1 is y and z1 is z  # groups without a map pass through as they were given
    assert sm.evaluate(x=None, s=s)[0] is None and _same(sm.evaluate(s=s)[3], _loop(gs, s))
