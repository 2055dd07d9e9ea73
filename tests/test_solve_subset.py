"""Subset solves (eicos_exit_class, eicos_batch_select / _solve_subset / _solve_where / _gather and their eicos_multi_* forms,
include/eicos_amd.h): one solve launch over a chosen set of instances -- an index list, or the instances of some exit classes, selected
on the GPU -- instead of the whole batch.

A subset launch is the unchanged solve kernel with the launch order = the chosen ids and the batch = their number.  So every GPU check
is an equality: an instance of the subset ends with the bits a whole-batch solve of a twin handle leaves, every other instance keeps
what it had (its info record included), select() returns what the host predicate exit_class gives over info_arrays(), and gather()
returns rows of solution() / duals() / info_arrays().  The CPU test checks the exit classes, which need no GPU."""
import os

import numpy as np
import pytest

import eicos_amd
from eicos_amd import binding
from eicos_amd.binding import ShiftMap
from eicos_amd.generate import feasible_batch, random_socp_pattern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KEYS = ("Gpr", "Apr", "c", "h", "b")
INFO_SKIP = ("solve_us",)  # (a time)
# the solve-kernel builds: the table of tests/test_settings.py
W2 = {"EICOS_UBL": "0", "EICOS_THREADS": "256"}
DEF256 = {"EICOS_UBL": "0", "EICOS_THREADS": "256", "EICOS_W2": "0"}
BUILDS = [
    ("lp_afiro", 8, {}, ("lds-resident", 128)),
    ("MPC02", 4, W2, ("w2", 256)),
    ("MPC02", 4, DEF256, ("default", 256)),
    ("MPC02", 4, {"EICOS_UBL": "0", "EICOS_W2": "0", "EICOS_THREADS": "128"}, ("default", 128)),
    ("MPC02", 4, {"EICOS_UBL": "0", "EICOS_W2": "0", "EICOS_THREADS": "512"}, ("default", 512)),
    ("issue98", 4, {"EICOS_THREADS": "256"}, ("u-in-lds", 256)),
    ("MPC02", 4, {"EICOS_NLDS": "0", "EICOS_DUAL": "0"}, "no-lds"),  # a handle without an LDS vector
    ("socp-random", 8, {}, None),                                     # second-order cones (and equality rows)
]
# the ten documented exit codes and their class bits (include/eicos_amd.h)
CLASS_OF = {0: "SEL_OPTIMAL", 1: "SEL_PINF", 2: "SEL_DINF", 10: "SEL_OPTIMAL_INACC", 11: "SEL_PINF_INACC", 12: "SEL_DINF_INACC",
            -1: "SEL_MAXIT", -2: "SEL_NUMERICS", -3: "SEL_OUTCONE", -7: "SEL_FATAL"}


# ---- helpers ----------------------------------------------------------------------------------------------------------------------
_DATA = {}


def _data(name, B):
    """Pattern and a batch of strictly feasible instances (feasible_batch: every instance has an optimum); computed once per case."""
    if (name, B) not in _DATA:
        if name == "socp-random":  # 8 LP rows, cones of 4 and 7, 6 equality rows
            pat, base = random_socp_pattern(30, 6, 8, [4, 7], seed=5)
        else:
            pat, sets = eicos_amd.read_epb(os.path.join(GOLDEN, name + ".epb"))
            base = sets[0]
        _DATA[name, B] = (pat, feasible_batch(pat, base, 0, B))
    return _DATA[name, B]


def _handle(pat, d, B, build=None):
    g = eicos_amd.BatchSolver(pat, B)
    if build == "no-lds":
        assert g.dims()["lds_bytes"] == 0
    elif build is not None:
        assert (g.kernel_build(), g.dims()["threads_per_block"]) == build, (g.kernel_build(), g.dims()["threads_per_block"])
    g.update(*[d[k] for k in KEYS])
    return g


def _setup(name, B, env, build, monkeypatch, handles=2):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pat, d = _data(name, B)
    return (pat, d) + tuple(_handle(pat, d, B, build) for _ in range(handles))


def _state(g, kkt=False):
    """Everything the host can read of every instance: every info field but the time, x, y, z, s (and the KKT values of debug_kkt)."""
    ia = g.info_arrays()
    y, z, s = g.duals()
    st = {"x": g.solution(), "y": y, "z": z, "s": s, **{"info." + k: v for k, v in ia.items() if k not in INFO_SKIP}}
    if kkt:
        st["kkt"] = np.stack([g.debug_kkt(i)[2] for i in range(g.batch)])
    return st


def _assert_rows(a, b, rows, what):
    """rows `rows` of two states are the same bits"""
    assert a.keys() == b.keys()
    rows = np.asarray(rows, dtype=np.int64)
    for k in a:
        assert np.array_equal(a[k][rows], b[k][rows], equal_nan=True), (what, k)


def _classes(g):
    ia = g.info_arrays()
    return np.array([eicos_amd.exit_class(int(c), int(f)) for c, f in zip(ia["exitcode"], ia["n_factor"])])


def _perturbed(d, seed=7):
    rng = np.random.default_rng(seed)
    return (d["c"] * (1 + 0.01 * rng.uniform(-1, 1, d["c"].shape)), d["h"] + 0.01 * (1 + np.abs(d["h"])) * rng.uniform(0, 1, d["h"].shape), d["b"])


# ---- CPU --------------------------------------------------------------------------------------------------------------------------
def test_exit_class_needs_no_gpu():
    bits = []
    for code, name in CLASS_OF.items():
        bit = getattr(eicos_amd, name)
        assert eicos_amd.exit_class(code, 1) == bit, (code, name)
        assert eicos_amd.exit_class(code, 7) == bit
        assert eicos_amd.exit_class(code, 0) == eicos_amd.SEL_UNSOLVED, code  # (a fresh record, whatever its code)
        assert bit & (bit - 1) == 0 and bit > 0  # a single bit
        bits.append(bit)
    assert len(set(bits)) == 10
    for code in (9, 5, -87, 3, 13, -4):  # (9 = MAXIT + the inaccuracy offset is documented but never formed)
        assert eicos_amd.exit_class(code, 1) == eicos_amd.SEL_OTHER, code
        assert eicos_amd.exit_class(code, 0) == eicos_amd.SEL_UNSOLVED
    assert eicos_amd.SEL_OTHER == 1 << 10 and eicos_amd.SEL_UNSOLVED == 1 << 11 and [b.bit_length() - 1 for b in bits] == list(range(10))
    assert eicos_amd.SEL_FAILED == eicos_amd.SEL_MAXIT | eicos_amd.SEL_NUMERICS | eicos_amd.SEL_OUTCONE | eicos_amd.SEL_FATAL
    every = 0
    for k in range(12):
        every |= 1 << k
    assert eicos_amd.SEL_NOT_OPTIMAL == every & ~eicos_amd.SEL_OPTIMAL
    # the subset calls refuse a NULL handle before they touch a GPU
    L = binding._lib()
    one = np.zeros(1, np.int32)
    assert L.eicos_batch_solve_subset(None, binding._ip(one), 1, None) == -1 and b"NULL handle" in L.eicos_last_error()
    assert L.eicos_batch_select(None, 1, None, None) == -1 and b"NULL handle" in L.eicos_last_error()
    assert L.eicos_multi_solve_where(None, 1, None, None, None) == -1 and b"NULL handle" in L.eicos_multi_last_error()
    assert L.eicos_multi_gather(None, binding._ip(one), 1, None, None, None, None, None) == -1 and b"NULL handle" in L.eicos_multi_last_error()


# ---- GPU --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,B,env,build", BUILDS)
def test_subset_equals_whole_and_rest_is_untouched(name, B, env, build, monkeypatch):
    pat, d, A, Bh, Ch = _setup(name, B, env, build, monkeypatch, handles=3)
    codes = A.solve()
    want, fresh = _state(A, kkt=True), _state(Ch, kkt=True)
    S = [B - 1, 0, 2]  # unsorted, with the first and the last instance
    rest = [i for i in range(B) if i not in S]
    got_codes = Bh.solve_subset(S)
    got = _state(Bh, kkt=True)
    assert np.array_equal(got_codes, codes[S]), (got_codes, codes)
    _assert_rows(got, want, S, (name, env, "subset rows"))
    _assert_rows(got, fresh, rest, (name, env, "rows outside the subset"))
    assert np.array_equal(Bh.info_arrays()["solve_us"][rest], np.zeros(len(rest)))  # (the time of an instance that never ran)
    got_codes = Bh.solve_subset(rest)
    assert np.array_equal(got_codes, codes[rest])
    _assert_rows(_state(Bh, kkt=True), want, range(B), (name, env, "after the complement"))
    for g in (A, Bh, Ch):
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("name,B,env,build", [BUILDS[1], BUILDS[7]])
def test_warm_subset_equals_warm_whole(name, B, env, build, shift, monkeypatch):
    pat, d, A, Bh = _setup(name, B, env, build, monkeypatch)
    if shift:  # the identity plus a constant offset on x
        ident = (np.full(pat.n, 1e-3), np.arange(pat.n + 1, dtype=np.int32), np.arange(pat.n, dtype=np.int32), np.ones(pat.n))
        smap = ShiftMap(pat.n, pat.p, pat.m, x=ident)
    c2, h2, b2 = _perturbed(d)
    for g in (A, Bh):
        g.set_warm_start(0.1)
        if shift:
            g.set_shift_map(smap)
            assert g.has_shift_map() == 1
        assert (g.solve() == 0).all()
        g.update_rhs(c2, h2, b2 if pat.p else None)
    before = _state(Bh, kkt=True)
    codes = A.solve()
    want = _state(A, kkt=True)
    S = [B - 1, 0, 2]
    rest = [i for i in range(B) if i not in S]
    assert np.array_equal(Bh.solve_subset(S), codes[S])
    got = _state(Bh, kkt=True)
    _assert_rows(got, want, S, (name, shift, "warm subset rows"))
    _assert_rows(got, before, rest, (name, shift, "rows outside the subset"))
    print(name, "shift", shift, "iterations cold", before["info.iter"], "warm", want["info.iter"])
    A.close()
    Bh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,env,build", [("MPC02", 8, W2, ("w2", 256)), ("lp_afiro", 8, {}, ("lds-resident", 128))])
def test_select_and_retry(name, B, env, build, monkeypatch):
    pat, d, twin, g = _setup(name, B, env, build, monkeypatch)
    S1, S2 = [6, 1, 4], [3, 0]
    rest = [i for i in range(B) if i not in S1 + S2]
    g.set_settings(iter_max=2)
    capped_codes = g.solve_subset(S1)
    g.set_settings(**eicos_amd.default_settings())
    assert (g.solve_subset(S2) == 0).all()
    cls = _classes(g)
    print(name, "codes of the capped instances", capped_codes, "classes", cls)
    assert (cls[S2] == eicos_amd.SEL_OPTIMAL).all() and (cls[rest] == eicos_amd.SEL_UNSOLVED).all()
    assert ((cls[S1] & (eicos_amd.SEL_OPTIMAL | eicos_amd.SEL_UNSOLVED)) == 0).all(), cls  # two passes are below every instance's count
    assert len(set(cls)) >= 3
    before = _state(g)
    for mask in (eicos_amd.SEL_OPTIMAL, eicos_amd.SEL_UNSOLVED, eicos_amd.SEL_NOT_OPTIMAL, eicos_amd.SEL_FAILED | eicos_amd.SEL_OPTIMAL_INACC):
        want = np.nonzero(cls & mask)[0]
        got = g.select(mask)
        assert got.dtype == np.int32 and np.array_equal(got, want), (mask, got, want)
    _assert_rows(_state(g), before, range(B), "select changes nothing")
    want = np.nonzero(cls & eicos_amd.SEL_NOT_OPTIMAL)[0]
    ids, codes = g.solve_where(eicos_amd.SEL_NOT_OPTIMAL)
    assert np.array_equal(ids, want) and set(ids) == set(S1 + rest)
    left = g.select(eicos_amd.SEL_UNSOLVED)  # (NOT_OPTIMAL holds the UNSOLVED bit: nobody is left)
    assert g.solve_subset(left).size == left.size
    twin_codes = twin.solve()
    assert np.array_equal(codes, twin_codes[ids])
    _assert_rows(_state(g, kkt=True), _state(twin, kkt=True), range(B), (name, "retried handle against the plain cold solve"))
    twin.close()
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,env,build", [BUILDS[0], BUILDS[1], BUILDS[7]])
def test_gather_returns_rows_of_the_results(name, B, env, build, monkeypatch):
    pat, d, g = _setup(name, B, env, build, monkeypatch, handles=1)
    g.solve_subset([1, B - 1])  # (solved and fresh records side by side)
    x, (y, z, s), ia = g.solution(), g.duals(), g.info_arrays()
    for idx in ([B - 1, 0, 2], list(range(B))[::-1], [1]):
        got = g.gather(idx)
        for k, full in (("x", x), ("y", y), ("z", z), ("s", s)):
            assert got[k].shape == (len(idx), full.shape[1]) and np.array_equal(got[k], full[idx], equal_nan=True), (name, idx, k)
        assert got["info"].keys() == ia.keys()
        for k in ia:  # (the same handle, nothing ran in between: the time too)
            assert np.array_equal(got["info"][k], ia[k][idx], equal_nan=True), (name, idx, k)
    empty = g.gather([])
    assert empty["x"].shape == (0, pat.n) and empty["info"]["exitcode"].size == 0
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,env,build", [BUILDS[0], BUILDS[1]])
def test_trace_after_a_subset_launch(name, B, env, build, monkeypatch):
    pat, d, A, Bh = _setup(name, B, env, build, monkeypatch)
    assert B <= A.dims()["resident_blocks"]
    A.solve()
    iters = A.info_arrays()["iter"]
    S = [B - 1, 0, 2]
    Bh.solve_subset(S)
    for i in range(B):
        if i in S:
            rows = int(iters[i]) + 1  # (the rows this solve wrote: the slot may hold older rows of another instance behind them)
            assert np.array_equal(Bh.debug_trace(i)[:rows], A.debug_trace(i)[:rows], equal_nan=True), (name, i)
        else:
            with pytest.raises(RuntimeError, match="not in the last launch"):
                Bh.debug_trace(i)
    # a plain solve afterwards is an ordinary whole-batch launch again: every instance has its slot (the twin solves again as well: the
    # first row of a trace shows the step and sigma the instance's previous solve ended with)
    Bh.solve_subset([i for i in range(B) if i not in S])
    Bh.solve()
    A.solve()
    for i in range(B):
        rows = int(iters[i]) + 1
        assert np.array_equal(Bh.debug_trace(i)[:rows], A.debug_trace(i)[:rows], equal_nan=True), (name, i)
    A.close()
    Bh.close()


@pytest.mark.gpu
def test_refusals_and_empty_subsets(monkeypatch):
    name, B, env, build = BUILDS[0]
    pat, d, g = _setup(name, B, env, build, monkeypatch, handles=1)
    g.solve_subset([0, 1, 2, 3])
    before, ms, hist = _state(g, kkt=True), g.last_solve_ms(), g.ms_history("solve")
    refused = [
        (lambda: g.solve_subset([1, 5, 1]), "duplicate index 1"),
        (lambda: g.solve_subset([0, B]), f"index {B} at position 1"),
        (lambda: g.solve_subset([-1]), "index -1 at position 0"),
        (lambda: g.solve_subset(list(range(B)) + [0]), f"count {B + 1}"),
        (lambda: g.solve_subset_async([2, 2]), "duplicate index 2"),
        (lambda: g.gather([0, B + 3]), f"index {B + 3} at position 1"),
        (lambda: g.gather([4, 4]), "duplicate index 4"),
        (lambda: g.select(0), "mask is 0"),
        (lambda: g.solve_where(0), "mask is 0"),
        (lambda: g.select(1 << 12), "bits above bit 11"),
        (lambda: g.solve_where(eicos_amd.SEL_OPTIMAL | 1 << 12), "bits above bit 11"),
    ]
    for call, msg in refused:
        with pytest.raises(RuntimeError, match=msg):
            call()
        _assert_rows(_state(g, kkt=True), before, range(B), msg)
        assert g.last_solve_ms() == ms and g.ms_history("solve") == hist, msg
    # not refused, and nothing is launched or recorded
    assert g.solve_subset([]).size == 0
    g.solve_subset_async([])
    ids, codes = g.solve_where(eicos_amd.SEL_FATAL)  # (nobody: four instances are optimal, four unsolved)
    assert ids.size == 0 and codes.size == 0 and g.select(eicos_amd.SEL_FATAL).size == 0
    _assert_rows(_state(g, kkt=True), before, range(B), "empty subsets")
    assert g.last_solve_ms() == ms and g.ms_history("solve") == hist
    g.close()


@pytest.mark.gpu
def test_multi_matches_the_single_handle(monkeypatch):
    for k, v in W2.items():
        monkeypatch.setenv(k, v)
    B = 5
    pat, d = _data("MPC02", B)
    eicos_amd.set_arithmetic_profile(1)  # (plans by the pattern alone: a shard of 3 or 2 gives the bits of the batch of 5)
    try:
        one = eicos_amd.BatchSolver(pat, B)
        multi = eicos_amd.MultiBatchSolver(pat, B, [0, 0])
    finally:
        eicos_amd.set_arithmetic_profile(0)
    assert [(f, c) for f, c, _ in multi.shards()] == [(0, 3), (3, 2)]
    for g in (one, multi):
        g.update(*[d[k] for k in KEYS])
    for S in ([4, 0, 2], [1, 0]):  # both shards; the first shard only
        assert np.array_equal(multi.solve_subset(S), one.solve_subset(S)), S
        _assert_rows(_state(multi), _state(one), range(B), ("multi solve_subset", S))
    with pytest.raises(RuntimeError, match="duplicate index 3"):
        multi.solve_subset([3, 0, 3])
    with pytest.raises(RuntimeError, match=f"index {B} at position 0"):
        multi.gather([B])
    _assert_rows(_state(multi), _state(one), range(B), "a refused list changes no shard")
    for mask in (eicos_amd.SEL_UNSOLVED, eicos_amd.SEL_OPTIMAL, eicos_amd.SEL_NOT_OPTIMAL):
        assert np.array_equal(multi.select(mask), one.select(mask)), mask
    assert np.array_equal(one.select(eicos_amd.SEL_UNSOLVED), [3])
    ids_m, codes_m = multi.solve_where(eicos_amd.SEL_UNSOLVED)  # (the second shard only)
    ids_1, codes_1 = one.solve_where(eicos_amd.SEL_UNSOLVED)
    assert np.array_equal(ids_m, ids_1) and np.array_equal(codes_m, codes_1) and np.array_equal(ids_1, [3])
    _assert_rows(_state(multi), _state(one), range(B), "multi solve_where")
    idx = [3, 0, 4, 1]
    gm, g1 = multi.gather(idx), one.gather(idx)
    x, (y, z, s) = one.solution(), one.duals()
    for k, full in (("x", x), ("y", y), ("z", z), ("s", s)):
        assert np.array_equal(gm[k], full[idx], equal_nan=True) and np.array_equal(g1[k], full[idx], equal_nan=True), k
    for k in g1["info"]:
        if k not in INFO_SKIP:
            assert np.array_equal(gm["info"][k], g1["info"][k], equal_nan=True), k
    one.close()
    multi.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,env,build", [BUILDS[0], BUILDS[2]])
def test_plain_solve_after_a_subset_launch(name, B, env, build, monkeypatch):
    """The launch record leaks no subset state: a whole-batch solve behind a subset launch gives the bits of a twin that never ran one."""
    pat, d, A, Bh = _setup(name, B, env, build, monkeypatch)
    c2, h2, b2 = _perturbed(d, seed=11)
    for g in (A, Bh):
        g.set_warm_start(0.1)
    A.solve()
    Bh.solve_subset([2, 0])
    Bh.solve_subset([1, 3] + list(range(4, B)))
    for g in (A, Bh):
        g.update_rhs(c2, h2, b2 if pat.p else None)
    codes = A.solve()
    assert np.array_equal(Bh.solve(), codes)
    _assert_rows(_state(Bh, kkt=True), _state(A, kkt=True), range(B), (name, "whole batch after subset launches"))
    A.close()
    Bh.close()


@pytest.mark.gpu
def test_subset_beyond_one_instance_per_cu_is_sorted_and_equal(monkeypatch):
    """More chosen instances than CUs (256 on an MI355X): the selection kernel orders them longest first through its counting sort, and
    more of them than resident workgroups go through the queue.  The order decides which workgroup solves what, never the result."""
    B = 1200
    pat, d = _data("lp_afiro", B)
    A, Bh = (_handle(pat, d, B) for _ in range(2))
    rng = np.random.default_rng(3)
    S = rng.permutation(B)[:700]
    rest = np.setdiff1d(np.arange(B), S)
    c2, h2, b2 = _perturbed(d, seed=5)
    for g in (A, Bh):
        g.set_warm_start(0.1)
        g.solve()  # (the previous solve's work is the sort key)
        g.update_rhs(c2, h2, b2 if pat.p else None)
    before = _state(Bh)
    codes = A.solve()
    assert np.array_equal(Bh.solve_subset(S), codes[S])
    got, want = _state(Bh), _state(A)
    assert len(set(want["info.n_ldlsolve"][S])) > 1  # (several keys: the sort has something to do)
    _assert_rows(got, want, S, "sorted subset rows")
    _assert_rows(got, before, rest, "rows outside the sorted subset")
    assert np.array_equal(Bh.solve_subset(rest), codes[rest])  # (level with the twin again)
    ids, codes_w = Bh.solve_where(eicos_amd.SEL_ALL)  # every instance, selected on the GPU: more than one tile of the scan
    assert np.array_equal(ids, np.arange(B)) and np.array_equal(codes_w, A.solve())
    _assert_rows(_state(Bh), _state(A), range(B), "whole batch by class")
    A.close()
    Bh.close()
