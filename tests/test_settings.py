"""Runtime solver settings (eicos_settings_default / _size, eicos_batch_set_settings / _get_settings and their eicos_multi_* forms,
include/eicos_amd.h): the exit tolerances and their relaxed counterparts, the iteration cap and the refinement controls of the KKT solves,
per handle, in effect from the next solve launch.

The settings change WHERE the interior-point loop stops and how long a KKT solve refines, never the arithmetic of a pass.  So the GPU tests
are equalities: explicit defaults give the bits of an untouched handle on every build of the solve kernel; a run capped at K passes
reports row K of the default run's per-pass trace; a run with loosened tolerances stops at the pass that the exit test, restated on the
host from that trace, predicts; and a closed loop under non-default settings is the same on the fused, the per-step and the host-loop
path.  The CPU tests check the defaults, the struct size and the refusals that need no GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import eicos_amd
from eicos_amd import binding
from eicos_amd.binding import OutputMap, ParamMap, PlantMap, ShiftMap
from eicos_amd.generate import feasible_batch, random_socp_pattern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KEYS = ("Gpr", "Apr", "c", "h", "b")
# the ten values of struct Settings of the reference (include/eicos.hpp:23-47)
REFERENCE_DEFAULTS = dict(feastol=1e-8, abstol=1e-8, reltol=1e-8, feastol_inacc=1e-4, abstol_inacc=5e-5, reltol_inacc=5e-5,
                          linsysacc=1e-14, irerrfact=6.0, iter_max=100, nitref=9)
# Exit codes of a run that stops at the iteration cap.  The kernel's checkExitConditions numbers a relaxed ("inaccurate") exit as the
# plain code + EICOS_INACC_OFFSET (10): 10 = close to optimal, 11 = close to primal infeasible, 12 = close to dual infeasible; when the
# relaxed test fails too the code is EICOS_MAXIT = -1 as it stands (9 = MAXIT + the offset is in the documented set, the kernel does
# not form it).
MAXIT, MAXIT_INACC, OPTIMAL_INACC, PINF_INACC, DINF_INACC = -1, 9, 10, 11, 12
CAP_CODES = (MAXIT, MAXIT_INACC, OPTIMAL_INACC, PINF_INACC, DINF_INACC)
ALL_CODES = (0, 1, 2, -1, -2, -3, -7, 10, 11, 12)  # (include/eicos_amd.h: exit codes per instance)
INFO_SKIP = ("solve_us",)  # (a time)
# the solve-kernel builds (the environment sets of the other files' build tables) and the other handles the issue names
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
TRACE = {k: j for j, k in enumerate(eicos_amd.BatchSolver.TRACE_COLS)}
ROW_KEYS = ("pcost", "dcost", "gap", "pres", "dres", "tau", "kap")  # what an info record and a trace row share


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


def _handle(pat, d, B, build=None, **settings):
    g = eicos_amd.BatchSolver(pat, B)
    if build == "no-lds":
        assert g.dims()["lds_bytes"] == 0
    elif build is not None:
        assert (g.kernel_build(), g.dims()["threads_per_block"]) == build, (g.kernel_build(), g.dims()["threads_per_block"])
    if settings:
        g.set_settings(**settings)
    g.update(*[d[k] for k in KEYS])
    return g


def _state(g, codes):
    """Everything a solve leaves that the host can read: exit codes, every info field but the time, x, y, z, s."""
    ia = g.info_arrays()
    y, z, s = g.duals()
    return {"codes": np.asarray(codes).copy(), "x": g.solution(), "y": y, "z": z, "s": s, **{"info." + k: v for k, v in ia.items() if k not in INFO_SKIP}}


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def _default_run(name, B, env, build, monkeypatch):
    """A cold solve under the default settings: the handle's state and the per-pass trace of every instance."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pat, d = _data(name, B)
    g = _handle(pat, d, B, build)
    st = _state(g, g.solve())
    traces = [g.debug_trace(i).copy() for i in range(B)]
    g.close()
    return pat, d, st, traces


_ORACLE_END = {}


def _oracle_end(name, B, i, **settings):
    """(exit code, iterations) of the CPU oracle on instance i of _data(name, B) under `settings`; computed once."""
    key = (name, B, i, tuple(sorted(settings.items())))
    if key not in _ORACLE_END:
        from eicos_amd.problem_io import Values
        from oracle.oracle import OracleSolver
        pat, d = _data(name, B)
        o = OracleSolver(pat, Values(*[d[k][i] for k in KEYS]))
        o.set_settings(**settings)
        _ORACLE_END[key] = (o.solve(), o.info()["iter"])
        o.close()
    return _ORACLE_END[key]


def _row_matches(st, i, row, what):
    for k in ROW_KEYS:
        a, b = st["info." + k][i], row[TRACE[k]]
        assert a == b or (np.isnan(a) and np.isnan(b)), (what, i, k, a, b)


# ---- CPU --------------------------------------------------------------------------------------------------------------------------
def test_settings_defaults_and_struct_size():
    L = binding._lib()
    st = binding.Settings()
    for k, _ in st._fields_:  # (every field is written by the call)
        setattr(st, k, -1)
    L.eicos_settings_default(C.byref(st))
    assert st.asdict() == REFERENCE_DEFAULTS
    assert (st.feastol, st.abstol, st.reltol, st.feastol_inacc, st.abstol_inacc, st.reltol_inacc) == (1e-8, 1e-8, 1e-8, 1e-4, 5e-5, 5e-5)
    assert (st.linsysacc, st.irerrfact, st.iter_max, st.nitref) == (1e-14, 6.0, 100, 9)
    assert C.sizeof(binding.Settings) == L.eicos_settings_size() == 8 * 8 + 2 * 4
    dflt = eicos_amd.default_settings()
    assert dflt == REFERENCE_DEFAULTS and len(dflt) == 10
    assert isinstance(dflt["iter_max"], int) and isinstance(dflt["nitref"], int)


def test_settings_refusals_without_a_handle():
    g = eicos_amd.BatchSolver.__new__(eicos_amd.BatchSolver)  # (no handle: an unknown name must be refused before the library is called)
    g._h = None
    with pytest.raises(TypeError, match="bogus"):
        g.set_settings(bogus=1)
    mg = eicos_amd.MultiBatchSolver.__new__(eicos_amd.MultiBatchSolver)
    mg._h = None
    with pytest.raises(TypeError, match="bogus"):
        mg.set_settings(feastol=1e-6, bogus=1)
    L = binding._lib()
    st = binding.Settings()
    L.eicos_settings_default(C.byref(st))
    for fn, err in ((L.eicos_batch_set_settings, L.eicos_last_error), (L.eicos_batch_get_settings, L.eicos_last_error),
                    (L.eicos_multi_set_settings, L.eicos_multi_last_error), (L.eicos_multi_get_settings, L.eicos_multi_last_error)):
        assert fn(None, C.byref(st)) == -1 and b"NULL handle" in err()  # (EICOS_E_INVALID)
    L.eicos_settings_default(None)  # (a NULL destination is ignored)


# ---- GPU --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,B,env,build", BUILDS)
def test_explicit_defaults_change_nothing(name, B, env, build, monkeypatch):
    pat, d, want, _ = _default_run(name, B, env, build, monkeypatch)
    g = _handle(pat, d, B, build, **eicos_amd.default_settings())
    assert g.settings() == REFERENCE_DEFAULTS
    _assert_same(_state(g, g.solve()), want, (name, B, env))
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,env,build", [BUILDS[0], BUILDS[1], BUILDS[2], BUILDS[6], BUILDS[7]])
def test_iteration_cap_replays_the_default_run(name, B, env, build, monkeypatch):
    pat, d, dflt, traces = _default_run(name, B, env, build, monkeypatch)
    assert (dflt["codes"] == 0).all(), dflt["codes"]
    N = int(dflt["info.iter"].min())  # (the cap is a setting of the handle: K < N is below every instance's count)
    assert N >= 4, N
    hit = 0
    for K in sorted({1, N // 2, N - 1}):
        g = _handle(pat, d, B, build, iter_max=K)
        st = _state(g, g.solve())
        g.close()
        what = (name, env, K)
        print(what, "codes", st["codes"], "iter", st["info.iter"])
        assert (st["info.iter"] <= K).all(), (what, st["info.iter"])
        assert np.isin(st["codes"], CAP_CODES).all(), (what, st["codes"])
        assert np.array_equal(st["codes"], st["info.exitcode"]), what
        for i in range(B):
            if st["info.iter"][i] == K:  # (no best iterate restored: the record describes pass K, and passes 0 .. K are the default run's)
                _row_matches(st, i, traces[i][K], what)
                hit += 1
    assert hit > 0  # (the equality was checked at least once)


def _predict(trace, n_iter, tau):
    """The OPTIMAL branch of the kernel's exit test restated on the rows 0 .. n_iter of a default run's trace, for feastol = abstol =
    reltol = tau, evaluated as the kernel evaluates it (left to right, `&&` and `||` stop at the first operand that decides).  Returns
    (pass, clear): the first pass at which the branch holds, and whether every quantity that is compared on the way lies a factor of
    two or more away from tau (then the rounding of the reconstructed c'x = pcost * tau and of relgap cannot matter).  The two
    infeasibility branches are not restated: the trace does not hold pinfres / dinfres, and the instances are strictly feasible -- a
    run that left through one of them would fail the exit-code assertion of the test."""
    clear = True

    def lt(v, bound):  # v < bound, with bound > 0
        nonlocal clear
        if not np.isfinite(v) or (bound / 2 <= v <= bound * 2):
            clear = False
        return v < bound

    for r in range(n_iter + 1):
        row = trace[r]
        pcost, dcost, gap, pres, dres, tau_ = (row[TRACE[k]] for k in ("pcost", "dcost", "gap", "pres", "dres", "tau"))
        if not (np.isfinite(pcost) and np.isfinite(dcost) and tau_ > 0):
            return r, False
        relgap = gap / (-pcost) if pcost < 0 else (gap / dcost if dcost > 0 else None)  # (formed as the kernel forms it)
        # (-c'x > 0 || -b'y - h'z >= -abstol) && (pres < feastol && dres < feastol) && (gap < abstol || relgap < reltol), with
        # c'x = pcost * tau and b'y + h'z = -(dcost * tau); an absent relgap compares as smaller
        if ((pcost < 0 or lt(-(dcost * tau_), tau)) and lt(pres, tau) and lt(dres, tau)
                and (lt(gap, tau) or relgap is None or lt(relgap, tau))):
            return r, clear
    return None, False


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,env,build", [("lp_afiro", 2, {}, ("lds-resident", 128)), BUILDS[1], BUILDS[2], ("socp-random", 4, {}, None)])
def test_a_loosened_tolerance_stops_at_the_pass_the_default_trace_predicts(name, B, env, build, monkeypatch):
    """The tolerance is a setting of the handle, so ONE value of the grid has to be clear of every instance of the batch, and an
    instance alone rules out about three quarters of the grid (its pres of every pass, and dres, gap and relgap of the later ones, each
    shut out a window of a factor four).  Hence the small batches: on the traces of the CPU oracle the grid leaves lp_afiro 4 values
    at batch 2 and none at 3, MPC02 3 values at batch 4, the cone pattern 8 values at batch 4."""
    pat, d, dflt, traces = _default_run(name, B, env, build, monkeypatch)
    assert (dflt["codes"] == 0).all(), dflt["codes"]
    iters = dflt["info.iter"]
    chosen = None
    for tau in np.logspace(-7, -3, 40):
        pred = [_predict(traces[i], int(iters[i]), float(tau)) for i in range(B)]
        if all(c and p is not None for p, c in pred):
            chosen = (float(tau), np.array([p for p, _ in pred]))
            break
    assert chosen is not None, "no tolerance of the grid is clear of every compared quantity"
    tau, passes = chosen
    print((name, env), "tau", tau, "predicted passes", passes, "default iterations", iters)
    assert (passes >= 1).all() and (passes <= iters).all()
    g = _handle(pat, d, B, build, feastol=tau, abstol=tau, reltol=tau)
    st = _state(g, g.solve())
    g.close()
    what = (name, env, tau)
    assert (st["codes"] == 0).all(), (what, st["codes"])
    assert np.array_equal(st["info.iter"], passes), (what, st["info.iter"], passes)
    for i in range(B):
        _row_matches(st, i, traces[i][passes[i]], what)
    assert (st["info.pres"] < tau).all() and (st["info.dres"] < tau).all(), what
    assert ((st["info.gap"] < tau) | ((st["info.has_relgap"] != 0) & (st["info.relgap"] < tau))).all(), what
    # cross-check: default tolerances, capped at that pass -- both runs backscale the same current iterate
    checked = 0
    for K in sorted(set(int(v) for v in passes)):
        c = _handle(pat, d, B, build, iter_max=K)
        cs = _state(c, c.solve())
        c.close()
        for i in np.nonzero((passes == K) & (cs["info.iter"] == K))[0]:
            for k in "xyzs":
                assert np.array_equal(cs[k][i], st[k][i], equal_nan=True), (what, K, i, k)
            checked += 1
    assert checked > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,env,build,dual", [
    ("MPC02", 4, DEF256, ("default", 256), 1),  # one workgroup per CU: the two systems of a pass are solved in one sweep
    ("MPC02", 4, {**DEF256, "EICOS_DUAL": "0"}, ("default", 256), 0),
    ("lp_afiro", 8, {}, ("lds-resident", 128), None),
    ("socp-random", 8, {}, None, None),
])
def test_refinement_settings(name, B, env, build, dual, monkeypatch):
    """Asserts no accuracy: only that the counters follow the settings -- and, on MPC02 and lp_afiro, that every instance ends where the
    CPU oracle ends under the same nitref (accuracy itself: tests/test_unrefined_solves.py)."""
    pat, d, dflt, _ = _default_run(name, B, env, build, monkeypatch)
    what = (name, env)
    if dual is not None:
        g = eicos_amd.BatchSolver(pat, B)
        assert g.dims()["dual_rhs"] == dual, what
        g.close()
    n1, n2 = dflt["info.nitref1"], dflt["info.nitref2"]
    print(what, "default nitref1", n1, "nitref2", n2, "nitref3", dflt["info.nitref3"], "n_ldlsolve", dflt["info.n_ldlsolve"])
    # the two initialisation solves of a cold start see the same systems whatever the settings
    for c in (0, 1, 3):
        g = _handle(pat, d, B, build, nitref=c)
        st = _state(g, g.solve())
        g.close()
        assert np.array_equal(st["info.nitref1"], np.minimum(n1, c)), (what, c, st["info.nitref1"], n1)
        assert np.array_equal(st["info.nitref2"], np.minimum(n2, c)), (what, c, st["info.nitref2"], n2)
        if c == 0:
            assert (st["info.nitref3"] == 0).all(), (what, st["info.nitref3"])
            assert (st["info.n_ldlsolve"] < dflt["info.n_ldlsolve"]).all(), (what, st["info.n_ldlsolve"], dflt["info.n_ldlsolve"])
            assert np.isin(st["codes"], ALL_CODES).all(), (what, st["codes"])
        if name in ("MPC02", "lp_afiro"):
            for i in range(B):
                oc, oiter = _oracle_end(name, B, i, nitref=c)
                print(what, "nitref", c, "instance", i, "gpu", st["codes"][i], st["info.iter"][i], "oracle", oc, oiter)
                assert st["codes"][i] == oc and abs(int(st["info.iter"][i]) - oiter) <= 1, (what, c, i, st["codes"][i], st["info.iter"][i], oc, oiter)
    g = _handle(pat, d, B, build, linsysacc=1e-6)
    st = _state(g, g.solve())
    g.close()
    assert (st["info.nitref1"] <= n1).all() and (st["info.nitref2"] <= n2).all(), (what, st["info.nitref1"], st["info.nitref2"])


# The branch _predict does not restate: a relaxed infeasibility exit at the iteration cap.  The caps are the CPU oracle's: infeasible1 ends
# with 12 at iter_max 3 and 4 and with -1 below (from 5 on the plain certificate 1 ends it: 11 is not reachable at any cap, so that case is
# left out); unboundedLP1 ends with 12 at iter_max 3 and 4.
@pytest.mark.gpu
@pytest.mark.parametrize("name,cap,code", [("unboundedLP1", 3, DINF_INACC), ("unboundedLP1", 4, DINF_INACC), ("infeasible1", 3, DINF_INACC)])
def test_relaxed_infeasibility_exit_at_the_cap_matches_the_oracle(name, cap, code):
    from eicos_amd.problem_io import Values
    from oracle.oracle import OracleSolver
    pat, sets = eicos_amd.read_epb(os.path.join(GOLDEN, name + ".epb"))
    v = sets[0]
    reached = {}
    for k in range(1, 101):  # (the oracle, at every cap: which relaxed codes this fixture can end with at all; a fresh solver each time,
        o = OracleSolver(pat, Values(v.Gpr, v.Apr, v.c, v.h, v.b))  # since pinfres / dinfres survive a solve on one object)
        o.set_settings(iter_max=k)
        reached.setdefault(o.solve(), []).append(k)
        o.close()
    assert cap in reached.get(code, []), (name, reached)
    if name == "infeasible1":
        assert PINF_INACC not in reached, reached  # (why no case asks for it)
    B = 2
    g = eicos_amd.BatchSolver(pat, B)
    g.set_settings(iter_max=cap)
    g.update(*[np.repeat(np.asarray(getattr(v, k), np.float64)[None, :], B, 0) for k in KEYS])
    codes = np.asarray(g.solve()).copy()
    iters = g.info_arrays()["iter"].copy()
    g.close()
    assert list(codes) == [code] * B and (iters <= cap).all(), (name, cap, codes, iters)


def _csr(rows):
    rowptr = np.concatenate(([0], np.cumsum([len(c) for c, _ in rows]))).astype(np.int32)
    col = np.concatenate([np.asarray(c, np.int64) for c, _ in rows] + [np.zeros(0, np.int64)]).astype(np.int32)
    val = np.concatenate([np.asarray(v, np.float64) for _, v in rows] + [np.zeros(0)])
    return rowptr, col, val


def _random_rows(rng, rows, cols, scale):
    """0-4 entries per row in shuffled order, row 0 with up to 8; the last row empty (from two rows on)."""
    out = []
    for j in range(rows):
        cnt = min(cols, 8) if j == 0 else int(rng.integers(0, min(4, cols) + 1))
        c = rng.permutation(cols)[:cnt]
        out.append((c, rng.uniform(-1, 1, c.size) * (scale if np.isscalar(scale) else scale[j])))
    if rows >= 2:
        out[-1] = (np.zeros(0, np.int64), np.zeros(0))
    return out


def _loop_maps(pat, d, k, r, seed=0):
    """A parameter map (c, h, b around instance 0's vectors, entries about 1e-3 of them), an output map (r rows over x), a plant map
    (theta+ = f0 + F [theta | u]: a few tenths on theta, hundredths on u) and a shift map (identity rows, a tenth of them altered)."""
    rng = np.random.default_rng(7000 + seed)
    groups = {}
    for gname in "chb":
        base = d[gname][0]
        if base.size:
            scale = 1e-3 * (np.abs(base) + np.mean(np.abs(base)) + 1e-6)
            groups[gname] = (base.copy(),) + _csr(_random_rows(rng, base.size, k, scale))
    pm = ParamMap(k, **groups)
    om = OutputMap(pat.n, (rng.uniform(-1, 1, r),) + _csr(_random_rows(rng, r, pat.n, 2.0)))
    frows = []
    for j, (c, v) in enumerate(_random_rows(rng, k, k + r, 1.0)):
        frows.append((c, np.where(c < k, 0.2, 0.01) * v))
    fm = PlantMap(k, r, (rng.uniform(0, 0.5, k),) + _csr(frows))
    sgroups = {}
    for gname, rows in (("x", pat.n), ("y", pat.p), ("z", pat.m), ("s", pat.m)):
        if rows < 2:
            continue
        srows = [([j], [1.0]) for j in range(rows)]
        for q, j in enumerate(rng.choice(rows, max(1, rows // 10), replace=False)):
            other = int((j + 1 + rng.integers(0, rows - 1)) % rows)
            srows[j] = ([other], [1.0]) if q % 2 == 0 else (sorted((int(j), other), reverse=True), [0.75, 0.25])
        sgroups[gname] = (np.zeros(rows),) + _csr(srows)
    return pm, om, fm, ShiftMap(pat.n, pat.p, pat.m, **sgroups)


def _host_loop(ref, fm, theta0, T):
    """T calls of update_param_solve, the theta rows advanced on the host by PlantMap.evaluate: u, theta, exit codes, iterations in the
    layout of rollout()."""
    B, k = theta0.shape
    pth, pu = eicos_amd.PinnedArray((B, k)), eicos_amd.PinnedArray((B, fm.r))
    th, thetas, us, codes, iters = theta0.copy(), [theta0.copy()], [], [], []
    for _ in range(T):
        pth.a[...] = th
        pu.a[...] = np.nan
        codes.append(np.asarray(ref.update_param_solve(pth.a, u_out=pu.a)).copy())
        iters.append(ref.info_arrays()["iter"].copy())
        us.append(pu.a.copy())
        th = fm.evaluate(th, us[-1], None)
        thetas.append(th)
    pth.close(); pu.close()
    return np.stack(us, axis=1), np.stack(thetas, axis=1), np.stack(codes, axis=1), np.stack(iters, axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,k,r", [("lp_afiro", 16, 1, 3), ("MPC02", 8, 7, 6)])
@pytest.mark.parametrize("warm", [False, True])
def test_closed_loop_under_settings_is_the_same_on_every_path(name, B, k, r, warm, monkeypatch):
    T, tau = 3, 1e-5
    pat, d = _data(name, B)
    pm, om, fm, sm = _loop_maps(pat, d, k, r)
    theta0 = np.random.default_rng(7100).uniform(0, 1, (B, k))

    def handle():
        g = _handle(pat, d, B)
        assert (g.solve() == 0).all()  # (default settings: a warm first step starts from an optimum, and is shifted)
        g.set_settings(iter_max=5, feastol=tau, abstol=tau, reltol=tau)
        g.set_param_map(pm); g.set_output_map(om); g.set_plant_map(fm)
        if warm:
            g.set_warm_start(0.1); g.set_shift_map(sm)
        return g

    what = (name, B, warm)
    g = handle()
    fused = g.rollout(theta0, T)
    assert g.last_rollout_launches() == 1, what
    fused_x = g.solution()
    g.close()
    monkeypatch.setenv("EICOS_FUSED_UPDATE", "0")
    g = handle()
    steps = g.rollout(theta0, T)
    assert g.last_rollout_launches() == T, what
    steps_x = g.solution()
    g.close()
    monkeypatch.delenv("EICOS_FUSED_UPDATE")
    g = handle()
    host = _host_loop(g, fm, theta0, T)
    host_x = g.solution()
    g.close()
    print(what, "codes", fused[2].tolist(), "iters", fused[3].tolist())
    for other, other_x, label in ((steps, steps_x, "per step"), (host, host_x, "host loop")):
        for q, (a, b) in enumerate(zip(fused, other)):
            assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), (what, label, ("u", "theta", "exitcodes", "iters")[q])
        assert np.array_equal(fused_x, other_x, equal_nan=True), (what, label, "x")
    assert (fused[3] <= 5).all(), (what, fused[3])


@pytest.mark.gpu
def test_settings_validation_names_the_field_and_changes_nothing():
    pat, d = _data("lp_afiro", 2)
    g = eicos_amd.BatchSolver(pat, 2)
    g.set_settings(feastol=1e-6, nitref=4, iter_max=50, irerrfact=3.0)
    before = g.settings()
    assert before == {**REFERENCE_DEFAULTS, "feastol": 1e-6, "nitref": 4, "iter_max": 50, "irerrfact": 3.0}
    L = binding._lib()
    bad = [(k, v) for k in binding.SETTINGS_FIELDS[:8] for v in (float("nan"), 0.0, -1e-8, float("inf"))]
    bad += [("iter_max", 0), ("iter_max", 101), ("iter_max", -3), ("nitref", -1), ("nitref", 101)]
    for k, v in bad:
        st = binding.Settings(**before)
        setattr(st, k, v)
        assert L.eicos_batch_set_settings(g._h, C.byref(st)) == -1, (k, v)  # (EICOS_E_INVALID)
        assert k.encode() in L.eicos_last_error(), (k, v, L.eicos_last_error())
        assert g.settings() == before, (k, v)
        with pytest.raises(RuntimeError, match=k):
            g.set_settings(**{k: v})
        assert g.settings() == before, (k, v)
    assert L.eicos_batch_set_settings(g._h, None) == -1 and L.eicos_batch_get_settings(g._h, None) == -1
    assert g.settings() == before
    # the edges of the ranges are accepted
    g.set_settings(iter_max=1, nitref=0)
    g.set_settings(iter_max=100, nitref=100)
    assert g.settings() == {**before, "iter_max": 100, "nitref": 100}
    g.close()


@pytest.mark.gpu
def test_multi_settings_match_one_handle():
    B = 8
    pat, d = _data("MPC02", B)
    custom = dict(feastol=1e-5, abstol=2e-5, reltol=3e-5, feastol_inacc=1e-3, abstol_inacc=5e-4, reltol_inacc=6e-4, linsysacc=1e-12,
                  irerrfact=4.0, iter_max=7, nitref=2)
    # (plans shaped by the pattern alone: an instance then gives the same bits in a shard of 4 and in a batch of 8, include/eicos_amd.h)
    eicos_amd.set_arithmetic_profile(1)
    try:
        m = eicos_amd.MultiBatchSolver(pat, B, [0, 0])
        one = eicos_amd.BatchSolver(pat, B)
    finally:
        eicos_amd.set_arithmetic_profile(0)
    assert m.shards() == [(0, 4, 0), (4, 4, 0)]
    assert m.settings() == REFERENCE_DEFAULTS
    m.set_settings(**custom)
    assert m.settings() == custom
    st = binding.Settings()
    assert binding._lib().eicos_multi_get_settings(m._h, C.byref(st)) == 0 and st.asdict() == custom
    with pytest.raises(RuntimeError, match="iter_max"):
        m.set_settings(iter_max=0)
    assert m.settings() == custom
    one.set_settings(**custom)
    for g in (m, one):
        g.update(*[d[k] for k in KEYS])
    got, want = _state(m, m.solve()), _state(one, one.solve())
    _assert_same(got, want, "multi")
    assert (got["info.iter"] <= 7).all()
    m.close(); one.close()


CPP = r'''
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>
#include "eicos.hpp"
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(f)), {});
    if (raw.size() < 36 || std::memcmp(raw.data(), "EPB1", 4)) return 2;
    const int *hd = reinterpret_cast<const int *>(raw.data() + 4);
    int n = hd[0], m = hd[1], p = hd[2], l = hd[3], nc = hd[4], nnzG = hd[5], nnzA = hd[6];
    const int *ip = hd + 8;
    std::vector<int> q(ip, ip + nc); ip += nc;
    std::vector<int> Gjc(ip, ip + n + 1); ip += n + 1;
    std::vector<int> Gir(ip, ip + nnzG); ip += nnzG;
    std::vector<int> Ajc(ip, ip + n + 1); ip += n + 1;
    std::vector<int> Air(ip, ip + nnzA); ip += nnzA;
    const double *dp = reinterpret_cast<const double *>(ip);
    std::vector<double> Gpr(dp, dp + nnzG); dp += nnzG;
    std::vector<double> Apr(dp, dp + nnzA); dp += nnzA;
    std::vector<double> c(dp, dp + n); dp += n;
    std::vector<double> h(dp, dp + m); dp += m;
    std::vector<double> b(dp, dp + p);
    EiCOS::Solver solver(n, m, p, l, nc, q.data(), m ? Gpr.data() : nullptr, Gjc.data(), Gir.data(),
                         p ? Apr.data() : nullptr, Ajc.data(), Air.data(), c.data(), h.data(), b.data());
    const EiCOS::exitcode first = solver.solve();
    std::printf("default: exit %d iter %zu\n", int(first), solver.getInfo().iter);
    solver.getSettings().iter_max = 3;
    const EiCOS::exitcode capped = solver.solve();
    std::printf("capped: exit %d iter %zu\n", int(capped), solver.getInfo().iter);
    eicos_settings held;
    // (a Solver is a batch of one: the handle is not exposed, so read the cap back through a second solve's behaviour and a bad value)
    solver.getSettings().iter_max = 0;
    const EiCOS::exitcode refused = solver.solve();
    std::printf("refused: exit %d (%s)\n", int(refused), eicos_last_error());
    solver.getSettings().iter_max = 100;
    const EiCOS::exitcode again = solver.solve();
    std::printf("restored: exit %d iter %zu\n", int(again), solver.getInfo().iter);
    eicos_settings_default(&held);
    EiCOS::Settings s = EiCOS::Settings::from(held);
    return (s.iter_max == 100 && s.maxit == 100) ? 0 : 3;
}
'''


@pytest.mark.gpu
def test_cpp_solver_pushes_its_settings(tmp_path):
    src, exe = tmp_path / "settings_demo.cpp", str(tmp_path / "settings_demo")
    src.write_text(CPP)
    lib = os.path.join(ROOT, "eicos_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", lib, "-leicos_amd", "-Wl,-rpath," + lib, "-o", exe])
    out = subprocess.run([exe, os.path.join(GOLDEN, "feas.epb")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(ln.split(": ", 1) for ln in out.stdout.strip().splitlines())
    code = lambda s: int(s.split()[1])      # noqa: E731
    iters = lambda s: int(s.split()[3])     # noqa: E731
    assert code(lines["default"]) == 0 and iters(lines["default"]) > 3, out.stdout
    assert iters(lines["capped"]) <= 3 and code(lines["capped"]) != 0, out.stdout  # (the cap reached the handle: not `optimal` any more)
    assert code(lines["refused"]) == -7 and "iter_max" in lines["refused"], out.stdout  # (exitcode::fatal; the message names the field)
    assert (code(lines["restored"]), iters(lines["restored"])) == (code(lines["default"]), iters(lines["default"])), out.stdout
