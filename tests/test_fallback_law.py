"""The fallback map: a backup output law for steps whose solve does not end in a wanted class (eicos_batch_set_fallback_map /
_fallback_mask / _fallback_counts and their eicos_multi_* forms, include/eicos_amd.h).

With the map on a handle, a step call that holds theta -- update_param_solve, update_param_solve_subset, rollout, rollout_jacobian --
forms the u row of an instance whose FINAL record is in a class of the mask as u = v0 + V theta instead of as the output map of x;
nothing else the call leaves or returns changes.  So every GPU check is an equality against a TWIN handle without the map: the twin's
u rows with the fired rows replaced on the host by FallbackMap.evaluate(theta) (a numpy-scalar restatement in the stated order), the
twin's state, codes and x rows as they are, and for rollout_jacobian the twin's param_jacobian with the fired rows replaced by
FallbackMap.dense() and 0.0.  Every GPU comparison is np.array_equal.

The iteration caps come from the CPU oracle's iteration counts on the data of the step (an instance that converges in k passes gets
through a cap c iff k <= c), so that where the counts differ some instances fall back and some do not; the tests assert that where
the oracle predicts it, and print the sets.  The CPU tests check the host restatement, the refusals that need no GPU and the ABI table."""
import ctypes as C

import numpy as np
import pytest

import eicos_amd
from eicos_amd import binding
from eicos_amd.binding import FallbackMap
from eicos_amd.problem_io import Values
import test_rhs_update as R       # (its device-array helpers)
import test_inlaunch_retry as RT  # (its _policy, _install, _host_retry)
import test_param_update as P     # (its _map, _theta, _data)
import test_rollout as RO         # (its _fmap, _w, _assert_rollout)
import test_rollout_jacobian as RJ  # (its _capped_handles)
from test_param_step import _omap
from test_solve_subset import BUILDS, KEYS, _assert_rows, _classes, _handle, _state

NOT_OPTIMAL = eicos_amd.SEL_NOT_OPTIMAL
K, NR = 7, 6
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
NO_LDS = BUILDS[6][2]
NOT_FUSED = {"EICOS_FUSED_UPDATE": "0"}


# ---- helpers ----------------------------------------------------------------------------------------------------------------------
def _fbmap(k, r, mask=NOT_OPTIMAL, seed=0):
    """The law of a case: r rows over k columns with 0-4 entries per row in shuffled order; row 0 repeats a column, the last row (from
    two rows on) is empty.  Entries of a few tenths, so that u stays at the size of theta."""
    rng = np.random.default_rng(6000 + seed)
    rows = [rng.permutation(k)[:rng.integers(0, min(4, k) + 1)] for _ in range(r)]
    c = int(rng.integers(0, k))
    rows[0] = np.array([c, (c + 1) % k, c])
    if r >= 2:
        rows[r - 1] = np.zeros(0, np.int64)
    rowptr = np.concatenate(([0], np.cumsum([len(v) for v in rows]))).astype(np.int32)
    col = np.concatenate(rows).astype(np.int32)
    return FallbackMap(rng.uniform(-0.1, 0.1, r), (rowptr, col, rng.uniform(-0.3, 0.3, col.size)), mask, k=k)


_ITERS = {}


def _oracle_iters(name, B, pm, theta, seed):
    """The CPU oracle's (iteration count, exit code) of every instance of the batch under the right-hand sides of pm at theta, cold and
    under the default settings; computed once per case."""
    if (name, B, seed) not in _ITERS:
        from oracle.oracle import OracleSolver
        pat, d = P._data(name, B)
        c, h, b = pm.evaluate(theta)
        out = []
        for i in range(B):
            o = OracleSolver(pat, Values(d["Gpr"][i], d["Apr"][i], d["c"][i] if c is None else c[i], d["h"][i] if h is None else h[i],
                                         d["b"][i] if b is None else b[i]))
            code = o.solve()
            out.append((int(o.info()["iter"]), int(code)))
        _ITERS[name, B, seed] = np.array(out)
    return _ITERS[name, B, seed]


def _cap(iters):
    """(cap, both): the smallest count as the cap when the counts differ -- the instances above it stop at the cap, the others get
    through --, one pass less when they are all equal (then every instance stops)."""
    lo, hi = int(iters.min()), int(iters.max())
    return (lo, True) if lo < hi else (max(lo - 1, 1), False)


def _case(name, B, env, build, monkeypatch, handles=2, seed=0):
    """`handles` cold handles of a build with the parameter and the output map, the theta rows of the step and the cap the oracle gives."""
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    pat, d = P._data(name, B)
    pm, om = P._map(d, K), _omap(pat.n, NR)
    theta = P._theta(B, K, seed=seed)
    oi = _oracle_iters(name, B, pm, theta, seed)
    cap, both = _cap(oi[:, 0])
    both = both and bool((oi[:, 1] == 0).all())  # (an instance the oracle does not take to OPTIMAL is outside the prediction)
    hs = []
    for _ in range(handles):
        g = _handle(pat, d, B, build)
        g.set_param_map(pm); g.set_output_map(om)
        g.set_settings(iter_max=cap)
        hs.append(g)
    return pat, theta, oi, cap, both, hs


def _fired(codes, mask):
    return np.array([(eicos_amd.exit_class(int(c), 1) & mask) != 0 for c in np.asarray(codes).ravel()]).reshape(np.shape(codes))


def _step(g, theta, kind, n):
    """One update_param_solve of g with theta / u_out / x_out in memory of `kind`; returns codes, u, x as numpy arrays."""
    B, r = theta.shape[0], g.output_count()
    if kind == "pageable":
        u, x = np.full((B, r), np.nan), np.full((B, n), np.nan)
        return g.update_param_solve(theta.copy(), u_out=u, x_out=x), u, x
    if kind in ("pinned", "pinned theta, pageable u"):
        pth, pu, px = (eicos_amd.PinnedArray(s) for s in (theta.shape, (B, r), (B, n)))
        pth.a[...] = theta; pu.a[...] = np.nan; px.a[...] = np.nan
        if kind == "pinned":
            codes, u, x = g.update_param_solve(pth.a, u_out=pu.a, x_out=px.a), pu.a.copy(), px.a.copy()
        else:
            u, x = np.full((B, r), np.nan), np.full((B, n), np.nan)
            codes = g.update_param_solve(pth.a, u_out=u, x_out=x)
        for p_ in (pth, pu, px):
            p_.close()
        return codes, u, x
    # device memory of the HIP runtime the library is linked against (torch brings a HIP runtime of its own, which finds no GPU in a
    # process where the library's runtime has opened it first -- as every test process has by now)
    assert kind == "device"
    L = binding._lib()
    dev = R._device_arrays((theta, np.full((B, r), np.nan), np.full((B, n), np.nan)))
    try:
        codes, u, x = np.zeros(B, np.int32), np.zeros((B, r)), np.zeros((B, n))
        rc = L.eicos_batch_update_param_solve(g._h, C.cast(dev[0], DP), C.cast(dev[1], DP), C.cast(dev[2], DP), codes.ctypes.data_as(IP))
        assert rc == 0, L.eicos_last_error()
        assert L.hipMemcpy(u.ctypes.data, dev[1], u.nbytes, 2) == 0 and L.hipMemcpy(x.ctypes.data, dev[2], x.nbytes, 2) == 0  # hipMemcpyDeviceToHost
    finally:
        R._free_device(dev)
    return codes, u, x


def _step_contract(A, Bh, fb, theta, kind, n, what):
    """The contract of one step: A holds the map, its twin Bh does not.  Returns the fired ids."""
    B = theta.shape[0]
    before = A.fallback_counts()
    codes_a, u_a, x_a = _step(A, theta, kind, n)
    codes_b, u_b, x_b = _step(Bh, theta, kind, n)
    fired = np.nonzero(_fired(codes_b, fb.mask))[0]
    want_u = u_b.copy()
    want_u[fired] = fb.evaluate(theta)[fired]
    print(what, kind, "codes", np.asarray(codes_b).tolist(), "fired", fired.tolist())
    assert np.array_equal(u_a, want_u), (what, kind, "u")
    assert np.all(np.isfinite(u_a)), (what, kind)
    _assert_rows(_state(A, kkt=True), _state(Bh, kkt=True), range(B), (what, kind, "state"))
    assert np.array_equal(codes_a, codes_b) and np.array_equal(x_a, x_b), (what, kind)
    counts = A.fallback_counts()
    want = np.zeros(B, np.int32)
    want[fired] = 1
    assert counts.dtype == np.int32 and np.array_equal(counts - before, want), (what, kind, counts, fired)
    return fired


def _rollout_handles(env, monkeypatch, n, name="MPC02", B=4, seed=0):
    """n cold handles with the three maps, theta0, w, T and the cap that splits step 0 by the oracle's counts."""
    pat, theta0, oi, cap, both, hs = _case(name, B, env, None, monkeypatch, handles=n, seed=seed)
    fm = RO._fmap(K, NR)
    for g in hs:
        g.set_plant_map(fm)
    T = 3
    return pat, theta0, RO._w(B, T, K), T, fm, oi, cap, both, hs


def _host_loop(ref, fm, fb, theta0, T, w, jac=False, retry=None):
    """The host loop on a handle WITHOUT the map: per step the parametric step (retry: the host retry sequence of test_inlaunch_retry
    behind it), the fired rows replaced on the host, the plant map on the host.  Returns (u, theta, codes, iters[, J, res]) in the
    layout of rollout() / rollout_jacobian(), and the fired steps [B, T]."""
    B, k = theta0.shape
    th, thetas, us, codes, iters, Js, ress, fired = theta0.copy(), [theta0.copy()], [], [], [], [], [], []
    for t in range(T):
        if retry is None:
            u = np.full((B, fm.r), np.nan)
            ref.update_param_solve(th.copy(), u_out=u)
        else:
            ref.update_param(th.copy())
            ref.solve()
            RT._host_retry(ref, range(B), *retry)
            u = ref.outputs()
        ia = ref.info_arrays()
        codes.append(ia["exitcode"].copy()); iters.append(ia["iter"].copy())
        f = (_classes(ref) & fb.mask) != 0
        if jac:
            J, res = ref.param_jacobian()
            J[f] = fb.dense(k); res[f] = 0.0
            Js.append(J); ress.append(res)
        u[f] = fb.evaluate(th)[f]
        fired.append(f); us.append(u)
        th = fm.evaluate(th, u, None if w is None else w[:, t])
        thetas.append(th)
    out = (np.stack(us, axis=1), np.stack(thetas, axis=1), np.stack(codes, axis=1), np.stack(iters, axis=1))
    if jac:
        out += (np.stack(Js, axis=1), np.stack(ress, axis=1))
    return out, np.stack(fired, axis=1)


# ---- CPU --------------------------------------------------------------------------------------------------------------------------
def test_fallback_map_evaluate_equals_a_scalar_loop_and_matches_a_dense_product():
    k, r, B = 5, 4, 6
    fb = _fbmap(k, r)
    theta = np.random.default_rng(1).standard_normal((B, k))
    got = fb.evaluate(theta)
    want = np.zeros((B, r))
    for b in range(B):
        for j in range(r):
            acc = float(fb.base[j])
            for t in range(int(fb.rowptr[j]), int(fb.rowptr[j + 1])):
                acc = acc + (float(fb.val[t]) * float(theta[b, fb.col[t]]))
            want[b, j] = acc
    assert np.array_equal(got, want)
    # the vectorised evaluation the other maps share keeps the same order
    assert np.array_equal(got, binding._affine_eval((fb.base, fb.rowptr, fb.col, fb.val), theta))
    # a dense product sums the same terms in another order: per entry at most (terms + 1) roundings of the sum of their magnitudes
    dense = fb.base[None, :] + theta @ fb.dense().T
    mags = np.abs(fb.base)[None, :] + np.abs(theta) @ np.abs(fb.dense(k)).T + 1e-300
    terms = np.diff(fb.rowptr).max() + 2  # (dense() has summed duplicates first: one more rounding)
    assert np.all(np.abs(got - dense) <= terms * np.finfo(float).eps * mags)
    with pytest.raises(ValueError):
        fb.evaluate(np.zeros((B, k - 1)))
    with pytest.raises(ValueError):
        fb.evaluate(np.zeros(k))


def test_fallback_map_dense_accumulates_duplicates_in_stored_order():
    # row 0: column 2 three times -- ((0 + 1e16) + 1) - 1e16 is 0.0 in stored order and 1.0 in any order that cancels first
    fb = FallbackMap(np.zeros(2), (np.array([0, 3, 4]), np.array([2, 2, 2, 0]), np.array([1e16, 1.0, -1e16, 3.0])), NOT_OPTIMAL, k=3)
    J = fb.dense()
    assert J.shape == (2, 3)
    assert J[0, 2] == ((0.0 + 1e16) + 1.0) + -1e16 == 0.0
    assert np.array_equal(J, np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0]]))
    assert fb.dense(5).shape == (2, 5) and np.array_equal(fb.dense(5)[:, :3], J)
    assert (fb.r, fb.k, fb.mask) == (2, 3, NOT_OPTIMAL)


def test_fallback_entry_points_refuse_a_null_handle():
    L = binding._lib()
    one = np.zeros(1, np.int32)
    for rc in (L.eicos_batch_set_fallback_map(None, NOT_OPTIMAL, None), L.eicos_batch_fallback_mask(None),
               L.eicos_batch_fallback_counts(None, 0, 1, binding._ip(one), 0)):
        assert rc == -1 and b"NULL handle" in L.eicos_last_error()
    for rc in (L.eicos_multi_set_fallback_map(None, NOT_OPTIMAL, None), L.eicos_multi_fallback_mask(None),
               L.eicos_multi_fallback_counts(None, 0, 1, binding._ip(one), 0)):
        assert rc == -1 and b"NULL handle" in L.eicos_multi_last_error()


def test_fallback_map_of_the_wrong_shape_is_refused_before_the_library_is_called():
    k, r = 5, 4

    class Probe(binding._Solver):  # (a solver object whose library call would raise something else: the checks stand in front of it)
        batch = 3

        def _call(self, name, *a):
            raise AssertionError("the library was called: " + name)

        def param_count(self):
            return k

        def output_count(self):
            return r

    with pytest.raises(ValueError):
        Probe().set_fallback_map(_fbmap(k, r + 1))  # (rows against the handle's output count)
    bad = _fbmap(k, r)
    bad.rowptr = bad.rowptr[:-1]
    with pytest.raises(ValueError):
        Probe().set_fallback_map(bad)
    bad = _fbmap(k, r)
    bad.val = bad.val[:-1]
    with pytest.raises(ValueError):
        Probe().set_fallback_map(bad)
    with pytest.raises(AssertionError, match="set_fallback_map"):  # (a well-shaped map does reach the library)
        Probe().set_fallback_map(_fbmap(k, r))
    with pytest.raises(AssertionError, match="set_fallback_map"):  # (and so does a removal)
        Probe().set_fallback_map(None)


def test_the_abi_table_holds_the_fallback_entry_points():
    names = {name: args for name, args, _ in binding._SIGNATURES}
    L = binding._lib()
    for prefix in ("eicos_batch_", "eicos_multi_"):
        for f, nargs in (("set_fallback_map", 3), ("fallback_mask", 1), ("fallback_counts", 5)):
            assert prefix + f in names and len(names[prefix + f]) == nargs, prefix + f
            assert getattr(L, prefix + f).argtypes is not None  # (the library exports it)
    for f in ("set_fallback_map", "fallback_mask", "fallback_counts"):
        assert callable(getattr(eicos_amd.BatchSolver, f)) and callable(getattr(eicos_amd.MultiBatchSolver, f))
    assert eicos_amd.FallbackMap is FallbackMap


# ---- GPU --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,B,env,build", BUILDS)
def test_step_falls_back_on_every_build(name, B, env, build, monkeypatch):
    """Case 1: pinned theta, u_out and x_out -- the fused step where the handle has one (the law inside the solve kernel), the range
    kernels on the handle without an LDS vector."""
    pat, theta, oi, cap, both, (A, Bh) = _case(name, B, env, build, monkeypatch)
    fb = _fbmap(K, NR)
    assert A.fallback_mask() == 0
    A.set_fallback_map(fb)
    assert A.fallback_mask() == NOT_OPTIMAL and Bh.fallback_mask() == 0
    print(name, env, "oracle (iterations, code)", oi.tolist(), "cap", cap)
    fired = _step_contract(A, Bh, fb, theta, "pinned", pat.n, (name, env))
    if build != "no-lds":
        assert A.last_update_path() == "fused into the solve"
    if both:  # (a condition of the test: somebody fell back and somebody did not)
        assert 0 < len(fired) < B, (name, fired, oi.tolist())
    want = np.zeros(B, np.int32)
    want[fired] = 1
    assert np.array_equal(A.fallback_counts(reset=True), want)
    assert np.array_equal(A.fallback_counts(), np.zeros(B, np.int32))
    assert np.array_equal(Bh.fallback_counts(), np.zeros(B, np.int32))  # (a handle that never had a map)
    # removed: the next step is the twin's again, and counts nothing
    A.set_fallback_map(None)
    assert A.fallback_mask() == 0
    codes_a, u_a, _ = _step(A, theta, "pinned", pat.n)
    codes_b, u_b, _ = _step(Bh, theta, "pinned", pat.n)
    assert np.array_equal(u_a, u_b) and np.array_equal(codes_a, codes_b)
    assert np.array_equal(A.fallback_counts(), np.zeros(B, np.int32))
    A.close(); Bh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,env", [("pageable", {}), ("pinned theta, pageable u", {}), ("device", {}), ("pinned", NOT_FUSED), ("device", NOT_FUSED),
                                      ("pageable", NO_LDS), ("device", NO_LDS)])
def test_step_falls_back_on_every_path(kind, env, monkeypatch):
    """Case 2, MPC02 batch 4: the three calls from pageable theta, the fused launch that leaves a pageable u_out to the range kernel,
    device arrays, the fused path switched off, the handle without an LDS vector."""
    build = "no-lds" if env == NO_LDS else None
    pat, theta, oi, cap, both, (A, Bh) = _case("MPC02", 4, env, build, monkeypatch)
    fb = _fbmap(K, NR, seed=1)
    A.set_fallback_map(fb)
    fired = _step_contract(A, Bh, fb, theta, kind, pat.n, ("MPC02", env))
    fused = not env and kind != "pageable"
    if kind != "device" or fused:  # (the device-pointer update leaves no path behind)
        assert (A.last_update_path() == "fused into the solve") == fused, (kind, env, A.last_update_path())
    assert both and 0 < len(fired) < 4, (fired, oi.tolist())
    # a second step on the same handles: the counters are cumulative
    theta2 = P._theta(4, K, seed=5)
    fired2 = _step_contract(A, Bh, fb, theta2, kind, pat.n, ("MPC02", env, "second step"))
    want = np.zeros(4, np.int32)
    want[fired] += 1; want[fired2] += 1
    assert np.array_equal(A.fallback_counts(), want)
    A.close(); Bh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,env", [("pinned", {}), ("pageable", {}), ("pinned", NOT_FUSED), ("pageable", NO_LDS)])
def test_subset_step_falls_back_in_list_order(kind, env, monkeypatch):
    """Case 3: batch 8, a list of three ids in non-ascending order; the theta and u rows are in list order, the other instances keep
    their state and a zero counter."""
    name, B = "MPC02", 8
    pat, theta_all, oi, cap, both, (A, Bh, Ch) = _case(name, B, env, "no-lds" if env == NO_LDS else None, monkeypatch, handles=3)
    over = np.nonzero(oi[:, 0] > cap)[0]
    under = np.nonzero(oi[:, 0] <= cap)[0]
    assert both and len(over) >= 1 and len(under) >= 2, oi.tolist()
    idx = [int(under[-1]), int(over[0]), int(under[0])]  # (not ascending: the largest passing id first)
    assert idx != sorted(idx)
    rest = [i for i in range(B) if i not in idx]
    theta = theta_all[idx]  # row q belongs to instance idx[q]: the oracle's counts go with the instance's own row
    fb = _fbmap(K, NR, seed=2)
    A.set_fallback_map(fb)
    fresh = _state(Ch, kkt=True)

    def step(g):
        if kind == "pageable":
            u, x = np.full((3, NR), np.nan), np.full((3, pat.n), np.nan)
            return g.update_param_solve_subset(idx, theta.copy(), u_out=u, x_out=x), u, x
        pth, pu, px = (eicos_amd.PinnedArray(s) for s in ((3, K), (3, NR), (3, pat.n)))
        pth.a[...] = theta; pu.a[...] = np.nan; px.a[...] = np.nan
        out = g.update_param_solve_subset(idx, pth.a, u_out=pu.a, x_out=px.a), pu.a.copy(), px.a.copy()
        for p_ in (pth, pu, px):
            p_.close()
        return out

    codes_a, u_a, x_a = step(A)
    if kind == "pinned" and not env:
        assert A.last_update_path() == "fused into the solve"
    codes_b, u_b, x_b = step(Bh)
    f = _fired(codes_b, fb.mask)
    print(name, env, kind, "list", idx, "codes", np.asarray(codes_b).tolist(), "fired positions", np.nonzero(f)[0].tolist())
    assert f.tolist() == [False, True, False], (codes_b, oi.tolist())
    want_u = u_b.copy()
    want_u[f] = fb.evaluate(theta)[f]
    assert np.array_equal(u_a, want_u) and np.array_equal(x_a, x_b) and np.array_equal(codes_a, codes_b)
    got = _state(A, kkt=True)
    _assert_rows(got, _state(Bh, kkt=True), range(B), (name, "subset step"))
    _assert_rows(got, fresh, rest, (name, "rows outside the list"))
    want = np.zeros(B, np.int32)
    want[idx[1]] = 1
    assert np.array_equal(A.fallback_counts(), want), (A.fallback_counts(), idx)
    for g in (A, Bh, Ch):
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{}, NOT_FUSED, NO_LDS], ids=["fused", "not-fused", "no-lds"])
def test_rollout_equals_the_host_loop_with_the_rows_replaced(env, monkeypatch):
    """Case 4: rollout with the map and a disturbance, T = 3, against the host loop on the twin."""
    pat, theta0, w, T, fm, oi, cap, both, (A, ref) = _rollout_handles(env, monkeypatch, 2)
    B = theta0.shape[0]
    fb = _fbmap(K, NR, seed=3)
    A.set_fallback_map(fb)
    got = A.rollout(theta0, T, w)
    assert A.last_rollout_launches() == (1 if not env else T)
    want, fired = _host_loop(ref, fm, fb, theta0, T, w)
    print("MPC02", env, "oracle step 0", oi.tolist(), "cap", cap, "codes", want[2].tolist(), "fired", fired.astype(int).tolist())
    assert both and 0 < fired[:, 0].sum() < B, (fired, oi.tolist())  # (step 0, the step the oracle predicts, has both kinds)
    RO._assert_rollout(got, want, ("MPC02", env, "rollout under a fallback map"))
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1]))
    _assert_rows(_state(A, kkt=True), _state(ref, kkt=True), range(B), ("MPC02", env, "final state"))
    assert np.array_equal(A.fallback_counts(), fired.sum(axis=1))
    A.close(); ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{}, NOT_FUSED], ids=["fused", "not-fused"])
def test_every_class_in_the_mask_makes_the_rollout_a_numpy_recursion(env, monkeypatch):
    """Case 5: with SEL_ALL every step takes the law, so u and theta are the recursion of FallbackMap.evaluate and PlantMap.evaluate --
    no solver result is in them -- while the solves still run: the codes are the twin's."""
    pat, theta0, w, T, fm, oi, cap, both, (A, ref) = _rollout_handles(env, monkeypatch, 2)
    B = theta0.shape[0]
    fb = _fbmap(K, NR, mask=eicos_amd.SEL_ALL, seed=4)
    A.set_fallback_map(fb)
    assert A.fallback_mask() == eicos_amd.SEL_ALL
    u, th, codes, iters = A.rollout(theta0, T, w)
    assert A.last_rollout_launches() == (1 if not env else T)
    cur, us, ths = theta0.copy(), [], [theta0.copy()]
    for t in range(T):
        us.append(fb.evaluate(cur))
        cur = fm.evaluate(cur, us[-1], w[:, t])
        ths.append(cur)
    assert np.array_equal(u, np.stack(us, axis=1)) and np.array_equal(th, np.stack(ths, axis=1))
    # the twin without the map, fed the same theta rows step by step
    tc, ti = [], []
    for t in range(T):
        tc.append(np.asarray(ref.update_param_solve(th[:, t].copy())).copy())
        ti.append(ref.info_arrays()["iter"].copy())
    assert np.array_equal(codes, np.stack(tc, axis=1)) and np.array_equal(iters, np.stack(ti, axis=1))
    assert np.array_equal(A.fallback_counts(), np.full(B, T, np.int32))
    A.close(); ref.close()


@pytest.mark.gpu
def test_retry_first_then_fallback(monkeypatch):
    """Case 6, lp_afiro batch 8 (the oracle's counts at theta seed 0 are 12 five times, 13 twice and 19): first attempt under a cap of
    12, a cold retry under a cap of 13 -- the two instances at 13 succeed on the retry, the one at 19 fails twice and falls back."""
    name, B = "lp_afiro", 8
    pat, theta, oi, cap, both, (A, ref) = _case(name, B, {}, None, monkeypatch)
    levels = np.unique(oi[:, 0])
    assert both and len(levels) >= 3 and cap == levels[0], oi.tolist()
    cap2 = int(levels[1])
    launch, pol = RT._policy(iter_max=cap), RT._policy(iter_max=cap2)
    fm, fb = RO._fmap(K, NR), _fbmap(K, NR, seed=5)
    for g in (A, ref):
        g.set_plant_map(fm)
    RT._install(A, pol)
    A.set_fallback_map(fb)
    # one step, fused
    pth, pu = eicos_amd.PinnedArray((B, K)), eicos_amd.PinnedArray((B, NR))
    pth.a[...] = theta; pu.a[...] = np.nan
    codes = A.update_param_solve(pth.a, u_out=pu.a)
    assert A.last_update_path() == "fused into the solve"
    ref.update_param(theta.copy())
    ref.solve()
    retried = RT._host_retry(ref, range(B), pol, launch)
    twice = np.nonzero((_classes(ref) & fb.mask) != 0)[0]
    print(name, "oracle", oi.tolist(), "caps", cap, cap2, "retried", retried, "failed twice", twice.tolist())
    assert 0 < len(twice) < len(retried) < B  # (some retried instances succeed, some fail again, some never retry)
    want_u = ref.outputs()
    want_u[twice] = fb.evaluate(theta)[twice]
    assert np.array_equal(pu.a, want_u) and np.array_equal(codes, ref.info_arrays()["exitcode"])
    _assert_rows(_state(A, kkt=True), _state(ref, kkt=True), range(B), (name, "retry, then fallback"))
    want = np.zeros(B, np.int32)
    want[twice] = 1
    assert np.array_equal(A.fallback_counts(reset=True), want) and np.array_equal(A.retry_counts(reset=True), RT._counts_of(retried, B))
    pth.close(); pu.close()
    # and a rollout, where the retry and the law both act between the steps of the one launch
    T, w = 2, RO._w(B, 2, K)
    got = A.rollout(theta, T, w)
    assert A.last_rollout_launches() == 1
    want, fired = _host_loop(ref, fm, fb, theta, T, w, retry=(pol, launch))
    RO._assert_rollout(got, want, (name, "rollout: retry, then fallback"))
    assert np.array_equal(A.fallback_counts(), fired.sum(axis=1)) and np.array_equal(np.nonzero(fired[:, 0])[0], twice)  # (step 0 is the step above)
    _assert_rows(_state(A, kkt=True), _state(ref, kkt=True), range(B), (name, "rollout: final state"))
    A.close(); ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{}, NOT_FUSED], ids=["fused", "not-fused"])
def test_rollout_jacobian_records_the_law_for_fired_steps(env, monkeypatch):
    """Case 7: J and res of a step that did not fire are the twin's param_jacobian, of a fired step FallbackMap.dense() and 0.0; where the
    twin without the map has NaN rows there are none; rollout_gradient is PlantMap.backprop on that J and is finite."""
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    # (the warm-started handles of test_rollout_jacobian's capped cases: under the smallest iteration count of the uncapped rollout some
    # steps stop at the cap with MAXIT -- a cold step that misses its cap by a pass ends OPTIMAL_INACC, whose Jacobian is still finite)
    (A, ref, plain), fm, theta0, w, T, B, iters0 = RJ._capped_handles(3)
    cap = int(iters0.min())
    for g in (A, ref, plain):
        g.set_settings(iter_max=cap)
    fb = _fbmap(K, NR, seed=6)
    A.set_fallback_map(fb)
    got = A.rollout_jacobian(theta0, T, w)
    assert A.last_rollout_launches() == (1 if not env else T)
    want, fired = _host_loop(ref, fm, fb, theta0, T, w, jac=True)
    print("MPC02", env, "cap", cap, "codes", want[2].tolist(), "fired", fired.astype(int).tolist())
    for q, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), (env, ("u", "theta", "exitcodes", "iters", "J", "res")[q])
    u, th, codes, iters, J, res = got
    assert fired.any() and not fired.all()
    assert np.array_equal(J[fired], np.broadcast_to(fb.dense(K), (int(fired.sum()), NR, K))) and not res[fired].any()
    assert np.all(np.isfinite(J)) and np.all(np.isfinite(res))
    Jp, resp = plain.rollout_jacobian(theta0, T, w)[4:]
    assert np.isnan(Jp).any() and np.isnan(resp).any()  # (the same rollout without the map does record NaN rows)
    assert fired[np.isnan(Jp).any(axis=(2, 3))[:, 0], 0].all()  # (step 0 is the same step on both: where it has NaN rows the law fired)
    # (the KKT values hold the scaling block, which an adjoint leaves as scratch: a fired last step ran none, the twin's param_jacobian did)
    got_state, want_state = _state(A, kkt=True), _state(ref, kkt=True)
    _assert_rows({k_: v for k_, v in got_state.items() if k_ != "kkt"}, {k_: v for k_, v in want_state.items() if k_ != "kkt"}, range(B),
                 ("MPC02", env, "final state"))
    _assert_rows(got_state, want_state, np.nonzero(~fired[:, -1])[0], ("MPC02", env, "final state of the instances whose last step did not fire"))
    rng = np.random.default_rng(5)
    gu, gth = rng.standard_normal(u.shape), rng.standard_normal(th.shape)
    g0, gw = A.rollout_gradient(gu, gth)
    w0, ww = fm.backprop(J, gu, gth)
    assert np.array_equal(g0, w0) and np.array_equal(gw, ww) and np.all(np.isfinite(g0)) and np.all(np.isfinite(gw))
    assert np.array_equal(A.fallback_counts(), fired.sum(axis=1))
    for g in (A, ref, plain):
        g.close()


@pytest.mark.gpu
def test_multi_forms_match_one_handle(monkeypatch):
    """Case 8: two shards on device 0, batch 8, global ids."""
    name, B, T = "MPC02", 8, 2
    pat, theta, oi, cap, both, (one,) = _case(name, B, {}, None, monkeypatch, handles=1)
    d = P._data(name, B)[1]
    pm, om, fm, fb = P._map(d, K), _omap(pat.n, NR), RO._fmap(K, NR), _fbmap(K, NR, seed=7)
    m = eicos_amd.MultiBatchSolver(pat, B, [0, 0])
    m.update(*[d[k_] for k_ in KEYS])
    m.set_param_map(pm); m.set_output_map(om); m.set_settings(iter_max=cap)
    for g in (one, m):
        g.set_plant_map(fm)
        g.set_fallback_map(fb)
    assert m.fallback_mask() == NOT_OPTIMAL
    um, uo = np.full((B, NR), np.nan), np.full((B, NR), np.nan)
    cm, co = m.update_param_solve(theta.copy(), u_out=um), one.update_param_solve(theta.copy(), u_out=uo)
    f = _fired(co, fb.mask)
    assert both and 0 < f.sum() < B and f[:4].any() and f[4:].any(), (co, oi.tolist())  # (fired instances on both shards)
    assert np.array_equal(um, uo) and np.array_equal(cm, co) and np.array_equal(um[f], fb.evaluate(theta)[f])
    assert np.array_equal(m.fallback_counts(), one.fallback_counts()) and np.array_equal(m.fallback_counts(), f.astype(np.int32))
    w = RO._w(B, T, K)
    RO._assert_rollout(m.rollout(theta, T, w), one.rollout(theta, T, w), (name, "multi rollout"))
    assert np.array_equal(m.fallback_counts(reset=True), one.fallback_counts(reset=True))
    assert not m.fallback_counts().any()
    m.set_fallback_map(None)
    assert m.fallback_mask() == 0
    m.close(); one.close()


@pytest.mark.gpu
def test_refusals_change_nothing(monkeypatch):
    """Case 9."""
    name, B = "MPC02", 4
    pat, theta, oi, cap, both, (g, bare) = _case(name, B, {}, None, monkeypatch)
    fb = _fbmap(K, NR, seed=8)
    L = binding._lib()

    def refused(h, f, mask, match):
        _keep, ptr = binding._affine_ptr((f.base, f.rowptr, f.col, f.val), f.r, "", "")
        before = h.fallback_mask()
        assert L.eicos_batch_set_fallback_map(h._h, mask, ptr) == -1
        assert match in L.eicos_last_error().decode(), L.eicos_last_error()
        assert h.fallback_mask() == before

    # no parameter map, no output map
    bare.set_output_map(None)
    refused(bare, fb, NOT_OPTIMAL, "no output map")
    bare.set_param_map(None)
    refused(bare, fb, NOT_OPTIMAL, "no parameter map")
    with pytest.raises(RuntimeError, match="no parameter map"):
        bare.set_fallback_map(fb)
    # a column outside [0, k), bits beyond SEL_ALL, SEL_UNSOLVED alone; with a map installed, which stays
    g.set_fallback_map(fb)
    bad = _fbmap(K, NR, seed=8)
    bad.col = bad.col.copy()
    bad.col[-1] = K
    refused(g, bad, NOT_OPTIMAL, "outside [0, k)")
    refused(g, fb, eicos_amd.SEL_ALL + 1, "mask has bits above")
    refused(g, fb, eicos_amd.SEL_UNSOLVED, "EICOS_SEL_UNSOLVED alone")
    bad = _fbmap(K, NR, seed=8)
    bad.rowptr = bad.rowptr.copy()
    bad.rowptr[0] = 1
    refused(g, bad, NOT_OPTIMAL, "rowptr[0] must be 0")
    u = np.full((B, NR), np.nan)
    g.update_param_solve(theta.copy(), u_out=u)  # (the installed map still works)
    assert np.all(np.isfinite(u)) and g.fallback_counts().any()
    # rollout_gradient after set_fallback_map: the recorded Jacobians belong to the maps they ran under
    g.set_plant_map(RO._fmap(K, NR))
    T = 2
    out = g.rollout_jacobian(theta, T)
    gu = np.ones(out[0].shape)
    g.rollout_gradient(gu)
    g.set_fallback_map(_fbmap(K, NR, seed=9))
    with pytest.raises(RuntimeError, match="fallback map was installed after"):
        g.rollout_gradient(gu)
    g.rollout_jacobian(theta, T)
    g.rollout_gradient(gu)
    g.set_fallback_map(None)
    with pytest.raises(RuntimeError, match="fallback map was installed after"):
        g.rollout_gradient(gu)
    # a step after the parameter map was replaced with another k
    g.set_fallback_map(fb)
    d = P._data(name, B)[1]
    g.set_param_map(P._map(d, K + 1))
    state = _state(g)
    with pytest.raises(RuntimeError, match="install it again"):
        g.update_param_solve(P._theta(B, K + 1), u_out=u)
    with pytest.raises(RuntimeError, match="install it again"):
        g.update_param_solve_subset([1, 0], P._theta(2, K + 1))
    _assert_rows(_state(g), state, range(B), "a refused step")
    g.close(); bare.close()
