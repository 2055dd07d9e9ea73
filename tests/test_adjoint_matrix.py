"""Adjoint sensitivities with respect to the matrix data (eicos_batch_adjoint_data, _param_jacobian / _device, _param_gradient / _device
and their eicos_multi_* forms; include/eicos_amd.h): the gradient of g'x with respect to the stored values of G and A,

    grad_G[e] = grad_c[j] z[i] - grad_h[i] x[j],      grad_A[e] = grad_c[j] y[i] - grad_b[i] x[j]      for the stored value e = (i, j),

and the derivative with respect to theta through whichever of the parameter map and the matrix map are installed.

The yardsticks are those of test_adjoint.py, whose helpers are imported: the numpy _Reference (dense K of the definition, LAPACK) and the
CPU oracle's central differences.  The CPU tests pin the formula (sign, index, transposes) against the oracle; the GPU tests pin every
stored value against the GPU's own vector gradients (which test_adjoint.py holds to 1e-8 of the reference), compare with the dense
reference, check the contracted forms against the host contraction of the gradient form, and take one case end to end against finite
differences of GPU solves under the matrix map.

Measured (docs/HISTORY.md A.22): CPU, formula against the oracle's central difference 2e-10 ... 3.2e-6 relative (bound 1e-3), all five
maps combined 2e-11 ... 5.2e-6; on one MI355X, dense parity of grad_G / grad_A 4e-16 ... 2.5e-12 against bounds of 4e-8 ... 6e-6,
Jacobian under a matrix map 3e-16 ... 2.5e-14 from the reference (bounds 6e-9 ... 2.5e-6), end to end 4.8e-6 and 1.8e-7 from the
central difference of GPU solves at max |J_fd| 110.6 (bound 0.11)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse

import eicos_amd
from eicos_amd import binding
from eicos_amd.binding import MatrixMap, OutputMap, ParamMap
from eicos_amd.problem_io import Values
from test_adjoint import (COND_MAX, EPS, ITER_CAP, KEYS, PARITY, _Reference, _assert_same, _csr_dense, _data, _handle, _oracle_x, _random_maps,
                          _random_rows, _setenv, _state, _vals)
from test_matrix_param import _mcsr

K, R = 3, 2


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------
def _cols(jc):
    """Column of every stored value of a CSC pattern."""
    return np.repeat(np.arange(jc.size - 1), np.diff(jc))


def _formula(pat, grads, x, y, z):
    """(grad_G, grad_A) [nrhs, nnz] of the definition from (grad_c, grad_h, grad_b) [nrhs, .] and one instance's x, y, z."""
    gc, gh, gb = grads
    Gi, Gj, Ai, Aj = pat.Gir, _cols(pat.Gjc), pat.Air, _cols(pat.Ajc)
    return gc[:, Gj] * z[Gi] - gh[:, Gi] * x[Gj], gc[:, Aj] * y[Ai] - gb[:, Ai] * x[Aj]


def _sp(pat, which, vals):
    if which == "G":
        return scipy.sparse.csc_matrix((vals, pat.Gir, pat.Gjc), shape=(pat.m, pat.n))
    return scipy.sparse.csc_matrix((vals, pat.Air, pat.Ajc), shape=(pat.p, pat.n))


def _matrix_map(pat, Gpr, Apr, k=K, seed=21):
    """The matrix map of a case: bases Gpr / Apr, rows from test_matrix_param._mcsr (values about 1e-3 of the base)."""
    rng = np.random.default_rng(seed)
    return MatrixMap(k, G=_mcsr(rng, Gpr, k), A=_mcsr(rng, Apr, k) if pat.nnzA else None)


def _dense_maps(pat, pmap, mmap, k=K):
    """(C [n, k], H [m, k], B [p, k], M_G [nnzG, k], M_A [nnzA, k]) dense; a group that is not mapped is zero."""
    Cm = _csr_dense(pmap.c, k) if pmap is not None and pmap.c is not None else np.zeros((pat.n, k))
    Hm = _csr_dense(pmap.h, k) if pmap is not None and pmap.h is not None else np.zeros((pat.m, k))
    Bm = _csr_dense(pmap.b, k) if pmap is not None and pmap.b is not None else np.zeros((pat.p, k))
    MG = _csr_dense(mmap.G, k) if mmap is not None and mmap.G is not None else np.zeros((pat.nnzG, k))
    MA = _csr_dense(mmap.A, k) if mmap is not None and mmap.A is not None else np.zeros((pat.nnzA, k))
    return Cm, Hm, Bm, MG, MA


def _host_contraction(five, maps):
    """(sum of the five products, sum of their absolute terms, number of terms per column) for gradients [rows, .] of one instance."""
    val = sum(g @ M for g, M in zip(five, maps))
    mag = sum(np.abs(g) @ np.abs(M) for g, M in zip(five, maps))
    nnz = np.maximum(1, sum((M != 0).sum(0) for M in maps))
    return val, mag, nnz


def _reference_columns(pat, ref, maps, x, y, z):
    """K^-1 [-C - dA'y - dG'z; B - dA x; H - dG x], column t along theta_t: d(x, y, z) / d theta from the numpy reference."""
    Cm, Hm, Bm, MG, MA = maps
    cols = []
    for t in range(Cm.shape[1]):
        dG, dA = _sp(pat, "G", MG[:, t]), _sp(pat, "A", MA[:, t])
        cols.append(np.concatenate([-Cm[:, t] - dA.T @ y - dG.T @ z, Bm[:, t] - dA @ x, Hm[:, t] - dG @ x]))
    return ref.solve(np.stack(cols, axis=1))


def _oracle_fd_matrix(pat, v, g, dG, dA, dc, dh, db, eps=1e-5):
    """Central difference of g'x of the oracle's solution along (dG, dA, dc, dh, db), default settings."""
    xs = []
    for sg in (1.0, -1.0):
        code, x, *_ = _oracle_x(pat, Values(v.Gpr + sg * eps * dG, v.Apr + sg * eps * dA, v.c + sg * eps * dc, v.h + sg * eps * dh, v.b + sg * eps * db))
        assert code == 0, code
        xs.append(x)
    return g @ (xs[0] - xs[1]) / (2.0 * eps)


# ---- CPU: the definition ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lp_afiro", "lp_blend", "vertex-small", "vertex-mid"])
def test_matrix_gradient_formula_is_the_derivative_of_the_oracle(name):
    # sign-and-formula check: a wrong sign, index or transpose is an O(1) error; the bound is the 1e-3 of test_adjoint.py
    pat, d = _data(name, 2)
    for i in range(2):
        v = _vals(d, i)
        code, x, y, z, s = _oracle_x(pat, v)
        assert code == 0
        ref = _Reference(pat, v, s, z)
        assert ref.cond <= COND_MAX, (name, i, ref.cond)
        rng = np.random.default_rng(2000 + i)
        g = rng.standard_normal(pat.n)
        dG, dA = rng.standard_normal(pat.nnzG) * np.abs(v.Gpr), rng.standard_normal(pat.nnzA) * np.abs(v.Apr)
        want = _oracle_fd_matrix(pat, v, g, dG, dA, 0.0, 0.0, 0.0)
        gG, gA = _formula(pat, ref.grads(g[None, :]), x, y, z)
        got = gG[0] @ dG + gA[0] @ dA
        rel = abs(got - want) / abs(want)
        print(name, i, "cond", ref.cond, "formula", got, "central difference", want, "relative distance", rel)
        assert rel <= 1e-3, (name, i, got, want)


@pytest.mark.parametrize("name", ["lp_afiro", "lp_blend", "vertex-small", "vertex-mid"])
def test_combined_directional_derivative_under_all_five_maps(name):
    pat, d = _data(name, 2)
    pmap, _ = _random_maps(pat, K, R)
    for i in range(2):
        v = _vals(d, i)
        mmap = _matrix_map(pat, v.Gpr, v.Apr)
        maps = _dense_maps(pat, pmap, mmap)
        code, x, y, z, s = _oracle_x(pat, v)
        assert code == 0
        ref = _Reference(pat, v, s, z)
        assert ref.cond <= COND_MAX, (name, i, ref.cond)
        rng = np.random.default_rng(3000 + i)
        g, dth = rng.standard_normal(pat.n), rng.standard_normal(K)
        Cm, Hm, Bm, MG, MA = maps
        want = _oracle_fd_matrix(pat, v, g, MG @ dth, MA @ dth, Cm @ dth, Hm @ dth, Bm @ dth)
        got = g @ (_reference_columns(pat, ref, maps, x, y, z)[: pat.n] @ dth)
        rel = abs(got - want) / abs(want)
        print(name, i, "cond", ref.cond, "reference", got, "central difference", want, "relative distance", rel)
        assert rel <= 1e-3, (name, i, got, want)


def test_new_entry_points_exist_and_refuse_a_null_handle():
    L = binding._lib()
    for prefix, err in (("eicos_batch_", L.eicos_last_error), ("eicos_multi_", L.eicos_multi_last_error)):
        calls = [("adjoint_data", (None, None, 1, 1, None, None, None, None, None, None, None)), ("param_jacobian", (None, None, 1, None, None)),
                 ("param_gradient", (None, None, 1, 1, None, None, None)), ("matrix_map_count", (None,))]
        if prefix == "eicos_batch_":
            calls += [("param_jacobian_device", (None, None, 1, None, None)), ("param_gradient_device", (None, None, 1, 1, None, None, None))]
        for name, args in calls:
            assert hasattr(L, prefix + name), prefix + name
            assert getattr(L, prefix + name)(*args) == -1 and b"NULL handle" in err(), prefix + name


# ---- the finite-difference case of the GPU test, first on the CPU ---------------------------------------------------------------------
FD_EPS = 1e-4


def _fd_case():
    """vertex-small, two instances on instance 1's data as the bases of all five maps, at two different small theta rows."""
    pat, d = _data("vertex-small", 2)
    v = _vals(d, 1)
    pm, omap = _random_maps(pat, K, R, seed=12)
    pmap = ParamMap(K, c=(v.c.copy(),) + tuple(pm.c[1:]), h=(v.h.copy(),) + tuple(pm.h[1:]), b=(v.b.copy(),) + tuple(pm.b[1:]))
    mmap = _matrix_map(pat, v.Gpr, v.Apr, seed=22)
    theta = np.array([[8e-3, -5e-3, 3e-3], [-6e-3, 9e-3, -2e-3]])
    return pat, pmap, mmap, omap, theta


def _fd_values(pmap, mmap, theta):
    (G, A), (c, h, b) = mmap.evaluate(theta), pmap.evaluate(theta)
    return [Values(G[i], A[i], c[i], h[i], b[i]) for i in range(theta.shape[0])]


def test_the_reference_stays_within_the_bound_of_the_gpu_finite_difference_case():
    # the end-to-end GPU test asks 1e-3 max|J_fd| of the library; here the numpy reference alone against the oracle's central difference
    pat, pmap, mmap, omap, theta = _fd_case()
    U = _csr_dense((omap.base, omap.rowptr, omap.col, omap.val), pat.n)
    maps = _dense_maps(pat, pmap, mmap)
    for i, v in enumerate(_fd_values(pmap, mmap, theta)):
        code, x, y, z, s = _oracle_x(pat, v)
        assert code == 0
        ref = _Reference(pat, v, s, z)
        assert ref.cond <= COND_MAX, (i, ref.cond)
        J = U @ _reference_columns(pat, ref, maps, x, y, z)[: pat.n]
        Jfd = np.zeros((R, K))
        for t in range(K):
            us = []
            for sg in (1.0, -1.0):
                th = theta[i:i + 1].copy(); th[0, t] += sg * FD_EPS
                code, xp, *_ = _oracle_x(pat, _fd_values(pmap, mmap, th)[0])
                assert code == 0
                us.append(U @ xp)
            Jfd[:, t] = (us[0] - us[1]) / (2.0 * FD_EPS)
        dist = np.max(np.abs(J - Jfd))
        print("instance", i, "cond", ref.cond, "max |J - J_fd|", dist, "max |J_fd|", np.max(np.abs(Jfd)))
        assert dist <= 1e-3 * np.max(np.abs(Jfd)), (i, dist)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------
def _parity_handle(name, B, env, build, monkeypatch):
    _setenv(monkeypatch, env)
    if name == "u-in-lds":
        for name in ("lp_adlittle", "lp_blend"):
            pat, d = _data(name, B)
            g = eicos_amd.BatchSolver(pat, B)
            if g.kernel_build() == "u-in-lds":
                break
            g.close()
        assert (g.kernel_build(), g.dims()["threads_per_block"]) == build
        g.update(*[d[k] for k in KEYS])
        return name, pat, d, g
    pat, d = _data(name, B)
    return name, pat, d, _handle(pat, d, B, build)


def _assert_sampled(what, got, a, u, b, v):
    """|got - (a u - b v)| <= 4 EPS (|a u| + |b v|) elementwise: two rounded products and a rounded difference, or a fused form of them."""
    want, mag = a * u - b * v, np.abs(a * u) + np.abs(b * v)
    bad = np.abs(got - want) > 4.0 * EPS * mag
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4], np.abs(got - want)[bad][:4], mag[bad][:4])


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,env,build,check", PARITY)
def test_matrix_gradients_are_the_sampled_outer_product_on_every_build(name, B, env, build, check, monkeypatch):
    name, pat, d, g = _parity_handle(name, B, env, build, monkeypatch)
    codes = g.solve()
    assert np.all(codes == 0), codes
    rows = _random_rows(pat, B, 2)
    gc0, gh0, gb0, res0 = g.adjoint(rows)
    gc, gh, gb, gG, gA, res = g.adjoint_data(rows)
    assert gG.shape == (B, 2, pat.nnzG) and gA.shape == (B, 2, pat.nnzA)
    for a, b in zip((gc0, gh0, gb0, res0), (gc, gh, gb, res)):
        assert np.array_equal(a, b)
    x, (y, z, s) = g.solution(), g.duals()
    Gi, Gj, Ai, Aj = pat.Gir, _cols(pat.Gjc), pat.Air, _cols(pat.Ajc)
    for i in range(B):
        _assert_sampled((name, i, "grad_G"), gG[i], gc[i][:, Gj], z[i][Gi], gh[i][:, Gi], x[i][Gj])
        _assert_sampled((name, i, "grad_A"), gA[i], gc[i][:, Aj], y[i][Ai], gb[i][:, Ai], x[i][Aj])
    L, dp = binding._lib(), C.POINTER(C.c_double)
    only = np.zeros_like(gc)  # grad_G == grad_A == NULL: eicos_batch_adjoint
    assert L.eicos_batch_adjoint_data(g._h, None, B, 2, rows.ctypes.data_as(dp), only.ctypes.data_as(dp), None, None, None, None, None) == 0
    assert np.array_equal(only, gc0)
    g.close()


_REFS = {}  # (name, instance) -> (s, z, _Reference) at the iterate a handle returned: one dense factorisation per iterate


def _reference_at(pat, d, name, i, s, z):
    hit = _REFS.get((name, i))
    if hit is None or not (np.array_equal(hit[0], s) and np.array_equal(hit[1], z)):
        hit = _REFS[(name, i)] = (s.copy(), z.copy(), _Reference(pat, _vals(d, i), s, z))
    assert hit[2].cond <= COND_MAX, (name, i, hit[2].cond)
    return hit[2]


THREE = [PARITY[0], PARITY[1], PARITY[9]]  # LDS-resident, two-wave, cones


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,env,build,check", THREE)
def test_matrix_gradients_match_the_dense_reference(name, B, env, build, check, monkeypatch):
    name, pat, d, g = _parity_handle(name, B, env, build, monkeypatch)
    assert np.all(g.solve() == 0)
    rows = _random_rows(pat, B, 2)
    gc, gh, gb, gG, gA, res = g.adjoint_data(rows)
    x, (y, z, s) = g.solution(), g.duals()
    for i in (range(B) if check is None else check):
        ref = _reference_at(pat, d, name, i, s[i], z[i])
        wc, wh, wb = ref.grads(rows[i])
        wG, wA = _formula(pat, (wc, wh, wb), x[i], y[i], z[i])
        amax = lambda a: np.max(np.abs(a), initial=0.0)
        for r in range(2):
            bG = 1e-8 * (amax(wc[r]) * amax(z[i]) + amax(wh[r]) * amax(x[i]))
            bA = 1e-8 * (amax(wc[r]) * amax(y[i]) + amax(wb[r]) * amax(x[i]))
            dG, dA = amax(gG[i, r] - wG[r]), amax(gA[i, r] - wA[r])
            print(name, "instance", i, "row", r, "grad_G distance", dG, "bound", bG, "grad_A distance", dA, "bound", bA, "cond", ref.cond)
            assert dG <= bG and dA <= bA, (name, i, r, dG, bG, dA, bA)
    g.close()


def _install(g, pmap, mmap, omap):
    g.set_param_map(pmap)
    g.set_matrix_map(mmap)
    g.set_output_map(omap)


def _within_order_bound(got, five, maps, what):
    host, mag, nnz = _host_contraction(five, maps)
    bound = 4.0 * nnz * EPS * mag
    assert np.all(np.abs(got - host) <= bound), (what, np.abs(got - host).max(), bound.min())
    return mag


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,env,build,check", THREE)
def test_param_jacobian_under_a_matrix_map(name, B, env, build, check, monkeypatch):
    name, pat, d, g = _parity_handle(name, B, env, build, monkeypatch)
    pmap, omap = _random_maps(pat, K, R)
    mmap = _matrix_map(pat, d["Gpr"][0], d["Apr"][0])
    _install(g, pmap, mmap, omap)
    assert np.all(g.solve() == 0)
    U = _csr_dense((omap.base, omap.rowptr, omap.col, omap.val), pat.n)
    maps = _dense_maps(pat, pmap, mmap)
    urows = np.broadcast_to(U, (B, R, pat.n)).copy()
    J, res = g.param_jacobian()
    Jd, resd = g.param_jacobian(device=True)
    assert J.shape == (B, R, K) and np.all(np.isfinite(res))
    assert np.array_equal(J, Jd) and np.array_equal(res, resd)  # the device form: the same bits
    *five, res2 = g.adjoint_data(urows)
    assert np.array_equal(res, res2)  # (the same right-hand sides through the same solve)
    mags = [_within_order_bound(J[i], [a[i] for a in five], maps, (name, i, "all five")) for i in range(B)]
    x, (y, z, s) = g.solution(), g.duals()
    for i in (range(B) if check is None else check):
        ref = _reference_at(pat, d, name, i, s[i], z[i])
        want = U @ _reference_columns(pat, ref, maps, x[i], y[i], z[i])[: pat.n]
        dist, T = np.max(np.abs(J[i] - want)), np.max(mags[i])
        print(name, "instance", i, "max |J - ref|", dist, "T", T, "max |J|", np.max(np.abs(want)))
        assert dist <= 1e-8 * T, (name, i, dist, T)
    # param_gradient: the rows of U give the bits of the Jacobian; random rows the contraction of their gradients; the device form the same bits
    gt, gres = g.param_gradient(urows)
    assert np.array_equal(gt, J) and np.array_equal(gres, res)
    rows = _random_rows(pat, B, 2)
    gt, gres = g.param_gradient(rows)
    gtd, gresd = g.param_gradient(rows, device=True)
    assert gt.shape == (B, 2, K) and np.array_equal(gt, gtd) and np.array_equal(gres, gresd)
    *rfive, rres = g.adjoint_data(rows)
    assert np.array_equal(gres, rres)
    for i in range(B):
        _within_order_bound(gt[i], [a[i] for a in rfive], maps, (name, i, "param_gradient"))
    # the matrix map alone: the matrix terms alone
    g.set_param_map(None)
    assert g.param_count() == 0 and g.matrix_map_count() == K
    Jm, resm = g.param_jacobian()
    assert np.array_equal(resm, res)
    for i in range(B):
        _within_order_bound(Jm[i], [a[i] for a in five[3:]], maps[3:], (name, i, "matrix terms alone"))
    gtm, _ = g.param_gradient(rows)
    for i in range(B):
        _within_order_bound(gtm[i], [a[i] for a in rfive[3:]], maps[3:], (name, i, "param_gradient, matrix terms alone"))
    # without the matrix map: the bits of output_jacobian
    g.set_param_map(pmap)
    g.set_matrix_map(None)
    J0, res0 = g.output_jacobian()
    J1, res1 = g.param_jacobian()
    assert np.array_equal(J0, J1) and np.array_equal(res0, res1)
    for i in range(B):
        _within_order_bound(J1[i], [a[i] for a in five[:3]], maps[:3], (name, i, "vector terms alone"))
    g.close()


@pytest.mark.gpu
def test_param_jacobian_against_finite_differences_of_gpu_solves():
    pat, pmap, mmap, omap, theta = _fd_case()
    B = theta.shape[0]
    g = eicos_amd.BatchSolver(pat, B)
    vs = _fd_values(pmap, mmap, theta)
    g.update(*[np.stack([getattr(v, k) for v in vs]) for k in KEYS])
    _install(g, pmap, mmap, omap)

    def step(th):
        u = np.zeros((B, R))
        codes = g.update_param_solve(th, u_out=u)
        assert np.all(codes == 0), codes
        return u

    Jfd = np.zeros((B, R, K))
    for t in range(K):
        e = np.zeros(K); e[t] = FD_EPS
        Jfd[:, :, t] = (step(theta + e) - step(theta - e)) / (2.0 * FD_EPS)
    step(theta)
    J, res = g.param_jacobian()
    for i in range(B):
        dist, scale = np.max(np.abs(J[i] - Jfd[i])), np.max(np.abs(Jfd[i]))
        print("instance", i, "max |J - J_fd|", dist, "max |J_fd|", scale, "res", res[i])
        assert dist <= 1e-3 * scale, (i, dist, scale)
    g.close()


def _device_doubles(count):
    hip = binding._lib()
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), 8 * count) == 0
    return p


@pytest.mark.gpu
def test_ineligible_instances_list_forms_refusals_and_nothing_moves():
    B, name = 8, "MPC02"
    pat, d = _data(name, B)
    g = _handle(pat, d, B)
    g.set_settings(iter_max=ITER_CAP)
    codes = g.solve()
    ok = (codes == 0) | (codes == 10)
    assert ok.any() and (~ok).any(), codes  # (the cap is chosen so that the batch splits)
    before = _state(g)
    L, ip, dp = binding._lib(), C.POINTER(C.c_int), C.POINTER(C.c_double)
    err = lambda: L.eicos_last_error().decode()
    width = max(pat.n, pat.m, pat.nnzG, pat.nnzA)
    hbuf = np.zeros(B * 2 * width)
    buf = hbuf.ctypes.data_as(dp)
    dev = _device_doubles(B * 2 * width)
    dbuf, vbuf = C.cast(dev, dp), C.c_void_p(hbuf.ctypes.data)
    ids = lambda v: np.asarray(v, np.int32).ctypes.data_as(ip)
    # without any map
    assert L.eicos_batch_param_jacobian(g._h, None, B, buf, None) != 0 and "output map" in err()
    assert L.eicos_batch_param_gradient(g._h, None, B, 1, buf, buf, None) != 0 and "parameter map or a matrix map" in err()
    pmap, omap = _random_maps(pat, K, R)
    g.set_output_map(omap)
    assert L.eicos_batch_param_jacobian(g._h, None, B, buf, None) != 0 and "parameter map or a matrix map" in err()
    assert L.eicos_batch_param_jacobian_device(g._h, None, B, dev, None) != 0 and "parameter map or a matrix map" in err()
    g.set_output_map(None)
    g.set_param_map(pmap)
    assert L.eicos_batch_param_jacobian(g._h, None, B, buf, None) != 0 and "output map" in err()
    _install(g, pmap, _matrix_map(pat, d["Gpr"][0], d["Apr"][0]), omap)
    # the list check, nrhs, NULL arrays
    assert L.eicos_batch_adjoint_data(g._h, ids([1, 1]), 2, 1, buf, buf, None, None, buf, None, None) != 0 and "duplicate index 1" in err()
    assert L.eicos_batch_adjoint_data(g._h, ids([1, B]), 2, 1, buf, buf, None, None, buf, None, None) != 0 and "outside" in err()
    assert L.eicos_batch_param_jacobian(g._h, ids([0, 0]), 2, buf, None) != 0 and "duplicate index 0" in err()
    assert L.eicos_batch_param_gradient(g._h, ids([0, B]), 2, 1, buf, buf, None) != 0 and "outside" in err()
    for nrhs in (0, 65):
        assert L.eicos_batch_adjoint_data(g._h, None, B, nrhs, buf, buf, None, None, buf, None, None) != 0 and "nrhs" in err()
        assert L.eicos_batch_param_gradient(g._h, None, B, nrhs, buf, buf, None) != 0 and "nrhs" in err()
        assert L.eicos_batch_param_gradient_device(g._h, None, B, nrhs, dev, dev, None) != 0 and "nrhs" in err()
    assert L.eicos_batch_adjoint_data(g._h, None, B, 1, None, buf, None, None, buf, None, None) != 0 and "g is NULL" in err()
    assert L.eicos_batch_param_jacobian(g._h, None, B, None, None) != 0 and "J is NULL" in err()
    assert L.eicos_batch_param_gradient(g._h, None, B, 1, None, buf, None) != 0 and "g is NULL" in err()
    assert L.eicos_batch_param_gradient(g._h, None, B, 1, buf, None, None) != 0 and "grad_theta is NULL" in err()
    # a pointer of the wrong kind
    assert L.eicos_batch_adjoint_data(g._h, None, B, 1, buf, buf, None, None, dbuf, None, None) != 0 and "host pointers" in err()
    assert L.eicos_batch_param_jacobian(g._h, None, B, dbuf, None) != 0 and "host pointers" in err()
    assert L.eicos_batch_param_jacobian_device(g._h, None, B, vbuf, None) != 0 and "device memory" in err()
    assert L.eicos_batch_param_gradient(g._h, None, B, 1, buf, dbuf, None) != 0 and "host pointers" in err()
    assert L.eicos_batch_param_gradient(g._h, None, B, 1, dbuf, buf, None) != 0 and "host pointers" in err()
    assert L.eicos_batch_param_gradient_device(g._h, None, B, 1, dev, vbuf, None) != 0 and "device memory" in err()
    assert L.eicos_batch_param_gradient_device(g._h, None, B, 1, vbuf, dev, None) != 0 and "device memory" in err()
    assert L.eicos_batch_output_jacobian(g._h, None, B, buf, None) != 0 and "matrix map" in err() and "eicos_batch_param_jacobian" in err()
    _assert_same(_state(g), before, "after the refusals")
    binding._lib().hipFree(dev)
    # NaN rows for the instances at the cap, the others finite; list forms: the bits of the whole-batch rows
    rows = _random_rows(pat, B, 2)
    idx = [B - 1, 0, 3, 2]
    whole = g.adjoint_data(rows)
    _assert_same(_state(g), before, "after adjoint_data")
    for a in whole:
        assert np.all(np.isnan(a[~ok])) and np.all(np.isfinite(a[ok]))
    for a, w in zip(g.adjoint_data(rows[idx], idx=idx), whole):
        assert np.array_equal(a, w[idx], equal_nan=True)
    for call, args in ((g.param_jacobian, ()), (g.param_gradient, (rows,))):
        whole = call(*args)
        _assert_same(_state(g), before, "after " + call.__name__)
        for a in whole:
            assert np.all(np.isnan(a[~ok])) and np.all(np.isfinite(a[ok]))
        sub = call(*[a[idx] for a in args], idx=idx)
        for a, w in zip(sub, whole):
            assert np.array_equal(a, w[idx], equal_nan=True)
        for a, w in zip(call(*args, device=True), whole):
            assert np.array_equal(a, w, equal_nan=True)
    _assert_same(_state(g), before, "after every new call")
    g.close()


@pytest.mark.gpu
def test_multi_forms_equal_the_single_handle():
    B, name = 5, "lp_afiro"
    pat, d = _data(name, 8)
    d = {k: v[:B] for k, v in d.items()}
    pmap, omap = _random_maps(pat, K, R)
    mmap = _matrix_map(pat, d["Gpr"][0], d["Apr"][0])
    eicos_amd.set_arithmetic_profile(1)  # (plans by the pattern alone: a shard gives the bits of the batch)
    try:
        single = eicos_amd.BatchSolver(pat, B)
        multi = eicos_amd.MultiBatchSolver(pat, B, [0, 0])
    finally:
        eicos_amd.set_arithmetic_profile(0)
    for g in (single, multi):
        g.update(*[d[k] for k in KEYS])
        _install(g, pmap, mmap, omap)
        assert np.all(g.solve() == 0)
    rows = _random_rows(pat, B, 2)
    idx = [4, 1, 2]
    for call, args in (("adjoint_data", (rows,)), ("param_jacobian", ()), ("param_gradient", (rows,))):
        want = getattr(single, call)(*args)
        for a, b in zip(want, getattr(multi, call)(*args)):
            assert a.size and np.array_equal(a, b), call
        for a, b in zip(want, getattr(multi, call)(*[v[idx] for v in args], idx=idx)):
            assert np.array_equal(a[idx], b), call
    for g in (single, multi):
        g.close()
