"""Rollout sensitivities: eicos_batch_rollout_jacobian, eicos_batch_rollout_gradient / _device, their eicos_multi_* forms and
PlantMap.backprop (include/eicos_amd.h).

rollout_jacobian is rollout() that also records J_t = d u_t / d theta_t of every step while the step's iterate is still in place; the
contract is bit-identity with the HOST TWIN -- per step update_param_solve, param_jacobian, the plant map on the host -- in every
returned array and in the handle's state afterwards, and with plain rollout() in everything rollout() returns.  rollout_gradient is a
backward sweep over the recorded Jacobians in a fixed order; PlantMap.backprop is its host restatement, bit for bit.  Every comparison
with the twin is np.array_equal.  Two tests go against finite differences, with the project's bound of test_adjoint*.py: 1e-3 of the
largest finite-difference entry (central differences at eps = 1e-4 of solves converged to 1e-8 carry noise of about 1e-4).

Measured (docs/HISTORY.md A.24): CPU, the numpy reference through PlantMap.backprop against the oracle's central difference of the
closed loop at T = 3: max |grad - grad_fd| 4.35e-6 at max |grad_fd| 33.3 and 8.97e-7 at 115.3 (bound 1e-3 of the latter); on one
MI355X, rollout_gradient against central differences of plain rollouts: the same figures to three digits, res 2.2e-15."""
import ctypes as C

import numpy as np
import pytest

import eicos_amd
from eicos_amd import binding
from eicos_amd.binding import PlantMap
import test_param_update as P
import test_rhs_update as R
import test_rollout as RO
import test_matrix_param as MM
import test_warm_shift as WS
import test_adjoint as AD
import test_adjoint_matrix as AM
from test_param_step import _omap

KEYS = R.KEYS
DP = C.POINTER(C.c_double)
IP = C.POINTER(C.c_int)
NAMES = ("u", "theta", "exitcodes", "iters", "J", "res")
FD_T = 3


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------
def _dense_plant(fm):
    """F [k, k + r] dense; repeated columns add up."""
    F = np.zeros((fm.k, fm.k + fm.r))
    for row in range(fm.k):
        np.add.at(F[row], fm.col[fm.rowptr[row]:fm.rowptr[row + 1]], fm.val[fm.rowptr[row]:fm.rowptr[row + 1]])
    return F


def _dense_chain(fm, J, gu, gth):
    """The gradient by the dense chain Phi_t = F_theta + F_u J_t: lambda_t = gth_t + J_t' gu_t + Phi_t' lambda_{t+1}."""
    F = _dense_plant(fm)
    Ft, Fu = F[:, :fm.k], F[:, fm.k:]
    B, T = J.shape[:2]
    g0, gw = np.zeros((B, fm.k)), np.zeros((B, T, fm.k))
    for b in range(B):
        lam = gth[b, T].copy()
        for t in range(T - 1, -1, -1):
            gw[b, t] = lam
            lam = gth[b, t] + J[b, t].T @ gu[b, t] + (Ft + Fu @ J[b, t]).T @ lam
        g0[b] = lam
    return g0, gw


def _fd_plant(k, r, seed=31):
    """The plant map of the finite-difference case: dense, small base and small entries on u, so that theta stays at the size of the
    case's theta rows (a few 1e-3) over the steps while F_u J_t stays comparable to F_theta (J is of the order 100 there)."""
    rng = np.random.default_rng(seed)
    rowptr = np.arange(0, k * (k + r) + 1, k + r).astype(np.int32)
    col = np.tile(np.arange(k + r), k).astype(np.int32)
    val = np.where(col < k, rng.uniform(-0.5, 0.5, col.size), rng.uniform(-2e-3, 2e-3, col.size))
    return PlantMap(k, r, (rng.uniform(-5e-3, 5e-3, k), rowptr, col, val))


def _fd_gu(B, T, r):
    return np.random.default_rng(77).uniform(0.5, 1.5, (B, T, r)) * np.random.default_rng(78).choice([-1.0, 1.0], (B, T, r))


def _host_loop_jac(ref, fm, theta0, T, w):
    """The host twin: T times update_param_solve on pinned theta and u, param_jacobian, the plant map on the host.  Returns u_traj,
    theta_traj, exitcodes, iters, J, res in the layout of rollout_jacobian()."""
    B, k = theta0.shape
    pth, pu = eicos_amd.PinnedArray((B, k)), eicos_amd.PinnedArray((B, fm.r))
    th, thetas, us, codes, iters, Js, ress = theta0.copy(), [theta0.copy()], [], [], [], [], []
    for t in range(T):
        pth.a[...] = th
        pu.a[...] = np.nan
        codes.append(np.asarray(ref.update_param_solve(pth.a, u_out=pu.a)).copy())
        iters.append(ref.info_arrays()["iter"].copy())
        J, res = ref.param_jacobian()
        Js.append(J); ress.append(res)
        us.append(pu.a.copy())
        th = fm.evaluate(th, us[-1], None if w is None else w[:, t])
        thetas.append(th)
    pth.close(); pu.close()
    return (np.stack(us, axis=1), np.stack(thetas, axis=1), np.stack(codes, axis=1), np.stack(iters, axis=1), np.stack(Js, axis=1),
            np.stack(ress, axis=1))


class _ShiftedTwin(WS._ShiftedHost):
    def param_jacobian(self):
        return self.ref.param_jacobian()


def _assert_six(got, want, what, n=6):
    for q, (a, b) in enumerate(zip(got[:n], want[:n])):
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), (what, NAMES[q])


def _same_handles(g, ref, B, what):
    R._assert_same(R._outputs(g, RO._final_codes(g)), R._outputs(ref, RO._final_codes(ref)), what)
    assert np.array_equal(g.retry_counts(), ref.retry_counts()), what
    assert np.array_equal(g.debug_kkt(B - 1)[2], ref.debug_kkt(B - 1)[2], equal_nan=True), what


def _compare(name, B, k, r, T, with_w, build=None, prepare=None, launches=None, full_rows=0, matrix=False, shift=None, third=True):
    """Three handles in the same state: one takes rollout_jacobian(), one the host twin, one plain rollout().  Returns (got, handle)
    after the comparisons; the caller closes nothing."""
    pat, d = P._data(name, B)
    pm, om, fm = P._map(d, k, full_rows=full_rows), _omap(pat.n, r), RO._fmap(k, r)
    mm = MM._mmap(d, k) if matrix else None
    sm = WS._smap(pat) if shift else None
    g, ref = P._twins(pat, d, B)
    hs = [g, ref] + (P._twins(pat, d, B)[:1] if third else [])
    if build is not None:
        assert (g.kernel_build(), g.dims()["threads_per_block"]) == build, (g.kernel_build(), g.dims()["threads_per_block"])
    for s in hs:
        if prepare:
            prepare(s)
        s.set_param_map(pm); s.set_output_map(om)
        if mm is not None:
            s.set_matrix_map(mm)
    for s in [g] + hs[2:]:
        s.set_plant_map(fm)
        if sm is not None:
            s.set_shift_map(sm)
    theta0, w = P._theta(B, k), (RO._w(B, T, k) if with_w else None)
    want = _host_loop_jac(_ShiftedTwin(ref, sm) if sm is not None else ref, fm, theta0, T, w)
    got = g.rollout_jacobian(theta0, T, w)
    what = (name, B, k, r, T, with_w, matrix, bool(shift))
    if launches is None and g.dims()["lds_bytes"] > 0:
        launches = 1
    if launches is not None:
        assert g.last_rollout_launches() == launches, (what, g.last_rollout_launches())
    _assert_six(got, want, what)
    _same_handles(g, ref, B, what)
    if third:
        plain = hs[2].rollout(theta0, T, w)
        _assert_six(got, plain, what, n=4)
        R._assert_same(R._outputs(g, RO._final_codes(g)), R._outputs(hs[2], RO._final_codes(hs[2])), what)
        hs[2].close()
    ref.close()
    return got, g, fm


# ---- CPU --------------------------------------------------------------------------------------------------------------------------------
def test_rollout_sensitivity_entry_points_exist_and_refuse_a_null_handle():
    L = binding._lib()
    dp = np.zeros(4).ctypes.data_as(DP)
    err = L.eicos_last_error
    for rc in (L.eicos_batch_rollout_jacobian(None, 1, dp, None, dp, None, None, None, dp, None), L.eicos_batch_rollout_gradient(None, dp, None, dp, None),
               L.eicos_batch_rollout_gradient_device(None, None, None, None, None), L.eicos_batch_rollout_jacobian_steps(None)):
        assert rc == -1 and b"NULL handle" in err()
    err = L.eicos_multi_last_error
    for rc in (L.eicos_multi_rollout_jacobian(None, 1, dp, None, dp, None, None, None, dp, None), L.eicos_multi_rollout_gradient(None, dp, None, dp, None)):
        assert rc == -1 and b"NULL handle" in err()
    for f in ("rollout_jacobian", "rollout_gradient"):
        assert callable(getattr(eicos_amd.BatchSolver, f)) and callable(getattr(eicos_amd.MultiBatchSolver, f))


def test_arrays_of_the_wrong_shape_are_refused_before_the_library_is_called():
    B, T, k, r = 3, 2, 4, 2
    fm = RO._fmap(k, r)
    J = np.zeros((B, T, r, k))
    for bad in (np.zeros((B, T, r, k + 1)), np.zeros((B, T, r + 1, k)), np.zeros((B, T * r, k))):
        with pytest.raises(ValueError):
            fm.backprop(bad, gu=np.zeros((B, T, r)))
    with pytest.raises(ValueError):
        fm.backprop(J)  # both cotangents missing
    for gu, gth in ((np.zeros((B, T + 1, r)), None), (np.zeros((B, T, r + 1)), None), (None, np.zeros((B, T, k))), (None, np.zeros((B + 1, T + 1, k)))):
        with pytest.raises(ValueError):
            fm.backprop(J, gu=gu, gtheta=gth)

    class Probe(binding._Solver):  # (a solver object whose library call would raise something else: the checks stand in front of it)
        batch, _rollout_shape = B, (T, k, r)

        def _call(self, name, *a):
            raise AssertionError("the library was called: " + name)

        def param_count(self):
            return k

        def output_count(self):
            return r

    for bad in (np.zeros((B, k + 1)), np.zeros((B + 1, k))):
        with pytest.raises(ValueError):
            Probe().rollout_jacobian(bad, T)
    with pytest.raises(ValueError):
        Probe().rollout_jacobian(np.zeros((B, k)), T, w=np.zeros((B, T + 1, k)))
    with pytest.raises(ValueError):
        Probe().rollout_gradient(gu=np.zeros((B, T + 1, r)))
    with pytest.raises(ValueError):
        Probe().rollout_gradient(gtheta=np.zeros((B, T, k)))
    with pytest.raises(AssertionError, match="rollout_gradient"):  # (well-shaped arrays do reach the library)
        Probe().rollout_gradient(gu=np.zeros((B, T, r)))


def test_backprop_against_the_dense_chain():
    # sums of at most k + r terms of O(1) values in fp64: 1e-12 relative
    k, r, T, B = 5, 4, 3, 3
    rng = np.random.default_rng(3)
    fm = RO._fmap(k, r, seed=9)
    fm = PlantMap(k, r, (fm.base, fm.rowptr, fm.col, rng.uniform(-1, 1, fm.col.size)))
    J, gu, gth = rng.standard_normal((B, T, r, k)), rng.standard_normal((B, T, r)), rng.standard_normal((B, T + 1, k))
    zu, zt = np.zeros_like(gu), np.zeros_like(gth)
    both, only_u, only_t = fm.backprop(J, gu, gth), fm.backprop(J, gu=gu), fm.backprop(J, gtheta=gth)
    for got, want in ((both, _dense_chain(fm, J, gu, gth)), (only_u, _dense_chain(fm, J, gu, zt)), (only_t, _dense_chain(fm, J, zu, gth))):
        for a, b in zip(got, want):
            assert a.shape == b.shape and np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(b)), np.max(np.abs(a - b))
    for q in range(2):  # linearity: the two halves add up to the whole
        assert np.max(np.abs(only_u[q] + only_t[q] - both[q])) <= 1e-12 * np.max(np.abs(both[q]))
    # a missing cotangent is 0.0 that is still added: the same bits as an array of zeros
    for a, b in zip(only_u, fm.backprop(J, gu, zt)):
        assert np.array_equal(a, b)
    # a NaN row of J reaches grad_theta0
    Jn = J.copy(); Jn[1, 0] = np.nan
    g0, _ = fm.backprop(Jn, gu, gth)
    assert np.all(np.isnan(g0[1])) and np.all(np.isfinite(g0[[0, 2]]))


def _fd_setup():
    pat, pmap, mmap, omap, theta = AM._fd_case()
    return pat, pmap, mmap, omap, theta, _fd_plant(AM.K, AM.R), _fd_gu(theta.shape[0], FD_T, AM.R)


def _oracle_rollout(pat, pmap, mmap, omap, fm, theta0, T, jac):
    """The closed loop on the CPU oracle; jac: J_t from the numpy reference of test_adjoint.py as well."""
    U = AD._csr_dense((omap.base, omap.rowptr, omap.col, omap.val), pat.n)
    maps = AM._dense_maps(pat, pmap, mmap)
    B = theta0.shape[0]
    th, us, Js = theta0.copy(), [], []
    for t in range(T):
        u, J = np.zeros((B, AM.R)), np.zeros((B, AM.R, AM.K))
        for i, v in enumerate(AM._fd_values(pmap, mmap, th)):
            code, x, y, z, s = AD._oracle_x(pat, v)
            assert code == 0, (t, i, code)
            u[i] = omap.evaluate(x[None, :])[0]
            if jac:
                ref = AD._Reference(pat, v, s, z)
                assert ref.cond <= AD.COND_MAX, (t, i, ref.cond)
                J[i] = U @ AM._reference_columns(pat, ref, maps, x, y, z)[: pat.n]
        us.append(u); Js.append(J)
        th = fm.evaluate(th, u)
    return np.stack(us, axis=1), np.stack(Js, axis=1)


def test_the_reference_stays_within_the_bound_of_the_gpu_finite_difference_case():
    """The end-to-end GPU test asks 1e-3 max|grad_fd| of the library; here the numpy reference's J_t through PlantMap.backprop alone
    against the oracle's central difference of the closed loop, T = 3.  Measured: max |grad - grad_fd| 4.35e-6 at max |grad_fd|
    33.3 (instance 0) and 8.97e-7 at 115.3 (instance 1), max |J| 110.6: three and five hundred times inside the bound."""
    pat, pmap, mmap, omap, theta, fm, gu = _fd_setup()
    B = theta.shape[0]
    _, J = _oracle_rollout(pat, pmap, mmap, omap, fm, theta, FD_T, True)
    grad, _ = fm.backprop(J, gu=gu)
    fd = np.zeros((B, AM.K))
    for c in range(AM.K):
        e = np.zeros(AM.K); e[c] = AM.FD_EPS
        up, _ = _oracle_rollout(pat, pmap, mmap, omap, fm, theta + e, FD_T, False)
        um, _ = _oracle_rollout(pat, pmap, mmap, omap, fm, theta - e, FD_T, False)
        fd[:, c] = ((up - um) * gu).sum(axis=(1, 2)) / (2.0 * AM.FD_EPS)
    for i in range(B):
        dist, scale = np.max(np.abs(grad[i] - fd[i])), np.max(np.abs(fd[i]))
        print("instance", i, "max |grad - grad_fd|", dist, "max |grad_fd|", scale, "max |J|", np.max(np.abs(J[i])))
        assert dist <= 1e-3 * scale, (i, dist, scale)


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case,name,B,k,r,T", [
    (0, "MPC02", 40, 7, 6, 3),
    (1, "MPC02", 600, 16, 4, 2),
    (2, "lp_afiro", 16, 1, 3, 3),
    (3, "issue98", 8, 5, 2, 3),
    (4, "socp-random", 8, 5, 5, 3),
    (5, "dense-front", 6, 3, 4, 3),
])
def test_rollout_jacobian_is_bit_identical_to_the_host_twin(case, name, B, k, r, T):
    _, g, _ = _compare(name, B, k, r, T, with_w=case % 2 == 1)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,env,build", [
    ("MPC02", 4, {"EICOS_UBL": "0", "EICOS_THREADS": "256"}, ("w2", 256)),
    ("MPC02", 4, {"EICOS_UBL": "0", "EICOS_THREADS": "256", "EICOS_W2": "0"}, ("default", 256)),
    ("MPC02", 4, {"EICOS_UBL": "0", "EICOS_W2": "0", "EICOS_THREADS": "128"}, ("default", 128)),
    ("MPC02", 4, {"EICOS_UBL": "0", "EICOS_W2": "0", "EICOS_THREADS": "512"}, ("default", 512)),
    ("issue98", 4, {"EICOS_THREADS": "256"}, ("u-in-lds", 256)),
    ("lp_bandm", 96, {}, ("u-in-lds", 512)),
    ("lp_afiro", 4, {}, ("lds-resident", 128)),
])
def test_rollout_jacobian_on_every_build_of_the_solve_kernel(name, B, env, build, monkeypatch):
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    _, g, _ = _compare(name, B, 5, 4, 2, with_w=True, build=build, launches=1)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,k,env", [
    ("MPC02", 40, 7, {"EICOS_FUSED_UPDATE": "0"}),
    ("MPC02", 40, 7, {"EICOS_NLDS": "0", "EICOS_DUAL": "0"}),
    ("lp_afiro", 5, 1100, {}),
])
def test_rollout_jacobian_without_the_fused_path_gives_the_same_bits(name, B, k, env, monkeypatch):
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    T = 3
    _, g, _ = _compare(name, B, k, 4, T, with_w=True, launches=T, full_rows=2)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("env,launches", [({}, 1), ({"EICOS_FUSED_UPDATE": "0"}, 2)])
def test_rollout_jacobian_under_a_matrix_map(env, launches, monkeypatch):
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    _, g, _ = _compare("MPC02", 8, 7, 6, 2, with_w=True, launches=launches, matrix=True)
    g.close()


@pytest.mark.gpu
def test_rollout_jacobian_with_warm_start_and_a_shift_map():
    # step t + 1 reads the slab step t left behind -- and nothing the adjoint of step t left
    def warm(s):
        assert (np.asarray(s.info_arrays()["exitcode"]) == 0).all()
        s.set_warm_start(0.1)

    _, g, _ = _compare("MPC02", 40, 7, 6, 3, with_w=True, prepare=warm, launches=1, shift=True)
    g.close()
    _, g, _ = _compare("MPC02", 40, 7, 6, 3, with_w=True, prepare=warm, launches=1)
    g.close()


def _capped_handles(n):
    """n warm-started MPC02 handles with the maps of test_inlaunch_retry's rollout case, and the iteration counts of the uncapped rollout."""
    name, B, K, NR, T = "MPC02", 4, 7, 6, 3
    pat, d = P._data(name, B)
    pm, om, fm = P._map(d, K), _omap(pat.n, NR), RO._fmap(K, NR)
    theta0, w = P._theta(B, K), RO._w(B, T, K)
    hs = []
    for _ in range(n + 1):
        g = eicos_amd.BatchSolver(pat, B)
        g.update(*[d[k_] for k_ in KEYS])
        assert (g.solve() == 0).all()
        g.set_param_map(pm); g.set_output_map(om); g.set_plant_map(fm)
        g.set_warm_start(0.1)
        hs.append(g)
    iters0 = hs[-1].rollout(theta0, T, w)[3]
    hs[-1].close()
    assert iters0.min() < iters0.max(), iters0
    return hs[:-1], fm, theta0, w, T, B, iters0


@pytest.mark.gpu
def test_rollout_jacobian_under_a_retry_policy():
    (A, ref), fm, theta0, w, T, B, iters0 = _capped_handles(2)
    cap = int(iters0.min())
    for g in (A, ref):
        g.set_settings(iter_max=cap)
        g.set_retry(eicos_amd.SEL_NOT_OPTIMAL)
    got = A.rollout_jacobian(theta0, T, w)
    assert A.last_rollout_launches() == 1
    # the twin, with its retried steps counted per step
    seen, per_step = np.zeros(B, np.int32), []

    class Counting:
        def update_param_solve(self, *a, **kw):
            out = ref.update_param_solve(*a, **kw)
            c = ref.retry_counts()
            per_step.append(c - seen); seen[...] = c
            return out

        def info_arrays(self):
            return ref.info_arrays()

        def param_jacobian(self):
            return ref.param_jacobian()

    want = _host_loop_jac(Counting(), fm, theta0, T, w)
    steps = np.stack(per_step, axis=1)
    print("uncapped iterations", iters0.tolist(), "cap", cap, "retried steps", steps.tolist())
    assert steps.any() and not steps.all(), steps  # at least one step retries and at least one does not
    _assert_six(got, want, "retry")
    _same_handles(A, ref, B, "retry")
    assert np.array_equal(A.retry_counts(), steps.sum(axis=1))
    A.close(); ref.close()


@pytest.mark.gpu
def test_a_step_that_is_not_optimal_gets_nan_rows_and_the_loop_goes_on():
    (A, ref), fm, theta0, w, T, B, iters0 = _capped_handles(2)
    cap = int(iters0.min())
    for g in (A, ref):
        g.set_settings(iter_max=cap)
    got = A.rollout_jacobian(theta0, T, w)
    want = _host_loop_jac(ref, fm, theta0, T, w)
    u, th, codes, iters, J, res = got
    ok = (codes == 0) | (codes == 10)
    print("uncapped iterations", iters0.tolist(), "cap", cap, "codes", codes.tolist())
    assert ok.any() and (~ok).any(), codes  # some but not all steps end at the cap
    _assert_six(got, want, "cap")
    _same_handles(A, ref, B, "cap")
    assert np.all(np.isnan(J[~ok])) and np.all(np.isnan(res[~ok])) and np.all(np.isfinite(u))  # NaN rows; the step keeps its u row
    assert np.all(np.isfinite(J[ok])) and np.all(np.isfinite(res[ok]))  # steps of other instances, and later steps, are unaffected
    rng = np.random.default_rng(5)
    gu, gth = rng.standard_normal(u.shape), rng.standard_normal(th.shape)
    g0, gw = A.rollout_gradient(gu, gth)
    w0, ww = fm.backprop(want[4], gu, gth)
    assert np.array_equal(g0, w0, equal_nan=True) and np.array_equal(gw, ww, equal_nan=True)
    bad = ~ok.all(axis=1)
    assert np.all(np.isnan(g0[bad]).any(axis=1)) and np.all(np.isfinite(g0[~bad])) and np.all(np.isfinite(gw[~bad]))
    A.close(); ref.close()


@pytest.mark.gpu
def test_rollout_gradient_is_bit_identical_to_backprop():
    got, g, fm = _compare("MPC02", 40, 7, 6, 3, with_w=True, launches=1, third=False)
    u, th, J = got[0], got[1], got[4]
    rng = np.random.default_rng(11)
    gu, gth = rng.standard_normal(u.shape), rng.standard_normal(th.shape)
    for a, b in ((gu, None), (None, gth), (gu, gth)):
        want = fm.backprop(J, a, b)
        for dev in (False, True):
            have = g.rollout_gradient(a, b, device=dev)
            assert np.array_equal(have[0], want[0]) and np.array_equal(have[1], want[1]), (a is None, b is None, dev)
    assert np.all(np.isfinite(want[0])) and np.abs(want[0]).max() > 0
    g.close()


@pytest.mark.gpu
def test_rollout_gradient_against_finite_differences_of_plain_rollouts():
    pat, pmap, mmap, omap, theta, fm, gu = _fd_setup()
    B, T = theta.shape[0], FD_T
    g = eicos_amd.BatchSolver(pat, B)
    vs = AM._fd_values(pmap, mmap, theta)
    g.update(*[np.stack([getattr(v, k) for v in vs]) for k in AD.KEYS])
    AM._install(g, pmap, mmap, omap)
    g.set_plant_map(fm)

    def loss(th0):
        u, _, codes, _ = g.rollout(th0, T)
        assert np.all(codes == 0), codes  # every instance qualifies: all its steps OPTIMAL on every run
        return (u * gu).sum(axis=(1, 2))

    fd = np.zeros((B, AM.K))
    for c in range(AM.K):
        e = np.zeros(AM.K); e[c] = AM.FD_EPS
        fd[:, c] = (loss(theta + e) - loss(theta - e)) / (2.0 * AM.FD_EPS)
    out = g.rollout_jacobian(theta, T)
    assert np.all(out[2] == 0), out[2]
    grad, _ = g.rollout_gradient(gu=gu)
    for i in range(B):
        dist, scale = np.max(np.abs(grad[i] - fd[i])), np.max(np.abs(fd[i]))
        print("instance", i, "max |grad - grad_fd|", dist, "max |grad_fd|", scale, "res", out[5][i].max())
        assert dist <= 1e-3 * scale, (i, dist, scale)
    g.close()


@pytest.mark.gpu
def test_refusals_move_nothing():
    B, k, r, T = 4, 3, 4, 2
    pat, d = P._data("lp_afiro", B)
    g = eicos_amd.BatchSolver(pat, B)
    g.update(*[d[k_] for k_ in KEYS]); g.solve()
    L = binding._lib()
    err = lambda: L.eicos_last_error().decode()
    pm, om, fm = P._map(d, k), _omap(pat.n, r), RO._fmap(k, r)
    theta0 = P._theta(B, k)
    u, J = np.zeros((B, T, r)), np.zeros((B, T, r, k))
    gu, gth, g0, gw = np.ones((B, T, r)), np.ones((B, T + 1, k)), np.zeros((B, k)), np.zeros((B, T, k))
    p = lambda a: None if a is None else a.ctypes.data_as(DP)

    def roll(steps=T, th=theta0, out=u, jac=J):
        return L.eicos_batch_rollout_jacobian(g._h, steps, p(th), None, p(out), None, None, None, p(jac), None)

    def grad(a=gu, b=gth, o=g0, ow=gw):
        return L.eicos_batch_rollout_gradient(g._h, p(a), p(b), p(o), p(ow))

    before = AD._state(g)
    assert roll() == -1 and "no parameter map" in err()
    g.set_param_map(pm)
    assert roll() == -1 and "no output map" in err()
    g.set_output_map(om)
    assert roll() == -1 and "no plant map" in err()
    assert grad() == -1 and "no Jacobian trajectory" in err()  # a gradient before any rollout_jacobian
    with pytest.raises(RuntimeError, match="no Jacobian trajectory"):
        g.rollout_gradient(gu=gu)
    g.set_plant_map(fm)
    assert roll(steps=0) == -1 and "steps" in err()
    assert roll(out=None) == -1 and "u_traj is NULL" in err()
    assert roll(th=None) == -1 and "theta0 is NULL" in err()
    assert roll(jac=None) == -1 and "J_traj is NULL" in err()
    assert grad() == -1 and "no Jacobian trajectory" in err()
    AD._assert_same(AD._state(g), before, "after the refusals of rollout_jacobian")
    assert roll() == 0 and g.last_rollout_launches() in (1, T)
    after = AD._state(g)
    assert grad() == 0
    assert grad(a=None, b=None) == -1 and "both NULL" in err()
    assert grad(o=None) == -1 and "grad_theta0 is NULL" in err()
    dev = AM._device_doubles(gth.size)
    dptr, vptr = C.cast(dev, DP), C.c_void_p(gu.ctypes.data)
    assert L.eicos_batch_rollout_gradient(g._h, dptr, p(gth), p(g0), None) == -1 and "host pointers" in err()
    assert L.eicos_batch_rollout_gradient(g._h, p(gu), None, dptr, None) == -1 and "host pointers" in err()
    assert L.eicos_batch_rollout_gradient_device(g._h, vptr, None, dev, None) == -1 and "device memory" in err()
    assert L.eicos_batch_rollout_gradient_device(g._h, dev, None, vptr, None) == -1 and "device memory" in err()
    L.hipFree(dev)
    # a map installed after the rollout: the trajectory no longer belongs to the handle's maps
    g.set_plant_map(fm)
    assert grad() == -1 and "installed after the rollout" in err()
    assert roll() == 0 and grad() == 0
    g.set_param_map(pm)
    assert grad() == -1 and "installed after the rollout" in err()
    # a matrix map that does not fit the parameter map
    g.set_matrix_map(MM._mmap(d, k, groups="G"))
    g.set_param_map(P._map(d, k, groups="cb"))  # (no h group: updateData reads h with Gpr)
    assert roll() == -1 and "matrix map of G" in err()
    g.set_matrix_map(None); g.set_param_map(pm)
    AD._assert_same(AD._state(g), after, "after the refusals of rollout_gradient")
    g.close()


@pytest.mark.gpu
def test_two_rollout_jacobians_chain_into_one():
    B, k, r = 40, 7, 6
    pat, d = P._data("MPC02", B)
    pm, om, fm = P._map(d, k), _omap(pat.n, r), RO._fmap(k, r)
    g, ref = P._twins(pat, d, B)
    for s in (g, ref):
        s.set_param_map(pm); s.set_output_map(om); s.set_plant_map(fm)
    theta0, w = P._theta(B, k), RO._w(B, 4, k)
    whole = ref.rollout_jacobian(theta0, 4, w)
    a = g.rollout_jacobian(theta0, 2, w[:, :2])
    b = g.rollout_jacobian(a[1][:, -1], 2, w[:, 2:])
    joined = [np.concatenate((x, y), axis=1) for x, y in zip(a, b)]
    joined[1] = np.concatenate((a[1], b[1][:, 1:]), axis=1)
    _assert_six(joined, whole, "2 + 2 against 4")
    _same_handles(g, ref, B, "2 + 2 against 4")
    g.close(); ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("devs", [[0, 0], [0, 0, 0]])
def test_multi_forms_match_one_handle(devs):
    B, k, r, T = 5, 7, 6, 3
    pat, d = P._data("MPC02", B)
    pm, om, fm = P._map(d, k), _omap(pat.n, r), RO._fmap(k, r)
    eicos_amd.set_arithmetic_profile(1)
    try:
        one = eicos_amd.BatchSolver(pat, B)
        m = eicos_amd.MultiBatchSolver(pat, B, devs)
        for s in (one, m):
            s.update(*[d[k_] for k_ in KEYS]); s.solve()
            s.set_param_map(pm); s.set_output_map(om); s.set_plant_map(fm)
        theta0, w = P._theta(B, k), RO._w(B, T, k)
        want = one.rollout_jacobian(theta0, T, w)
        got = m.rollout_jacobian(theta0, T, w)
        _assert_six(got, want, devs)
        rng = np.random.default_rng(2)
        gu, gth = rng.standard_normal(want[0].shape), rng.standard_normal(want[1].shape)
        for a, b in ((gu, None), (gu, gth)):
            for x, y in zip(m.rollout_gradient(a, b), one.rollout_gradient(a, b)):
                assert np.array_equal(x, y), devs
        y, z, s = m.duals(); ia = m.info_arrays()
        R._assert_same([ia["exitcode"], m.solution(), y, z, s] + [ia[k_] for k_ in R.INFO_KEYS], R._outputs(one, RO._final_codes(one)), devs)
        m.close(); one.close()
    finally:
        eicos_amd.set_arithmetic_profile(0)
