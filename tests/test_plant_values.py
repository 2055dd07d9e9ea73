"""Per-instance plant values and the gradient with respect to the plant's entries: eicos_batch_set_plant_values / _device,
_plant_values, _has_plant_values, _clear_plant_values, _rollout_plant_gradient / _device, their eicos_multi_* forms, and
PlantMap.evaluate(f0=, val=) / backprop(val=) / backprop_values (include/eicos_amd.h).

A handle with a plant map may hold, per instance, rows of its own in the place of the map's base (f0_i [batch][k]) and of its stored
values (val_i [batch][nnzF]); the pattern stays shared.  Every rollout form then runs instance i against its own plant with exactly the
arithmetic of the shared map, so the contract stays bit-identity: rollout() equals the host loop of update_param_solve with the plant
evaluated per instance on the host, rollout_jacobian() its host twin, rollout_gradient() PlantMap.backprop(val=), and
rollout_plant_gradient() PlantMap.backprop_values on all four arrays.  Every comparison is np.array_equal, except the two
finite-difference checks:

  * CPU, backprop_values against central differences (eps = 1e-6) of a numpy closed loop under a linear law u = u0 + K theta (J_t = K
    exactly): the loss is a polynomial of degree T in a plant entry, so the central difference is exact up to eps^2 times a third
    derivative of order one (1e-12) and the rounding of the loss, about 1e-15 |L| / eps = 1e-9 absolute at |L| of a few; the bound is
    1e-8 max|grad|.  Measured: 2.4e-11 ... 1.5e-9 of max|grad| (the largest where max|grad| is below one).
  * the closed loop of test_rollout_jacobian's finite-difference case with per-instance plants, on the CPU oracle (calibration) and
    through the library on the GPU: 1e-3 max|grad_fd| per instance, the bound of the existing gradient test (central differences at
    eps = 1e-4 of solves converged to 1e-8 carry noise of about 1e-4).  Measured on the CPU oracle: see
    test_the_reference_stays_within_the_bound_of_the_gpu_plant_gradient_case."""
import ctypes as C

import numpy as np
import pytest

import eicos_amd
from eicos_amd import binding
from eicos_amd.binding import PlantMap
import test_param_update as P
import test_rhs_update as R
import test_rollout as RO
import test_rollout_jacobian as RJ
import test_adjoint as AD
import test_adjoint_matrix as AM
from test_param_step import _omap

KEYS = R.KEYS
DP = C.POINTER(C.c_double)
FD_VALS, FD_ROWS = (0, 2, 3, 4, 6, 14), (0, 2)  # the stored values and f0 rows the two closed-loop finite-difference checks visit


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------
def _values(fm, B, seed=0):
    """Per-instance rows of a map: its base and stored values, each scaled within +-10 %, another factor per instance and entry."""
    rng = np.random.default_rng(6000 + seed)
    return fm.base[None, :] * rng.uniform(0.9, 1.1, (B, fm.k)), fm.val[None, :] * rng.uniform(0.9, 1.1, (B, fm.nnz()))


class _Plant:
    """A PlantMap with per-instance rows bound, in the place of the map in the host loops of test_rollout / test_rollout_jacobian."""

    def __init__(self, fm, f0=None, val=None):
        self.fm, self.f0, self.val, self.k, self.r = fm, f0, val, fm.k, fm.r

    def evaluate(self, theta, u, w=None):
        return self.fm.evaluate(theta, u, w, f0=self.f0, val=self.val)


def _setup(name, B, k, r, n_handles=2, full_rows=0, prepare=None):
    pat, d = P._data(name, B)
    pm, om, fm = P._map(d, k, full_rows=full_rows), _omap(pat.n, r), RO._fmap(k, r)
    hs = []
    while len(hs) < n_handles:
        hs += P._twins(pat, d, B)
    for extra in hs[n_handles:]:
        extra.close()
    hs = hs[:n_handles]
    for s in hs:
        if prepare:
            prepare(s)
        s.set_param_map(pm); s.set_output_map(om); s.set_plant_map(fm)
    return pat, fm, hs


def _same_state(g, ref, B, what):
    R._assert_same(R._outputs(g, RO._final_codes(g)), R._outputs(ref, RO._final_codes(ref)), what)
    assert np.array_equal(g.debug_kkt(B - 1)[2], ref.debug_kkt(B - 1)[2], equal_nan=True), what


def _compare_rollout(name, B, k, r, T, with_w, groups="fv", build=None, launches=None, full_rows=0, device=False):
    """Twin handles: one holds per-instance values and takes rollout(), the other the host loop with the plant evaluated per instance."""
    pat, fm, (g, ref) = _setup(name, B, k, r, full_rows=full_rows)
    if build is not None:
        assert (g.kernel_build(), g.dims()["threads_per_block"]) == build, (g.kernel_build(), g.dims()["threads_per_block"])
    f0, val = _values(fm, B)
    f0, val = (f0 if "f" in groups else None), (val if "v" in groups else None)
    assert g.has_plant_values() == 0
    g.set_plant_values(f0=f0, val=val, device=device)
    assert g.has_plant_values() == (1 if f0 is not None else 0) | (2 if val is not None else 0)
    theta0, w = P._theta(B, k), (RO._w(B, T, k) if with_w else None)
    want = RO._host_loop(ref, _Plant(fm, f0, val), theta0, T, w)
    got = g.rollout(theta0, T, w)
    what = (name, B, k, r, T, with_w, groups)
    if launches is None and g.dims()["lds_bytes"] > 0:
        launches = 1
    if launches is not None:
        assert g.last_rollout_launches() == launches, (what, g.last_rollout_launches())
    RO._assert_rollout(got, want, what)
    _same_state(g, ref, B, what)
    # ... and the values made a difference: the shared plant gives other theta rows
    assert not np.array_equal(got[1], RO._host_loop(ref, fm, theta0, T, w)[1]), what
    g.close(); ref.close()
    return got


# ---- CPU --------------------------------------------------------------------------------------------------------------------------------
def test_plant_value_entry_points_exist_and_refuse_a_null_handle():
    L = binding._lib()
    dp = np.zeros(4).ctypes.data_as(DP)
    err = L.eicos_last_error
    for rc in (L.eicos_batch_set_plant_values(None, 0, 1, dp, None), L.eicos_batch_set_plant_values_device(None, 0, 1, None, None),
               L.eicos_batch_plant_values(None, 0, 1, dp, None), L.eicos_batch_has_plant_values(None), L.eicos_batch_clear_plant_values(None),
               L.eicos_batch_rollout_plant_gradient(None, dp, None, dp, dp, dp, None, None, None),
               L.eicos_batch_rollout_plant_gradient_device(None, None, None, None, None, None, None, None, None)):
        assert rc == -1 and b"NULL handle" in err()
    err = L.eicos_multi_last_error
    for rc in (L.eicos_multi_set_plant_values(None, 0, 1, dp, None), L.eicos_multi_plant_values(None, 0, 1, dp, None),
               L.eicos_multi_has_plant_values(None), L.eicos_multi_clear_plant_values(None),
               L.eicos_multi_rollout_plant_gradient(None, dp, None, dp, dp, dp, None, None, None)):
        assert rc == -1 and b"NULL handle" in err()
    listed = {full for full, _, _ in binding._SIGNATURES}
    for f in ("set_plant_values", "plant_values", "has_plant_values", "clear_plant_values", "rollout_plant_gradient"):
        assert {"eicos_batch_" + f, "eicos_multi_" + f} <= listed, f
        assert callable(getattr(eicos_amd.BatchSolver, f)) and callable(getattr(eicos_amd.MultiBatchSolver, f))
    assert {"eicos_batch_set_plant_values_device", "eicos_batch_rollout_plant_gradient_device"} <= listed


def _scalar_case():
    """The map of test_plant_map_evaluate_equals_a_scalar_loop_in_the_stated_order, with other values per instance."""
    k, r = 4, 2
    base = np.array([0.1, -2.5, 3.0, 1e-3])
    rowptr = np.array([0, 4, 4, 5, 9], np.int32)
    col = np.array([5, 0, 3, 4, 1, 4, 2, 4, 1], np.int32)  # (row 1 is empty; rows 0 and 3 are not sorted; row 3 holds column 4 twice)
    val = np.array([1 / 3, 1e-7, -0.7, 0.9, 2 / 7, 1e10, 0.3, -1e10, 1 / 7])
    theta = np.array([[0.1, 0.7, 1 / 9, 0.3], [0.9, 0.7, 0.123456789, -0.2]])
    u = np.array([[1 / 3, -0.6], [2.5, 1 / 11]])
    w = np.array([[1e-3, 1 / 7, -0.5, 1e-9], [0.25, -1 / 3, 0.0, 3.0]])
    f0 = np.array([[0.3, -2.0, 1 / 3, 2e-3], [-0.1, 7.5, 3.0, 1 / 13]])
    vals = np.stack((val * np.array([1.1, 0.9, 1 / 3, 1.0, -1.0, 1.0, 3.0, 1.0, 0.5]), val[::-1].copy()))
    return PlantMap(k, r, (base, rowptr, col, val)), theta, u, w, f0, vals


def test_evaluate_with_per_instance_values_equals_a_scalar_loop_in_the_stated_order():
    # acc = f0[i][j]; for s in stored order: acc = acc + (val[i][s] * z[col[s]]); then acc = acc + w[j] -- on Python floats
    fm, theta, u, w, f0, vals = _scalar_case()
    z = np.concatenate((theta, u), axis=1)
    for dist in (None, w):
        for f0_i, val_i in ((f0, vals), (f0, None), (None, vals)):
            got = fm.evaluate(theta, u, dist, f0=f0_i, val=val_i)
            assert got.shape == (2, fm.k)
            for i in range(2):
                for j in range(fm.k):
                    acc = float(fm.base[j] if f0_i is None else f0_i[i, j])
                    for s in range(fm.rowptr[j], fm.rowptr[j + 1]):
                        acc = acc + (float(fm.val[s] if val_i is None else val_i[i, s]) * float(z[i, fm.col[s]]))
                    if dist is not None:
                        acc = acc + float(dist[i, j])
                    assert got[i, j] == acc, (i, j, dist is not None, f0_i is None, val_i is None)


def test_the_broadcast_shared_values_give_the_bits_of_the_plain_calls():
    fm, theta, u, w, _, _ = _scalar_case()
    B = theta.shape[0]
    f0, val = np.repeat(fm.base[None, :], B, axis=0), np.repeat(fm.val[None, :], B, axis=0)
    for dist in (None, w):
        plain = fm.evaluate(theta, u, dist)
        for a, b in ((f0, val), (f0, None), (None, val)):
            got = fm.evaluate(theta, u, dist, f0=a, val=b)
            assert got.shape == plain.shape and np.array_equal(got, plain)
    rng = np.random.default_rng(1)
    T = 3
    J, gu, gth = rng.standard_normal((B, T, fm.r, fm.k)), rng.standard_normal((B, T, fm.r)), rng.standard_normal((B, T + 1, fm.k))
    for a, b in zip(fm.backprop(J, gu, gth, val=val), fm.backprop(J, gu, gth)):
        assert a.shape == b.shape and np.array_equal(a, b)


def test_backprop_with_per_instance_values_equals_plain_backprop_per_instance():
    k, r, T, B = 5, 4, 3, 3
    rng = np.random.default_rng(3)
    fm = RO._fmap(k, r, seed=9)
    _, val = _values(fm, B, seed=2)
    J, gu, gth = rng.standard_normal((B, T, r, k)), rng.standard_normal((B, T, r)), rng.standard_normal((B, T + 1, k))
    for a, b in ((gu, None), (None, gth), (gu, gth)):
        g0, gw = fm.backprop(J, a, b, val=val)
        full = fm.backprop_values(J, rng.standard_normal((B, T, r)), rng.standard_normal((B, T + 1, k)), a, b, val=val)
        assert np.array_equal(full[0], g0) and np.array_equal(full[1], gw)  # (backprop_values returns backprop's bits in front)
        for i in range(B):
            one = PlantMap(k, r, (fm.base, fm.rowptr, fm.col, val[i]))
            w0, ww = one.backprop(J[i:i + 1], None if a is None else a[i:i + 1], None if b is None else b[i:i + 1])
            assert np.array_equal(g0[i], w0[0]) and np.array_equal(gw[i], ww[0]), i
    # a NaN Jacobian of ANY step, step 0 included, makes all of the instance's rows NaN, and only that instance's
    u, th = rng.standard_normal((B, T, r)), rng.standard_normal((B, T + 1, k))
    for t in range(T):
        Jn = J.copy(); Jn[1, t] = np.nan
        _, _, gf0, gval = fm.backprop_values(Jn, u, th, gu, gth, val=val)
        assert np.all(np.isnan(gf0[1])) and np.all(np.isnan(gval[1])), t
        assert np.all(np.isfinite(gf0[[0, 2]])) and np.all(np.isfinite(gval[[0, 2]])), t
        clean = fm.backprop_values(J, u, th, gu, gth, val=val)
        assert np.array_equal(gf0[[0, 2]], clean[2][[0, 2]]) and np.array_equal(gval[[0, 2]], clean[3][[0, 2]])


@pytest.mark.parametrize("k,r,T", [(1, 3, 3), (5, 2, 4), (7, 6, 3), (16, 4, 8)])
def test_backprop_values_against_central_differences_of_a_linear_closed_loop(k, r, T):
    B, eps = 4, 1e-6
    rng = np.random.default_rng(100 * k + r)
    fm = RO._fmap(k, r, seed=k)
    f0, val = _values(fm, B, seed=k)
    K, u0 = rng.uniform(-0.5, 0.5, (r, k)), rng.uniform(-1, 1, r)
    theta0, gu, gth = P._theta(B, k), rng.standard_normal((B, T, r)), rng.standard_normal((B, T + 1, k))

    def loop(f0_, val_):
        th, ths, us = theta0, [theta0], []
        for _ in range(T):
            us.append(u0[None, :] + th @ K.T)
            th = fm.evaluate(th, us[-1], f0=f0_, val=val_)
            ths.append(th)
        u, th = np.stack(us, axis=1), np.stack(ths, axis=1)
        return u, th, (u * gu).sum(axis=(1, 2)) + (th * gth).sum(axis=(1, 2))

    u, th, _ = loop(f0, val)
    J = np.broadcast_to(K, (B, T, r, k))
    _, _, gf0, gval = fm.backprop_values(J, u, th, gu, gth, val=val)
    fd_val, fd_f0 = np.zeros_like(gval), np.zeros_like(gf0)
    for s in range(fm.nnz()):  # (the instances are independent: one perturbed run moves entry s of all of them)
        e = np.zeros(fm.nnz()); e[s] = eps
        fd_val[:, s] = (loop(f0, val + e)[2] - loop(f0, val - e)[2]) / (2.0 * eps)
    for j in range(k):
        e = np.zeros(k); e[j] = eps
        fd_f0[:, j] = (loop(f0 + e, val)[2] - loop(f0 - e, val)[2]) / (2.0 * eps)
    for i in range(B):
        for name, g, fd in (("val", gval[i], fd_val[i]), ("f0", gf0[i], fd_f0[i])):
            dist, scale = np.max(np.abs(g - fd)), np.max(np.abs(g))
            print((k, r, T), "instance", i, name, "max |grad - grad_fd|", dist, "max |grad|", scale, "relative", dist / scale)
            assert scale > 0 and dist <= 1e-8 * scale, (i, name, dist, scale)


def _fd_values(fm, B):
    rng = np.random.default_rng(91)
    return fm.base[None, :] * rng.uniform(0.9, 1.1, (B, fm.k)), fm.val[None, :] * rng.uniform(0.9, 1.1, (B, fm.nnz()))


def test_the_reference_stays_within_the_bound_of_the_gpu_plant_gradient_case():
    """The calibration of the GPU finite-difference test below: on test_rollout_jacobian's finite-difference case with the plant's base
    and values scaled per instance within +-10 %, the numpy reference's J_t through backprop_values against the oracle's central
    differences of the closed loop -- stored values 0, 2, 3, 4, 6, 14 at eps = 1e-4, f0 rows 0, 2 at eps = 1e-6; bound 1e-3 max|grad_fd|
    per instance.  Measured: val, max |grad - grad_fd| 1.2e-7 at max |grad_fd| 95.0 (instance 0) and 1.4e-6 at 186.4 (instance 1); f0, 4.0e-7 at
    306.1 and 1.0e-6 at 132.9: more than two decades inside the bound."""
    pat, pmap, mmap, omap, theta, fm, gu = RJ._fd_setup()
    B, T = theta.shape[0], RJ.FD_T
    assert (B, fm.k, fm.r, fm.nnz()) == (2, 3, 2, 15)
    f0, val = _fd_values(fm, B)

    def loss(f0_, val_, jac=False):
        u, J = RJ._oracle_rollout(pat, pmap, mmap, omap, _Plant(fm, f0_, val_), theta, T, jac)
        return u, J, (u * gu).sum(axis=(1, 2))

    u, J, _ = loss(f0, val, jac=True)
    ths = [theta]
    for t in range(T):
        ths.append(fm.evaluate(ths[-1], u[:, t], f0=f0, val=val))
    _, _, gf0, gval = fm.backprop_values(J, u, np.stack(ths, axis=1), gu=gu, val=val)
    fd_val, fd_f0 = np.zeros((B, len(FD_VALS))), np.zeros((B, len(FD_ROWS)))
    for q, s in enumerate(FD_VALS):
        e = np.zeros(fm.nnz()); e[s] = AM.FD_EPS
        fd_val[:, q] = (loss(f0, val + e)[2] - loss(f0, val - e)[2]) / (2.0 * AM.FD_EPS)
    for q, j in enumerate(FD_ROWS):
        e = np.zeros(fm.k); e[j] = 1e-6
        fd_f0[:, q] = (loss(f0 + e, val)[2] - loss(f0 - e, val)[2]) / (2.0 * 1e-6)
    for i in range(B):
        for name, g, fd in (("val", gval[i, list(FD_VALS)], fd_val[i]), ("f0", gf0[i, list(FD_ROWS)], fd_f0[i])):
            dist, scale = np.max(np.abs(g - fd)), np.max(np.abs(fd))
            print("instance", i, name, "max |grad - grad_fd|", dist, "max |grad_fd|", scale)
            assert dist <= 1e-3 * scale, (i, name, dist, scale)


def test_arrays_of_the_wrong_shape_are_refused_before_the_library_is_called():
    B, T, k, r = 3, 2, 4, 2
    fm = RO._fmap(k, r)
    nnz = fm.nnz()
    th, u, J = np.zeros((B, k)), np.zeros((B, r)), np.zeros((B, T, r, k))
    for f0, val in ((np.zeros((B, k + 1)), None), (np.zeros((B + 1, k)), None), (np.zeros(B * k), None), (None, np.zeros((B, nnz + 1))),
                    (None, np.zeros((B + 1, nnz))), (None, np.zeros(nnz))):
        with pytest.raises(ValueError):
            fm.evaluate(th, u, f0=f0, val=val)
    for val in (np.zeros((B, nnz + 1)), np.zeros((B + 1, nnz)), np.zeros(nnz)):
        with pytest.raises(ValueError):
            fm.backprop(J, gu=np.zeros((B, T, r)), val=val)
        with pytest.raises(ValueError):
            fm.backprop_values(J, np.zeros((B, T, r)), np.zeros((B, T + 1, k)), gu=np.zeros((B, T, r)), val=val)
    for uu, tt in ((np.zeros((B, T + 1, r)), np.zeros((B, T + 1, k))), (np.zeros((B, T, r)), np.zeros((B, T, k))), (None, np.zeros((B, T + 1, k))),
                   (np.zeros((B, T, r)), None)):
        with pytest.raises(ValueError):
            fm.backprop_values(J, uu, tt, gu=np.zeros((B, T, r)))
    with pytest.raises(ValueError):
        fm.backprop_values(J, np.zeros((B, T, r)), np.zeros((B, T + 1, k)))  # both cotangents missing

    class Probe(binding._Solver):  # (a solver object whose library call would raise something else: the checks stand in front of it)
        batch, _rollout_shape, _plant_shape = B, (T, k, r), (k, nnz)

        def _call(self, name, *a):
            raise AssertionError("the library was called: " + name)

        def has_plant_map(self):
            return True

    for kw in ({}, {"f0": np.zeros((B, k + 1))}, {"f0": np.zeros(k)}, {"val": np.zeros((B, nnz - 1))}, {"f0": np.zeros((B, k)), "val": np.zeros((B - 1, nnz))},
               {"f0": np.zeros((B, k)), "first": 1}, {"f0": np.zeros((1, k)), "first": -1}, {"f0": np.zeros((1, k)), "first": B}):
        with pytest.raises(ValueError):
            Probe().set_plant_values(**kw)
    with pytest.raises(AssertionError, match="set_plant_values"):  # (well-shaped rows do reach the library)
        Probe().set_plant_values(f0=np.zeros((2, k)), val=np.zeros((2, nnz)), first=1)
    good = dict(u=np.zeros((B, T, r)), theta=np.zeros((B, T + 1, k)), gu=np.zeros((B, T, r)))
    for bad in ({"u": np.zeros((B, T + 1, r))}, {"theta": np.zeros((B, T, k))}, {"gu": np.zeros((B, T, r + 1))}, {"gu": None}, {"u": None},
                {"gtheta": np.zeros((B, T, k))}):
        with pytest.raises(ValueError):
            Probe().rollout_plant_gradient(**dict(good, **bad))
    with pytest.raises(AssertionError, match="rollout_plant_gradient"):
        Probe().rollout_plant_gradient(**good)


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,B,k,r,T,with_w,groups", [
    ("MPC02", 40, 7, 6, 3, False, "fv"),
    ("MPC02", 600, 16, 4, 2, True, "v"),      # more instances than resident workgroups: a workgroup pulls whole trajectories and indexes by id
    ("lp_afiro", 16, 1, 3, 3, False, "f"),    # the LDS-resident build
    ("issue98", 8, 5, 2, 3, False, "fv"),     # cones
])
def test_rollout_with_plant_values_is_bit_identical_to_the_host_loop(name, B, k, r, T, with_w, groups):
    _compare_rollout(name, B, k, r, T, with_w, groups)


@pytest.mark.gpu
def test_partial_ranges_leave_the_shared_rows_everywhere_else():
    B, k, r, T = 40, 7, 6, 2
    pat, fm, (g, ref) = _setup("MPC02", B, k, r)
    f0, val = _values(fm, B)
    g.set_plant_values(val=val[3:8], first=3)
    assert g.has_plant_values() == 2
    g.set_plant_values(f0=f0[30:40], first=30)
    assert g.has_plant_values() == 3
    want_f0, want_val = np.repeat(fm.base[None, :], B, axis=0), np.repeat(fm.val[None, :], B, axis=0)
    want_f0[30:40], want_val[3:8] = f0[30:40], val[3:8]
    back = g.plant_values()
    assert np.array_equal(back[0], want_f0) and np.array_equal(back[1], want_val)
    part = g.plant_values(first=5, count=28)  # (a range that starts and ends inside the two given ones)
    assert np.array_equal(part[0], want_f0[5:33]) and np.array_equal(part[1], want_val[5:33])
    theta0, w = P._theta(B, k), RO._w(B, T, k)
    got = g.rollout(theta0, T, w)
    assert g.last_rollout_launches() == 1
    RO._assert_rollout(got, RO._host_loop(ref, _Plant(fm, *back), theta0, T, w), "partial ranges")
    _same_state(g, ref, B, "partial ranges")
    # a second call of a group overwrites its range and keeps the rest
    g.set_plant_values(val=val[6:12], first=6)
    want_val[6:12] = val[6:12]
    assert np.array_equal(g.plant_values()[1], want_val)
    g.close(); ref.close()


@pytest.mark.gpu
def test_the_broadcast_shared_values_clear_and_set_plant_map_give_the_plain_rollout():
    B, k, r, T = 40, 7, 6, 3
    pat, fm, (g, twin) = _setup("MPC02", B, k, r)
    theta0, w = P._theta(B, k), RO._w(B, T, k)
    assert g.has_plant_values() == 0
    back = g.plant_values()  # (without per-instance values: the shared ones)
    assert np.array_equal(back[0], np.repeat(fm.base[None, :], B, axis=0)) and np.array_equal(back[1], np.repeat(fm.val[None, :], B, axis=0))
    g.set_plant_values(*back)
    assert g.has_plant_values() == 3
    RO._assert_rollout(g.rollout(theta0, T, w), twin.rollout(theta0, T, w), "broadcast shared values")
    _same_state(g, twin, B, "broadcast shared values")
    f0, val = _values(fm, B)
    g.set_plant_values(f0, val)
    g.clear_plant_values()
    assert g.has_plant_values() == 0
    th1 = P._theta(B, k, seed=1)
    RO._assert_rollout(g.rollout(th1, T, w), twin.rollout(th1, T, w), "after clear_plant_values")
    _same_state(g, twin, B, "after clear_plant_values")
    g.set_plant_values(f0, val)
    g.set_plant_map(fm)  # (installing a map drops the values: the pattern may have changed)
    assert g.has_plant_values() == 0
    th2 = P._theta(B, k, seed=2)
    RO._assert_rollout(g.rollout(th2, T, w), twin.rollout(th2, T, w), "after set_plant_map")
    g.set_plant_values(f0, val)
    g.set_plant_map(None)
    assert g.has_plant_values() == 0 and not g.has_plant_map()
    g.close(); twin.close()


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
def test_plant_values_on_every_build_of_the_solve_kernel(name, B, env, build, monkeypatch):
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    _compare_rollout(name, B, 5, 4, 2, True, build=build, launches=1)


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,k,env", [
    ("MPC02", 40, 7, {"EICOS_FUSED_UPDATE": "0"}),
    ("MPC02", 40, 7, {"EICOS_NLDS": "0", "EICOS_DUAL": "0"}),  # a handle without an LDS vector
    ("lp_afiro", 5, 1100, {}),                                   # a theta row that does not fit the LDS vector
])
def test_plant_values_without_the_fused_path_give_the_same_bits(name, B, k, env, monkeypatch):
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    T = 3
    _compare_rollout(name, B, k, 4, T, True, launches=T, full_rows=2)


@pytest.mark.gpu
def test_the_host_and_the_device_form_of_set_plant_values_give_the_same_rollout():
    host = _compare_rollout("MPC02", 40, 7, 6, 3, True)
    dev = _compare_rollout("MPC02", 40, 7, 6, 3, True, device=True)
    RO._assert_rollout(dev, host, "device form against host form")


@pytest.mark.gpu
@pytest.mark.parametrize("env,launches", [({}, 1), ({"EICOS_FUSED_UPDATE": "0"}, 3)])
def test_rollout_jacobian_with_plant_values_is_bit_identical_to_the_host_twin(env, launches, monkeypatch):
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    B, k, r, T = 40, 7, 6, 3
    pat, fm, (g, ref, plain) = _setup("MPC02", B, k, r, n_handles=3)
    f0, val = _values(fm, B)
    for s in (g, plain):
        s.set_plant_values(f0, val)
    theta0, w = P._theta(B, k), RO._w(B, T, k)
    want = RJ._host_loop_jac(ref, _Plant(fm, f0, val), theta0, T, w)
    got = g.rollout_jacobian(theta0, T, w)
    assert g.last_rollout_launches() == launches
    RJ._assert_six(got, want, env)
    RJ._same_handles(g, ref, B, env)
    RJ._assert_six(got, plain.rollout(theta0, T, w), env, n=4)
    for s in (g, ref, plain):
        s.close()


def _recorded(B=40, k=7, r=6, T=3, values=True):
    """A handle after rollout_jacobian (with per-instance values or with the shared plant), what it returned, and the rows it ran under."""
    pat, fm, (g,) = _setup("MPC02", B, k, r, n_handles=1)
    f0, val = _values(fm, B) if values else (None, None)
    if values:
        g.set_plant_values(f0, val)
    got = g.rollout_jacobian(P._theta(B, k), T, RO._w(B, T, k))
    assert g.last_rollout_launches() == 1
    return g, fm, got, val


@pytest.mark.gpu
def test_rollout_gradient_with_plant_values_is_bit_identical_to_backprop():
    g, fm, got, val = _recorded()
    u, th, J = got[0], got[1], got[4]
    rng = np.random.default_rng(11)
    gu, gth = rng.standard_normal(u.shape), rng.standard_normal(th.shape)
    for a, b in ((gu, None), (None, gth), (gu, gth)):
        want = fm.backprop(J, a, b, val=val)
        for dev in (False, True):
            have = g.rollout_gradient(a, b, device=dev)
            assert np.array_equal(have[0], want[0]) and np.array_equal(have[1], want[1]), (a is None, b is None, dev)
    assert np.all(np.isfinite(want[0])) and np.abs(want[0]).max() > 0
    assert not np.array_equal(want[0], fm.backprop(J, gu, gth)[0])  # (the shared values give another gradient)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("values", [True, False])
def test_rollout_plant_gradient_is_bit_identical_to_backprop_values(values):
    g, fm, got, val = _recorded(values=values)
    u, th, J = got[0], got[1], got[4]
    rng = np.random.default_rng(12)
    gu, gth = rng.standard_normal(u.shape), rng.standard_normal(th.shape)
    for a, b in ((gu, None), (None, gth), (gu, gth)):
        want = fm.backprop_values(J, u, th, a, b, val=val)
        plain = g.rollout_gradient(a, b)
        assert np.array_equal(plain[0], want[0]) and np.array_equal(plain[1], want[1])
        for dev in (False, True):
            have = g.rollout_plant_gradient(u, th, a, b, device=dev)
            for q, name in enumerate(("grad_theta0", "grad_w", "grad_f0", "grad_val")):
                assert have[q].shape == want[q].shape and np.array_equal(have[q], want[q]), (name, a is None, b is None, dev, values)
        for q in (2, 3):
            assert np.all(np.isfinite(want[q])) and np.abs(want[q]).max() > 0
    # every output is optional: the wanted ones keep their bits
    L = binding._lib()
    p = lambda a: a.ctypes.data_as(DP)
    gval, gf0 = np.full(want[3].shape, 7.0), np.full(want[2].shape, 7.0)
    assert L.eicos_batch_rollout_plant_gradient(g._h, p(gu), p(gth), p(u), p(th), None, None, None, p(gval)) == 0, L.eicos_last_error()
    assert L.eicos_batch_rollout_plant_gradient(g._h, p(gu), p(gth), p(u), p(th), None, None, p(gf0), None) == 0, L.eicos_last_error()
    assert np.array_equal(gval, want[3]) and np.array_equal(gf0, want[2])
    g.close()


@pytest.mark.gpu
def test_a_step_that_is_not_optimal_makes_the_rows_of_its_instance_nan():
    (A, ref), fm, theta0, w, T, B, iters0 = RJ._capped_handles(2)
    cap = int(iters0.min())
    f0, val = _values(fm, B)
    A.set_plant_values(f0, val)
    for g in (A, ref):
        g.set_settings(iter_max=cap)
    got = A.rollout_jacobian(theta0, T, w)
    want = RJ._host_loop_jac(ref, _Plant(fm, f0, val), theta0, T, w)
    u, th, codes, iters, J, res = got
    ok = (codes == 0) | (codes == 10)
    print("uncapped iterations", iters0.tolist(), "cap", cap, "codes", codes.tolist())
    assert ok.any() and (~ok).any(), codes  # some but not all steps end at the cap
    RJ._assert_six(got, want, "cap")
    rng = np.random.default_rng(5)
    gu, gth = rng.standard_normal(u.shape), rng.standard_normal(th.shape)
    have = A.rollout_plant_gradient(u, th, gu, gth)
    for a, b in zip(have, fm.backprop_values(want[4], u, th, gu, gth, val=val)):
        assert np.array_equal(a, b, equal_nan=True)
    bad = ~ok.all(axis=1)
    print("instances with a step at the cap", bad.tolist(), "their first such step", [int(np.argmin(o)) for o in ok[bad]])
    assert np.all(np.isnan(have[2][bad])) and np.all(np.isnan(have[3][bad]))
    assert np.all(np.isfinite(have[2][~bad])) and np.all(np.isfinite(have[3][~bad]))
    A.close(); ref.close()


@pytest.mark.gpu
def test_rollout_plant_gradient_against_finite_differences_of_plain_rollouts():
    pat, pmap, mmap, omap, theta, fm, gu = RJ._fd_setup()
    B, T = theta.shape[0], RJ.FD_T
    f0, val = _fd_values(fm, B)
    g = eicos_amd.BatchSolver(pat, B)
    vs = AM._fd_values(pmap, mmap, theta)
    g.update(*[np.stack([getattr(v, k) for v in vs]) for k in AD.KEYS])
    AM._install(g, pmap, mmap, omap)
    g.set_plant_map(fm)
    g.set_plant_values(f0, val)
    out = g.rollout_jacobian(theta, T)
    assert np.all(out[2] == 0), out[2]
    _, _, gf0, gval = g.rollout_plant_gradient(out[0], out[1], gu=gu)

    def loss(f0_, val_):
        g.set_plant_values(f0_, val_)
        u, _, codes, _ = g.rollout(theta, T)
        assert np.all(codes == 0), codes  # every instance qualifies: all its steps OPTIMAL on every run
        return (u * gu).sum(axis=(1, 2))

    fd_val, fd_f0 = np.zeros((B, len(FD_VALS))), np.zeros((B, len(FD_ROWS)))
    for q, s in enumerate(FD_VALS):
        e = np.zeros(fm.nnz()); e[s] = AM.FD_EPS
        fd_val[:, q] = (loss(f0, val + e) - loss(f0, val - e)) / (2.0 * AM.FD_EPS)
    for q, j in enumerate(FD_ROWS):
        e = np.zeros(fm.k); e[j] = 1e-6
        fd_f0[:, q] = (loss(f0 + e, val) - loss(f0 - e, val)) / (2.0 * 1e-6)
    for i in range(B):
        for name, gr, fd in (("val", gval[i, list(FD_VALS)], fd_val[i]), ("f0", gf0[i, list(FD_ROWS)], fd_f0[i])):
            dist, scale = np.max(np.abs(gr - fd)), np.max(np.abs(fd))
            print("instance", i, name, "max |grad - grad_fd|", dist, "max |grad_fd|", scale, "res", out[5][i].max())
            assert dist <= 1e-3 * scale, (i, name, dist, scale)
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
    nnz = fm.nnz()
    f0, val = _values(fm, B)
    theta0 = P._theta(B, k)
    p = lambda a: None if a is None else a.ctypes.data_as(DP)
    setv = lambda first=0, count=B, a=f0, b=val: L.eicos_batch_set_plant_values(g._h, first, count, p(a), p(b))
    g.set_param_map(pm); g.set_output_map(om)
    assert setv() == -1 and "no plant map" in err()
    assert L.eicos_batch_plant_values(g._h, 0, B, p(np.zeros((B, k))), None) == -1 and "no plant map" in err()
    assert g.has_plant_values() == 0
    g.set_plant_map(fm)
    g.set_plant_values(f0, val)
    before = g.rollout(theta0, T)
    rows = g.plant_values()
    # the setter
    assert setv(first=-1, count=1) == -1 and "out of bounds" in err()
    assert setv(first=B, count=1) == -1 and "out of bounds" in err()
    assert setv(first=1, count=B) == -1 and "out of bounds" in err()
    assert setv(count=-1) == -1 and "out of bounds" in err()
    assert setv(a=None, b=None) == -1 and "both NULL" in err()
    assert L.eicos_batch_plant_values(g._h, 2, B - 1, p(np.zeros((B, k))), None) == -1 and "out of bounds" in err()
    assert L.eicos_batch_plant_values(g._h, 0, B, None, None) == -1 and "both NULL" in err()
    dev = AM._device_doubles(B * max(k, nnz, (T + 1) * k, T * r))
    dptr, vptr = C.cast(dev, DP), C.c_void_p(f0.ctypes.data)
    assert L.eicos_batch_set_plant_values(g._h, 0, B, dptr, p(val)) == -1 and "host pointers" in err()
    assert L.eicos_batch_set_plant_values(g._h, 0, B, p(f0), dptr) == -1 and "host pointers" in err()
    assert L.eicos_batch_set_plant_values_device(g._h, 0, B, vptr, None) == -1 and "device memory" in err()
    assert L.eicos_batch_set_plant_values_device(g._h, 0, B, dev, vptr) == -1 and "device memory" in err()
    assert L.eicos_batch_plant_values(g._h, 0, B, dptr, None) == -1 and "host arrays" in err()
    back = g.plant_values()
    assert np.array_equal(back[0], rows[0]) and np.array_equal(back[1], rows[1]) and g.has_plant_values() == 3
    # the gradient
    gu, gth = np.ones((B, T, r)), np.ones((B, T + 1, k))
    outs = [np.zeros((B, k)), np.zeros((B, T, k)), np.zeros((B, k)), np.zeros((B, nnz))]

    def grad(a=gu, b=gth, u="u", th="th", o=(0, 1, 2, 3), fn=L.eicos_batch_rollout_plant_gradient):
        return fn(g._h, p(a), p(b), p(traj[0] if u == "u" else u), p(traj[1] if th == "th" else th), *[p(outs[q]) if q in o else None for q in range(4)])

    traj = (np.zeros((B, T, r)), np.zeros((B, T + 1, k)))
    assert grad() == -1 and "no Jacobian trajectory" in err()
    with pytest.raises(RuntimeError, match="no Jacobian trajectory"):
        g.rollout_plant_gradient(traj[0], traj[1], gu=gu)
    rec = g.rollout_jacobian(theta0, T)
    traj = (rec[0], rec[1])
    assert grad() == 0, err()
    good = [o.copy() for o in outs]
    assert grad(a=None, b=None) == -1 and "both NULL" in err()
    assert grad(u=None) == -1 and "u_traj is NULL" in err()
    assert grad(th=None) == -1 and "theta_traj is NULL" in err()
    assert grad(o=()) == -1 and "all NULL" in err()
    assert L.eicos_batch_rollout_plant_gradient(g._h, dptr, p(gth), p(traj[0]), p(traj[1]), p(outs[0]), None, None, None) == -1 and "host pointers" in err()
    assert L.eicos_batch_rollout_plant_gradient(g._h, p(gu), None, p(traj[0]), dptr, p(outs[0]), None, None, None) == -1 and "host pointers" in err()
    assert L.eicos_batch_rollout_plant_gradient(g._h, p(gu), None, p(traj[0]), p(traj[1]), None, None, None, dptr) == -1 and "host pointers" in err()
    assert L.eicos_batch_rollout_plant_gradient_device(g._h, vptr, None, dev, dev, dev, None, None, None) == -1 and "device memory" in err()
    assert L.eicos_batch_rollout_plant_gradient_device(g._h, dev, None, dev, dev, None, None, vptr, None) == -1 and "device memory" in err()
    L.hipFree(dev)
    assert grad() == 0 and all(np.array_equal(a, b) for a, b in zip(outs, good))  # (the refusals left the trajectory usable)
    # values set or cleared after the rollout: the trajectory no longer belongs to the handle's plant
    g.set_plant_values(f0=f0[:1])
    assert grad() == -1 and "installed after the rollout" in err()
    assert L.eicos_batch_rollout_gradient(g._h, p(gu), p(gth), p(outs[0]), None) == -1 and "installed after the rollout" in err()
    with pytest.raises(RuntimeError, match="installed after the rollout"):
        g.rollout_gradient(gu=gu)
    g.rollout_jacobian(theta0, T)
    assert grad() == 0
    g.clear_plant_values()
    assert grad() == -1 and "installed after the rollout" in err()
    # nothing moved: the same rows give the rollout they gave before
    g.set_plant_values(*rows)
    RO._assert_rollout(g.rollout(theta0, T), before, "after the refusals")
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("devs", [[0, 0], [0, 0, 0]])
def test_multi_forms_match_one_handle(devs):
    B, k, r, T = 5, 7, 6, 3
    pat, d = P._data("MPC02", B)
    pm, om, fm = P._map(d, k), _omap(pat.n, r), RO._fmap(k, r)
    f0, val = _values(fm, B)
    eicos_amd.set_arithmetic_profile(1)
    try:
        one = eicos_amd.BatchSolver(pat, B)
        m = eicos_amd.MultiBatchSolver(pat, B, devs)
        firsts = [first for first, _, _ in m.shards()]
        assert any(1 < f < 4 for f in firsts), firsts  # (the range [1, 4) below straddles a shard boundary)
        for s in (one, m):
            s.update(*[d[k_] for k_ in KEYS]); s.solve()
            s.set_param_map(pm); s.set_output_map(om); s.set_plant_map(fm)
            assert s.has_plant_values() == 0
            s.set_plant_values(f0=f0[1:4], val=val[1:4], first=1)
            assert s.has_plant_values() == 3
        for a, b in zip(m.plant_values(), one.plant_values()):
            assert np.array_equal(a, b)
        assert np.array_equal(m.plant_values(first=2, count=2)[1], one.plant_values()[1][2:4])
        theta0, w = P._theta(B, k), RO._w(B, T, k)
        RO._assert_rollout(m.rollout(theta0, T, w), one.rollout(theta0, T, w), devs)
        want = one.rollout_jacobian(theta0, T, w)
        got = m.rollout_jacobian(theta0, T, w)
        RJ._assert_six(got, want, devs)
        rng = np.random.default_rng(2)
        gu, gth = rng.standard_normal(want[0].shape), rng.standard_normal(want[1].shape)
        for a, b in ((gu, None), (gu, gth)):
            for x, y in zip(m.rollout_plant_gradient(got[0], got[1], a, b), one.rollout_plant_gradient(want[0], want[1], a, b)):
                assert x.shape == y.shape and np.array_equal(x, y), devs
        m.clear_plant_values()
        assert m.has_plant_values() == 0
        m.close(); one.close()
    finally:
        eicos_amd.set_arithmetic_profile(0)
