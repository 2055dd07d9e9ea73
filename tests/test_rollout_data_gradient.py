"""The rollout gradient with respect to the controller's own data: eicos_batch_set_rollout_recording / _rollout_records,
eicos_batch_rollout_data_gradient / _device, their eicos_multi_* forms and binding.rollout_data_backprop (include/eicos_amd.h, DESIGN.md
4.1).

A recording rollout_jacobian also leaves, per step, the rows grad_c / grad_h / grad_b of every output row (W) and the step's x, y, z on
the GPU; the contract is bit-identity of those records with the HOST TWIN -- per step update_param_solve, adjoint(g = the dense rows of
the output map), solution(), duals() -- and of everything rollout_jacobian returns, and of the handle's state, with recording off.
rollout_data_gradient is a second backward sweep in a fixed order; rollout_data_backprop is its host restatement, bit for bit.  Every
bit comparison is np.array_equal(..., equal_nan=True).  The finite-difference tests use the project's bound of test_adjoint*.py: 1e-3
of the largest finite-difference entry of the group.

Measured (docs/HISTORY.md A.30), CPU, the numpy reference's rows through rollout_data_backprop against the oracle's central difference
of the closed loop at T = 3, eps = 1e-4, max |grad - grad_fd| at max |grad_fd| over the perturbed entries of each group:
h0 1.36e-6 at 94.67, b0 3.0e-7 at 45.41, slope of H 5.0e-9 at 0.4385, G 2.01e-4 at 196.55, A 6.6e-7 at 35.71, U 7.8e-9 at 9.54:
980 times inside the bound (G) and better, every group on its own scale.  The derivative with respect to c0 is exactly 0 at the case's
LP vertex: its entries are held under an absolute noise floor instead (noise floor 5.9e-3, max |fd_c| 2.6e-6, max |grad_c| 7.6e-7; _c0_noise_floor_check)."""
import ctypes as C

import numpy as np
import pytest

import eicos_amd
from eicos_amd import binding
from eicos_amd.binding import DATA_GRADIENT_KEYS, DataGradient, MatrixMap, OutputMap, ParamMap, rollout_data_backprop
import test_param_update as P
import test_rhs_update as R
import test_rollout as RO
import test_matrix_param as MM
import test_adjoint as AD
import test_adjoint_matrix as AM
import test_rollout_jacobian as RJ
from test_fallback_law import _fbmap
from test_param_step import _omap

KEYS = R.KEYS
DP = C.POINTER(C.c_double)
EPS = np.finfo(np.float64).eps
REC = ("Wc", "Wh", "Wb", "x", "y", "z")


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------
def _same(a, b, what):
    assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), what


def _same_dict(got, want, what):
    assert set(got) == set(want), what
    for q in got:
        _same(got[q], want[q], (what, q))


def _twin_records(ref, om, fm, theta0, T, w):
    """The host twin of a recording rollout_jacobian: per step update_param_solve on pinned theta and u, param_jacobian, adjoint with the
    dense rows of the output map, solution(), duals(), the plant map on the host.  Returns (the six arrays of rollout_jacobian, the six
    records)."""
    B, k = theta0.shape
    g = np.repeat(binding._dense_rows(om)[None], B, axis=0)
    pth, pu = eicos_amd.PinnedArray((B, k)), eicos_amd.PinnedArray((B, fm.r))
    th, six, rec = theta0.copy(), [[theta0.copy()]] + [[] for _ in range(5)], [[] for _ in range(6)]
    for t in range(T):
        pth.a[...] = th
        pu.a[...] = np.nan
        six[2].append(np.asarray(ref.update_param_solve(pth.a, u_out=pu.a)).copy())
        six[3].append(ref.info_arrays()["iter"].copy())
        J, res = ref.param_jacobian()
        six[4].append(J); six[5].append(res)
        gc, gh, gb, _ = ref.adjoint(g)
        y, z, _s = ref.duals()
        for q, a in enumerate((gc, gh, gb, ref.solution(), y, z)):
            rec[q].append(a)
        six[1].append(pu.a.copy())
        th = fm.evaluate(th, six[1][-1], None if w is None else w[:, t])
        six[0].append(th)
    pth.close(); pu.close()
    u, thetas = np.stack(six[1], axis=1), np.stack(six[0], axis=1)
    return (u, thetas) + tuple(np.stack(a, axis=1) for a in six[2:]), tuple(np.stack(a, axis=1) for a in rec)


def _record_case(name, B, k, r, T, with_w=True, build=None, launches=None, full_rows=0, matrix=False, prepare=None, twin=True):
    """Three handles in the same state: one takes rollout_jacobian() under recording, one the host twin, one rollout_jacobian() with
    recording off.  Returns a dict of what the caller goes on with; it closes the recording handle itself."""
    pat, d = P._data(name, B)
    pm, om, fm = P._map(d, k, full_rows=full_rows), _omap(pat.n, r), RO._fmap(k, r)
    mm = MM._mmap(d, k) if matrix else None
    g, ref = P._twins(pat, d, B)
    off = P._twins(pat, d, B)[0]
    if build is not None:
        assert (g.kernel_build(), g.dims()["threads_per_block"]) == build, (g.kernel_build(), g.dims()["threads_per_block"])
    for s in (g, ref, off):
        if prepare:
            prepare(s)
        s.set_param_map(pm); s.set_output_map(om)
        if mm is not None:
            s.set_matrix_map(mm)
    for s in (g, off):
        s.set_plant_map(fm)
    assert not g.rollout_recording()
    g.set_rollout_recording(True)
    assert g.rollout_recording() and not off.rollout_recording()
    theta0, w = P._theta(B, k), (RO._w(B, T, k) if with_w else None)
    what = (name, B, k, r, T, matrix)
    got = g.rollout_jacobian(theta0, T, w)
    recs = g.rollout_records()
    if launches is not None:
        assert g.last_rollout_launches() == launches, (what, g.last_rollout_launches())
    # recording on against recording off: the six returned arrays and the handle's state
    plain = off.rollout_jacobian(theta0, T, w)
    RJ._assert_six(got, plain, what)
    RJ._same_handles(g, off, B, what)
    with pytest.raises(RuntimeError, match="no recorded rows"):
        off.rollout_records()
    off.close()
    if twin:
        want, want_recs = _twin_records(ref, om, fm, theta0, T, w)
        RJ._assert_six(got, want, what)
        for q, (a, b) in enumerate(zip(recs, want_recs)):
            _same(a, b, (what, REC[q]))
        RJ._same_handles(g, ref, B, what)
    ref.close()
    return dict(g=g, pat=pat, pm=pm, om=om, fm=fm, mm=mm, got=got, recs=recs, what=what)


def _restated(c, gu, gth, val=None, want=DATA_GRADIENT_KEYS):
    got, recs = c["got"], c["recs"]
    return rollout_data_backprop(c["pat"], c["pm"], c["om"], c["fm"], got[4], recs[:3], recs[3], recs[4], recs[5], got[1], gu, gth, val=val, want=want)


def _wanted(pm):
    """Every output the maps of a case allow: a slope only for a group that has a map."""
    return tuple(q for q in DATA_GRADIENT_KEYS if q not in ("grad_Cval", "grad_Hval", "grad_Bval") or pm.groups()["CHB".index(q[5])] is not None)


# ---- CPU --------------------------------------------------------------------------------------------------------------------------------
def test_data_gradient_entry_points_exist_and_refuse_a_null_handle():
    L = binding._lib()
    dp = np.zeros(4).ctypes.data_as(DP)
    st = DataGradient(grad_c=np.zeros(4).ctypes.data)
    assert L.eicos_data_gradient_size() == C.sizeof(DataGradient) == 10 * C.sizeof(C.c_void_p)
    err = L.eicos_last_error
    for rc in (L.eicos_batch_set_rollout_recording(None, 1), L.eicos_batch_rollout_recording(None), L.eicos_batch_rollout_records(None, dp, None, None, None, None, None),
               L.eicos_batch_rollout_data_gradient(None, dp, None, dp, C.byref(st)), L.eicos_batch_rollout_data_gradient_device(None, None, None, None, C.byref(st))):
        assert rc == -1 and b"NULL handle" in err()
    err = L.eicos_multi_last_error
    for rc in (L.eicos_multi_set_rollout_recording(None, 1), L.eicos_multi_rollout_recording(None), L.eicos_multi_rollout_records(None, dp, None, None, None, None, None),
               L.eicos_multi_rollout_data_gradient(None, dp, None, dp, C.byref(st))):
        assert rc == -1 and b"NULL handle" in err()
    listed = {full for full, _, _ in binding._SIGNATURES}
    for f in ("set_rollout_recording", "rollout_recording", "rollout_records", "rollout_data_gradient"):
        assert {"eicos_batch_" + f, "eicos_multi_" + f} <= listed, f
        assert callable(getattr(eicos_amd.BatchSolver, f)) and callable(getattr(eicos_amd.MultiBatchSolver, f))
    assert "eicos_batch_rollout_data_gradient_device" in listed and callable(eicos_amd.rollout_data_backprop)


def test_arrays_of_the_wrong_shape_are_refused_before_the_library_is_called():
    pat, pmap, mmap, omap, theta0, fm, gu = RJ._fd_setup()
    B, T, k, r, n, m, p = theta0.shape[0], RJ.FD_T, AM.K, AM.R, pat.n, pat.m, pat.p

    class Probe(binding._Solver):  # (a solver object whose library call would raise something else: the checks stand in front of it)
        batch, _rollout_shape, _param_nnz, _out_nnz = B, (T, k, r), (1, 1, 1), 1

        def _call(self, name, *a):
            raise AssertionError("the library was called: " + name)

    Probe.pat = pat
    good = dict(theta=np.zeros((B, T + 1, k)), gu=np.zeros((B, T, r)))
    for bad in ({"theta": np.zeros((B, T, k))}, {"theta": None}, {"gu": np.zeros((B, T + 1, r))}, {"gu": None}, {"gtheta": np.zeros((B, T, k))},
                {"want": ()}, {"want": ("grad_c", "grad_x")}):
        with pytest.raises(ValueError):
            Probe().rollout_data_gradient(**dict(good, **bad))
    with pytest.raises(AssertionError, match="rollout_data_gradient"):  # (well-shaped arrays do reach the library)
        Probe().rollout_data_gradient(**good)
    # the restatement checks its arrays the same way
    J, th = np.zeros((B, T, r, k)), np.zeros((B, T + 1, k))
    W, x, y, z = (np.zeros((B, T, r, n)), np.zeros((B, T, r, m)), np.zeros((B, T, r, p))), np.zeros((B, T, n)), np.zeros((B, T, p)), np.zeros((B, T, m))
    args = lambda **kw: dict(dict(pattern=pat, pmap=pmap, omap=omap, fmap=fm, J=J, W=W, x=x, y=y, z=z, theta=th, gu=gu), **kw)
    assert set(rollout_data_backprop(**args())) == set(DATA_GRADIENT_KEYS)
    for bad in ({"J": np.zeros((B, T, r, k + 1))}, {"W": (W[0], W[1])}, {"W": (W[0], W[2], W[1])}, {"x": np.zeros((B, T + 1, n))}, {"y": None},
                {"theta": np.zeros((B, T, k))}, {"gu": None}, {"gu": np.zeros((B, T, r + 1))}, {"want": ("grad_q",)},
                {"pmap": ParamMap(k, c=pmap.c), "want": ("grad_Hval",)}):
        with pytest.raises(ValueError):
            rollout_data_backprop(**args(**bad))


def test_restatement_against_a_dense_einsum_chain():
    """Random small arrays on the pattern and the maps of the finite-difference case.  The dense chain forms mu_t with matrix products and
    every gradient as one einsum; the restatement adds the same terms one by one, so the two differ by rounding alone: at most 64 ulps
    of the accumulated magnitude (the same sums over absolute values; T r = 6 terms per entry on a mu that is itself T (k + r) = 15
    rounded terms deep)."""
    pat, pmap, mmap, omap, theta0, fm, _ = RJ._fd_setup()
    B, T, k, r, n, m, p = 3, 3, AM.K, AM.R, pat.n, pat.m, pat.p
    rng = np.random.default_rng(17)
    fm = binding.PlantMap(k, r, (fm.base, fm.rowptr, fm.col, rng.uniform(-1, 1, fm.col.size)))
    J, gu, gth, th = rng.standard_normal((B, T, r, k)), rng.standard_normal((B, T, r)), rng.standard_normal((B, T + 1, k)), rng.standard_normal((B, T + 1, k))
    W = tuple(rng.standard_normal((B, T, r, w)) for w in (n, m, p))
    x, y, z = rng.standard_normal((B, T, n)), rng.standard_normal((B, T, p)), rng.standard_normal((B, T, m))
    got = rollout_data_backprop(pat, pmap, omap, fm, J, W, x, y, z, th, gu, gth)

    def chain(J, gu, gth, W, x, y, z, th, maps, F):
        """mu_t by the dense chain, then every gradient as an einsum over (t, a)."""
        Ft, Fu = F[:, :k], F[:, k:]
        mu, lam = np.zeros((B, T, r)), gth[:, T].copy()
        for t in range(T - 1, -1, -1):
            mu[:, t] = gu[:, t] + lam @ Fu
            lam = gth[:, t] + lam @ Ft + np.einsum("bak,ba->bk", J[:, t], mu[:, t])
        d = [np.einsum("bta,btai->bti", mu, Wg) for Wg in W]
        Gi, Gj, Ai, Aj = pat.Gir, AM._cols(pat.Gjc), pat.Air, AM._cols(pat.Ajc)
        out = {"grad_c": d[0].sum(1), "grad_h": d[1].sum(1), "grad_b": d[2].sum(1),
               "grad_G": (maps["sgn"][0] * d[0][:, :, Gj] * z[:, :, Gi] + maps["sgn"][1] * d[1][:, :, Gi] * x[:, :, Gj]).sum(1),
               "grad_A": (maps["sgn"][0] * d[0][:, :, Aj] * y[:, :, Ai] + maps["sgn"][1] * d[2][:, :, Ai] * x[:, :, Aj]).sum(1),
               "grad_u0": mu.sum(1), "grad_Uval": np.einsum("bts,bts->bs", mu[:, :, maps["Urow"]], x[:, :, omap.col])}
        for q, (name, grp) in enumerate(zip(("grad_Cval", "grad_Hval", "grad_Bval"), pmap.groups())):
            rows = np.repeat(np.arange(grp[0].size), np.diff(grp[1]))
            out[name] = np.einsum("bts,bts->bs", d[q][:, :, rows], th[:, :T, grp[2]])
        return out

    Urow = np.repeat(np.arange(r), np.diff(omap.rowptr))
    F = RJ._dense_plant(fm)
    want = chain(J, gu, gth, W, x, y, z, th, {"sgn": (1.0, -1.0), "Urow": Urow}, F)
    mag = chain(*[np.abs(a) for a in (J, gu, gth)], tuple(np.abs(a) for a in W), *[np.abs(a) for a in (x, y, z, th)], {"sgn": (1.0, 1.0), "Urow": Urow}, np.abs(F))
    for q in DATA_GRADIENT_KEYS:
        dist = np.abs(got[q] - want[q])
        assert got[q].shape == want[q].shape and np.all(dist <= 64 * EPS * mag[q]), (q, np.max(dist / np.maximum(mag[q], 1e-300)) / EPS)
    # a missing cotangent is 0.0 that is still added: the same bits as an array of zeros; the halves add up to the whole
    only_u, only_t = (rollout_data_backprop(pat, pmap, omap, fm, J, W, x, y, z, th, a, b) for a, b in ((gu, None), (None, gth)))
    _same_dict(only_u, rollout_data_backprop(pat, pmap, omap, fm, J, W, x, y, z, th, gu, np.zeros_like(gth)), "gtheta missing")
    for q in DATA_GRADIENT_KEYS:
        assert np.all(np.abs(only_u[q] + only_t[q] - got[q]) <= 64 * EPS * mag[q]), q
    # `want` only selects
    part = rollout_data_backprop(pat, pmap, omap, fm, J, W, x, y, z, th, gu, gth, want=("grad_G", "grad_u0"))
    _same_dict(part, {q: got[q] for q in ("grad_G", "grad_u0")}, "want")
    # NaN rows of one step poison the data gradients of their own instance only
    Wn = tuple(a.copy() for a in W)
    for a in Wn:
        a[1, 1] = np.nan
    Jn = J.copy(); Jn[1, 1] = np.nan
    bad = rollout_data_backprop(pat, pmap, omap, fm, Jn, Wn, x, y, z, th, gu, gth)
    for q in DATA_GRADIENT_KEYS:
        if q not in ("grad_u0", "grad_Uval"):
            assert np.all(np.isnan(bad[q][1])), q
        _same(bad[q][[0, 2]], got[q][[0, 2]], q)


def _oracle_records(pat, pmap, mmap, omap, fm, theta0, T):
    """The closed loop of RJ._oracle_rollout with, per step, the numpy reference's rows: J_t, W_t = grads(dense U) and x, y, z."""
    U = AD._csr_dense((omap.base, omap.rowptr, omap.col, omap.val), pat.n)
    maps = AM._dense_maps(pat, pmap, mmap)
    B = theta0.shape[0]
    th, out = theta0.copy(), [[] for _ in range(9)]
    thetas = [th.copy()]
    for t in range(T):
        row = [np.zeros((B,) + s) for s in ((AM.R,), (AM.R, AM.K), (AM.R, pat.n), (AM.R, pat.m), (AM.R, pat.p), (pat.n,), (pat.p,), (pat.m,))]
        for i, v in enumerate(AM._fd_values(pmap, mmap, th)):
            code, x, y, z, s = AD._oracle_x(pat, v)
            assert code == 0, (t, i, code)
            ref = AD._Reference(pat, v, s, z)
            assert ref.cond <= AD.COND_MAX, (t, i, ref.cond)
            row[0][i] = omap.evaluate(x[None, :])[0]
            row[1][i] = U @ AM._reference_columns(pat, ref, maps, x, y, z)[: pat.n]
            row[2][i], row[3][i], row[4][i] = ref.grads(U)
            row[5][i], row[6][i], row[7][i] = x, y, z
        for q, a in enumerate(row):
            out[q].append(a)
        th = fm.evaluate(th, row[0])
        thetas.append(th.copy())
    u, J, Wc, Wh, Wb, x, y, z = (np.stack(a, axis=1) for a in out[:8])
    return u, np.stack(thetas, axis=1), J, (Wc, Wh, Wb), x, y, z


def _perturbed(pmap, mmap, omap, group, e, delta):
    """The maps of the finite-difference case with entry e of one group moved by delta: c0 / h0 / b0 the base vectors, Hval a slope of
    the h group, G / A a base value of the matrix map (= the stored value at every step), Uval a value of the output map."""
    def moved(grp, part):
        arrs = [a.copy() for a in grp]
        arrs[part][e] += delta
        return tuple(arrs)

    if group in ("c0", "h0", "b0", "Hval"):
        gs = dict(zip("chb", pmap.groups()))
        key = group[0].lower()
        gs[key] = moved(gs[key], 3 if group == "Hval" else 0)
        pmap = ParamMap(pmap.k, **gs)
    elif group in ("G", "A"):
        gs = dict(zip("GA", mmap.groups()))
        gs[group] = moved(gs[group], 0)
        mmap = MatrixMap(mmap.k, **gs)
    else:
        omap = OutputMap(omap.n, moved((omap.base, omap.rowptr, omap.col, omap.val), 3))
    return pmap, mmap, omap


FD_KEY = {"c0": "grad_c", "h0": "grad_h", "b0": "grad_b", "Hval": "grad_Hval", "G": "grad_G", "A": "grad_A", "Uval": "grad_Uval"}
# The groups a bound is taken over, each on its own scale, and how many entries of each kind are perturbed.  c0 is not among them: the
# case is a strictly complementary LP vertex (every cone inactive), where x is fixed by the active rows and does not depend on c at
# all.  d L / d c0 is exactly 0 there, so there is no finite-difference scale to take 1e-3 of: _c0_noise_floor_check states what holds.
FD_GROUPS = (("h0", (("h0", 3),)), ("b0", (("b0", 3),)), ("map slope", (("Hval", 1),)), ("G", (("G", 1),)), ("A", (("A", 1),)), ("U", (("Uval", 1),)))
SOLVE_TOL = 1e-8  # feastol = abstol = reltol of the default settings: what a returned x is determined to, relative to max(1, |x|)


def _fd_entries(grad, count):
    """The `count` entries of a group with the largest gradient over the instances: away from inactive rows, whose derivative is 0."""
    return [int(e) for e in np.argsort(-np.abs(grad).max(axis=0))[:count]]


def _fd_check(grad, groups, fd_of):
    """Per group: the perturbed entries' gradient against fd_of(kind, entry) -> [B], with the project's bound over the group."""
    for label, kinds in groups:
        have, fd, names = [], [], []
        for kind, count in kinds:
            for e in _fd_entries(grad[FD_KEY[kind]], count):
                have.append(grad[FD_KEY[kind]][:, e]); fd.append(fd_of(kind, e)); names.append((kind, e))
        have, fd = np.stack(have, axis=1), np.stack(fd, axis=1)
        for (kind, e), a, b in zip(names, have.T, fd.T):
            print("   ", kind, e, "grad", a.tolist(), "fd", b.tolist())
        dist, scale = np.max(np.abs(have - fd)), np.max(np.abs(fd))
        print(label, "max |grad - grad_fd|", dist, "max |grad_fd|", scale)
        assert scale > 0 and dist <= 1e-3 * scale, (label, names, dist, scale)


def _c0_noise_floor_check(grad, fd_of, gu, omap, x, count=3):
    """d L / d c0 on the LP-vertex case, where the derivative is exactly 0: an ABSOLUTE NOISE FLOOR, not a relative bound.  A returned x
    is determined to SOLVE_TOL max(1, |x|), so L = sum gu' (u0 + U x) of one run to SOLVE_TOL max(1, |x|_inf) sum |gu| max_a |U_a|_1, and
    a central difference of two runs to that over eps: floor = (SOLVE_TOL / FD_EPS) sum_t,a |gu| max_a |U_a|_1 max(1, |x|_inf), about
    4e-3 here against gradients of 20 ... 200 in the other groups.  Both the central difference (the solves' noise) and grad_c (the
    adjoint's smoothed value at the vertex) of every perturbed entry must lie under it.  This says that grad_c is 0 to the resolution of
    a finite difference; it cannot tell a smoothed value from its double.  The arithmetic that forms grad_c is the arithmetic of
    grad_h and grad_b (one loop over the three groups in the kernel and in the restatement), which the groups above hold to 1e-3."""
    U = np.abs(binding._dense_rows(omap)).sum(axis=1).max()
    floor = (SOLVE_TOL / AM.FD_EPS) * np.abs(gu).sum(axis=(1, 2)).max() * U * max(1.0, np.abs(x).max())
    entries = _fd_entries(grad["grad_c"], count)
    fd = np.stack([fd_of("c0", e) for e in entries], axis=1)
    have = grad["grad_c"][:, entries]
    print("c0 entries", entries, "noise floor", floor, "max |grad_c|", np.max(np.abs(have)), "max |fd_c|", np.max(np.abs(fd)), "max |grad_c| over all entries", np.max(np.abs(grad["grad_c"])))
    assert np.max(np.abs(fd)) <= floor and np.max(np.abs(grad["grad_c"])) <= floor, (entries, floor, np.max(np.abs(fd)), np.max(np.abs(grad["grad_c"])))


def test_the_reference_stays_within_the_bound_against_the_oracle_central_differences():
    """The numpy reference's rows (AD._Reference, AM._reference_columns) through rollout_data_backprop against the oracle's central
    difference of the closed loop, T = 3, eps = AM.FD_EPS, over the perturbed entries of every group of FD_GROUPS, each group on its own
    scale (the entries with the largest gradient: three each of h0 and b0, one slope of H, one stored value of G, one of A, one value
    of U), and three entries of c0 against the noise floor of _c0_noise_floor_check.  Measured max |grad - grad_fd| at max |grad_fd|:
    h0 1.36e-6 at 94.67, b0 3.0e-7 at 45.41, slope of H 5.0e-9 at 0.4385, G 2.01e-4 at 196.55, A 6.6e-7 at 35.71, U 7.8e-9 at 9.54 -- against a bound of 1e-3 of the latter; c0: noise floor 5.9e-3, max |fd_c| 2.6e-6, max |grad_c| 7.6e-7."""
    pat, pmap, mmap, omap, theta, fm, gu = RJ._fd_setup()
    T = RJ.FD_T
    u, th, J, W, x, y, z = _oracle_records(pat, pmap, mmap, omap, fm, theta, T)
    u2, J2 = RJ._oracle_rollout(pat, pmap, mmap, omap, fm, theta, T, True)
    assert np.array_equal(u, u2) and np.array_equal(J, J2)
    grad = rollout_data_backprop(pat, pmap, omap, fm, J, W, x, y, z, th, gu=gu)

    def fd_of(kind, e):
        up, _ = RJ._oracle_rollout(pat, *_perturbed(pmap, mmap, omap, kind, e, AM.FD_EPS), fm, theta, T, False)
        um, _ = RJ._oracle_rollout(pat, *_perturbed(pmap, mmap, omap, kind, e, -AM.FD_EPS), fm, theta, T, False)
        return ((up - um) * gu).sum(axis=(1, 2)) / (2.0 * AM.FD_EPS)

    _fd_check(grad, FD_GROUPS, fd_of)
    _c0_noise_floor_check(grad, fd_of, gu, omap, x)


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,B,k,r,T", [
    ("MPC02", 4, 5, 4, 2),
    ("lp_afiro", 4, 5, 4, 2),
    ("issue98", 8, 5, 4, 2),
    ("socp-random", 8, 5, 4, 2),
    ("dense-front", 6, 5, 4, 2),
])
def test_records_are_bit_identical_to_the_host_twin(name, B, k, r, T):
    c = _record_case(name, B, k, r, T)
    if name == "MPC02":  # (every step of this case ends optimal: the rows are numbers, and not all of them 0.0)
        assert np.all(c["got"][2] == 0) and all(np.all(np.isfinite(a)) for a in c["recs"]) and np.abs(c["recs"][0]).max() > 0
    c["g"].close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,env,build", [
    ("MPC02", 4, {"EICOS_UBL": "0", "EICOS_THREADS": "256"}, ("w2", 256)),
    ("MPC02", 4, {"EICOS_UBL": "0", "EICOS_THREADS": "256", "EICOS_W2": "0"}, ("default", 256)),
    ("MPC02", 4, {"EICOS_UBL": "0", "EICOS_W2": "0", "EICOS_THREADS": "128"}, ("default", 128)),
    ("MPC02", 4, {"EICOS_UBL": "0", "EICOS_W2": "0", "EICOS_THREADS": "512"}, ("default", 512)),
    ("issue98", 4, {"EICOS_THREADS": "256"}, ("u-in-lds", 256)),
    ("lp_bandm", 4, {}, ("u-in-lds", 512)),
    ("lp_afiro", 4, {}, ("lds-resident", 128)),
])
def test_records_on_every_build_of_the_solve_kernel(name, B, env, build, monkeypatch):
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    c = _record_case(name, B, 5, 4, 2, build=build, launches=1)
    c["g"].close()


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"EICOS_FUSED_UPDATE": "0"}, {"EICOS_NLDS": "0", "EICOS_DUAL": "0"}])
def test_records_without_the_fused_path_give_the_same_bits(env, monkeypatch):
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    T = 2
    c = _record_case("MPC02", 4, 5, 4, T, launches=T, full_rows=2)
    c["g"].close()


@pytest.mark.gpu
@pytest.mark.parametrize("env,launches", [({}, 1), ({"EICOS_FUSED_UPDATE": "0"}, 2)])
def test_records_with_parts_of_no_width_give_the_same_bits_on_both_paths(env, launches, monkeypatch):
    """feas, the smallest fixture without equality rows (p = 0): the record's parts Wb and y have no width, so each starts where the
    part behind it starts.  B = 3, T = 2, k = 3, r = 2; the fused path and the one that is not, against the same host twin."""
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    c = _record_case("feas", 3, 3, 2, 2, launches=launches)
    assert c["pat"].p == 0 and c["recs"][2].shape[-1] == 0 and c["recs"][4].shape[-1] == 0 and c["recs"][0].size > 0
    c["g"].close()


@pytest.mark.gpu
def test_data_gradient_is_bit_identical_to_the_restatement():
    c = _record_case("MPC02", 4, 5, 4, 3, launches=1, twin=False)
    g, got = c["g"], c["got"]
    rng = np.random.default_rng(11)
    gu, gth = rng.standard_normal(got[0].shape), rng.standard_normal(got[1].shape)
    every = _wanted(c["pm"])
    for a, b in ((gu, None), (None, gth), (gu, gth)):
        want = _restated(c, a, b, want=every)
        for dev in (False, True):
            _same_dict(g.rollout_data_gradient(got[1], a, b, want=every, device=dev), want, (a is None, b is None, dev))
    assert all(np.all(np.isfinite(v)) for v in want.values()) and np.abs(want["grad_c"]).max() > 0 and np.abs(want["grad_G"]).max() > 0
    # a subset of the outputs: the same bits, nothing else touched
    part = g.rollout_data_gradient(got[1], gu, gth, want=("grad_h", "grad_Uval"))
    _same_dict(part, {q: want[q] for q in part}, "subset")
    # mu is rollout_gradient's: the sweep that is already there still gives its bits on a recording handle
    g0, gw = g.rollout_gradient(gu, gth)
    w0, ww = c["fm"].backprop(got[4], gu, gth)
    assert np.array_equal(g0, w0) and np.array_equal(gw, ww)
    # switching recording off frees the record; the J trajectory stays on the handle
    g.set_rollout_recording(False)
    with pytest.raises(RuntimeError, match="no recorded rows"):
        g.rollout_records()
    with pytest.raises(RuntimeError, match="no recorded rows"):
        g.rollout_data_gradient(got[1], gu, gth, want=("grad_c",))
    assert np.array_equal(g.rollout_gradient(gu, gth)[0], w0)
    g.close()


@pytest.mark.gpu
def test_data_gradient_with_per_instance_plant_values():
    name, B, k, r, T = "MPC02", 4, 5, 4, 3
    pat, d = P._data(name, B)
    pm, om, fm = P._map(d, k), _omap(pat.n, r), RO._fmap(k, r)
    g = P._twins(pat, d, B)[0]
    g.set_param_map(pm); g.set_output_map(om); g.set_plant_map(fm)
    val = fm.val[None, :] * np.random.default_rng(4).uniform(0.9, 1.1, (B, fm.nnz()))
    g.set_plant_values(val=val)
    g.set_rollout_recording(True)
    got = g.rollout_jacobian(P._theta(B, k), T, RO._w(B, T, k))
    c = dict(pat=pat, pm=pm, om=om, fm=fm, got=got, recs=g.rollout_records())
    rng = np.random.default_rng(12)
    gu, gth = rng.standard_normal(got[0].shape), rng.standard_normal(got[1].shape)
    every = _wanted(pm)
    want = _restated(c, gu, gth, val=val, want=every)
    _same_dict(g.rollout_data_gradient(got[1], gu, gth, want=every), want, "plant values")
    shared = _restated(c, gu, gth, want=every)
    assert not np.array_equal(shared["grad_c"], want["grad_c"])  # (the values do enter mu)
    g.close()


@pytest.mark.gpu
def test_data_gradient_under_a_matrix_map():
    c = _record_case("MPC02", 4, 5, 4, 2, launches=1, matrix=True)
    g, got = c["g"], c["got"]
    rng = np.random.default_rng(13)
    gu, gth = rng.standard_normal(got[0].shape), rng.standard_normal(got[1].shape)
    every = _wanted(c["pm"])
    _same_dict(g.rollout_data_gradient(got[1], gu, gth, want=every), _restated(c, gu, gth, want=every), "matrix map")
    g.close()


@pytest.mark.gpu
def test_records_and_data_gradient_under_a_retry_policy():
    (A, ref), fm, theta0, w, T, B, iters0 = RJ._capped_handles(2)
    pat, d = P._data("MPC02", B)
    pm, om = P._map(d, 7), _omap(pat.n, 6)
    cap = int(iters0.min())
    for g in (A, ref):
        g.set_settings(iter_max=cap)
        g.set_retry(eicos_amd.SEL_NOT_OPTIMAL)
    A.set_rollout_recording(True)
    got = A.rollout_jacobian(theta0, T, w)
    recs = A.rollout_records()
    want, want_recs = _twin_records(ref, om, fm, theta0, T, w)
    assert A.retry_counts().any()
    RJ._assert_six(got, want, "retry")
    for q, (a, b) in enumerate(zip(recs, want_recs)):  # (x, y, z: the final attempt)
        _same(a, b, ("retry", REC[q]))
    RJ._same_handles(A, ref, B, "retry")
    c = dict(pat=pat, pm=pm, om=om, fm=fm, got=got, recs=recs)
    rng = np.random.default_rng(14)
    gu, gth = rng.standard_normal(got[0].shape), rng.standard_normal(got[1].shape)
    every = _wanted(pm)
    _same_dict(A.rollout_data_gradient(got[1], gu, gth, want=every), _restated(c, gu, gth, want=every), "retry")
    A.close(); ref.close()


@pytest.mark.gpu
def test_data_gradient_against_finite_differences_of_plain_rollouts():
    """rollout_data_gradient against central differences of plain rollouts at T = 3 on the case of RJ._fd_setup, without its matrix map,
    so that a stored value of G is perturbed through update(): three entries each of c0 and h0 perturbed by re-installing the parameter
    map, one stored value of G.  Bound: 1e-3 of the largest finite-difference entry of the group for h0 and for G; the c0 entries,
    whose derivative is exactly 0 on this case, under the noise floor of _c0_noise_floor_check.  Measured on one MI355X:
    max |grad - grad_fd| at max |grad_fd| h0 1.36e-6 at 94.67, G 2.01e-4 at 196.55 (the CPU figures of the reference to three
    digits); c0: noise floor 5.9e-3, max |fd_c| 2.6e-6, max |grad_c| 7.6e-7; res 2.5e-15."""
    pat, pmap, mmap, omap, theta, fm, gu = RJ._fd_setup()
    B, T = theta.shape[0], RJ.FD_T
    Gpr, Apr = np.repeat(mmap.G[0][None], B, axis=0), np.repeat(mmap.A[0][None], B, axis=0)
    c0, h0, b0 = pmap.evaluate(theta)
    g = eicos_amd.BatchSolver(pat, B)
    g.update(Gpr, Apr, c0, h0, b0)
    AM._install(g, pmap, None, omap)
    g.set_plant_map(fm)
    g.set_rollout_recording(True)
    out = g.rollout_jacobian(theta, T)
    assert np.all(out[2] == 0), out[2]
    grad = g.rollout_data_gradient(out[1], gu=gu, want=("grad_c", "grad_h", "grad_G"))
    x_rec = g.rollout_records()[3]

    def loss():
        u, _, codes, _ = g.rollout(theta, T)
        assert np.all(codes == 0), codes
        return (u * gu).sum(axis=(1, 2))

    def fd_of(kind, e):
        side = []
        for sg in (1.0, -1.0):
            if kind == "G":
                Gp = Gpr.copy(); Gp[:, e] += sg * AM.FD_EPS
                g.update(Gp, Apr, c0, h0, b0)
            else:
                g.set_param_map(_perturbed(pmap, mmap, omap, kind, e, sg * AM.FD_EPS)[0])
            side.append(loss())
        g.update(Gpr, Apr, c0, h0, b0); g.set_param_map(pmap)
        return (side[0] - side[1]) / (2.0 * AM.FD_EPS)

    print("res", out[5].max())
    _fd_check(grad, (("h0", (("h0", 3),)), ("G", (("G", 1),))), fd_of)
    _c0_noise_floor_check(grad, fd_of, gu, omap, x_rec)
    g.close()


@pytest.mark.gpu
def test_steps_that_are_not_optimal_give_nan_gradients_for_their_instances_only():
    (A,), fm, theta0, w, T, B, iters0 = RJ._capped_handles(1)
    pat, d = P._data("MPC02", B)
    pm, om = P._map(d, 7), _omap(pat.n, 6)
    A.set_settings(iter_max=int(iters0.min()))
    A.set_rollout_recording(True)
    got = A.rollout_jacobian(theta0, T, w)
    u, th, codes, iters, J, res = got
    recs = A.rollout_records()
    ok = (codes == 0) | (codes == 10)
    assert ok.any() and (~ok).any(), codes
    for Wg in recs[:3]:
        assert np.all(np.isnan(Wg[~ok])) and np.all(np.isfinite(Wg[ok]))  # NaN rows as J has them
    assert all(np.all(np.isfinite(a)) for a in recs[3:])  # x, y, z are recorded whatever the exit code
    rng = np.random.default_rng(5)
    gu, gth = rng.standard_normal(u.shape), rng.standard_normal(th.shape)
    every = _wanted(pm)
    grad = A.rollout_data_gradient(th, gu, gth, want=every)
    _same_dict(grad, _restated(dict(pat=pat, pm=pm, om=om, fm=fm, got=got, recs=recs), gu, gth, want=every), "cap")
    g0, _ = A.rollout_gradient(gu, gth)
    # (rollout_gradient: a NaN step t >= 1 reaches grad_theta0 through lambda, one of step 0 through J_0 itself)
    bad = np.isnan(g0).any(axis=1)
    assert np.array_equal(bad, ~ok.all(axis=1)) and bad.any() and (~bad).any()
    for q in every:
        if q not in ("grad_u0", "grad_Uval"):
            assert np.all(np.isnan(grad[q][bad])) and np.all(np.isfinite(grad[q][~bad])), q
    A.close()


@pytest.mark.gpu
@pytest.mark.parametrize("env,launches", [({}, 1), ({"EICOS_FUSED_UPDATE": "0"}, 3)])
def test_a_step_whose_fallback_fired_has_zero_rows(env, launches, monkeypatch):
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    (A, E), fm, theta0, w, T, B, iters0 = RJ._capped_handles(2)
    A.set_settings(iter_max=int(iters0.min()))
    A.set_fallback_map(_fbmap(7, 6, mask=eicos_amd.SEL_ALL & ~(eicos_amd.SEL_OPTIMAL | eicos_amd.SEL_OPTIMAL_INACC)))
    A.set_rollout_recording(True)
    got = A.rollout_jacobian(theta0, T, w)
    assert A.last_rollout_launches() == launches
    codes = got[2]
    fired = ~((codes == 0) | (codes == 10))
    assert fired.any() and (~fired).any() and A.fallback_counts().sum() == fired.sum()
    recs = A.rollout_records()
    for Wg in recs[:3]:
        assert np.all(Wg[fired] == 0.0) and np.all(np.isfinite(Wg)) and np.abs(Wg[~fired]).max() > 0
    assert all(np.all(np.isfinite(a)) for a in recs[3:]) and np.abs(recs[3][fired]).max() > 0  # x, y, z all the same
    # a mask that fires everywhere: the loop does not depend on the controller's data at all
    E.set_fallback_map(_fbmap(7, 6, mask=eicos_amd.SEL_ALL))
    E.set_rollout_recording(True)
    out = E.rollout_jacobian(theta0, T, w)
    grad = E.rollout_data_gradient(out[1], gu=np.ones_like(out[0]), want=("grad_c", "grad_h", "grad_G"))
    for q, a in grad.items():
        assert np.all(a == 0.0), q
    A.close(); E.close()


@pytest.mark.gpu
def test_refusals_move_nothing():
    B, k, r, T = 4, 3, 4, 2
    pat, d = P._data("lp_afiro", B)
    g = eicos_amd.BatchSolver(pat, B)
    g.update(*[d[k_] for k_ in KEYS]); g.solve()
    L = binding._lib()
    err = lambda: L.eicos_last_error().decode()
    pm, om, fm = P._map(d, k, groups="ch"), _omap(pat.n, r), RO._fmap(k, r)  # (no map of the b group)
    g.set_param_map(pm); g.set_output_map(om); g.set_plant_map(fm)
    theta0 = P._theta(B, k)
    SENT = -7.25
    gu, gth = np.ones((B, T, r)), np.ones((B, T + 1, k))
    outs = {"grad_c": np.full((B, pat.n), SENT), "grad_Bval": np.full((B, 4), SENT), "grad_Cval": np.full((B, int(pm.c[1][-1])), SENT)}
    p = lambda a: None if a is None else a.ctypes.data_as(DP)

    def grad(a=gu, b=gth, th="traj", names=("grad_c",), fn=L.eicos_batch_rollout_data_gradient, st=None):
        st = st if st is not None else DataGradient(**{q: outs[q].ctypes.data for q in names})
        return fn(g._h, p(a), p(b), p(traj if isinstance(th, str) else th), C.byref(st))

    traj = np.zeros((B, T + 1, k))
    with pytest.raises(RuntimeError, match="no Jacobian trajectory"):
        g.rollout_data_gradient(traj, gu=gu)
    assert grad() == -1 and "no Jacobian trajectory" in err()
    # a rollout with recording off: a trajectory, but no rows
    traj = g.rollout_jacobian(theta0, T)[1]
    assert grad() == -1 and "no recorded rows" in err()
    assert L.eicos_batch_rollout_records(g._h, p(np.zeros(B * T * r * pat.n)), None, None, None, None, None) == -1 and "no recorded rows" in err()
    g.set_rollout_recording(True)
    assert grad() == -1 and "no recorded rows" in err()  # (switching it on records nothing by itself)
    traj = g.rollout_jacobian(theta0, T)[1]
    before = AD._state(g)
    assert grad() == 0 and not np.any(outs["grad_c"] == SENT)
    outs["grad_c"][...] = SENT
    assert grad(a=None, b=None) == -1 and "both NULL" in err()
    assert grad(th=None) == -1 and "theta_traj is NULL" in err()
    assert L.eicos_batch_rollout_data_gradient(g._h, p(gu), None, p(traj), None) == -1 and "out is NULL" in err()
    assert grad(st=DataGradient()) == -1 and "every output" in err()
    assert grad(names=("grad_c", "grad_Bval")) == -1 and "no b group" in err()
    dev = AM._device_doubles(gth.size)
    dptr, vptr = C.cast(dev, DP), C.c_void_p(gu.ctypes.data)
    assert L.eicos_batch_rollout_data_gradient(g._h, dptr, None, p(traj), C.byref(DataGradient(grad_c=outs["grad_c"].ctypes.data))) == -1 and "host pointers" in err()
    assert grad(st=DataGradient(grad_c=C.cast(dev, C.c_void_p).value)) == -1 and "host pointers" in err()
    assert L.eicos_batch_rollout_data_gradient_device(g._h, vptr, None, dev, C.byref(DataGradient(grad_c=C.cast(dev, C.c_void_p).value))) == -1 and "device memory" in err()
    assert L.eicos_batch_rollout_data_gradient_device(g._h, dev, None, dev, C.byref(DataGradient(grad_c=outs["grad_c"].ctypes.data))) == -1 and "device memory" in err()
    L.hipFree(dev)
    # a map installed after the rollout: the records no longer belong to the handle's maps
    g.set_output_map(om)
    assert grad() == -1 and "installed after the rollout" in err()
    for a in outs.values():
        assert np.all(a == SENT)
    assert L.eicos_batch_rollout_jacobian_steps(g._h) == T
    AD._assert_same(AD._state(g), before, "after the refusals of rollout_data_gradient")
    traj = g.rollout_jacobian(theta0, T)[1]
    assert grad(names=("grad_c", "grad_Cval")) == 0 and not np.any(outs["grad_c"] == SENT) and not np.any(outs["grad_Cval"] == SENT)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("devs", [[0, 0], [0, 0, 0]])
def test_multi_forms_match_one_handle(devs):
    B, k, r, T = 5, 5, 4, 2
    pat, d = P._data("MPC02", B)
    pm, om, fm = P._map(d, k), _omap(pat.n, r), RO._fmap(k, r)
    eicos_amd.set_arithmetic_profile(1)
    try:
        one = eicos_amd.BatchSolver(pat, B)
        m = eicos_amd.MultiBatchSolver(pat, B, devs)
        for s in (one, m):
            s.update(*[d[k_] for k_ in KEYS]); s.solve()
            s.set_param_map(pm); s.set_output_map(om); s.set_plant_map(fm)
            s.set_rollout_recording(True)
            assert s.rollout_recording()
        theta0, w = P._theta(B, k), RO._w(B, T, k)
        want = one.rollout_jacobian(theta0, T, w)
        got = m.rollout_jacobian(theta0, T, w)
        RJ._assert_six(got, want, devs)
        for q, (a, b) in enumerate(zip(m.rollout_records(), one.rollout_records())):
            _same(a, b, (devs, REC[q]))
        rng = np.random.default_rng(2)
        gu, gth = rng.standard_normal(want[0].shape), rng.standard_normal(want[1].shape)
        every = _wanted(pm)
        for a, b in ((gu, None), (gu, gth)):
            _same_dict(m.rollout_data_gradient(want[1], a, b, want=every), one.rollout_data_gradient(want[1], a, b, want=every), devs)
        m.close(); one.close()
    finally:
        eicos_amd.set_arithmetic_profile(0)
