"""Adjoint sensitivities (eicos_batch_adjoint, _output_jacobian / _device and their eicos_multi_* forms; include/eicos_amd.h):
the gradient of g'x with respect to (c, h, b) at the iterate a solve returned, and the Jacobian of the output map through the
parameter map.

Every test goes through ONE numpy reference (_Reference): the dense K of the definition from the caller's data and the NT scaling
nt_w2(s, z), scaled symmetrically by D_i = 1 / sqrt(max_j |K_ij|), solved by LAPACK.  A dense comparison asserts cond(scaled K) <= 1e4
itself, so that an ill-posed input cannot pass as agreement.  The CPU test pins the definition (sign, formula, D) against central
differences of the CPU oracle; the GPU tests compare the library with the reference, check that the Jacobian form is the host
contraction of the gradient form, take the hard case (a cone active at the optimum, cond 1e10 and more) against the oracle's central
difference, and check that an adjoint call moves nothing a later call reads.

Measured on one MI355X (docs/HISTORY.md A.21): dense parity 5e-16 ... 6e-13 of the 1e-8 bound (grad_c, the small vector, is the
worst), res 1e-16 ... 5e-15; Jacobian 4e-16 ... 2e-15 from the reference; active cone: GPU 8.5e-7 ... 1.3e-4 |fd| from the central
difference with the numpy reference 8.7e-7 ... 1.2e-4 |fd| from it."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse
import scipy.sparse.linalg

import eicos_amd
from eicos_amd import binding
from eicos_amd.binding import MatrixMap, OutputMap, ParamMap, ShiftMap
from eicos_amd.generate import feasible_batch, random_socp_pattern
from eicos_amd.problem_io import Values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KEYS = ("Gpr", "Apr", "c", "h", "b")
INFO_SKIP = ("solve_us",)  # (a time)
COND_MAX = 1e4
EPS = np.finfo(np.float64).eps
W2 = {"EICOS_UBL": "0", "EICOS_THREADS": "256"}
DEF256 = {"EICOS_UBL": "0", "EICOS_THREADS": "256", "EICOS_W2": "0"}
NOLDS = {"EICOS_NLDS": "0", "EICOS_DUAL": "0"}
VERTEX = {"vertex-small": (10, 3, 12, [3, 5]), "vertex-mid": (30, 6, 40, [4, 7])}
# the seeds of the active-cone instances: seed 2 of the small pattern draws active rows that do not pin a vertex (cond 4e16 at the oracle's
# iterate, the numpy reference itself 2e4 |fd| away from the oracle's central difference) -- not a member of the family, so seed 3 stands in
ACTIVE_SEEDS = {"vertex-small": (1, 3), "vertex-mid": (1, 2)}


# ---- the numpy reference ------------------------------------------------------------------------------------------------------------
def nt_w2(pat, s, z):
    """The squared NT scaling W^2 of (s, z) as a dense m x m matrix: s_i / z_i on an LP row; per second-order cone eta^2 Wbar^2 with
    Wbar = [[a, q'], [q, I + q q' / (1 + a)]] of the normalised points (W^2 z = s)."""
    W2m = np.zeros((pat.m, pat.m))
    i = np.arange(pat.l)
    W2m[i, i] = s[: pat.l] / z[: pat.l]
    o = pat.l
    for d in (int(v) for v in pat.q):
        sc, zc = s[o:o + d], z[o:o + d]
        sn, zn = np.sqrt(sc[0] ** 2 - sc[1:] @ sc[1:]), np.sqrt(zc[0] ** 2 - zc[1:] @ zc[1:])
        sb, zb = sc / sn, zc / zn
        gam = np.sqrt(0.5 * (1.0 + sb @ zb))
        a, q = 0.5 / gam * (sb[0] + zb[0]), 0.5 / gam * (sb[1:] - zb[1:])
        Wb = np.empty((d, d))
        Wb[0, 0], Wb[0, 1:], Wb[1:, 0] = a, q, q
        Wb[1:, 1:] = np.eye(d - 1) + np.outer(q, q) / (1.0 + a)
        W2m[o:o + d, o:o + d] = (sn / zn) * (Wb @ Wb)
        o += d
    return W2m


def _dense(pat, v):
    G = scipy.sparse.csc_matrix((v.Gpr, pat.Gir, pat.Gjc), shape=(pat.m, pat.n)).toarray()
    A = scipy.sparse.csc_matrix((v.Apr, pat.Air, pat.Ajc), shape=(pat.p, pat.n)).toarray()
    return G, A


class _Reference:
    """K of the definition for one instance at (s, z), scaled and factorised once: solve(rhs) = K^-1 rhs for columns rhs [N, cols];
    grads(g) = (grad_c, grad_h, grad_b) for rows g [nrhs, n]; cond = the 2-norm condition number of the scaled matrix."""

    def __init__(self, pat, vals, s, z):
        n, p, m = pat.n, pat.p, pat.m
        G, A = _dense(pat, vals)
        K = np.zeros((n + p + m, n + p + m))
        K[:n, n:n + p], K[:n, n + p:] = A.T, G.T
        K[n:n + p, :n], K[n + p:, :n] = A, G
        K[n + p:, n + p:] = -nt_w2(pat, s, z)
        self.pat, self.D = pat, 1.0 / np.sqrt(np.abs(K).max(axis=1))
        Ks = self.D[:, None] * K * self.D[None, :]
        self.lu = scipy.linalg.lu_factor(Ks)
        if Ks.shape[0] <= 1500:
            self.cond = np.linalg.cond(Ks)
        else:  # (symmetric: the singular values are the |eigenvalues|; the extreme ones from sparse Lanczos runs instead of a dense SVD)
            Ksp = scipy.sparse.csc_matrix(Ks)
            big = abs(scipy.sparse.linalg.eigsh(Ksp, k=1, which="LM", return_eigenvectors=False)[0])
            small = abs(scipy.sparse.linalg.eigsh(Ksp, k=1, sigma=0.0, which="LM", return_eigenvectors=False)[0])
            self.cond = big / small

    def solve(self, rhs):
        return self.D[:, None] * scipy.linalg.lu_solve(self.lu, self.D[:, None] * rhs)

    def grads(self, g):
        n, p = self.pat.n, self.pat.p
        rhs = np.zeros((self.D.size, g.shape[0]))
        rhs[:n] = g.T
        w = self.solve(rhs)
        return -w[:n].T, w[n + p:].T, w[n:n + p].T


def _directional(grads, dc, dh, db):
    gc, gh, gb = grads
    return gc @ dc + gh @ dh + gb @ db


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
_DATA = {}


def vertex_instance(pat, base, seed, active_cone=False):
    """The inactive-cone vertex family: x0, y0 random, n - p random LP rows active (s = 0, z in U(0.5, 1.5)), the others slack
    (s in U(0.5, 1.5), z = 0), every cone strictly inside (s = (2 |t| + 0.5, t), z = 0); h = G x0 + s0, b = A x0, c = -A'y0 - G'z0: a
    unique, strictly complementary optimum at x0.  active_cone: the first cone strictly complementary ON its boundary instead
    (s = (|t|, t), z = 0.7 (|t|, -t)) and one active LP row fewer."""
    rng = np.random.default_rng(seed)
    G, A = _dense(pat, base)
    x0, y0 = rng.standard_normal(pat.n), rng.standard_normal(pat.p)
    s0, z0 = np.zeros(pat.m), np.zeros(pat.m)
    nact = pat.n - pat.p - (1 if active_cone else 0)
    act = np.zeros(pat.l, bool)
    act[rng.choice(pat.l, nact, replace=False)] = True
    z0[: pat.l][act] = rng.uniform(0.5, 1.5, nact)
    s0[: pat.l][~act] = rng.uniform(0.5, 1.5, pat.l - nact)
    o = pat.l
    for ci, d in enumerate(int(v) for v in pat.q):
        t = rng.standard_normal(d - 1)
        nt = np.linalg.norm(t)
        if active_cone and ci == 0:
            s0[o], s0[o + 1:o + d] = nt, t
            z0[o], z0[o + 1:o + d] = 0.7 * nt, -0.7 * t
        else:
            s0[o], s0[o + 1:o + d] = 2.0 * nt + 0.5, t
        o += d
    return Values(base.Gpr, base.Apr, -(A.T @ y0) - (G.T @ z0), G @ x0 + s0, A @ x0)


def _data(name, B, active_cone=False):
    """(pattern, dict of [B, ...] arrays): feasible_batch instances 0 .. B-1 of a fixture, or seeds 1 .. B of a vertex pattern
    (active_cone: ACTIVE_SEEDS)."""
    key = (name, B, active_cone)
    if key not in _DATA:
        if name in VERTEX:
            n, p, l, q = VERTEX[name]
            pat, base = random_socp_pattern(n, p, l, q, seed=5)
            vs = [vertex_instance(pat, base, seed, active_cone) for seed in (ACTIVE_SEEDS[name][:B] if active_cone else range(1, B + 1))]
            d = {k: np.stack([getattr(v, k) for v in vs]) for k in KEYS}
        else:
            pat, sets = eicos_amd.read_epb(os.path.join(GOLDEN, name + ".epb"))
            d = feasible_batch(pat, sets[0], 0, B)
        _DATA[key] = (pat, d)
    return _DATA[key]


def _vals(d, i):
    return Values(*[d[k][i] for k in KEYS])


def _oracle_x(pat, v):
    from oracle.oracle import OracleSolver
    o = OracleSolver(pat, v)
    code = o.solve()
    x, (y, z, s) = o.x().copy(), [a.copy() for a in o.yzs()]
    o.close()
    return code, x, y, z, s


def _oracle_fd(pat, v, g, dc, dh, db, eps=1e-5):
    """Central difference of g'x of the oracle's solution along (dc, dh, db), default settings."""
    xs = []
    for sg in (1.0, -1.0):
        code, x, *_ = _oracle_x(pat, Values(v.Gpr, v.Apr, v.c + sg * eps * dc, v.h + sg * eps * dh, v.b + sg * eps * db))
        assert code == 0, code
        xs.append(x)
    return g @ (xs[0] - xs[1]) / (2.0 * eps)


def _direction(pat, seed):
    rng = np.random.default_rng(1000 + seed)
    return rng.standard_normal(pat.n), rng.standard_normal(pat.n), rng.standard_normal(pat.m), rng.standard_normal(pat.p)


# ---- CPU: the definition --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lp_afiro", "lp_blend", "vertex-small", "vertex-mid"])
def test_reference_is_the_derivative_of_the_oracle(name):
    # sign-and-formula check: a wrong sign or a missing D is an O(1) error; measured 9e-11 ... 4e-7 on these inputs, the bound is 1e-3
    pat, d = _data(name, 2)
    for i in range(2):
        v = _vals(d, i)
        code, x, y, z, s = _oracle_x(pat, v)
        assert code == 0
        ref = _Reference(pat, v, s, z)
        assert ref.cond <= COND_MAX, (name, i, ref.cond)
        g, dc, dh, db = _direction(pat, i)
        want = _oracle_fd(pat, v, g, dc, dh, db)
        got = _directional(ref.grads(g[None, :]), dc, dh, db)[0]
        rel = abs(got - want) / abs(want)
        print(name, i, "cond", ref.cond, "reference", got, "central difference", want, "relative distance", rel)
        assert rel <= 1e-3, (name, i, got, want)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
def _handle(pat, d, B, build=None):
    g = eicos_amd.BatchSolver(pat, B)
    if build == "no-lds":
        assert g.dims()["lds_bytes"] == 0
    elif build is not None:
        assert (g.kernel_build(), g.dims()["threads_per_block"]) == build, (g.kernel_build(), g.dims()["threads_per_block"])
    g.update(*[d[k] for k in KEYS])
    return g


def _setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _gpu_reference(pat, d, g, i):
    """The reference at the iterate the GPU returned for instance i."""
    (y, z, s) = g.duals()
    return _Reference(pat, _vals(d, i), s[i], z[i])


def _random_rows(pat, B, nrhs, seed=7):
    return np.random.default_rng(seed).standard_normal((B, nrhs, pat.n))


PARITY = [
    ("lp_afiro", 8, {}, ("lds-resident", 128), None),
    ("MPC02", 4, W2, ("w2", 256), [0]),  # (a 5991^2 dense solve per instance: instance 0 only)
    ("MPC02", 4, DEF256, ("default", 256), [0]),
    ("MPC02", 4, {"EICOS_UBL": "0", "EICOS_W2": "0", "EICOS_THREADS": "128"}, ("default", 128), [0]),
    ("MPC02", 4, {"EICOS_UBL": "0", "EICOS_W2": "0", "EICOS_THREADS": "512"}, ("default", 512), [0]),
    ("u-in-lds", 4, {"EICOS_THREADS": "256"}, ("u-in-lds", 256), None),  # (lp_adlittle or lp_blend: whichever the handle reports as U in LDS)
    ("MPC02", 4, NOLDS, "no-lds", [0]),
    ("lp_bandm", 2, {}, None, None),                        # the hybrid factor path
    ("vertex-small", 2, {"EICOS_TILES": "1"}, None, None),  # the tile path
    ("vertex-small", 2, {}, None, None),                    # cones on the scalar path
    ("vertex-mid", 2, {}, None, None),
]
_REF = {}  # (name, instance) -> _Reference at the iterate of the first handle that solved it (every build returns it to 1e-8 and better)


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,env,build,check", PARITY)
def test_gradients_match_the_dense_reference_on_every_build(name, B, env, build, check, monkeypatch):
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
    else:
        pat, d = _data(name, B)
        g = _handle(pat, d, B, build)
    codes = g.solve()
    assert np.all(codes == 0), codes
    rows = _random_rows(pat, B, 2)
    gc, gh, gb, res = g.adjoint(rows)
    assert gc.shape == (B, 2, pat.n) and gh.shape == (B, 2, pat.m) and gb.shape == (B, 2, pat.p) and res.shape == (B, 2)
    assert np.all(np.isfinite(res)), res
    print(name, env, g.kernel_build(), "res", res.min(), "...", res.max())
    for i in (range(B) if check is None else check):
        ref = _gpu_reference(pat, d, g, i)
        assert ref.cond <= COND_MAX, (name, i, ref.cond)
        want = ref.grads(rows[i])
        for what, got, w in zip(("grad_c", "grad_h", "grad_b"), (gc[i], gh[i], gb[i]), want):
            for r in range(2):
                if w.shape[1] == 0:
                    continue
                dist, scale = np.max(np.abs(got[r] - w[r])), np.max(np.abs(w[r]))
                print(name, "instance", i, what, "row", r, "distance", dist, "relative", dist / scale, "cond", ref.cond)
                assert dist <= 1e-8 * scale, (name, env, i, what, r, dist, scale)
    g.close()


def _random_maps(pat, k=3, r=2, seed=11):
    """Random sparse maps: every row of C, H, B has 0 .. 2 entries in distinct columns of the k, every row of U four entries in distinct columns."""
    rng = np.random.default_rng(seed)

    def group(rows, cols, per_row):
        rowptr, col, val = [0], [], []
        for _ in range(rows):
            c = np.sort(rng.choice(cols, min(cols, per_row()), replace=False))
            col += list(c); val += list(rng.standard_normal(c.size)); rowptr.append(len(col))
        return (rng.standard_normal(rows), np.asarray(rowptr, np.int32), np.asarray(col, np.int32), np.asarray(val, np.float64))

    few = lambda: int(rng.integers(0, 3))
    pmap = ParamMap(k, c=group(pat.n, k, few), h=group(pat.m, k, few), b=group(pat.p, k, few) if pat.p else None)
    omap = OutputMap(pat.n, group(r, pat.n, lambda: 4))
    return pmap, omap


def _csr_dense(grp, cols):
    base, rowptr, col, val = grp
    M = np.zeros((base.size, cols))
    for j in range(base.size):
        for t in range(rowptr[j], rowptr[j + 1]):
            M[j, col[t]] += val[t]
    return M


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,env,build,check", [PARITY[0], PARITY[1], PARITY[9]])
def test_output_jacobian_is_the_contraction_of_the_gradients(name, B, env, build, check, monkeypatch):
    _setenv(monkeypatch, env)
    pat, d = _data(name, B)
    g = _handle(pat, d, B, build)
    k, r = 3, 2
    pmap, omap = _random_maps(pat, k, r)
    g.set_param_map(pmap); g.set_output_map(omap)
    assert np.all(g.solve() == 0)
    U = _csr_dense((omap.base, omap.rowptr, omap.col, omap.val), pat.n)
    Cm, Hm = _csr_dense(pmap.c, k), _csr_dense(pmap.h, k)
    Bm = _csr_dense(pmap.b, k) if pmap.b is not None else np.zeros((0, k))
    J, res = g.output_jacobian()
    Jd, resd = g.output_jacobian(device=True)
    assert J.shape == (B, r, k) and np.all(np.isfinite(res))
    assert np.array_equal(J, Jd) and np.array_equal(res, resd)  # the device form: the same bits
    gc, gh, gb, res2 = g.adjoint(np.broadcast_to(U, (B, r, pat.n)).copy())
    assert np.array_equal(res, res2)  # (the same right-hand sides through the same solve)
    nnz = np.maximum(1, (Cm != 0).sum(0) + (Hm != 0).sum(0) + (Bm != 0).sum(0))  # terms of a column's sum
    for i in range(B):
        host = gc[i] @ Cm + gh[i] @ Hm + gb[i] @ Bm
        bound = 4.0 * nnz * EPS * (np.abs(gc[i]) @ np.abs(Cm) + np.abs(gh[i]) @ np.abs(Hm) + np.abs(gb[i]) @ np.abs(Bm))
        assert np.all(np.abs(J[i] - host) <= bound), (name, i, np.abs(J[i] - host).max(), bound.min())
    for i in (range(B) if check is None else check):
        ref = _gpu_reference(pat, d, g, i)
        assert ref.cond <= COND_MAX
        rhs = np.concatenate([-Cm, Bm, Hm])  # K^-1 [-C; B; H]: the columns d(x, y, z) / d theta
        want = U @ ref.solve(rhs)[: pat.n]
        dist = np.max(np.abs(J[i] - want))
        print(name, "instance", i, "max |J - ref|", dist, "max |J|", np.max(np.abs(want)))
        assert dist <= 1e-8 * np.max(np.abs(want)), (name, i, dist)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["vertex-small", "vertex-mid"])
def test_active_cone_against_the_oracle_central_difference(name):
    """A cone strictly complementary on its boundary: cond(scaled K) is 2e10 ... 1e13 at the returned iterate, so there is no dense
    comparison.  The yardstick is the oracle's central difference fd; the numpy reference sits d_ref = 3e-6 ... 4e-4 (relative) from
    it, and the GPU must sit within 4 d_ref + 1e-6 |fd| of the same fd."""
    B = 2
    pat, d = _data(name, B, active_cone=True)
    g = _handle(pat, d, B)
    assert np.all(g.solve() == 0)
    dirs = [_direction(pat, 50 + i) for i in range(B)]
    gc, gh, gb, res = g.adjoint(np.stack([dr[0] for dr in dirs])[:, None, :])
    for i in range(B):
        gvec, dc, dh, db = dirs[i]
        fd = _oracle_fd(pat, _vals(d, i), gvec, dc, dh, db)
        ref = _directional(_gpu_reference(pat, d, g, i).grads(gvec[None, :]), dc, dh, db)[0]
        got = gc[i, 0] @ dc + gh[i, 0] @ dh + gb[i, 0] @ db
        d_ref = abs(ref - fd)
        assert d_ref <= 1e-3 * abs(fd), (name, i, ref, fd)  # (the yardstick itself: the definition holds on this instance)
        print(name, "instance", i, "fd", fd, "gpu", got, "|gpu - fd|", abs(got - fd), "d_ref", d_ref, "res", res[i, 0])
        assert abs(got - fd) <= 4.0 * d_ref + 1e-6 * abs(fd), (name, i, got, fd, ref)
    g.close()


def _state(g):
    """Everything the host can read of every instance: every info field but the time, x, y, z, s, and the retry counts."""
    ia = g.info_arrays()
    y, z, s = g.duals()
    return {"x": g.solution(), "y": y, "z": z, "s": s, "retries": g.retry_counts(), **{"info." + k: v for k, v in ia.items() if k not in INFO_SKIP}}


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,env,build", [("MPC02", 4, W2, ("w2", 256)), ("lp_afiro", 8, {}, ("lds-resident", 128)), ("MPC02", 4, NOLDS, "no-lds")])
def test_an_adjoint_call_moves_nothing(name, B, env, build, monkeypatch):
    _setenv(monkeypatch, env)
    pat, d = _data(name, B)
    pmap, omap = _random_maps(pat)
    ident = (np.full(pat.n, 1e-3), np.arange(pat.n + 1, dtype=np.int32), np.arange(pat.n, dtype=np.int32), np.ones(pat.n))
    twins = [_handle(pat, d, B, build) for _ in range(2)]
    for g in twins:
        g.set_param_map(pmap); g.set_output_map(omap)
        g.solve()
    before = _state(twins[0])
    _assert_same(before, _state(twins[1]), (name, "twins after the first solve"))
    twins[0].adjoint(_random_rows(pat, B, 2))
    twins[0].output_jacobian()
    twins[0].adjoint(_random_rows(pat, 2, 1), idx=[B - 1, 0])
    _assert_same(_state(twins[0]), before, (name, "before and after the adjoint calls"))
    rng = np.random.default_rng(3)
    c2, h2 = d["c"] * (1 + 1e-3 * rng.standard_normal(d["c"].shape)), d["h"] + 1e-3 * rng.uniform(0, 1, d["h"].shape)
    for g in twins:  # the second solve: warm-started through a shift map
        g.set_warm_start(1e-3); g.set_shift_map(ShiftMap(pat.n, pat.p, pat.m, x=ident))
        g.update_rhs(c=c2, h=h2)
        g.solve()
    _assert_same(_state(twins[0]), _state(twins[1]), (name, "twins after the warm second solve"))
    for g in twins:
        g.close()


@pytest.mark.gpu
def test_subset_ineligible_instances_and_refusals(monkeypatch):
    B, name = 8, "MPC02"
    pat, d = _data(name, B)
    g = _handle(pat, d, B)
    g.set_settings(iter_max=ITER_CAP)
    codes = g.solve()
    ok = (codes == 0) | (codes == 10)
    print("exit codes under iter_max", ITER_CAP, codes)
    assert ok.any() and (~ok).any(), codes  # (the cap is chosen so that the batch splits)
    rows = _random_rows(pat, B, 2)
    gc, gh, gb, res = g.adjoint(rows)
    for a in (gc, gh, gb, res):
        assert np.all(np.isnan(a[~ok])) and np.all(np.isfinite(a[ok]))
    idx = [B - 1, 0, 3, 2]
    sub = g.adjoint(rows[idx], idx=idx)
    for a, w in zip(sub, (gc, gh, gb, res)):
        assert np.array_equal(a, w[idx], equal_nan=True)
    L, ip, dp = binding._lib(), C.POINTER(C.c_int), C.POINTER(C.c_double)
    err = lambda: L.eicos_last_error().decode()
    buf = np.zeros(B * 65 * max(pat.n, pat.m)).ctypes.data_as(dp)
    ids = lambda v: np.asarray(v, np.int32).ctypes.data_as(ip)
    before = _state(g)
    assert L.eicos_batch_adjoint(g._h, ids([1, 1]), 2, 1, buf, buf, None, None, None) != 0 and "duplicate index 1" in err()
    assert L.eicos_batch_adjoint(g._h, ids([1, B]), 2, 1, buf, buf, None, None, None) != 0 and "outside" in err()
    for nrhs in (0, 65):
        assert L.eicos_batch_adjoint(g._h, None, B, nrhs, buf, buf, None, None, None) != 0 and "nrhs" in err()
    assert L.eicos_batch_output_jacobian(g._h, None, B, buf, None) != 0 and "parameter map and an output map" in err()
    pmap, omap = _random_maps(pat)
    g.set_param_map(pmap)
    assert L.eicos_batch_output_jacobian(g._h, None, B, buf, None) != 0 and "parameter map and an output map" in err()
    g.set_output_map(omap)
    J, _ = g.output_jacobian()
    assert np.all(np.isnan(J[~ok])) and np.all(np.isfinite(J[ok]))
    Js, _ = g.output_jacobian(idx=idx)
    assert np.array_equal(Js, J[idx], equal_nan=True)
    assert L.eicos_batch_output_jacobian(g._h, ids([0, 0]), 2, buf, None) != 0 and "duplicate index 0" in err()
    one = (np.zeros(pat.nnzG), np.arange(pat.nnzG + 1, dtype=np.int32), np.zeros(pat.nnzG, np.int32), np.full(pat.nnzG, 1e-9))
    g.set_matrix_map(MatrixMap(3, G=(d["Gpr"][0].copy(),) + one[1:]))
    assert L.eicos_batch_output_jacobian(g._h, None, B, buf, None) != 0 and "matrix map" in err() and "dG" in err()
    _assert_same(_state(g), before, "after the refusals")
    g.close()


ITER_CAP = 12  # MPC02 instances 0 .. 7 of feasible_batch need 11 ... 14 passes under the defaults: some end under the cap, some at it


@pytest.mark.gpu
def test_multi_output_jacobian_equals_the_single_handle():
    B, name = 5, "lp_afiro"
    pat, d = _data(name, 8)
    d = {k: v[:B] for k, v in d.items()}
    pmap, omap = _random_maps(pat)
    eicos_amd.set_arithmetic_profile(1)  # (plans by the pattern alone: a shard gives the bits of the batch)
    try:
        single = eicos_amd.BatchSolver(pat, B)
        multi = eicos_amd.MultiBatchSolver(pat, B, [0, 0])
    finally:
        eicos_amd.set_arithmetic_profile(0)
    for g in (single, multi):
        g.update(*[d[k] for k in KEYS])
        g.set_param_map(pmap); g.set_output_map(omap)
        assert np.all(g.solve() == 0)
    J, res = single.output_jacobian()
    Jm, resm = multi.output_jacobian()
    assert np.array_equal(J, Jm) and np.array_equal(res, resm)
    idx = [4, 1, 2]
    Jm, resm = multi.output_jacobian(idx=idx)
    assert np.array_equal(J[idx], Jm) and np.array_equal(res[idx], resm)
    rows = _random_rows(pat, B, 2)
    for a, b in zip(single.adjoint(rows), multi.adjoint(rows)):
        assert np.array_equal(a, b)
    for g in (single, multi):
        g.close()
