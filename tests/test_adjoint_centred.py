"""The re-centred cone scaling of the adjoint (eicos_batch_set_adjoint_scaling, EICOS_ADJOINT_CENTRED; include/eicos_amd.h, DESIGN.md 4.1,
docs/HISTORY.md A.32): K of the adjoint with the NT scaling of centred_pair(s, z) instead of (s, z).

Where an active second-order cone's curvature fixes the optimum -- fewer active LP rows than n - p - 1, so that the optimum can slide on
the cone's surface -- the NT scaling of the returned pair has eta^2 wrong by the ratio of the two complementary products, whatever
centrality error the last step left.  The CPU tests hold the numpy restatement (binding.centred_pair in _Reference of test_adjoint.py)
against central differences of the CPU oracle on ten such instances, on which the NT reference is 0.16 ... 7.6 |fd| away; the GPU
tests hold the library against the restatement on well-conditioned off-centre pairs (every build, every cone class), against the
oracle's central difference on four of the ten, and check that the default moves nothing, that the fused rollout Jacobian still is its
host twin bit for bit, the multi-GPU form, and the refusals.

Bounds: 5e-3 |fd| for the restatement against fd(1e-5) (the difference's own spread, asserted at 1e-3 |fd| between eps = 1e-5 and
1e-4, and the worst distance measured on the CPU, 1.5e-3); 1e-8 of a row's largest entry for the dense comparison at cond <= 1e4, as
in test_adjoint.py; 4 d_ref + 1e-6 |fd| for the GPU on the curvature cases, as in its active-cone test.

Measured on one MI355X (docs/HISTORY.md A.32): dense comparison 2.4e-16 ... 3.3e-14 of the 1e-8 bound's scale at cond 22 ... 325, res
2.9e-17 ... 2.4e-16, NT and centred 5.1e-2 ... 5.3e-1 apart on the same rows; curvature cases: GPU 1.4e-6 ... 2.1e-5 |fd| from the
central difference with the restatement at the GPU's iterate 1.6e-6 ... 6.6e-5 |fd| from it, the NT mode 0.16 ... 2.2 |fd|."""
import numpy as np
import pytest

import eicos_amd
from eicos_amd import binding
from eicos_amd.binding import centred_pair
from eicos_amd.generate import random_socp_pattern
from eicos_amd.problem_io import Values
from test_adjoint import (COND_MAX, DEF256, KEYS, NOLDS, VERTEX, W2, _Reference, _assert_same, _dense, _direction, _directional, _handle,
                          _oracle_fd, _oracle_x, _random_maps, _random_rows, _setenv, _state, _vals)

# (pattern, the cone on its boundary, active LP rows fewer than n - p, seed): the ten instances on which the curvature of the active
# cone fixes the optimum
CURVATURE = [
    ("vertex-small", 0, 2, 4), ("vertex-small", 1, 2, 1), ("vertex-small", 1, 3, 1), ("vertex-small", 1, 3, 2),
    ("vertex-mid", 0, 2, 4), ("vertex-mid", 0, 3, 3), ("vertex-mid", 1, 2, 2), ("vertex-mid", 1, 3, 1), ("vertex-mid", 1, 3, 2),
    ("vertex-mid", 1, 3, 3),
]
GPU_CURVATURE = {"vertex-small": [CURVATURE[0], CURVATURE[2]], "vertex-mid": [CURVATURE[5], CURVATURE[8]]}
CLASSES = "class-edges"  # one cone on each side of every class boundary of the per-cone loops (tests/test_cone_classes.py)
CLASS_DIMS = (24, 4, 30, [2, 4, 5, 31, 32, 64, 65])
_PAT, _CASE = {}, {}


def _pattern(name):
    if name not in _PAT:
        n, p, l, q = CLASS_DIMS if name == CLASSES else VERTEX[name]
        _PAT[name] = random_socp_pattern(n, p, l, q, density=0.3, seed=5) if name == CLASSES else random_socp_pattern(n, p, l, q, seed=5)
    return _PAT[name]


def curvature_instance(pat, base, seed, cone, fewer):
    """vertex_instance of test_adjoint.py generalised, the same draws in the same order: n - p - fewer LP rows active, the cone with
    index `cone` strictly complementary on its boundary (s = (|t|, t), z = 0.7 (|t|, -t)), the other cones strictly inside."""
    rng = np.random.default_rng(seed)
    G, A = _dense(pat, base)
    x0, y0 = rng.standard_normal(pat.n), rng.standard_normal(pat.p)
    s0, z0 = np.zeros(pat.m), np.zeros(pat.m)
    nact = pat.n - pat.p - fewer
    act = np.zeros(pat.l, bool)
    act[rng.choice(pat.l, nact, replace=False)] = True
    z0[: pat.l][act] = rng.uniform(0.5, 1.5, nact)
    s0[: pat.l][~act] = rng.uniform(0.5, 1.5, pat.l - nact)
    o = pat.l
    for ci, d in enumerate(int(v) for v in pat.q):
        t = rng.standard_normal(d - 1)
        nt = np.linalg.norm(t)
        if ci == cone:
            s0[o], s0[o + 1:o + d] = nt, t
            z0[o], z0[o + 1:o + d] = 0.7 * nt, -0.7 * t
        else:
            s0[o], s0[o + 1:o + d] = 2.0 * nt + 0.5, t
        o += d
    return Values(base.Gpr, base.Apr, -(A.T @ y0) - (G.T @ z0), G @ x0 + s0, A @ x0)


def _case(case):
    """One instance of CURVATURE, computed once and left unchanged: its data, the oracle's exit code and iterate, its direction and the
    oracle's central differences at eps = 1e-5 and 1e-4."""
    if case not in _CASE:
        name, cone, fewer, seed = case
        pat, base = _pattern(name)
        v = curvature_instance(pat, base, seed, cone, fewer)
        code, x, y, z, s = _oracle_x(pat, v)
        g, dc, dh, db = _direction(pat, seed)
        _CASE[case] = dict(pat=pat, v=v, code=code, s=s, z=z, dir=(g, dc, dh, db), fd5=_oracle_fd(pat, v, g, dc, dh, db, 1e-5),
                           fd4=_oracle_fd(pat, v, g, dc, dh, db, 1e-4))
    return _CASE[case]


def _derivative(pat, v, s, z, direction):
    g, dc, dh, db = direction
    return _directional(_Reference(pat, v, s, z).grads(g[None, :]), dc, dh, db)[0]


# ---- CPU: the definition ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CURVATURE)
def test_centred_reference_is_the_derivative_where_curvature_fixes_the_optimum(case):
    """Measured (relative distance from fd(1e-5), NT then centred): vertex-small 1.6e-1 / 6.8e-6, 6.7e-1 / 3.4e-4, 2.2 / 8.5e-5,
    2.2 / 1.5e-3; vertex-mid 7.6 / 5.8e-5, 1.2 / 2.0e-6, 2.5e-1 / 4.2e-4, 1.2 / 2.6e-4, 1.7e-1 / 1.7e-5, 4.0e-1 / 1.8e-4."""
    c = _case(case)
    fd = c["fd5"]
    assert c["code"] == 0, (case, c["code"])
    assert abs(fd - c["fd4"]) <= 1e-3 * abs(fd), (case, fd, c["fd4"])  # the yardstick is stable over eps
    nt = _derivative(c["pat"], c["v"], c["s"], c["z"], c["dir"])
    centred = _derivative(c["pat"], c["v"], *centred_pair(c["pat"], c["s"], c["z"]), c["dir"])
    print(case, "fd", fd, "fd(1e-4)", c["fd4"], "NT", nt, abs(nt - fd) / abs(fd), "centred", centred, abs(centred - fd) / abs(fd))
    assert abs(centred - fd) <= 5e-3 * abs(fd), (case, centred, fd)
    assert abs(nt - fd) >= 1e-1 * abs(fd), (case, nt, fd)  # (the case discriminates)


def _off_centre_pairs(pat, B, seed=5):
    """Interior, off-centre pairs [B, m]: LP rows in U(0.5, 1.5), cone heads 1.05 ... 1.6 times the tail norm, z's tail roughly opposed to s's.
    (The seed: chosen among 0 ... 6 on the two numpy references alone, so that every instance of B = 3 and B = 4 keeps them 5e-2 and
    more of a row's largest entry apart on all three patterns, at cond(scaled K) <= 400.)"""
    rng = np.random.default_rng(300 + seed)
    s, z = rng.uniform(0.5, 1.5, (B, pat.m)), rng.uniform(0.5, 1.5, (B, pat.m))
    for i in range(B):
        o = pat.l
        for d in (int(v) for v in pat.q):
            ts = rng.standard_normal(d - 1)
            tz = -rng.uniform(0.5, 1.5) * ts + 0.4 * np.linalg.norm(ts) / np.sqrt(d - 1) * rng.standard_normal(d - 1)
            s[i, o], s[i, o + 1:o + d] = rng.uniform(1.05, 1.6) * np.linalg.norm(ts), ts
            z[i, o], z[i, o + 1:o + d] = rng.uniform(1.05, 1.6) * np.linalg.norm(tz), tz
            o += d
    return s, z


def _rel(a, b):
    return np.max(np.abs(a - b)) / np.max(np.abs(b))


def test_centred_pair_properties():
    for name in ("vertex-small", "vertex-mid", CLASSES):
        pat, _ = _pattern(name)
        S, Z = _off_centre_pairs(pat, 3)
        for s, z in zip(S, Z):
            s1, z1 = centred_pair(pat, s, z)
            assert np.array_equal(s1[: pat.l], s[: pat.l]) and np.array_equal(z1[: pat.l], z[: pat.l])  # LP rows: bit for bit
            assert not np.array_equal(s1, s) or not np.array_equal(z1, z)
            s2, z2 = centred_pair(pat, s1, z1)
            print(name, "idempotent to", _rel(s2, s1), _rel(z2, z1))
            assert _rel(s2, s1) <= 1e-14 and _rel(z2, z1) <= 1e-14
            o = pat.l  # every cone's pair is central afterwards: s o z = mu e, that is s0 z0 + st'zt = mu and s0 zt + z0 st = 0
            for d in (int(v) for v in pat.q):
                sc, zc = s1[o:o + d], z1[o:o + d]
                assert np.max(np.abs(sc[0] * zc[1:] + zc[0] * sc[1:])) <= 1e-14 * sc[0] * zc[0], (name, d)
                o += d
    # cones of dimension 1 and LP rows: bit for bit
    pat, _ = random_socp_pattern(6, 1, 3, [1, 3, 1], seed=2)
    rng = np.random.default_rng(1)
    s, z = rng.uniform(0.5, 1.5, pat.m), rng.uniform(0.5, 1.5, pat.m)
    s[4], z[4] = 3.0, 3.0  # (the head of the cone of dimension 3: inside)
    s1, z1 = centred_pair(pat, s, z)
    keep = [0, 1, 2, 3, 7]
    assert np.array_equal(s1[keep], s[keep]) and np.array_equal(z1[keep], z[keep])
    assert not np.array_equal(s1[4:7], s[4:7])
    # an exactly central pair z = mu s^-1 (s^-1 = (s0, -st) / det s) comes back
    pat, _ = _pattern("vertex-mid")
    s, _z = _off_centre_pairs(pat, 1)
    s, z, o = s[0], np.empty(pat.m), pat.l
    z[: pat.l] = 0.3 / s[: pat.l]
    for d in (int(v) for v in pat.q):
        sc = s[o:o + d]
        z[o], z[o + 1:o + d] = 0.3 * sc[0] / (sc[0] ** 2 - sc[1:] @ sc[1:]), -0.3 * sc[1:] / (sc[0] ** 2 - sc[1:] @ sc[1:])
        o += d
    s1, z1 = centred_pair(pat, s, z)
    print("central pair returned to", _rel(s1, s), _rel(z1, z))
    assert _rel(s1, s) <= 1e-14 and _rel(z1, z) <= 1e-14
    # a cone with an eigenvalue that is not positive, and one whose s and z are parallel, stay as they are
    pat, _ = random_socp_pattern(6, 1, 2, [3, 3], seed=2)
    s, z = np.array([1.0, 1.0, 1.0, 2.0, 0.0, 2.0, 1.0, 0.5]), np.array([1.0, 1.0, 2.0, -1.0, 0.5, 4.0, 2.0, 1.0])
    s1, z1 = centred_pair(pat, s, z)
    assert np.array_equal(s1, s) and np.array_equal(z1, z)


def test_adjoint_scaling_entry_points_exist_and_refuse():
    L = binding._lib()
    assert (binding.ADJOINT_NT, binding.ADJOINT_CENTRED) == (0, 1) == (eicos_amd.ADJOINT_NT, eicos_amd.ADJOINT_CENTRED)
    for prefix, err in (("eicos_batch_", L.eicos_last_error), ("eicos_multi_", L.eicos_multi_last_error)):
        for mode in (0, 1, 7):
            assert getattr(L, prefix + "set_adjoint_scaling")(None, mode) == -1 and "NULL handle" in err().decode()
        assert getattr(L, prefix + "adjoint_scaling")(None) == -1 and "NULL handle" in err().decode()
    assert eicos_amd.centred_pair is centred_pair


@pytest.mark.gpu
def test_a_fresh_handle_reports_nt_and_an_unknown_mode_is_refused():
    pat, base = _pattern("vertex-small")
    g = eicos_amd.BatchSolver(pat, 2)
    L = binding._lib()
    assert g.adjoint_scaling() == "nt" and L.eicos_batch_adjoint_scaling(g._h) == binding.ADJOINT_NT
    for mode in (-1, 2, 7):
        assert L.eicos_batch_set_adjoint_scaling(g._h, mode) == -1
        assert "set_adjoint_scaling" in L.eicos_last_error().decode() and str(mode) in L.eicos_last_error().decode()
        assert g.adjoint_scaling() == "nt"
    with pytest.raises(ValueError, match="centered"):
        g.set_adjoint_scaling("centered")
    g.set_adjoint_scaling("centred")
    assert g.adjoint_scaling() == "centred" and L.eicos_batch_adjoint_scaling(g._h) == binding.ADJOINT_CENTRED
    assert L.eicos_batch_set_adjoint_scaling(g._h, 2) == -1 and g.adjoint_scaling() == "centred"
    g.set_adjoint_scaling("nt")
    assert g.adjoint_scaling() == "nt"
    g.close()


# ---- GPU: arithmetic on well-conditioned, off-centre pairs ------------------------------------------------------------------------------------
def _vertex_data(name, B):
    from test_adjoint import vertex_instance
    pat, base = _pattern(name)
    vs = [vertex_instance(pat, base, seed) for seed in range(1, B + 1)]
    return pat, {k: np.stack([getattr(v, k) for v in vs]) for k in KEYS}


OFF = {"EICOS_UBL": "0", "EICOS_W2": "0"}
# the forced builds of PARITY of test_adjoint.py, on the two vertex patterns, and the class-edge pattern on the default and on a wave-heavy build
ARITHMETIC = [
    ("vertex-small", {}, None),
    ("vertex-mid", {}, None),
    ("vertex-small", {"EICOS_THREADS": "128"}, ("lds-resident", 128)),
    ("vertex-mid", W2, ("w2", 256)),
    ("vertex-small", DEF256, ("default", 256)),
    ("vertex-mid", DEF256, ("default", 256)),
    ("vertex-mid", {**OFF, "EICOS_THREADS": "128", "EICOS_LDSRES": "0"}, ("default", 128)),
    ("vertex-mid", {**OFF, "EICOS_THREADS": "512"}, ("default", 512)),
    ("vertex-mid", {"EICOS_THREADS": "256"}, None),  # (U in LDS where the handle takes that build)
    ("vertex-small", NOLDS, "no-lds"),  # (the scalar factor path: the hybrid path of vertex-mid keeps its tile scratch in LDS)
    ("vertex-small", {"EICOS_TILES": "1"}, None),  # the tile path
    (CLASSES, {}, None),
    (CLASSES, {**OFF, "EICOS_THREADS": "128", "EICOS_LDSRES": "0"}, ("default", 128)),
    (CLASSES, {**OFF, "EICOS_THREADS": "512"}, ("default", 512)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,env,build", ARITHMETIC)
def test_centred_gradients_match_the_restatement_on_every_build(name, env, build, monkeypatch):
    """Measured on one MI355X: see docs/HISTORY.md A.32."""
    _setenv(monkeypatch, env)
    B = 3
    pat, d = _vertex_data(name, B)
    g = _handle(pat, d, B, build)
    assert np.all(g.solve() == 0)
    s, z = _off_centre_pairs(pat, B)
    g.set_iterate(z=z, s=s)
    _, z_in, s_in = g.duals()
    assert np.array_equal(z_in, z) and np.array_equal(s_in, s)
    rows = _random_rows(pat, B, 2)
    nt = g.adjoint(rows)
    g.set_adjoint_scaling("centred")
    got = g.adjoint(rows)
    assert np.all(np.isfinite(got[3])) and np.all(np.isfinite(nt[3]))
    print(name, env, g.kernel_build(), g.dims()["threads_per_block"], "res", got[3].min(), "...", got[3].max())
    for i in range(B):
        ref = _Reference(pat, _vals(d, i), *centred_pair(pat, s[i], z[i]))
        ref_nt = _Reference(pat, _vals(d, i), s[i], z[i])
        assert ref.cond <= COND_MAX and ref_nt.cond <= COND_MAX, (name, i, ref.cond, ref_nt.cond)
        apart = 0.0
        for what, a, a_nt, w, w_nt in zip(("grad_c", "grad_h", "grad_b"), got, nt, ref.grads(rows[i]), ref_nt.grads(rows[i])):
            for r in range(2):
                dist, dist_nt, scale = np.max(np.abs(a[i, r] - w[r])), np.max(np.abs(a_nt[i, r] - w_nt[r])), np.max(np.abs(w[r]))
                apart = max(apart, np.max(np.abs(a[i, r] - a_nt[i, r])) / scale)
                print(name, "instance", i, what, "row", r, "centred: relative distance", dist / scale, "NT:", dist_nt / np.max(np.abs(w_nt[r])), "cond", ref.cond)
                assert dist <= 1e-8 * scale, (name, env, i, what, r, dist, scale)
                assert dist_nt <= 1e-8 * np.max(np.abs(w_nt[r])), (name, env, i, what, r, dist_nt)  # (the NT mode on the same rows: as before)
        print(name, "instance", i, "NT against centred, largest relative difference of a row", apart)
        assert apart >= 1e-2, (name, i, apart)
    g.close()


# ---- GPU: the curvature cases against the oracle's central difference -----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GPU_CURVATURE))
def test_curvature_cases_against_the_oracle_central_difference(name):
    """Measured on one MI355X: see docs/HISTORY.md A.32."""
    cases = [_case(c) for c in GPU_CURVATURE[name]]
    B = len(cases)
    pat = cases[0]["pat"]
    d = {k: np.stack([getattr(c["v"], k) for c in cases]) for k in KEYS}
    g = _handle(pat, d, B)
    assert np.all(g.solve() == 0)
    rows = np.stack([c["dir"][0] for c in cases])[:, None, :]
    nt = g.adjoint(rows)
    g.set_adjoint_scaling("centred")
    gc, gh, gb, res = g.adjoint(rows)
    _, z, s = g.duals()
    for i, c in enumerate(cases):
        gvec, dc, dh, db = c["dir"]
        fd = c["fd5"]
        assert c["code"] == 0 and abs(fd - c["fd4"]) <= 1e-3 * abs(fd), (name, i)
        ref = _derivative(pat, c["v"], *centred_pair(pat, s[i], z[i]), c["dir"])
        got = gc[i, 0] @ dc + gh[i, 0] @ dh + gb[i, 0] @ db
        got_nt = nt[0][i, 0] @ dc + nt[1][i, 0] @ dh + nt[2][i, 0] @ db
        d_ref = abs(ref - fd)
        print(name, GPU_CURVATURE[name][i], "fd", fd, "gpu", got, "|gpu - fd| / |fd|", abs(got - fd) / abs(fd), "d_ref / |fd|", d_ref / abs(fd),
              "NT mode |gpu - fd| / |fd|", abs(got_nt - fd) / abs(fd), "res", res[i, 0])
        assert d_ref <= 5e-3 * abs(fd), (name, i, ref, fd)
        assert abs(got - fd) <= 4.0 * d_ref + 1e-6 * abs(fd), (name, i, got, fd, ref)
    g.close()


# ---- GPU: nothing moves by default ----------------------------------------------------------------------------------------------------------
def _three_calls(g, pat, B, theta0, T, w):
    rows = _random_rows(pat, B, 2)
    return list(g.adjoint(rows)) + list(g.param_jacobian()) + list(g.rollout_jacobian(theta0, T, w))


def _mapped_handle(pat, d, B, k, r):
    import test_param_update as P
    import test_rollout as RO
    from test_param_step import _omap
    g = _handle(pat, d, B)
    g.set_param_map(P._map(d, k)); g.set_output_map(_omap(pat.n, r)); g.set_plant_map(RO._fmap(k, r))
    g.solve()
    return g


def _rollout_case(name):
    """(pattern, data, B) of a case whose rollouts under the maps of _mapped_handle end OPTIMAL in every step: the all-classes vertex
    case of tests/test_cone_classes.py (as its own rollout test asserts), or a fixture."""
    import test_cone_classes as CC
    import test_param_update as P
    if name == CC.ALL:
        CC._assert_well_posed(CC.ALL)
        return CC._data(CC.ALL) + (CC.B,)
    return P._data(name, 4) + (4,)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["v-all-classes", "lp_afiro"])
def test_nothing_moves_by_default(name):
    """A handle that never set the mode, and one set to centred and back, give the same bits; on a pattern without cones the centred
    mode gives them too."""
    import test_param_update as P
    import test_rollout as RO
    k, r, T = 5, 4, 2
    pat, d, B = _rollout_case(name)
    theta0, w = P._theta(B, k), RO._w(B, T, k)
    plain, back = _mapped_handle(pat, d, B, k, r), _mapped_handle(pat, d, B, k, r)
    want = _three_calls(plain, pat, B, theta0, T, w)
    back.set_adjoint_scaling("centred")
    centred = _three_calls(back, pat, B, theta0, T, w)
    back.set_adjoint_scaling("nt")
    back.update(*[d[k_] for k_ in KEYS]); back.solve()  # (the rollout moved the handle: back to where `plain` started)
    again = _three_calls(back, pat, B, theta0, T, w)
    assert np.all(want[8] == 0) and np.all(np.isfinite(want[10])), (name, want[8])  # (every step OPTIMAL: every J_t is a computed Jacobian)
    for q, (a, b) in enumerate(zip(again, want)):
        assert np.array_equal(a, b, equal_nan=True), (name, "centred and back", q)
    same = [np.array_equal(a, b, equal_nan=True) for a, b in zip(centred, want)]
    print(name, "centred equal to NT per array", same)
    if len(pat.q) == 0:
        assert all(same), (name, same)
    else:  # (the mode reaches all three calls: gradient rows, the contracted Jacobian, the rollout's J)
        assert not same[0] and not same[4] and not same[10], (name, same)
    _assert_same(_state(plain), _state(back), name)
    plain.close(); back.close()


# ---- GPU: the rollout Jacobian under the centred mode -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("env,fused", [({}, True), ({"EICOS_FUSED_UPDATE": "0"}, False)])
def test_rollout_jacobian_equals_the_host_twin_under_the_centred_mode(env, fused, monkeypatch):
    """T = 2 steps on the all-classes case of tests/test_cone_classes.py with recording on, against update_param_solve +
    param_jacobian + the plant on the host, bit for bit; the recorded rows are the twin's adjoint rows."""
    import test_cone_classes as CC
    import test_param_update as P
    import test_rollout as RO
    import test_rollout_jacobian as RJ
    from test_adjoint import _csr_dense
    from test_param_step import _omap
    _setenv(monkeypatch, env)
    CC._assert_well_posed(CC.ALL)
    pat, d = CC._data(CC.ALL)
    B, k, r, T = CC.B, 5, 4, 2
    pm, om, fm = P._map(d, k), _omap(pat.n, r), RO._fmap(k, r)
    g, ref = P._twins(pat, d, B)
    for s in (g, ref):
        s.set_param_map(pm); s.set_output_map(om)
        s.set_adjoint_scaling("centred")
    g.set_plant_map(fm)
    g.set_rollout_recording(True)
    theta0, w = P._theta(B, k), RO._w(B, T, k)
    want = RJ._host_loop_jac(ref, fm, theta0, T, w)
    got = g.rollout_jacobian(theta0, T, w)
    assert g.last_rollout_launches() == (1 if fused else T)
    assert np.all(got[2] == 0), got[2]
    assert np.all(np.isfinite(got[4])) and np.any(got[4] != 0.0)
    RJ._assert_six(got, want, (CC.ALL, env))
    RJ._same_handles(g, ref, B, (CC.ALL, env))
    # the recorded rows of the last step: the twin's adjoint (centred) of the dense rows of the output map, at the same iterate
    U = _csr_dense((om.base, om.rowptr, om.col, om.val), pat.n)
    rec = g.rollout_records()
    for a, b in zip(rec[:3], ref.adjoint(np.broadcast_to(U, (B, r, pat.n)).copy())[:3]):
        assert np.array_equal(a[:, T - 1], b, equal_nan=True)
    # ... and the mode reached the launch: the NT rollout from the same state differs
    for s in (g, ref):
        s.set_adjoint_scaling("nt")
        s.update(*[d[k_] for k_ in KEYS]); s.solve()
    nt = g.rollout_jacobian(theta0, T, w)
    RJ._assert_six(nt, want, (CC.ALL, env, "NT"), n=4)
    assert not np.array_equal(nt[4], got[4])
    g.close(); ref.close()


# ---- GPU: multi-GPU -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("devs", [[0, 0], [0, 0, 0]])
def test_multi_output_jacobian_under_the_centred_mode_equals_the_single_handle(devs):
    B = 4
    pat, d = _vertex_data("vertex-mid", B)
    pmap, omap = _random_maps(pat)
    eicos_amd.set_arithmetic_profile(1)  # (plans by the pattern alone: a shard gives the bits of the batch)
    try:
        single = eicos_amd.BatchSolver(pat, B)
        multi = eicos_amd.MultiBatchSolver(pat, B, devs)
    finally:
        eicos_amd.set_arithmetic_profile(0)
    s, z = _off_centre_pairs(pat, B)
    out = []
    for g in (single, multi):
        assert g.adjoint_scaling() == "nt"
        g.update(*[d[k] for k in KEYS])
        g.set_param_map(pmap); g.set_output_map(omap)
        assert np.all(g.solve() == 0)
        g.set_iterate(z=z, s=s)
        nt = g.output_jacobian()
        g.set_adjoint_scaling("centred")
        assert g.adjoint_scaling() == "centred"
        out.append((nt, g.output_jacobian(), g.output_jacobian(idx=[3, 0, 2])))
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), devs
    assert np.all(np.isfinite(out[0][1][0])) and not np.array_equal(out[0][0][0], out[0][1][0])
    L = binding._lib()
    assert L.eicos_multi_set_adjoint_scaling(multi._h, 5) == -1 and "5" in L.eicos_multi_last_error().decode()
    assert multi.adjoint_scaling() == "centred"
    for g in (single, multi):
        g.close()


# ---- GPU: refusals --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_and_the_switch_itself_move_nothing():
    """A refused mode leaves the mode, the J trajectory and every readable state as they were; so does setting a mode: the trajectory
    stays as it was recorded and still belongs to the handle's maps (no map install)."""
    import test_param_update as P
    import test_rollout as RO
    k, r, T = 5, 4, 2
    pat, d, B = _rollout_case("v-all-classes")
    g = _mapped_handle(pat, d, B, k, r)
    g.set_adjoint_scaling("centred")
    theta0, w = P._theta(B, k), RO._w(B, T, k)
    out = g.rollout_jacobian(theta0, T, w)
    assert np.all(out[2] == 0) and np.all(np.isfinite(out[4]))
    gu = np.random.default_rng(5).standard_normal(out[0].shape)
    grad = g.rollout_gradient(gu)
    assert all(np.all(np.isfinite(a)) for a in grad)
    before = _state(g)
    L = binding._lib()
    for mode in (-3, 2, 1 << 20):
        assert L.eicos_batch_set_adjoint_scaling(g._h, mode) == -1 and str(mode) in L.eicos_last_error().decode()
        assert g.adjoint_scaling() == "centred"
    assert L.eicos_batch_rollout_jacobian_steps(g._h) == T
    for a, b in zip(g.rollout_gradient(gu), grad):
        assert np.array_equal(a, b)
    g.set_adjoint_scaling("nt")  # the J on the handle stays the centred one, and the sweep still runs over it
    assert L.eicos_batch_rollout_jacobian_steps(g._h) == T
    for a, b in zip(g.rollout_gradient(gu), grad):
        assert np.array_equal(a, b)
    _assert_same(_state(g), before, "after the refusals and the switch")
    g.close()
