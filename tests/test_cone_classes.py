"""Every cone class of the solve kernel at its dimension and count edges (DESIGN.md 4.2 "Per-cone loops", 6).

The per-cone loops have four forms, chosen per cone by dimension -- tiny (1 ... 4 rows, for_tiny), mid (5 ... 31, the generic body one thread
per cone), wave (32 ... 64, for_wave) and huge (more than 64, the generic body one wavefront per cone) -- and a pass over the cones of a
class handles a fixed number of cones per trip, the last partial trip by clamped loads and a guarded body.  The inputs here put every
class boundary (4|5, 31|32, 64|65), the second and third trip of a huge cone's lanes (65, 129, 130 rows), trip + 1 cones of each class
in front of every workgroup size, and wave cones of different dimension in one trip, in front of the solve, the scaling stage, the
adjoint, the Jacobians and the rollout Jacobian.

Two input families, both asserted on the CPU oracle before a GPU result is looked at (test_inputs_are_well_posed_on_the_oracle):
  V  vertex_instance of test_adjoint.py on random_socp_pattern(n, p, l, q, density=0.3, seed=5), l >= n - p: a unique, strictly
     complementary optimum with every cone strictly inside; cond(scaled K) <= 1e4 at the oracle's iterate, so x is held to the 1e-8 of
     well-posed batches and the adjoint to the dense reference;
  F  feasible_batch(pat, base, 0, 3, seed=211) on random_socp_pattern(..., seed=11): cones active at the optimum, cond 1e10 ... 1e13,
     x held to the 1e-6 of test_random_socp_with_equalities.

Measured on one MI355X (maxima over the three instances of every case; iteration counts equal to the oracle's on every instance):
  solve, family V: x 9e-16 ... 6.8e-14 of the 1e-8 bound's scale (worst: the all-classes case under EICOS_TILES=1), pcost 3e-16 ... 5e-15,
  residuals 5e-12 ... 6.8e-10; family F: x 1.1e-12 ... 2.0e-10 (worst: 33 wave cones at 512 threads), pcost 1e-15 ... 1.1e-13, residuals
  5e-11 ... 6.2e-9; the forced builds give the same figures to the digit or two shown.
  scaling block: 1.3e-13 max(1, |V_oracle|) at 128 and at 512 threads, three late failures found at each of the four cones.
  adjoint against the dense reference: 7e-13 ... 2.8e-10 of a row's largest entry (bound 1e-8; grad_c, the small vector, is the worst),
  res 6e-17 ... 1.6e-14; output Jacobian 4e-15 ... 8.5e-13 at max |J| 7 ... 42; grad_G / grad_A 4e-15 ... 3.4e-11 against bounds of 2e-8 ...
  1.8e-5.  Before the adjoint's stop rule kept a step whose error norm lands just above the threshold it had reached (kernels.hip,
  kkt_solve, ADJ), instance 2 of the all-classes case sat 4.7e-6 off in grad_c, row 0: the test that found it.
"""
import numpy as np
import pytest

import eicos_amd
from eicos_amd.generate import feasible_batch, random_socp_pattern
from eicos_amd.problem_io import Values
from oracle.oracle import OracleSolver
from test_oracle_golden import in_cone, kkt_residuals
from test_adjoint import COND_MAX, _Reference, _handle, _setenv, nt_w2, vertex_instance  # noqa: F401 (nt_w2: the scaling _Reference builds on)

KEYS = ("Gpr", "Apr", "c", "h", "b")
PCOST_RTOL = 1e-8
B = 3
ALL = "v-all-classes"

# (n, p, l, q): family V
V_CASES = {
    "v-wave-edges": (16, 3, 20, [32, 64, 3]),
    "v-huge-edges": (16, 3, 20, [65, 129]),
    ALL: (24, 4, 30, [1, 4, 5, 31, 32, 64, 65, 130]),
    "v-wave-9": (20, 4, 24, [32] * 9),
    "v-wave-17": (20, 4, 24, [33] * 17 + [2]),
    "v-huge-5": (20, 4, 24, [66] * 5),
    "v-wave-33": (20, 4, 24, [32] * 33),
    "v-tiny-1025": (20, 4, 24, [1, 2, 3, 4] * 256 + [3]),
    "v-huge-9": (20, 4, 24, [65] * 9),
    "v-wave-mixed-5": (20, 4, 24, [32, 64, 33, 63, 48]),  # different dimensions in one trip, a count that is no multiple of any trip
    "v-wave-8": (20, 4, 24, [32] * 8),                    # a count that IS a whole trip (256 threads) and two whole trips (128)
}
FIRST_SIX = list(V_CASES)[:6]
# (n, p, l, q, density): family F
F_CASES = {
    "f-mid-wave": (40, 6, 5, [31, 32, 5], 0.3),
    "f-wave-huge": (70, 8, 6, [64, 65, 3], 0.3),
    "f-huge-trips": (120, 10, 4, [65, 128, 129, 2], 0.3),
    "f-all-classes": (100, 5, 0, [1, 4, 5, 31, 32, 64, 65, 90], 0.3),
    "f-wave-17": (150, 6, 3, [33] * 17 + [3, 7], 0.3),
    "f-huge-5": (120, 6, 3, [66] * 5, 0.3),
    "f-wave-33": (40, 4, 3, [32] * 33, 0.1),
    "f-huge-9": (60, 4, 3, [65] * 9, 0.2),
    "f-mid-513": (150, 10, 5, [5] * 513, 0.05),
    "f-tiny-257": (120, 10, 5, [3] * 257, 0.3),
}
FIRST_FOUR_F = list(F_CASES)[:4]

_DATA, _ORACLE = {}, {}


def _data(name):
    """(pattern, dict of [B, ...] arrays) of a case of the tables."""
    if name not in _DATA:
        if name in V_CASES:
            n, p, l, q = V_CASES[name]
            assert l >= n - p
            pat, base = random_socp_pattern(n, p, l, q, density=0.3, seed=5)
            vs = [vertex_instance(pat, base, seed) for seed in range(1, B + 1)]
            d = {k: np.stack([getattr(v, k) for v in vs]) for k in KEYS}
        else:
            n, p, l, q, dens = F_CASES[name]
            pat, base = random_socp_pattern(n, p, l, q, density=dens, seed=11)
            d = feasible_batch(pat, base, 0, B, seed=211)
        _DATA[name] = (pat, d)
    return _DATA[name]


def _vals(d, i):
    return Values(*[d[k][i] for k in KEYS])


def _oracle(name):
    """The CPU oracle on the B instances of a case, computed once: a list of dicts (code, iter, pcost, x, y, z, s; cond for family V)."""
    if name not in _ORACLE:
        pat, d = _data(name)
        out = []
        for i in range(B):
            v = _vals(d, i)
            o = OracleSolver(pat, v)
            code = o.solve()
            info = o.info()
            y, z, s = [a.copy() for a in o.yzs()]
            r = dict(code=code, iter=info["iter"], pcost=info["pcost"], x=o.x().copy(), y=y, z=z, s=s)
            o.close()
            if name in V_CASES and code == 0:
                r["cond"] = _Reference(pat, v, s, z).cond
            out.append(r)
        _ORACLE[name] = out
    return _ORACLE[name]


def _assert_well_posed(name):
    """The issue's condition on an input, asserted on the oracle alone: every instance OPTIMAL, and cond <= COND_MAX in family V."""
    for i, r in enumerate(_oracle(name)):
        assert r["code"] == 0, (name, i, r["code"])
        if name in V_CASES:
            assert r["cond"] <= COND_MAX, (name, i, r["cond"])


# ---- CPU: the inputs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(V_CASES) + list(F_CASES))
def test_inputs_are_well_posed_on_the_oracle(name):
    _assert_well_posed(name)
    rs = _oracle(name)
    print(name, "iterations", [r["iter"] for r in rs], "cond", ["%.1e" % r["cond"] for r in rs] if name in V_CASES else "-")


def test_the_tables_cover_every_class_boundary_and_trip_edge():
    """The coverage claim itself, from the dimensions alone: both sides of 4|5, 31|32 and 64|65, a huge cone with a second and a third trip per
    lane, and for every trip width of a build (wave cones: 4, 8, 16, 32; tiny cones: 256, 512, 1024 and, in the commit phase, 128; huge
    cones: the 2, 4, 8 wavefronts of a workgroup; mid cones: 512 threads) a case with one cone more than whole trips."""
    dims = set()
    for t in list(V_CASES.values()) + list(F_CASES.values()):
        dims |= set(t[3])
    assert {1, 2, 3, 4, 5, 31, 32, 64, 65, 129, 130} <= dims
    wave = {k: sum(32 <= d <= 64 for d in t[3]) for k, t in {**V_CASES, **F_CASES}.items()}
    tiny = {k: sum(d <= 4 for d in t[3]) for k, t in {**V_CASES, **F_CASES}.items()}
    huge = {k: sum(d > 64 for d in t[3]) for k, t in {**V_CASES, **F_CASES}.items()}
    for _, threads, trip, names in COUNT_EDGES:
        for nm in names:
            if "wave" in nm and "mixed" not in nm and nm != "v-wave-8":
                assert wave[nm] % trip == 1, (nm, trip)
            if "tiny" in nm:
                assert tiny[nm] % (2 * threads) == 1 and tiny[nm] % threads == 1, (nm, threads)
            if "huge" in nm:
                assert huge[nm] % (threads // 64) == 1, (nm, threads)
            if "mid" in nm:
                assert sum(5 <= d < 32 for d in F_CASES[nm][3]) % threads == 1, (nm, threads)
    assert wave["v-wave-8"] == 8 and wave["v-wave-mixed-5"] == 5 and len(set(V_CASES["v-wave-mixed-5"][3])) == 5


# ---- GPU: 1. solve parity per class ---------------------------------------------------------------------------------------------------------
def _solve_against_the_oracle(name, build=None):
    """Batch B of a case against the oracle, instance by instance; returns the measured maxima (x, pcost, residual, iteration difference)."""
    _assert_well_posed(name)
    pat, d = _data(name)
    g = _handle(pat, d, B, build)
    codes = g.solve()
    ia = g.info_arrays()
    x = g.solution(); y, z, s = g.duals()
    x_rtol = 1e-8 if name in V_CASES else 1e-6
    mx = dict(x=0.0, pcost=0.0, res=0.0, dit=0)
    for i, r in enumerate(_oracle(name)):
        v = _vals(d, i)
        xerr = np.abs(x[i] - r["x"]).max() / max(1.0, np.abs(r["x"]).max())
        perr = abs(ia["pcost"][i] - r["pcost"]) / max(1.0, abs(r["pcost"]))
        rp, re, rd, gap = kkt_residuals(pat, v, x[i], y[i], z[i], s[i])
        dit = int(ia["iter"][i]) - int(r["iter"])
        print(name, g.kernel_build(), g.dims()["threads_per_block"], "instance", i, "code", codes[i], "iter", int(ia["iter"][i]), "oracle", r["iter"],
              "xerr", xerr, "pcost", perr, "residuals", max(rp, re, rd))
        assert codes[i] == r["code"] == 0, (name, i, codes[i])
        assert abs(dit) <= 1, (name, i, ia["iter"][i], r["iter"])
        assert perr <= PCOST_RTOL, (name, i, ia["pcost"][i], r["pcost"])
        assert max(rp, re, rd) < 1e-7, (name, i, rp, re, rd)
        assert in_cone(pat, s[i], 1e-7) and in_cone(pat, z[i], 1e-7), (name, i)
        if dit == 0:
            assert xerr <= x_rtol, (name, i, xerr)
            mx["x"] = max(mx["x"], xerr)
        mx["pcost"], mx["res"], mx["dit"] = max(mx["pcost"], perr), max(mx["res"], rp, re, rd), max(mx["dit"], abs(dit))
    g.close()
    print(name, "maxima", mx)
    return mx


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(V_CASES) + FIRST_FOUR_F)
def test_solve_matches_the_oracle_per_class(name):
    _solve_against_the_oracle(name)


@pytest.mark.gpu
@pytest.mark.parametrize("tiles", ["0", "1", "2"])
def test_all_classes_under_every_tile_layout(tiles, monkeypatch):
    monkeypatch.setenv("EICOS_TILES", tiles)  # (the expansion rows of a cone sit differently in the tile layouts)
    _solve_against_the_oracle(ALL)


# ---- GPU: 2. count edges per build ----------------------------------------------------------------------------------------------------------
OFF = {"EICOS_UBL": "0", "EICOS_W2": "0"}
# (environment, (build, threads), wave cones per trip, cases): trip = U * threads / 64 wave cones; 2 * threads tiny cones (threads or
# 2 * threads in the commit phase); threads / 64 huge cones and `threads` mid cones per round
COUNT_EDGES = [
    ({**OFF, "EICOS_THREADS": "128", "EICOS_LDSRES": "0"}, 128, 4,
     ["v-wave-9", "v-wave-mixed-5", "f-wave-17", "v-wave-8", "v-tiny-1025", "f-tiny-257", "v-huge-5", "f-huge-5", "f-mid-513"]),
    ({**OFF, "EICOS_THREADS": "256"}, 256, 8, ["v-wave-9", "v-wave-mixed-5", "f-wave-17", "v-wave-8", "v-tiny-1025", "v-huge-5", "f-huge-5", "f-mid-513"]),
    ({**OFF, "EICOS_THREADS": "512"}, 512, 32, ["v-wave-33", "f-wave-33", "v-wave-mixed-5", "v-tiny-1025", "v-huge-9", "f-huge-9", "f-mid-513"]),
    ({"EICOS_UBL": "0", "EICOS_THREADS": "256"}, 256, 16, ["v-wave-17", "f-wave-17", "v-wave-mixed-5", "v-tiny-1025", "v-huge-5"]),
]
BUILD_OF = ["default", "default", "default", "w2"]
EDGE_PARAMS = [(j, nm) for j, row in enumerate(COUNT_EDGES) for nm in row[3]]


@pytest.mark.gpu
@pytest.mark.parametrize("row,name", EDGE_PARAMS)
def test_count_edges_on_every_build(row, name, monkeypatch):
    """No bit-identity across workgroup sizes is claimed by the project (the block reductions differ): every build against the oracle alone."""
    env, threads, _, _ = COUNT_EDGES[row]
    _setenv(monkeypatch, env)
    _solve_against_the_oracle(name, (BUILD_OF[row], threads))


# ---- GPU: 3. the scaling stage per class, failure semantics across several cones ---------------------------------------------------------------
SC_Q = [1, 2, 4, 5, 31, 32, 64, 65, 130]
SC_CLASS = ["tiny", "tiny", "tiny", "mid", "mid", "wave", "wave", "huge", "huge"]


def _blocks(pat):
    """Slices of the scaling block: the LP part, then one per cone (3 d + 1 entries)."""
    out, o = [slice(0, pat.l)], pat.l
    for d in (int(v) for v in pat.q):
        out.append(slice(o, o + 3 * d + 1)); o += 3 * d + 1
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("threads", ["128", "512"])
def test_scaling_stage_per_class_and_failure_semantics(threads, monkeypatch):
    """updateScalings + updateKKTScalings of both sides on the same (s, z), on a pattern with one cone of every class and both sides of
    every boundary.  The reference walks the cones in order and returns at the first failure: cones before it are new, the failing cone
    and those after it keep the old state (a LATE failure: the new eta^2 and q with the old d1, u0, u1, v1), the LP block is new.  The GPU
    does this in two parallel phases; the oracle's block fixes where its commit has to stop.

    The bound is the 1e-9 max(1, |V_oracle|) of test_update_scalings_failure_modes_match_oracle throughout.  What makes it meaningful
    close to the boundary is the input, not the bound.  sres = s0^2 - sum t_k^2 cancels: at s0 = |t| (1 + eps) an error of j ulps in the
    sum is a relative error of j 1.1e-16 / (2 eps) in sres, and a wavefront reduction and the oracle's sequential loop differ by a few
    ulps whenever the terms are not exact -- 1e-7 at eps = 1e-9, which says nothing about either side.  So the pairs at eps <= 1e-6 draw
    t_k from +-{1 ... 8} / 8: every square and every partial sum is exact in fp64, in any order, every row is non-zero, and the two
    sides see the same sres to the bit.  The pairs at eps >= 1e-3 draw t from a normal distribution.

    A late failure needs a >= 1e7 in c2byu02 - d ~ 1 / a^2 against 2 (measured in numpy: no failure at a <= 1e6, 12 % of a ~ 1e7 ...
    1e8), a = (s0 / snorm + z0 / znorm) / (2 gam): both points within a few ulps of the boundary AND gam ~ 1, which is z's tail
    pointing against s's.  Independent random tails, as the existing test draws them, do not get there in any dimension above 2 (0 of 4000
    draws at dimensions 5 ... 130 on the oracle; what the existing test counts are early failures by rounding of the sum).  So the
    failing cone is drawn here as s = (|a| + k1 ulp, a e_j), z = (|b| + k2 ulp, -b e_j) with random a, b, row j and k1, k2 in 1 ... 3:
    every sum over the rows then has at most two non-zero terms and is the same in any order, which is what makes a cone that is summed
    across lanes comparable with the oracle at all at that distance.  7 % of such draws fail late on the oracle."""
    _setenv(monkeypatch, {**OFF, "EICOS_THREADS": threads})
    pat, base = random_socp_pattern(24, 4, 6, SC_Q, seed=5)
    d = feasible_batch(pat, base, 0, 1, seed=3)
    o = OracleSolver(pat, _vals(d, 0))
    g = _handle(pat, d, 1)
    assert g.dims()["threads_per_block"] == int(threads)
    rng = np.random.default_rng(0)
    blk = _blocks(pat)
    nc = len(SC_Q)
    worst = [0.0]

    def point(eps_of, exact=False):
        out = [rng.uniform(0.5, 2, pat.l)]
        for c, dd in enumerate(SC_Q):
            t = rng.integers(1, 9, dd - 1) * rng.choice([-1.0, 1.0], dd - 1) / 8.0 if exact else rng.standard_normal(dd - 1)
            nt = np.linalg.norm(t) if dd > 1 else rng.uniform(0.5, 2)
            out.append(np.concatenate([[nt * (1 + eps_of(c))], t]))
        return np.concatenate(out)

    def both(s, z, what):
        ok, Vo = o.debug_scalings(s, z)
        ran, Vg = g.debug_scalings(s, z)
        assert ran
        rel = np.abs(Vg - Vo) / np.maximum(1.0, np.abs(Vo))
        worst[0] = max(worst[0], rel.max())
        bad = np.flatnonzero(rel > 1e-9)
        assert bad.size == 0, (what, ok, rel.max(), bad[:8], [j for j, b in enumerate(blk) if b.start <= bad[0] < b.stop])
        return ok, Vo

    def fresh():
        ok, V0 = both(point(lambda c: 0.5), point(lambda c: 0.7), "fresh interior pair")
        assert ok
        return V0

    fresh()
    for eps in (1e-3, 1e-6, 1e-9):  # interior pairs ever closer to the boundary
        ok, _ = both(point(lambda c: eps, eps <= 1e-6), point(lambda c: eps, eps <= 1e-6), ("interior", eps))
        assert ok, eps
        print("threads", threads, "interior eps", eps, "max relative distance so far", worst[0])

    def check_groups(V, V0, first, late):
        """On the ORACLE's output: LP new, cones before `first` new, cones after it old, `first` itself old (early) or mixed (late)."""
        assert not np.any(V[blk[0]] == V0[blk[0]])
        for c in range(nc):
            same = np.array_equal(V[blk[1 + c]], V0[blk[1 + c]])
            if c < first:
                assert not same, (first, c)
            elif c > first or not late:
                assert same, (first, c)
            else:  # (the new eta^2 multiplies every entry of the block, the kept d1, u0, u1, v1 included: the block DID change)
                assert not same, (first, c)

    # early failure, one cone at a time
    for bad in range(1, nc):
        V0 = fresh()
        ok, V = both(point(lambda c: -0.1 if c == bad else 0.3), point(lambda c: 0.4), ("early failure at cone", bad, SC_Q[bad]))
        assert not ok
        check_groups(V, V0, bad, False)
    # two cones of different classes outside at once: the commit stops at the first in cone order
    for a, b_ in ((3, 6), (5, 8), (2, 7), (1, 5)):
        assert SC_CLASS[a] != SC_CLASS[b_]
        V0 = fresh()
        for which in ("s", "sz"):  # both in s; the first in z and the second in s
            s = point(lambda c: -0.1 if (c == b_ or (c == a and which == "s")) else 0.3)
            z = point(lambda c: -0.1 if (c == a and which == "sz") else 0.4)
            ok, V = both(s, z, ("two cones outside", a, b_, which))
            assert not ok
            check_groups(V, V0, a, False)
    # late failure (c2byu02 - d <= 0 with both points strictly inside) on a cone of every class: a bounded number of draws, at least
    # one found per cone
    def up(x, k):
        for _ in range(k):
            x = np.nextafter(x, np.inf)
        return x

    for cone in (1, 3, 6, 8):
        off, dd = pat.l + sum(SC_Q[:cone]), SC_Q[cone]
        late = 0
        for _ in range(150):
            V0 = fresh()
            s, z = point(lambda c: 0.5), point(lambda c: 0.7)
            a, b_, j = abs(rng.standard_normal()) + 0.1, abs(rng.standard_normal()) + 0.1, int(rng.integers(1, dd))
            s[off:off + dd], z[off:off + dd] = 0.0, 0.0
            s[off], s[off + j] = up(a, int(rng.integers(1, 4))), a
            z[off], z[off + j] = up(b_, int(rng.integers(1, 4))), -b_
            assert s[off] ** 2 - s[off + j] ** 2 > 0 and z[off] ** 2 - z[off + j] ** 2 > 0  # strictly inside
            ok, V = both(s, z, ("late-failure draw", cone))
            if ok:
                continue
            late += 1
            check_groups(V, V0, cone, True)
            if late >= 3:
                break
        print("threads", threads, "cone", cone, "dimension", dd, "late failures found", late)
        assert late >= 1, cone
    print("threads", threads, "max relative distance of the scaling block", worst[0])
    g.close(); o.close()


# ---- GPU: 4. adjoint and Jacobians over wave and huge cones ------------------------------------------------------------------------------------
def _gpu_refs(name, pat, d, g):
    y, z, s = g.duals()
    refs = []
    for i in range(B):
        ref = _Reference(pat, _vals(d, i), s[i], z[i])
        assert ref.cond <= COND_MAX, (name, i, ref.cond)
        refs.append(ref)
    return refs


@pytest.mark.gpu
@pytest.mark.parametrize("name,env,build", [(nm, {}, None) for nm in FIRST_SIX] + [("v-wave-33", {**OFF, "EICOS_THREADS": "512"}, ("default", 512))])
def test_adjoint_matches_the_dense_reference_over_wave_and_huge_cones(name, env, build, monkeypatch):
    from test_adjoint import _random_rows
    _setenv(monkeypatch, env)
    _assert_well_posed(name)
    pat, d = _data(name)
    g = _handle(pat, d, B, build)
    assert np.all(g.solve() == 0)
    rows = _random_rows(pat, B, 2)
    gc, gh, gb, res = g.adjoint(rows)
    assert np.all(np.isfinite(res)), res
    worst = 0.0
    for i, ref in enumerate(_gpu_refs(name, pat, d, g)):
        for what, got, w in zip(("grad_c", "grad_h", "grad_b"), (gc[i], gh[i], gb[i]), ref.grads(rows[i])):
            for r in range(2):
                dist, scale = np.max(np.abs(got[r] - w[r])), np.max(np.abs(w[r]))
                worst = max(worst, dist / scale)
                assert dist <= 1e-8 * scale, (name, i, what, r, dist, scale, ref.cond)
    print(name, g.kernel_build(), g.dims()["threads_per_block"], "worst relative distance", worst, "res", res.min(), "...", res.max())
    g.close()


@pytest.mark.gpu
def test_output_jacobian_and_matrix_gradients_on_the_all_classes_case():
    from test_adjoint import _csr_dense, _random_maps, _random_rows
    from test_adjoint_matrix import _formula
    _assert_well_posed(ALL)
    pat, d = _data(ALL)
    g = _handle(pat, d, B)
    k, r = 3, 2
    pmap, omap = _random_maps(pat, k, r)
    g.set_param_map(pmap); g.set_output_map(omap)
    assert np.all(g.solve() == 0)
    refs = _gpu_refs(ALL, pat, d, g)
    U = _csr_dense((omap.base, omap.rowptr, omap.col, omap.val), pat.n)
    Cm, Hm, Bm = _csr_dense(pmap.c, k), _csr_dense(pmap.h, k), _csr_dense(pmap.b, k)
    J, res = g.output_jacobian()
    Jd, resd = g.output_jacobian(device=True)
    assert J.shape == (B, r, k) and np.all(np.isfinite(res))
    assert np.array_equal(J, Jd) and np.array_equal(res, resd)
    for i, ref in enumerate(refs):
        want = U @ ref.solve(np.concatenate([-Cm, Bm, Hm]))[: pat.n]
        dist = np.max(np.abs(J[i] - want))
        print(ALL, "instance", i, "max |J - ref|", dist, "max |J|", np.max(np.abs(want)))
        assert dist <= 1e-8 * np.max(np.abs(want)), (i, dist)
    rows = _random_rows(pat, B, 2)
    gc, gh, gb, gG, gA, res = g.adjoint_data(rows)
    x, (y, z, s) = g.solution(), g.duals()
    amax = lambda a: np.max(np.abs(a), initial=0.0)
    for i, ref in enumerate(refs):
        wc, wh, wb = ref.grads(rows[i])
        wG, wA = _formula(pat, (wc, wh, wb), x[i], y[i], z[i])
        for q in range(2):  # (the bound of test_matrix_gradients_match_the_dense_reference: 1e-8 of the magnitudes of the two products)
            bG = 1e-8 * (amax(wc[q]) * amax(z[i]) + amax(wh[q]) * amax(x[i]))
            bA = 1e-8 * (amax(wc[q]) * amax(y[i]) + amax(wb[q]) * amax(x[i]))
            dG, dA = amax(gG[i, q] - wG[q]), amax(gA[i, q] - wA[q])
            print(ALL, "instance", i, "row", q, "grad_G distance", dG, "bound", bG, "grad_A distance", dA, "bound", bA)
            assert dG <= bG and dA <= bA, (i, q, dG, bG, dA, bA)
    g.close()


@pytest.mark.gpu
def test_rollout_jacobian_equals_the_host_twin_on_the_all_classes_case():
    """One rollout_jacobian of T = 2 steps against update_param_solve + param_jacobian + the plant on the host, bit for bit, as
    tests/test_rollout_jacobian.py defines it: k_roll_sens over wave and huge cones."""
    import test_param_update as P
    import test_rollout as RO
    import test_rollout_jacobian as RJ
    from test_param_step import _omap
    _assert_well_posed(ALL)
    pat, d = _data(ALL)
    k, r, T = 5, 4, 2
    pm, om, fm = P._map(d, k), _omap(pat.n, r), RO._fmap(k, r)
    g, ref = P._twins(pat, d, B)
    for s in (g, ref):
        s.set_param_map(pm); s.set_output_map(om)
    g.set_plant_map(fm)
    theta0, w = P._theta(B, k), RO._w(B, T, k)
    want = RJ._host_loop_jac(ref, fm, theta0, T, w)
    got = g.rollout_jacobian(theta0, T, w)
    assert np.all(got[2] == 0), got[2]              # every step of every instance ended OPTIMAL: every J_t is a computed Jacobian
    assert np.all(np.isfinite(got[4])) and np.any(got[4] != 0.0)
    RJ._assert_six(got, want, ALL)
    RJ._same_handles(g, ref, B, ALL)
    g.close(); ref.close()
