"""The KKT sweeps without refinement on top, against the CPU oracle under the same settings.

Every KKT solve is a pair of triangular sweeps followed by iterative refinement, and under the default settings (nitref = 9, linsysacc =
1e-14) refinement repairs what a subtly wrong sweep got wrong: the answer stays, only the refinement effort grows.  So this file compares

  * the first rows of the per-pass trace at nitref = 0 (what the raw sweeps produce) with the oracle's at nitref = 0, on every forced
    build of the solve kernel and on the paths the four variant fixtures do not reach;
  * whole unrefined runs on LPs (exit code, iteration count, optimality conditions from the raw data);
  * the refinement effort under the defaults (n_ldlsolve, nitref1, nitref2) with the oracle's.

The CPU part is the calibration of those comparisons, on the oracle alone.  oracle_debug_perturb_sweep makes the oracle's backward
substitution wrong on purpose (the last stored entry of every column j % 7 == 3 of L scaled by 1 + rel), and liboracle_fma.so is a second,
legitimate rounding of the same source.  The calibration shows: a sweep wrong by 1e-3 passes the default-settings comparison of
test_gpu_parity.py (b); legitimate rounding moves rows 0 and 1 of the unrefined trace by less than 1e-6 / 30 (a); the 1e-3 sweep error
moves them by more than 1e-4 (c).  1e-6 is the bound test_trajectory_matches_oracle_iteration_by_iteration holds early rows to.

The row deviation (ROW_TOL is compared with it) is the maximum over trace columns 0-10 of |a - b| / scale, where pcost and dcost are scaled
by max(1, |pcost|, |dcost|) of the reference row and every other column by max(|reference|, 1e-8)."""
import os

import numpy as np
import pytest

from conftest import ALL_FIXTURES, GOLDEN, load_fixture
import eicos_amd
from eicos_amd.generate import feasible_batch, mpc_soc_variant, random_socp_pattern
from eicos_amd.problem_io import Values
from oracle.oracle import OracleSolver, default_settings, lib_fma
from test_gpu_parity import KERNEL_VARIANT_ENVS, KERNEL_VARIANT_FIXTURES, dense_front_pattern
from test_oracle_golden import in_cone, kkt_residuals
from test_settings import BUILDS, DEF256

KEYS = ("Gpr", "Apr", "c", "h", "b")
ROW_TOL = 1e-6         # GPU row deviation at nitref = 0 (set by the trajectory test's early-row bound, never by what the GPU gives)
ROUNDING = ROW_TOL / 30  # what two legitimate roundings of the oracle may differ by in a compared row: calibration (a)
POWER = 1e-4           # what a wrong sweep must move a compared row by: calibration (c), 100 x ROW_TOL
RATIO_CAP = 1.25       # GPU n_ldlsolve / oracle n_ldlsolve under the defaults (the 1e-6 perturbation gives >= 1.5 but on issue98)
# The trace rows compared per case: rows 0 and 1, row 2 where (a) holds for it at ROUNDING, row 0 alone where (a) fails at row 1
# (test_calibration_a_... asserts (a) for exactly these rows).  Measured portable-vs-FMA deviations of rows 0 / 1 / 2:
#   lp_bandm 7e-10 / 1e-8 / 4e-9     update_data 3e-10 / 2e-9 / 5e-9   issue98 0 / 2e-10 / 1e-8     lp_afiro <= 1e-14
#   MPC02 1e-10 / 5e-9 / 7e-9        MPC-SOC 6e-10 / 5e-9 / 2e-8       infeasible1 0 / 5e-10 / 2e-7 (row 2 out)
#   dense-front 3e-11 / 3.9e-8 / 1.5e-6 (row 1 misses 3.3e-8: row 0 only)
ROWS = {"lp_bandm": (0, 1, 2), "update_data": (0, 1, 2), "issue98": (0, 1, 2), "lp_afiro": (0, 1, 2), "MPC02": (0, 1, 2),
        "MPC-SOC": (0, 1, 2), "infeasible1": (0, 1), "dense-front": (0,)}
# random_socp_pattern(60, 10, 20, [40, 33, 2], seed=6), the case for wave and tiny cones, fails (a) in every row: its two big cones leave the
# raw sweeps a delta-regularised system whose unrefined solution is decided by rounding.  Measured: portable vs FMA 1.8e-7 / 3.2e-7 /
# 8.6e-7 in rows 0 / 1 / 2; the portable oracle against itself on data perturbed by 1e-16 relative (48 draws) up to 7.8e-7 / 5.0e-6 /
# 2.2e-6 (medians 3e-7 / 1.6e-6 / 9e-7); the GPU 1.4e-7 / 2.4e-6.  From row 1 on ROW_TOL lies below the reference's own error, so the
# case is held to row 0 alone, where legitimate rounding stays below ROW_TOL by a factor of about 3, not 30 (test_calibration_of_the_
# wave_and_tiny_cone_case asserts that weaker margin) -- and where the 1e-6 sweep error moves the row by 3.8, the 1e-3 one by 3.8e3.
ROWS_THIN_MARGIN = {"socp-wave-tiny": (0,)}
# the ten fixtures whose run at nitref = 0 ends with the default run's exit code and iteration count (test_pinned_inputs): (code, iterations)
PINNED = {"lp_afiro": (0, 9), "update_data": (0, 10), "issue98": (0, 6), "MPC02": (0, 14), "lp_bandm": (0, 21), "lp_blend": (0, 12),
          "lp_adlittle": (0, 12), "infeasible1": (1, 5), "unboundedLP1": (2, 5), "feas": (0, 5)}


# ---- cases and references, computed once ------------------------------------------------------------------------------------------------
_CASES, _ORACLE = {}, {}


def _case(name, B=1):
    """(pattern, batch arrays [B][...]) of a case: ONE instance -- a fixture's own data, or strictly feasible instance 0 (feasible_batch) of
    a generated pattern -- in every row, so that each instance of a GPU batch is the instance that the calibration measured."""
    if name not in _CASES:
        if name == "MPC-SOC":
            pat, sets = load_fixture("MPC02")
            pat = mpc_soc_variant(pat, sets[0])
            one = feasible_batch(pat, sets[0], 0, 1)
        elif name == "dense-front":
            pat, base = dense_front_pattern(n=150, k=4, d=40)
            one = feasible_batch(pat, base, 0, 1)
        elif name == "socp-wave-tiny":
            pat, base = random_socp_pattern(60, 10, 20, [40, 33, 2], seed=6)
            one = feasible_batch(pat, base, 0, 1, seed=106)
        else:
            pat, sets = load_fixture(name)
            one = {k: getattr(sets[0], k)[None, :] for k in KEYS}
        _CASES[name] = (pat, {k: np.ascontiguousarray(one[k][0], dtype=np.float64) for k in KEYS})
    pat, v = _CASES[name]
    return pat, {k: np.repeat(v[k][None, :], B, 0) for k in KEYS}


def _values(d, i):
    return Values(*[d[k][i] for k in KEYS])


def _oracle_run(pat, v, fma=False, perturb=0.0, **settings):
    o = OracleSolver(pat, v, fma=fma)
    if settings:
        o.set_settings(**settings)
    hit = o.perturb_sweep(perturb)
    code = o.solve()
    y, z, s = o.yzs()
    out = dict(code=code, info=o.info(), trace=o.trace().copy(), x=o.x().copy(), y=y.copy(), z=z.copy(), s=s.copy(), perturbed_entries=hit)
    o.close()
    return out


def _oracle(name, **settings):
    """The clean portable oracle on a case under `settings`: solved once, shared, never modified."""
    key = (name, tuple(sorted(settings.items())))
    if key not in _ORACLE:
        pat, d = _case(name)
        _ORACLE[key] = _oracle_run(pat, _values(d, 0), **settings)
    return _ORACLE[key]


def row_deviation(t, ref, rows):
    """Per compared row: max over columns 0-10 of |t - ref| / scale (module docstring)."""
    rows = [r for r in rows if r < min(len(t), len(ref))]
    a, b = t[rows, :11], ref[rows, :11]
    scale = np.maximum(np.abs(b), 1e-8)
    scale[:, 0] = scale[:, 1] = np.maximum(1.0, np.maximum(np.abs(b[:, 0]), np.abs(b[:, 1])))
    return (np.abs(a - b) / scale).max(axis=1)


# ---- CPU: the oracle's settings ----------------------------------------------------------------------------------------------------------
def test_oracle_settings_follow_the_gpu_binding():
    assert default_settings() == eicos_amd.default_settings()
    pat, d = _case("lp_afiro")
    o = OracleSolver(pat, _values(d, 0))
    assert o.settings() == default_settings()
    o.set_settings(feastol=1e-6, nitref=4, iter_max=50, irerrfact=3.0)
    before = o.settings()
    assert before == {**default_settings(), "feastol": 1e-6, "nitref": 4, "iter_max": 50, "irerrfact": 3.0}
    with pytest.raises(TypeError, match="bogus"):
        o.set_settings(feastol=1e-5, bogus=1)
    assert o.settings() == before
    bad = [(k, v) for k in eicos_amd.binding.SETTINGS_FIELDS[:8] for v in (float("nan"), 0.0, -1e-8, float("inf"))]
    bad += [("iter_max", 0), ("iter_max", 101), ("iter_max", -3), ("nitref", -1), ("nitref", 101)]
    for k, v in bad:  # (the list test_settings_validation_names_the_field_and_changes_nothing refuses on the GPU handle)
        with pytest.raises(RuntimeError, match=k):
            o.set_settings(**{k: v})
        assert o.settings() == before, (k, v)
    o.set_settings(iter_max=1, nitref=0)
    o.set_settings(iter_max=100, nitref=100)
    assert o.settings() == {**before, "iter_max": 100, "nitref": 100}
    o.close()


@pytest.mark.parametrize("name", ALL_FIXTURES)
def test_explicit_defaults_change_nothing_in_the_oracle(name):
    pat, sets = load_fixture(name)
    runs = [_oracle_run(pat, sets[0]), _oracle_run(pat, sets[0], **default_settings())]
    assert all(a == b or (a != a and b != b) for a, b in zip(runs[0]["info"].values(), runs[1]["info"].values())), (name, runs[0]["info"], runs[1]["info"])
    for k in ("code", "x", "y", "z", "s", "trace"):
        assert np.array_equal(runs[0][k], runs[1][k], equal_nan=True), (name, k)


@pytest.mark.parametrize("name", ["lp_afiro", "issue98", "MPC02", "lp_bandm"])
def test_default_trace_is_the_recorded_one_bit_for_bit(name):
    """tests/golden/oracle_trace_<name>.npy: OracleSolver.trace() of the oracle as it was while its settings were compile-time constants."""
    pat, sets = load_fixture(name)
    assert np.array_equal(_oracle_run(pat, sets[0])["trace"], np.load(os.path.join(GOLDEN, f"oracle_trace_{name}.npy")))


@pytest.mark.parametrize("name", list(PINNED))
def test_pinned_inputs(name):
    """What makes these fixtures usable for whole unrefined runs: nitref = 0 ends where the default run ends."""
    dflt, raw = _oracle(name), _oracle(name, nitref=0)
    assert (dflt["code"], dflt["info"]["iter"]) == PINNED[name] == (raw["code"], raw["info"]["iter"]), (name, dflt["code"], raw["code"])
    assert (raw["info"]["nitref1"], raw["info"]["nitref2"], raw["info"]["nitref3"]) == (0, 0, 0)
    assert raw["info"]["n_ldlsolve"] == 2 + 3 * raw["info"]["iter"]  # (two initialisation solves, three per completed pass)


# ---- CPU: calibration --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ROWS))
def test_calibration_a_two_roundings_of_the_oracle_agree_in_the_compared_rows(name):
    if lib_fma() is None:
        pytest.skip("no FMA build of the oracle on this machine")
    pat, d = _case(name)
    dev = row_deviation(_oracle_run(pat, _values(d, 0), fma=True, nitref=0)["trace"], _oracle(name, nitref=0)["trace"], (0, 1, 2))
    print(name, "portable vs FMA, rows 0 / 1 / 2:", dev)
    for r in ROWS[name]:
        assert dev[r] <= ROUNDING, (name, r, dev)
    assert 0 in ROWS[name]


@pytest.mark.parametrize("name", ["lp_bandm", "issue98", "infeasible1", "update_data"])
def test_calibration_b_default_settings_do_not_see_a_sweep_that_is_wrong_by_1e_3(name):
    """The documented blindness of the default-settings comparison: what test_every_kernel_variant_matches_oracle asserts of the GPU (and
    x to 1e-8 on top) holds for an oracle whose backward substitution is wrong by 1e-3 in every seventh column."""
    pat, d = _case(name)
    clean, wrong = _oracle(name), _oracle_run(pat, _values(d, 0), perturb=1e-3)
    assert wrong["code"] == clean["code"] and abs(wrong["info"]["iter"] - clean["info"]["iter"]) <= 1
    assert abs(wrong["info"]["pcost"] - clean["info"]["pcost"]) <= 1e-8 * max(1.0, abs(clean["info"]["pcost"]))
    assert np.abs(wrong["x"] - clean["x"]).max() <= 1e-8 * max(1.0, np.abs(clean["x"]).max())
    if wrong["perturbed_entries"]:  # (what it costs instead: refinement effort)
        assert wrong["info"]["n_ldlsolve"] > clean["info"]["n_ldlsolve"]


@pytest.mark.parametrize("name,rel", [(n, 1e-3) for n in ROWS if n != "infeasible1"] +
                         [(n, 1e-6) for n in ("lp_bandm", "update_data", "MPC02", "MPC-SOC", "dense-front")])
def test_calibration_c_unrefined_rows_see_it(name, rel):
    pat, d = _case(name)
    wrong = _oracle_run(pat, _values(d, 0), perturb=rel, nitref=0)
    assert wrong["perturbed_entries"] > 0
    rows = [r for r in ROWS[name] if r < 2]
    dev = row_deviation(wrong["trace"], _oracle(name, nitref=0)["trace"], rows)
    print(name, rel, "rows", rows, dev)
    assert dev.max() >= POWER, (name, rel, dev)


def test_calibration_of_the_wave_and_tiny_cone_case():
    """ROWS_THIN_MARGIN: row 0 alone, two roundings of the oracle within ROW_TOL / 3 of each other, and the power of (c) in that row."""
    name = "socp-wave-tiny"
    pat, d = _case(name)
    clean = _oracle(name, nitref=0)["trace"]
    if lib_fma() is not None:
        dev = row_deviation(_oracle_run(pat, _values(d, 0), fma=True, nitref=0)["trace"], clean, (0, 1, 2))
        print(name, "portable vs FMA, rows 0 / 1 / 2:", dev)
        assert dev[0] <= ROW_TOL / 3, dev
    for rel in (1e-3, 1e-6):
        wrong = _oracle_run(pat, _values(d, 0), perturb=rel, nitref=0)
        assert wrong["perturbed_entries"] > 0 and row_deviation(wrong["trace"], clean, (0,))[0] >= POWER, rel


@pytest.mark.parametrize("name", ["infeasible1", "feas"])
def test_calibration_cases_without_a_perturbed_entry_have_no_power(name):
    """No column j % 7 == 3 of these factors stores an entry: the hook changes nothing, so nobody may count on them in (c)."""
    pat, d = _case(name)
    for nitref in (0, 9):
        wrong = _oracle_run(pat, _values(d, 0), perturb=1e-3, nitref=nitref)
        assert wrong["perturbed_entries"] == 0
        assert np.array_equal(wrong["trace"], _oracle(name, nitref=nitref)["trace"])


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
def _gpu_unrefined(pat, d, B, check=None, device=False, monkeypatch=None):
    """A cold solve at nitref = 0; `check(g)` asserts the path before anything runs.  device=True hands the data over through device
    pointers (update_device), which is what lets a batch share its matrix values."""
    g = eicos_amd.BatchSolver(pat, B)
    try:
        if check:
            check(g, monkeypatch)
        g.set_settings(nitref=0)
        if device:
            from test_shared_values import Dev
            dev = Dev()
            try:
                g.update_device(*dev.put(d))
                assert g.shared_values()  # (identical Gpr / Apr rows: the backward level-0 slices come from the batch's one copy)
                codes = np.asarray(g.solve()).copy()
            finally:
                dev.free()
        else:
            g.update(*[d[k] for k in KEYS])
            codes = np.asarray(g.solve()).copy()
        ia = {k: np.asarray(v).copy() for k, v in g.info_arrays().items()}
        traces = [g.debug_trace(i).copy() for i in range(B)]
        y, z, s = g.duals()
        return dict(codes=codes, ia=ia, traces=traces, x=g.solution().copy(), y=y.copy(), z=z.copy(), s=s.copy())
    finally:
        g.close()


def _assert_first_rows(what, name, B, got, rows):
    assert (got["ia"]["nitref1"] == 0).all() and (got["ia"]["nitref2"] == 0).all() and (got["ia"]["nitref3"] == 0).all(), what
    worst = np.zeros(len(rows))
    want = _oracle(name, nitref=0)
    for i in range(B):
        assert got["ia"]["iter"][i] >= max(rows) and want["info"]["iter"] >= max(rows), what  # (the rows exist in both traces)
        worst = np.maximum(worst, row_deviation(got["traces"][i], want["trace"], rows))
    print("UNREFINED-ROWS", what, "rows", rows, "deviation", worst)
    assert (worst <= ROW_TOL).all(), (what, rows, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("env", KERNEL_VARIANT_ENVS)
def test_first_passes_unrefined_on_every_build(env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    B = 2
    for name in KERNEL_VARIANT_FIXTURES:
        pat, d = _case(name, B)
        _assert_first_rows((env, name), name, B, _gpu_unrefined(pat, d, B), ROWS[name])


def _is_build(build):
    def check(g, monkeypatch=None):
        if build == "no-lds":
            assert g.dims()["lds_bytes"] == 0
        else:
            assert (g.kernel_build(), g.dims()["threads_per_block"]) == build, (g.kernel_build(), g.dims()["threads_per_block"])
    return check


def _both(*checks):
    def check(g, monkeypatch):
        for c in checks:
            c(g, monkeypatch)
    return check


def _dims(**want):
    def check(g, monkeypatch=None):
        d = g.dims()
        assert {k: d[k] for k in want} == want, d
    return check


def _wave_and_tiny_cones(g, monkeypatch=None):
    # (the cone classes are a function of the dimensions alone, device_types.hpp: a wavefront per cone from 32 to 64 rows, a thread per
    # cone of two rows; dims() has no field for them)
    q = [int(v) for v in g.pat.q]
    assert g.dims()["ncones"] == 3 and sorted(q) == [2, 33, 40]


def _no_g_tiles(g, monkeypatch):
    monkeypatch.setenv("EICOS_GTILES", "1")
    tiled = eicos_amd.BatchSolver(g.pat, g.batch)
    small = tiled.dims()["inst_bytes"]
    tiled.close()
    monkeypatch.setenv("EICOS_GTILES", "0")
    assert g.dims()["inst_bytes"] > small  # (the two ELL copies of G are back in the instance slab)


# MPC02 on the builds of test_settings.py, and the paths no variant fixture reaches: (id, case, B, environment, path check, device pointers)
MPC02_BUILDS = [(env, build) for name, _, env, build in BUILDS if name == "MPC02"]
OTHER_PATHS = [("MPC02-" + "-".join(map(str, build)) if isinstance(build, tuple) else "MPC02-" + build, "MPC02", 2, env, _is_build(build), False)
               for env, build in MPC02_BUILDS]
OTHER_PATHS += [
    ("MPC02-default-256-dual", "MPC02", 2, DEF256, _both(_is_build(("default", 256)), _dims(dual_rhs=1)), False),
    ("MPC02-default-256-single", "MPC02", 2, {**DEF256, "EICOS_DUAL": "0"}, _both(_is_build(("default", 256)), _dims(dual_rhs=0)), False),
    ("lp_afiro-lds-resident", "lp_afiro", 2, {}, _both(_is_build(("lds-resident", 128)), _dims(lds_resident=1)), False),
    ("dense-front-tiles-dual", "dense-front", 2, {}, _dims(factor_path=1, dual_rhs=1), False),
    ("dense-front-no-g-tiles", "dense-front", 2, {"EICOS_GTILES": "0"}, _both(_dims(factor_path=1), _no_g_tiles), False),
    ("MPC-SOC", "MPC-SOC", 2, {}, _dims(ncones=332, l=3000), False),
    ("socp-wave-tiny", "socp-wave-tiny", 2, {}, _wave_and_tiny_cones, False),
    ("MPC02-shared-copy", "MPC02", 4, {}, _dims(shared_operands=1), True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("label,name,B,env,check,device", OTHER_PATHS, ids=[c[0] for c in OTHER_PATHS])
def test_first_passes_unrefined_on_the_other_paths(label, name, B, env, check, device, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pat, d = _case(name, B)
    rows = {**ROWS, **ROWS_THIN_MARGIN}[name]
    _assert_first_rows(label, name, B, _gpu_unrefined(pat, d, B, check, device, monkeypatch), rows)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lp_afiro", "update_data", "MPC02", "lp_bandm", "infeasible1", "unboundedLP1", "feas"])
def test_whole_unrefined_runs_on_lps(name):
    B = 2
    pat, d = _case(name, B)
    got, want = _gpu_unrefined(pat, d, B), _oracle(name, nitref=0)
    print("UNREFINED-RUN", name, "codes", got["codes"], "iter", got["ia"]["iter"], "oracle", want["code"], want["info"]["iter"])
    assert list(got["codes"]) == [want["code"]] * B, (name, got["codes"], want["code"])
    assert (np.abs(got["ia"]["iter"] - want["info"]["iter"]) <= 1).all(), (name, got["ia"]["iter"], want["info"]["iter"])
    if want["code"] in (0, 10):  # (the thresholds of test_fixture_matches_oracle; none of them depends on the oracle)
        for i in range(B):
            v = _values(d, i)
            rp, re, rd, gap = kkt_residuals(pat, v, got["x"][i], got["y"][i], got["z"][i], got["s"][i])
            print("UNREFINED-RUN", name, i, "residuals", rp, re, rd, "gap", gap)
            assert max(rp, re, rd) < 1e-6 and abs(gap) < 1e-6 * max(1.0, abs(got["ia"]["pcost"][i])), (name, rp, re, rd, gap)
            assert in_cone(pat, got["s"][i], 1e-7) and in_cone(pat, got["z"][i], 1e-7), name


# environment sets whose clean build exceeds RATIO_CAP, each with its measured ratio (at most three: more means the assertion goes)
RATIO_EXEMPT = {}


def _assert_effort(what, name, B, pat, d, exempt_ratio):
    g = eicos_amd.BatchSolver(pat, B)
    try:
        g.update(*[d[k] for k in KEYS])
        codes = np.asarray(g.solve()).copy()
        ia = {k: np.asarray(v).copy() for k, v in g.info_arrays().items()}
    finally:
        g.close()
    want = _oracle(name)
    oi = want["info"]
    for i in range(B):
        assert codes[i] == want["code"], (what, codes, want["code"])
        ratio = ia["n_ldlsolve"][i] / oi["n_ldlsolve"]
        print("EFFORT", what, i, "iter", ia["iter"][i], oi["iter"], "n_ldlsolve", ia["n_ldlsolve"][i], oi["n_ldlsolve"], "ratio %.3f" % ratio,
              "nitref1", ia["nitref1"][i], oi["nitref1"], "nitref2", ia["nitref2"][i], oi["nitref2"])
        assert ia["nitref1"][i] <= oi["nitref1"] + 1 and ia["nitref2"][i] <= oi["nitref2"] + 1, (what, ia["nitref1"][i], ia["nitref2"][i], oi)
        if ia["iter"][i] == oi["iter"] and not exempt_ratio:
            assert ratio <= RATIO_CAP, (what, ia["n_ldlsolve"][i], oi["n_ldlsolve"])


@pytest.mark.gpu
@pytest.mark.parametrize("env", KERNEL_VARIANT_ENVS)
def test_refinement_effort_under_the_defaults_on_every_build(env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    B = 2
    for name in KERNEL_VARIANT_FIXTURES:
        pat, d = _case(name, B)
        # (issue98: the 1e-6 perturbation raises its n_ldlsolve by 49 -> 53 only, a ratio below the cap: no power, so no ratio assertion)
        _assert_effort((env, name), name, B, pat, d, name == "issue98" or tuple(sorted(env.items())) in RATIO_EXEMPT)


@pytest.mark.gpu
@pytest.mark.parametrize("env,build", MPC02_BUILDS, ids=[str(b) for _, b in MPC02_BUILDS])
def test_refinement_effort_under_the_defaults_on_the_mpc02_builds(env, build, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    B = 2
    pat, d = _case("MPC02", B)
    g = eicos_amd.BatchSolver(pat, B)
    try:
        _is_build(build)(g)
    finally:
        g.close()
    _assert_effort(("MPC02", build), "MPC02", B, pat, d, False)
