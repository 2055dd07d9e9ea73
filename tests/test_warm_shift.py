"""A caller-supplied starting point and the warm-start shift map (eicos_batch_set_iterate / _set_iterate_device / _set_shift_map /
_has_shift_map and their eicos_multi_* forms, include/eicos_amd.h).

set_iterate writes rows of x, y, z, s into the instance slabs and marks the instances warm-startable.  A shift map -- per vector a square
affine map -- is applied by the solve kernel itself to every instance it warm-starts, before the warm start's re-equilibration and cone
push.  The contract is bit-identity: a solve of a handle with a shift map and warm start > 0 leaves exactly the state of a twin without
the map on which the host fetches solution() / duals() of the instances whose last exit code is 0 or 10, evaluates the map
(ShiftMap.evaluate) and calls set_iterate with the result before the same solve -- on every build of the solve kernel, for single solves
and inside a rollout, fused or per step.  Every GPU comparison is np.array_equal: the feature adds no arithmetic freedom.  The CPU tests
check ShiftMap.evaluate, from_sources and the refusals that need no GPU."""
import ctypes as C

import numpy as np
import pytest

import eicos_amd
from eicos_amd import binding
from eicos_amd.binding import ShiftMap
import test_param_update as P  # (its _data, _map, _theta, _twins)
import test_rhs_update as R    # (its _second_rhs, _outputs, _assert_same and device-array helpers)
import test_rollout as RO      # (its _fmap, _w, _host_loop, _assert_rollout and the table of solve-kernel builds)
import test_matrix_param as MM  # (its _mmap)
from test_param_step import _omap

KEYS = R.KEYS
DP = C.POINTER(C.c_double)


def _identity(rows):
    return [np.array([j], np.int64) for j in range(rows)], [np.ones(1) for _ in range(rows)]


def _group(rng, rows, frac, cross=(), min_alt=3):
    """One group of the test map: identity rows (new[j] = old[j]), of which about `frac` are altered in turn into a copy from another
    index, a two-entry combination (stored with the larger column first: unsorted), and an empty row (new[j] = base[j] = 0); `cross` =
    (row, column) pairs that copy an entry across a cone boundary."""
    cols, vals = _identity(rows)
    base = np.zeros(rows)
    n_alt = min(rows, max(min_alt, int(round(frac * rows)))) if rows >= 2 else 0
    for q, j in enumerate(rng.choice(rows, n_alt, replace=False) if n_alt else ()):
        other = int((j + 1 + rng.integers(0, rows - 1)) % rows)
        if q % 3 == 0:
            cols[j], vals[j] = np.array([other]), np.ones(1)
        elif q % 3 == 1:
            pair = sorted((int(j), other), reverse=True)
            cols[j], vals[j] = np.array(pair), np.array([0.75, 0.25])
        else:
            cols[j], vals[j] = np.zeros(0, np.int64), np.zeros(0)
    for j, c in cross:
        cols[j], vals[j] = np.array([c]), np.ones(1)
    rowptr = np.concatenate(([0], np.cumsum([len(c) for c in cols]))).astype(np.int32)
    return base, rowptr, np.concatenate(cols).astype(np.int32), np.concatenate(vals)


def _smap(pat, seed=0, frac=0.1, groups="xyzs", min_alt=3, cross_groups="zs"):
    """The shift map of a case: mostly identity rows, about a tenth altered (_group); on a pattern with cones, rows of z and s that
    move entries across the boundary between the LP rows and the first cone and between two cones (`cross_groups`: the groups that get
    those rows).  A group the pattern does not have
    gets no map -- the library refuses one (test_shift_map_replace_remove_refuse)."""
    rng = np.random.default_rng(8000 + seed)
    cross = []
    q = [int(v) for v in pat.q][:pat.ncones]
    if q:
        l = pat.l
        if l > 0:
            cross += [(l - 1, l), (l, l - 1)]               # the last LP row takes a cone head, the head takes the LP row
        if len(q) >= 2:
            cross += [(l + q[0], l + q[0] - 1), (l + 1, l + q[0])]  # the second cone's head takes the first cone's last entry, and back
    rows = {"x": pat.n, "y": pat.p, "z": pat.m, "s": pat.m}
    return ShiftMap(pat.n, pat.p, pat.m, **{g: _group(rng, rows[g], frac, cross if g in cross_groups else (), min_alt) for g in groups if rows[g] > 0})


def _host_shift(ref, sm):
    """The contract's host sequence on handle `ref`: solution() and duals() of the instances whose last exit code is 0 or 10 through the
    map on the host, written back with set_iterate (one call per run of such instances); an unmapped group is not passed."""
    codes = np.asarray(ref.info_arrays()["exitcode"])
    x = ref.solution(); y, z, s = ref.duals()
    new = sm.evaluate(x, y, z, s)
    new = [v if g is not None else None for v, g in zip(new, sm.groups())]
    idx = np.nonzero((codes == 0) | (codes == 10))[0]
    if idx.size == 0:
        return
    cuts = np.nonzero(np.diff(idx) > 1)[0] + 1
    for run in np.split(idx, cuts):
        a, b = int(run[0]), int(run[-1]) + 1
        ref.set_iterate(*[None if v is None else v[a:b] for v in new], first=a, count=b - a)


class _ShiftedHost:
    """A handle as RO._host_loop drives it, with the contract's host sequence in front of every update_param_solve."""

    def __init__(self, ref, sm):
        self.ref, self.sm = ref, sm

    def update_param_solve(self, *a, **kw):
        _host_shift(self.ref, self.sm)
        return self.ref.update_param_solve(*a, **kw)

    def info_arrays(self):
        return self.ref.info_arrays()


def _state(g):
    return R._outputs(g, g.info_arrays()["exitcode"])


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_warm_shift_entry_points_refuse_a_null_handle():
    L = binding._lib()
    dp = np.zeros(4).ctypes.data_as(DP)
    err = L.eicos_last_error
    for rc in (L.eicos_batch_set_iterate(None, 0, 1, dp, None, None, None), L.eicos_batch_set_iterate_device(None, 0, 1, None, None, None, None),
               L.eicos_batch_set_shift_map(None, None, None, None, None), L.eicos_batch_has_shift_map(None)):
        assert rc == -1 and b"NULL handle" in err()
    err = L.eicos_multi_last_error
    for rc in (L.eicos_multi_set_iterate(None, 0, 1, dp, None, None, None), L.eicos_multi_set_shift_map(None, None, None, None, None),
               L.eicos_multi_has_shift_map(None)):
        assert rc == -1 and b"NULL handle" in err()


def test_shift_map_evaluate_equals_a_scalar_loop_in_the_stated_order():
    # new[j] = base[j]; for t in stored order: new[j] = new[j] + (val[t] * old[col[t]]) on Python floats (IEEE doubles, no fused
    # multiply-add); old = the vector before the shift, whatever rows were formed before row j
    base = np.array([0.1, -2.5, 3.0, 1e-3])
    rowptr = np.array([0, 4, 4, 5, 9], np.int32)
    col = np.array([3, 0, 2, 1, 1, 2, 0, 2, 3], np.int32)  # (row 1 is empty; rows 0 and 3 are not sorted; row 3 holds column 2 twice)
    val = np.array([1 / 3, 1e-7, -0.7, 0.9, 2 / 7, 1e10, 0.3, -1e10, 1 / 7])  # (the two entries of row 3 on column 2 cancel)
    old = np.array([[0.1, 0.7, 1 / 9, 0.3], [0.9, 0.7, 0.123456789, -0.2]])
    other = np.array([[1.0, 2.0], [3.0, 4.0]])
    sm = ShiftMap(4, 2, 4, x=(base, rowptr, col, val), s=(base, rowptr, col, val))
    gx, gy, gz, gs = sm.evaluate(old, other, old, 2 * old)
    assert gy is other and gz is old  # (groups without a map come back as they were passed)
    for got, v in ((gx, old), (gs, 2 * old)):
        assert got.shape == (2, 4)
        for i in range(2):
            for j in range(4):
                acc = float(base[j])
                for t in range(rowptr[j], rowptr[j + 1]):
                    acc = acc + (float(val[t]) * float(v[i, col[t]]))
                assert got[i, j] == acc, (i, j)


def test_shift_map_evaluate_matches_a_dense_product():
    rng = np.random.default_rng(11)
    B = 5
    for rows in (2, 9, 64):
        base, rowptr, col, val = _group(rng, rows, 0.3)
        base = rng.standard_normal(rows)
        val = val * rng.uniform(0.5, 1.5, val.size)
        sm = ShiftMap(rows, 0, rows, x=(base, rowptr, col, val), z=(base, rowptr, col, val))
        v = rng.standard_normal((B, rows))
        M = np.zeros((rows, rows))
        for j in range(rows):
            np.add.at(M[j], col[rowptr[j]:rowptr[j + 1]], val[rowptr[j]:rowptr[j + 1]])
        want = base[None, :] + v @ M.T
        gx, _, gz, gs = sm.evaluate(x=v, z=v)
        assert gs is None
        for got in (gx, gz):
            assert np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(want))


def test_shift_map_from_sources_reproduces_the_source_entries():
    rng = np.random.default_rng(12)
    n, p, m, B = 12, 3, 7, 4
    x_src = np.minimum(np.arange(n) + 3, n - 1)  # stage t <- stage t + 1 with a stage of 3 variables, the last stage kept
    z_src = rng.integers(0, m, m)
    sm = ShiftMap.from_sources(n, p, m, x_src=x_src, z_src=z_src)
    assert sm.y is None and sm.s is None
    x, y, z, s = rng.standard_normal((B, n)), rng.standard_normal((B, p)), rng.standard_normal((B, m)), rng.standard_normal((B, m))
    gx, gy, gz, gs = sm.evaluate(x, y, z, s)
    assert np.array_equal(gx, x[:, x_src]) and np.array_equal(gz, z[:, z_src]) and gy is y and gs is s
    assert np.array_equal(sm.x[0], np.zeros(n)) and np.array_equal(sm.x[3], np.ones(n)) and np.array_equal(sm.x[1], np.arange(n + 1))


def test_shift_arrays_of_the_wrong_shape_are_refused_before_the_library_is_called():
    pat, _ = R.load_fixture("lp_afiro")
    n, p, m = pat.n, pat.p, pat.m
    ok = ShiftMap.from_sources(n, p, m, x_src=np.arange(n), s_src=np.arange(m))
    keep, ptrs = binding._shift_map_ptrs(ok, pat)
    assert ptrs[0] is not None and ptrs[1] is None and ptrs[2] is None and ptrs[3] is not None
    with pytest.raises(ValueError):  # sources of the wrong length
        ShiftMap.from_sources(n, p, m, x_src=np.arange(n + 1))
    with pytest.raises(ValueError):  # a base of the wrong length
        binding._shift_map_ptrs(ShiftMap(n, p, m, x=(np.zeros(n + 1), np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n))), pat)
    with pytest.raises(ValueError):  # row pointers that run past the stored entries
        binding._shift_map_ptrs(ShiftMap(n, p, m, z=(np.zeros(m), np.arange(m + 1, dtype=np.int32) * 2, np.zeros(m, np.int32), np.ones(m))), pat)
    with pytest.raises(ValueError):  # a map made for another pattern
        binding._shift_map_ptrs(ShiftMap.from_sources(n + 1, p, m, x_src=np.arange(n + 1)), pat)
    with pytest.raises(ValueError):
        ok.evaluate(x=np.zeros((3, n + 1)))
    with pytest.raises(ValueError):
        ok.evaluate(s=np.zeros(m))

    class _Never(binding._Solver):  # (set_iterate checks the shapes before it touches the handle: none is needed)
        def __init__(self):
            self.pat, self.batch, self._h = pat, 4, None

        def _call(self, *a):
            raise AssertionError("the library was called")

    for bad in (dict(x=np.zeros((4, n + 1))), dict(z=np.zeros((3, m)), count=4), dict(x=np.zeros((4, n)), s=np.zeros((4, m + 1))),
                dict(y=np.zeros(4 * p))):
        with pytest.raises(ValueError):
            _Never().set_iterate(**bad)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def _own(g):
    x = g.solution(); y, z, s = g.duals()
    return x, y, z, s


@pytest.mark.gpu
@pytest.mark.parametrize("memory", ["pageable", "pinned", "device", "sub-range"])
def test_set_iterate_of_an_instances_own_solution_changes_nothing(memory):
    B = 40
    pat, d = P._data("MPC02", B)
    g, ref = P._twins(pat, d, B)
    for s_ in (g, ref):
        s_.set_warm_start(0.1)
        s_.update_rhs(*R._second_rhs(d))
    own = _own(g)
    before = _state(g)
    if memory == "pageable":
        g.set_iterate(*own)
        assert g.last_update_path() == "pinned bounce"
    elif memory == "pinned":
        pins = [eicos_amd.PinnedArray(a.shape) for a in own]
        for p_, a in zip(pins, own):
            p_.a[...] = a
        g.set_iterate(*[p_.a for p_ in pins])
        assert g.last_update_path() == "pinned source in place"
        for p_ in pins:
            p_.a[...] = np.nan  # (the call is synchronous: the arrays are the caller's again)
    elif memory == "device":
        dev = R._device_arrays(own)
        g.set_iterate_device(*dev)
        g.sync()
        R._free_device(dev)
    else:
        first, count = 13, 11
        g.set_iterate(*[a[first:first + count] for a in own], first=first, count=count)
    R._assert_same(_state(g), before, (memory, "before the solve"))
    R._assert_same(R._outputs(g, g.solve()), R._outputs(ref, ref.solve()), memory)
    if memory == "sub-range":
        # other values into a sub-range: those rows read back exactly, every other instance keeps its vectors and its record
        first, count = 7, 5
        own = _own(g)
        before = _state(g)
        new = [1.5 * a[first:first + count] + 0.25 for a in own]
        g.set_iterate(*new, first=first, count=count)
        after = _state(g)
        for k_, (a, b) in enumerate(zip(after, before)):
            if 1 <= k_ <= 4:
                want = b.copy(); want[first:first + count] = new[k_ - 1]
                assert np.array_equal(a, want), k_
            else:
                assert np.array_equal(a, b, equal_nan=True), k_  # (exit codes were OPTIMAL already: the record is as it was)
    g.close(); ref.close()


@pytest.mark.gpu
def test_a_never_solved_instance_starts_from_the_supplied_point():
    from eicos_amd.problem_io import Values
    from oracle.oracle import OracleSolver
    B = 8
    pat, d = P._data("MPC02", B)
    c2, h2, b2 = R._second_rhs(d)
    # the oracle's own spread between a warm re-solve from the neighbouring right-hand side's solution and the cold solve
    spread = 0.0
    for i in range(B):
        o = OracleSolver(pat, Values(d["Gpr"][i], d["Apr"][i], c2[i], h2[i], b2[i]))
        o.set_warm_start(0.1)
        assert o.solve() == 0
        o.update(Values(d["Gpr"][i], d["Apr"][i], d["c"][i], d["h"][i], d["b"][i]))
        assert o.solve() == 0
        warm_it, warm_pc = o.info()["iter"], o.info()["pcost"]
        o.close()
        o = OracleSolver(pat, Values(d["Gpr"][i], d["Apr"][i], d["c"][i], d["h"][i], d["b"][i]))
        assert o.solve() == 0
        print(f"oracle instance {i}: warm {warm_it} iterations, cold {o.info()['iter']}, pcost warm - cold = {warm_pc - o.info()['pcost']:.3e}")
        spread = max(spread, abs(warm_pc - o.info()["pcost"]) / max(1.0, abs(o.info()["pcost"])))
        o.close()
    print(f"oracle warm-minus-cold spread: {spread:.3e} relative")
    assert spread <= 1e-7  # (otherwise the bound below would have to be ten times the oracle's spread)
    # the point: what a twin found for the second right-hand sides
    twin = eicos_amd.BatchSolver(pat, B)
    twin.update(d["Gpr"], d["Apr"], c2, h2, b2)
    assert (twin.solve() == 0).all()
    point = _own(twin)
    twin.close()
    cold = eicos_amd.BatchSolver(pat, B)
    cold.update(*[d[k_] for k_ in KEYS])
    assert (cold.solve() == 0).all()
    ia_cold = cold.info_arrays()
    cold.close()
    a = eicos_amd.BatchSolver(pat, B)
    a.update(*[d[k_] for k_ in KEYS])
    a.set_iterate(*point)
    ia = a.info_arrays()
    assert (ia["exitcode"] == 0).all() and (ia["n_factor"] == 1).all() and (ia["iter"] == 0).all()
    R._assert_same(_own(a), point, "the point reads back")
    a.set_warm_start(0.1)
    codes = a.solve()
    ia = a.info_arrays()
    print("iterations from the supplied point", ia["iter"], "cold", ia_cold["iter"])
    print("pcost - cold", ia["pcost"] - ia_cold["pcost"])
    assert (codes == 0).all()
    assert (ia["nitref1"] == 0).all()  # (the warm path: no initialisation solves)
    assert (ia["iter"] < ia_cold["iter"]).all(), (ia["iter"], ia_cold["iter"])
    assert (np.abs(ia["pcost"] - ia_cold["pcost"]) <= 1e-6 * np.maximum(1.0, np.abs(ia_cold["pcost"]))).all()
    # with warm start 0 a supplied point is ignored: the solve runs cold and overwrites it
    a.update(*[d[k_] for k_ in KEYS])
    a.set_iterate(*point)
    a.set_warm_start(0.0)
    a.solve()
    assert np.array_equal(a.info_arrays()["iter"], ia_cold["iter"])
    a.close()


def _compare_single(name, B, env=None, build=None, monkeypatch=None, no_lds=False):
    """Twins after update(...); solve(), warm start 0.1: the shift map on one, the host sequence on the other, then
    update_rhs(_second_rhs) and solve on both -- every output and the KKT values of the last instance equal bit for bit."""
    for k_, v in (env or {}).items():
        monkeypatch.setenv(k_, v)
    pat, d = P._data(name, B)
    sm = _smap(pat)
    g, ref = P._twins(pat, d, B)
    assert g.dims() == ref.dims() and g.kernel_build() == ref.kernel_build()
    if build is not None:
        assert (g.kernel_build(), g.dims()["threads_per_block"]) == build, (g.kernel_build(), g.dims()["threads_per_block"])
    if no_lds:
        assert g.dims()["lds_bytes"] == 0
    for s_ in (g, ref):
        assert (np.asarray(s_.info_arrays()["exitcode"]) == 0).all(), name  # (every instance will be warm-started: the case proves something)
        s_.set_warm_start(0.1)
    assert g.has_shift_map() == 0
    g.set_shift_map(sm)
    assert g.has_shift_map() == sum(1 << q for q, grp in enumerate(sm.groups()) if grp is not None) and ref.has_shift_map() == 0
    _host_shift(ref, sm)
    for s_ in (g, ref):
        s_.update_rhs(*R._second_rhs(d))
    what = (name, B, env)
    R._assert_same(R._outputs(g, g.solve()), R._outputs(ref, ref.solve()), what)
    assert np.array_equal(g.debug_kkt(B - 1)[2], ref.debug_kkt(B - 1)[2], equal_nan=True), what
    assert (g.info_arrays()["nitref1"] == 0).all()  # (the warm path: no initialisation solves)
    g.close(); ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,B", [
    ("MPC02", 40),
    ("MPC02", 600),       # more instances than resident workgroups: the queue
    ("lp_afiro", 16),     # the LDS-resident build where the handle reports it
    ("issue98", 8),       # cones: rows of z and s cross the cone boundaries
    ("socp-random", 8),   # cones and equality rows: the y map
    ("dense-front", 6),   # the tile path
])
def test_shift_map_is_bit_identical_to_the_host_sequence(name, B):
    _compare_single(name, B)


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
def test_shift_map_on_every_build_of_the_solve_kernel(name, B, env, build, monkeypatch):
    # (the table of test_rollout_on_every_build_of_the_solve_kernel: the seven compilations of k_solve all carry the shift)
    _compare_single(name, B, env, build, monkeypatch)


@pytest.mark.gpu
def test_shift_map_on_a_handle_without_an_lds_vector(monkeypatch):
    # the old values are staged in the workspace's sweep vector instead
    _compare_single("MPC02", 40, {"EICOS_NLDS": "0", "EICOS_DUAL": "0"}, None, monkeypatch, no_lds=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,T,env,matrix,launches,mild", [
    ("MPC02", 40, 3, {}, False, 1, {}),
    ("MPC02", 40, 3, {"EICOS_FUSED_UPDATE": "0"}, False, 3, {}),
    ("issue98", 8, 3, {}, False, None, dict(min_alt=1, groups="xs")),
    ("MPC02", 8, 2, {}, True, 1, {}),   # the matrix map of test_matrix_param.py installed as well
])
def test_rollout_with_a_shift_map_against_the_host_loop(name, B, T, env, matrix, launches, mild, monkeypatch):
    """mild: what makes the shift map of a case milder than _smap's default, so that the case meets its condition (at every step after
    the first at least half of the instances warm-startable, all of them on the plain MPC02 cases).  issue98 is a degenerate problem
    (h = 0, x and s of the order 1e-10 at the optimum, 5 variables, 6 LP rows and one cone of 5).  On an MI355X its rollout gave, per
    step, these exit codes / iteration counts: cold 0 0 0 / 6 6 6; warm without a map 0 0 0 / 9 10 9; one altered row of x only, or
    one altered row of s with the cone-boundary rows of s, the same; but with the two cone-boundary rows in z (the last LP row takes
    the cone head and the head takes the LP row) -2 0 -2 / 0 6 0, whatever else the map holds -- the unchanged warm path leaves that
    point after one iteration through its safeguard and restores iteration 0.  So the map of this case shifts x and s only, one
    altered row each, and crosses the cone boundary in s; the assertion on the share is as the case was set.  The plain MPC02 cases gave share 1, 1, 1
    with 29.15 / 13 / 13 mean iterations."""
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    k, r = 7, 6
    pat, d = P._data(name, B)
    pm, om, fm, sm = P._map(d, k), _omap(pat.n, r), RO._fmap(k, r), _smap(pat, **mild)
    mm = MM._mmap(d, k) if matrix else None
    g, ref = P._twins(pat, d, B)
    first = np.asarray(g.info_arrays()["exitcode"]).copy()
    for s_ in (g, ref):
        s_.set_warm_start(0.1)
        s_.set_param_map(pm); s_.set_output_map(om)
        if mm is not None:
            s_.set_matrix_map(mm)
    g.set_plant_map(fm); g.set_shift_map(sm)
    theta0, w = P._theta(B, k), RO._w(B, T, k)
    want = RO._host_loop(_ShiftedHost(ref, sm), fm, theta0, T, w)
    got = g.rollout(theta0, T, w)
    what = (name, B, T, env, matrix)
    if launches is not None:
        assert g.last_rollout_launches() == launches, (what, g.last_rollout_launches())
    # the condition of the case, read from the codes the rollout returns: the instances that a step warm-started (and shifted)
    prev = np.concatenate((first[:, None], got[2][:, :-1]), axis=1)
    share = np.mean((prev == 0) | (prev == 10), axis=0)
    print("warm-startable share per step", share, "iterations", got[3].mean(axis=0))
    assert (share[1:] >= 0.5).all(), (what, share)
    if name == "MPC02" and not matrix:
        assert (share == 1.0).all(), (what, share)
    RO._assert_rollout(got, want, what)
    R._assert_same(R._outputs(g, RO._final_codes(g)), R._outputs(ref, RO._final_codes(ref)), what)
    assert np.array_equal(got[2][:, -1], RO._final_codes(g)), what
    assert np.array_equal(g.debug_kkt(B - 1)[2], ref.debug_kkt(B - 1)[2], equal_nan=True), what
    g.close(); ref.close()


@pytest.mark.gpu
def test_shift_map_replace_remove_refuse():
    B = 8
    pat, d = P._data("MPC02", B)
    sm1, sm2 = _smap(pat, seed=1), _smap(pat, seed=2, groups="xs")
    rhs2 = R._second_rhs(d)

    def handle(warm=0.1):
        g = eicos_amd.BatchSolver(pat, B)
        g.update(*[d[k_] for k_ in KEYS])
        assert (g.solve() == 0).all()
        g.set_warm_start(warm)
        return g

    def step(g):
        g.update_rhs(*rhs2)
        return R._outputs(g, g.solve())

    # a second map replaces the first
    g, ref = handle(), handle()
    g.set_shift_map(sm1); g.set_shift_map(sm2)
    assert g.has_shift_map() == 0b1001
    _host_shift(ref, sm2)
    out2 = step(ref)
    R._assert_same(step(g), out2, "replaced")
    g.close(); ref.close()
    # all groups None removes it: the results of a handle that never had one -- which differ from the shifted ones
    g, ref = handle(), handle()
    g.set_shift_map(sm1)
    g.set_shift_map(ShiftMap(pat.n, pat.p, pat.m))
    assert g.has_shift_map() == 0
    plain = step(ref)
    R._assert_same(step(g), plain, "removed")
    assert not np.array_equal(plain[1], out2[1])
    g.close(); ref.close()
    # with warm start 0 a map changes nothing
    g, ref = handle(0.0), handle(0.0)
    g.set_shift_map(sm1)
    R._assert_same(step(g), step(ref), "warm start 0")
    # refusals of the map
    L = binding._lib()
    err = L.eicos_last_error

    def install(h_, pat_, **groups):
        keep, ptrs = binding._shift_map_ptrs(ShiftMap(pat_.n, pat_.p, pat_.m, **groups), pat_)
        return L.eicos_batch_set_shift_map(h_._h, *ptrs)

    base, rowptr, col, val = sm1.z
    bad = rowptr.copy(); bad[0] = 1
    assert install(g, pat, z=(base, bad, col, val)) == -1 and b"shift map of z" in err() and b"rowptr[0]" in err()
    bad = rowptr.copy(); bad[3] = bad[2] - 1
    assert install(g, pat, s=(base, bad, col, val)) == -1 and b"shift map of s" in err() and b"rowptr decreases" in err()
    bad = col.copy(); bad[-1] = pat.m
    assert install(g, pat, z=(base, rowptr, bad, val)) == -1 and b"outside [0, rows)" in err()
    bad = sm1.x[2].copy(); bad[0] = -1
    assert install(g, pat, x=(sm1.x[0], sm1.x[1], bad, sm1.x[3])) == -1 and b"shift map of x" in err() and b"outside [0, rows)" in err()
    assert g.has_shift_map() == 0b1111  # (a refused map leaves the installed one alone)
    # refusals of set_iterate
    own = _own(g)
    ptr = [a.ctypes.data_as(DP) for a in own]
    assert L.eicos_batch_set_iterate(g._h, 0, B, None, None, None, None) == -1 and b"all NULL" in err()
    assert L.eicos_batch_set_iterate_device(g._h, 0, B, None, None, None, None) == -1 and b"all NULL" in err()
    assert L.eicos_batch_set_iterate(g._h, 2, B - 1, *ptr) == -1 and b"out of bounds" in err()
    assert L.eicos_batch_set_iterate(g._h, -1, 1, *ptr) == -1 and b"out of bounds" in err()
    assert L.eicos_batch_set_iterate_device(g._h, 0, B + 1, *ptr) == -1 and b"out of bounds" in err()
    with pytest.raises(ValueError):
        g.set_iterate(x=own[0][:, :-1])
    g.close(); ref.close()
    # a group the pattern does not have: the dense-front pattern has no equality rows
    pat0, d0 = P._data("dense-front", 2)
    assert pat0.p == 0
    g = eicos_amd.BatchSolver(pat0, 2)
    empty = (np.zeros(0), np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    with pytest.raises(RuntimeError, match="shift map of y: the pattern has no such vector"):
        g.set_shift_map(ShiftMap(pat0.n, 0, pat0.m, y=empty))
    one = np.zeros(2)
    assert L.eicos_batch_set_iterate(g._h, 0, 2, None, one.ctypes.data_as(DP), None, None) == -1 and b"y given" in err() and b"p = 0" in err()
    g.close()


@pytest.mark.gpu
def test_multi_shift_map_and_set_iterate_match_one_handle():
    # device list {0, 0}, ragged shards, arithmetic profile 1 (plans independent of the shard size): the shift map on every shard and
    # set_iterate rows in global instance order, across the shard boundary, give the bits of one handle
    B = 9
    pat, d = P._data("MPC02", B)
    sm = _smap(pat)
    rhs2 = R._second_rhs(d)
    eicos_amd.set_arithmetic_profile(1)
    try:
        one = eicos_amd.BatchSolver(pat, B)
        m = eicos_amd.MultiBatchSolver(pat, B, [0, 0])
        assert m.has_shift_map() == 0
        outs = []
        for s_ in (one, m):
            s_.update(*[d[k_] for k_ in KEYS])
            assert (s_.solve() == 0).all()
            s_.set_warm_start(0.1)
            s_.set_shift_map(sm)
            s_.update_rhs(*rhs2)
            codes = s_.solve()
            x = s_.solution(); y, z, s = s_.duals(); ia = s_.info_arrays()
            outs.append([codes, x, y, z, s] + [ia[k_] for k_ in R.INFO_KEYS])
        assert m.has_shift_map() == 0b1111
        R._assert_same(outs[1], outs[0], "shift map")
        # the host sequence on a third handle gives the same again
        ref = eicos_amd.BatchSolver(pat, B)
        ref.update(*[d[k_] for k_ in KEYS]); ref.solve(); ref.set_warm_start(0.1)
        _host_shift(ref, sm)
        ref.update_rhs(*rhs2)
        R._assert_same(R._outputs(ref, ref.solve()), outs[0], "host sequence")
        ref.close()
        # a starting point for instances [2, 8): both shards take their rows
        first, count = 2, 6
        new = [1.25 * a[first:first + count] + 0.125 for a in outs[0][1:5]]
        outs = []
        for s_ in (one, m):
            s_.set_shift_map(None)
            s_.set_iterate(*new, first=first, count=count)
            x = s_.solution(); y, z, s = s_.duals()
            for a, b in zip((x, y, z, s), new):
                assert np.array_equal(a[first:first + count], b)
            s_.update(*[d[k_] for k_ in KEYS])
            codes = s_.solve()
            x = s_.solution(); y, z, s = s_.duals(); ia = s_.info_arrays()
            outs.append([codes, x, y, z, s] + [ia[k_] for k_ in R.INFO_KEYS])
        R._assert_same(outs[1], outs[0], "set_iterate")
        one.close(); m.close()
    finally:
        eicos_amd.set_arithmetic_profile(0)


@pytest.mark.gpu
def test_cpp_warm_shift_demo_over_a_device_list(tmp_path):
    # examples/warm_shift_demo.cpp: a small stage-ordered MPC written in the program, the same closed-loop rollout cold, warm and warm
    # with the receding-horizon shift map, over the device list {0, 0}; the iteration counts are printed, not asserted
    import os, re, subprocess
    from conftest import ROOT
    exe = str(tmp_path / "warm_shift_demo")
    lib = os.path.join(ROOT, "eicos_amd")
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "warm_shift_demo.cpp"),
                           "-L", lib, "-leicos_amd", "-Wl,-rpath," + lib, "-o", exe])
    out = subprocess.run([exe, "16", "6", "4", "0,0"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "over 2 shard(s)" in out.stdout, out.stdout
    found = dict(re.findall(r"^(cold|warm|warm \+ shift)\s*: mean iterations per step ([0-9.eE+-]+|nan|inf)", out.stdout, re.M))
    assert set(found) == {"cold", "warm", "warm + shift"}, out.stdout
    for v in found.values():
        assert np.isfinite(float(v)) and float(v) > 0, out.stdout
