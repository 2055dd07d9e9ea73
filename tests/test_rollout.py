"""The closed-loop rollout: plant map and eicos_batch_rollout (eicos_batch_set_plant_map / _has_plant_map / _rollout /
_last_rollout_launches and their eicos_multi_* forms, include/eicos_amd.h).

A handle holds a third map beside the parameter and the output map: theta+ = f0 + F [theta | u] (+ w).  rollout(theta0, steps, w) takes
every instance through `steps` closed-loop steps in one call -- with an LDS vector on the handle in ONE launch of the solve kernel, whose
workgroups run the steps of their instances themselves.  The contract is bit-identity: the rollout leaves exactly the state and the arrays
of a twin handle driven by `steps` calls of update_param_solve whose theta rows a host loop advances with PlantMap.evaluate -- on every
build of the solve kernel, fused or not, whatever memory the arrays live in.  Every comparison is np.array_equal: the feature adds no
arithmetic freedom.  Bit-identity does not need optimal exits, and none is asserted.  The CPU tests check PlantMap.evaluate and the
refusals that need no GPU."""
import ctypes as C

import numpy as np
import pytest

import eicos_amd
from eicos_amd import binding
from eicos_amd.binding import PlantMap
import test_param_update as P  # (its _data, _map, _theta, _twins)
import test_rhs_update as R    # (its _outputs, _assert_same and device-array helpers)
from test_param_step import _omap

KEYS = R.KEYS
DP = C.POINTER(C.c_double)
IP = C.POINTER(C.c_int)


def _fmap(k, r, seed=0):
    """The plant map of a case: k rows over the k + r columns of z = [theta | u] with 0-4 entries per row in shuffled (unsorted) order --
    and row 0 over 8 entries that include columns 0, k - 1, k and k + r - 1 and column k twice, one empty row (the last, from two rows
    on), and, from three rows on, a short row that repeats a column.  Entries on theta are a few tenths and entries on u a few
    hundredths, so that a handful of steps keeps theta at the size it started with."""
    rng = np.random.default_rng(4000 + seed)
    kr = k + r
    rows = [rng.permutation(kr)[:rng.integers(0, min(4, kr) + 1)] for _ in range(k)]
    rows[0] = rng.permutation(np.concatenate(([0, k - 1, k, kr - 1], rng.integers(0, kr, 3), [k])))
    if k >= 2:
        rows[k - 1] = np.zeros(0, np.int64)
    if k >= 3:
        c = int(rng.integers(0, kr))
        rows[1] = np.array([c, (c + 1) % kr, c])
    rowptr = np.concatenate(([0], np.cumsum([len(v) for v in rows]))).astype(np.int32)
    col = np.concatenate(rows).astype(np.int32)
    val = np.where(col < k, rng.uniform(-0.2, 0.2, col.size), rng.uniform(-0.01, 0.01, col.size))
    return PlantMap(k, r, (rng.uniform(0, 0.5, k), rowptr, col, val))


def _w(B, T, k, seed=0):
    return np.random.default_rng(5000 + seed).uniform(-0.05, 0.05, (B, T, k))


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_rollout_entry_points_refuse_a_null_handle():
    L = binding._lib()
    dp = np.zeros(4).ctypes.data_as(DP)
    err = L.eicos_last_error
    for rc in (L.eicos_batch_set_plant_map(None, None), L.eicos_batch_has_plant_map(None),
               L.eicos_batch_rollout(None, 1, dp, None, dp, None, None, None), L.eicos_batch_last_rollout_launches(None)):
        assert rc == -1 and b"NULL handle" in err()
    err = L.eicos_multi_last_error
    for rc in (L.eicos_multi_set_plant_map(None, None), L.eicos_multi_has_plant_map(None),
               L.eicos_multi_rollout(None, 1, dp, None, dp, None, None, None)):
        assert rc == -1 and b"NULL handle" in err()


def test_plant_map_evaluate_equals_a_scalar_loop_in_the_stated_order():
    # acc = base[j]; for s in stored order: acc = acc + (val[s] * z[col[s]]); then acc = acc + w[j] -- on Python floats (IEEE doubles,
    # no fused multiply-add), z = [theta | u]
    k, r = 4, 2
    base = np.array([0.1, -2.5, 3.0, 1e-3])
    rowptr = np.array([0, 4, 4, 5, 9], np.int32)
    col = np.array([5, 0, 3, 4, 1, 4, 2, 4, 1], np.int32)  # (row 1 is empty; rows 0 and 3 are not sorted; row 3 holds column 4 twice)
    val = np.array([1 / 3, 1e-7, -0.7, 0.9, 2 / 7, 1e10, 0.3, -1e10, 1 / 7])  # (the two entries of row 3 on column 4 cancel)
    assert {0, k - 1, k, k + r - 1} <= set(col.tolist())
    theta = np.array([[0.1, 0.7, 1 / 9, 0.3], [0.9, 0.7, 0.123456789, -0.2]])
    u = np.array([[1 / 3, -0.6], [2.5, 1 / 11]])
    w = np.array([[1e-3, 1 / 7, -0.5, 1e-9], [0.25, -1 / 3, 0.0, 3.0]])
    fm = PlantMap(k, r, (base, rowptr, col, val))
    z = np.concatenate((theta, u), axis=1)
    for dist in (None, w):
        got = fm.evaluate(theta, u, dist)
        assert got.shape == (2, k)
        for i in range(2):
            for j in range(k):
                acc = float(base[j])
                for s in range(rowptr[j], rowptr[j + 1]):
                    acc = acc + (float(val[s]) * float(z[i, col[s]]))
                if dist is not None:
                    acc = acc + float(dist[i, j])
                assert got[i, j] == acc, (i, j, dist is not None)


def test_plant_map_evaluate_matches_a_dense_product():
    rng = np.random.default_rng(7)
    B = 5
    for k, r in ((1, 3), (5, 2), (16, 4)):
        fm = _fmap(k, r, seed=k)
        theta, u, w = rng.standard_normal((B, k)), rng.standard_normal((B, r)), rng.standard_normal((B, k))
        F = np.zeros((k, k + r))
        for row in range(k):
            np.add.at(F[row], fm.col[fm.rowptr[row]:fm.rowptr[row + 1]], fm.val[fm.rowptr[row]:fm.rowptr[row + 1]])  # (repeated columns add up)
        want = fm.base[None, :] + np.concatenate((theta, u), axis=1) @ F.T
        assert np.max(np.abs(fm.evaluate(theta, u) - want)) <= 1e-13 * np.max(np.abs(want))
        assert np.max(np.abs(fm.evaluate(theta, u, w) - (want + w))) <= 1e-13 * np.max(np.abs(want + w))
        # the shape of the test maps themselves: columns 0, k - 1, k, k + r - 1 and a repeated column in row 0, an empty last row
        first = fm.col[:fm.rowptr[1]]
        assert {0, k - 1, k, k + r - 1} <= set(first.tolist()) and len(set(first.tolist())) < first.size
        assert k < 2 or fm.rowptr[-1] == fm.rowptr[-2]


def test_rollout_arrays_of_the_wrong_shape_are_refused_before_the_library_is_called():
    B, T, k, r = 3, 2, 4, 2
    fm = _fmap(k, r)
    keep, ptr = binding._plant_map_ptr(fm, k, r)
    assert ptr is not None
    for bad in (np.zeros((B, k + 1)), np.zeros((B + 1, k)), np.zeros(B * k)):
        with pytest.raises(ValueError):
            binding._theta_rows(bad, k, B)  # theta0 not [B][k]
    assert binding._disturbance(None, B, T, k) is None and binding._disturbance(np.zeros((B, T, k)), B, T, k).shape == (B, T, k)
    for bad in (np.zeros((B, T, k + 1)), np.zeros((B, T + 1, k)), np.zeros((B + 1, T, k)), np.zeros((B, T * k)), np.zeros((T, B, k))):
        with pytest.raises(ValueError):
            binding._disturbance(bad, B, T, k)  # w not [B][T][k]
    with pytest.raises(ValueError):
        fm.evaluate(np.zeros((B, k + 1)), np.zeros((B, r)))
    with pytest.raises(ValueError):
        fm.evaluate(np.zeros((B, k)), np.zeros((B, r + 1)))
    with pytest.raises(ValueError):
        fm.evaluate(np.zeros((B, k)), np.zeros((B, r)), np.zeros((B + 1, k)))
    with pytest.raises(ValueError):  # a base of the wrong length
        binding._plant_map_ptr(PlantMap(k, r, (np.zeros(k + 1), fm.rowptr, fm.col, fm.val)), k, r)
    with pytest.raises(ValueError):  # row pointers that run past the stored entries
        binding._plant_map_ptr(PlantMap(2, r, (np.zeros(2), np.array([0, 2, 5], np.int32), np.zeros(3, np.int32), np.zeros(3))), 2, r)
    with pytest.raises(ValueError):  # a map made for another k ...
        binding._plant_map_ptr(_fmap(k + 1, r), k, r)
    with pytest.raises(ValueError):  # ... or another r
        binding._plant_map_ptr(_fmap(k, r + 1), k, r)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def _host_loop(ref, fm, theta0, T, w):
    """The reference: T calls of update_param_solve on pinned theta and u, the theta rows advanced on the host by PlantMap.evaluate.
    Returns u_traj, theta_traj, exitcodes, iters in the layout of rollout()."""
    B, k = theta0.shape
    pth, pu = eicos_amd.PinnedArray((B, k)), eicos_amd.PinnedArray((B, fm.r))
    th, thetas, us, codes, iters = theta0.copy(), [theta0.copy()], [], [], []
    for t in range(T):
        pth.a[...] = th
        pu.a[...] = np.nan
        codes.append(np.asarray(ref.update_param_solve(pth.a, u_out=pu.a)).copy())
        iters.append(ref.info_arrays()["iter"].copy())
        us.append(pu.a.copy())
        th = fm.evaluate(th, us[-1], None if w is None else w[:, t])
        thetas.append(th)
    pth.close(); pu.close()
    return np.stack(us, axis=1), np.stack(thetas, axis=1), np.stack(codes, axis=1), np.stack(iters, axis=1)


def _assert_rollout(got, want, what):
    for q, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), (what, ("u", "theta", "exitcodes", "iters")[q])


def _final_codes(g):
    return g.info_arrays()["exitcode"]


def _compare_rollout(name, B, k, r, T, with_w, make=None, build=None, prepare=None, launches=None, full_rows=0):
    """Twin handles after update(...); solve(): one takes rollout(), the other the host loop; per step u, the next theta, the exit codes
    and the iteration counts, and after the last step every output and the KKT values of the last instance, must be equal bit for bit."""
    pat, d = P._data(name, B)
    pm, om, fm = P._map(d, k, full_rows=full_rows), _omap(pat.n, r), _fmap(k, r)
    g, ref = P._twins(pat, d, B, make)
    assert g.dims() == ref.dims() and g.kernel_build() == ref.kernel_build()
    if build is not None:
        assert (g.kernel_build(), g.dims()["threads_per_block"]) == build, (g.kernel_build(), g.dims()["threads_per_block"])
    for s in (g, ref):
        if prepare:
            prepare(s)
        s.set_param_map(pm); s.set_output_map(om)
    assert not g.has_plant_map()
    g.set_plant_map(fm)
    assert g.has_plant_map()
    theta0, w = P._theta(B, k), (_w(B, T, k) if with_w else None)
    want = _host_loop(ref, fm, theta0, T, w)
    got = g.rollout(theta0, T, w)
    what = (name, B, k, r, T, with_w)
    if launches is None and g.dims()["lds_bytes"] > 0:
        launches = 1
    if launches is not None:
        assert g.last_rollout_launches() == launches, (what, g.last_rollout_launches())
    _assert_rollout(got, want, what)
    R._assert_same(R._outputs(g, _final_codes(g)), R._outputs(ref, _final_codes(ref)), what)
    assert np.array_equal(got[2][:, -1], _final_codes(g)), what
    assert np.array_equal(g.debug_kkt(B - 1)[2], ref.debug_kkt(B - 1)[2], equal_nan=True), what
    g.close(); ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case,name,B,k,r,T", [
    (0, "MPC02", 40, 7, 6, 3),
    (1, "MPC02", 600, 16, 4, 2),      # more instances than resident workgroups: the queue pulls whole trajectories
    (2, "lp_afiro", 16, 1, 3, 3),     # the LDS-resident build where the handle reports it; one parameter
    (3, "issue98", 8, 5, 2, 3),       # cones
    (4, "socp-random", 8, 5, 5, 3),   # cones and equality rows: b is mapped
    (5, "dense-front", 6, 3, 4, 3),   # the tile path
])
def test_rollout_is_bit_identical_to_the_host_loop_over_param_steps(case, name, B, k, r, T):
    _compare_rollout(name, B, k, r, T, with_w=case % 2 == 1)


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
def test_rollout_on_every_build_of_the_solve_kernel(name, B, env, build, monkeypatch):
    # the seven compilations of k_solve all carry the loop over the steps and the plant map: steer a pattern through each
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    _compare_rollout(name, B, 5, 4, 2, with_w=True, build=build, launches=1)


@pytest.mark.gpu
def test_rollout_with_warm_start_chains_the_steps():
    # step t + 1 starts from the solution step t left in the instance slab: the case in which a step depends on the state before it
    def warm(s):
        assert (np.asarray(s.info_arrays()["exitcode"]) == 0).all()  # (the twins' first solve is optimal)
        s.set_warm_start(0.1)

    _compare_rollout("MPC02", 40, 7, 6, 3, with_w=True, prepare=warm, launches=1)


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,k,env", [
    ("MPC02", 40, 7, {"EICOS_FUSED_UPDATE": "0"}),
    ("MPC02", 40, 7, {"EICOS_NLDS": "0", "EICOS_DUAL": "0"}),  # a handle without an LDS vector
    ("lp_afiro", 5, 1100, {}),                                   # a theta row that does not fit the LDS vector
])
def test_rollout_without_the_fused_path_gives_the_same_bits(name, B, k, env, monkeypatch):
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    T = 3
    _compare_rollout(name, B, k, 4, T, with_w=True, launches=T, full_rows=2)


@pytest.mark.gpu
def test_rollout_over_every_kind_of_memory():
    B, k, r, T = 40, 7, 6, 2
    pat, d = P._data("MPC02", B)
    pm, om, fm = P._map(d, k), _omap(pat.n, r), _fmap(k, r)
    g, ref = P._twins(pat, d, B)
    for s in (g, ref):
        s.set_param_map(pm); s.set_output_map(om)
    g.set_plant_map(fm)
    L = binding._lib()
    shapes = ((B, k), (B, T, k), (B, T, r), (B, T + 1, k))
    theta_last = [P._theta(B, k, seed=50)]

    def reference(seed):
        w = _w(B, T, k, seed=seed)
        theta0 = theta_last[0]
        want = _host_loop(ref, fm, theta0, T, w)
        theta_last[0] = want[1][:, -1].copy()
        return theta0, w, want

    def call(ptrs):
        codes, iters = np.full((B, T), 99, np.int32), np.full((B, T), 99, np.int32)
        assert L.eicos_batch_rollout(g._h, T, *[C.cast(p, DP) for p in ptrs], codes.ctypes.data_as(IP), iters.ctypes.data_as(IP)) == 0, L.eicos_last_error()
        assert g.last_rollout_launches() == 1
        return codes, iters

    def check(u, th, codes, iters, want, what):
        _assert_rollout((u, th, codes, iters), want, what)
        R._assert_same(R._outputs(g, _final_codes(g)), R._outputs(ref, _final_codes(ref)), what)

    # pinned arrays
    theta0, w, want = reference(1)
    pins = [eicos_amd.PinnedArray(s) for s in shapes]
    pins[0].a[...] = theta0; pins[1].a[...] = w; pins[2].a[...] = np.nan; pins[3].a[...] = np.nan
    codes, iters = call([p_.a.ctypes.data for p_ in pins])
    check(pins[2].a, pins[3].a, codes, iters, want, "pinned")
    for p_ in pins:
        p_.close()
    # registered caller-owned arrays
    theta0, w, want = reference(2)
    own = [theta0.copy(), w.copy(), np.full(shapes[2], np.nan), np.full(shapes[3], np.nan)]
    for a in own:
        eicos_amd.host_register(a)
    try:
        codes, iters = call([a.ctypes.data for a in own])
        check(own[2], own[3], codes, iters, want, "registered")
    finally:
        for a in own:
            eicos_amd.host_unregister(a)
    # device arrays, read back with hipMemcpy
    theta0, w, want = reference(3)
    dev = R._device_arrays((theta0, w, np.full(shapes[2], np.nan), np.full(shapes[3], np.nan)))
    try:
        codes, iters = call(dev)
        u, th = np.zeros(shapes[2]), np.zeros(shapes[3])
        assert L.hipMemcpy(u.ctypes.data, dev[2], u.nbytes, 2) == 0 and L.hipMemcpy(th.ctypes.data, dev[3], th.nbytes, 2) == 0  # hipMemcpyDeviceToHost
        check(u, th, codes, iters, want, "device")
    finally:
        R._free_device(dev)
    # pageable arrays
    theta0, w, want = reference(4)
    u, th, codes, iters = g.rollout(theta0, T, w)
    assert g.last_rollout_launches() == 1
    check(u, th, codes, iters, want, "pageable")
    g.close(); ref.close()


@pytest.mark.gpu
def test_two_rollouts_chain_into_one():
    # two rollouts of two steps, the second started from the last theta row of the first, equal one rollout of four steps
    B, k, r = 40, 7, 6
    pat, d = P._data("MPC02", B)
    pm, om, fm = P._map(d, k), _omap(pat.n, r), _fmap(k, r)
    g, ref = P._twins(pat, d, B)
    for s in (g, ref):
        s.set_param_map(pm); s.set_output_map(om); s.set_plant_map(fm)
    theta0, w = P._theta(B, k), _w(B, 4, k)
    whole = ref.rollout(theta0, 4, w)
    a = g.rollout(theta0, 2, w[:, :2])
    b = g.rollout(a[1][:, -1], 2, w[:, 2:])
    assert np.array_equal(a[1][:, -1], b[1][:, 0])
    joined = (np.concatenate((a[0], b[0]), axis=1), np.concatenate((a[1], b[1][:, 1:]), axis=1),
              np.concatenate((a[2], b[2]), axis=1), np.concatenate((a[3], b[3]), axis=1))
    _assert_rollout(joined, whole, "2 + 2 against 4")
    R._assert_same(R._outputs(g, _final_codes(g)), R._outputs(ref, _final_codes(ref)), "2 + 2 against 4")
    g.close(); ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("devs", [[0, 0], [0, 0, 0]])
def test_multi_rollout_matches_one_handle(devs):
    # ragged shards (5 instances over 2 and 3 shards), arithmetic profile 1 (plans independent of the shard size): the arrays in global
    # instance order give the bits of one handle driven by the host loop
    B, k, r, T = 5, 7, 6, 3
    pat, d = P._data("MPC02", B)
    pm, om, fm = P._map(d, k), _omap(pat.n, r), _fmap(k, r)
    eicos_amd.set_arithmetic_profile(1)
    try:
        one = eicos_amd.BatchSolver(pat, B)
        one.update(*[d[k_] for k_ in KEYS]); one.solve()
        one.set_param_map(pm); one.set_output_map(om)
        m = eicos_amd.MultiBatchSolver(pat, B, devs)
        m.update(*[d[k_] for k_ in KEYS]); m.solve()
        m.set_param_map(pm); m.set_output_map(om)
        assert not m.has_plant_map()
        m.set_plant_map(fm)
        assert m.has_plant_map()
        theta0, w = P._theta(B, k), _w(B, T, k)
        want = _host_loop(one, fm, theta0, T, w)
        _assert_rollout(m.rollout(theta0, T, w), want, devs)
        y, z, s = m.duals(); ia = m.info_arrays()
        R._assert_same([ia["exitcode"], m.solution(), y, z, s] + [ia[k_] for k_ in R.INFO_KEYS], R._outputs(one, _final_codes(one)), devs)
        m.close(); one.close()
    finally:
        eicos_amd.set_arithmetic_profile(0)


@pytest.mark.gpu
def test_rollout_refusals():
    B, k, r, T = 4, 3, 4, 2
    pat, d = P._data("lp_afiro", B)
    g = eicos_amd.BatchSolver(pat, B)
    g.update(*[d[k_] for k_ in KEYS]); g.solve()
    L = binding._lib()
    err = L.eicos_last_error
    pm, om, fm = P._map(d, k), _omap(pat.n, r), _fmap(k, r)
    theta0, u = P._theta(B, k), np.zeros((B, T, r))

    def install(f):
        m_ = binding.AffineMap(binding._dp(f.base), binding._ip(f.rowptr), binding._ip(f.col), binding._dp(f.val))
        return L.eicos_batch_set_plant_map(g._h, C.pointer(m_))

    def roll(steps=T, th=theta0, out=u):
        return L.eicos_batch_rollout(g._h, steps, None if th is None else th.ctypes.data_as(DP), None,
                                     None if out is None else out.ctypes.data_as(DP), None, None, None)

    # a plant map needs the two maps it refers to
    assert install(fm) == -1 and b"no parameter map" in err()
    g.set_param_map(pm)
    assert install(fm) == -1 and b"no output map" in err()
    assert roll() == -1 and b"no output map" in err()
    g.set_output_map(om)
    assert roll() == -1 and b"no plant map" in err()
    with pytest.raises(RuntimeError, match="no plant map"):
        g.rollout(theta0, T)
    # faults of the map itself
    bad = PlantMap(k, r, (fm.base, fm.rowptr.copy(), fm.col, fm.val)); bad.rowptr[0] = 1
    assert install(bad) == -1 and b"rowptr[0]" in err()
    bad = PlantMap(k, r, (fm.base, fm.rowptr.copy(), fm.col, fm.val)); bad.rowptr[2] = bad.rowptr[1] - 1
    assert install(bad) == -1 and b"rowptr decreases" in err()
    bad = PlantMap(k, r, (fm.base, fm.rowptr, fm.col.copy(), fm.val)); bad.col[-1] = k + r  # a column equal to k + r
    assert install(bad) == -1 and b"outside [0, k + r)" in err()
    bad = PlantMap(k, r, (fm.base, fm.rowptr, fm.col.copy(), fm.val)); bad.col[0] = -1
    assert install(bad) == -1 and b"outside [0, k + r)" in err()
    assert not g.has_plant_map()  # (a refused map installs nothing)
    g.set_plant_map(fm)
    assert g.has_plant_map()
    # faults of the call
    assert roll(steps=0) == -1 and b"steps" in err()
    assert roll(out=None) == -1 and b"u_traj is NULL" in err()
    assert roll(th=None) == -1 and b"theta0 is NULL" in err()
    with pytest.raises(ValueError):
        g.rollout(np.zeros((B, k + 1)), T)
    with pytest.raises(ValueError):
        g.rollout(theta0, T, w=np.zeros((B, T + 1, k)))
    assert roll() == 0
    # each missing map, on a handle that had all three
    g.set_param_map(None)
    assert roll() == -1 and b"no parameter map" in err()
    g.set_param_map(pm)
    assert roll() == 0
    # a plant map made stale by an output map with another r: refused, naming both pairs, until it is installed again
    g.set_output_map(_omap(pat.n, r + 1))
    assert roll(out=np.zeros((B, T, r + 1))) == -1 and b"(3, 4)" in err() and b"(3, 5)" in err()
    with pytest.raises(ValueError):
        g.set_plant_map(fm)
    g.set_plant_map(_fmap(k, r + 1))
    assert roll(out=np.zeros((B, T, r + 1))) == 0
    g.set_plant_map(None)
    assert not g.has_plant_map() and roll(out=np.zeros((B, T, r + 1))) == -1 and b"no plant map" in err()
    g.close()
