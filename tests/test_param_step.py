"""The closed-loop step: output map and eicos_batch_update_param_solve (eicos_batch_set_output_map / _output_count / _outputs /
_outputs_device / _update_param_solve and their eicos_multi_* forms, include/eicos_amd.h).

A handle holds one output map u = u0 + U x (CSR with n columns, r rows); update_param_solve(theta, u_out, x_out) is update_param + solve +
outputs in one call, and with theta the GPU addresses directly every workgroup of the solve kernel expands its instance's theta row and
writes that instance's u row (and x row) itself.  The contract is bit-identity: the step leaves exactly the state of a twin handle driven
by update_param(theta); solve(), and u equals OutputMap.evaluate(solution()) -- on every build of the solve kernel and every transfer
path.  Every comparison is np.array_equal: the feature adds no arithmetic freedom.  Bit-identity does not need optimal exits, and none
is asserted.  The CPU tests check OutputMap.evaluate and the refusals that need no GPU."""
import ctypes as C

import numpy as np
import pytest

import eicos_amd
from eicos_amd import binding
from eicos_amd.binding import OutputMap
import test_param_update as P  # (its _data, _map, _theta, _twins)
import test_rhs_update as R    # (its _outputs, _assert_same and device-array helpers)

KEYS = R.KEYS
DP = C.POINTER(C.c_double)
IP = C.POINTER(C.c_int)


def _omap(n, r, seed=0):
    """The output map of a case: r rows over n variables with 0-4 entries per row, in shuffled (unsorted) column order -- and row 0
    over at least 8 entries that include columns 0 and n - 1 and one column twice, one empty row (the last), and, from three rows
    on, a short row that repeats a column."""
    rng = np.random.default_rng(3000 + seed)
    rows = []
    for j in range(r):
        rows.append(rng.permutation(n)[:rng.integers(0, min(4, n) + 1)])
    mid = rng.permutation(np.arange(1, max(n - 1, 1)))[:7] if n > 2 else np.zeros(0, np.int64)
    long = np.concatenate(([0, n - 1], mid, [0]))
    while long.size < 8:  # (a pattern with fewer than 8 variables: columns repeat)
        long = np.concatenate((long, long))[:8]
    rows[0] = rng.permutation(long)
    if r >= 2:
        rows[r - 1] = np.zeros(0, np.int64)
    if r >= 3:
        c = int(rng.integers(0, n))
        rows[1] = np.array([c, (c + 1) % n, c])
    rowptr = np.concatenate(([0], np.cumsum([len(v) for v in rows]))).astype(np.int32)
    col = np.concatenate(rows).astype(np.int32)
    return OutputMap(n, (rng.uniform(-1, 1, r), rowptr, col, rng.uniform(-2, 2, col.size)))


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_step_entry_points_refuse_a_null_handle():
    L = binding._lib()
    dp = np.zeros(4).ctypes.data_as(DP)
    err = L.eicos_last_error
    for rc in (L.eicos_batch_set_output_map(None, 1, None), L.eicos_batch_output_count(None), L.eicos_batch_outputs(None, 0, 1, dp),
               L.eicos_batch_outputs_device(None, 0, 1, None), L.eicos_batch_update_param_solve(None, dp, dp, None, None)):
        assert rc == -1 and b"NULL handle" in err()
    err = L.eicos_multi_last_error
    for rc in (L.eicos_multi_set_output_map(None, 1, None), L.eicos_multi_output_count(None), L.eicos_multi_outputs(None, 0, 1, dp),
               L.eicos_multi_update_param_solve(None, dp, dp, None, None)):
        assert rc == -1 and b"NULL handle" in err()


def test_output_map_evaluate_equals_a_scalar_loop_in_the_stated_order():
    # acc = base[row]; for t in stored order: acc = acc + (val[t] * x[col[t]]) on Python floats (IEEE doubles, no fused multiply-add)
    base = np.array([0.1, -2.5, 3.0, 1e-3])
    rowptr = np.array([0, 3, 3, 4, 7], np.int32)
    col = np.array([2, 0, 1, 1, 0, 2, 1], np.int32)  # (row 1 is empty; row 3 is not sorted)
    val = np.array([1 / 3, 1e-7, -0.7, 2 / 7, 0.3, 1e10, -1e10])  # (row 3 ends with a cancelling pair)
    x = np.array([[0.1, 0.7, 1 / 9], [0.9, 0.7, 0.123456789]])
    om = OutputMap(3, (base, rowptr, col, val))
    got = om.evaluate(x)
    assert om.r == 4 and got.shape == (2, 4)
    for i in range(2):
        for r in range(4):
            acc = float(base[r])
            for t in range(rowptr[r], rowptr[r + 1]):
                acc = acc + (float(val[t]) * float(x[i, col[t]]))
            assert got[i, r] == acc, (i, r)


def test_output_map_evaluate_matches_a_dense_product():
    rng = np.random.default_rng(6)
    n, B = 37, 5
    for r in (2, 3, 6):
        om = _omap(n, r, seed=r)
        x = rng.standard_normal((B, n))
        U = np.zeros((r, n))
        for row in range(r):
            np.add.at(U[row], om.col[om.rowptr[row]:om.rowptr[row + 1]], om.val[om.rowptr[row]:om.rowptr[row + 1]])  # (repeated columns add up)
        want = om.base[None, :] + x @ U.T
        assert np.max(np.abs(om.evaluate(x) - want)) <= 1e-13 * np.max(np.abs(want))
        # the shape of the test maps themselves: an empty row, columns 0 and n - 1, a row over >= 8 entries, a repeated column
        length = np.diff(om.rowptr)
        assert length[-1] == 0 and length[0] >= 8 and {0, n - 1} <= set(om.col[:length[0]]) and len(set(om.col[:length[0]])) < length[0]


def test_step_arrays_of_the_wrong_shape_are_refused_before_the_library_is_called():
    pat, _ = R.load_fixture("lp_afiro")
    B, r = 3, 4
    om = _omap(pat.n, r)
    keep, ptr = binding._output_map_ptr(om, pat)
    assert ptr is not None
    assert binding._result_rows(np.zeros((B, r)), B, r, "u_out") is not None and binding._result_rows(None, B, r, "u_out") is None
    for bad in (np.zeros((B, r + 1)), np.zeros((B + 1, r)), np.zeros(B * r), np.zeros((B, r), np.float32), np.zeros((r, B)).T):
        with pytest.raises(ValueError):
            binding._result_rows(bad, B, r, "u_out")  # u_out not [B][r]
    with pytest.raises(ValueError):
        binding._result_rows(np.zeros((B, pat.n + 1)), B, pat.n, "x_out")  # x_out not [B][n]
    with pytest.raises(ValueError):
        om.evaluate(np.zeros((B, pat.n + 1)))  # x not [B][n]
    with pytest.raises(ValueError):
        om.evaluate(np.zeros(pat.n))
    with pytest.raises(ValueError):  # a base of the wrong length
        binding._output_map_ptr(OutputMap(pat.n, (np.zeros(r + 1), om.rowptr, om.col, om.val)), pat)
    with pytest.raises(ValueError):  # row pointers that run past the stored entries
        binding._output_map_ptr(OutputMap(pat.n, (np.zeros(2), np.array([0, 2, 5], np.int32), np.zeros(3, np.int32), np.zeros(3))), pat)
    with pytest.raises(ValueError):  # a map made for another number of variables
        binding._output_map_ptr(_omap(pat.n + 1, r), pat)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def _pinned(*shapes):
    return [eicos_amd.PinnedArray(s) for s in shapes]


def _compare_steps(name, B, k, r, steps=2, make=None, build=None, prepare=None):
    """Twin handles after update(...); solve().  `steps` consecutive theta: one twin takes update_param + solve, the other the one-call
    step with pinned theta, u_out and x_out; every output, u and the KKT values of the last instance must be equal bit for bit."""
    pat, d = P._data(name, B)
    pm, om = P._map(d, k), _omap(pat.n, r)
    g, ref = P._twins(pat, d, B, make)
    assert g.dims() == ref.dims() and g.kernel_build() == ref.kernel_build()
    if build is not None:
        assert (g.kernel_build(), g.dims()["threads_per_block"]) == build, (g.kernel_build(), g.dims()["threads_per_block"])
    for s in (g, ref):
        if prepare:
            prepare(s)
        s.set_param_map(pm)
    assert g.output_count() == 0
    g.set_output_map(om)
    assert g.output_count() == r
    pth, pu, px = _pinned((B, k), (B, r), (B, pat.n))
    rows, cols, _ = g.debug_kkt(B - 1)
    ag = (rows < pat.n) & (cols >= pat.n)  # the equilibrated A', G' entries of the KKT matrix (the scaling block is solve state)
    for step in range(steps):
        what = (name, "step", step)
        pth.a[...] = P._theta(B, k, seed=step)
        ref.update_param(pth.a.copy())
        out_ref = R._outputs(ref, ref.solve())
        kkt0 = g.debug_kkt(B - 1)[2].copy()
        pu.a[...] = np.nan; px.a[...] = np.nan
        codes = g.update_param_solve(pth.a, u_out=pu.a, x_out=px.a)
        if g.dims()["lds_bytes"] > 0:
            assert g.last_update_path() == "fused into the solve", what
        R._assert_same(R._outputs(g, codes), out_ref, what)
        assert np.array_equal(pu.a, om.evaluate(out_ref[1])), what
        assert np.array_equal(px.a, g.solution()), what
        kkt1 = g.debug_kkt(B - 1)[2]
        assert np.array_equal(kkt1[ag], kkt0[ag]), what                      # the update part leaves A, G alone ...
        assert np.array_equal(kkt1, ref.debug_kkt(B - 1)[2], equal_nan=True), what  # ... and the whole matrix equals the twin's
    g.close(); ref.close()
    for p_ in (pth, pu, px):
        p_.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,k,r", [
    ("MPC02", 40, 7, 6),
    ("MPC02", 600, 16, 4),       # more instances than resident workgroups: queue pulls, the longest-first order from the second step on
    ("lp_afiro", 16, 1, 3),      # the LDS-resident build where the handle reports it
    ("issue98", 8, 5, 2),        # cones
    ("socp-random", 8, 5, 5),    # cones and equality rows: b is mapped
    ("dense-front", 6, 3, 4),    # the tile path
])
def test_fused_param_step_is_bit_identical_to_update_param_then_solve(name, B, k, r):
    _compare_steps(name, B, k, r)


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
def test_fused_param_step_on_every_build_of_the_solve_kernel(name, B, env, build, monkeypatch):
    # the seven compilations of k_solve all carry the parametric update and the output rows: steer a pattern through each
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    _compare_steps(name, B, 5, 4, build=build)


@pytest.mark.gpu
def test_param_step_over_every_transfer_path(monkeypatch):
    B, k, r = 40, 7, 6
    pat, d = P._data("MPC02", B)
    pm, om = P._map(d, k), _omap(pat.n, r)
    g, ref = P._twins(pat, d, B)
    for s in (g, ref):
        s.set_param_map(pm)
    g.set_output_map(om)
    L = binding._lib()
    pth, pu, px = _pinned((B, k), (B, r), (B, pat.n))
    seed = [100]

    def reference():
        seed[0] += 1
        theta = P._theta(B, k, seed=seed[0])
        ref.update_param(theta)
        out = R._outputs(ref, ref.solve())
        return theta, out, om.evaluate(out[1])

    def check(codes, u, x, out_ref, u_ref, fused, what):
        if fused is not None:
            assert (g.last_update_path() == "fused into the solve") == fused, (what, g.last_update_path())
        R._assert_same(R._outputs(g, codes), out_ref, what)
        assert np.array_equal(u, u_ref), what
        if x is not None:
            assert np.array_equal(x, out_ref[1]), what

    # registered caller-owned theta, pageable u_out: fused, u by the range kernel and a copy
    theta, out_ref, u_ref = reference()
    own = theta.copy()
    eicos_amd.host_register(own)
    try:
        u = np.full((B, r), np.nan)
        check(g.update_param_solve(own, u_out=u), u, None, out_ref, u_ref, True, "registered theta, pageable u_out")
    finally:
        eicos_amd.host_unregister(own)
    # device theta, device u_out and x_out: fused, read back with hipMemcpy
    theta, out_ref, u_ref = reference()
    dev = R._device_arrays((theta, np.full((B, r), np.nan), np.full((B, pat.n), np.nan)))
    try:
        codes = np.zeros(B, np.int32)
        assert L.eicos_batch_update_param_solve(g._h, C.cast(dev[0], DP), C.cast(dev[1], DP), C.cast(dev[2], DP), codes.ctypes.data_as(IP)) == 0
        u, x = np.zeros((B, r)), np.zeros((B, pat.n))
        assert L.hipMemcpy(u.ctypes.data, dev[1], u.nbytes, 2) == 0 and L.hipMemcpy(x.ctypes.data, dev[2], x.nbytes, 2) == 0  # hipMemcpyDeviceToHost
        check(codes, u, x, out_ref, u_ref, True, "device")
        # the same without the fused path: the device-pointer update, device results filled by the range kernel / a copy on the device
        monkeypatch.setenv("EICOS_FUSED_UPDATE", "0")
        theta, out_ref, u_ref = reference()
        assert L.hipMemcpy(dev[0], theta.ctypes.data, theta.nbytes, 1) == 0  # hipMemcpyHostToDevice
        assert L.eicos_batch_update_param_solve(g._h, C.cast(dev[0], DP), C.cast(dev[1], DP), C.cast(dev[2], DP), codes.ctypes.data_as(IP)) == 0
        assert L.hipMemcpy(u.ctypes.data, dev[1], u.nbytes, 2) == 0 and L.hipMemcpy(x.ctypes.data, dev[2], x.nbytes, 2) == 0
        check(codes, u, x, out_ref, u_ref, None, "device, not fused")  # (the device-pointer update leaves no path behind)
        monkeypatch.delenv("EICOS_FUSED_UPDATE")
    finally:
        R._free_device(dev)
    # pageable theta: update_param through the bounce pipeline, solve, outputs
    theta, out_ref, u_ref = reference()
    check(g.update_param_solve(theta, u_out=pu.a, x_out=px.a), pu.a, px.a, out_ref, u_ref, False, "pageable theta")
    assert g.last_update_path() == "pinned bounce"
    # pinned theta with the fused path switched off
    monkeypatch.setenv("EICOS_FUSED_UPDATE", "0")
    pth.a[...], out_ref, u_ref = reference()
    check(g.update_param_solve(pth.a, u_out=pu.a, x_out=px.a), pu.a, px.a, out_ref, u_ref, False, "EICOS_FUSED_UPDATE=0")
    assert g.last_update_path() == "pinned source in place"
    monkeypatch.delenv("EICOS_FUSED_UPDATE")
    # and switched on again: the same handle takes the fused path
    pth.a[...], out_ref, u_ref = reference()
    check(g.update_param_solve(pth.a, u_out=pu.a, x_out=px.a), pu.a, px.a, out_ref, u_ref, True, "pinned")
    g.close(); ref.close()
    for p_ in (pth, pu, px):
        p_.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,k,env,fused", [
    # a handle without an LDS vector.  EICOS_NLDS=0 alone does not make one at this batch: a launch of at most one workgroup per CU solves
    # its two right-hand sides together and keeps its LDS vector for that (dims()["dual_rhs"]), whatever EICOS_NLDS says -- so the case
    # runs once with the dual solve switched off as well (no LDS vector: not fused) and once as it is (the path follows the handle)
    ("MPC02", 40, 7, {"EICOS_NLDS": "0", "EICOS_DUAL": "0"}, False),
    ("MPC02", 40, 7, {"EICOS_NLDS": "0"}, None),
    ("lp_afiro", 5, 1100, {}, False),  # a theta row that does not fit the LDS vector
])
def test_param_step_without_the_fused_path_gives_the_same_bits(name, B, k, env, fused, monkeypatch):
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    r = 4
    pat, d = P._data(name, B)
    pm, om = P._map(d, k, full_rows=2), _omap(pat.n, r)
    g, ref = P._twins(pat, d, B)
    for s in (g, ref):
        s.set_param_map(pm)
    g.set_output_map(om)
    pth, pu, px = _pinned((B, k), (B, r), (B, pat.n))
    for step in range(2):
        pth.a[...] = P._theta(B, k, seed=step)
        ref.update_param(pth.a.copy())
        out_ref = R._outputs(ref, ref.solve())
        codes = g.update_param_solve(pth.a, u_out=pu.a, x_out=px.a)
        want_fused = bool(g.dims()["dual_rhs"]) if fused is None else fused
        assert g.last_update_path() == ("fused into the solve" if want_fused else "pinned source in place"), (name, env, g.dims()["dual_rhs"])
        R._assert_same(R._outputs(g, codes), out_ref, (name, step))
        assert np.array_equal(pu.a, om.evaluate(out_ref[1])) and np.array_equal(px.a, out_ref[1])
    g.close(); ref.close()
    for p_ in (pth, pu, px):
        p_.close()


@pytest.mark.gpu
def test_outputs_on_their_own():
    B, k = 40, 7
    pat, d = P._data("MPC02", B)
    g = eicos_amd.BatchSolver(pat, B)
    g.update(*[d[k_] for k_ in KEYS]); g.solve()
    L = binding._lib()
    om = _omap(pat.n, 6)
    g.set_output_map(om)
    x = g.solution()
    want = om.evaluate(x)
    assert g.output_count() == 6 and np.array_equal(g.outputs(), want)
    f, n = B // 4, B // 3
    assert np.array_equal(g.outputs(first=f, count=n), want[f:f + n])
    assert g.outputs(first=B, count=0).shape == (0, 6)
    pin = eicos_amd.PinnedArray((B, 6)); pin.a[...] = np.nan
    assert L.eicos_batch_outputs(g._h, 0, B, pin.a.ctypes.data_as(DP)) == 0 and np.array_equal(pin.a, want)
    dev = R._device_arrays((np.full((n, 6), np.nan),))
    try:
        g.outputs_device(dev[0], first=f, count=n); g.sync()
        u = np.zeros((n, 6))
        assert L.hipMemcpy(u.ctypes.data, dev[0], u.nbytes, 2) == 0 and np.array_equal(u, want[f:f + n])  # hipMemcpyDeviceToHost
        # a device pointer handed to the host-pointer entry point is refused, naming the right call
        assert L.eicos_batch_outputs(g._h, f, n, C.cast(dev[0], DP)) == -1 and b"eicos_batch_outputs_device" in L.eicos_last_error()
    finally:
        R._free_device(dev)
    assert L.eicos_batch_outputs(g._h, 2, B - 1, pin.a.ctypes.data_as(DP)) == -1 and b"out of bounds" in L.eicos_last_error()
    assert L.eicos_batch_outputs_device(g._h, -1, 1, None) == -1 and b"out of bounds" in L.eicos_last_error()
    # a later call replaces the map
    om2 = _omap(pat.n, 3, seed=1)
    g.set_output_map(om2)
    want2 = om2.evaluate(x)
    assert g.output_count() == 3 and np.array_equal(g.outputs(), want2) and want2.shape != want.shape
    # without a map: outputs() and a step that asks for u are refused; a step that asks for nothing still solves
    pm = P._map(d, k)
    g.set_param_map(pm)
    ref = eicos_amd.BatchSolver(pat, B)
    ref.update(*[d[k_] for k_ in KEYS]); ref.solve()
    ref.set_param_map(pm)
    theta = P._theta(B, k)
    pth = eicos_amd.PinnedArray((B, k)); pth.a[...] = theta
    for remove in (lambda: g.set_output_map(None), lambda: L.eicos_batch_set_output_map(g._h, 3, None)):
        g.set_output_map(om2)
        remove()
        assert g.output_count() == 0
        with pytest.raises(RuntimeError, match="no output map"):
            g.outputs()
        assert L.eicos_batch_outputs_device(g._h, 0, B, None) == -1 and b"no output map" in L.eicos_last_error()
        assert L.eicos_batch_update_param_solve(g._h, pth.a.ctypes.data_as(DP), pin.a.ctypes.data_as(DP), None, None) == -1
        assert b"no output map" in L.eicos_last_error()
    ref.update_param(theta)
    out_ref = R._outputs(ref, ref.solve())
    codes = g.update_param_solve(pth.a)
    assert g.last_update_path() == "fused into the solve"
    R._assert_same(R._outputs(g, codes), out_ref)
    g.close(); ref.close(); pin.close(); pth.close()


@pytest.mark.gpu
def test_param_step_refusals():
    B = 4
    pat, d = P._data("lp_afiro", B)
    g = eicos_amd.BatchSolver(pat, B)
    L = binding._lib()
    err = L.eicos_last_error
    good = _omap(pat.n, 4)

    def install(r, base, rowptr, col, val):
        one = np.zeros(1)
        m = binding.AffineMap(binding._dp(base), binding._ip(rowptr), binding._ip(col if col.size else np.zeros(1, np.int32)), binding._dp(val if val.size else one))
        return L.eicos_batch_set_output_map(g._h, r, C.pointer(m))

    base, rowptr, col, val = good.base, good.rowptr, good.col, good.val
    bad = rowptr.copy(); bad[0] = 1
    assert install(4, base, bad, col, val) == -1 and b"rowptr[0]" in err()
    bad = rowptr.copy(); bad[2] = bad[1] - 1
    assert install(4, base, bad, col, val) == -1 and b"rowptr decreases" in err()
    bad = col.copy(); bad[-1] = pat.n  # a column equal to n
    assert install(4, base, rowptr, bad, val) == -1 and b"outside [0, n)" in err()
    bad = col.copy(); bad[0] = -1
    assert install(4, base, rowptr, bad, val) == -1 and b"outside [0, n)" in err()
    assert install(-1, base, rowptr, col, val) == -1 and b"must not be negative" in err()
    assert g.output_count() == 0  # (a refused map installs nothing)
    assert install(4, base, rowptr, col, val) == 0 and g.output_count() == 4
    # a step without a parameter map
    theta = np.zeros((B, 3))
    u = np.zeros((B, 4))
    assert L.eicos_batch_update_param_solve(g._h, theta.ctypes.data_as(DP), u.ctypes.data_as(DP), None, None) == -1 and b"no parameter map" in err()
    with pytest.raises(RuntimeError, match="no parameter map"):
        g.update_param_solve(theta, u_out=u)
    g.set_param_map(P._map(d, 3))
    with pytest.raises(ValueError):
        g.update_param_solve(np.zeros((B, 4)), u_out=u)  # theta rows of the wrong width
    with pytest.raises(ValueError):
        g.update_param_solve(theta, u_out=np.zeros((B, 5)))
    with pytest.raises(ValueError):
        g.update_param_solve(theta, x_out=np.zeros((B + 1, pat.n)))
    assert L.eicos_batch_update_param_solve(g._h, None, u.ctypes.data_as(DP), None, None) == -1 and b"theta is NULL" in err()
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,B", [("MPC02", 8), ("issue98", 4)])
def test_param_step_with_warm_start_and_dynamic_regularisation(name, B):
    def both(s):
        s.set_warm_start(0.1)
        s.set_dynamic_regularization(2e-7, 1e-13)

    _compare_steps(name, B, 7, 4, steps=3, prepare=both)


@pytest.mark.gpu
@pytest.mark.parametrize("devs", [[0, 0], [0, 0, 0]])
def test_multi_param_step_matches_one_handle(devs):
    # uneven shards (10 instances over 2 and 3 shards), arithmetic profile 1 (plans independent of the shard size): theta, u_out and x_out
    # in global instance order give the bits of one handle
    B, k, r = 10, 7, 6
    pat, d = P._data("MPC02", B)
    pm, om = P._map(d, k), _omap(pat.n, r)
    eicos_amd.set_arithmetic_profile(1)
    try:
        one = eicos_amd.BatchSolver(pat, B)
        one.update(*[d[k_] for k_ in KEYS]); one.solve()
        one.set_param_map(pm)
        m = eicos_amd.MultiBatchSolver(pat, B, devs)
        m.update(*[d[k_] for k_ in KEYS]); m.solve()
        m.set_param_map(pm); m.set_output_map(om)
        assert m.output_count() == r
        pth, pu, px = _pinned((B, k), (B, r), (B, pat.n))
        for step, pinned in enumerate((True, False)):
            theta = P._theta(B, k, seed=step)
            one.update_param(theta)
            out_ref = R._outputs(one, one.solve())
            u_ref = om.evaluate(out_ref[1])
            if pinned:
                pth.a[...] = theta
                u, x = pu.a, px.a
                codes = m.update_param_solve(pth.a, u_out=u, x_out=x)
            else:
                u, x = np.full((B, r), np.nan), np.full((B, pat.n), np.nan)
                codes = m.update_param_solve(theta, u_out=u, x_out=x)
            y, z, s = m.duals(); ia = m.info_arrays()
            R._assert_same([codes, m.solution(), y, z, s] + [ia[k_] for k_ in R.INFO_KEYS], out_ref, (devs, pinned))
            assert np.array_equal(u, u_ref) and np.array_equal(x, out_ref[1]), (devs, pinned)
            assert np.array_equal(m.outputs(), u_ref) and np.array_equal(m.outputs(first=3, count=5), u_ref[3:8]), (devs, pinned)
        m.close(); one.close()
        for p_ in (pth, pu, px):
            p_.close()
    finally:
        eicos_amd.set_arithmetic_profile(0)


@pytest.mark.gpu
def test_cpp_param_step_demo_over_a_device_list(tmp_path):
    # examples/param_update_demo.cpp: EiCOS::BatchSolver::setOutputMap / outputs / stepParam from host C++, device list {0, 0}; the program
    # checks that stepParam's u equals the output map applied to solution() bit for bit and prints the step times of the four forms
    import os, subprocess
    from conftest import ROOT
    exe = str(tmp_path / "param_update_demo")
    lib = os.path.join(ROOT, "eicos_amd")
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "param_update_demo.cpp"),
                           "-L", lib, "-leicos_amd", "-Wl,-rpath," + lib, "-o", exe])
    out = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "MPC02.epb"), "48", "0,0", "16", "3"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "over 2 shard(s)" in out.stdout, out.stdout
    for line in ("stepParam u vs the output map applied to solution(): bit-identical", "closed loop, every step: bit-identical",
                 "stepParam (pinned theta, pinned u)"):
        assert line in out.stdout, out.stdout
