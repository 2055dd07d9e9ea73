"""Parametric right-hand-side updates (eicos_batch_set_param_map / _update_param / _update_param_device and their eicos_multi_* forms,
include/eicos_amd.h).

A handle holds one map c = c0 + C theta, h = h0 + H theta, b = b0 + B theta (CSR matrices with k columns, a group may be left out);
update_param sends theta [count][k] and the GPU expands it, every product and every sum rounded to fp64 on its own, in stored order,
then divides by the stored scalings.  The contract is bit-identity: update_param(theta) leaves exactly the state that
update_rhs(*map.evaluate(theta)) leaves, so every later solve gives the same x, y, z, s, exit codes and counters -- on every transfer
path.  Bit-identity does not need optimal exits, and none is asserted.  The CPU tests check ParamMap.evaluate and the refusals that need
no GPU."""
import ctypes as C

import numpy as np
import pytest

import eicos_amd
from eicos_amd import binding
from eicos_amd.binding import ParamMap
from eicos_amd.generate import feasible_batch, random_socp_pattern
import test_rhs_update as R  # (its _data, _outputs, _assert_same and device-array helpers)

KEYS = R.KEYS
DP = C.POINTER(C.c_double)


def _csr(rng, base, k, full_rows=0):
    """One group of the test map: the base vector, 0-5 entries per row (a fifth of the rows empty; `full_rows` rows hold all k columns,
    in shuffled order), values about 1e-3 of the base."""
    rows = base.size
    length = np.where(rng.random(rows) < 0.2, 0, rng.integers(0, min(5, k) + 1, rows))
    if rows:
        length[rng.choice(rows, min(full_rows, rows), replace=False)] = k
    rowptr = np.concatenate(([0], np.cumsum(length))).astype(np.int32)
    col = np.concatenate([rng.permutation(k)[:n_] for n_ in length] + [np.zeros(0, np.int64)]).astype(np.int32)
    scale = 1e-3 * (np.abs(base) + np.mean(np.abs(base)) + 1e-6)
    val = rng.uniform(-1, 1, col.size) * np.repeat(scale, length)
    return base.copy(), rowptr, col, val


def _map(d, k, groups="chb", seed=0, full_rows=0):
    """The synthetic map of a case: base = instance 0's (c, h, b) of the generated batch (G and A are the same for every instance).  A
    group the pattern does not have (no equality rows: b) gets no map -- the library refuses one (test_param_update_refusals)."""
    rng = np.random.default_rng(1000 + seed)
    return ParamMap(k, **{g: _csr(rng, d[g][0], k, full_rows) for g in groups if d[g].shape[1] > 0})


def _data(name, B):
    if name == "socp-random":  # cones AND equality rows (no fixture has both): 8 LP rows, cones of 4 and 7, 6 equalities
        pat, base = random_socp_pattern(30, 6, 8, [4, 7], seed=3)
        return pat, feasible_batch(pat, base, 0, B)
    return R._data(name, B)


def _theta(B, k, seed=0):
    return np.random.default_rng(2000 + seed).uniform(0, 1, (B, k))


def _twins(pat, d, B, make=None):
    """Two handles in the same state: update(G, A, c, h, b) and one solve."""
    out = []
    for _ in range(2):
        g = make() if make else eicos_amd.BatchSolver(pat, B)
        g.update(*[d[k_] for k_ in KEYS])
        g.solve()
        out.append(g)
    return out


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_param_entry_points_refuse_a_null_handle():
    L = binding._lib()
    z = np.zeros(4)
    dp = z.ctypes.data_as(DP)
    err = L.eicos_last_error
    for rc in (L.eicos_batch_set_param_map(None, 1, None, None, None), L.eicos_batch_param_count(None), L.eicos_batch_update_param(None, 0, 1, dp),
               L.eicos_batch_update_param_device(None, 0, 1, None)):
        assert rc == -1 and b"NULL handle" in err()
    err = L.eicos_multi_last_error
    for rc in (L.eicos_multi_set_param_map(None, 1, None, None, None), L.eicos_multi_param_count(None), L.eicos_multi_update_param(None, 0, 1, dp),
               L.eicos_multi_update_param_device(None, 0, 0, 1, None)):
        assert rc == -1 and b"NULL handle" in err()


def test_param_map_evaluate_matches_a_dense_product():
    rng = np.random.default_rng(5)
    k, B = 9, 7
    base = {g: rng.standard_normal(r) for g, r in (("c", 40), ("h", 63), ("b", 11))}
    pm = ParamMap(k, c=_csr(rng, base["c"], k, full_rows=3), h=_csr(rng, base["h"], k), b=None)
    theta = rng.uniform(0, 1, (B, k))
    c, h, b = pm.evaluate(theta)
    assert b is None and c.shape == (B, 40) and h.shape == (B, 63)
    for got, (b0, rowptr, col, val) in ((c, pm.c), (h, pm.h)):
        P = np.zeros((b0.size, k))
        for r in range(b0.size):
            P[r, col[rowptr[r]:rowptr[r + 1]]] = val[rowptr[r]:rowptr[r + 1]]
        want = b0[None, :] + theta @ P.T
        assert np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(want))


def test_param_map_evaluate_equals_a_scalar_loop_in_the_stated_order():
    # acc = base[r]; for t in stored order: acc = acc + (val[t] * theta[col[t]]) on Python floats (IEEE doubles, no fused multiply-add)
    base = np.array([0.1, -2.5, 3.0, 1e-3])
    rowptr = np.array([0, 3, 3, 4, 7], np.int32)
    col = np.array([2, 0, 1, 1, 0, 2, 1], np.int32)  # (row 1 is empty; row 3 repeats no column but is not sorted)
    val = np.array([1 / 3, 1e-7, -0.7, 2 / 7, 0.3, 1e10, -1e10])
    theta = np.array([[0.1, 0.7, 1 / 9], [0.9, 0.3, 0.123456789]])
    got = ParamMap(3, h=(base, rowptr, col, val)).evaluate(theta)
    assert got[0] is None and got[2] is None
    for i in range(2):
        for r in range(4):
            acc = float(base[r])
            for t in range(rowptr[r], rowptr[r + 1]):
                acc = acc + (float(val[t]) * float(theta[i, col[t]]))
            assert got[1][i, r] == acc, (i, r)


def test_theta_of_the_wrong_shape_is_refused_before_the_library_is_called():
    theta, count = binding._theta_rows(np.zeros((3, 5)), 5, None)
    assert count == 3 and theta.dtype == np.float64
    for bad, k, count in ((np.zeros((3, 4)), 5, None), (np.zeros(15), 5, None), (np.zeros((3, 5)), 5, 4), (np.zeros((3, 5, 1)), 5, 3)):
        with pytest.raises(ValueError):
            binding._theta_rows(bad, k, count)
    with pytest.raises(ValueError):
        ParamMap(5, c=(np.zeros(2), np.zeros(3, np.int32), np.zeros(0, np.int32), np.zeros(0))).evaluate(np.zeros((3, 4)))
    pat, _ = R.load_fixture("lp_afiro")
    ok = ParamMap(2, c=(np.zeros(pat.n), np.zeros(pat.n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0)))
    keep, ptrs = binding._param_map_ptrs(ok, pat)
    assert ptrs[0] is not None and ptrs[1] is None and ptrs[2] is None
    with pytest.raises(ValueError):  # a base of the wrong length
        binding._param_map_ptrs(ParamMap(2, c=(np.zeros(pat.n + 1), np.zeros(pat.n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0))), pat)
    with pytest.raises(ValueError):  # row pointers that run past the stored entries
        binding._param_map_ptrs(ParamMap(2, c=(np.zeros(pat.n), np.full(pat.n + 1, 3, np.int32), np.zeros(2, np.int32), np.zeros(2))), pat)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,B,k,groups,full_rows,env", [
    ("MPC02", 40, 7, "chb", 0, {}),
    ("lp_afiro", 16, 1, "chb", 0, {}),
    ("issue98", 8, 5, "hb", 0, {}),              # cones; c is not parametric (and the fixture has no equality rows: h alone is mapped)
    ("socp-random", 8, 5, "hb", 0, {}),          # cones with equality rows: h and b mapped, c not
    ("MPC02", 600, 200, "chb", 6, {}),           # several queue rounds, rows that hold all 200 columns
    ("MPC02", 40, 7, "chb", 0, {"EICOS_NLDS": "0"}),
    ("dense-front", 6, 3, "ch", 0, {}),          # (the pattern has no equality rows)
    ("lp_afiro", 5, 1100, "chb", 2, {}),         # theta rows too long for LDS: read through the cache; a last group of one instance
])
def test_param_update_is_bit_identical_to_update_rhs_of_the_evaluated_vectors(name, B, k, groups, full_rows, env, monkeypatch):
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    pat, d = _data(name, B)
    pm = _map(d, k, groups, full_rows=full_rows)
    theta = _theta(B, k)
    g, ref = _twins(pat, d, B)
    assert g.dims() == ref.dims() and g.kernel_build() == ref.kernel_build()
    assert g.param_count() == 0
    g.set_param_map(pm)
    assert g.param_count() == k
    kkt1 = g.debug_kkt(B - 1)[2].copy()
    g.update_param(theta)
    assert g.last_update_path() == "pinned bounce"
    assert np.array_equal(g.debug_kkt(B - 1)[2], kkt1)  # A, G, the scaling block and the constants are not touched
    ref.update_rhs(*pm.evaluate(theta))
    R._assert_same(R._outputs(g, g.solve()), R._outputs(ref, ref.solve()), name)
    # a second theta on the solved state
    theta2 = _theta(B, k, seed=1)
    g.update_param(theta2)
    ref.update_rhs(*pm.evaluate(theta2))
    R._assert_same(R._outputs(g, g.solve()), R._outputs(ref, ref.solve()), name + " second step")
    g.close(); ref.close()


@pytest.mark.gpu
def test_param_map_of_b_alone_keeps_c_and_h():
    B, k = 40, 4
    pat, d = _data("MPC02", B)
    pm = _map(d, k, "b")
    theta = _theta(B, k)
    c, h, b = pm.evaluate(theta)
    assert c is None and h is None
    g, ref = _twins(pat, d, B)
    g.set_param_map(pm)
    # c and h keep their bits: b moved by update_param and put back by update_rhs, with no solve in between (a solve leaves its
    # Information behind, as the reference's does), gives the second solve of an untouched handle exactly
    g.update_param(theta)
    g.update_rhs(b=d["b"])
    out0 = R._outputs(ref, ref.solve())
    R._assert_same(R._outputs(g, g.solve()), out0)
    # and solving with the mapped b equals update_rhs(b=...)
    g.update_param(theta)
    ref.update_rhs(b=b)
    out = R._outputs(g, g.solve())
    R._assert_same(out, R._outputs(ref, ref.solve()))
    assert not np.array_equal(out[1], out0[1])
    g.close(); ref.close()


@pytest.mark.gpu
def test_param_update_of_a_sub_range_touches_only_its_instances():
    B, k = 40, 7
    pat, d = _data("MPC02", B)
    pm = _map(d, k)
    theta = _theta(B, k)
    f, n = B // 4, B // 3
    g, ref = _twins(pat, d, B)
    g.set_param_map(pm)
    g.update_param(theta[f:f + n], first=f, count=n)
    c, h, b = (v[f:f + n] for v in pm.evaluate(theta))
    ref.update_rhs(c, h, b, first=f, count=n)
    out = R._outputs(g, g.solve())
    R._assert_same(out, R._outputs(ref, ref.solve()))
    untouched = eicos_amd.BatchSolver(pat, B)
    untouched.update(*[d[k_] for k_ in KEYS]); untouched.solve()
    x0 = (untouched.solve(), untouched.solution())[1]
    keep = np.r_[0:f, f + n:B]
    assert np.array_equal(out[1][keep], x0[keep]) and not np.array_equal(out[1][f:f + n], x0[f:f + n])
    g.close(); ref.close(); untouched.close()


@pytest.mark.gpu
def test_param_map_can_be_replaced_and_removed():
    B = 16
    pat, d = _data("lp_afiro", B)
    g, ref = _twins(pat, d, B)
    g.set_param_map(_map(d, 3, seed=1))
    g.update_param(_theta(B, 3))
    pm = _map(d, 6, "ch", seed=2)  # another k, another set of groups
    g.set_param_map(pm)
    assert g.param_count() == 6
    with pytest.raises(ValueError):
        g.update_param(_theta(B, 3))  # rows of the old width
    theta = _theta(B, 6, seed=3)
    g.update_param(theta)
    c, h, b = pm.evaluate(theta)
    # (b was set by the first map's update: the twin gets those bits through the first map as well)
    first = _map(d, 3, seed=1)
    ref.update_rhs(*first.evaluate(_theta(B, 3)))
    ref.update_rhs(c, h, None)
    R._assert_same(R._outputs(g, g.solve()), R._outputs(ref, ref.solve()))
    L = binding._lib()
    for remove in (lambda: g.set_param_map(None), lambda: g.set_param_map(ParamMap(6))):
        g.set_param_map(pm)
        remove()
        assert g.param_count() == 0
        assert L.eicos_batch_update_param(g._h, 0, B, theta.ctypes.data_as(DP)) == -1
        assert b"no parameter map" in L.eicos_last_error()
        assert L.eicos_batch_update_param_device(g._h, 0, B, None) == -1 and b"no parameter map" in L.eicos_last_error()
        with pytest.raises(RuntimeError, match="no parameter map"):
            g.update_param(theta)
    g.close(); ref.close()


@pytest.mark.gpu
def test_param_update_over_every_transfer_path():
    B, k = 64, 7
    pat, d = _data("MPC02", B)
    pm = _map(d, k)
    g, ref = _twins(pat, d, B)
    g.set_param_map(pm)
    L = binding._lib()

    def check(theta, what):
        ref.update_rhs(*pm.evaluate(theta))
        R._assert_same(R._outputs(g, g.solve()), R._outputs(ref, ref.solve()), what)

    theta = _theta(B, k, seed=10)
    g.update_param(theta)
    assert g.last_update_path() == "pinned bounce"
    check(theta, "pageable")
    pin = eicos_amd.PinnedArray((B, k)); pin.a[...] = _theta(B, k, seed=11)
    g.update_param(pin.a)
    assert g.last_update_path() == "pinned source in place"
    check(pin.a, "pinned")
    own = _theta(B, k, seed=12)
    eicos_amd.host_register(own)
    try:
        g.update_param(own)
        assert g.last_update_path() == "pinned source in place"
        check(own, "registered")
    finally:
        eicos_amd.host_unregister(own)
    theta = _theta(B, k, seed=13)
    dev = R._device_arrays((theta,))
    try:
        g.update_param_device(dev[0])
        check(theta, "device")
        # a device pointer handed to the host-pointer entry point is refused, naming the right call
        assert L.eicos_batch_update_param(g._h, 0, B, C.cast(dev[0], DP)) == -1
        assert b"eicos_batch_update_param_device" in L.eicos_last_error()
    finally:
        R._free_device(dev)
    g.close(); ref.close(); pin.close()


@pytest.mark.gpu
def test_param_update_before_any_matrices_keeps_the_vectors_as_given():
    # no updateData yet: scalings of 1, as for update_rhs; a later updateData that keeps c equilibrates it exactly as a given one
    B, k = 8, 7
    pat, d = _data("MPC02", B)
    pm = _map(d, k)
    theta = _theta(B, k)
    c, h, b = pm.evaluate(theta)
    ref = eicos_amd.BatchSolver(pat, B)
    ref.update(d["Gpr"], d["Apr"], c, h, b)
    out_ref = R._outputs(ref, ref.solve())
    g = eicos_amd.BatchSolver(pat, B)
    g.set_param_map(pm)
    g.update_param(theta)
    g.update(d["Gpr"], d["Apr"], None, h, b)  # (h, b travel with G, A in updateData; c is kept)
    R._assert_same(R._outputs(g, g.solve()), out_ref)
    g.close(); ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["MPC02", "issue98"])
def test_param_update_with_warm_start_and_dynamic_regularisation(name):
    B, k = 32, 7
    pat, d = _data(name, B)
    pm = _map(d, k)
    theta = _theta(B, k)
    outs = []
    for param in (False, True):
        g = eicos_amd.BatchSolver(pat, B)
        g.update(*[d[k_] for k_ in KEYS]); g.solve()
        g.set_warm_start(0.1)
        g.set_dynamic_regularization(2e-7, 1e-13)
        if param:
            g.set_param_map(pm)
            g.update_param(theta)
        else:
            g.update_rhs(*pm.evaluate(theta))
        outs.append(R._outputs(g, g.solve()))
        g.close()
    R._assert_same(outs[0], outs[1])


@pytest.mark.gpu
def test_multi_param_update_matches_one_handle():
    # device lists {0, 0} and {0, 0, 0, 0}, arithmetic profile 1 (plans independent of the shard size): host theta, device theta and a
    # sub-range across a shard boundary give the bits of one handle
    B, k = 256, 7
    pat, d = _data("MPC02", B)
    pm = _map(d, k)
    theta, theta2 = _theta(B, k), _theta(B, k, seed=1)
    eicos_amd.set_arithmetic_profile(1)
    try:
        # one handle goes through the same sequence of calls as every multi handle below (a solve leaves its Information behind, as the
        # reference's does, so both sides get the same history): twice update + solve + theta + solve, then instances [100, 160) move on
        # to theta2
        c, h, b = (v[100:160] for v in pm.evaluate(theta2))
        one = eicos_amd.BatchSolver(pat, B)
        out_ref = []
        for how in ("device", "host"):
            one.update(*[d[k_] for k_ in KEYS]); one.solve()
            one.update_rhs(*pm.evaluate(theta))
            out_ref.append(R._outputs(one, one.solve()))
        one.update_rhs(c, h, b, first=100, count=60)
        out_sub = R._outputs(one, one.solve())
        one.close()
        dev = R._device_arrays((theta,))
        try:
            for devs in ([0, 0], [0, 0, 0, 0]):
                m = eicos_amd.MultiBatchSolver(pat, B, devs)
                m.set_param_map(pm)
                assert m.param_count() == k

                def outputs(codes):
                    x = m.solution(); y, z, s = m.duals(); ia = m.info_arrays()
                    return [codes, x, y, z, s] + [ia[k_] for k_ in R.INFO_KEYS]

                for how, want in zip(("device", "host"), out_ref):
                    m.update(*[d[k_] for k_ in KEYS]); m.solve()
                    if how == "host":
                        m.update_param(theta)
                    else:
                        m.update_param_device(0, dev[0])
                    R._assert_same(outputs(m.solve()), want, (devs, how))
                m.update_param(theta2[100:160], first=100, count=60)
                R._assert_same(outputs(m.solve()), out_sub, (devs, "sub-range"))
                m.close()
        finally:
            R._free_device(dev)
    finally:
        eicos_amd.set_arithmetic_profile(0)


@pytest.mark.gpu
def test_param_update_refusals():
    B = 4
    pat, d = _data("lp_afiro", B)
    g = eicos_amd.BatchSolver(pat, B)
    L = binding._lib()
    err = L.eicos_last_error
    good = _map(d, 3)

    def install(k, c=None, h=None, b=None):
        keep, ptrs = binding._param_map_ptrs(ParamMap(k, c=c, h=h, b=b), pat)
        return L.eicos_batch_set_param_map(g._h, k, *ptrs)

    base, rowptr, col, val = good.c
    bad = rowptr.copy(); bad[0] = 1
    assert install(3, c=(base, bad, col, val)) == -1 and b"rowptr[0]" in err()
    r = int(np.nonzero(rowptr[:-1] >= 1)[0][0])
    bad = rowptr.copy(); bad[r + 1] = bad[r] - 1
    assert install(3, c=(base, bad, col, val)) == -1 and b"rowptr decreases" in err()
    bad = col.copy(); bad[-1] = 3
    assert install(3, c=(base, rowptr, bad, val)) == -1 and b"outside [0, k)" in err()
    bad = col.copy(); bad[0] = -1
    assert install(3, c=(base, rowptr, bad, val)) == -1 and b"outside [0, k)" in err()
    assert g.param_count() == 0  # (a refused map installs nothing)
    g.set_param_map(good)
    theta = _theta(B, 3)
    dp = theta.ctypes.data_as(DP)
    assert L.eicos_batch_update_param(g._h, 2, 3, dp) == -1 and b"out of bounds" in err()
    assert L.eicos_batch_update_param(g._h, -1, 1, dp) == -1 and b"out of bounds" in err()
    assert L.eicos_batch_update_param_device(g._h, 0, 5, dp) == -1 and b"out of bounds" in err()
    with pytest.raises(ValueError):
        g.update_param(theta[:3], count=4)
    with pytest.raises(ValueError):
        g.update_param(np.zeros((B, 4)))
    g.close()
    # a map for a group the pattern does not have: the dense-front pattern has no equality rows
    pat, d = _data("dense-front", 2)
    g = eicos_amd.BatchSolver(pat, 2)
    empty = (np.zeros(0), np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    with pytest.raises(RuntimeError, match="parameter map of b: the pattern has no such group"):
        g.set_param_map(ParamMap(2, b=empty))
    g.close()


@pytest.mark.gpu
def test_cpp_param_update_demo_over_a_device_list(tmp_path):
    # examples/param_update_demo.cpp: EiCOS::BatchSolver::setParamMap / updateParam from host C++, device list {0, 0}; the program compares
    # updateParam + solve with updateRHS of the host-evaluated vectors bit for bit, then times a short closed loop in both forms
    import os, subprocess
    from conftest import ROOT
    exe = str(tmp_path / "param_update_demo")
    lib = os.path.join(ROOT, "eicos_amd")
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "param_update_demo.cpp"),
                           "-L", lib, "-leicos_amd", "-Wl,-rpath," + lib, "-o", exe])
    out = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "MPC02.epb"), "48", "0,0"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "over 2 shard(s)" in out.stdout, out.stdout
    for line in ("updateParam + solve vs updateRHS of the host-evaluated vectors: bit-identical", "sub-range updateParam: bit-identical",
                 "closed loop, every step: bit-identical"):
        assert line in out.stdout, out.stdout
