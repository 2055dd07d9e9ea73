"""Parametric matrix updates: the stored values of G and A affine in theta (eicos_batch_set_matrix_map / _has_matrix_map and their
eicos_multi_* forms, include/eicos_amd.h).

A handle holds a matrix map beside the parameter map: Gpr = G0 + Gm theta, Apr = A0 + Am theta, one CSR row per stored value.  With it
installed every call that consumes theta (update_param, update_param_device, update_param_solve, rollout) is a full updateData whose
inputs the GPU forms from theta.  The contract is bit-identity with the host sequence

    update(G(theta) or None, A(theta) or None, c(theta) or None, h(theta) if G is mapped, b(theta) if A is mapped)
    update_rhs(None, h(theta) if h is mapped and G is not, b(theta) if b is mapped and A is not)        (when not empty)

on the host-evaluated arrays: the KKT values, x, y, z, s, the exit codes and every counter -- on the range path, fused into the solve
launch, in a rollout, on every build of the solve kernel and every transfer path.  Every comparison is np.array_equal.  Bit-identity does
not need optimal exits, and none is asserted.  The CPU tests check MatrixMap.evaluate and the refusals that need no GPU."""
import numpy as np
import pytest

import eicos_amd
from eicos_amd import binding
from eicos_amd.binding import MatrixMap
import test_param_update as P  # (its _data, _map, _theta, _twins)
import test_rhs_update as R    # (its _outputs, _assert_same and device-array helpers)
import test_rollout as RO      # (its _fmap, _w, _host_loop, _assert_rollout)
from test_param_step import _omap, _pinned

KEYS = R.KEYS


def _mcsr(rng, base, k, full_rows=0):
    """One matrix of the test map: the base values, about 80 % of the rows empty and 1-3 entries in the others (`full_rows` rows hold
    all k columns, in shuffled order), values about 1e-3 of the base."""
    rows = base.size
    length = np.where(rng.random(rows) < 0.8, 0, rng.integers(1, min(3, k) + 1, rows))
    if rows:
        length[rng.choice(rows, min(full_rows, rows), replace=False)] = k
    rowptr = np.concatenate(([0], np.cumsum(length))).astype(np.int32)
    col = np.concatenate([rng.permutation(k)[:n_] for n_ in length] + [np.zeros(0, np.int64)]).astype(np.int32)
    scale = 1e-3 * (np.abs(base) + np.mean(np.abs(base)) + 1e-6)
    val = rng.uniform(-1, 1, col.size) * np.repeat(scale, length)
    return base.copy(), rowptr, col, val


def _mmap(d, k, groups="GA", seed=0, full_rows=0):
    """The matrix map of a case: base = instance 0's Gpr / Apr of the generated batch."""
    rng = np.random.default_rng(6000 + seed)
    return MatrixMap(k, **{g: _mcsr(rng, d[g + "pr"][0], k, full_rows) for g in groups})


def _host_sequence(ref, pm, mm, theta, first=0):
    """The contract's right-hand side on handle `ref`, for the instances [first, first + len(theta))."""
    G, A = mm.evaluate(theta) if mm is not None else (None, None)
    c, h, b = pm.evaluate(theta)
    n = theta.shape[0]
    if mm is None:
        ref.update_rhs(c, h, b, first=first, count=n)
        return
    ref.update(G, A, c, h if G is not None else None, b if A is not None else None, first=first, count=n)
    h2, b2 = (h if G is None else None), (b if A is None else None)
    if h2 is not None or b2 is not None:
        ref.update_rhs(None, h2, b2, first=first, count=n)


def _one(pat, d, B):
    """One more handle in the state of P._twins: update(G, A, c, h, b) and one solve."""
    g = eicos_amd.BatchSolver(pat, B)
    g.update(*[d[k_] for k_ in KEYS])
    g.solve()
    return g


def _same_state(g, ref, B, what):
    assert np.array_equal(g.debug_kkt(B - 1)[2], ref.debug_kkt(B - 1)[2], equal_nan=True), (what, "kkt")
    R._assert_same(R._outputs(g, g.solve()), R._outputs(ref, ref.solve()), what)


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_matrix_map_entry_points_refuse_a_null_handle():
    L = binding._lib()
    for rc in (L.eicos_batch_set_matrix_map(None, None, None), L.eicos_batch_has_matrix_map(None)):
        assert rc == -1 and b"NULL handle" in L.eicos_last_error()
    for rc in (L.eicos_multi_set_matrix_map(None, None, None), L.eicos_multi_has_matrix_map(None)):
        assert rc == -1 and b"NULL handle" in L.eicos_multi_last_error()


def test_matrix_map_evaluate_equals_a_scalar_loop_in_the_stated_order():
    # acc = base[e]; for t in stored order: acc = acc + (val[t] * theta[col[t]]) on Python floats (IEEE doubles, no fused multiply-add)
    base = np.array([0.1, -2.5, 3.0, 1e-3])
    rowptr = np.array([0, 3, 3, 4, 7], np.int32)
    col = np.array([2, 0, 1, 1, 0, 2, 1], np.int32)  # (row 1 is empty; rows 0 and 3 are not sorted)
    val = np.array([1 / 3, 1e-7, -0.7, 2 / 7, 0.3, 1e10, -1e10])  # (row 3 ends with 1e10 terms that all but cancel)
    theta = np.array([[0.1, 0.7, 1 / 9], [0.9, 0.3, 0.123456789]])
    for which in (0, 1):
        mm = MatrixMap(3, **{"GA"[which]: (base, rowptr, col, val)})
        got = mm.evaluate(theta)
        assert got[1 - which] is None and got[which].shape == (2, 4)
        for i in range(2):
            for e in range(4):
                acc = float(base[e])
                for t in range(rowptr[e], rowptr[e + 1]):
                    acc = acc + (float(val[t]) * float(theta[i, col[t]]))
                assert got[which][i, e] == acc, (which, i, e)
        assert np.array_equal(got[which][:, 1], [base[1]] * 2)  # the empty row is its base


def test_matrix_map_arrays_of_the_wrong_size_are_refused_before_the_library_is_called():
    nG, nA = 6, 4
    none = (np.zeros(0, np.int32), np.zeros(0))
    ok = MatrixMap(2, G=(np.zeros(nG), np.zeros(nG + 1, np.int32), *none), A=None)
    keep, ptrs = binding._matrix_map_ptrs(ok, nG, nA)
    assert ptrs[0] is not None and ptrs[1] is None
    with pytest.raises(ValueError, match="matrix map of G"):  # a base of the wrong length
        binding._matrix_map_ptrs(MatrixMap(2, G=(np.zeros(nG + 1), np.zeros(nG + 1, np.int32), *none)), nG, nA)
    with pytest.raises(ValueError, match="matrix map of A"):  # row pointers that run past the stored entries
        binding._matrix_map_ptrs(MatrixMap(2, A=(np.zeros(nA), np.full(nA + 1, 3, np.int32), np.zeros(2, np.int32), np.zeros(2))), nG, nA)
    with pytest.raises(ValueError):  # theta of the wrong shape
        ok.evaluate(np.zeros((3, 3)))
    with pytest.raises(ValueError):
        ok.evaluate(np.zeros(2))


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,B,k,mats,vecs,full_rows,env", [
    ("MPC02", 40, 7, "GA", "chb", 0, {}),
    ("lp_afiro", 16, 1, "GA", "chb", 0, {}),
    ("issue98", 8, 5, "G", "h", 0, {}),                    # cones; no equality rows
    ("socp-random", 8, 5, "GA", "hb", 0, {}),              # cones with equality rows; c is not mapped and is kept
    ("MPC02", 40, 7, "A", "hb", 0, {}),                    # G is not mapped: h goes through the update_rhs follow-up
    ("MPC02", 40, 7, "GA", "chb", 0, {"EICOS_NLDS": "0"}),  # no LDS vector
    ("lp_afiro", 5, 1100, "GA", "chb", 2, {}),             # theta rows too long for LDS; a last group of one instance
    ("dense-front", 6, 3, "G", "h", 0, {}),                # values not in LDS: k_update_lds<512, false> behind the staging buffer
    # several queue rounds, rows that hold all 200 columns; one instance expands to 123 760 bytes of inputs (+ padding), so a staging
    # cap of 32 MB holds 270 instances and the 600 go in three chunks
    ("MPC02", 600, 200, "GA", "chb", 4, {"EICOS_MATRIX_STAGE_MB": "32"}),
])
def test_matrix_param_update_is_bit_identical_to_update_of_the_evaluated_arrays(name, B, k, mats, vecs, full_rows, env, monkeypatch):
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    pat, d = P._data(name, B)
    pm, mm = P._map(d, k, vecs, full_rows=full_rows), _mmap(d, k, mats, full_rows=full_rows)
    g, ref = P._twins(pat, d, B)
    assert g.dims() == ref.dims() and g.kernel_build() == ref.kernel_build()
    g.set_param_map(pm)
    assert g.has_matrix_map() == 0
    g.set_matrix_map(mm)
    assert g.has_matrix_map() == ("G" in mats) * 1 + ("A" in mats) * 2
    rows, cols, kkt0 = g.debug_kkt(B - 1)
    kkt0 = kkt0.copy()
    ag = (rows < pat.n) & (cols >= pat.n)  # the equilibrated A', G' entries of the KKT matrix
    for step in range(2):  # (the second theta on the solved state)
        theta = P._theta(B, k, seed=step)
        g.update_param(theta)
        assert g.last_update_path() == "pinned bounce"
        _host_sequence(ref, pm, mm, theta)
        if step == 0:
            assert not np.array_equal(g.debug_kkt(B - 1)[2][ag], kkt0[ag])  # the matrices did move
        _same_state(g, ref, B, (name, "step", step))
    g.close(); ref.close()


@pytest.mark.gpu
def test_matrix_param_update_of_a_sub_range_touches_only_its_instances():
    B, k = 40, 7
    pat, d = P._data("MPC02", B)
    pm, mm = P._map(d, k), _mmap(d, k)
    theta = P._theta(B, k)
    f, n = B // 4, B // 3
    g, ref = P._twins(pat, d, B)
    untouched = _one(pat, d, B)
    g.set_param_map(pm); g.set_matrix_map(mm)
    g.update_param(theta[f:f + n], first=f, count=n)
    _host_sequence(ref, pm, mm, theta[f:f + n], first=f)
    keep = np.r_[0:f, f + n:B]
    slab = [g.debug_kkt(i)[2].copy() for i in (0, f, B - 1)]
    assert np.array_equal(slab[0], untouched.debug_kkt(0)[2]) and np.array_equal(slab[2], untouched.debug_kkt(B - 1)[2])
    assert np.array_equal(slab[1], ref.debug_kkt(f)[2]) and not np.array_equal(slab[1], untouched.debug_kkt(f)[2])
    out = R._outputs(g, g.solve())
    R._assert_same(out, R._outputs(ref, ref.solve()))
    x0 = (untouched.solve(), untouched.solution())[1]
    assert np.array_equal(out[1][keep], x0[keep]) and not np.array_equal(out[1][f:f + n], x0[f:f + n])
    g.close(); ref.close(); untouched.close()


@pytest.mark.gpu
def test_matrix_param_update_over_every_transfer_path():
    B, k = 64, 7
    pat, d = P._data("MPC02", B)
    pm, mm = P._map(d, k), _mmap(d, k)
    g, ref = P._twins(pat, d, B)
    g.set_param_map(pm); g.set_matrix_map(mm)

    def check(theta, what):
        _host_sequence(ref, pm, mm, theta)
        _same_state(g, ref, B, what)

    theta = P._theta(B, k, seed=10)
    g.update_param(theta)
    assert g.last_update_path() == "pinned bounce"
    check(theta, "pageable")
    pin = eicos_amd.PinnedArray((B, k)); pin.a[...] = P._theta(B, k, seed=11)
    g.update_param(pin.a)
    assert g.last_update_path() == "pinned source in place"
    check(pin.a, "pinned")
    theta = P._theta(B, k, seed=13)
    dev = R._device_arrays((theta,))
    try:
        g.update_param_device(dev[0])
        check(theta, "device")
    finally:
        R._free_device(dev)
    g.close(); ref.close(); pin.close()


@pytest.mark.gpu
def test_multi_matrix_param_update_from_device_theta_matches_one_handle():
    # device list {0, 0}, arithmetic profile 1 (plans independent of the shard size): theta in the HBM of device 0 gives the bits of one handle
    B, k = 64, 7
    pat, d = P._data("MPC02", B)
    pm, mm = P._map(d, k), _mmap(d, k)
    theta = P._theta(B, k)
    eicos_amd.set_arithmetic_profile(1)
    try:
        one = _one(pat, d, B)
        _host_sequence(one, pm, mm, theta)
        want = R._outputs(one, one.solve())
        one.close()
        m = eicos_amd.MultiBatchSolver(pat, B, [0, 0])
        m.update(*[d[k_] for k_ in KEYS]); m.solve()
        m.set_param_map(pm)
        assert m.has_matrix_map() == 0
        m.set_matrix_map(mm)
        assert m.has_matrix_map() == 3
        dev = R._device_arrays((theta,))
        try:
            m.update_param_device(0, dev[0])
            codes = m.solve()
        finally:
            R._free_device(dev)
        x = m.solution(); y, z, s = m.duals(); ia = m.info_arrays()
        R._assert_same([codes, x, y, z, s] + [ia[k_] for k_ in R.INFO_KEYS], want, "multi {0, 0}, device theta")
        m.set_matrix_map(None)
        assert m.has_matrix_map() == 0
        m.close()
    finally:
        eicos_amd.set_arithmetic_profile(0)


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,mats,vecs,env,build", [
    ("MPC02", 4, "GA", "chb", {"EICOS_UBL": "0", "EICOS_THREADS": "256"}, ("w2", 256)),
    ("MPC02", 4, "GA", "chb", {"EICOS_UBL": "0", "EICOS_THREADS": "256", "EICOS_W2": "0"}, ("default", 256)),
    ("MPC02", 4, "GA", "chb", {"EICOS_UBL": "0", "EICOS_W2": "0", "EICOS_THREADS": "128"}, ("default", 128)),
    ("MPC02", 4, "GA", "chb", {"EICOS_UBL": "0", "EICOS_W2": "0", "EICOS_THREADS": "512"}, ("default", 512)),
    ("issue98", 4, "G", "h", {"EICOS_THREADS": "256"}, ("u-in-lds", 256)),
    ("lp_bandm", 96, "GA", "chb", {}, ("u-in-lds", 512)),
    ("lp_afiro", 4, "GA", "chb", {}, ("lds-resident", 128)),
    ("MPC02", 40, "A", "chb", {}, None),   # h without G: evaluated by the fused step itself
])
def test_fused_matrix_param_step_equals_the_range_path_on_every_build_of_the_solve_kernel(name, B, mats, vecs, env, build, monkeypatch):
    # the (pattern, batch, knobs) of test_param_step.py that reach each compilation of k_solve.  Three handles in the same state: `g` takes
    # the one-call step with pinned theta, u_out and x_out; `ref` update_param + solve + outputs; `unf` the one-call step with the fused
    # update switched off.  The step is fused (path 5) when the handle has an LDS vector and the pattern is inside the in-register
    # accumulators of the fused updateData (n, p <= 8, m <= 16 entries per thread: include/eicos_amd.h) -- MPC02 (m = 3996) at 128
    # threads is not, and takes the range path.
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    k, r = 5, 4
    pat, d = P._data(name, B)
    pm, mm, om = P._map(d, k, vecs), _mmap(d, k, mats), _omap(pat.n, r)
    g, ref = P._twins(pat, d, B)
    unf = _one(pat, d, B)
    T = g.dims()["threads_per_block"]
    if build is not None:
        assert (g.kernel_build(), T) == build, (g.kernel_build(), T)
    for s in (g, ref, unf):
        s.set_param_map(pm); s.set_matrix_map(mm); s.set_output_map(om)
    fused = g.dims()["lds_bytes"] > 0 and pat.n <= 8 * T and pat.p <= 8 * T and pat.m <= 16 * T
    assert fused == (build != ("default", 128)), (build, fused)
    pth, pu, px = _pinned((B, k), (B, r), (B, pat.n))
    qu, qx = _pinned((B, r), (B, pat.n))
    for step in range(2):
        what = (name, build, "step", step)
        pth.a[...] = P._theta(B, k, seed=step)
        ref.update_param(pth.a.copy())
        out_ref = R._outputs(ref, ref.solve())
        u_ref = ref.outputs()
        for a in (pu, px, qu, qx):
            a.a[...] = np.nan
        codes = g.update_param_solve(pth.a, u_out=pu.a, x_out=px.a)
        assert (g.last_update_path() == "fused into the solve") == fused, (what, g.last_update_path())
        monkeypatch.setenv("EICOS_FUSED_UPDATE", "0")
        codes0 = unf.update_param_solve(pth.a, u_out=qu.a, x_out=qx.a)
        monkeypatch.delenv("EICOS_FUSED_UPDATE")
        assert unf.last_update_path() == "pinned source in place", what
        for s, c_, u, x in ((g, codes, pu.a, px.a), (unf, codes0, qu.a, qx.a)):
            R._assert_same(R._outputs(s, c_), out_ref, what)
            assert np.array_equal(u, u_ref) and np.array_equal(u, om.evaluate(out_ref[1])), what
            assert np.array_equal(x, out_ref[1]), what
            assert np.array_equal(s.debug_kkt(B - 1)[2], ref.debug_kkt(B - 1)[2], equal_nan=True), what
    # ... and the twin itself is the host sequence on the evaluated arrays
    host = _one(pat, d, B)
    for step in range(2):
        _host_sequence(host, pm, mm, P._theta(B, k, seed=step))
        out_host = R._outputs(host, host.solve())
    R._assert_same(out_host, out_ref, (name, build, "host sequence"))
    for s in (g, ref, unf, host):
        s.close()
    for p_ in (pth, pu, px, qu, qx):
        p_.close()


@pytest.mark.gpu
@pytest.mark.parametrize("B", [8, 40])
def test_matrix_param_rollout_fused_unfused_and_host_loop_agree(B, monkeypatch):
    name, k, r, T = "MPC02", 7, 6, 3
    pat, d = P._data(name, B)
    pm, mm, om, fm = P._map(d, k), _mmap(d, k), _omap(pat.n, r), RO._fmap(k, r)
    g, ref = P._twins(pat, d, B)
    unf = _one(pat, d, B)
    for s in (g, ref, unf):
        s.set_param_map(pm); s.set_matrix_map(mm); s.set_output_map(om)
    g.set_plant_map(fm); unf.set_plant_map(fm)
    theta0, w = P._theta(B, k), RO._w(B, T, k)
    want = RO._host_loop(ref, fm, theta0, T, w)
    got = g.rollout(theta0, T, w)
    assert g.last_rollout_launches() == 1
    monkeypatch.setenv("EICOS_FUSED_UPDATE", "0")
    got0 = unf.rollout(theta0, T, w)
    monkeypatch.delenv("EICOS_FUSED_UPDATE")
    assert unf.last_rollout_launches() == T
    for s, res, what in ((g, got, "fused"), (unf, got0, "not fused")):
        RO._assert_rollout(res, want, (B, what))
        R._assert_same(R._outputs(s, RO._final_codes(s)), R._outputs(ref, RO._final_codes(ref)), (B, what))
        assert np.array_equal(s.debug_kkt(B - 1)[2], ref.debug_kkt(B - 1)[2], equal_nan=True), (B, what)
    for s in (g, ref, unf):
        s.close()


@pytest.mark.gpu
def test_matrix_param_update_with_warm_start():
    B, k = 32, 7
    pat, d = P._data("MPC02", B)
    pm, mm = P._map(d, k), _mmap(d, k)
    g, ref = P._twins(pat, d, B)
    for s in (g, ref):
        s.set_warm_start(0.1)
    g.set_param_map(pm); g.set_matrix_map(mm)
    for step in range(2):
        theta = P._theta(B, k, seed=step)
        g.update_param(theta)
        _host_sequence(ref, pm, mm, theta)
        _same_state(g, ref, B, ("warm", step))
    g.close(); ref.close()


@pytest.mark.gpu
def test_matrix_map_can_be_replaced_and_removed_and_is_checked_against_the_parameter_map():
    B, k = 16, 3
    pat, d = P._data("lp_afiro", B)
    pm = P._map(d, k)
    g, ref = P._twins(pat, d, B)
    g.set_param_map(pm)
    g.set_matrix_map(_mmap(d, k, "GA", seed=1))
    assert g.has_matrix_map() == 3
    theta = P._theta(B, k)
    g.update_param(theta)
    _host_sequence(ref, pm, _mmap(d, k, "GA", seed=1), theta)
    # replaced by a map for G alone: A is kept and re-equilibrated, b goes through the right-hand-side follow-up
    mm = _mmap(d, k, "G", seed=2)
    g.set_matrix_map(mm)
    assert g.has_matrix_map() == 1
    theta = P._theta(B, k, seed=1)
    g.update_param(theta)
    _host_sequence(ref, pm, mm, theta)
    _same_state(g, ref, B, "replaced")
    # removed: update_param is the right-hand-side update again and leaves G, A and the scalings alone
    g.set_matrix_map(None)
    assert g.has_matrix_map() == 0
    kkt1 = g.debug_kkt(B - 1)[2].copy()
    theta = P._theta(B, k, seed=2)
    g.update_param(theta)
    assert np.array_equal(g.debug_kkt(B - 1)[2], kkt1)
    _host_sequence(ref, pm, None, theta)
    _same_state(g, ref, B, "removed")
    # the parameter map replaced behind the matrix map's back: another k, then a map without h while G is mapped
    g.set_matrix_map(mm)
    g.set_param_map(P._map(d, 6, seed=3))
    with pytest.raises(RuntimeError, match=r"installed for k = 3.*k = 6"):
        g.update_param(P._theta(B, 6))
    g.set_param_map(P._map(d, k, "cb", seed=4))
    with pytest.raises(RuntimeError, match="matrix map of G: the parameter map has no h group"):
        g.update_param(theta)
    with pytest.raises(RuntimeError, match="no h group"):
        g.update_param_solve(theta)
    with pytest.raises(RuntimeError, match="no h group"):  # ... and at installation
        g.set_matrix_map(_mmap(d, k, "G", seed=5))
    assert g.has_matrix_map() == 1  # (a refused map replaces nothing)
    g.set_param_map(P._map(d, k, "ch", seed=4))
    with pytest.raises(RuntimeError, match="matrix map of A: the parameter map has no b group"):
        g.set_matrix_map(_mmap(d, k, "A", seed=5))
    g.set_param_map(pm)
    # content refusals
    base, rowptr, col, val = _mmap(d, k, "G", seed=6).G
    bad = col.copy(); bad[-1] = k
    with pytest.raises(RuntimeError, match=r"matrix map of G: column 3 .* outside \[0, k\)"):
        g.set_matrix_map(MatrixMap(k, G=(base, rowptr, bad, val)))
    bad = rowptr.copy(); bad[0] = 1
    with pytest.raises(RuntimeError, match=r"rowptr\[0\]"):
        g.set_matrix_map(MatrixMap(k, G=(base, bad, col, val)))
    e = int(np.nonzero(np.diff(rowptr) >= 1)[0][0])
    bad = rowptr.copy(); bad[e + 1] = bad[e] - 1
    with pytest.raises(RuntimeError, match="rowptr decreases"):
        g.set_matrix_map(MatrixMap(k, G=(base, bad, col, val)))
    g.set_matrix_map(None)
    g.set_param_map(None)
    with pytest.raises(RuntimeError, match="matrix map of G: no parameter map"):
        g.set_matrix_map(mm)
    g.close(); ref.close()
    # an A map on a pattern without equality rows
    pat, d = P._data("issue98", 2)
    g = eicos_amd.BatchSolver(pat, 2)
    g.set_param_map(P._map(d, 2, "h"))
    empty = (np.zeros(0), np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    with pytest.raises(RuntimeError, match="matrix map of A: the pattern has no such matrix"):
        g.set_matrix_map(MatrixMap(2, A=empty))
    g.close()
