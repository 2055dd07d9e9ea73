"""Right-hand-side-only updateData (eicos_batch_update_rhs / _device / _solve and their eicos_multi_* forms, include/eicos_amd.h).

New c, h, b are divided by the scalings each instance's last updateData stored; A, G and the equilibration stay.  The contract is
bit-identity: update(G, A, c1, h1, b1) followed by update_rhs(c2, h2, b2) gives exactly what update(G, A, c2, h2, b2) gives -- the KKT
values, the solution, the duals and every counter -- on every update path (bounce, pinned in place, device, fused into the solve).
The CPU tests check the refusals that need no GPU."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_fixture
import eicos_amd
from eicos_amd import binding
from eicos_amd.generate import dense_front_pattern, feasible_batch, perturbed_batch

KEYS = ("Gpr", "Apr", "c", "h", "b")
INFO_KEYS = ("iter", "pcost", "dcost", "pres", "dres", "n_factor", "n_ldlsolve", "nitref1", "nitref2", "nitref3", "exitcode")


def test_rhs_entry_points_refuse_a_null_handle():
    L = binding._lib()
    z = np.zeros(4)
    dp = z.ctypes.data_as(C.POINTER(C.c_double))
    assert L.eicos_batch_update_rhs(None, 0, 1, dp, None, None) == -1
    assert b"NULL handle" in L.eicos_last_error()
    assert L.eicos_batch_update_rhs_device(None, 0, 1, None, None, None) == -1
    assert L.eicos_batch_update_rhs_solve(None, dp, None, None, None, None) == -1
    assert L.eicos_multi_update_rhs(None, 0, 1, dp, None, None) == -1
    assert L.eicos_multi_update_rhs_device(None, 0, 0, 1, None, None, None) == -1
    assert L.eicos_multi_update_rhs_solve(None, dp, None, None, None, None) == -1


def test_rhs_arrays_of_the_wrong_size_are_refused_before_the_library_is_called():
    pat, _ = load_fixture("lp_afiro")
    arrs, ptrs = binding._rhs_ptrs(pat, 3, np.zeros((3, pat.n)), None, np.zeros((3, pat.p)))
    assert arrs[1] is None and ptrs[1] is None and ptrs[0] is not None and ptrs[2] is not None
    with pytest.raises(ValueError):
        binding._rhs_ptrs(pat, 3, np.zeros((2, pat.n)), None, None)
    with pytest.raises(ValueError):
        binding._rhs_ptrs(pat, 3, None, np.zeros((3, pat.m + 1)), None)


# ---------------------------------------------------------------------------------------------------------------------------------
def _data(name, B):
    if name == "dense-front":
        pat, base = dense_front_pattern(n=150, k=4, d=40)
        return pat, feasible_batch(pat, base, 0, B)
    pat, sets = load_fixture(name)
    if name.startswith("lp_"):
        return pat, perturbed_batch(pat, sets[0], 0, B)
    if name == "MPC02":
        return pat, feasible_batch(pat, sets[0], 0, B)
    return pat, {k: np.repeat(np.asarray(getattr(sets[0], k))[None], B, 0) for k in KEYS}


def _second_rhs(d):
    """A second set of right-hand sides: every group changed (c scaled, inequalities relaxed, b moved a little)."""
    return d["c"] * 1.01, d["h"] + 0.01 * np.abs(d["h"]), d["b"] * (1.0 + 1e-3)


def _outputs(g, codes):
    x = g.solution(); y, z, s = g.duals(); ia = g.info_arrays()
    return [np.asarray(codes).copy(), x, y, z, s] + [ia[k] for k in INFO_KEYS]


def _assert_same(a, b, what=""):
    for k, (u, v) in enumerate(zip(a, b)):
        assert np.array_equal(u, v, equal_nan=True), (what, k)


def _device_arrays(arrs):
    """hipMalloc + hipMemcpy copies of host arrays (the HIP runtime the library is linked against; no torch)."""
    hip = binding._lib()
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    out = []
    for v in arrs:
        v = np.ascontiguousarray(v)
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), max(v.nbytes, 8)) == 0
        if v.nbytes:
            assert hip.hipMemcpy(p, v.ctypes.data, v.nbytes, 1) == 0  # hipMemcpyHostToDevice
        out.append(p.value)
    return out


def _free_device(ptrs):
    hip = binding._lib()
    for p in ptrs:
        hip.hipFree(C.c_void_p(p))


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,env", [("MPC02", 64, {}), ("MPC02", 600, {}), ("lp_afiro", 16, {}), ("lp_adlittle", 32, {}),
                                        ("lp_bandm", 64, {}), ("issue98", 8, {}), ("update_data", 8, {}), ("dense-front", 6, {}),
                                        ("MPC02", 40, {"EICOS_UPDATE_LDS": "0"}), ("MPC02", 40, {"EICOS_NLDS": "0"})])
def test_rhs_update_is_bit_identical_to_a_full_update_with_unchanged_matrices(name, B, env, monkeypatch):
    # every launch shape the pattern and batch pick (LDS-resident, U in LDS, queue order, tiles, the generic updateData kernel, no LDS
    # vector): update(G, A, c1, h1, b1) + update_rhs(c2, h2, b2) == update(G, A, c2, h2, b2), KKT values untouched by update_rhs
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pat, d = _data(name, B)
    c2, h2, b2 = _second_rhs(d)
    G, A = d["Gpr"], d["Apr"]

    ref = eicos_amd.BatchSolver(pat, B)
    ref.update(G, A, c2, h2, b2)
    out_ref = _outputs(ref, ref.solve())
    r, c, kkt_ref = ref.debug_kkt(B - 1)
    ag = (r < pat.n) & (c >= pat.n)  # the equilibrated A', G' entries of the KKT matrix (the scaling block is solve state)

    g = eicos_amd.BatchSolver(pat, B)
    assert g.dims() == ref.dims() and g.kernel_build() == ref.kernel_build()
    g.update(G, A, d["c"], d["h"], d["b"])
    g.solve()
    kkt1 = g.debug_kkt(B - 1)[2].copy()
    g.update_rhs(c2, h2, b2)
    assert g.last_update_path() == "pinned bounce"
    assert np.array_equal(g.debug_kkt(B - 1)[2], kkt1)  # A, G, the scaling block and the constants are not touched ...
    assert np.array_equal(kkt1[ag], kkt_ref[ag])        # ... and A, G equal what a full update with the same matrices stores
    _assert_same(_outputs(g, g.solve()), out_ref, name)

    # NULL keeps a group: only h changes, on both sides
    h3 = h2 + 0.02 * np.abs(d["h"])
    g.update_rhs(h=h3)
    ref.update(G, A, c2, h3, b2)
    _assert_same(_outputs(g, g.solve()), _outputs(ref, ref.solve()), name + " h only")
    # a sub-range touches only its instances
    f, n = B // 4, max(1, B // 3)
    c4 = c2.copy(); c4[f:f + n] = d["c"][f:f + n] * 0.99
    g.update_rhs(c=c4[f:f + n], first=f, count=n)
    ref.update(G, A, c4, h3, b2)
    _assert_same(_outputs(g, g.solve()), _outputs(ref, ref.solve()), name + " sub-range")
    g.close(); ref.close()


@pytest.mark.gpu
def test_rhs_update_keeps_the_bits_of_unchanged_vectors_where_a_kept_matrix_update_moves_them():
    # the reason for the call: re-sending c alone through updateData un-equilibrates and re-equilibrates the kept A, G (reference
    # semantics, src/eicos.cpp:2053-2082), which moves the last bits of the instances; update_rhs with the same c changes nothing
    pat, d = _data("MPC02", 64)
    g = eicos_amd.BatchSolver(pat, 64)
    g.update(*[d[k] for k in KEYS])
    out0 = _outputs(g, g.solve())
    g.update_rhs(c=d["c"][10:30], first=10, count=20)
    _assert_same(_outputs(g, g.solve()), out0)
    g.update(None, None, d["c"][10:30], None, None, first=10, count=20)
    g.solve()
    assert not np.array_equal(g.solution()[10:30], out0[1][10:30])
    g.close()


@pytest.mark.gpu
def test_rhs_update_before_any_matrices_keeps_the_vectors_as_given():
    # no updateData yet: the zero-filled slab has no scalings, the vectors are stored as given (scalings of 1, never a division by an
    # unset value); a later updateData that keeps c equilibrates it exactly as a given one
    pat, d = _data("MPC02", 8)
    ref = eicos_amd.BatchSolver(pat, 8)
    ref.update(*[d[k] for k in KEYS])
    out_ref = _outputs(ref, ref.solve())
    g = eicos_amd.BatchSolver(pat, 8)
    g.update_rhs(d["c"], d["h"], d["b"])
    g.update(d["Gpr"], d["Apr"], None, d["h"], d["b"])  # (h, b travel with G, A in updateData; c is kept)
    _assert_same(_outputs(g, g.solve()), out_ref)
    # the same with a pinned c beside pageable h, b (every array of a call must be pinned for the in-place path)
    g2 = eicos_amd.BatchSolver(pat, 8)
    pc = eicos_amd.PinnedArray(d["c"].shape); pc.a[...] = d["c"]
    g2.update_rhs(pc.a, d["h"], d["b"])
    assert g2.last_update_path() == "pinned bounce"  # (c pinned, h and b pageable: the bounce pipeline for all three)
    g2.update(d["Gpr"], d["Apr"], None, d["h"], d["b"])
    _assert_same(_outputs(g2, g2.solve()), out_ref)
    g.close(); g2.close(); ref.close(); pc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,B", [("MPC02", 600), ("MPC02", 40), ("lp_afiro", 300), ("lp_bandm", 64), ("issue98", 8)])
def test_fused_rhs_update_solve_is_bit_identical_to_update_rhs_then_solve(name, B, monkeypatch):
    # eicos_batch_update_rhs_solve: pinned, registered and device inputs are scaled by the solve kernel's own workgroups (path 5), x goes
    # straight into a pinned x_out; pageable inputs take update_rhs (bounce) + solve, or -- switched on -- the staged form; same bits
    pat, d = _data(name, B)
    c2, h2, b2 = _second_rhs(d)
    G, A = d["Gpr"], d["Apr"]
    ref = eicos_amd.BatchSolver(pat, B)
    ref.update(G, A, d["c"], d["h"], d["b"]); ref.solve()
    ref.update_rhs(c2, h2, b2)
    out_ref = _outputs(ref, ref.solve())
    ref.update_rhs(c=d["c"])
    out_ref_c = _outputs(ref, ref.solve())
    ref.close()

    g = eicos_amd.BatchSolver(pat, B)
    g.update(G, A, d["c"], d["h"], d["b"]); g.solve()
    pins = [eicos_amd.PinnedArray(v.shape) for v in (c2, h2, b2)]
    for p_, v in zip(pins, (c2, h2, b2)):
        p_.a[...] = v
    px = eicos_amd.PinnedArray((B, pat.n))
    codes = g.update_rhs_solve(*[p_.a for p_ in pins], x_out=px.a)
    assert g.last_update_path() == "fused into the solve"
    out = _outputs(g, codes)
    _assert_same(out, out_ref, "pinned")
    assert np.array_equal(px.a, out_ref[1])
    # registered (caller-owned) c only, pageable result array
    own = np.ascontiguousarray(d["c"])
    eicos_amd.host_register(own)
    try:
        xb = np.zeros((B, pat.n))
        codes = g.update_rhs_solve(c=own, x_out=xb)
        assert g.last_update_path() == "fused into the solve"
        _assert_same(_outputs(g, codes), out_ref_c, "registered")
        assert np.array_equal(xb, out_ref_c[1])
    finally:
        eicos_amd.host_unregister(own)
    # device-resident inputs
    dev = _device_arrays((c2, h2, b2))
    try:
        L = binding._lib()
        codes = np.zeros(B, np.int32)
        px.a[...] = 0.0
        assert L.eicos_batch_update_rhs_solve(g._h, *[C.cast(p_, C.POINTER(C.c_double)) for p_ in dev], px.a.ctypes.data_as(C.POINTER(C.c_double)),
                                              codes.ctypes.data_as(C.POINTER(C.c_int))) == 0
        assert g.last_update_path() == "fused into the solve"
        _assert_same(_outputs(g, codes), out_ref, "device")
        assert np.array_equal(px.a, out_ref[1])
        # the device-pointer range form, then a plain solve
        g.update_rhs(c=d["c"])
        g.update_rhs_device(*dev)
        _assert_same(_outputs(g, g.solve()), out_ref, "update_rhs_device")
        # without the fused path the same call takes the device-pointer update, and a device x_out is filled by a copy on the device
        monkeypatch.setenv("EICOS_FUSED_UPDATE", "0")
        dx = _device_arrays((np.zeros((B, pat.n)),))
        try:
            g.update_rhs(c=d["c"])
            codes = np.zeros(B, np.int32)
            assert L.eicos_batch_update_rhs_solve(g._h, *[C.cast(p_, C.POINTER(C.c_double)) for p_ in dev], C.cast(dx[0], C.POINTER(C.c_double)),
                                                  codes.ctypes.data_as(C.POINTER(C.c_int))) == 0
            xd = np.full((B, pat.n), np.nan)
            assert L.hipMemcpy(xd.ctypes.data, dx[0], xd.nbytes, 2) == 0  # hipMemcpyDeviceToHost
            _assert_same(_outputs(g, codes), out_ref, "device, not fused")
            assert np.array_equal(xd, out_ref[1]) and np.array_equal(xd, g.solution())
        finally:
            _free_device(dx)
            monkeypatch.delenv("EICOS_FUSED_UPDATE")
        # a device pointer handed to the host-pointer entry point is refused, naming the right call
        assert L.eicos_batch_update_rhs(g._h, 0, B, C.cast(dev[0], C.POINTER(C.c_double)), None, None) == -1
        assert b"eicos_batch_update_rhs_device" in L.eicos_last_error()
    finally:
        _free_device(dev)
    # pageable inputs: update_rhs through the bounce pipeline, then the solve
    g.update_rhs(c=d["c"])
    codes = g.update_rhs_solve(c2, h2, b2, x_out=px.a)
    assert g.last_update_path() == "pinned bounce"
    _assert_same(_outputs(g, codes), out_ref, "pageable")
    assert np.array_equal(px.a, out_ref[1])
    # ... or staged into the pinned buffer while the kernel runs (experiment switch)
    monkeypatch.setenv("EICOS_FUSED_STAGED", "1")
    g.update_rhs(c=d["c"])
    codes = g.update_rhs_solve(c2, h2, b2, x_out=px.a)
    assert g.last_update_path() == "fused into the solve, staged while it runs"
    _assert_same(_outputs(g, codes), out_ref, "staged")
    g.close()
    for p_ in pins + [px]:
        p_.close()


@pytest.mark.gpu
@pytest.mark.parametrize("soc", [False, True])
def test_rhs_update_with_warm_start_and_dynamic_regularisation(soc):
    # the warm start re-equilibrates the previous solution with the stored scalings and dynamic regularisation acts in the factorisation:
    # both see exactly the state a full update with the same matrices leaves
    pat, d = _data("issue98" if soc else "MPC02", 32)
    c2, h2, b2 = _second_rhs(d)
    outs = []
    for rhs in (False, True):
        g = eicos_amd.BatchSolver(pat, 32)
        g.update(*[d[k] for k in KEYS]); g.solve()
        g.set_warm_start(0.1)
        g.set_dynamic_regularization(2e-7, 1e-13)
        if rhs:
            g.update_rhs(c2, h2, b2)
        else:
            g.update(d["Gpr"], d["Apr"], c2, h2, b2)
        outs.append(_outputs(g, g.solve()))
        g.close()
    _assert_same(outs[0], outs[1])


@pytest.mark.gpu
def test_multi_rhs_update_matches_one_handle():
    # eicos_multi_update_rhs / _device / _solve over device lists {0, 0} and {0, 0, 0, 0}: the rows of every shard, in global order, give the
    # bits of one handle (arithmetic profile 1: plans independent of the shard size)
    pat, d = _data("MPC02", 256)
    c2, h2, b2 = _second_rhs(d)
    eicos_amd.set_arithmetic_profile(1)
    try:
        one = eicos_amd.BatchSolver(pat, 256)
        one.update(*[d[k] for k in KEYS]); one.solve()
        one.update_rhs(c2, h2, b2)
        out_ref = _outputs(one, one.solve())
        one.close()
        dev = _device_arrays((c2, h2, b2))
        try:
            for devs in ([0, 0], [0, 0, 0, 0]):
                m = eicos_amd.MultiBatchSolver(pat, 256, devs)
                for how in ("host", "device", "fused"):
                    m.update(*[d[k] for k in KEYS]); m.solve()
                    if how == "host":
                        m.update_rhs(c2, h2, b2); codes = m.solve()
                    elif how == "device":
                        m.update_rhs_device(0, *dev); codes = m.solve()
                    else:
                        codes = m.update_rhs_solve(c2, h2, b2)
                    x = m.solution(); y, z, s = m.duals(); ia = m.info_arrays()
                    _assert_same([codes, x, y, z, s] + [ia[k] for k in INFO_KEYS], out_ref, (devs, how))
                # a sub-range across the shard boundary
                m.update_rhs(c=d["c"][100:160], first=100, count=60)
                c5 = c2.copy(); c5[100:160] = d["c"][100:160]
                x = (m.solve(), m.solution())
                m.close()
                one = eicos_amd.BatchSolver(pat, 256)
                one.update(d["Gpr"], d["Apr"], c5, h2, b2)
                assert np.array_equal(x[0], one.solve()) and np.array_equal(x[1], one.solution()), devs
                one.close()
        finally:
            _free_device(dev)
    finally:
        eicos_amd.set_arithmetic_profile(0)


@pytest.mark.gpu
def test_rhs_update_refusals():
    pat, d = _data("lp_afiro", 4)
    g = eicos_amd.BatchSolver(pat, 4)
    L = binding._lib()
    dp = d["c"].ctypes.data_as(C.POINTER(C.c_double))
    assert L.eicos_batch_update_rhs(g._h, 2, 3, dp, None, None) == -1  # range out of bounds
    assert b"out of bounds" in L.eicos_last_error()
    assert L.eicos_batch_update_rhs(g._h, -1, 1, dp, None, None) == -1
    assert L.eicos_batch_update_rhs_device(g._h, 0, 5, None, None, None) == -1
    with pytest.raises(ValueError):
        g.update_rhs(c=d["c"][:3], count=4)  # 3 rows for 4 instances
    with pytest.raises(ValueError):
        g.update_rhs_solve(h=np.zeros((4, pat.m + 1)))
    g.close()


@pytest.mark.gpu
def test_cpp_rhs_update_demo_over_a_device_list(tmp_path):
    # examples/rhs_update_demo.cpp: EiCOS::BatchSolver::updateRHS and solve(c, h, b, x_out) from host C++, device list {0, 0}; the program
    # compares every form with updateData of the unchanged matrices bit for bit
    import os, subprocess
    from conftest import ROOT
    exe = str(tmp_path / "rhs_update_demo")
    lib = os.path.join(ROOT, "eicos_amd")
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "rhs_update_demo.cpp"),
                           "-L", lib, "-leicos_amd", "-Wl,-rpath," + lib, "-o", exe])
    out = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "MPC02.epb"), "48", "0,0"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "48 / 48 optimal over 2 shard(s)" in out.stdout, out.stdout
    for line in ("updateRHS + solve vs updateData with unchanged matrices: bit-identical", "one-call solve(c, h, b) on pinned arrays: bit-identical",
                 "sub-range updateRHS: bit-identical"):
        assert line in out.stdout, out.stdout
