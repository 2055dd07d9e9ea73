"""Shared matrix values (eicos_batch_shared_values, knob EICOS_SHARED_VALUES).

When a full device-pointer updateData hands every instance the same Gpr and Apr, equilibration -- which reads A and G only -- leaves the same
bits in every instance's product value copies, and the solve's three matrix-vector products stream instance 0's copies for all of them.  The
feature is transparent: x, y, z, s, the exit codes and every info field except the device wall time are bit for bit those of a handle
created with the knob off, whatever the matrices are; the diagnostic says whether the next solve shares."""
import ctypes

import numpy as np
import pytest

from conftest import load_fixture
import eicos_amd
from eicos_amd.binding import _lib
from eicos_amd.generate import feasible_batch, mpc_soc_variant, perturbed_batch

KEYS = ("Gpr", "Apr", "c", "h", "b")
INFO_SKIP = ("solve_us",)  # device wall time of the instance's solve: the only field that is not a function of the data


def _n_cu():
    n = ctypes.c_int()
    assert _lib().hipDeviceGetAttribute(ctypes.byref(n), 63, 0) == 0  # (hipDeviceAttributeMultiprocessorCount, through the solver's runtime)
    return n.value


class Dev:
    """Device copies of a batch's five arrays (plain hipMalloc / hipMemcpy through the runtime the library is linked against)."""

    def __init__(self):
        self.hip = _lib()
        self.hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        self.hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        self.hip.hipFree.argtypes = [ctypes.c_void_p]
        self.bufs = []

    def put(self, d):
        out = []
        for k in KEYS:
            v = np.ascontiguousarray(d[k], dtype=np.float64)
            p = ctypes.c_void_p()
            if v.size:
                assert self.hip.hipMalloc(ctypes.byref(p), v.nbytes) == 0
                assert self.hip.hipMemcpy(p, v.ctypes.data, v.nbytes, 1) == 0  # hipMemcpyHostToDevice
                self.bufs.append(p.value)
            out.append(p.value or 0)
        return out

    def free(self):
        for p in self.bufs:
            self.hip.hipFree(ctypes.c_void_p(p))
        self.bufs = []


def _results(g, codes=None):
    codes = np.asarray(g.solve() if codes is None else codes).copy()
    y, z, s = g.duals()
    out = dict(codes=codes, x=g.solution().copy(), y=y.copy(), z=z.copy(), s=s.copy())
    out.update({"info." + k: np.asarray(v).copy() for k, v in g.info_arrays().items() if k not in INFO_SKIP})
    return out


def _same(a, b):
    assert set(a) == set(b) and {"info.iter", "info.pcost", "info.n_ldlsolve"} <= set(a)
    for k in sorted(a):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def _mpc02(B):
    pat, sets = load_fixture("MPC02")
    return pat, feasible_batch(pat, sets[0], 0, B)


def _mpc_soc(B):
    pat, sets = load_fixture("MPC02")
    pat = mpc_soc_variant(pat, sets[0])
    return pat, feasible_batch(pat, sets[0], 0, B)


def _netlib(name, B):
    pat, sets = load_fixture(name)
    return pat, perturbed_batch(pat, sets[0], 0, B)


def _dense_front(B):
    from test_gpu_parity import dense_front_pattern
    pat, base = dense_front_pattern(n=150, k=4, d=40)
    return pat, feasible_batch(pat, base, 0, B)


# name -> (batch or None = one more instance than CUs, problem, what kernel_build() / dims() must say, shares)
SHAPES = {
    "mpc02_b6": (6, _mpc02, lambda kb, d, B: kb != "lds-resident" and d["resident_blocks"] == B, True),
    # one instance more than CUs: the smallest batch that runs two workgroups per CU, i.e. the 256-VGPR build of the headline
    "mpc02_two_per_cu": (None, _mpc02, lambda kb, d, B: kb == "w2" and d["resident_blocks"] == B and d["iterate_park"] == 1, True),
    "mpc_soc_b6": (6, _mpc_soc, lambda kb, d, B: kb != "lds-resident" and d["ncones"] > 0, True),
    "lp_bandm_b4": (4, lambda B: _netlib("lp_bandm", B), lambda kb, d, B: kb == "u-in-lds" and d["factor_path"] == 2, True),  # hybrid, U in LDS
    "dense_front_b6": (6, _dense_front, lambda kb, d, B: kb != "lds-resident" and d["factor_path"] == 1, True),  # tile products (i_Gt)
    "lp_afiro_b4": (4, lambda B: _netlib("lp_afiro", B), lambda kb, d, B: kb == "lds-resident" and d["lds_resident"] == 1, False),
}
_CACHE = {}


def _problem(name):
    """(pattern, batch arrays, B) of a shape: generated once, shared by the tests, never modified (the tests copy what they change)."""
    if name not in _CACHE:
        B, make, _, _ = SHAPES[name]
        B = _n_cu() + 1 if B is None else B
        pat, d = make(B)
        for k in ("Gpr", "Apr"):
            assert d[k].size == 0 or np.array_equal(d[k], np.broadcast_to(d[k][0], d[k].shape))  # every instance gets the same matrices
            d[k].setflags(write=False)
        _CACHE[name] = (pat, d, B)
    return _CACHE[name]


def _pair(name, monkeypatch):
    """(handle with the feature, handle created with the knob off) of a shape, builds confirmed."""
    pat, d, B = _problem(name)
    monkeypatch.setenv("EICOS_SHARED_VALUES", "0")
    off = eicos_amd.BatchSolver(pat, B)
    monkeypatch.delenv("EICOS_SHARED_VALUES")
    on = eicos_amd.BatchSolver(pat, B)
    check = SHAPES[name][2]
    for g in (on, off):
        assert check(g.kernel_build(), g.dims(), B), (g.kernel_build(), g.dims())
    assert not on.shared_values() and not off.shared_values()
    return on, off, pat, d, B


def _changed(d, i, e=0, value=None):
    """The batch with entry e of instance i's G replaced (default: scaled by 1 + 2^-20)."""
    out = dict(d)
    G = d["Gpr"].copy()
    G[i, e] = G[i, e] * (1 + 2.0 ** -20) if value is None else value
    assert value is not None or G[i, e] != d["Gpr"][i, e]
    out["Gpr"] = G
    return out


def _update_both(on, off, dev, d):
    ptrs = dev.put(d)
    on.update_device(*ptrs)
    off.update_device(*ptrs)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_identical_matrices_are_shared_and_one_differing_entry_is_not(name, monkeypatch):
    on, off, pat, d, B = _pair(name, monkeypatch)
    shares = SHAPES[name][3]
    dev = Dev()
    try:
        # identical matrices
        _update_both(on, off, dev, d)
        assert on.shared_values() == shares and not off.shared_values()
        ref = _results(off)
        _same(_results(on), ref)
        assert (ref["codes"] == 0).any()
        # one entry of G differs: in the last instance, then in instance 0 (the reference itself)
        for i in (B - 1, 0):
            dd = _changed(d, i, e=d["Gpr"].shape[1] // 2)
            _update_both(on, off, dev, dd)
            assert not on.shared_values()
            _same(_results(on), _results(off))
        # identical again: shared again, and the first results again
        _update_both(on, off, dev, d)
        assert on.shared_values() == shares
        _same(_results(on), ref)
    finally:
        dev.free(); on.close(); off.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_signed_zero_is_a_difference(name, monkeypatch):
    # bit patterns, not values: +0.0 in every instance is shared, -0.0 in one of them is not (a float comparison would call them equal)
    on, off, pat, d, B = _pair(name, monkeypatch)
    shares = SHAPES[name][3]
    dev = Dev()
    try:
        e = d["Gpr"].shape[1] - 1
        plus = dict(d); G = d["Gpr"].copy(); G[:, e] = 0.0; plus["Gpr"] = G
        _update_both(on, off, dev, plus)
        assert on.shared_values() == shares
        _same(_results(on), _results(off))
        minus = _changed(plus, B // 2, e=e, value=-0.0)
        assert np.array_equal(minus["Gpr"], plus["Gpr"]) and np.signbit(minus["Gpr"][B // 2, e])
        _update_both(on, off, dev, minus)
        assert not on.shared_values()
        _same(_results(on), _results(off))
    finally:
        dev.free(); on.close(); off.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_invalidation_order(name, monkeypatch):
    on, off, pat, d, B = _pair(name, monkeypatch)
    shares = SHAPES[name][3]
    dev = Dev()
    try:
        full = dev.put(d)
        # a full identical update shares
        on.update_device(*full); off.update_device(*full)
        assert on.shared_values() == shares
        # a sub-range update of one instance with other values does not, and the results are those of the knob-off handle
        other = _changed(d, B - 1, e=1)
        one = [other[k][B - 1:B] for k in KEYS]
        on.update(*one, first=B - 1, count=1); off.update(*one, first=B - 1, count=1)
        assert not on.shared_values()
        _same(_results(on), _results(off))
        # a full identical update shares again
        on.update_device(*full); off.update_device(*full)
        assert on.shared_values() == shares
        # a right-hand-side-only update keeps it (host arrays and device pointers)
        c2 = d["c"] * (1 + 2.0 ** -12)
        on.update_rhs(c2, d["h"], d["b"]); off.update_rhs(c2, d["h"], d["b"])
        assert on.shared_values() == shares
        on.update_rhs_device(full[2], full[3], full[4]); off.update_rhs_device(full[2], full[3], full[4])
        assert on.shared_values() == shares
        ref = _results(off)
        _same(_results(on), ref)
        # a sub-range device update of ALL but one instance, and a full one that keeps A or G, are not the detecting launch
        on.update_device(*full, first=0, count=B - 1); off.update_device(*full, first=0, count=B - 1)
        assert not on.shared_values()
        on.update_device(*full); off.update_device(*full)
        assert on.shared_values() == shares
        if pat.p > 0:  # (A kept: un-equilibrated and equilibrated again from every instance's own slab)
            on.update_device(full[0], 0, full[2], full[3], 0); off.update_device(full[0], 0, full[2], full[3], 0)
            assert not on.shared_values()
            _same(_results(on), _results(off))
            on.update_device(*full); off.update_device(*full)
            assert on.shared_values() == shares
        # update_solve drops it
        host = [d[k] for k in KEYS]
        codes_on = on.update_solve(*host); codes_off = off.update_solve(*host)
        assert not on.shared_values()
        _same(_results(on, codes_on), _results(off, codes_off))
    finally:
        dev.free(); on.close(); off.close()


@pytest.mark.gpu
def test_two_shards_on_one_device_each_have_their_own_reference(monkeypatch):
    # eicos_multi_* over the device list {0, 0}: every shard compares with ITS first instance and streams ITS reference -- the two shards
    # get different matrices here (identical inside each), and everything equals one knob-off handle over the whole batch
    pat, d6, _ = _problem("mpc02_b6")
    B, half = 12, 6
    d = {k: np.concatenate([d6[k], d6[k]]) for k in KEYS}
    d["Gpr"][half:] *= 1 + 2.0 ** -16
    assert not np.array_equal(d["Gpr"][0], d["Gpr"][half])
    dev = Dev()
    monkeypatch.setenv("EICOS_SHARED_VALUES", "0")
    off = eicos_amd.BatchSolver(pat, B)
    monkeypatch.delenv("EICOS_SHARED_VALUES")
    m = eicos_amd.MultiBatchSolver(pat, B, [0, 0])
    try:
        assert m.shards() == [(0, half, 0), (half, half, 0)]
        ptrs = dev.put(d)
        off.update_device(*ptrs)
        ref = _results(off)
        assert not off.shared_values()
        m.update_device(0, *ptrs)
        assert m.shard_shared_values(0) and m.shard_shared_values(1)
        _same(_results(m), ref)
        # a difference inside shard 1 only: shard 0 still shares
        dd = _changed(d, B - 1, e=3)
        ptrs = dev.put(dd)
        off.update_device(*ptrs); m.update_device(0, *ptrs)
        assert m.shard_shared_values(0) and not m.shard_shared_values(1)
        _same(_results(m), _results(off))
    finally:
        dev.free(); m.close(); off.close()


def test_the_binding_declares_the_diagnostic():
    import os
    from conftest import ROOT
    assert open(os.path.join(ROOT, "include", "eicos_amd.h")).read().count("int eicos_batch_shared_values(eicos_batch *hd);") == 1
    assert callable(eicos_amd.BatchSolver.shared_values) and callable(eicos_amd.MultiBatchSolver.shard_shared_values)
