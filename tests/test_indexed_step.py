"""Update, read and step a chosen subset (eicos_batch_update_indexed / _update_rhs_indexed / _update_param_indexed / _set_iterate_indexed and
their _device forms, _outputs_indexed, _update_param_solve_subset, and the eicos_multi_* forms; include/eicos_amd.h).

An indexed update is its range namesake with the slab taken from a list; the step over a subset is the three indexed calls in one launch.
So every GPU check is an equality: the handle ends with the bits of a twin that ran the loop of count = 1 range calls (resp. the three
calls), and every instance outside the list keeps what a snapshot taken before the call shows.  The CPU tests check what needs no GPU: the
entry points refuse a NULL handle, and the Python wrappers refuse mis-shaped rows and non-integer lists before the library is called."""
import ctypes as C

import numpy as np
import pytest

import eicos_amd
from eicos_amd import binding
from eicos_amd.binding import ShiftMap
import test_param_update as P   # (its _map, _theta)
import test_rhs_update as R     # (its device-array helpers)
import test_solve_subset as S   # (its BUILDS, _data, _handle, _setup, _state, _assert_rows)
from test_matrix_param import _mmap
from test_param_step import _omap

KEYS = S.KEYS
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
K, NR = 5, 4  # parameters and outputs of the test maps
FUSED = "fused into the solve"


# ---- helpers ----------------------------------------------------------------------------------------------------------------------
def _list(B):
    """An unsorted list with the first and the last instance."""
    return [B - 1, 0, 2]


def _rest(B, idx):
    return [i for i in range(B) if i not in set(int(v) for v in idx)]


def _rows_for(d, idx, seed):
    """New rows for the instances idx: the matrices scaled a little (the pattern kept), c and h moved as S._perturbed moves them."""
    rng = np.random.default_rng(seed)
    sub = {k: d[k][idx] for k in KEYS}
    return {"Gpr": sub["Gpr"] * (1 + 1e-3), "Apr": sub["Apr"].copy(),
            "c": sub["c"] * (1 + 0.01 * rng.uniform(-1, 1, sub["c"].shape)),
            "h": sub["h"] + 0.01 * (1 + np.abs(sub["h"])) * rng.uniform(0, 1, sub["h"].shape), "b": sub["b"].copy()}


def _none_if_empty(a):
    return a if a.shape[1] else None


class _Registered:
    """Copies of host arrays in ONE page-aligned buffer that is registered as a whole (eicos_amd.host_register): small arrays of their
    own could share a page, which registers only once."""

    def __init__(self, arrs):
        sizes = [0 if a is None else (a.size + 7) // 8 * 8 for a in arrs]
        self._buf = np.zeros(sum(sizes) + 1024)
        off = (-self._buf.ctypes.data % 4096) // 8
        self._all = self._buf[off:off + max(sum(sizes), 8)]
        eicos_amd.host_register(self._all)
        self.views, at = [], 0
        for a, n in zip(arrs, sizes):
            if a is None:
                self.views.append(None)
                continue
            v = self._all[at:at + a.size].reshape(a.shape)
            v[...] = a
            self.views.append(v)
            at += n

    def release(self):
        eicos_amd.host_unregister(self._all)


def _call_indexed(g, kind, idx, arrs, memory):
    """One indexed update of `kind` on g from `arrs` (None keeps a group) held in `memory`; returns the update path it must leave (None:
    the call leaves none)."""
    if memory == "pageable":
        getattr(g, kind + "_indexed")(idx, *arrs)
        return "pinned bounce"
    if memory == "pinned":
        reg = _Registered(arrs)
        try:
            getattr(g, kind + "_indexed")(idx, *reg.views)
        finally:
            reg.release()
        return "pinned source in place"
    dev = R._device_arrays([a for a in arrs if a is not None])
    try:
        it = iter(dev)
        getattr(g, kind + "_indexed_device")(idx, *[0 if a is None else next(it) for a in arrs])
        g.sync()
    finally:
        R._free_device(dev)
    return None


def _call_loop(ref, kind, idx, arrs):
    """The contract's right-hand side: the loop of count = 1 range calls on the twin."""
    for q, i in enumerate(idx):
        getattr(ref, kind)(*[None if a is None else a[q:q + 1] for a in arrs], first=int(i), count=1)


def _maps(pat, d, g_list, k=K, r=NR):
    pm, om = P._map(d, k), _omap(pat.n, r)
    for g in g_list:
        g.set_param_map(pm)
        g.set_output_map(om)
    return pm, om


def _three_calls(ref, idx, theta):
    """update_param_indexed + solve_subset + outputs_indexed (+ the x rows) on the twin."""
    ref.update_param_indexed(idx, theta)
    codes = ref.solve_subset(idx)
    return codes, ref.outputs_indexed(idx), ref.solution()[np.asarray(idx, dtype=np.int64)]


def _step_and_compare(g, ref, idx, theta, what, kkt=True, u_out=None, x_out=None, expect_fused=None):
    """One update_param_solve_subset on g against the three calls on ref: codes, u, x, the state of the listed rows, and every other row
    against the snapshot (info and solve_us included)."""
    B = g.batch
    rest = _rest(B, idx)
    before, us = S._state(g, kkt=kkt), g.info_arrays()["solve_us"].copy()
    codes = g.update_param_solve_subset(idx, theta, u_out=u_out, x_out=x_out)
    if expect_fused is not None:
        assert (g.last_update_path() == FUSED) == expect_fused, (what, g.last_update_path())
    want_codes, want_u, want_x = _three_calls(ref, idx, np.array(theta))
    assert np.array_equal(codes, want_codes), (what, codes, want_codes)
    if u_out is not None:
        assert np.array_equal(u_out, want_u), (what, "u")
    if x_out is not None:
        assert np.array_equal(x_out, want_x), (what, "x")
    got, want = S._state(g, kkt=kkt), S._state(ref, kkt=kkt)
    S._assert_rows(got, want, idx, (what, "listed rows"))
    S._assert_rows(got, before, rest, (what, "rows outside the list"))
    assert np.array_equal(g.info_arrays()["solve_us"][rest], us[rest]), (what, "solve_us outside the list")
    assert np.array_equal(g.outputs_indexed(idx), want_u), (what, "outputs_indexed")
    return codes


class _NoLibrary(binding.BatchSolver):
    """A BatchSolver that never reaches the library: what the wrappers check on their own is checked without a GPU."""

    def __init__(self, pat, batch, k, r):
        self.pat, self.batch, self._k, self._r, self._h = pat, batch, k, r, None

    def _call(self, name, *args):
        raise AssertionError("the library was called: " + name)

    def param_count(self):
        return self._k

    def output_count(self):
        return self._r

    def close(self):
        pass


# ---- CPU --------------------------------------------------------------------------------------------------------------------------
def test_indexed_entry_points_refuse_a_null_handle():
    L = binding._lib()
    one = np.zeros(1, np.int32)
    ip, dp = binding._ip(one), binding._dp(np.zeros(4))
    single = [
        L.eicos_batch_update_indexed(None, ip, 1, dp, dp, dp, dp, dp), L.eicos_batch_update_rhs_indexed(None, ip, 1, dp, dp, dp),
        L.eicos_batch_update_param_indexed(None, ip, 1, dp), L.eicos_batch_set_iterate_indexed(None, ip, 1, dp, dp, dp, dp),
        L.eicos_batch_update_indexed_device(None, ip, 1, None, None, None, None, None),
        L.eicos_batch_update_rhs_indexed_device(None, ip, 1, None, None, None), L.eicos_batch_update_param_indexed_device(None, ip, 1, None),
        L.eicos_batch_set_iterate_indexed_device(None, ip, 1, None, None, None, None),
        L.eicos_batch_outputs_indexed(None, ip, 1, dp), L.eicos_batch_outputs_indexed_device(None, ip, 1, None),
        L.eicos_batch_update_param_solve_subset(None, ip, 1, dp, None, None, None),
    ]
    for k, rc in enumerate(single):
        assert rc == -1, k
    assert L.eicos_batch_update_param_solve_subset(None, ip, 1, dp, None, None, None) == -1 and b"NULL handle" in L.eicos_last_error()
    assert L.eicos_batch_update_rhs_indexed(None, ip, 0, None, None, None) == -1 and b"NULL handle" in L.eicos_last_error()
    multi = [
        lambda: L.eicos_multi_update_indexed(None, ip, 1, dp, dp, dp, dp, dp), lambda: L.eicos_multi_update_rhs_indexed(None, ip, 1, dp, dp, dp),
        lambda: L.eicos_multi_update_param_indexed(None, ip, 1, dp), lambda: L.eicos_multi_set_iterate_indexed(None, ip, 1, dp, dp, dp, dp),
        lambda: L.eicos_multi_outputs_indexed(None, ip, 1, dp), lambda: L.eicos_multi_update_param_solve_subset(None, ip, 1, dp, None, None, None),
    ]
    for k, call in enumerate(multi):
        assert call() == -1 and b"NULL handle" in L.eicos_multi_last_error(), k


def test_python_wrappers_refuse_bad_rows_and_lists_before_the_library_is_called():
    pat, _ = S._data("lp_afiro", 8)
    g = _NoLibrary(pat, 8, K, NR)
    idx = [3, 0, 5]
    row = lambda w, n=3: np.zeros((n, w))  # noqa: E731
    bad_rows = [
        lambda: g.update_indexed(idx, Gpr=row(pat.nnzG, 2), h=row(pat.m)),
        lambda: g.update_indexed(idx, c=row(pat.n + 1)),
        lambda: g.update_rhs_indexed(idx, c=row(pat.n, 4)),
        lambda: g.update_rhs_indexed(idx, h=np.zeros(3 * pat.m)),          # the right size, no row per index
        lambda: g.update_param_indexed(idx, np.zeros((2, K))),
        lambda: g.update_param_indexed(idx, np.zeros((3, K + 1))),
        lambda: g.set_iterate_indexed(idx, x=row(pat.n, 8)),
        lambda: g.update_param_solve_subset(idx, np.zeros((8, K))),
        lambda: g.update_param_solve_subset(idx, np.zeros((3, K)), u_out=np.zeros((8, NR))),
        lambda: g.update_param_solve_subset(idx, np.zeros((3, K)), x_out=np.zeros((3, pat.n + 1))),
        lambda: g.update_indexed([[0, 1], [2, 3]], c=row(pat.n, 4)),       # a list of lists
    ]
    for k, call in enumerate(bad_rows):
        with pytest.raises(ValueError):
            call()
    for lst in ([0.0, 2.0], np.array([1.5]), ["a"], [True, 2.5]):
        for call in (lambda: g.update_rhs_indexed(lst, c=row(pat.n, len(lst))), lambda: g.outputs_indexed(lst),
                     lambda: g.update_param_solve_subset(lst, np.zeros((len(lst), K))), lambda: g.update_param_indexed_device(lst, 0)):
            with pytest.raises(TypeError):
                call()
    # what is well-formed does reach the library
    with pytest.raises(AssertionError, match="update_rhs_indexed"):
        g.update_rhs_indexed(np.array(idx, np.int64), c=row(pat.n))
    with pytest.raises(AssertionError, match="update_param_solve_subset"):
        g.update_param_solve_subset([], np.zeros((0, K)))


# ---- GPU --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("memory", ["pageable", "pinned", "device"])
@pytest.mark.parametrize("name,B", [("lp_afiro", 8), ("MPC02", 6), ("socp-random", 8)])
def test_each_indexed_kind_equals_the_loop_of_range_calls(name, B, memory, monkeypatch):
    pat, d, g, ref = S._setup(name, B, {}, None, monkeypatch)
    pm = P._map(d, K)
    for s in (g, ref):
        s.set_param_map(pm)
        s.set_warm_start(0.1)
    idx = _list(B)
    rest = _rest(B, idx)
    new = _rows_for(d, idx, seed=21)
    x0 = None
    for step, kind in enumerate(("update", "update_rhs", "update_param", "set_iterate")):
        if kind == "update":
            arrs = [new[k] if new[k].shape[1] else None for k in KEYS]
        elif kind == "update_rhs":
            arrs = [_none_if_empty(a) for a in (new["c"] * 1.01, new["h"] * 1.01, new["b"])]
        elif kind == "update_param":
            arrs = [P._theta(len(idx), K, seed=step)]
        else:  # a point near the one the last solve left, inside the cones
            y, z, s_ = x0[1]
            arrs = [_none_if_empty(a) for a in (x0[0][idx] * (1 + 1e-3), y[idx], z[idx] * 1.001, s_[idx] * 1.001)]
        before, path0 = S._state(g, kkt=True), g.last_update_path()
        path = _call_indexed(g, kind, idx, arrs, memory)
        assert g.last_update_path() == (path if path is not None else path0), (name, kind, memory)
        S._assert_rows(S._state(g, kkt=True), before, rest, (name, kind, memory, "rows outside the list before the solve"))
        _call_loop(ref, kind, idx, arrs)
        S._assert_rows(S._state(g, kkt=True), S._state(ref, kkt=True), range(B), (name, kind, memory, "before the solve"))
        assert np.array_equal(g.solve(), ref.solve()), (name, kind, memory)
        S._assert_rows(S._state(g, kkt=True), S._state(ref, kkt=True), range(B), (name, kind, memory, "after the solve"))
        x0 = (g.solution(), g.duals())
    g.close()
    ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,mats,vecs,env", [
    ("MPC02", 13, "G", "chb", {"EICOS_MATRIX_STAGE_MB": "1"}),   # G only (b through the right-hand-side follow-up); 8 instances per staging chunk
    ("MPC02", 13, "GA", "chb", {"EICOS_MATRIX_STAGE_MB": "1"}),  # both matrices; a list of 11 takes two chunks
    ("dense-front", 6, "G", "h", {}),                            # values not in LDS: k_update_lds<512, false>
    ("MPC02", 6, "GA", "chb", {"EICOS_UPDATE_LDS": "0"}),        # the generic updateData kernel
])
def test_param_indexed_under_a_matrix_map(name, B, mats, vecs, env, monkeypatch):
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    pat, d = P._data(name, B)
    g, ref = P._twins(pat, d, B)
    pm, mm = P._map(d, K, vecs), _mmap(d, K, mats)
    for s in (g, ref):
        s.set_param_map(pm)
        s.set_matrix_map(mm)
    idx = [int(v) for v in np.random.default_rng(4).permutation(B)[:max(3, B - 2)]]
    if 0 not in idx:
        idx[0] = 0
    if B - 1 not in idx:
        idx[1] = B - 1
    assert len(set(idx)) == len(idx)
    rest = _rest(B, idx)
    theta = P._theta(len(idx), K, seed=9)
    before = S._state(g, kkt=True)
    g.update_param_indexed(idx, theta)
    assert g.last_update_path() == "pinned bounce"
    for q, i in enumerate(idx):
        ref.update_param(theta[q:q + 1], first=i, count=1)
    got = S._state(g, kkt=True)
    S._assert_rows(got, before, rest, (name, mats, "rows outside the list"))
    S._assert_rows(got, S._state(ref, kkt=True), range(B), (name, mats, "before the solve"))
    assert not np.array_equal(got["kkt"][idx[0]], before["kkt"][idx[0]])  # (the matrices did move)
    assert np.array_equal(g.solve(), ref.solve())
    S._assert_rows(S._state(g, kkt=True), S._state(ref, kkt=True), range(B), (name, mats, "after the solve"))
    g.close()
    ref.close()


@pytest.mark.gpu
def test_shared_values_across_the_indexed_calls(monkeypatch):
    for k_, v in S.W2.items():
        monkeypatch.setenv(k_, v)
    B = 6
    pat, d = S._data("MPC02", B)
    assert np.array_equal(d["Gpr"], np.broadcast_to(d["Gpr"][0], d["Gpr"].shape))  # (feasible_batch: the same matrices in every instance)
    g, ref = eicos_amd.BatchSolver(pat, B), eicos_amd.BatchSolver(pat, B)
    dev = R._device_arrays([d[k] for k in KEYS])
    try:
        for s in (g, ref):
            s.update_device(*dev)
            s.set_warm_start(0.1)
            assert s.shared_values()
        pm, om = _maps(pat, d, (g, ref))
        idx = _list(B)
        new = _rows_for(d, idx, seed=33)
        assert np.array_equal(g.solve(), ref.solve())
        x, (y, z, s_) = g.solution(), g.duals()
        kept = [("update_rhs", [new["c"], new["h"], new["b"]]), ("update_param", [P._theta(len(idx), K, seed=1)]),
                ("set_iterate", [_none_if_empty(a) for a in (x[idx] * (1 + 1e-3), y[idx], z[idx] * 1.001, s_[idx] * 1.001)])]
        for kind, arrs in kept:
            getattr(g, kind + "_indexed")(idx, *arrs)
            _call_loop(ref, kind, idx, arrs)
            assert g.shared_values() and ref.shared_values(), kind
            assert np.array_equal(g.solve(), ref.solve()), kind
            S._assert_rows(S._state(g, kkt=True), S._state(ref, kkt=True), range(B), (kind, "shared values kept"))
        # the step over a subset without a matrix map keeps them too
        pth = binding.PinnedArray((len(idx), K))
        pth.a[...] = P._theta(len(idx), K, seed=2)
        _step_and_compare(g, ref, idx, pth.a, "shared values, step over a subset", expect_fused=True)
        assert g.shared_values() and ref.shared_values()
        # the full form drops them, as a sub-range update does
        arrs = [new[k] for k in KEYS]
        g.update_indexed(idx, *arrs)
        _call_loop(ref, "update", idx, arrs)
        assert not g.shared_values() and not ref.shared_values()
        assert np.array_equal(g.solve(), ref.solve())
        S._assert_rows(S._state(g, kkt=True), S._state(ref, kkt=True), range(B), "shared values dropped")
        pth.close()
    finally:
        R._free_device(dev)
        g.close()
        ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,env,build", S.BUILDS)
def test_step_over_a_subset_equals_the_three_calls(name, B, env, build, monkeypatch):
    pat, d, g, ref = S._setup(name, B, env, build, monkeypatch)
    _maps(pat, d, (g, ref))
    lds = g.dims()["lds_bytes"] > 0
    assert lds == (build != "no-lds") or build is None
    L = binding._lib()
    idx = _list(B)
    n = len(idx)
    pth, pu, px = (binding.PinnedArray(s) for s in ((n, K), (n, NR), (n, pat.n)))
    # cold, pinned theta and pinned results: one launch where the handle has an LDS vector
    pth.a[...] = P._theta(n, K, seed=1)
    pu.a[...] = np.nan
    px.a[...] = np.nan
    _step_and_compare(g, ref, idx, pth.a, (name, build, "pinned"), u_out=pu.a, x_out=px.a, expect_fused=lds)
    # on the solved state, another list, pageable results
    idx2 = [1, B - 1, 0] if B > 3 else [1, 0]
    pth2 = binding.PinnedArray((len(idx2), K))
    pth2.a[...] = P._theta(len(idx2), K, seed=2)
    u, x = np.full((len(idx2), NR), np.nan), np.full((len(idx2), pat.n), np.nan)
    _step_and_compare(g, ref, idx2, pth2.a, (name, build, "pageable results"), u_out=u, x_out=x, expect_fused=lds)
    # device theta and device results
    theta = P._theta(n, K, seed=3)
    dev = R._device_arrays((theta, np.full((n, NR), np.nan), np.full((n, pat.n), np.nan)))
    try:
        before = S._state(g, kkt=True)
        codes, ii = np.zeros(n, np.int32), np.asarray(idx, np.int32)
        assert L.eicos_batch_update_param_solve_subset(g._h, ii.ctypes.data_as(IP), n, C.cast(dev[0], DP), C.cast(dev[1], DP), C.cast(dev[2], DP),
                                                       codes.ctypes.data_as(IP)) == 0, L.eicos_last_error()
        assert (g.last_update_path() == FUSED) == lds
        u, x = np.zeros((n, NR)), np.zeros((n, pat.n))
        assert L.hipMemcpy(u.ctypes.data, dev[1], u.nbytes, 2) == 0 and L.hipMemcpy(x.ctypes.data, dev[2], x.nbytes, 2) == 0
        want_codes, want_u, want_x = _three_calls(ref, idx, theta)
        assert np.array_equal(codes, want_codes) and np.array_equal(u, want_u) and np.array_equal(x, want_x), (name, build, "device")
        got = S._state(g, kkt=True)
        S._assert_rows(got, S._state(ref, kkt=True), idx, (name, build, "device, listed rows"))
        S._assert_rows(got, before, _rest(B, idx), (name, build, "device, rows outside the list"))
    finally:
        R._free_device(dev)
    # pageable theta: the three calls
    u = np.full((n, NR), np.nan)
    _step_and_compare(g, ref, idx, P._theta(n, K, seed=4), (name, build, "pageable theta"), u_out=u, x_out=px.a, expect_fused=False)
    assert g.last_update_path() == "pinned bounce"
    # the fused path switched off
    monkeypatch.setenv("EICOS_FUSED_UPDATE", "0")
    pth.a[...] = P._theta(n, K, seed=5)
    _step_and_compare(g, ref, idx, pth.a, (name, build, "EICOS_FUSED_UPDATE=0"), u_out=pu.a, x_out=px.a, expect_fused=False)
    monkeypatch.delenv("EICOS_FUSED_UPDATE")
    # the identity list is the whole-batch step
    pall, uall = binding.PinnedArray((B, K)), binding.PinnedArray((B, NR))
    pall.a[...] = P._theta(B, K, seed=6)
    u_ref = np.zeros((B, NR))
    codes = g.update_param_solve_subset(list(range(B)), pall.a, u_out=uall.a)
    assert (g.last_update_path() == FUSED) == lds
    assert np.array_equal(codes, ref.update_param_solve(pall.a.copy(), u_out=u_ref)) and np.array_equal(uall.a, u_ref)
    S._assert_rows(S._state(g, kkt=True), S._state(ref, kkt=True), range(B), (name, build, "identity list"))
    for a in (pth, pu, px, pth2, pall, uall):
        a.close()
    g.close()
    ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["warm + shift map", "matrix map"])
def test_step_over_a_subset_warm_shifted_and_under_a_matrix_map(case, monkeypatch):
    name, B, env, build = S.BUILDS[1]
    B = 6
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    pat, d = S._data(name, B)
    g, ref = eicos_amd.BatchSolver(pat, B), eicos_amd.BatchSolver(pat, B)
    dev = R._device_arrays([d[k] for k in KEYS])
    try:
        for s in (g, ref):
            s.update_device(*dev)  # (the detecting update: shared matrix values)
            s.set_warm_start(0.1)
        _maps(pat, d, (g, ref))
        if case == "matrix map":
            mm = _mmap(d, K, "GA")
            for s in (g, ref):
                s.set_matrix_map(mm)
        else:
            ident = (np.full(pat.n, 1e-3), np.arange(pat.n + 1, dtype=np.int32), np.arange(pat.n, dtype=np.int32), np.ones(pat.n))
            smap = ShiftMap(pat.n, pat.p, pat.m, x=ident)
            for s in (g, ref):
                s.set_shift_map(smap)
        assert np.array_equal(g.solve(), ref.solve()) and g.shared_values()
        idx = [4, 0, B - 1, 2]
        pth, pu = binding.PinnedArray((len(idx), K)), binding.PinnedArray((len(idx), NR))
        for step in range(2):  # (the second step warm-starts from the first)
            pth.a[...] = P._theta(len(idx), K, seed=40 + step)
            _step_and_compare(g, ref, idx, pth.a, (case, step), u_out=pu.a, expect_fused=True)
            assert g.shared_values() == ref.shared_values() == (case != "matrix map"), (case, step)
        assert np.array_equal(g.solve(), ref.solve())
        S._assert_rows(S._state(g, kkt=True), S._state(ref, kkt=True), range(B), (case, "a whole-batch solve afterwards"))
        pth.close()
        pu.close()
    finally:
        R._free_device(dev)
        g.close()
        ref.close()


@pytest.mark.gpu
def test_step_over_more_instances_than_cus_keeps_rows_in_list_order(monkeypatch):
    """More chosen instances than CUs: the selection kernel permutes the launch order (longest first) while theta, u and x stay in list
    order -- a row map indexed by launch position instead of by id would hand instances each other's rows."""
    B = 1200
    pat, d = S._data("lp_afiro", B)
    A, Bh = (S._handle(pat, d, B) for _ in range(2))
    _maps(pat, d, (A, Bh))
    idx = np.random.default_rng(3).permutation(B)[:700]
    c2, h2, b2 = S._perturbed(d, seed=5)
    for g in (A, Bh):
        g.set_warm_start(0.1)
        g.solve()  # (the previous solve's work is the sort key)
        g.update_rhs(c2, h2, b2 if pat.p else None)
    pth, pu, px = (binding.PinnedArray(s) for s in ((idx.size, K), (idx.size, NR), (idx.size, pat.n)))
    pth.a[...] = P._theta(idx.size, K, seed=8)
    _step_and_compare(Bh, A, idx, pth.a, "700 of 1200", kkt=False, u_out=pu.a, x_out=px.a, expect_fused=True)
    assert len(set(A.info_arrays()["n_ldlsolve"][idx])) > 1  # (several keys: the sort has something to do)
    assert not np.array_equal(pu.a[0], pu.a[1])              # (rows that differ: a permutation would show)
    for a in (pth, pu, px):
        a.close()
    A.close()
    Bh.close()


@pytest.mark.gpu
def test_refusals_and_empty_lists(monkeypatch):
    name, B, env, build = S.BUILDS[0]
    pat, d, g = S._setup(name, B, env, build, monkeypatch, handles=1)
    g.solve_subset([0, 1, 2, 3])
    row = lambda w, n=2: np.zeros((n, w))  # noqa: E731
    L = binding._lib()

    def snapshot():
        return S._state(g, kkt=True), g.last_solve_ms(), g.ms_history("solve"), g.ms_history("update"), g.last_update_path()

    def unchanged(snap, what):
        S._assert_rows(S._state(g, kkt=True), snap[0], range(B), what)
        assert (g.last_solve_ms(), g.ms_history("solve"), g.ms_history("update"), g.last_update_path()) == snap[1:], what

    snap = snapshot()
    no_maps = [
        (lambda: g.update_param_indexed([0, 1], row(K)), "no parameter map"),
        (lambda: g.update_param_solve_subset([0, 1], row(K)), "no parameter map"),
        (lambda: g.outputs_indexed([0, 1]), "no output map"),
    ]
    for call, msg in no_maps:
        with pytest.raises(RuntimeError, match=msg):
            call()
        unchanged(snap, msg)
    g.set_param_map(P._map(d, K))
    two = np.array([0, 1], np.int32)  # u_out without an output map
    assert L.eicos_batch_update_param_solve_subset(g._h, binding._ip(two), 2, binding._dp(row(K)), binding._dp(row(NR)), None, None) == -1 \
        and b"no output map" in L.eicos_last_error()
    unchanged(snap, "u_out without an output map")
    g.set_output_map(_omap(pat.n, NR))
    lists = [([1, 5, 1], "duplicate index 1", 3), ([0, B], f"index {B} at position 1", 2), ([-1], "index -1 at position 0", 1),
             (list(range(B)) + [0], f"count {B + 1}", B + 1)]
    for lst, msg, n in lists:
        calls = [
            lambda: g.update_indexed(lst, c=row(pat.n, n)), lambda: g.update_rhs_indexed(lst, c=row(pat.n, n)),
            lambda: g.update_param_indexed(lst, row(K, n)), lambda: g.set_iterate_indexed(lst, x=row(pat.n, n)),
            lambda: g.update_rhs_indexed_device(lst, 0, 0, 0), lambda: g.outputs_indexed(lst), lambda: g.outputs_indexed_device(lst, 0),
            lambda: g.update_param_solve_subset(lst, row(K, n)),
        ]
        for k, call in enumerate(calls):
            with pytest.raises(RuntimeError, match=msg):
                call()
            unchanged(snap, (msg, k))
    # NULL idx with count > 0, and the namesakes' own refusals
    assert L.eicos_batch_update_rhs_indexed(g._h, None, 2, binding._dp(row(pat.n)), None, None) == -1 and b"idx is NULL" in L.eicos_last_error()
    assert L.eicos_batch_update_param_solve_subset(g._h, None, 2, binding._dp(row(K)), None, None, None) == -1 and b"idx is NULL" in L.eicos_last_error()
    assert L.eicos_batch_update_param_indexed(g._h, binding._ip(two), 2, None) == -1 and b"theta is NULL" in L.eicos_last_error()
    assert L.eicos_batch_update_indexed(g._h, binding._ip(two), 2, binding._dp(row(pat.nnzG)), None, None, None, None) == -1 \
        and b"Gpr given without h" in L.eicos_last_error()
    assert L.eicos_batch_outputs_indexed(g._h, binding._ip(two), 2, None) == -1 and b"u is NULL" in L.eicos_last_error()
    unchanged(snap, "NULL arguments")
    # empty lists: EICOS_OK, nothing enqueued, nothing recorded
    g.update_indexed([], c=row(pat.n, 0))
    g.update_rhs_indexed([], c=row(pat.n, 0))
    g.update_param_indexed([], row(K, 0))
    g.set_iterate_indexed([], x=row(pat.n, 0))
    g.update_param_indexed_device([], 0)
    assert g.outputs_indexed([]).shape == (0, NR)
    assert g.update_param_solve_subset([], row(K, 0)).size == 0
    unchanged(snap, "empty lists")
    g.close()


@pytest.mark.gpu
def test_multi_matches_the_single_handle(monkeypatch):
    for k_, v in S.W2.items():
        monkeypatch.setenv(k_, v)
    B = 5
    pat, d = S._data("MPC02", B)
    eicos_amd.set_arithmetic_profile(1)  # (plans by the pattern alone: a shard of 3 or 2 gives the bits of the batch of 5)
    try:
        one = eicos_amd.BatchSolver(pat, B)
        multi = eicos_amd.MultiBatchSolver(pat, B, [0, 0])
    finally:
        eicos_amd.set_arithmetic_profile(0)
    assert [(f, c) for f, c, _ in multi.shards()] == [(0, 3), (3, 2)]
    for g in (one, multi):
        g.update(*[d[k] for k in KEYS])
        g.set_warm_start(0.1)
    _maps(pat, d, (one, multi))
    assert np.array_equal(multi.solve(), one.solve())
    for step, idx in enumerate(([4, 0, 2], [1, 0])):  # both shards; the first shard only
        new = _rows_for(d, idx, seed=50 + step)
        x, (y, z, s_) = one.solution(), one.duals()
        calls = [("update_indexed", [new[k] for k in KEYS]), ("update_rhs_indexed", [new["c"] * 1.01, new["h"], new["b"]]),
                 ("update_param_indexed", [P._theta(len(idx), K, seed=step)]),
                 ("set_iterate_indexed", [_none_if_empty(a) for a in (x[idx] * (1 + 1e-3), y[idx], z[idx] * 1.001, s_[idx] * 1.001)])]
        for kind, arrs in calls:
            for g in (one, multi):
                getattr(g, kind)(idx, *arrs)
            S._assert_rows(S._state(multi), S._state(one), range(B), ("multi", kind, idx, "before the solve"))
            assert np.array_equal(multi.solve(), one.solve()), (kind, idx)
            S._assert_rows(S._state(multi), S._state(one), range(B), ("multi", kind, idx))
            assert np.array_equal(multi.outputs_indexed(idx), one.outputs_indexed(idx)), (kind, idx)
        theta = P._theta(len(idx), K, seed=10 + step)
        um, u1 = np.full((len(idx), NR), np.nan), np.full((len(idx), NR), np.nan)
        xm, x1 = np.full((len(idx), pat.n), np.nan), np.full((len(idx), pat.n), np.nan)
        assert np.array_equal(multi.update_param_solve_subset(idx, theta, u_out=um, x_out=xm), one.update_param_solve_subset(idx, theta, u_out=u1, x_out=x1))
        assert np.array_equal(um, u1) and np.array_equal(xm, x1), idx
        S._assert_rows(S._state(multi), S._state(one), range(B), ("multi step over a subset", idx))
    before = S._state(multi)
    for call, msg in ((lambda: multi.update_rhs_indexed([3, 0, 3], c=np.zeros((3, pat.n))), "duplicate index 3"),
                      (lambda: multi.update_param_solve_subset([B], np.zeros((1, K))), f"index {B} at position 0"),
                      (lambda: multi.update_indexed([0, -2], c=np.zeros((2, pat.n))), "index -2 at position 1")):
        with pytest.raises(RuntimeError, match=msg):
            call()
    S._assert_rows(S._state(multi), before, range(B), "a refused list changes no shard")
    one.close()
    multi.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,env,build", [S.BUILDS[0], S.BUILDS[1], S.BUILDS[7]])
def test_outputs_indexed_returns_rows_of_outputs(name, B, env, build, monkeypatch):
    pat, d, g = S._setup(name, B, env, build, monkeypatch, handles=1)
    g.set_output_map(_omap(pat.n, NR))
    g.solve_subset([1, B - 1])  # (solved and fresh instances side by side)
    full = g.outputs()
    for idx in ([B - 1, 0, 2], list(range(B))[::-1], [1]):
        assert np.array_equal(g.outputs_indexed(idx), full[idx], equal_nan=True), (name, idx)
        dev = R._device_arrays((np.full((len(idx), NR), np.nan),))
        try:
            g.outputs_indexed_device(idx, dev[0])
            g.sync()
            u = np.zeros((len(idx), NR))
            assert binding._lib().hipMemcpy(u.ctypes.data, dev[0], u.nbytes, 2) == 0
            assert np.array_equal(u, full[idx], equal_nan=True), (name, idx, "device")
        finally:
            R._free_device(dev)
    g.close()
