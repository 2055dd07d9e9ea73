"""Fused and plain launches interleaved on one handle: no step record outlives the call that made it.

A step fused into the solve launch (update_solve, update_rhs_solve, update_param_solve, rollout) hands the launch a record of input and
output arrays.  The record belongs to that one call: the plain solve() behind it must launch as if the call had never been, and a call
that is refused must leave nothing behind either.  Handle `g` alternates every fused call with a plain solve, its inputs in pinned
arrays that are filled with NaN between the two -- a launch that still carried the record would read the NaN rows, or write into the
pinned result arrays, and both show.  Handle `ref` does the same work with the separate calls only (update / update_rhs / update_param,
solve, outputs; for the rollout the host loop over parametric steps of test_rollout.py, in separate calls as well).  After every step the
exit codes, the iteration counts, x, the duals and u of the two are equal bit for bit: the refactored launch adds no arithmetic freedom."""
import ctypes as C

import numpy as np
import pytest

import eicos_amd
from eicos_amd import binding
import test_param_update as P  # (its _data, _map, _theta, _twins)
import test_rhs_update as R    # (its _outputs, _assert_same, _second_rhs)
from test_param_step import _omap
from test_rollout import _fmap, _w

KEYS = R.KEYS
DP = C.POINTER(C.c_double)
FUSED = "fused into the solve"


def _same_state(g, ref, codes_g, codes_ref, what):
    R._assert_same(R._outputs(g, codes_g), R._outputs(ref, codes_ref), what)  # exit codes, x, y, z, s, iterations and the other counters
    ug, ur = g.outputs(), ref.outputs()
    assert ug.shape == ur.shape and np.array_equal(ug, ur, equal_nan=True), (what, "u")


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,env,build", [
    ("MPC02", 4, {"EICOS_UBL": "0", "EICOS_THREADS": "256"}, ("w2", 256)),  # the two-wave build
    ("lp_afiro", 4, {}, ("lds-resident", 128)),                              # the LDS-resident build
    ("issue98", 4, {"EICOS_THREADS": "256"}, ("u-in-lds", 256)),             # cones, U in LDS
])
def test_fused_and_plain_launches_interleaved_on_one_handle(name, B, env, build, monkeypatch):
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    k, r, T = 5, 4, 2
    pat, d = P._data(name, B)
    pm, om, fm = P._map(d, k), _omap(pat.n, r), _fmap(k, r)
    g, ref = P._twins(pat, d, B)
    assert g.dims() == ref.dims() and (g.kernel_build(), g.dims()["threads_per_block"]) == build
    for s in (g, ref):
        s.set_param_map(pm); s.set_output_map(om)
    g.set_plant_map(fm)
    L = binding._lib()

    pins = {key: eicos_amd.PinnedArray(d[key].shape) for key in KEYS}
    pth, pu, px = (eicos_amd.PinnedArray(s) for s in ((B, k), (B, r), (B, pat.n)))
    inputs = [pins[key] for key in KEYS] + [pth]
    results = [pu, px]

    def plain_solve(what):
        """The pinned inputs turn to NaN, then both handles take a plain solve: equal state, and nothing written into the result arrays."""
        for p_ in inputs + results:
            p_.a[...] = np.nan
        codes_g, codes_ref = g.solve(), ref.solve()
        _same_state(g, ref, codes_g, codes_ref, (name, "solve after", what))
        for p_ in results:
            assert np.isnan(p_.a).all(), (name, "a plain solve wrote a result array of", what)

    # 1. update_solve
    c2, h2, b2 = R._second_rhs(d)
    full = dict(Gpr=d["Gpr"], Apr=d["Apr"], c=c2, h=h2, b=b2)
    for key in KEYS:
        pins[key].a[...] = full[key]
    px.a[...] = np.nan
    codes = g.update_solve(*[pins[key].a for key in KEYS], x_out=px.a)
    assert g.last_update_path() == FUSED
    ref.update(*[full[key] for key in KEYS])
    _same_state(g, ref, codes, ref.solve(), (name, "update_solve"))
    assert np.array_equal(px.a, ref.solution())
    # 2.
    plain_solve("update_solve")

    # 3. update_rhs_solve
    c3, h3, b3 = c2 * 0.995, h2 + 0.02 * np.abs(h2), b2 * (1.0 - 2e-3)
    for key, v in zip(("c", "h", "b"), (c3, h3, b3)):
        pins[key].a[...] = v
    px.a[...] = np.nan
    codes = g.update_rhs_solve(pins["c"].a, pins["h"].a, pins["b"].a, x_out=px.a)
    assert g.last_update_path() == FUSED
    ref.update_rhs(c3, h3, b3)
    _same_state(g, ref, codes, ref.solve(), (name, "update_rhs_solve"))
    assert np.array_equal(px.a, ref.solution())
    # 4.
    plain_solve("update_rhs_solve")

    # 5. update_param_solve with u_out
    theta = P._theta(B, k, seed=7)
    pth.a[...] = theta
    pu.a[...] = np.nan; px.a[...] = np.nan
    codes = g.update_param_solve(pth.a, u_out=pu.a, x_out=px.a)
    assert g.last_update_path() == FUSED
    ref.update_param(theta)
    _same_state(g, ref, codes, ref.solve(), (name, "update_param_solve"))
    assert np.array_equal(pu.a, ref.outputs()) and np.array_equal(px.a, ref.solution())
    # 6.
    plain_solve("update_param_solve")

    # 7. rollout(steps = 2), theta0 pinned; the reference: the host loop, every step in separate calls
    theta0, w = P._theta(B, k, seed=8), _w(B, T, k)
    pth.a[...] = theta0
    u_traj, th_traj, codes_traj, iters_traj = g.rollout(pth.a, T, w)
    assert g.last_update_path() == FUSED and g.last_rollout_launches() == 1
    th = theta0.copy()
    for t in range(T):
        assert np.array_equal(th_traj[:, t], th), (name, "rollout theta", t)
        ref.update_param(th)
        codes_ref = ref.solve()
        u = ref.outputs()
        assert np.array_equal(codes_traj[:, t], codes_ref) and np.array_equal(iters_traj[:, t], ref.info_arrays()["iter"]), (name, "rollout", t)
        assert np.array_equal(u_traj[:, t], u), (name, "rollout u", t)
        th = fm.evaluate(th, u, w[:, t])
    assert np.array_equal(th_traj[:, T], th)
    _same_state(g, ref, codes_traj[:, -1], codes_ref, (name, "rollout"))
    # 8.
    plain_solve("rollout")

    # 9. refused calls: by the binding (theta rows of the wrong width) and by the library (a step without theta, a rollout of no steps)
    pth.a[...] = P._theta(B, k, seed=9)
    with pytest.raises(ValueError):
        g.update_param_solve(np.zeros((B, k + 1)), u_out=pu.a)
    assert L.eicos_batch_update_param_solve(g._h, None, pu.a.ctypes.data_as(DP), px.a.ctypes.data_as(DP), None) == -1
    assert b"theta is NULL" in L.eicos_last_error()
    assert L.eicos_batch_rollout(g._h, 0, pth.a.ctypes.data_as(DP), None, pu.a.ctypes.data_as(DP), None, None, None) == -1
    assert b"steps" in L.eicos_last_error()
    # 10.
    plain_solve("a refused call")

    g.close(); ref.close()
    for p_ in inputs + results:
        p_.close()
