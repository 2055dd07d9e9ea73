"""The buffers a handle grows on demand (eicos_amd/csrc/resources.hpp: Buffer::reserve, PinnedSlot) on the GPU: a handle that made a
small call first -- and so had to replace its buffer for the large one -- ends bit for bit where a fresh handle ends that made only the
large call, and stays usable.  One case per grow site, map replacement, and destruction of a handle on which every such buffer exists.
Every comparison is np.array_equal on x, y, z, s, the exit codes and the iteration counts."""
import numpy as np
import pytest

import eicos_amd
import test_matrix_param as M  # (its _mmap)
import test_param_update as P  # (its _data, _map, _theta, _twins)
import test_rhs_update as R    # (its _second_rhs)
import test_rollout as RO      # (its _fmap)
from test_param_step import _omap
from test_rollout_data_gradient import _wanted

B = 8
KEYS = R.KEYS
_CASE = []


def _case():
    """lp_afiro, a batch of eight: the pattern and the data, generated once."""
    if not _CASE:
        _CASE.append(P._data("lp_afiro", B))
    return _CASE[0]


def _state(g, codes):
    x = g.solution(); y, z, s = g.duals(); ia = g.info_arrays()
    return [np.asarray(codes).copy(), x, y, z, s, ia["exitcode"], ia["iter"]]


def _assert_same(a, b, what):
    for k, (u, v) in enumerate(zip(a, b)):
        assert np.array_equal(u, v, equal_nan=True), (what, k)


def _still_usable(g, ref, what):
    """one more plain solve on both"""
    _assert_same(_state(g, g.solve()), _state(ref, ref.solve()), (what, "plain solve afterwards"))
    g.close(); ref.close()


@pytest.mark.gpu
def test_bounce_buffers_grow_between_two_updates():
    """Two FRESH handles (a pageable update of the whole batch, as in _twins, would size the buffers for good): the first host-pointer
    call g ever makes is the one over two instances, so its bounce buffers are allocated for a chunk of two; the call over eight needs a
    chunk four times as large (staging grows with the count: a chunk is the whole call below 16 instances) and replaces both buffers
    while the event of the small call's kernel is what PinnedSlot::reserve has to wait for.  ref allocates for eight at once."""
    pat, d = _case()
    g, ref = eicos_amd.BatchSolver(pat, B), eicos_amd.BatchSolver(pat, B)
    rows = [d[k] for k in KEYS]
    assert g.last_update_path() == "none"  # nothing has come through the bounce buffers: there are none yet
    g.update(*[a[:2] for a in rows], count=2)
    assert g.last_update_path() == "pinned bounce"
    g.update(*rows, count=B)
    ref.update(*rows, count=B)
    assert g.last_update_path() == ref.last_update_path() == "pinned bounce"
    _assert_same(_state(g, g.solve()), _state(ref, ref.solve()), "bounce")
    assert np.array_equal(g.solution(), ref.solution())
    c2, h2, b2 = R._second_rhs(d)  # ... and once more through the grown buffers, a small call last
    for s in (g, ref):
        s.update(d["Gpr"] * 1.001, d["Apr"], c2, h2, b2, count=B)
        s.update_rhs(d["c"][:3], d["h"][:3], d["b"][:3], count=3)
    _assert_same(_state(g, g.solve()), _state(ref, ref.solve()), "bounce, second round")
    _still_usable(g, ref, "bounce")


@pytest.mark.gpu
def test_gather_buffer_grows_between_two_gathers():
    pat, d = _case()
    g, ref = P._twins(pat, d, B)
    x = g.solution(); y, z, s = g.duals(); ia = g.info_arrays()
    for ids in ([3], list(range(B))):
        got = g.gather(ids)
        for name, rows in zip("xyzs", (x, y, z, s)):
            assert np.array_equal(got[name], rows[ids]), (ids, name)
        for k in ia:
            assert np.array_equal(got["info"][k], ia[k][ids], equal_nan=True), (ids, k)
    want = ref.gather(list(range(B)))
    for name in "xyzs":
        assert np.array_equal(got[name], want[name]), name
    for k in R.INFO_KEYS:  # (every field but the measured solve time)
        assert np.array_equal(got["info"][k], want["info"][k], equal_nan=True), k
    _still_usable(g, ref, "gather")


def _closed_loop_maps(pat, d, k=3, r=2):
    return P._map(d, k), _omap(pat.n, r), RO._fmap(k, r)


@pytest.mark.gpu
def test_rollout_buffer_grows_between_two_rollouts():
    pat, d = _case()
    g, ref = P._twins(pat, d, B)
    pm, om, fm = _closed_loop_maps(pat, d)
    for s in (g, ref):
        s.set_param_map(pm); s.set_output_map(om); s.set_plant_map(fm)
    theta0 = P._theta(B, pm.k)
    short = g.rollout(theta0, 1)
    got, want = g.rollout(theta0, 3), ref.rollout(theta0, 3)
    _assert_same(got, want, "rollout")  # u_traj, theta_traj, exit codes, iterations
    _assert_same([a[:, :1] for a in (short[0], short[2], short[3])], [a[:, :1] for a in (want[0], want[2], want[3])], "first step")
    _assert_same(_state(g, got[2][:, -1]), _state(ref, want[2][:, -1]), "rollout: final state")
    _still_usable(g, ref, "rollout")


@pytest.mark.gpu
def test_adjoint_staging_grows_between_two_adjoint_calls():
    """d_adj: one right-hand side for instance 3 alone, then two for every instance of the batch."""
    pat, d = _case()
    g, ref = P._twins(pat, d, B)
    rhs = np.random.default_rng(5).standard_normal((B, 2, pat.n))
    small = g.adjoint_data(rhs[[3], :1], idx=[3])
    got, want = g.adjoint_data(rhs), ref.adjoint_data(rhs)
    _assert_same(got, want, "adjoint")  # grad_c, grad_h, grad_b, grad_G, grad_A, res
    _assert_same(small, ref.adjoint_data(rhs[[3], :1], idx=[3]), "adjoint: the small call, in the grown buffer")
    _still_usable(g, ref, "adjoint")


def _recording_twins():
    """Two solved handles under the closed-loop maps with recording on, and theta0."""
    pat, d = _case()
    g, ref = P._twins(pat, d, B)
    pm, om, fm = _closed_loop_maps(pat, d)
    for s in (g, ref):
        s.set_param_map(pm); s.set_output_map(om); s.set_plant_map(fm); s.set_rollout_recording(True)
    return g, ref, P._theta(B, pm.k), pm


@pytest.mark.gpu
@pytest.mark.parametrize("fused", ["1", "0"])
def test_jacobian_trajectory_and_record_grow_between_two_recording_rollouts(fused, monkeypatch):
    """d_rollJ and d_rollW: one step, then three.  Not fused, both also hold one step's rows behind the trajectories."""
    monkeypatch.setenv("EICOS_FUSED_UPDATE", fused)
    g, ref, theta0, _ = _recording_twins()
    short = list(g.rollout_jacobian(theta0, 1)) + list(g.rollout_records())
    got, want = list(g.rollout_jacobian(theta0, 3)), list(ref.rollout_jacobian(theta0, 3))
    got += g.rollout_records(); want += ref.rollout_records()
    assert g.last_rollout_launches() == ref.last_rollout_launches() and (fused == "1" or g.last_rollout_launches() == 3)
    _assert_same(got, want, "recording rollout")  # u, theta, codes, iters, J, res, Wc, Wh, Wb, x, y, z
    first = [q for q in range(len(want)) if q != 1]  # (theta has a row more than steps)
    _assert_same([short[q][:, :1] for q in first], [want[q][:, :1] for q in first], "first step")
    _assert_same([short[1][:, :2]], [want[1][:, :2]], "first step: theta")
    _still_usable(g, ref, "recording rollout")


def _sweeps_after_each_rollout(sweep, what):
    """g: a recording rollout of one step and the sweep over it, then the same over three steps; ref: the three steps alone."""
    g, ref, theta0, pm = _recording_twins()

    def run(s, steps):
        out = s.rollout_jacobian(theta0, steps)
        rng = np.random.default_rng(7)
        return list(sweep(s, pm, out[0], out[1], rng.standard_normal(out[0].shape), rng.standard_normal(out[1].shape)))

    run(g, 1)
    _assert_same(run(g, 3), run(ref, 3), what)
    _still_usable(g, ref, what)


@pytest.mark.gpu
def test_gradient_staging_grows_between_two_rollout_gradients():
    """d_rollG, through both of its calls."""
    _sweeps_after_each_rollout(lambda s, pm, u, th, gu, gth: s.rollout_gradient(gu, gth) + s.rollout_plant_gradient(u, th, gu, gth), "rollout gradient")


@pytest.mark.gpu
def test_data_gradient_staging_grows_between_two_data_gradients():
    """d_rollD: every output the maps allow."""
    _sweeps_after_each_rollout(lambda s, pm, u, th, gu, gth: s.rollout_data_gradient(th, gu, gth, want=_wanted(pm)).values(), "data gradient")


@pytest.mark.gpu
def test_matrix_staging_buffer_grows_between_two_param_updates(monkeypatch):
    monkeypatch.setenv("EICOS_MATRIX_STAGE_MB", "1")  # (conftest.py sets EICOS_EXPERIMENT=1; as tests/test_matrix_param.py sets the knob)
    pat, d = _case()
    g, ref = P._twins(pat, d, B)
    pm, mm = P._map(d, 3), M._mmap(d, 3)
    for s in (g, ref):
        s.set_param_map(pm); s.set_matrix_map(mm)
    theta = P._theta(B, 3)
    g.update_param(theta[:2], count=2)
    g.update_param(theta, count=B)
    ref.update_param(theta, count=B)
    assert np.array_equal(g.debug_kkt(B - 1)[2], ref.debug_kkt(B - 1)[2], equal_nan=True)
    _assert_same(_state(g, g.solve()), _state(ref, ref.solve()), "matrix staging")
    _still_usable(g, ref, "matrix staging")


@pytest.mark.gpu
def test_subset_list_buffer_is_reused_between_two_subset_solves():
    pat, d = _case()
    g, ref = P._twins(pat, d, B)
    c2, h2, b2 = R._second_rhs(d)
    for s in (g, ref):
        s.update_rhs(c2, h2, b2)  # (so that a subset solve moves its instances and nobody else)
    rows = [0, 7, 2]
    g.solve_subset([5])
    got, want = g.solve_subset(rows), ref.solve_subset(rows)
    # (instance 5 is solved on g alone: the rows of the large call are what the two handles share until the plain solve below)
    _assert_same([got] + [a[rows] for a in _state(g, got)[1:]], [want] + [a[rows] for a in _state(ref, want)[1:]], "subset")
    _still_usable(g, ref, "subset")


@pytest.mark.gpu
def test_a_replaced_and_a_removed_map_leave_the_state_of_the_final_one():
    pat, d = _case()
    g, ref = P._twins(pat, d, B)
    first, final = P._map(d, 2), P._map(d, 5, seed=1)
    g.set_param_map(first)
    g.update_param(P._theta(B, 2))
    g.solve()
    g.set_param_map(final)
    ref.set_param_map(final)
    assert g.param_count() == ref.param_count() == 5
    theta = P._theta(B, 5, seed=1)
    g.update_param(theta); ref.update_param(theta)
    _assert_same(_state(g, g.solve()), _state(ref, ref.solve()), "replaced map")
    g.set_param_map(None)
    assert g.param_count() == 0
    with pytest.raises(RuntimeError, match="no parameter map"):
        g.update_param(theta)
    _still_usable(g, ref, "removed map")  # (a plain solve reads no map: the handle without one equals the handle that keeps the final one)


@pytest.mark.gpu
def test_destroying_a_handle_with_every_optional_buffer_leaves_the_device_usable(monkeypatch):
    monkeypatch.setenv("EICOS_MATRIX_STAGE_MB", "1")
    pat, d = _case()
    g, ref = P._twins(pat, d, B)
    want = _state(ref, ref.solve())
    pm, om, fm = _closed_loop_maps(pat, d)
    g.gather([1, 2])                                         # gather buffer (and the bounce buffers: _twins updated from pageable arrays)
    g.solve_subset([4])                                      # subset list buffer
    monkeypatch.setenv("EICOS_FUSED_STAGED", "1")
    g.update_solve(*[d[k] for k in KEYS])                    # pinned staging buffer, ready flags and error word of the staged fused update
    assert g.last_update_path() == "fused into the solve, staged while it runs"
    monkeypatch.delenv("EICOS_FUSED_STAGED")
    g.set_param_map(pm); g.set_output_map(om); g.set_plant_map(fm)
    g.rollout(P._theta(B, pm.k), 2)                          # rollout buffer, behind three maps
    g.adjoint_data(np.ones((B, 1, pat.n)))                   # adjoint staging
    g.set_rollout_recording(True)
    out = g.rollout_jacobian(P._theta(B, pm.k), 2)           # Jacobian trajectory and record
    g.rollout_gradient(gu=np.ones_like(out[0]))              # gradient staging
    g.rollout_plant_gradient(out[0], out[1], gu=np.ones_like(out[0]))
    g.rollout_data_gradient(out[1], gu=np.ones_like(out[0]), want=_wanted(pm))  # data-gradient staging
    g.set_matrix_map(M._mmap(d, pm.k))
    g.update_param(P._theta(B, pm.k))                        # matrix staging buffer
    g.close()
    again = eicos_amd.BatchSolver(pat, B)  # (the descriptor slot g held is free again: the lowest free one is handed out)
    again.update(*[d[k] for k in KEYS])
    _assert_same(_state(again, again.solve()), want, "after destroy")
    again.close(); ref.close()
