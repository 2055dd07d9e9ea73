"""The retry policy: a second attempt inside the solve launch (eicos_retry, eicos_batch_set_retry / _get_retry / _retry_counts and
their eicos_multi_* forms, include/eicos_amd.h).

With a policy on the handle, a workgroup whose instance ends in an exit class of the policy's mask solves the same instance once more,
under the policy's settings, before anything reads the result.  The contract is an equality: every instance ends with the bits of the
HOST SEQUENCE on a twin handle -- the same launch without the policy, the ids of the launch whose class is in the mask, the policy's
settings / warm start / dynamic regularisation set, solve_subset(ids), the three settings restored -- and the outputs, x rows and the
plant map of a fused step are taken after it.  Every GPU comparison is np.array_equal.

The inputs and iteration caps are chosen from the CPU oracle's iteration counts (an instance that converges in k passes gets through a
cap c iff k <= c: the exit test stands in front of the cap test), so that in every case but the cone pattern some instances retry and
some do not; the tests assert that, and print the sets.  The CPU tests check the defaults, the struct mirror and the refusals that need
no GPU."""
import ctypes as C

import numpy as np
import pytest

import eicos_amd
from eicos_amd import binding
from eicos_amd.binding import ShiftMap
import test_param_update as P  # (its _map, _theta)
import test_rollout as RO      # (its _fmap, _w)
from test_param_step import _omap
from test_solve_subset import BUILDS, KEYS, W2, _assert_rows, _classes, _data, _handle, _perturbed, _setup, _state

NOT_OPTIMAL = eicos_amd.SEL_NOT_OPTIMAL
# case 1: per pattern the batch, the iteration cap of the first attempt and whether the right-hand sides are the perturbed ones
CASES = {"lp_afiro": (8, 9, False), "MPC02": (8, 14, True), "issue98": (4, 7, False), "socp-random": (8, 4, False)}


# ---- helpers ----------------------------------------------------------------------------------------------------------------------
def _policy(mask=NOT_OPTIMAL, warm=0.0, dyn=(0.0, 0.0), **fields):
    return {"mask": mask, "warm": warm, "dyn": dyn, "fields": fields}


def _install(g, pol):
    g.set_retry(pol["mask"], warm=pol["warm"], dyn=pol["dyn"], **pol["fields"])


def _apply(g, settings, warm, dyn):
    g.set_settings(**settings)
    g.set_warm_start(warm)
    g.set_dynamic_regularization(*dyn)


def _host_retry(g, S, pol, launch):
    """Steps 2-5 of the contract on handle g, whose launch over the instances S has just run under `launch` (settings fields over the
    defaults, warm, dyn): returns the retried ids."""
    cls = _classes(g)
    ids = [int(i) for i in S if cls[i] & pol["mask"]]
    _apply(g, {**eicos_amd.default_settings(), **pol["fields"]}, pol["warm"], pol["dyn"])
    g.solve_subset(ids)
    _apply(g, {**eicos_amd.default_settings(), **launch["fields"]}, launch["warm"], launch["dyn"])
    return ids


def _counts_of(ids, B):
    want = np.zeros(B, np.int32)
    want[ids] = 1
    return want


def _case_handles(name, env, build, monkeypatch, handles=2):
    B, cap, perturbed = CASES[name]
    out = _setup(name, B, env, build, monkeypatch, handles=handles)
    pat, d = out[:2]
    if perturbed:
        c2, h2, b2 = _perturbed(d)
        for g in out[2:]:
            g.update_rhs(c2, h2, b2 if pat.p else None)
    return (B, cap) + out


# ---- CPU --------------------------------------------------------------------------------------------------------------------------
def test_retry_default_and_struct_mirror_need_no_gpu():
    L = binding._lib()
    r = binding.Retry()
    r.mask, r.warm, r.dyn_delta, r.dyn_eps = 77, 3.0, 4.0, 5.0
    L.eicos_retry_default(C.byref(r))
    assert (r.mask, r.warm, r.dyn_delta, r.dyn_eps) == (0, 0.0, 0.0, 0.0)
    assert r.settings.asdict() == eicos_amd.default_settings()
    assert L.eicos_retry_size() == C.sizeof(binding.Retry)
    assert binding.default_retry() == {"mask": 0, "warm": 0.0, "dyn": (0.0, 0.0), "settings": eicos_amd.default_settings()}


def test_retry_entry_points_refuse_a_null_handle():
    L = binding._lib()
    r = binding.Retry()
    L.eicos_retry_default(C.byref(r))
    r.mask = NOT_OPTIMAL
    one = np.zeros(1, np.int32)
    for rc in (L.eicos_batch_set_retry(None, C.byref(r)), L.eicos_batch_get_retry(None, C.byref(r)),
               L.eicos_batch_retry_counts(None, 0, 1, binding._ip(one), 0)):
        assert rc == -1 and b"NULL handle" in L.eicos_last_error()
    for rc in (L.eicos_multi_set_retry(None, C.byref(r)), L.eicos_multi_get_retry(None, C.byref(r)),
               L.eicos_multi_retry_counts(None, 0, 1, binding._ip(one), 0)):
        assert rc == -1 and b"NULL handle" in L.eicos_multi_last_error()


def test_set_retry_refuses_an_unknown_field_before_the_library_is_called():
    class Probe(binding._Solver):  # a solver object whose library call would raise something else
        batch = 1

        def _call(self, name, *args):
            raise AssertionError("the library was called: " + name)

    with pytest.raises(TypeError, match="bogus"):
        Probe().set_retry(bogus=1)
    with pytest.raises(TypeError, match="bogus"):
        Probe().set_retry(NOT_OPTIMAL, warm=0.1, iter_max=50, bogus=1)
    with pytest.raises(AssertionError, match="set_retry"):  # (known fields do reach the library)
        Probe().set_retry(NOT_OPTIMAL, iter_max=50)


# ---- GPU --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,_b,env,build", BUILDS)
def test_inlaunch_retry_equals_the_host_sequence_on_every_build(name, _b, env, build, monkeypatch):
    """Case 1 (capped first attempt, cold retry under the defaults) on the eight handles of the build table.
    The oracle's iteration counts predict the retried sets: MPC02 on the perturbed data under cap 14 {0, 4}, lp_afiro under 9 {5, 7},
    issue98 under 7 all but 2, the cone pattern under 4 all."""
    B, cap, pat, d, A, Bh = _case_handles(name, env, build, monkeypatch)
    launch, pol = _policy(iter_max=cap), _policy()
    for g in (A, Bh):
        g.set_settings(iter_max=cap)
    _install(A, pol)
    codes = A.solve()
    Bh.solve()
    ids = _host_retry(Bh, range(B), pol, launch)
    got, want = _state(A, kkt=True), _state(Bh, kkt=True)
    counts = A.retry_counts()
    print(name, env, "cap", cap, "retried", ids, "iterations", want["info.iter"], "codes", codes)
    _assert_rows(got, want, range(B), (name, env, "in-launch retry against the host sequence"))
    assert np.array_equal(codes, want["info.exitcode"])
    assert counts.dtype == np.int32 and np.array_equal(counts, _counts_of(ids, B)), (counts, ids)
    if name != "socp-random":
        assert 0 < len(ids) < B, (name, ids)  # (a condition of the test: somebody retried and somebody did not)
    assert np.array_equal(A.retry_counts(reset=True), _counts_of(ids, B))
    assert np.array_equal(A.retry_counts(), np.zeros(B, np.int32))
    assert np.array_equal(Bh.retry_counts(), np.zeros(B, np.int32))  # (a handle that never had a policy)
    A.close()
    Bh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [False, True])
def test_warm_first_attempt_cold_retry(shift, monkeypatch):
    """Case 2: MPC02 on the w2 build, solved cold, new right-hand sides, then warm-started under a cap of 10 passes with a cold retry
    under the defaults.  The oracle's warm counts are 10, 11, 8, 12, 10, 8, 10, 9."""
    name, B = "MPC02", 8
    pat, d, A, Bh = _setup(name, B, W2, ("w2", 256), monkeypatch)
    if shift:  # the identity plus a constant offset on x
        ident = (np.full(pat.n, 1e-3), np.arange(pat.n + 1, dtype=np.int32), np.arange(pat.n, dtype=np.int32), np.ones(pat.n))
        smap = ShiftMap(pat.n, pat.p, pat.m, x=ident)
    c2, h2, b2 = _perturbed(d)
    launch, pol = _policy(warm=0.1, iter_max=10), _policy()
    for g in (A, Bh):
        if shift:
            g.set_shift_map(smap)
        assert (g.solve() == 0).all()
        g.update_rhs(c2, h2, b2 if pat.p else None)
        g.set_warm_start(0.1)
        g.set_settings(iter_max=10)
    _install(A, pol)
    codes = A.solve()
    Bh.solve()
    first_iters = Bh.info_arrays()["iter"].copy()
    ids = _host_retry(Bh, range(B), pol, launch)
    want = _state(Bh, kkt=True)
    print(name, "shift", shift, "warm iterations of the first attempt", first_iters, "retried", ids, "final", want["info.iter"])
    _assert_rows(_state(A, kkt=True), want, range(B), (name, shift, "warm first attempt, cold retry"))
    assert np.array_equal(codes, want["info.exitcode"])
    assert np.array_equal(A.retry_counts(), _counts_of(ids, B))
    if not shift:  # (the oracle's counts are those of the unshifted start)
        assert {1, 3} <= set(ids) and not {2, 5} & set(ids), ids
    assert 0 < len(ids) < B, ids
    A.close()
    Bh.close()


@pytest.mark.gpu
def test_policy_with_regularisation_tolerances_and_a_warm_retry(monkeypatch):
    """Case 3: the policy changes the dynamic regularisation and the tolerances and warm-starts the second attempt -- where the capped
    first attempt ended OPTIMAL_INACC its record allows it, where it ended MAXIT the second attempt is cold."""
    name, _b, env, build = BUILDS[0]
    B, cap, pat, d, A, Bh = _case_handles(name, env, build, monkeypatch)
    launch = _policy(iter_max=cap)
    pol = _policy(warm=0.1, dyn=(2e-7, 1e-13), feastol=1e-6, abstol=1e-6, reltol=1e-6)
    for g in (A, Bh):
        g.set_settings(iter_max=cap)
    _install(A, pol)
    codes = A.solve()
    Bh.solve()
    first = Bh.info_arrays()["exitcode"].copy()
    ids = _host_retry(Bh, range(B), pol, launch)
    want = _state(Bh, kkt=True)
    print(name, "first codes", first, "retried", ids, "final codes", want["info.exitcode"], "iterations", want["info.iter"])
    _assert_rows(_state(A, kkt=True), want, range(B), (name, "policy with regularisation and tolerances"))
    assert np.array_equal(codes, want["info.exitcode"]) and np.array_equal(A.retry_counts(), _counts_of(ids, B))
    assert 0 < len(ids) < B, ids
    # the launch's own values are back: the next launch of A, policy removed, is the capped launch of a twin
    A.set_retry(None)
    for g in (A, Bh):
        g.solve()
    _assert_rows(_state(A, kkt=True), _state(Bh, kkt=True), range(B), (name, "the launch after"))
    A.close()
    Bh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,_b,env,build", [BUILDS[0], BUILDS[1]])
def test_subset_launch_under_a_policy(name, _b, env, build, monkeypatch):
    """Case 4, solve_subset: the host sequence restricted to the list; the other rows keep every bit, their counters included."""
    B, cap, pat, d, A, Bh, Ch = _case_handles(name, env, build, monkeypatch, handles=3)
    launch, pol = _policy(iter_max=cap), _policy()
    S = [B - 1, 0, 2]
    rest = [i for i in range(B) if i not in S]
    for g in (A, Bh):
        g.set_settings(iter_max=cap)
    _install(A, pol)
    fresh = _state(Ch, kkt=True)
    codes = A.solve_subset(S)
    Bh.solve_subset(S)
    ids = _host_retry(Bh, S, pol, launch)
    got, want = _state(A, kkt=True), _state(Bh, kkt=True)
    print(name, "list", S, "retried", ids, "codes", codes)
    _assert_rows(got, want, range(B), (name, "subset launch under a policy"))
    _assert_rows(got, fresh, rest, (name, "rows outside the list"))
    assert np.array_equal(codes, want["info.exitcode"][S])
    counts = A.retry_counts()
    assert np.array_equal(counts, _counts_of(ids, B)) and not counts[rest].any()
    assert len(ids) > 0, ids  # (the list holds an instance the cap stops: lp_afiro 7, MPC02 0)
    for g in (A, Bh, Ch):
        g.close()


@pytest.mark.gpu
def test_fused_subset_step_under_a_policy(monkeypatch):
    """Case 4, update_param_solve_subset with pinned theta: update from theta -> solve -> retry -> u and x rows."""
    name, B, K, NR = "MPC02", 8, 7, 6
    pat, d, A, Bh = _setup(name, B, W2, ("w2", 256), monkeypatch)
    pm, om = P._map(d, K), _omap(pat.n, NR)
    idx = [B - 1, 0, 2, 4]
    rest = [i for i in range(B) if i not in idx]
    theta = P._theta(len(idx), K, seed=3)
    launch, pol = _policy(warm=0.1, iter_max=10), _policy()
    for g in (A, Bh):
        g.set_param_map(pm); g.set_output_map(om)
        assert (g.solve() == 0).all()
        g.set_warm_start(0.1)
        g.set_settings(iter_max=10)
    _install(A, pol)
    before = _state(A, kkt=True)
    pth, pu, px = (binding.PinnedArray(s) for s in ((len(idx), K), (len(idx), NR), (len(idx), pat.n)))
    pth.a[...] = theta; pu.a[...] = np.nan; px.a[...] = np.nan
    codes = A.update_param_solve_subset(idx, pth.a, u_out=pu.a, x_out=px.a)
    assert A.last_update_path() == "fused into the solve"
    Bh.update_param_indexed(idx, theta)
    Bh.solve_subset(idx)
    first_iters = Bh.info_arrays()["iter"][idx].copy()
    ids = _host_retry(Bh, idx, pol, launch)
    got, want = _state(A, kkt=True), _state(Bh, kkt=True)
    print(name, "list", idx, "warm iterations of the first attempt", first_iters, "retried", ids)
    _assert_rows(got, want, range(B), (name, "fused subset step under a policy"))
    _assert_rows(got, before, rest, (name, "rows outside the list"))
    assert np.array_equal(codes, want["info.exitcode"][idx])
    assert np.array_equal(pu.a, Bh.outputs_indexed(idx)) and np.array_equal(px.a, want["x"][idx])
    counts = A.retry_counts()
    assert np.array_equal(counts, _counts_of(ids, B)) and not counts[rest].any()
    assert 0 < len(ids) <= len(idx), ids
    for p_ in (pth, pu, px):
        p_.close()
    A.close()
    Bh.close()


def _host_rollout(ref, fm, theta0, T, w, pol, launch):
    """The host loop of tests/test_rollout.py with the host retry sequence inside each step: update from theta -> solve -> retry ->
    outputs -> plant.  Returns u_traj, theta_traj, exitcodes, iters in the layout of rollout(), and the retried steps per instance."""
    B = theta0.shape[0]
    th, thetas, us, codes, iters, retried = theta0.copy(), [theta0.copy()], [], [], [], np.zeros(B, np.int32)
    for t in range(T):
        ref.update_param(th)
        ref.solve()
        retried[_host_retry(ref, range(B), pol, launch)] += 1
        ia = ref.info_arrays()
        codes.append(ia["exitcode"].copy()); iters.append(ia["iter"].copy())
        us.append(ref.outputs())
        th = fm.evaluate(th, us[-1], None if w is None else w[:, t])
        thetas.append(th)
    return (np.stack(us, axis=1), np.stack(thetas, axis=1), np.stack(codes, axis=1), np.stack(iters, axis=1)), retried


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{}, BUILDS[6][2]], ids=["lds", "no-lds"])
def test_rollout_retries_between_its_steps(env, monkeypatch):
    """Case 5: a warm-started rollout whose cap is the smallest iteration count of the uncapped rollout, so that some steps retry cold
    inside the one launch and some do not."""
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    name, B, K, NR, T = "MPC02", 4, 7, 6, 3
    pat, d = P._data(name, B)
    pm, om, fm = P._map(d, K), _omap(pat.n, NR), RO._fmap(K, NR)
    theta0, w = P._theta(B, K), RO._w(B, T, K)
    handles = []
    for _ in range(3):
        g = eicos_amd.BatchSolver(pat, B)
        g.update(*[d[k_] for k_ in KEYS])
        assert (g.solve() == 0).all()
        g.set_param_map(pm); g.set_output_map(om)
        g.set_warm_start(0.1)
        handles.append(g)
    A, ref, twin = handles
    lds = A.dims()["lds_bytes"] > 0
    assert lds == (not env)
    A.set_plant_map(fm); twin.set_plant_map(fm)
    iters0 = twin.rollout(theta0, T, w)[3]
    assert iters0.min() < iters0.max(), iters0
    cap = int(iters0.min())
    launch, pol = _policy(warm=0.1, iter_max=cap), _policy()
    for g in (A, ref):
        g.set_settings(iter_max=cap)
    _install(A, pol)
    got = A.rollout(theta0, T, w)
    assert A.last_rollout_launches() == (1 if lds else T)
    want, retried = _host_rollout(ref, fm, theta0, T, w, pol, launch)
    counts = A.retry_counts()
    print(name, env, "uncapped iterations", iters0.tolist(), "cap", cap, "retried steps", retried, "iterations", want[3].tolist())
    RO._assert_rollout(got, want, (name, env, "rollout with retries"))
    _assert_rows(_state(A, kkt=True), _state(ref, kkt=True), range(B), (name, env, "state after the rollout"))
    assert np.array_equal(counts, retried)
    assert 0 < counts.sum() < B * T, counts
    for g in handles:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]])
def test_multi_retry_matches_the_single_handle(devices, monkeypatch):
    """Case 6: the policy on every shard; the counters come back in global ids."""
    for k, v in W2.items():
        monkeypatch.setenv(k, v)
    name = "MPC02"
    B, cap, _ = CASES[name]
    pat, d = _data(name, B)
    eicos_amd.set_arithmetic_profile(1)  # (plans by the pattern alone: a shard gives the bits of the batch)
    try:
        one = eicos_amd.BatchSolver(pat, B)
        multi = eicos_amd.MultiBatchSolver(pat, B, devices)
    finally:
        eicos_amd.set_arithmetic_profile(0)
    assert len(multi.shards()) == len(devices)
    c2, h2, b2 = _perturbed(d)
    pol = _policy()
    for g in (one, multi):
        g.update(*[d[k] for k in KEYS])
        g.update_rhs(c2, h2, b2 if pat.p else None)
        g.set_settings(iter_max=cap)
        _install(g, pol)
        assert g.retry() == one.retry() and g.retry()["mask"] == NOT_OPTIMAL
    codes = one.solve()
    assert np.array_equal(multi.solve(), codes)
    _assert_rows(_state(multi), _state(one), range(B), ("multi retry", devices))
    counts = one.retry_counts()
    print(name, devices, "retried", np.nonzero(counts)[0])
    assert 0 < counts.sum() < B and np.array_equal(multi.retry_counts(reset=True), counts)
    assert not multi.retry_counts().any() and np.array_equal(one.retry_counts(), counts)
    with pytest.raises(RuntimeError, match="EICOS_SEL_UNSOLVED"):
        multi.set_retry(eicos_amd.SEL_UNSOLVED)
    assert multi.retry() == one.retry()
    multi.set_retry(None)
    assert multi.retry()["mask"] == 0
    one.close()
    multi.close()


@pytest.mark.gpu
def test_retry_refusals_round_trip_and_removal(monkeypatch):
    """Case 7: a refused policy names its cause and changes nothing; get returns what was set; a removed policy leaves no trace."""
    name, _b, env, build = BUILDS[0]
    B, cap, pat, d, g, twin = _case_handles(name, env, build, monkeypatch)
    assert g.retry() == binding.default_retry()
    g.set_retry(eicos_amd.SEL_MAXIT | eicos_amd.SEL_NUMERICS, warm=0.25, dyn=(3e-7, 2e-13), iter_max=77, nitref=4, reltol=1e-7)
    held = g.retry()
    assert held == {"mask": eicos_amd.SEL_MAXIT | eicos_amd.SEL_NUMERICS, "warm": 0.25, "dyn": (3e-7, 2e-13),
                    "settings": {**eicos_amd.default_settings(), "iter_max": 77, "nitref": 4, "reltol": 1e-7}}
    refused = [
        (lambda: g.set_retry(1 << 12), "bits above bit 11"),
        (lambda: g.set_retry(eicos_amd.SEL_MAXIT | 1 << 20), "bits above bit 11"),
        # (UNSOLVED alone can never act; beside other classes the bit is idle -- SEL_NOT_OPTIMAL, the mask of every case here, holds it)
        (lambda: g.set_retry(eicos_amd.SEL_UNSOLVED), "EICOS_SEL_UNSOLVED"),
        (lambda: g.set_retry(NOT_OPTIMAL, warm=-0.1), "warm"),
        (lambda: g.set_retry(NOT_OPTIMAL, warm=float("nan")), "warm"),
        (lambda: g.set_retry(NOT_OPTIMAL, dyn=(-1e-7, 0.0)), "dyn_delta"),
        (lambda: g.set_retry(NOT_OPTIMAL, feastol=0.0), "feastol"),
        (lambda: g.set_retry(NOT_OPTIMAL, reltol_inacc=float("inf")), "reltol_inacc"),
        (lambda: g.set_retry(NOT_OPTIMAL, iter_max=0), "iter_max"),
        (lambda: g.set_retry(NOT_OPTIMAL, iter_max=101), "iter_max"),
        (lambda: g.set_retry(NOT_OPTIMAL, nitref=-1), "nitref"),
    ]
    for call, msg in refused:
        with pytest.raises(RuntimeError, match=msg):
            call()
        assert g.retry() == held, msg
    L = binding._lib()
    out = np.zeros(B, np.int32)
    assert L.eicos_batch_retry_counts(g._h, 1, B, binding._ip(out), 0) == -1 and b"out of bounds" in L.eicos_last_error()
    assert L.eicos_batch_retry_counts(g._h, 0, B, None, 0) == -1 and b"NULL" in L.eicos_last_error()
    # removal: the next solve is that of a handle that never had a policy
    g.set_retry(None)
    assert g.retry() == binding.default_retry()
    for h in (g, twin):
        h.set_settings(iter_max=cap)
    assert np.array_equal(g.solve(), twin.solve())
    _assert_rows(_state(g, kkt=True), _state(twin, kkt=True), range(B), "after the policy was removed")
    assert not g.retry_counts().any()
    g.set_retry(0)  # (mask 0 removes as well)
    assert g.retry()["mask"] == 0
    g.close()
    twin.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,_b,env,build", [BUILDS[0], BUILDS[1]])
def test_no_policy_gives_the_first_launch_alone(name, _b, env, build, monkeypatch):
    """Case 8: a handle that never called set_retry, and one that set and removed a policy, give the bits of the capped launch alone --
    and a policy whose mask holds nobody's class changes nothing either."""
    B, cap, pat, d, never, removed, other = _case_handles(name, env, build, monkeypatch, handles=3)
    _install(removed, _policy())
    removed.set_retry(None)
    other.set_retry(eicos_amd.SEL_PINF | eicos_amd.SEL_DINF | eicos_amd.SEL_FATAL)  # (nobody ends there)
    codes = []
    for g in (never, removed, other):
        g.set_settings(iter_max=cap)
        codes.append(g.solve())
    want = _state(never, kkt=True)
    assert (_classes(never) & NOT_OPTIMAL).any()  # (the cap does stop somebody: a policy would have had work)
    for g, c in zip((removed, other), codes[1:]):
        assert np.array_equal(c, codes[0])
        _assert_rows(_state(g, kkt=True), want, range(B), (name, "no policy in effect"))
        assert not g.retry_counts().any()
    for g in (never, removed, other):
        g.close()
