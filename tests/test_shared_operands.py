"""Shared factor operands (eicos_dims.shared_operands, knob EICOS_SHARED_OPERANDS).

While a batch shares its matrices (eicos_batch_shared_values = 1) every operand of the LDL' code whose value is a plain A, G, +-delta or 0
entry of K holds the same bits in every instance: the K entries of the numeric factorisation outside the scaling block, and the level-0
columns of U = L.*D that the backward sweep streams.  A handle on the scalar factor path that keeps U in the workspace slab fills one copy of
both from instance 0 and lets every instance read it.  The same values from another address: x, y, z, s, the exit codes and every info
field except the device wall time are bit for bit those of a twin handle created with the knob off, through every kind of update."""
import os

import numpy as np
import pytest

from conftest import ROOT, load_fixture
import eicos_amd
from eicos_amd.generate import feasible_batch, mpc_soc_variant, perturbed_batch
from test_shared_values import KEYS, Dev, _changed, _results, _same


def _mpc02(B):
    pat, sets = load_fixture("MPC02")
    return pat, feasible_batch(pat, sets[0], 0, B)


def _mpc_soc(B):
    pat, sets = load_fixture("MPC02")
    pat = mpc_soc_variant(pat, sets[0])
    return pat, feasible_batch(pat, sets[0], 0, B)


def _adlittle(B):
    pat, sets = load_fixture("lp_adlittle")
    return pat, perturbed_batch(pat, sets[0], 0, B)


def _afiro(B):
    pat, sets = load_fixture("lp_afiro")
    return pat, perturbed_batch(pat, sets[0], 0, B)


# name -> (batch, problem, kernel build, workgroup size, shared_operands, shared_values after a full identical update)
# (None = whatever the launch shape chooses on the device at hand; a shape's knobs, if any, are in SHAPE_ENV)
SHAPES = {
    "mpc02_b300": (300, _mpc02, "w2", 256, 1, True),        # two workgroups per CU: the 256-VGPR build of the headline
    "mpc02_b600": (600, _mpc02, None, 256, 1, True),        # between two and three per CU: the launch shape's own choice
    "mpc02_b600_default": (600, _mpc02, "default", 256, 1, True),  # ... and the 168-VGPR build that three per CU run, by its knob
    "mpc02_b1100": (1100, _mpc02, None, 256, 1, True),      # more instances than resident workgroups: two rounds
    "mpc_soc_b300": (300, _mpc_soc, "w2", 256, 1, True),    # cone blocks: scaling-block entries off the diagonal of K
    "mpc02_b3": (3, _mpc02, "default", 512, 1, True),       # one workgroup per CU: 512 threads, both right-hand sides in one sweep
    "lp_adlittle_b4": (4, _adlittle, "u-in-lds", 256, 0, True),  # the factor operands are in LDS already
    "lp_afiro_b4": (4, _afiro, "lds-resident", 128, 0, False),
}
SHAPE_ENV = {"mpc02_b600_default": {"EICOS_W2": "0"}}
_CACHE = {}


def _problem(name):
    """(pattern, batch arrays, B) of a shape: generated once, shared by the tests, never modified (the tests copy what they change)."""
    if name not in _CACHE:
        B, make = SHAPES[name][:2]
        same = [v for k, v in _CACHE.items() if SHAPES[k][:2] == (B, make)]
        pat, d = same[0][:2] if same else make(B)
        for k in ("Gpr", "Apr"):
            assert d[k].size == 0 or np.array_equal(d[k], np.broadcast_to(d[k][0], d[k].shape))  # every instance gets the same matrices
        for k in KEYS:
            d[k].setflags(write=False)
        _CACHE[name] = (pat, d, B)  # (shapes of one problem and batch share the arrays)
    return _CACHE[name]


def _pair(name, monkeypatch):
    """(handle with the feature, twin created with the knob off) of a shape, builds and the dims field confirmed."""
    pat, d, B = _problem(name)
    _, _, build, threads, operands, _ = SHAPES[name]
    for k, v in SHAPE_ENV.get(name, {}).items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("EICOS_SHARED_OPERANDS", "0")
    off = eicos_amd.BatchSolver(pat, B)
    monkeypatch.delenv("EICOS_SHARED_OPERANDS")
    on = eicos_amd.BatchSolver(pat, B)
    for g in (on, off):
        dims = g.dims()
        assert build is None or g.kernel_build() == build, g.kernel_build()
        assert threads is None or dims["threads_per_block"] == threads, dims
        assert dims["factor_path"] == 0
    assert on.dims()["shared_operands"] == operands and off.dims()["shared_operands"] == 0
    if name == "mpc02_b1100":
        assert on.dims()["resident_blocks"] < B  # (two rounds)
    if name == "mpc02_b3":
        assert on.dims()["dual_rhs"] == 1
    return on, off, pat, d, B


def _update_both(on, off, dev, d, **kw):
    ptrs = dev.put(d)
    on.update_device(*ptrs, **kw)
    off.update_device(*ptrs, **kw)
    return ptrs


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_identical_matrices_read_one_copy_and_give_the_twins_bits(name, monkeypatch):
    on, off, pat, d, B = _pair(name, monkeypatch)
    shares = SHAPES[name][5]
    dev = Dev()
    try:
        _update_both(on, off, dev, d)
        assert on.shared_values() == shares and off.shared_values() == shares  # (the twin shares the product values too: only the operands differ)
        ref = _results(off)
        _same(_results(on), ref)
        assert (ref["codes"] == 0).any()
        _same(_results(on), ref)  # a second solve of the same data: the arrays are still valid
    finally:
        dev.free(); on.close(); off.close()


@pytest.mark.gpu
def test_one_differing_bit_in_one_instance_reads_nothing_shared(monkeypatch):
    name = "mpc02_b300"
    on, off, pat, d, B = _pair(name, monkeypatch)
    dev = Dev()
    try:
        _update_both(on, off, dev, d)
        assert on.shared_values()
        e = d["Gpr"].shape[1] // 2
        v = np.array([d["Gpr"][7, e]])
        v.view(np.uint64)[0] ^= 1  # the last mantissa bit
        dd = _changed(d, 7, e=e, value=v[0])
        _update_both(on, off, dev, dd)
        assert not on.shared_values() and not off.shared_values()  # (the word reads -1)
        _same(_results(on), _results(off))
        _update_both(on, off, dev, d)  # identical again: the copy is filled again
        assert on.shared_values()
        _same(_results(on), _results(off))
    finally:
        dev.free(); on.close(); off.close()


@pytest.mark.gpu
def test_updates_that_drop_or_keep_the_shared_state(monkeypatch):
    name = "mpc02_b300"
    on, off, pat, d, B = _pair(name, monkeypatch)
    dev = Dev()
    try:
        full = _update_both(on, off, dev, d)
        assert on.shared_values()
        # a sub-range updateData with other matrices: the word drops, every instance reads its own operands
        other = _changed(d, B - 1, e=1)
        one = [other[k][B - 1:B] for k in KEYS]
        on.update(*one, first=B - 1, count=1); off.update(*one, first=B - 1, count=1)
        assert not on.shared_values()
        _same(_results(on), _results(off))
        # identical again, then a right-hand-side-only update: it keeps the matrices, the word and the copy
        on.update_device(*full); off.update_device(*full)
        c2 = d["c"] * (1 + 2.0 ** -12)
        on.update_rhs(c2, d["h"], d["b"]); off.update_rhs(c2, d["h"], d["b"])
        assert on.shared_values()
        _same(_results(on), _results(off))
        # a full update that keeps a group (A): not the detecting launch
        assert pat.p > 0
        on.update_device(full[0], 0, full[2], full[3], 0); off.update_device(full[0], 0, full[2], full[3], 0)
        assert not on.shared_values()
        _same(_results(on), _results(off))
        # ... and one that keeps c but gives both matrices is
        on.update_device(full[0], full[1], 0, full[3], full[4]); off.update_device(full[0], full[1], 0, full[3], full[4])
        assert on.shared_values()
        _same(_results(on), _results(off))
    finally:
        dev.free(); on.close(); off.close()


@pytest.mark.gpu
def test_warm_start_and_dynamic_regularisation(monkeypatch):
    name = "mpc02_b300"
    on, off, pat, d, B = _pair(name, monkeypatch)
    dev = Dev()
    try:
        full = _update_both(on, off, dev, d)
        for g in (on, off):
            g.set_warm_start(0.1)
        _same(_results(on), _results(off))          # cold: nothing to start from yet
        c2 = d["c"] * (1 + 2.0 ** -10)
        on.update_rhs(c2, d["h"], d["b"]); off.update_rhs(c2, d["h"], d["b"])
        warm = _results(on)
        _same(warm, _results(off))                  # warm: from the previous solution
        assert warm["info.iter"].mean() > 0
        # dynamic regularisation changes the pivots, not the K entries
        for g in (on, off):
            g.set_warm_start(0.0); g.set_dynamic_regularization(2e-7, 1e-13)
        on.update_device(*full); off.update_device(*full)
        assert on.shared_values()
        _same(_results(on), _results(off))
    finally:
        dev.free(); on.close(); off.close()


@pytest.mark.gpu
def test_two_shards_each_fill_their_own_copy(monkeypatch):
    pat, d300, _ = _problem("mpc02_b300")
    B, half = 600, 300
    d = {k: np.concatenate([d300[k], d300[k]]) for k in KEYS}
    d["Gpr"][half:] *= 1 + 2.0 ** -16  # the two shards get different matrices, identical inside each
    dev = Dev()
    monkeypatch.setenv("EICOS_SHARED_OPERANDS", "0")
    off = eicos_amd.MultiBatchSolver(pat, B, [0, 0])
    monkeypatch.delenv("EICOS_SHARED_OPERANDS")
    on = eicos_amd.MultiBatchSolver(pat, B, [0, 0])
    try:
        assert on.shards() == [(0, half, 0), (half, half, 0)]
        assert [on.shard_dims(s)["shared_operands"] for s in (0, 1)] == [1, 1]
        assert [off.shard_dims(s)["shared_operands"] for s in (0, 1)] == [0, 0]
        ptrs = dev.put(d)
        on.update_device(0, *ptrs); off.update_device(0, *ptrs)
        assert on.shard_shared_values(0) and on.shard_shared_values(1)
        _same(_results(on), _results(off))
    finally:
        dev.free(); on.close(); off.close()


def test_the_report_field_is_declared_once_on_both_sides():
    from eicos_amd import binding
    names = [f for f, _ in binding.Dims._fields_]
    assert names.count("shared_operands") == 1
    header = open(os.path.join(ROOT, "include", "eicos_amd.h")).read()
    assert header.count("int shared_operands;") == 1
    # the ctypes mirror lists the fields in the header's order
    body = header[header.index("typedef struct eicos_dims {"):header.index("} eicos_dims;")]
    assert body.index("int shared_operands;") < body.index("int iterate_park;")
    assert names.index("shared_operands") < names.index("iterate_park")
