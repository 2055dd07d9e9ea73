"""The parked refinement iterate of the KKT solve (eicos_dims.iterate_park, knob EICOS_XPARK).

With one LDS vector per workgroup (several workgroups per CU) the vector alternates between the sweep vector and the iterate X, and a
refinement step has to put X somewhere while the sweeps run.  The two-waves-per-SIMD build of the 256-thread kernel keeps it in registers
of the thread that owns each element (at most 26 per thread, so dim_K <= 26 * 256); every other handle keeps it in the workspace slab.
Both paths move the same values through the same operations: the contract is bit-identity of everything a caller can read."""
import os

import numpy as np
import pytest

from conftest import ROOT, load_fixture
import eicos_amd
from eicos_amd.generate import feasible_batch, mpc_soc_variant, perturbed_batch

CAP = 26 * 256  # XPARK_R * threads (eicos_amd/csrc/device_types.hpp)
INFO_SKIP = ("solve_us",)  # device wall time of the instance's solve: the only field that is not a function of the data
# the 256-thread kernel with one LDS vector, one right-hand side per solve, at most two workgroups per CU, factor operands in the slab
SHAPE = {"EICOS_THREADS": "256", "EICOS_NLDS": "1", "EICOS_DUAL": "0", "EICOS_UBL": "0", "EICOS_BLOCKS_PER_CU": "2"}


def _run(pat, d, B, monkeypatch, knob):
    monkeypatch.setenv("EICOS_XPARK", knob)
    g = eicos_amd.BatchSolver(pat, B)
    g.update(d["Gpr"], d["Apr"], d["c"], d["h"], d["b"])
    codes = np.asarray(g.solve()).copy()
    y, z, s = g.duals()
    ia = g.info_arrays()
    out = dict(codes=codes, x=g.solution().copy(), y=y.copy(), z=z.copy(), s=s.copy())
    out.update({"info." + k: np.asarray(v).copy() for k, v in ia.items() if k not in INFO_SKIP})
    dims, build = g.dims(), g.kernel_build()
    g.close()
    return out, dims, build


def _both(pat, d, B, monkeypatch):
    for k, v in SHAPE.items():
        monkeypatch.setenv(k, v)
    off, d_off, b_off = _run(pat, d, B, monkeypatch, "0")
    on, d_on, b_on = _run(pat, d, B, monkeypatch, "1")
    assert b_off == b_on == "w2" and d_off["threads_per_block"] == d_on["threads_per_block"] == 256
    assert d_off["iterate_park"] == 0
    assert set(off) == set(on) and {"info.n_ldlsolve", "info.nitref1", "info.iter", "info.pcost"} <= set(on)
    for k in sorted(on):
        assert np.array_equal(off[k], on[k], equal_nan=True), k
    return on, d_on


def _two_per_cu(dims, B):
    import ctypes
    from eicos_amd.binding import _lib
    n = ctypes.c_int()
    assert _lib().hipDeviceGetAttribute(ctypes.byref(n), 63, 0) == 0  # (hipDeviceAttributeMultiprocessorCount, through the solver's runtime)
    return B > n.value and dims["resident_blocks"] == min(B, 2 * n.value)  # (more instances than CUs, two resident workgroups on each)


@pytest.mark.gpu
@pytest.mark.parametrize("soc,B", [(False, 512), (True, 776)])
def test_registers_and_slab_give_the_same_bits_on_the_headline_patterns(soc, B, monkeypatch):
    pat, sets = load_fixture("MPC02")
    if soc:
        pat = mpc_soc_variant(pat, sets[0])
    d = feasible_batch(pat, sets[0], 0, B)
    on, dims = _both(pat, d, B, monkeypatch)
    assert dims["dim_K"] <= CAP and dims["iterate_park"] == 1 and _two_per_cu(dims, B)
    assert (on["codes"] == 0).all()
    assert (on["info.n_ldlsolve"] > 3 * (on["info.iter"] + 1) + 2).any()  # (two solves to initialise, three per pass: some solve took a refinement step)


@pytest.mark.gpu
def test_registers_and_slab_give_the_same_bits_through_multi_step_refinement(monkeypatch):
    # lp_agg, perturbed: stalled, ill-conditioned instances (some end "optimal, reduced accuracy") whose solves take several refinement
    # steps, so that the registers are parked, added to and parked again within one solve, and the "got worse: undo" exit is in reach
    pat, sets = load_fixture("lp_agg")
    B = 512
    d = perturbed_batch(pat, sets[0], 0, B)
    on, dims = _both(pat, d, B, monkeypatch)
    assert dims["iterate_park"] == 1 and _two_per_cu(dims, B)
    nit = np.maximum(np.maximum(on["info.nitref1"], on["info.nitref2"]), on["info.nitref3"])
    assert nit.max() > 1, nit.max()  # (nitref*: refinement steps of the three solves of an instance's last pass)
    # ... and over the whole solve: at most 2 + 3 (iter + 1) systems are solved (two to initialise, three per pass), each with one LDL solve
    # per refinement step + 1 -- more than two per system means that some system took at least two steps
    calls = 2 + 3 * (on["info.iter"] + 1)
    assert (on["info.n_ldlsolve"] > 2 * calls).any()


@pytest.mark.gpu
def test_a_pattern_beyond_the_register_cap_keeps_the_slab(monkeypatch):
    # one more cone than the MPC-SOC variant: dim_K = 26 * 256 + 1, one element past what 256 threads hold
    pat, sets = load_fixture("MPC02")
    pat = mpc_soc_variant(pat, sets[0], rows_from=2997)
    B = 4
    d = feasible_batch(pat, sets[0], 0, B)
    on, dims = _both(pat, d, B, monkeypatch)
    assert dims["dim_K"] == CAP + 1 and dims["iterate_park"] == 0
    assert (on["codes"] == 0).all()


def test_dims_mirror_ends_with_the_park_field():
    from eicos_amd import binding
    assert binding.Dims._fields_[-1][0] == "iterate_park"
    assert open(os.path.join(ROOT, "include", "eicos_amd.h")).read().count("int iterate_park;") == 1
