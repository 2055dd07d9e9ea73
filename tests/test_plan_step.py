"""The host-only steps of handle creation (eicos_amd/csrc/plan_step.cpp: pattern intake, analysis, plan, LDS budget) and the host self
checks (host_check.cpp), run without a GPU through a stand-alone program built with the address and undefined-behaviour sanitizers:
tests/host/plan_step_check.cpp.  The program is built once and runs in its own process per case; nothing sanitized is loaded into this
one.  The tests of test_abi_and_symbolic.py that call the same entries through the library stay as they are."""
import os
import subprocess

import pytest

from conftest import ALL_FIXTURES, GOLDEN, ROOT

CSRC = os.path.join(ROOT, "eicos_amd", "csrc")
# `checks` (the three host self checks) runs on this subset -- the LDS-resident build, the apex alternative, hybrid, scalar with apex, cones
# and the empty edge -- because the deep Netlib patterns take tens of seconds each under the sanitizers; `plans` runs on every fixture.
CHECK_FIXTURES = ["lp_afiro", "lp_blend", "lp_bandm", "MPC02", "issue98", "unboundedMaxSqrt", "update_data", "emptyProblem"]


@pytest.fixture(scope="module")
def plan_step_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_step") / "plan_step_check")
    # (the sanitizer runtimes linked statically: the program then also starts where the environment preloads a library into every process)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-Wall", "-Wno-unused-parameter",
                           "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "plan_step_check.cpp")] +
                          [os.path.join(CSRC, f) for f in ("plan_step.cpp", "host_check.cpp", "symbolic.cpp", "plans.cpp", "tiles.cpp")] +
                          ["-o", exe])
    return exe


def _run(exe, mode, name):
    env = {k: v for k, v in os.environ.items() if not k.startswith("EICOS_")}  # (no experiment knob reaches the plans)
    out = subprocess.run([exe, mode, os.path.join(GOLDEN, name + ".epb")], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr
    return out.stdout


@pytest.mark.parametrize("name", ALL_FIXTURES)
def test_plans_address_what_they_own(plan_step_check, name):
    """Every configuration of the pattern -- batch 1, 256, 1024 x arithmetic profile 0, 1 x apex off / on where the analysis allows, 256 CUs
    -- plans with EICOS_OK, and the plan holds: (a) every pool slot inside the pool and 16-byte aligned, (b) every LDS region the DevPat
    names inside the dynamic LDS, disjoint from the others (but for the in-place apex image of the LDS-resident build), and the dynamic
    LDS plus the static block inside the CU's 160 KiB, (c) every 16-bit packed index array decoded by the kernel's rule gives its 32-bit
    form and the pad value beyond K."""
    out = _run(plan_step_check, "plans", name)
    assert ", 0 failures" in out and "FAIL" not in out, out


@pytest.mark.parametrize("name", CHECK_FIXTURES)
def test_host_self_checks_under_sanitizers(plan_step_check, name):
    """The scalar, tile and hybrid host checks on the pattern, with the bounds of test_abi_and_symbolic.py: residual in [0, 1e-12),
    hybrid -10 or in [0, 1e-12); tiles and hybrid not on the empty problem."""
    out = _run(plan_step_check, "checks", name)
    assert "FAIL" not in out, out


def test_fingerprints_are_reproducible(plan_step_check):
    """The fingerprint lines (compared between two builds of the plan step when it is refactored) are the same from run to run."""
    a, b = (_run(plan_step_check, "fingerprint", "lp_blend") for _ in range(2))
    assert a == b and len(a.splitlines()) >= 6, a
