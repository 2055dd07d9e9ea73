"""The host's copy pool (eicos_amd/csrc/host_copy.hpp, host_copy.cpp: stream_copy, the piece rule, CopyPool) -- the library's only
multithreaded host code -- checked without a GPU through a stand-alone program, tests/host/host_copy_check.cpp, built once with the
address and undefined-behaviour sanitizers and once with the thread sanitizer.  The program runs in its own process per setting of the
pool (a singleton that reads its knobs once); nothing sanitized is loaded into this one."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "eicos_amd", "csrc")
SANITIZERS = {
    # (the sanitizer runtimes linked statically: the program then also starts where the environment preloads a library into every process)
    "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"],
    "tsan": ["-fsanitize=thread", "-static-libtsan"],
}


@pytest.fixture(scope="module", params=sorted(SANITIZERS))
def host_copy_check(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_copy_" + request.param) / "host_copy_check")
    # (no HIP include path: host_copy.cpp is compiled as the library's Makefile compiles it)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread"] + SANITIZERS[request.param] +
                          ["-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "host", "host_copy_check.cpp"),
                           os.path.join(CSRC, "host_copy.cpp"), "-o", exe])
    return exe


def _run(exe, args, knobs):
    env = {k: v for k, v in os.environ.items() if not k.startswith("EICOS_")}
    env.update(knobs)
    out = subprocess.run([exe] + args, capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr
    return out.stdout


def test_pieces_tile_the_copy(host_copy_check):
    """The piece rule as arithmetic: for 0, 1, 15, 4095, 4096, 4097, 1 MB - 1, 1 MB + 1, 3 MB + 17 and 12 MB + 5 bytes over 0, 1, 3, 10
    and 64 helpers the pieces tile [0, bytes) in order without overlap and start on multiples of 64; part counts, piece lengths and
    boundaries against numbers worked out by hand; two sizes whose last pieces are empty."""
    assert "all passed" in _run(host_copy_check, ["pieces"], {})


@pytest.mark.parametrize("nt", [1, 0])
@pytest.mark.parametrize("threads", [0, 1, 3])
def test_concurrent_copies_are_exact(host_copy_check, threads, nt):
    """Four host threads call CopyPool::copy at once on a pool of `threads` helpers, with and without non-temporal stores: every size
    above, source and destination 0, 1, 7 and 15 bytes off a 16-byte boundary; each destination equals its source byte for byte and
    the 64 guard bytes on either side of it are untouched."""
    out = _run(host_copy_check, ["copy", str(threads)],
               {"EICOS_EXPERIMENT": "1", "EICOS_COPY_THREADS": str(threads), "EICOS_COPY_NT": str(nt)})
    assert "all passed" in out
