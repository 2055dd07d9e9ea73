"""CPU: the C-ABI library loads, exports every symbol include/eicos_amd.h declares, refuses to
compute without a GPU (no CPU fallback), and the host-side symbolic analysis (ordering, L
pattern, level schedule, factor program) is numerically right on every fixture pattern."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ALL_FIXTURES, ROOT, load_fixture
import eicos_amd
from eicos_amd.binding import host_check, library_path


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "eicos_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(eicos_[a-z_0-9]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(library_path())
    syms = declared_symbols()
    assert len(syms) >= 18
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/eicos_amd.h but not exported"


def declared_prototypes():
    """{name: (return type, [parameter types])} of every prototype of include/eicos_amd.h, as C text without `const`, parameter names
    and spare blanks: "int", "double *", "eicos_batch * *", ..."""
    text = open(os.path.join(ROOT, "include", "eicos_amd.h")).read()
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    text = re.sub(r"^[ \t]*#[^\n]*", ";", text, flags=re.M)  # (preprocessor lines: not part of a declaration)

    def ctype_text(decl, named):
        decl = re.sub(r"\bconst\b", " ", decl).replace("*", " * ").split()
        return " ".join(decl[:-1] if named and decl[-1] != "*" else decl)

    protos = {}
    for ret, name, params in re.findall(r"([\w\s\*]*?)\b(eicos_[a-z_0-9]+)\s*\(([^();{}]*)\)\s*;", text):
        assert name not in protos, name
        params = [] if params.strip() in ("", "void") else params.split(",")
        protos[name] = (ctype_text(ret, False), [ctype_text(p, True) for p in params])
    return protos


def test_binding_prototypes_are_the_header():
    """What eicos_amd.binding installs on the library is what include/eicos_amd.h declares: for EVERY declared function the argument
    count, scalar against scalar ctype, pointer against pointer ctype (c_void_p passes for any pointer: raw device addresses), the
    pointee of a typed pointer, and the return type; and the binding's table names no eicos_ function the header lacks."""
    from eicos_amd import binding
    lib = binding._lib()
    scalars = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "double": ctypes.c_double, "float": ctypes.c_float, "size_t": ctypes.c_size_t}
    structs = {"eicos_info": binding.Info, "eicos_dims": binding.Dims, "eicos_affine_map": binding.AffineMap,
               "eicos_settings": binding.Settings, "eicos_retry": binding.Retry}
    returns = dict(scalars, **{"char *": ctypes.c_char_p, "void *": ctypes.c_void_p, "void": None})
    protos = declared_prototypes()
    assert sorted(protos) == declared_symbols()  # (the parser found every declared function)
    for name, (ret, params) in protos.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None, f"{name}: no argtypes installed"
        assert len(fn.argtypes) == len(params), f"{name}: {len(fn.argtypes)} argtypes, the header has {len(params)} parameters"
        assert ret in returns and fn.restype is returns[ret], f"{name}: restype {fn.restype}, the header returns {ret}"
        for k, (param, ct) in enumerate(zip(params, fn.argtypes)):
            where = f"{name}, argument {k}: header `{param}`, ctypes {ct.__name__}"
            base, stars = param.split()[0], param.count("*")
            if stars == 0:
                assert param in scalars and ct is scalars[param], where
            elif ct is not ctypes.c_void_p:
                assert issubclass(ct, ctypes._Pointer), where
                pointee = ctypes.c_void_p if stars == 2 else scalars.get(base) or structs.get(base)
                assert stars <= 2 and pointee is not None and ct._type_ is pointee, where
    listed = {full for full, _, _ in binding._SIGNATURES if full.startswith("eicos_")}
    assert listed <= set(protos), f"in the binding's table but not in the header: {sorted(listed - set(protos))}"


def test_cpp_header_compiles_against_c_header():
    # include/eicos.hpp (EiCOS::Solver wrapper) must at least parse with a host compiler
    import subprocess, tempfile
    hdr = os.path.join(ROOT, "include", "eicos.hpp")
    if not os.path.exists(hdr):
        pytest.skip("C++ wrapper header not present")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        open(src, "w").write('#include "eicos.hpp"\nint main(){return 0;}\n')
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), src])


def test_ecos_shim_and_demo_compile():
    # include/ecos.h (drop-in for the reference's test/ecos.h) and examples/run_demo.cpp (counterpart of
    # the reference's src/run.cpp) must build against the C ABI with a plain host compiler
    import subprocess, tempfile
    inc = os.path.join(ROOT, "include")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        open(src, "w").write('#include "ecos.h"\nint main(){ pwork *w = nullptr; (void)w; return ECOS_OPTIMAL; }\n')
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", inc, src])
        subprocess.check_call(["g++", "-std=c++17", "-I", inc, os.path.join(ROOT, "examples", "run_demo.cpp"),
                               "-L", os.path.join(ROOT, "eicos_amd"), "-leicos_amd", "-o", os.path.join(d, "run_demo")])
        # ... and the multi-GPU demo (EiCOS::BatchSolver over a device list, include/eicos.hpp on top of eicos_multi_*); without a GPU
        # it must fail loudly at creation, naming the shard (no CPU fallback)
        exe = os.path.join(d, "multi_gpu_demo")
        subprocess.check_call(["g++", "-std=c++17", "-I", inc, os.path.join(ROOT, "examples", "multi_gpu_demo.cpp"),
                               "-L", os.path.join(ROOT, "eicos_amd"), "-leicos_amd", "-Wl,-rpath," + os.path.join(ROOT, "eicos_amd"), "-o", exe])
        if eicos_amd.device_count() == 0:
            out = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "lp_afiro.epb"), "4", "0,0"], capture_output=True, text=True)
            assert out.returncode != 0 and "no HIP device" in out.stderr and "shard 0" in out.stderr, out.stderr


@pytest.mark.skipif(eicos_amd.device_count() > 0, reason="GPU present")
def test_no_cpu_fallback_without_gpu():
    pat, _ = load_fixture("lp_afiro")
    with pytest.raises(RuntimeError, match="no HIP device"):
        eicos_amd.BatchSolver(pat, 4)


@pytest.mark.parametrize("name", ALL_FIXTURES)
def test_symbolic_program_solves_kkt(name):
    pat, _ = load_fixture(name)
    res, st = host_check(pat, seed=7)
    assert 0.0 <= res < 1e-12, (name, res)
    assert st["dim_K"] == pat.n + pat.p + pat.m + 2 * pat.ncones
    nV = pat.l + sum(3 * int(d) + 1 for d in pat.q)
    assert st["nnzK"] == pat.nnzA + pat.nnzG + pat.n + pat.p + nV  # reference src/eicos.cpp:1750-1759
    assert st["nnzL"] >= st["nnzK"] - st["dim_K"]


@pytest.mark.parametrize("mode", [0, 1, 3])
def test_orderings_agree(mode):
    pat, _ = load_fixture("lp_blend")
    res, st = host_check(pat, seed=3, order_mode=mode)
    assert 0.0 <= res < 1e-12 and st["order_mode"] == mode


def test_level_ordering_beats_sequential_depth_on_mpc():
    pat, _ = load_fixture("MPC02")
    _, seq = host_check(pat, order_mode=0)
    _, auto = host_check(pat, order_mode=-1)
    assert auto["nlevels"] * 10 < seq["nlevels"]       # chain peeled from both ends vs dissected
    assert auto["nnzL"] < 1.3 * seq["nnzL"]


def test_generator_is_shard_invariant():
    from eicos_amd.generate import feasible_batch, shard_range
    pat, sets = load_fixture("update_data")
    full = feasible_batch(pat, sets[0], 0, 6)
    parts = []
    for r in range(4):
        f, c = shard_range(6, r, 4)
        parts.append(feasible_batch(pat, sets[0], f, c)["h"])
    assert np.array_equal(np.concatenate(parts), full["h"])


def test_ecos_header_loader_round_trip(tmp_path):
    # N1 of SURVEY.md 8f: the ECOS data.h layout (what src/run.cpp:18-31 consumes) <-> EPB1, both directions,
    # with and without a name prefix, with absent groups (no A / no cones)
    import numpy as np
    import eicos_amd
    from conftest import load_fixture
    for name, prefix in (("update_data", "udd_"), ("lp_afiro", ""), ("issue98", "x_")):
        pat, sets = load_fixture(name)
        h = str(tmp_path / f"{name}.h")
        eicos_amd.write_ecos_header(h, pat, sets[0], prefix)
        pat2, sets2 = eicos_amd.read_problem(h)
        for k in ("n", "m", "p", "l"):
            assert getattr(pat, k) == getattr(pat2, k)
        for k in ("q", "Gjc", "Gir", "Ajc", "Air"):
            assert np.array_equal(getattr(pat, k), getattr(pat2, k)), (name, k)
        for k in ("Gpr", "Apr", "c", "h", "b"):
            assert np.array_equal(getattr(sets[0], k), getattr(sets2[0], k)), (name, k)
        e = str(tmp_path / f"{name}.epb")
        eicos_amd.write_epb(e, pat2, sets2)
        pat3, sets3 = eicos_amd.read_problem(e)
        assert np.array_equal(sets3[0].Gpr, sets[0].Gpr) and pat3.nnzA == pat.nnzA


def test_product_never_references_the_oracle():
    # oracle/ is test infrastructure: nothing under eicos_amd/, include/ or examples/ may import, include or link it,
    # and the shared library must not depend on liboracle.so
    import os, re, subprocess
    from conftest import ROOT
    pat = re.compile(r"^\s*(from\s+oracle|import\s+oracle|#\s*include\s*[\"<].*oracle)", re.M)
    for top in ("eicos_amd", "include", "examples"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".py", ".cpp", ".hpp", ".h", ".hip")) or f == "Makefile":
                    text = open(os.path.join(dirpath, f), errors="ignore").read()
                    assert not pat.search(text), os.path.join(dirpath, f)
                    if f == "Makefile":
                        assert "oracle" not in text
    lib = os.path.join(ROOT, "eicos_amd", "libeicos_amd.so")
    if os.path.exists(lib):
        needed = subprocess.run(["readelf", "-d", lib], capture_output=True, text=True).stdout
        assert "oracle" not in needed
    # and the ctypes mirror fails loudly without the HIP library instead of falling back to anything
    import eicos_amd.binding as b
    src = open(b.__file__).read()
    assert "oracle" not in src


def test_cpp_surfaces_compile_including_the_eigen_typed_overloads(tmp_path):
    # include/eicos.hpp as every kind of caller sees it (compile + link against the library, nothing runs):
    #  * raw-pointer callers without Eigen (examples/run_demo.cpp), solution() is a std::vector then;
    #  * the ECOS shim runner (examples/ecos_runner.cpp over include/ecos.h);
    #  * a caller shaped like the reference's src/run.cpp:11-50 using the Eigen-typed constructor / updateData and
    #    `const Eigen::VectorXd &solution()` (reference include/eicos.hpp:138-148,160), against the stand-in
    #    Eigen/Sparse of tests/eigen_standin (Eigen is not installed here) with -Wall -Wextra -Werror.
    import os, subprocess
    from conftest import ROOT
    lib = os.path.join(ROOT, "eicos_amd")
    inc = os.path.join(ROOT, "include")
    link = ["-L", lib, "-leicos_amd", "-Wl,-rpath," + lib] if os.path.exists(os.path.join(lib, "libeicos_amd.so")) else ["-c"]
    base = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", inc]
    subprocess.check_call(base + [os.path.join(ROOT, "examples", "run_demo.cpp"), "-o", str(tmp_path / "a")] + link)
    subprocess.check_call(base + [os.path.join(ROOT, "examples", "ecos_runner.cpp"), "-o", str(tmp_path / "b")] + link)
    subprocess.check_call(base + ["-I", os.path.join(ROOT, "tests", "eigen_standin"), os.path.join(ROOT, "tests", "cpp", "run_eigen_demo.cpp"),
                                  "-o", str(tmp_path / "c")] + link)
    # the return type really is the Eigen vector when Eigen is visible, and a std::vector when it is not
    probe = tmp_path / "probe.cpp"
    probe.write_text('#include <type_traits>\n#include "eicos.hpp"\n'
                     '#ifdef EICOS_HAVE_EIGEN\n'
                     'static_assert(std::is_same<decltype(std::declval<const EiCOS::Solver&>().solution()), const Eigen::VectorXd&>::value, "");\n'
                     '#else\n'
                     'static_assert(std::is_same<decltype(std::declval<const EiCOS::Solver&>().solution()), const std::vector<double>&>::value, "");\n'
                     '#endif\nint main() { return 0; }\n')
    subprocess.check_call(base + ["-fsyntax-only", str(probe)])
    subprocess.check_call(base + ["-fsyntax-only", "-I", os.path.join(ROOT, "tests", "eigen_standin"), str(probe)])


def test_tile_and_hybrid_plans_on_the_host():
    # The dense-front path without a GPU: the block-sparse 16 x 16 tile plan (ordering, blocks, tile pair program, finalise
    # lists, CSR / CSC tile views, tile-internal element order, inverse diagonal tiles, identity-tile skipping) and the
    # hybrid plan (scalar programs below the cut, extra forward level, image destinations, tiles on the top block) are
    # executed on the host exactly as the kernels index them: || K x - b || / || b || on random quasi-definite values.
    import eicos_amd
    from eicos_amd import binding as b
    from eicos_amd.generate import dense_front_pattern, random_socp_pattern
    from conftest import ALL_FIXTURES, load_fixture
    hybrid = {}
    for name in ALL_FIXTURES:
        pat, _ = load_fixture(name)
        if pat.n == 0:
            continue
        r, st = b.host_check_tiles(pat)                      # pure tile mode forced on every pattern
        assert 0 <= r < 1e-12, (name, r, eicos_amd.binding._lib().eicos_last_error())
        assert st["blocks"] * 16 >= st["dim_K"] and st["block_levels"] >= 1
        r, st = b.host_check_tiles(pat, hybrid=True)
        assert r == -10.0 or 0 <= r < 1e-12, (name, r)
        hybrid[name] = (r, st)
    # the deep Netlib patterns end in a chain of single-node levels and do qualify; the MPC pattern (log-depth tree) does not
    for name in ("lp_25fv47", "lp_agg", "lp_agg2", "lp_agg3", "lp_bandm", "lp_beaconfd", "lp_bnl1"):
        assert hybrid[name][0] >= 0 and hybrid[name][1]["blocks"] >= 3, (name, hybrid[name])
    assert hybrid["MPC02"][0] == -10.0
    # BASELINE.json config 4 in full (n = 2000, 32 cones x 64): the tile program replaces 5.8 M scalar pairs
    pat, _ = dense_front_pattern(2000, 32, 64)
    r, st = b.host_check_tiles(pat)
    assert 0 <= r < 1e-12 and st["tile_pairs"] < 4000 and st["block_levels"] <= 16 and st["nnzL"] > 16 * st["dim_K"], (r, st)
    for seed in range(3):
        pat, _ = random_socp_pattern(40 + 10 * seed, 8, 12, [20, 3, 17], density=0.4, seed=seed)
        r, st = b.host_check_tiles(pat, seed=seed + 1)
        assert 0 <= r < 1e-12, (seed, r)


def test_host_debug_entries_refuse_malformed_csc():
    # the host-only debug entries take the pattern through the same checks as eicos_batch_create: an out-of-range row index and
    # decreasing column pointers are refused with the entry's error value and a message, not read out of bounds
    import ctypes as C
    from eicos_amd.binding import _lib, _ip
    L = _lib()
    pat, _ = load_fixture("lp_afiro")
    q, Gjc, Gir, Ajc, Air = [np.ascontiguousarray(a, dtype=np.int32) for a in (pat.q, pat.Gjc, pat.Gir, pat.Ajc, pat.Air)]
    qp = _ip(q) if pat.ncones else None
    bad_row = Gir.copy(); bad_row[-1] = pat.m + 1000
    bad_ptr = Gjc.copy(); j = pat.n // 2; bad_ptr[j] = bad_ptr[j + 1] + 1
    for jc, ir, msg in ((Gjc, bad_row, b"G row index out of range"), (bad_ptr, Gir, b"G: column pointers decrease")):
        args = (pat.n, pat.m, pat.p, pat.ncones, qp, _ip(jc), _ip(ir), _ip(Ajc), _ip(Air))
        for fn in (L.eicos_debug_host_check, L.eicos_debug_host_check_tiles, L.eicos_debug_host_check_hybrid):
            assert fn(*args, 1, -1, None) == -2.0 and msg in L.eicos_last_error(), (fn, L.eicos_last_error())
        r = L.eicos_debug_host_tile_order(*args, C.c_int(-1), None, None, None, None, None)
        assert r == -2 and msg in L.eicos_last_error(), (r, L.eicos_last_error())
    assert L.eicos_debug_host_check(pat.n, pat.m, pat.p, pat.ncones, qp, _ip(Gjc), _ip(Gir), _ip(Ajc), _ip(Air), 1, -1, None) >= 0


def test_multi_gpu_layer_refuses_bad_arguments_and_has_no_cpu_fallback():
    # eicos_multi_* (SURVEY.md 8b / 8e): argument checks run before any device is touched; without a GPU creation fails with
    # EICOS_E_NOGPU like the single-GPU entry point (no CPU fallback anywhere)
    import ctypes as C
    import numpy as np
    from eicos_amd.binding import _lib, _ip
    pat, _ = load_fixture("lp_afiro")
    L = _lib()
    q, Gjc, Gir, Ajc, Air = [np.ascontiguousarray(a, dtype=np.int32) for a in (pat.q, pat.Gjc, pat.Gir, pat.Ajc, pat.Air)]
    h = C.c_void_p()
    dev = np.zeros(2, np.int32)
    create = lambda batch, devs, nd: L.eicos_multi_create(pat.n, pat.m, pat.p, pat.l, 0, None, _ip(Gjc), _ip(Gir), _ip(Ajc), _ip(Air), batch, devs, nd, C.byref(h))
    assert create(8, None, 2) == -1 and b"device" in L.eicos_multi_last_error()
    assert create(8, _ip(dev), 0) == -1
    assert create(1, _ip(dev), 2) == -1 and b"batch smaller" in L.eicos_multi_last_error()
    if eicos_amd.device_count() == 0:
        assert create(8, _ip(dev), 2) == -2 and b"no HIP device" in L.eicos_multi_last_error() and not h.value
    assert L.eicos_multi_destroy(None) == 0 and L.eicos_multi_sync(None) == -1 and L.eicos_multi_num_shards(None) == -1


def test_stage_functions_save_no_callee_saved_registers(tmp_path):
    """The non-inlined stage functions of k_solve have internal linkage and are never tail-called, so LLVM's interprocedural register
    allocation gives them no callee-saved registers.  Without that every stage call saves and restores the 64
    callee-saved VGPRs of the AMDGPU calling convention (+256 bytes of private segment per call depth, 128 scratch instructions per thread
    and call, -3.5 % on the headline).  The private segment the code objects declare for k_solve is the cheap witness."""
    import shutil
    import subprocess
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("llvm-objdump / llvm-readelf of the ROCm toolchain not present")
    lib = tmp_path / "lib.so"
    shutil.copy(library_path(), lib)
    subprocess.run([objdump, "--offloading", str(lib)], cwd=tmp_path, check=True, capture_output=True)
    seen = {}
    for co in sorted(tmp_path.glob("lib.so.*gfx950*")):
        notes = subprocess.run([readelf, "--notes", str(co)], check=True, capture_output=True, text=True).stdout
        name = None
        for line in notes.splitlines():
            m = re.search(r"\.name:\s+(\S+)", line)
            if m:
                name = m.group(1)
            m = re.search(r"\.private_segment_fixed_size:\s+(\d+)", line)
            if m and name and "k_solve" in name:
                seen[name] = int(m.group(1))
    assert len(seen) >= 28, seen  # seven builds of kernels.hip (per workgroup size, LDS-resident, two waves per SIMD, U in LDS x 2)
    # measured with the saves: 816 (256-VGPR build of the 256-thread kernel), 528-560 (168-VGPR build), 912 (512 threads), 704 (LDS-resident)
    for name, size in seen.items():
        limit = 600 if ("w2" in name or "ldsres" in name or "ubl" in name or "ILi512E" in name) else 450  # (256-VGPR builds / 512 threads; else the 168-VGPR build)
        assert size <= limit, (name, size)


def test_bench_launch_mode_never_runs_fewer_gpus_than_asked():
    """bench.py --gpus N: under torch.distributed.run it is one process per GPU; WITHOUT a launcher N > 1 takes the
    product's own multi-GPU layer over devices 0..N-1 -- or exits non-zero; it never falls through to a 1-GPU run labelled N."""
    import bench
    lm = bench.launch_mode
    assert lm(1, {}, None, lambda: 0) == ("single", None)
    assert lm(1, {"RANK": "0", "WORLD_SIZE": "1", "MASTER_PORT": "29500"}, None, lambda: 0) == ("single", None)  # torchrun with one rank
    assert lm(8, {"RANK": "3", "LOCAL_RANK": "3", "WORLD_SIZE": "8", "MASTER_PORT": "29500"}, None, lambda: 8) == ("dist", None)
    assert lm(8, {}, None, lambda: 8) == ("multi", list(range(8)))       # the driver's `python bench.py --gpus 8` on an 8-GPU node
    assert lm(2, {}, None, lambda: 8) == ("multi", [0, 1])
    assert lm(1, {}, "0,0,0", lambda: 1) == ("multi", [0, 0, 0])         # a device may be listed several times
    for bad in ((8, {}, None, lambda: 1),                                # 8 asked, one visible: refuse, do not run one GPU as "8"
                (4, {"RANK": "0", "WORLD_SIZE": "8", "MASTER_PORT": "1"}, None, lambda: 8),  # launcher world != --gpus
                (1, {}, "0,1", lambda: 1),                               # --multi names a device that is not there
                (2, {"RANK": "0", "WORLD_SIZE": "2", "MASTER_PORT": "1"}, "0,1", lambda: 2)):  # --multi under a launcher
        with pytest.raises(SystemExit) as e:
            lm(*bad)
        assert e.value.code not in (0, None)
    # without a GPU in this container the real entry point refuses --gpus 2 before importing torch.cuda or touching a device
    if eicos_amd.device_count() == 0:
        import subprocess, sys
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"], capture_output=True, text=True, cwd=ROOT)
        assert out.returncode != 0 and "visible devices" in out.stderr and not out.stdout.strip()


def test_bench_dump_outputs_is_a_fixed_sample_within_the_byte_cap(tmp_path, monkeypatch):
    """bench.py --dump-outputs: float64 files, one row per instance with its global index; beyond the byte cap a seeded sample of the
    instances, the same rows whether the batch is dumped whole or shard by shard."""
    import bench

    class Fake:  # the result surface of BatchSolver / MultiBatchSolver over instances first .. first + B - 1
        def __init__(self, first, B):
            self.g = np.arange(first, first + B, dtype=np.float64)[:, None]
        def solution(self):
            return self.g * np.ones((1, 5))
        def duals(self):
            return self.g * np.ones((1, 2)), -self.g * np.ones((1, 3)), 2 * self.g * np.ones((1, 3))
        def info_arrays(self):
            return {"exitcode": np.zeros(len(self.g), np.int32), "iter": self.g[:, 0].astype(np.int32), "pcost": -self.g[:, 0],
                    "solve_us": np.random.rand(len(self.g)), "reserved_": np.zeros(len(self.g), np.int32)}

    total = 100
    bench.dump_outputs(Fake(0, total), str(tmp_path / "whole"), 0, total)
    whole = {f[:-4]: np.load(tmp_path / "whole" / f) for f in os.listdir(tmp_path / "whole")}
    assert set(whole) == {"instance", "x", "y", "z", "s", "info_exitcode", "info_iter", "info_pcost"}
    assert all(v.dtype == np.float64 and len(v) == total for v in whole.values())
    assert np.array_equal(whole["instance"], np.arange(total)) and np.array_equal(whole["x"][:, 0], np.arange(total))
    row = 8 * (1 + 5 + 2 + 3 + 3 + 3)
    monkeypatch.setattr(bench, "DUMP_BYTES", 30 * row + 1024 * 8)  # (eight files: 1 KB of header room each)
    for tag in ("a", "b"):
        bench.dump_outputs(Fake(0, total), str(tmp_path / tag), 0, total)
    for lo, hi in ((0, 37), (37, 100)):
        bench.dump_outputs(Fake(lo, hi - lo), str(tmp_path / f"shard{lo}"), lo, total)
    a, b = ({f[:-4]: np.load(tmp_path / t / f) for f in os.listdir(tmp_path / t)} for t in ("a", "b"))
    sh = [{f[:-4]: np.load(tmp_path / f"shard{lo}" / f) for f in os.listdir(tmp_path / f"shard{lo}")} for lo in (0, 37)]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= bench.DUMP_BYTES
    assert len(a["instance"]) == 30 and np.all(np.diff(a["instance"]) > 0) and not np.array_equal(a["instance"], np.arange(30))
    for k in a:
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], np.concatenate([s_[k] for s_ in sh])), k
    assert np.array_equal(a["x"][:, 0], a["instance"]) and np.array_equal(a["info_pcost"], -a["instance"])
