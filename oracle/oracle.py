"""ctypes binding of the CPU oracle (oracle/liboracle.so).

TEST INFRASTRUCTURE ONLY: importable from tests/, __graft_entry__.smoke() and the
cpu_baseline leg of bench.py.  The product package eicos_amd never imports this module.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
_LIB_NATIVE = None
_LIB_FMA = None


class OracleInfo(C.Structure):
    _fields_ = [(k, C.c_double) for k in (
        "pcost", "dcost", "pres", "dres", "gap", "relgap", "sigma", "mu", "step", "step_aff",
        "kapovert", "pinfres", "dinfres", "tau", "kap")] + [(k, C.c_int) for k in (
        "has_relgap", "has_pinfres", "has_dinfres", "pinf", "dinf", "iter", "nitref1", "nitref2",
        "nitref3", "exitcode", "n_factor", "n_ldlsolve")]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class OracleSettings(C.Structure):
    """struct oracle_settings: the fields and the order of eicos_amd.binding.Settings."""
    _fields_ = [(k, C.c_double) for k in ("feastol", "abstol", "reltol", "feastol_inacc", "abstol_inacc", "reltol_inacc",
                                          "linsysacc", "irerrfact")] + [("iter_max", C.c_int), ("nitref", C.c_int)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


SETTINGS_FIELDS = tuple(k for k, _ in OracleSettings._fields_)


def build(force: bool = False) -> str:
    so = os.path.join(_HERE, "liboracle.so")
    src = os.path.join(_HERE, "eicos_oracle.cpp")
    if force or not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", _HERE, "-B", "liboracle.so"], stdout=subprocess.DEVNULL)
    return so


def build_native() -> str | None:
    """The same oracle compiled on THIS machine with the reference's Release flags (`-O2 -march=native`, reference
    CMakeLists.txt:22) -- used by bench.py's cpu_baseline leg for the timing only.  Built where it runs (a -march=native
    object must not travel between machines: liboracle_native.so is git- and gpurun-ignored); None if the compiler is missing."""
    so = os.path.join(_HERE, "liboracle_native.so")
    src = os.path.join(_HERE, "eicos_oracle.cpp")
    tag = so + ".host"  # which CPU the object was built for: a copy that travelled here from another machine is rebuilt, never run
    try:
        import hashlib
        cpu = [l for l in open("/proc/cpuinfo") if l.startswith(("model name", "flags"))][:2]
        sig = hashlib.sha256("".join(cpu).encode()).hexdigest()
        have = open(tag).read().strip() if os.path.exists(tag) else ""
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src) or have != sig:
            subprocess.check_call(["make", "-C", _HERE, "-B", "liboracle_native.so"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            open(tag, "w").write(sig)
    except (OSError, subprocess.CalledProcessError):
        return None
    return so


def build_fma() -> str | None:
    """The same oracle with fused multiply-adds contracted (`-mfma -ffp-contract=fast`): a second, equally legitimate rounding of the
    same arithmetic, used by the calibration of tests/test_unrefined_solves.py.  Built where it runs, like liboracle_native.so; None
    when this CPU has no FMA (no `fma` flag in /proc/cpuinfo) or the compiler is missing."""
    so = os.path.join(_HERE, "liboracle_fma.so")
    src = os.path.join(_HERE, "eicos_oracle.cpp")
    try:
        flags = next((l for l in open("/proc/cpuinfo") if l.startswith("flags")), "")
        if "fma" not in flags.split():
            return None
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(os.path.join(_HERE, "eicos_oracle.h"))):
            subprocess.check_call(["make", "-C", _HERE, "-B", "liboracle_fma.so"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    except (OSError, subprocess.CalledProcessError):
        return None
    return so


def _prototype_batch(L):
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.oracle_batch_solve.restype = C.c_double
    L.oracle_batch_solve.argtypes = [C.c_int] * 4 + [ip] * 5 + [C.c_int] + [dp] * 5 + [C.c_int, ip, ip, dp, dp, dp,
                                                                              C.POINTER(C.c_longlong)]
    return L


def lib_native():
    """liboracle_native.so (only oracle_batch_solve is prototyped), or None when it cannot be built here."""
    global _LIB_NATIVE
    if _LIB_NATIVE is None:
        so = build_native()
        _LIB_NATIVE = _prototype_batch(C.CDLL(so)) if so else False
    return _LIB_NATIVE or None


def lib_fma():
    """liboracle_fma.so with every prototype of lib(), or None when it cannot be built here."""
    global _LIB_FMA
    if _LIB_FMA is None:
        so = build_fma()
        _LIB_FMA = _prototype(C.CDLL(so)) if so else False
    return _LIB_FMA or None


def lib():
    global _LIB
    if _LIB is None:
        _LIB = _prototype(C.CDLL(build()))
    return _LIB


def _prototype(L):
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.oracle_create.restype = C.c_void_p
    L.oracle_create.argtypes = [C.c_int] * 5 + [ip, dp, ip, ip, dp, ip, ip, dp, dp, dp]
    L.oracle_update.argtypes = [C.c_void_p, dp, dp, dp, dp, dp]
    L.oracle_solve.argtypes = [C.c_void_p]
    L.oracle_solve.restype = C.c_int
    L.oracle_get_info.argtypes = [C.c_void_p, C.POINTER(OracleInfo)]
    L.oracle_get_x.argtypes = [C.c_void_p, dp]
    L.oracle_get_yzs.argtypes = [C.c_void_p, dp, dp, dp]
    L.oracle_get_dims.argtypes = [C.c_void_p, ip, ip, ip]
    L.oracle_destroy.argtypes = [C.c_void_p]
    L.oracle_set_warm_start.argtypes = [C.c_void_p, C.c_double]
    L.oracle_set_dynamic_regularization.argtypes = [C.c_void_p, C.c_double, C.c_double]
    L.oracle_get_trace.argtypes = [C.c_void_p, dp, C.c_int]
    L.oracle_get_trace.restype = C.c_int
    L.oracle_debug_scalings.argtypes = [C.c_void_p, dp, dp, dp]
    L.oracle_debug_scalings.restype = C.c_int
    L.oracle_debug_kkt.argtypes = [C.c_void_p, ip, ip, dp]
    L.oracle_debug_kkt.restype = C.c_int
    sp = C.POINTER(OracleSettings)
    L.oracle_settings_default.argtypes = [sp]
    L.oracle_settings_default.restype = None
    L.oracle_set_settings.argtypes = [C.c_void_p, sp]
    L.oracle_get_settings.argtypes = [C.c_void_p, sp]
    L.oracle_last_error.restype = C.c_char_p
    L.oracle_debug_perturb_sweep.argtypes = [C.c_void_p, C.c_double]
    L.oracle_debug_perturb_sweep.restype = C.c_int
    return _prototype_batch(L)


def _dp(a):
    return None if a is None or a.size == 0 else a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))


class OracleSolver:
    """Mirror of the reference's raw-pointer Solver API (include/eicos.hpp:151-163)."""

    def __init__(self, pat, vals, fma: bool = False):
        """fma=True: the solver lives in liboracle_fma.so (lib_fma(): the same source, contracted multiply-adds); RuntimeError
        when that build is not available here."""
        self.pat = pat
        self._h = None
        L = lib_fma() if fma else lib()
        if L is None:
            raise RuntimeError("liboracle_fma.so cannot be built on this machine")
        self._L = L
        self._keep = [np.ascontiguousarray(a) for a in (pat.q.astype(np.int32), pat.Gjc, pat.Gir, pat.Ajc, pat.Air)]
        q, Gjc, Gir, Ajc, Air = self._keep
        haveG = pat.m > 0
        haveA = pat.p > 0
        v = self._c(vals)
        self._h = L.oracle_create(
            pat.n, pat.m, pat.p, pat.l, pat.ncones, _ip(q) if pat.ncones else None,
            _dp(v.Gpr) if haveG else None, _ip(Gjc) if haveG else None, _ip(Gir) if haveG else None,
            _dp(v.Apr) if haveA else None, _ip(Ajc) if haveA else None, _ip(Air) if haveA else None,
            _dp(v.c), _dp(v.h), _dp(v.b))

    @staticmethod
    def _c(vals):
        import copy
        v = copy.copy(vals)
        for k in ("Gpr", "Apr", "c", "h", "b"):
            setattr(v, k, np.ascontiguousarray(getattr(vals, k), dtype=np.float64))
        return v

    def update(self, vals):
        v = self._c(vals)
        self._L.oracle_update(self._h, _dp(v.Gpr), _dp(v.Apr), _dp(v.c), _dp(v.h), _dp(v.b))

    def solve(self) -> int:
        return self._L.oracle_solve(self._h)

    def info(self) -> dict:
        o = OracleInfo()
        self._L.oracle_get_info(self._h, C.byref(o))
        return o.asdict()

    def x(self):
        x = np.zeros(max(self.pat.n, 1))
        self._L.oracle_get_x(self._h, _dp(x))
        return x[: self.pat.n]

    def yzs(self):
        y, z, s = np.zeros(max(self.pat.p, 1)), np.zeros(max(self.pat.m, 1)), np.zeros(max(self.pat.m, 1))
        self._L.oracle_get_yzs(self._h, _dp(y), _dp(z), _dp(s))
        return y[: self.pat.p], z[: self.pat.m], s[: self.pat.m]

    def set_warm_start(self, shift: float):
        self._L.oracle_set_warm_start(self._h, float(shift))

    def set_dynamic_regularization(self, delta: float, eps: float):
        self._L.oracle_set_dynamic_regularization(self._h, float(delta), float(eps))

    def set_settings(self, **fields):
        """The ten runtime settings with the names, ranges and refusals of eicos_amd.BatchSolver.set_settings: fields that are not
        named keep their value, an unknown name raises TypeError before the library is called, a refused value RuntimeError with the
        solver's settings unchanged."""
        unknown = sorted(set(fields) - set(SETTINGS_FIELDS))
        if unknown:
            raise TypeError(f"set_settings: unknown field(s) {', '.join(unknown)} (the settings are {', '.join(SETTINGS_FIELDS)})")
        st = OracleSettings()
        self._L.oracle_get_settings(self._h, C.byref(st))
        for k, v in fields.items():
            setattr(st, k, int(v) if k in ("iter_max", "nitref") else float(v))
        if self._L.oracle_set_settings(self._h, C.byref(st)) != 0:
            raise RuntimeError(self._L.oracle_last_error().decode())

    def settings(self) -> dict:
        st = OracleSettings()
        self._L.oracle_get_settings(self._h, C.byref(st))
        return st.asdict()

    def perturb_sweep(self, rel: float) -> int:
        """Test hook oracle_debug_perturb_sweep: every LDL solve from now on scales the last stored entry of every column j % 7 == 3
        of L by 1 + rel in the backward substitution (rel = 0: off).  Returns the number of entries concerned."""
        return self._L.oracle_debug_perturb_sweep(self._h, float(rel))

    def trace(self):
        out = np.zeros((102, 12))
        n = self._L.oracle_get_trace(self._h, _dp(out), 102)
        return out[:n]

    def dims(self):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        self._L.oracle_get_dims(self._h, C.byref(a), C.byref(b), C.byref(c))
        return dict(dimK=a.value, nnzK=b.value, nnzL=c.value)

    def debug_scalings(self, s, z):
        """updateScalings + updateKKTScalings for (s, z): (ok, scaling block of K in cacheIndices order)."""
        pat = self.pat
        nV = pat.l + int(sum(3 * int(d) + 1 for d in pat.q))
        s, z = np.ascontiguousarray(s, np.float64), np.ascontiguousarray(z, np.float64)
        V = np.zeros(max(nV, 1))
        ok = self._L.oracle_debug_scalings(self._h, _dp(s), _dp(z), _dp(V))
        return bool(ok), V[:nV]

    def debug_kkt(self):
        """Upper triangle of the KKT matrix as it stands (CSC: ptr, idx, val), reference column layout."""
        d = self.dims()
        Kp, Ki, Kx = np.zeros(d["dimK"] + 1, np.int32), np.zeros(max(d["nnzK"], 1), np.int32), np.zeros(max(d["nnzK"], 1))
        nnz = self._L.oracle_debug_kkt(self._h, _ip(Kp), _ip(Ki), _dp(Kx))
        return Kp, Ki[:nnz], Kx[:nnz]

    def close(self):
        if self._h:
            self._L.oracle_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def default_settings() -> dict:
    st = OracleSettings()
    lib().oracle_settings_default(C.byref(st))
    return st.asdict()


def batch_solve(pat, Gpr, Apr, c, h, b, nthreads: int, want_x: bool = False, native: bool = False):
    """CPU baseline: arrays [B][...]; returns dict with wall seconds of the solve phase.
    native=True: run the `-O2 -march=native` build of the same source (build_native) when it is available."""
    L = (lib_native() if native else None) or lib()
    B = c.shape[0] if pat.n else h.shape[0]
    Gpr, Apr, c, h, b = (np.ascontiguousarray(a, dtype=np.float64) for a in (Gpr, Apr, c, h, b))
    q = np.ascontiguousarray(pat.q.astype(np.int32))
    ex = np.zeros(B, np.int32)
    it = np.zeros(B, np.int32)
    pc = np.zeros(B)
    xo = np.zeros((B, pat.n)) if want_x else None
    upd = C.c_double()
    ns = C.c_longlong()
    dpn = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    wall = L.oracle_batch_solve(pat.n, pat.m, pat.p, pat.ncones, _ip(q), _ip(pat.Gjc), _ip(pat.Gir), _ip(pat.Ajc),
                                _ip(pat.Air), B, dpn(Gpr), dpn(Apr), dpn(c), dpn(h), dpn(b), nthreads, _ip(ex), _ip(it),
                                dpn(pc), dpn(xo) if want_x else None, C.byref(upd), C.byref(ns))
    return dict(seconds=wall, update_seconds=upd.value, exitcodes=ex, iters=it, pcost=pc, x=xo,
                ldlsolves=int(ns.value), native=bool(native and L is not lib()))
